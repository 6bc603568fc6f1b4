"""What the ragged input pipeline promises that a machine without a GPU can check: the new symbol (exported, declared, within ABI 18), the
keyed point shuffle restated in numpy from the header's text (a bijection, different per cloud and per step, every position reachable),
the signatures of the step, the driver and the CLI, the CloudBatch round trip and the cluster dataset."""
import importlib.util
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import PKG, sub                      # noqa: E402
import cloud_input_ref as R                        # noqa: E402

SIZES = (1, 2, 3, 5, 8, 64, 90, 128, 1000, 1024, 1025, 4097, 12288)


def test_the_library_exports_the_symbol_within_abi_18_and_the_header_declares_it():
    L = sub("_lib")
    lib = L.lib()
    assert lib.ampnet_abi_version() == 18 == L.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    assert int(re.search(r"#define AMPNET_ABI_VERSION (\d+)", text).group(1)) == 18
    assert hasattr(lib, "ampnet_cloud_input_f32")
    assert re.search(r"\bint ampnet_cloud_input_f32\(", text)
    assert callable(L.cloud_input_f32)
    assert "ampnet_cloud_input_f32" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("n", SIZES)
def test_the_restated_shuffle_is_a_bijection(n):
    for seed, step, cloud in ((0x6A09E667, 0, 0), (7, 3, 17), (0xFFFFFFFF, 0xFFFFFFFF, 287)):
        p, rounds = R.perm(seed, step, cloud, n, return_rounds=True)
        assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), (n, seed, step, cloud)
        assert rounds <= 64, rounds                  # the domain holds at most 4 n values: a walk of tens of rounds is the tail


def test_clouds_and_steps_shuffle_differently():
    n = 1024
    a = R.perm(7, 0, 0, n)
    assert not np.array_equal(a, np.arange(n))
    assert not np.array_equal(a, R.perm(7, 0, 1, n)) and not np.array_equal(a, R.perm(7, 1, 0, n)) and not np.array_equal(a, R.perm(8, 0, 0, n))
    assert np.array_equal(a, R.perm(7, 0, 0, n))                         # a function of its keys
    angles = [R.step_angle(7, s) for s in range(64)]
    assert all(0.0 <= t < 2 * np.pi for t in angles) and len(set(angles)) == 64
    S = sub("pointNet.pn2_step")
    assert [S.step_angle(7, s) for s in range(64)] == angles and S.step_angle(0xFFFFFFFF, 0xFFFFFFFF) == R.step_angle(0xFFFFFFFF, 0xFFFFFFFF)


def test_every_position_reaches_every_source_at_n_8():
    hits = np.zeros((8, 8), dtype=np.int64)
    for step in range(4096):
        hits[np.arange(8), R.perm(0x6A09E667, step, 0, 8)] += 1
    print("n = 8, 4096 steps: (position, source) cells min", hits.min(), "max", hits.max(), "(uniform: 512)")
    assert hits.min() >= 1 and hits.sum() == 8 * 4096


def test_the_label_table_and_the_padding_rule():
    codes = np.array([3, 4, 5, 14, 15, 0, 2, 255, 300.0, -1.0, 15.9, 256.0], dtype=np.float32)
    assert R.labels(codes).tolist() == [3, 3, 4, 2, 1, 0, 0, 0, 0, 0, 1, 0]
    raw = np.arange(7 * 10, dtype=np.float32).reshape(7, 10)
    raw[:, 9] = [15, 14, 3, 5, 4, 0, 15]
    rows, tg, src, padded = R.cloud_input(raw, [2, 5], 4, 1, 1, permute=False, rotate=False)
    assert padded == [4, 5] and src.tolist() == [0, 1, 0, 1, 2, 3, 4, 5, 6] and tg.tolist() == [1, 2, -1, -1, 3, 4, 3, 0, 1]
    assert np.array_equal(rows, raw[src, :9])
    U = sub("utils.utils")
    p, _, gather, keep = U.pad_cloud_sizes([2, 5], 4)
    assert p == padded and np.array_equal(gather, src) and np.array_equal(np.flatnonzero(tg != -1), keep)


def test_signatures_of_the_step_and_the_driver():
    S, T = sub("pointNet.pn2_step"), sub("pointNet.pn2_train")
    sig = inspect.signature(S.cloud_input)
    assert list(sig.parameters) == ["raw", "sizes", "npoint", "train", "seed", "step", "want_src"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("train", "seed", "step", "want_src"))
    assert sig.parameters["want_src"].default is False
    assert list(inspect.signature(S.train_loop_clouds).parameters) == ["clouds", "optimizer", "class_w", "model", "train", "device_outputs"]
    sig = inspect.signature(S.train_loop_clouds_aug)              # train_loop_clouds' list is pinned: the keyword lives on its twin
    assert list(sig.parameters) == ["clouds", "optimizer", "class_w", "model", "train", "device_outputs", "augment"]
    assert sig.parameters["augment"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["augment"].default is None
    sig = inspect.signature(T.train_pn2_clouds)
    assert list(sig.parameters) == ["cluster_dir", "path_list_files", "output_folder", "files_per_step", "epochs", "learning_rate",
                                    "number_of_workers", "model_checkpoint", "device", "allow_pickle", "seed"]
    assert (sig.parameters["number_of_workers"].default, sig.parameters["seed"].default) == (4, 0x6A09E667)
    assert "precision" not in sig.parameters
    a = S.CloudAugment()
    assert (a.seed, a._step) == (0x6A09E667, 0) and a.state_dict() == {"seed": 0x6A09E667, "step": 0}
    b = S.CloudAugment(7)
    b._step = 5
    a.load_state_dict(b.state_dict())
    assert (a.seed, a._step) == (7, 5) and all(type(v) is int for v in a.state_dict().values())


def test_the_cli_has_the_flags_of_its_family_and_no_precision():
    path = os.path.join(ROOT, PKG, "pointNet", "pointnet2", "train_pointnet2_clouds.py")
    spec = importlib.util.spec_from_file_location("train_pointnet2_clouds", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    flags = {s for a in parser._actions for s in a.option_strings}
    for f in ("--cluster_dir", "--path_list_files", "--files_per_step", "--epochs", "--learning_rate", "--number_of_workers",
              "--model_checkpoint", "--seed"):
        assert f in flags, f
    assert "--precision" not in flags
    a = parser.parse_args(["--cluster_dir", "c", "--files_per_step", "3", "--seed", "0x10"])
    assert (a.cluster_dir, a.files_per_step, a.seed) == ("c", 3, 16)
    assert parser.parse_args([]).seed == 0x6A09E667


def test_cloud_batch_round_trips_through_collate_clouds(synth):
    C = sub("pointNet.collate_fns")
    f0, _ = synth.test_file_clusters(3, 3, n_points=40, spread=9)
    f1, _ = synth.test_file_clusters(4, 2, n_points=40, spread=9)
    f1 = [torch.cat([c, torch.zeros(c.shape[0], 2)], dim=1).double() for c in f1]       # wider, another dtype: ten columns are kept, as float32
    cb = C.collate_clouds([f0, f1])
    assert isinstance(cb, C.CloudBatch) and len(cb) == 2 and cb.names == ["", ""]
    assert cb.sizes == [c.shape[0] for c in f0 + f1] and cb.raw.shape == (sum(cb.sizes), 10) and cb.raw.dtype == torch.float32
    assert not cb.is_cuda and cb.raw.is_contiguous()
    for got, want in zip(cb.raw.split(cb.sizes), f0 + f1):
        assert torch.equal(got, want[:, :10].float())
    moved = cb.to("cpu")
    assert isinstance(moved, C.CloudBatch) and torch.equal(moved.raw, cb.raw) and moved.sizes == cb.sizes and moved.names == cb.names
    cb.record_stream(None)                          # a host batch has nothing to record
    for m in ("pin_memory", "to", "record_stream"):
        assert callable(getattr(C.CloudBatch, m)) and callable(getattr(C.RaggedBatch, m))
    with pytest.raises(ValueError):
        C.collate_clouds([[torch.zeros(4, 9)]])
    with pytest.raises(ValueError):
        C.collate_clouds([[]])


def test_cluster_dataset_reads_what_write_cluster_dataset_wrote_and_refuses_an_oversized_cluster(synth, tmp_path):
    D, C, L = sub("pointNet.datasets"), sub("pointNet.collate_fns"), sub("_lib")
    paths = synth.write_cluster_dataset(str(tmp_path), n_train=2, n_val=1, n_test=1, seed=40, n_points=64, spread=20)
    lists = {s: open(os.path.join(paths["lists"], f"{s}_seg_files.txt")).read().split() for s in ("train", "val", "test")}
    assert [len(v) for v in lists.values()] == [2, 1, 1] and len({n for v in lists.values() for n in v}) == 4
    ds = D.LidarClusterDataset(paths["clusters"], lists["train"])
    assert len(ds) == 2
    sizes = [[int(c.shape[0]) for c in ds[i]] for i in range(2)]
    assert sizes[0][1] == 33 and all(64 <= n < 84 for n in sizes[0][:1] + sizes[0][2:] + sizes[1])          # small=True: one cut cluster
    assert all(c.shape[1] == 10 and c.dtype == torch.float32 for i in range(2) for c in ds[i]) and ds[0].name == lists["train"][0]
    want = torch.load(os.path.join(paths["clusters"], lists["train"][1].split(".")[0] + "_clusters_list.pkl"), weights_only=True)
    assert all(torch.equal(a, b) for a, b in zip(ds[1], want))
    cb = C.collate_clouds([ds[0], ds[1]])
    assert cb.names == lists["train"] and cb.sizes == sizes[0] + sizes[1]
    same = synth.write_cluster_dataset(str(tmp_path / "again"), n_train=2, n_val=1, n_test=1, seed=40, n_points=64, spread=20, small=False)
    full = D.LidarClusterDataset(same["clusters"], lists["train"])[0]
    assert full[1].shape[0] >= 64 and torch.equal(full[1][:33], ds[0][1]) and torch.equal(full[0], ds[0][0])
    # the test split is what pn2_infer.test reads
    assert os.path.exists(os.path.join(paths["clusters"], lists["test"][0].split(".")[0] + "_clusters_list.pkl"))
    big = os.path.join(paths["clusters"], "huge_clusters_list.pkl")
    torch.save([torch.zeros(5, 10), torch.zeros(D.CLUSTER_MAX_POINTS + 1, 10)], big)
    with pytest.raises(L.AmpnetError, match=r"huge_clusters_list\.pkl: cluster 1 holds 12289 points"):
        D.LidarClusterDataset(paths["clusters"], ["some/dir/huge.pkl"])[0]
