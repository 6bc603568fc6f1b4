"""The host side of data-parallel pointnet_2_seg without a GPU: the pinned argument lists, pn2_step.global_loss under a two-rank gloo group
on CPU tensors (the pattern of tests/test_dp_cpu.py), the flat gradient buffer, the shards of the drivers, and the documents."""
import inspect
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402

# per rank: (its weighted-mean loss S_r / W_r, W_r); rank 2 of the three-rank case has no live row (NaN loss, W = 0)
LOSSES = {2: [(0.75, 12.0), (1.5, 20.0)], 3: [(0.75, 12.0), (1.5, 20.0), (float("nan"), 0.0)]}


def test_the_pinned_argument_lists_are_unchanged():
    S, T = sub("pointNet.pn2_step"), sub("pointNet.pn2_train")
    names = lambda f: list(inspect.signature(f).parameters)         # noqa: E731
    assert names(S.train_loop) == ["data", "optimizer", "class_w", "model", "train", "device_outputs"]
    assert names(S.train_loop_clouds) == ["clouds", "optimizer", "class_w", "model", "train", "device_outputs"]
    assert names(S.train_loop_clouds_aug) == ["clouds", "optimizer", "class_w", "model", "train", "device_outputs", "augment"]
    assert inspect.signature(S.train_loop_clouds_aug).parameters["augment"].kind is inspect.Parameter.KEYWORD_ONLY
    assert names(T.train_pn2) == ["dataset_folder", "path_list_files", "output_folder", "n_points", "batch_size", "epochs", "learning_rate",
                                  "number_of_workers", "model_checkpoint", "device"]
    assert names(T.train_pn2_clouds) == ["cluster_dir", "path_list_files", "output_folder", "files_per_step", "epochs", "learning_rate",
                                         "number_of_workers", "model_checkpoint", "device", "allow_pickle", "seed"]


def _loss_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        S = sub("pointNet.pn2_step")
        loss, w = LOSSES[world][rank]
        total, seed = S.global_loss(torch.tensor(loss, dtype=torch.float32), torch.tensor(w, dtype=torch.float64))
        torch.save((total, seed), os.path.join(out_dir, f"loss{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_global_loss_is_the_weighted_mean_of_the_global_batch(tmp_path, world):
    mp.spawn(_loss_worker, args=(world, 33000 + world + os.getpid() % 2000, str(tmp_path)), nprocs=world, join=True)
    S_sum = sum(l * w for l, w in LOSSES[world] if w > 0)
    W_sum = sum(w for _, w in LOSSES[world])
    seeds = []
    for rank, (_, w) in enumerate(LOSSES[world]):
        total, seed = torch.load(tmp_path / f"loss{rank}.pt", weights_only=True)
        assert total.dtype == seed.dtype == torch.float32 and total.dim() == 0
        assert float(total) == pytest.approx(S_sum / W_sum, rel=1e-6)              # sum S / sum W, the same on every rank
        assert float(seed) == pytest.approx(world * w / W_sum, rel=1e-6)           # world * W_r / sum W
        seeds.append(float(seed))
    assert sum(seeds) == pytest.approx(world, rel=1e-6)             # after the 1 / world average the ranks' weights add up to 1


def test_loss_weight_sum_counts_the_live_rows():
    S = sub("pointNet.pn2_step")
    target = torch.tensor([0, 1, -1, 4, 2, 7, 1])
    class_w = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0])
    assert float(S.loss_weight_sum(target, class_w, 5)) == 1.0 + 2.0 + 1.0 + 2.0 + 2.0
    assert float(S.loss_weight_sum(target, None, 5)) == 5.0
    assert S.loss_weight_sum(target, class_w, 5).dtype == torch.float64


def test_flat_grads_views_survive_a_backward():
    """The views alias ONE buffer, 256-byte aligned; autograd adds into them in place, and zero_attach() puts back what
    optimizer.zero_grad() (set to None) would have dropped."""
    S = sub("pointNet.pn2_step")
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    net[0].bias.requires_grad_(False)
    st = S.FlatGrads(net)
    assert len(st.params) == 3 and st.matches(net)
    st.zero_attach()
    for p, v in zip(st.params, st.views):
        assert p.grad.data_ptr() == v.data_ptr() and (v.data_ptr() - st.flat.data_ptr()) % 256 == 0
    net(torch.ones(2, 5)).sum().backward()
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(st.params, st.views)) and float(st.flat.abs().sum()) > 0
    want = st.flat.clone()
    torch.optim.SGD(net.parameters(), lr=0.1).zero_grad()
    assert net[1].weight.grad is None
    st.zero_attach()
    assert float(st.flat.abs().sum()) == 0
    net(torch.ones(2, 5)).sum().backward()
    assert torch.equal(st.flat, want)
    net[0].bias.requires_grad_(True)
    assert not st.matches(net)


def test_driver_shards_are_equal_and_disjoint():
    T = sub("pointNet.pn2_train")
    files = [f"tile{i}.pt" for i in range(7)]
    assert T._shard(files, 0, 1) is files
    shards = [T._shard(files, r, 3) for r in range(3)]
    assert [len(s) for s in shards] == [2, 2, 2]                    # equal step counts: the seventh file is dropped
    flat = [f for s in shards for f in s]
    assert len(set(flat)) == 6 and set(flat) <= set(files)


def test_the_documents_say_how_it_is_launched():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()           # noqa: E731
    header = read("include", "ampnet_hip.h")
    at = header.index("global-batch BatchNorm under data parallelism")
    block = header[at:at + 6000]
    for name in ("ampnet_fp_train_forward_f32", "ampnet_fp_train_backward_f32", "ampnet_sa_train_forward_f32", "ampnet_sa_train_backward_f32",
                 "ampnet_seg_head_train_forward_f32", "ampnet_seg_head_train_backward_f32", "ragged", "world_size"):
        assert name in block, name
    assert "#define AMPNET_ABI_VERSION 18" in header
    integration = read("INTEGRATION.md")
    assert "pointnet_2_seg" in integration and "AMPNET_SYNC_BN=1" in integration and "train_pn2_clouds" in integration
    for doc in (read("README.md"), read("DESIGN.md"), read(sub("").__path__[0], "pointNet", "pn2_train.py"),
                read(sub("").__path__[0], "pointNet", "pn2_step.py")):
        assert "data parallelism is not built" not in doc and "Not built: data parallelism" not in doc
        assert "data-parallel training of\npointnet_2_seg is not built" not in doc
    assert "torch.distributed.run" in read("README.md") and "prof_pn2_dp.py" in read("DESIGN.md")
