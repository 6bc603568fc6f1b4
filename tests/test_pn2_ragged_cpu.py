"""What the ragged PointNet++ inference path promises that a machine without a GPU can check: the two new symbols (exported, declared, within
ABI 18), the driver's signatures, the CLI's flags, the host-side packing behind pointnet_2_seg.predict_clouds and the GPU-only refusal."""
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
from conftest import PKG, sub                      # noqa: E402

SYMBOLS = ("ampnet_ball_query_ragged_f32", "ampnet_three_nn_ragged_f32")


def test_the_library_exports_the_two_symbols_within_abi_18_and_the_header_declares_them():
    L = sub("_lib")
    lib = L.lib()
    assert lib.ampnet_abi_version() == 18 == L.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    assert int(re.search(r"#define AMPNET_ABI_VERSION (\d+)", text).group(1)) == 18
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(r"\bint " + s + r"\(", text), s
    for f in ("ball_query_ragged_f32", "three_nn_ragged_f32"):
        assert callable(getattr(L, f)), f
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in integration, s


def test_the_driver_imports_without_a_gpu_and_has_the_signatures_of_its_family():
    I, A = sub("pointNet.pn2_infer"), sub("pointNet.model.pointnetAtt")
    assert list(inspect.signature(I.test).parameters) == ["dataset_path", "out_path", "n_points", "number_of_workers", "model_checkpoint",
                                                          "path_list_files", "cluster_dir", "device", "allow_pickle", "files_per_launch"]
    p = inspect.signature(I.test).parameters
    assert (p["cluster_dir"].default, p["device"].default, p["allow_pickle"].default, p["files_per_launch"].default) == \
        ("k_means_25", "cuda", None, 1)
    assert list(inspect.signature(I.segment_file).parameters) == ["model", "clusters_list", "device", "device_outputs"]
    assert list(inspect.signature(I.segment_files).parameters) == ["model", "files", "device", "device_outputs"]
    assert inspect.signature(I.segment_file).parameters["device_outputs"].default is False
    assert inspect.signature(I.segment_files).parameters["device_outputs"].default is False
    assert "precision" not in p
    for m in ("forward_ragged", "predict_ragged", "predict_clouds"):
        assert callable(getattr(A.pointnet_2_seg, m)), m
    assert list(inspect.signature(A.pointnet_2_seg.forward_ragged).parameters) == ["self", "rows", "sizes"]
    # what the existing tests pin stays: pn2_train is not touched
    T = sub("pointNet.pn2_train")
    assert list(inspect.signature(T.segment_file).parameters) == ["model", "clusters_list", "device"]


def test_the_cli_carries_the_test_clis_flags_plus_cluster_dir_and_files_per_launch():
    def load(name):
        spec = importlib.util.spec_from_file_location("cli_" + name, os.path.join(ROOT, PKG, "pointNet", "pointnet2", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    a = load("infer_pointnet2_segmen").build_parser().parse_args(["--cluster_dir", "c", "--files_per_launch", "4"])
    assert (a.cluster_dir, a.files_per_launch) == ("c", 4) and not hasattr(a, "precision")
    d = vars(load("infer_pointnet2_segmen").build_parser().parse_args([]))
    assert (d.pop("cluster_dir"), d.pop("files_per_launch")) == ("k_means_25", 1)
    assert d == vars(load("test_pointnet2_segmen").build_parser().parse_args([]))


def test_the_packing_behind_predict_clouds():
    U = sub("utils.utils")
    padded, off, gather, keep = U.pad_cloud_sizes([90, 128, 300], 128)
    assert padded == [128, 128, 300]
    assert off.dtype == np.int64 and off.tolist() == [0, 128, 256, 556]
    want = np.concatenate([np.arange(128) % 90, 90 + np.arange(128), 218 + np.arange(300)])
    assert gather.dtype == np.int64 and np.array_equal(gather, want)
    assert keep.dtype == np.int64 and np.array_equal(keep, np.concatenate([np.arange(90), np.arange(128, 256), np.arange(256, 556)]))
    # the padded rows that are kept are the clouds' own rows, in order: the padding's predictions are what is dropped
    assert np.array_equal(gather[keep], np.arange(90 + 128 + 300))
    # nothing to pad: the identity
    padded, off, gather, keep = U.pad_cloud_sizes([128, 129], 128)
    assert padded == [128, 129] and np.array_equal(gather, np.arange(257)) and np.array_equal(keep, np.arange(257))
    with pytest.raises(ValueError):
        U.pad_cloud_sizes([0, 5], 4)


def test_the_ragged_searches_have_no_cpu_path():
    U, L = sub("utils.utils"), sub("_lib")
    rows, centres = torch.zeros(10, 3), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(L.AmpnetError, match="must live on the GPU"):
        U.ball_query_ragged(rows, [4, 6], centres, 0.1, 4)
    with pytest.raises(L.AmpnetError, match="must live on the GPU"):
        U.three_nn_ragged(rows, [4, 6], torch.zeros(2, 3, 3))
    assert list(inspect.signature(U.ball_query_ragged).parameters)[:7] == ["rows", "sizes", "centres", "radius", "nsample", "return_counts",
                                                                          "global_index"]
    assert list(inspect.signature(U.three_nn_ragged).parameters) == ["fine_rows", "sizes", "coarse_xyz", "global_index"]
    assert issubclass(U.CentreRangeError, L.AmpnetError) and issubclass(U.CentreRangeError, IndexError)
