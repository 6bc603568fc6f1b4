"""The yardstick of the loss kernel behind the segmentation head, checked without a GPU: tests/seg_loss_ref.py against torch's float64
F.nll_loss (value and autograd), and the host side of the feature -- the C symbols within ABI 18, the modules and CLI files of the
pointnet_2_seg drivers importing and parsing their arguments on a CPU-only machine, the `return_perm` keyword of the two augment functions."""
import importlib.util
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import PKG, sub                      # noqa: E402
import seg_loss_ref as R                           # noqa: E402


def _torch_nll(logp, target, w):
    """torch float64 nll_loss(weight, ignore_index=-1, 'mean') and its gradient; a target outside [0, C) is mapped to -1 first (torch
    refuses other out-of-range values; the kernel ignores them all)."""
    C = logp.shape[1]
    lp = torch.from_numpy(logp.astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.where((target >= 0) & (target < C), target, -1))
    loss = F.nll_loss(lp, t, None if w is None else torch.from_numpy(w.astype(np.float64)), ignore_index=-1, reduction="mean")
    (loss * float(R.GRAD)).backward()
    return float(loss.detach()), lp.grad.numpy()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", R.CLASSES)
@pytest.mark.parametrize("M", [1, 65, 4099])
def test_reference_equals_torch_float64(M, C, weighted):
    logp, target, w, ref = R.case(M, C, weighted)
    want, dwant = _torch_nll(logp, target, w)
    assert abs(ref["loss"] - want) <= 1e-12 * abs(want)
    d = R.nll_backward(target, w, ref["sums"][1], R.GRAD, C)
    assert float(np.abs(d - dwant).max()) <= 1e-12 * float(np.abs(dwant).max())
    assert (d[~ref["live"]] == 0).all() and (dwant[~ref["live"]] == 0).all()
    # the predictions are the lowest arg-max and the counts are the confusion matrix of the live rows plus the ignored rows
    assert (logp[np.arange(M), ref["preds"]] == logp.max(1)).all()
    for m in np.flatnonzero((logp == logp.max(1, keepdims=True)).sum(1) > 1):
        assert ref["preds"][m] == np.flatnonzero(logp[m] == logp[m].max())[0]
    live = ref["live"]
    cm = np.zeros((C, C), dtype=np.int64)
    for t, p in zip(target[live], ref["preds"][live]):
        cm[t, p] += 1
    assert np.array_equal(ref["counts"][:C * C].reshape(C, C), cm) and ref["counts"][C * C] == (~live).sum() and ref["counts"].sum() == M


def test_cases_hold_what_the_gpu_test_relies_on():
    logp, target, w, ref = R.case(4099, 5, True)
    C = 5
    assert 0.15 < float((target == -1).mean()) < 0.25 and (target == C + 3).sum() == 1 and not (target == C - 1).any()
    ties = (logp == logp.max(1, keepdims=True)).sum(1) > 1
    assert 0.03 < float(ties.mean()) < 0.07
    highest = C - 1 - logp[ties][:, ::-1].argmax(1)
    assert (ref["preds"][ties] < highest).all()                      # the lowest and the highest arg-max differ: the rule matters
    assert w is not None and w.dtype == np.float32 and (w >= 0.5).all() and (w <= 2.0).all()
    assert R.case(1, 2, False)[3]["live"].all()


def test_all_rows_ignored_is_nan_with_a_zero_gradient_as_in_torch():
    logp, _, w, _ = R.case(65, 5, True)
    target = np.full(65, -1, dtype=np.int64)
    ref = R.nll(logp, target, w)
    want, dwant = _torch_nll(logp, target, w)
    assert math.isnan(ref["loss"]) and math.isnan(want)
    assert (R.nll_backward(target, w, ref["sums"][1], R.GRAD, 5) == 0).all() and (dwant == 0).all()
    assert ref["counts"][25] == 65 and ref["counts"][:25].sum() == 0


def test_symbols_exist_within_abi_18():
    L = sub("_lib")
    lib = L.lib()
    assert lib.ampnet_abi_version() == L.ABI_VERSION == 18      # new symbols, nothing else moved
    for s in ("ampnet_seg_nll_forward_f32", "ampnet_seg_nll_forward_workspace_bytes", "ampnet_seg_nll_backward_f32"):
        assert hasattr(lib, s), s
    for f in ("seg_nll_forward_f32", "seg_nll_forward_workspace_bytes", "seg_nll_backward_f32"):
        assert callable(getattr(L, f)), f
    # the size function answers on the host: one double[2] row per workgroup of 256 rows, at most 1024 of them; 0 = refused
    assert L.seg_nll_forward_workspace_bytes(1) == 16 and L.seg_nll_forward_workspace_bytes(257) == 32
    assert L.seg_nll_forward_workspace_bytes(256 * 1024 + 3) == 1024 * 16
    with pytest.raises(L.AmpnetError, match="rows must be in"):
        L.seg_nll_forward_workspace_bytes(0)


def _load_cli(name):
    path = os.path.join(ROOT, PKG, "pointNet", "pointnet2", name + ".py")
    spec = importlib.util.spec_from_file_location("cli_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_drivers_import_and_the_cli_files_parse_on_a_cpu_machine():
    T, S, U, A = sub("pointNet.pn2_train"), sub("pointNet.pn2_step"), sub("pointNet.model.pointnet2_utils"), sub("pointNet.model.pointnetAtt")
    assert list(inspect.signature(T.train_pn2).parameters) == ["dataset_folder", "path_list_files", "output_folder", "n_points", "batch_size",
                                                               "epochs", "learning_rate", "number_of_workers", "model_checkpoint", "device"]
    assert list(inspect.signature(T.test).parameters) == ["dataset_folder", "output_folder", "n_points", "number_of_workers", "model_checkpoint",
                                                          "path_list_files", "device", "allow_pickle"]
    assert list(inspect.signature(T.segment_file).parameters) == ["model", "clusters_list", "device"]
    assert list(inspect.signature(S.train_loop).parameters) == ["data", "optimizer", "class_w", "model", "train", "device_outputs"]
    assert list(inspect.signature(U.seg_nll_loss).parameters) == ["log_probs", "target", "weight", "want_preds", "want_counts"]
    assert callable(A.pointnet_2_seg.forward_rows) and callable(A.pointnet_2_seg.predict_rows)
    assert "precision" not in inspect.signature(T.train_pn2).parameters and "precision" not in inspect.signature(T.test).parameters
    with pytest.raises(sub("_lib").AmpnetError, match="must live on the GPU"):
        U.seg_nll_loss(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
    a = _load_cli("train_pointnet2_segmen").build_parser().parse_args(["--dataset_path", "d", "--path_list_files", "l", "--batch_size", "4",
                                                                      "--epochs", "2", "--learning_rate", "0.001"])
    assert (a.dataset_path, a.path_list_files, a.batch_size, a.epochs, a.learning_rate, a.number_of_points) == ("d", "l", 4, 2, 0.001, 2048)
    assert not hasattr(a, "precision")
    b = _load_cli("test_pointnet2_segmen").build_parser().parse_args(["--model_checkpoint", "ck.pth", "--out_path", "o"])
    assert (b.model_checkpoint, b.out_path, b.number_of_points) == ("ck.pth", "o", 2048) and not hasattr(b, "precision")
    # the window selection of the step, on the host: window (b, w) is real iff cperm[w] < w_b
    idx = S.real_window_index(np.array([2, 0, 1]), [1, 3])
    assert idx.dtype == torch.int64 and idx.tolist() == [1, 3, 4, 5]
    pad = torch.full((2, 8, 3), -1, dtype=torch.int64)
    pad[0, :, :1], pad[1, :, :3] = 0, 1
    assert S.window_counts(None, pad) == [1, 3]


def test_return_perm_is_a_keyword_of_both_augment_functions_and_defaults_to_false():
    S = sub("pointNet.amp_step")
    for fn in (S.augment_batch_device, S.augment_ragged_device):
        p = inspect.signature(fn).parameters["return_perm"]
        assert p.default is False
