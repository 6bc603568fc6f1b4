"""What training on clouds of unequal size promises that a machine without a GPU can check: the four new symbols (exported, declared,
within ABI 18, listed in INTEGRATION.md), the wrappers' and the step's signatures, and the seeded cases of tests/test_ragged_bwd_gpu.py
against their float64 references (the ReLU margins hold, the indices keep to their cloud)."""
import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import fp_bwd_ref                                  # noqa: E402
import fp_train_ref                                # noqa: E402
import ragged_bwd_cases as C                       # noqa: E402
import sa_bwd_ref                                  # noqa: E402
import sa_train_ref                                # noqa: E402

SYMBOLS = ("ampnet_fp_backward_ragged_f32", "ampnet_fp_train_backward_ragged_f32", "ampnet_sa_backward_ragged_f32",
           "ampnet_sa_train_backward_ragged_f32")


def test_the_library_exports_the_four_symbols_within_abi_18_and_the_header_declares_them():
    L = sub("_lib")
    lib = L.lib()
    assert lib.ampnet_abi_version() == 18 == L.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    assert int(re.search(r"#define AMPNET_ABI_VERSION (\d+)", text).group(1)) == 18
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        decl = re.search(r"\bint " + s + r"\(([^;]*)\);", text)
        assert decl, s
        assert re.search(r"const int32_t \*cloud_off, int n_clouds,\s+int total", decl.group(1)), s      # in place of (n_clouds, n)
        assert s in integration, s
    for f in ("fp_backward_f32", "fp_train_backward_f32", "sa_backward_f32", "sa_train_backward_f32"):
        assert inspect.signature(getattr(L, f)).parameters["cloud_off"].default is None, f


def test_the_step_and_the_autograd_entry_points_carry_the_table():
    S, A = sub("pointNet.pn2_step"), sub("autograd")
    p = inspect.signature(S.train_loop_clouds).parameters
    assert list(p) == ["clouds", "optimizer", "class_w", "model", "train", "device_outputs"]
    assert (p["train"].default, p["device_outputs"].default) == (True, True)
    assert "BatchNorm statistics" in S.train_loop_clouds.__doc__ and "NOT the loss" in S.train_loop_clouds.__doc__
    for f in ("fp_apply", "fp_train_apply", "sa_apply", "sa_train_apply"):
        assert inspect.signature(getattr(A, f)).parameters["cloud_off"].default is None, f
    assert list(inspect.signature(S.train_loop).parameters) == ["data", "optimizer", "class_w", "model", "train", "device_outputs"]


def test_the_seeded_cases_keep_their_margins_and_their_clouds():
    synth = sub("synthetic")
    for train, R in ((False, fp_bwd_ref), (True, fp_train_ref)):
        i = C.fp_inputs(synth, train)
        ref = R.fp_train if train else R.fp_backward
        _, worst = ref(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
        assert worst > R.RELU_MARGIN
        cloud = np.repeat(np.arange(C.Q), C.SIZES)[:, None]
        assert (i["idx"][0] // C.FP_S == cloud).all() and (i["idx"][0] - cloud * C.FP_S == i["local_idx"]).all()
    for train, R in ((False, sa_bwd_ref), (True, sa_train_ref)):
        j = C.sa_inputs(synth, train)
        _, worst = R.forward_tape(j["xyz"], j["centres"], j["group_idx"], j["feats"], j["layers"], j["eps"])
        assert worst > sa_bwd_ref.RELU_MARGIN
        g = j["group_idx"].reshape(C.Q, C.SA_S, C.SA_NSAMPLE)
        assert all(((g[b] >= C.OFF[b]) & (g[b] < C.OFF[b + 1])).all() for b in range(C.Q))
    assert len(C.fp_inputs(synth, True, C.DEEP_WIDTHS)["layers"]) == 3 and len(C.sa_inputs(synth, True, C.DEEP_WIDTHS)["layers"]) == 3
