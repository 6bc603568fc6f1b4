"""The window token without a GPU: the float64 restatement of tests/token_pool_ref.py against torch's own F.linear(...).amax and its
autograd in float64 (uniform and ragged sizes, negative-only outputs, tie-free random inputs), the conditions the seeded GPU cases have to
meet, and the host side of the feature -- the C symbols within ABI 18, the header, the bindings and the Python surface."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import token_pool_ref as R                         # noqa: E402

SYMBOLS = ("ampnet_token_pool_forward_f32", "ampnet_token_pool_backward_f32", "ampnet_token_pool_forward_workspace_bytes",
           "ampnet_token_pool_backward_workspace_bytes")


def _torch_side(rows, sizes, W, bias, dout):
    x = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    w = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    off = R.offsets(sizes)
    out = torch.stack([F.linear(x[off[q]:off[q + 1]], w, b).amax(0) for q in range(len(sizes))])
    (out * torch.tensor(dout, dtype=torch.float64)).sum().backward()
    return out.detach().numpy(), x.grad.numpy(), w.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("sizes,cin,cout,bias_shift", [([7, 7, 7], 32, 32, 0.0), ([1, 31, 32, 33, 5], 32, 64, 0.0), ([40, 3], 64, 32, -50.0)])
def test_the_restatement_is_torchs_linear_amax_and_its_autograd(synth, sizes, cin, cout, bias_shift):
    total = sum(sizes)
    rows = synth.uniform(71, (total, cin), -1.0, 1.0)
    W = synth.uniform(72, (cout, cin), -1.0, 1.0)
    bias = synth.uniform(73, (cout,), -0.5, 0.5) + np.float32(bias_shift)
    dout = synth.uniform(74, (len(sizes), cout), -1.0, 1.0)
    out, arg, bar_out = R.forward(rows, sizes, W, bias)
    t_out, t_dx, t_dW, t_db = _torch_side(rows, sizes, W, bias, dout)
    y, _ = R.row_values(rows, W, bias)
    off = R.offsets(sizes)
    for q in range(len(sizes)):                    # tie-free: torch's even split and the lowest-row rule are then the same gradient
        blk = np.sort(y[off[q]:off[q + 1]], 0)
        assert len(blk) == 1 or (blk[-1] > blk[-2]).all()
    assert np.array_equal(out, t_out)
    if bias_shift:
        assert (out < 0).all()
    assert (bar_out > 0).all() and (bar_out < 1e-4 * (1 + abs(bias_shift))).all()
    R.check_arg(arg, rows, sizes, W, bias)
    got = R.backward(rows, sizes, W, arg, dout)
    for name, want in (("dx", t_dx), ("dW", t_dW), ("db", t_db)):
        v, b = got[name]
        assert v.shape == want.shape and (b >= 0).all()
        assert np.allclose(v, want, rtol=1e-13, atol=1e-13), name
    assert (got["dx"][0][~R.winner_rows(arg, sizes)] == 0).all() and (got["dx"][1][~R.winner_rows(arg, sizes)] == 0).all()


def test_duplicate_rows_give_torchs_parameter_gradients(synth):
    """The tie rule: torch splits a tie's gradient evenly, the restatement gives it to the lowest row; on exact duplicates dW and db agree."""
    c = R.case_inputs(synth, "duplicates")
    out, arg, _ = R.forward(c["rows"], c["sizes"], c["W"], c["bias"])
    assert (arg < 35).all()
    t_out, t_dx, t_dW, t_db = _torch_side(c["rows"], c["sizes"], c["W"], c["bias"], c["dout"])
    got = R.backward(c["rows"], c["sizes"], c["W"], arg, c["dout"])
    assert np.array_equal(out, t_out)
    assert np.allclose(got["dW"][0], t_dW, rtol=1e-13, atol=1e-13) and np.allclose(got["db"][0], t_db, rtol=1e-13, atol=1e-13)
    assert np.allclose(got["dx"][0][:35], t_dx[:35] + t_dx[35:], rtol=1e-13, atol=1e-13) and (got["dx"][0][35:] == 0).all()


@pytest.mark.parametrize("name", ["many_tiles", "long_runs"])
def test_the_planted_cases_have_their_winners_where_they_were_planted(synth, name):
    c = R.case_inputs(synth, name)
    _, arg, _ = R.forward(c["rows"], c["sizes"], c["W"], c["bias"])
    planted = R.planted_rows(name, c["sizes"])
    assert len(set(planted)) == len(planted) and all(0 < p < c["sizes"][0] for p in planted)
    for i, p in enumerate(planted):
        assert arg[0, i] == p, (i, p, arg[0, i])
    assert set(arg[0].tolist()) <= set(planted) | {0}


def test_the_negative_case_is_negative_everywhere(synth):
    c = R.case_inputs(synth, "negative")
    out, _, _ = R.forward(c["rows"], c["sizes"], c["W"], c["bias"])
    assert (out < -40).all()


def test_the_library_exports_the_symbols_within_abi_18_and_the_header_declares_them():
    L = sub("_lib")
    lib = L.lib()
    assert lib.ampnet_abi_version() == 18 == L.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    assert int(re.search(r"#define AMPNET_ABI_VERSION (\d+)", text).group(1)) == 18
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(r"\b(int|size_t) " + s + r"\(", text), s
    assert "ampnet_token_pool_forward_f32" in integration and "ampnet_token_pool_backward_f32" in integration
    for f in ("token_pool_forward_f32", "token_pool_backward_f32", "token_pool_forward_workspace_bytes", "token_pool_backward_workspace_bytes"):
        assert callable(getattr(L, f)), f


def test_workspace_sizes_answer_on_the_host_and_refuse_by_name():
    L = sub("_lib")
    assert L.token_pool_forward_workspace_bytes(128, 128, 576, 576 * 2048) > 0
    assert L.token_pool_backward_workspace_bytes(128, 128, 576, 576 * 2048) > 0
    for fn in (L.token_pool_forward_workspace_bytes, L.token_pool_backward_workspace_bytes):
        with pytest.raises(L.AmpnetError, match=r"ampnet_token_pool_\w+_workspace_bytes: cin=48"):
            fn(48, 128, 1, 10)
        with pytest.raises(L.AmpnetError, match=r"ampnet_token_pool_\w+_workspace_bytes: cout=288"):
            fn(128, 288, 1, 10)
        with pytest.raises(L.AmpnetError, match="Q=3 clouds, total=2 rows"):
            fn(32, 32, 3, 2)


def test_the_python_surface_exists():
    U2 = sub("pointNet.model.pointnet2_utils")
    M = sub("pointNet.model.pointnetAtt")
    A = sub("autograd")
    assert list(inspect.signature(U2.token_pool).parameters) == ["rows", "weight", "bias", "sizes", "want_arg"]
    assert issubclass(A._TokenPoolFn, torch.autograd.Function)
    for name in ("forward_tokens", "forward_tokens_ragged", "_backbone_ragged"):
        assert callable(getattr(M.pointnet_2, name)), name
    assert M.pointnet_2_seg.forward_tokens is not M.pointnet_2.forward_tokens
    for text in (U2.token_pool.__doc__, M.pointnet_2.forward_tokens.__doc__):
        assert "LOWEST" in text and "amax" in text and "fp32" in text


def test_token_pool_refuses_cpu_tensors_by_name():
    L = sub("_lib")
    U2 = sub("pointNet.model.pointnet2_utils")
    with pytest.raises(L.AmpnetError, match="rows must live on the GPU"):
        U2.token_pool(torch.zeros(2, 4, 32), torch.zeros(32, 32), torch.zeros(32))
