"""The window token on the GPU, as a layer: ampnet_token_pool_forward_f32 / _backward_f32 (csrc/token_pool.hip) against the float64
restatement of tests/token_pool_ref.py within bars from tests/pw_probe.py::bar, and the exact properties of the contract: every element
written, the same bits on every run and under a precision scope, a row's value independent of its place (the packed rows run as clouds of
ONE row give y32, whose numpy max and first argmax per cloud are out and arg_out exactly), the lowest row on ties, dx exactly zero outside
the winners, optional outputs that change nothing else, and refusals that name what is wrong.  The cases are the smallest shapes at which
the kernel can still go wrong (token_pool_ref.CASES)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import token_pool_ref as R                         # noqa: E402
from pw_probe import err_ratio                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    return sub("_lib"), sub("utils.utils"), sub("pointNet.model.pointnet2_utils")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _forward(rows, sizes, W, bias, want_arg=True, fill=(float("nan"), -1)):
    """The C entry point through _lib on packed GPU rows -> (out, arg or None) as numpy."""
    L, U, _ = _mods()
    lay = U.ragged_layout("test", rows, sizes)
    Q, cout = len(lay.sizes), W.shape[0]
    out = torch.full((Q, cout), fill[0], dtype=torch.float32, device=DEV)
    arg = torch.full((Q, cout), fill[1], dtype=torch.int32, device=DEV) if want_arg else None
    ws = torch.empty(L.token_pool_forward_workspace_bytes(rows.shape[1], cout, Q, rows.shape[0]), dtype=torch.uint8, device=DEV)
    L.token_pool_forward_f32(rows, lay.off, W, bias, out, ws, arg_out=arg)
    return out.cpu().numpy(), None if arg is None else arg.cpu().numpy()


def _backward(rows, sizes, W, arg, dout, want=("dx", "dW", "db"), fill=float("nan")):
    L, U, _ = _mods()
    lay = U.ragged_layout("test", rows, sizes)
    Q, (cout, cin) = len(lay.sizes), W.shape
    outs = {"dx": torch.full((rows.shape[0], cin), fill, dtype=torch.float32, device=DEV) if "dx" in want else None,
            "dW": torch.full((cout, cin), fill, dtype=torch.float32, device=DEV) if "dW" in want else None,
            "db": torch.full((cout,), fill, dtype=torch.float32, device=DEV) if "db" in want else None}
    ws = torch.empty(L.token_pool_backward_workspace_bytes(cin, cout, Q, rows.shape[0]), dtype=torch.uint8, device=DEV)
    L.token_pool_backward_f32(rows, lay.off, W, _gpu(arg.astype(np.int32)), _gpu(dout), outs["dx"], outs["dW"], outs["db"], ws)
    return {k: v.cpu().numpy() for k, v in outs.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's inputs, their GPU copies, the float64 reference and the first GPU run: computed once, shared, never changed."""
    synth = sub("synthetic")
    c = R.case_inputs(synth, name)
    c["g"] = {k: _gpu(c[k]) for k in ("rows", "W", "bias")}
    c["ref"] = R.forward(c["rows"], c["sizes"], c["W"], c["bias"])
    c["out"], c["arg"] = _forward(c["g"]["rows"], c["sizes"], c["g"]["W"], c["g"]["bias"])
    return c


@pytest.mark.parametrize("name", R.NAMES)
def test_forward(name):
    L, _, U2 = _mods()
    c = _case(name)
    g, sizes = c["g"], c["sizes"]
    out, arg = c["out"], c["arg"]
    off = R.offsets(sizes)
    # every element written over the NaN / -1 pre-fill
    assert np.isfinite(out).all() and (arg >= 0).all()
    # another pre-fill, a bf16 precision scope, no arg_out: the same bits
    out2, arg2 = _forward(g["rows"], sizes, g["W"], g["bias"], fill=(7.0, 12345))
    assert np.array_equal(out, out2) and np.array_equal(arg, arg2)
    with L.precision_scope("bf16"):
        out3, arg3 = _forward(g["rows"], sizes, g["W"], g["bias"])
    assert np.array_equal(out, out3) and np.array_equal(arg, arg3)
    out4, _ = _forward(g["rows"], sizes, g["W"], g["bias"], want_arg=False)
    assert np.array_equal(out, out4)
    # the float64 restatement
    out64, _, bar_out = c["ref"]
    worst = err_ratio(out, out64, bar_out)
    print(f"token_pool forward {name}: worst error / bar = {worst:.4f}")
    assert worst <= 1.0
    R.check_arg(arg, c["rows"], sizes, c["W"], c["bias"])
    # position independence, bit for bit: the same packed rows as `total` clouds of one row
    y32, a1 = _forward(g["rows"], [1] * int(off[-1]), g["W"], g["bias"])
    assert (a1 == 0).all()
    for q in range(len(sizes)):
        blk = y32[off[q]:off[q + 1]]
        assert np.array_equal(blk.max(0), out[q]), f"cloud {q}"
        assert np.array_equal(blk.argmax(0).astype(np.int32), arg[q]), f"cloud {q}"      # (numpy's argmax: the first, the lowest row)
    # the public call: packed with sizes is the entry point's bits, and uniform [Q, n, cin] input equals the packed call
    t, a = U2.token_pool(g["rows"], g["W"], g["bias"], sizes=sizes, want_arg=True)
    assert np.array_equal(t.cpu().numpy(), out) and np.array_equal(a.cpu().numpy(), arg)
    n_u = sizes[0] if len(set(sizes)) == 1 else min(33, int(off[-1]))
    q_u = int(off[-1]) // n_u
    sub_rows = g["rows"][:q_u * n_u].contiguous()
    tu, au = U2.token_pool(sub_rows.view(q_u, n_u, -1), g["W"].unsqueeze(2), g["bias"], want_arg=True)
    tp, ap = U2.token_pool(sub_rows, g["W"], g["bias"], sizes=[n_u] * q_u, want_arg=True)
    assert torch.equal(tu, tp) and torch.equal(au, ap)
    if name == "duplicates":
        assert (arg < 35).all()
    if name == "negative":
        assert (out < 0).all()
    if name in ("many_tiles", "long_runs"):
        planted = R.planted_rows(name, sizes)
        assert [int(arg[0, i]) for i in range(len(planted))] == planted
        assert set(arg[0].tolist()) <= set(planted) | {0}


@pytest.mark.parametrize("name", R.NAMES)
def test_backward(name):
    c = _case(name)
    g, sizes = c["g"], c["sizes"]
    cout = c["W"].shape[0]
    for which, arg in enumerate([c["arg"]] + R.hand_args(sizes, cout)):
        ref = R.backward(c["rows"], sizes, c["W"], arg, c["dout"])
        got = _backward(g["rows"], sizes, g["W"], arg, c["dout"])
        for k in ("dx", "dW", "db"):
            worst = err_ratio(got[k], *ref[k])
            print(f"token_pool backward {name} arg {which} {k}: worst error / bar = {worst:.4f}")
            assert worst <= 1.0, k
        assert (got["dx"][~R.winner_rows(arg, sizes)] == 0).all()
        again = _backward(g["rows"], sizes, g["W"], arg, c["dout"], fill=3.0)
        for k in got:
            assert np.array_equal(got[k], again[k]), k
        for k in got:                                  # the other two outputs NULL: this one is unchanged
            alone = _backward(g["rows"], sizes, g["W"], arg, c["dout"], want=(k,))
            assert list(alone) == [k] and np.array_equal(alone[k], got[k]), k


def test_refusals_name_what_is_wrong():
    L, U, U2 = _mods()
    rows = torch.zeros((10, 32), device=DEV)
    W, bias = torch.zeros((32, 32), device=DEV), torch.zeros(32, device=DEV)
    off = U.ragged_layout("test", rows, [4, 6]).off
    out = torch.empty((2, 32), device=DEV)
    arg = torch.empty((2, 32), dtype=torch.int32, device=DEV)
    need = L.token_pool_forward_workspace_bytes(32, 32, 2, 10)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.token_pool_forward_f32(rows, off, W, bias, out, ws, arg_out=arg)                     # the accepted call
    with pytest.raises(L.AmpnetError, match=r"ampnet_token_pool_forward_f32: workspace of \d+ bytes, \d+ are needed"):
        L.token_pool_forward_f32(rows, off, W, bias, out, ws[:need - 256], arg_out=arg)
    with pytest.raises(L.AmpnetError, match=r"token_pool_forward: out must be \[Q, cout\] = \[2, 32\]"):
        L.token_pool_forward_f32(rows, off, W, bias, torch.empty((3, 32), device=DEV), ws, arg_out=arg)
    with pytest.raises(L.AmpnetError, match=r"token_pool_forward: arg_out must be \[Q, cout\] = \[2, 32\]"):
        L.token_pool_forward_f32(rows, off, W, bias, out, ws, arg_out=arg[:, :16].contiguous())
    with pytest.raises(L.AmpnetError, match="arg_out must be a contiguous 2-d torch.int32 GPU tensor"):
        L.token_pool_forward_f32(rows, off, W, bias, out, ws, arg_out=arg.long())
    with pytest.raises(L.AmpnetError, match="cin=48"):
        U2.token_pool(torch.zeros((10, 48), device=DEV), torch.zeros((32, 48), device=DEV), bias, sizes=[4, 6])
    with pytest.raises(L.AmpnetError, match="cout=288"):
        U2.token_pool(rows, torch.zeros((288, 32), device=DEV), torch.zeros(288, device=DEV), sizes=[4, 6])
    rows48, off48 = torch.zeros((10, 48), device=DEV), off
    with pytest.raises(L.AmpnetError, match=r"ampnet_token_pool_forward_f32: cin=48"):
        L.token_pool_forward_f32(rows48, off48, torch.zeros((32, 48), device=DEV), bias, out, ws, arg_out=arg)
    with pytest.raises(L.AmpnetError, match=r"ampnet_token_pool_backward_f32: cout=288"):
        L.token_pool_backward_f32(rows, off, torch.zeros((288, 32), device=DEV), torch.zeros((2, 288), dtype=torch.int32, device=DEV),
                                  torch.zeros((2, 288), device=DEV), None, None, torch.empty(288, device=DEV), ws)
    with pytest.raises(L.AmpnetError, match=r"token_pool: sizes \(sum 9\) do not tile the 10 rows"):
        U2.token_pool(rows, W, bias, sizes=[4, 5])
    with pytest.raises(L.AmpnetError, match=r"token_pool: sizes \(sum 10\) do not tile the 10 rows"):
        U2.token_pool(rows, W, bias, sizes=[10, 0])                                        # a zero size
    with pytest.raises(L.AmpnetError, match="rows must live on the GPU"):
        U2.token_pool(rows.cpu(), W, bias, sizes=[4, 6])
    with pytest.raises(L.AmpnetError, match="rows must be a contiguous 2-d torch.float32 GPU tensor"):
        L.token_pool_forward_f32(rows.cpu(), off, W, bias, out, ws, arg_out=arg)
    with pytest.raises(L.AmpnetError, match=r"token_pool_backward: dx must be \[10, 32\]"):
        L.token_pool_backward_f32(rows, off, W, arg, out, torch.empty((9, 32), device=DEV), None, None, ws)


def test_autograd_follows_torchs_graph_rules_and_routes_the_three_gradients():
    _, _, U2 = _mods()
    c = _case("borders")
    g, sizes = c["g"], c["sizes"]
    assert not U2.token_pool(g["rows"], g["W"], g["bias"], sizes=sizes).requires_grad
    x, w, b = (g[k].clone().requires_grad_(True) for k in ("rows", "W", "bias"))
    with torch.no_grad():
        assert not U2.token_pool(x, w, b, sizes=sizes).requires_grad
    t, a = U2.token_pool(x, w.unsqueeze(2), b, sizes=sizes, want_arg=True)
    assert t.requires_grad and not a.requires_grad
    assert np.array_equal(t.detach().cpu().numpy(), c["out"]) and np.array_equal(a.cpu().numpy(), c["arg"])
    (t * _gpu(c["dout"])).sum().backward()
    want = _backward(g["rows"], sizes, g["W"], c["arg"], c["dout"])
    assert np.array_equal(x.grad.cpu().numpy(), want["dx"]) and np.array_equal(w.grad.cpu().numpy(), want["dW"])
    assert np.array_equal(b.grad.cpu().numpy(), want["db"])
    w2 = g["W"].clone().requires_grad_(True)                     # only the weight asks: the rows get no dense gradient
    U2.token_pool(g["rows"], w2, g["bias"], sizes=sizes).sum().backward()
    assert w2.grad is not None and g["rows"].grad is None
