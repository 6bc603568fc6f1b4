"""The group_all set-abstraction backward (include/ampnet_hip.h: ampnet_sa_all_backward_f32) against the float64 restatement
tests/sa_all_ref.py, which is given the forward kernel's own arg_out (first checked to be admissible).  The bars are
sa_bwd_ref.sa_backward's; the worst error / bar ratio of every output of every case is printed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import sa_all_ref as R                             # noqa: E402
import sa_bwd_ref                                  # noqa: E402
from sa_all_run import GUARD, case as _case, run_forward, to_gpu as _t   # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in R.CASES]


def _run(L, i, arg, prefill=float("nan"), dout=None, ws_short=0, dfeats="auto", layers=None, feats="auto"):
    """-> {name: numpy array}.  Every output lives in front of 64 guard elements, which the kernels must leave alone; the workspace
    starts as NaN bit patterns."""
    f = i["feats"] if isinstance(feats, str) else feats
    layers = i["layers"] if layers is None else layers
    B, n = i["xyz"].shape[:2]
    bufs = {}

    def out(name, shape):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), prefill, dtype=torch.float32, device="cuda")
        buf[numel:] = GUARD
        bufs[name] = buf
        return buf[:numel].view(*shape)

    res = {}
    if isinstance(dfeats, str):
        dfeats = None if f is None else out("dfeats", f.shape)
    if dfeats is not None:
        res["dfeats"] = dfeats
    grads = []
    for l, layer in enumerate(layers):
        grads.append(tuple(out(f"{k}{l}", layer[j].shape) for k, j in (("dW", 0), ("dbias", 1), ("dgamma", 1), ("dbeta", 1))))
        res.update({f"{k}{l}": g for k, g in zip(("dW", "dbias", "dgamma", "dbeta"), grads[-1])})
    try:
        need = L.sa_all_backward_workspace_bytes(0 if f is None else f.shape[2], B, n, [layer[0].shape[0] for layer in layers])
    except L.AmpnetError:
        need = 1 << 20                                             # a refused shape: sa_all_backward_f32 has to say so itself
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device="cuda").view(torch.uint8)[:need - ws_short]
    L.sa_all_backward_f32(_t(i["xyz"]), _t(f), [tuple(_t(a) for a in layer) for layer in layers], [R.BN_EPS] * len(layers), _t(arg),
                          _t(i["dout"] if dout is None else dout), dfeats, grads, ws)
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert (buf[-64:] == GUARD).all(), f"{name}: written past its end"
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", NAMES)
def test_sa_all_backward_within_the_derived_bar(name):
    L = sub("_lib")
    i, tape = _case(name)
    n = i["xyz"].shape[1]
    _, arg = run_forward(L, i)
    R.check_argmax(arg, tape, i["xyz"], i["feats"])
    got = _run(L, i, arg)                                          # every output starts as NaN: every element must be written
    names = sa_bwd_ref.output_names(len(i["layers"]), i["feats"] is not None)
    assert sorted(got) == sorted(names)
    for k, v in got.items():
        assert np.isfinite(v).all(), (name, k)
    again = _run(L, i, arg, prefill=-7.0)
    for k in got:
        assert np.array_equal(got[k], again[k]), (name, k)         # bitwise the same on a second run
    with L.precision_scope("bf16"):
        scoped = _run(L, i, arg)
    for k in got:
        assert np.array_equal(got[k], scoped[k]), (name, k)        # exact fp32 whatever the precision scope
    if i["feats"] is not None:
        no_df = _run(L, i, arg, dfeats=None)                       # dfeats = NULL at D > 0: nothing else changes
        for k in set(names) - {"dfeats"}:
            assert np.array_equal(got[k], no_df[k]), (name, k)
    want = R.backward(i["xyz"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
    ratios = {}
    for k in names:
        v, bar = want[k]
        assert got[k].shape == v.shape, (name, k)
        ratios[k] = float((np.abs(got[k].astype(np.float64) - v) / np.maximum(bar, 1e-300)).max())
    print(f"sa_all_backward {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    if i["feats"] is not None:
        for b in range(R.N_CLOUDS):
            losers = np.setdiff1d(np.arange(n), arg[b])
            assert (got["dfeats"][b, losers] == 0).all(), (name, b)            # exactly zero outside the winners, and written
        assert (got["dfeats"] != 0).any()
    if name == "dead_channel":
        last = len(i["layers"]) - 1
        assert all((got[f"{k}{last}"][R.DEAD] == 0).all() for k in ("dW", "dbias", "dgamma", "dbeta"))
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


def test_sa_all_backward_refusals():
    """Every misuse is an AmpnetError that says what is wrong."""
    L = sub("_lib")
    i, _ = _case("n32")                                            # n 32, D 6, [32, 64]
    arg = np.zeros((2, 64), np.int32)
    with pytest.raises(L.AmpnetError, match="workspace"):
        _run(L, i, arg, ws_short=1)
    with pytest.raises(L.AmpnetError, match="dout"):
        _run(L, i, arg, dout=i["dout"][:, :32])
    with pytest.raises(L.AmpnetError, match="dout"):
        _run(L, i, arg, dout=i["dout"][:, None, :])
    with pytest.raises(L.AmpnetError, match="arg"):
        _run(L, i, arg[:, :32])
    with pytest.raises(L.AmpnetError, match="arg"):
        _run(L, i, arg.astype(np.int64))
    with pytest.raises(L.AmpnetError, match="layer 0"):
        _run(L, i, arg, feats=i["feats"][:, :, :5])                # weight [32, 9] against cin_0 = 3 + 5
    with pytest.raises(L.AmpnetError, match="dfeats"):
        _run(L, i, arg, dfeats=torch.zeros((2, 32, 4), device="cuda"))
    j, _ = _case("n33")                                            # D = 0
    with pytest.raises(L.AmpnetError, match="dfeats"):
        _run(L, j, np.zeros((2, 32), np.int32), dfeats=torch.zeros((2, 33, 4), device="cuda"))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, dict(i, dout=i["dout"][:, :48]), arg[:, :48], layers=R.sa_ref.make_layers(1, 9, [48]))
    with pytest.raises(L.AmpnetError, match="layers"):
        _run(L, dict(i, dout=i["dout"][:, :32]), arg[:, :32], layers=R.sa_ref.make_layers(1, 9, [32, 32, 32, 32]))
    for missing in ("xyz", "arg", "dout"):
        args = dict(xyz=_t(i["xyz"]), arg=_t(arg), dout=_t(i["dout"]))
        args[missing] = None
        with pytest.raises(L.AmpnetError, match=missing):
            L.sa_all_backward_f32(args["xyz"], _t(i["feats"]), [tuple(_t(a) for a in layer) for layer in i["layers"]], [R.BN_EPS] * 2,
                                  args["arg"], args["dout"], None, [], torch.empty(16, dtype=torch.uint8, device="cuda"))


def test_sa_all_backward_takes_out_of_range_arg_without_reading_out_of_bounds():
    """arg is an input: values outside [0, N) are clamped, as every index the kernels take is."""
    L = sub("_lib")
    i, _ = _case("n32")
    arg = np.full((2, 64), 1 << 30, np.int32)
    arg[:, ::2] = -5
    got = _run(L, i, arg)
    want = _run(L, i, np.clip(arg, 0, 31))
    for k in got:
        assert np.array_equal(got[k], want[k]), k
