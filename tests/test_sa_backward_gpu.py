"""The fused set-abstraction backward (include/ampnet_hip.h: ampnet_sa_backward_f32) against the float64 restatement tests/sa_bwd_ref.py.
The kernel's own argmax (arg_out) is first checked to be admissible (sa_bwd_ref.check_argmax), then every output is compared with the
restatement evaluated AT that argmax.  The bars are derived in sa_bwd_ref.sa_backward's docstring; the worst error / bar ratio of every
output of every case is printed."""
import ctypes
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
import sa_bwd_ref as R                             # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234.5
NAMES = [c[0] for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, forward tape) of a case, computed once and shared (nobody writes to them)."""
    i = R.case_inputs(sub("synthetic"), name)
    tape, _ = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    return i, tape


def _forward(L, i, per_row):
    """ampnet_sa_forward_f32 on the case -> out [B, s, cout_last]; per_row: every row as a group of its own (centre repeated, nsample = 1)
    -> the forward's own float32 relu(y) of every row, [B, s, nsample, cout_last]."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, s, nsample = i["group_idx"].shape
    cen, gi = i["centres"], i["group_idx"]
    if per_row:
        cen, gi = np.repeat(cen, nsample, 1), gi.reshape(B, s * nsample, 1)
    out = torch.full((B, cen.shape[1], i["layers"][-1][0].shape[0]), float("nan"), device="cuda")
    L.sa_forward_f32(t(i["xyz"]), t(cen), t(gi), t(i["feats"]), [tuple(t(a) for a in layer) for layer in i["layers"]],
                     [R.BN_EPS] * len(i["layers"]), out, torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda"))
    out = out.cpu().numpy()
    return out.reshape(B, s, nsample, -1) if per_row else out


def _run(L, i, prefill=float("nan"), dout=None, ws_short=0, dfeats="auto", want_arg=True, layers=None, feats="auto", group_idx=None):
    """-> {name: numpy array}, "arg" among them.  Every output lives in front of 64 guard elements, which the kernels must leave alone."""
    dev = "cuda"
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = i["feats"] if isinstance(feats, str) else feats
    layers = i["layers"] if layers is None else layers
    gi = i["group_idx"] if group_idx is None else group_idx
    B, s, nsample = gi.shape
    bufs = {}

    def out(name, shape, dtype=torch.float32, fill=prefill, guard=GUARD):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), fill, dtype=dtype, device=dev)
        buf[numel:] = guard
        bufs[name] = (buf, guard)
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
    couts = [layer[0].shape[0] for layer in layers]
    arg = out("arg", (B, s, couts[-1]), torch.int32, -1, -77) if want_arg else None
    if arg is not None:
        res["arg"] = arg
    try:
        need = L.sa_backward_workspace_bytes(0 if f is None else f.shape[2], B, s, nsample, couts)
    except L.AmpnetError:
        need = 1 << 20                                             # a refused shape: sa_backward_f32 has to say so itself
    ws = torch.full((need - ws_short,), 0xAB, dtype=torch.uint8, device=dev)
    L.sa_backward_f32(t(i["xyz"]), t(i["centres"]), t(gi), t(f), [tuple(t(a) for a in layer) for layer in layers],
                      [R.BN_EPS] * len(layers), t(i["dout"] if dout is None else dout), dfeats, grads, ws, arg_out=arg)
    torch.cuda.synchronize()
    for name, (buf, guard) in bufs.items():
        assert (buf[-64:] == guard).all(), f"{name}: written past its end"
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", NAMES)
def test_sa_backward_within_the_derived_bar(name):
    L = sub("_lib")
    i, tape = _case(name)
    got = _run(L, i)                                               # every output starts as NaN / -1: every element must be written
    names = R.output_names(len(i["layers"]), i["feats"] is not None)
    assert sorted(got) == sorted(names + ["arg"])
    for k, v in got.items():
        assert np.isfinite(v).all(), (name, k)
    again = _run(L, i, prefill=-7.0)
    for k in got:
        assert np.array_equal(got[k], again[k]), (name, k)         # bitwise the same on a second run
    with L.precision_scope("bf16"):
        scoped = _run(L, i)
    for k in got:
        assert np.array_equal(got[k], scoped[k]), (name, k)        # exact fp32 whatever the precision scope
    no_arg = _run(L, i, want_arg=False)
    for k in names:
        assert np.array_equal(got[k], no_arg[k]), (name, k)        # arg_out = NULL changes nothing else
    if i["feats"] is not None:
        no_df = _run(L, i, dfeats=None)                            # dfeats = NULL at D > 0: layer 0's dx and the gather are skipped
        for k in set(names) - {"dfeats"}:
            assert np.array_equal(got[k], no_df[k]), (name, k)
        assert np.array_equal(got["arg"], no_df["arg"])
    # the backward's recompute is the forward's, bit for bit: the forward run on every row as a group of its own gives the float32 relu(y)
    # per row; its max is the forward's output and its lowest maximal row is arg_out, exactly
    rows32 = _forward(L, i, per_row=True)
    assert np.array_equal(rows32.max(2), _forward(L, i, per_row=False)), name
    assert np.array_equal(rows32.argmax(2), got["arg"]), name
    R.check_argmax(got["arg"], tape, i["group_idx"])
    want = R.sa_backward(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], got["arg"], tape)
    ratios = {}
    for k in names:
        v, bar = want[k]
        assert got[k].shape == v.shape, (name, k)
        ratios[k] = float((np.abs(got[k].astype(np.float64) - v) / np.maximum(bar, 1e-300)).max())
    print(f"sa_backward {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    if i["feats"] is not None:
        for c, u in enumerate(i["unpicked"]):
            assert (got["dfeats"][c, u] == 0).all(), (name, c, u)  # in no group: exact zeros, and written
        assert not np.array_equal(got["dfeats"][0], got["dfeats"][1])
        assert (got["dfeats"] != 0).any()
    if name == "unpicked":
        assert all(len(u) >= 2 for u in i["unpicked"])
    if name == "sparse_ball":
        assert (i["count"] == 1).any()                             # some ball holds its centre alone
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


def test_sa_backward_refusals():
    """Every misuse is an AmpnetError that says what is wrong; shapes outside the forward's limits, and those whose tiles do not fit the
    LDS, are refused the same way."""
    L = sub("_lib")
    i, _ = _case("tail_group")                                     # n 70, s 9, nsample 20, D 6, [32, 64]
    with pytest.raises(L.AmpnetError, match="dout"):
        _run(L, i, dout=i["dout"][:, :, :32])
    with pytest.raises(L.AmpnetError, match="dout"):
        _run(L, i, dout=i["dout"][:, :8])
    with pytest.raises(L.AmpnetError, match="workspace"):
        _run(L, i, ws_short=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for missing in ("xyz", "centres", "group_idx", "dout"):
        args = dict(xyz=t(i["xyz"]), centres=t(i["centres"]), group_idx=t(i["group_idx"]), dout=t(i["dout"]))
        args[missing] = None
        with pytest.raises(L.AmpnetError, match=missing):
            L.sa_backward_f32(args["xyz"], args["centres"], args["group_idx"], t(i["feats"]), [tuple(t(a) for a in layer) for layer in i["layers"]],
                              [R.BN_EPS] * 2, args["dout"], None, [], torch.empty(16, dtype=torch.uint8, device="cuda"))
    j, _ = _case("no_feats")                                       # D = 0
    with pytest.raises(L.AmpnetError, match="dfeats"):
        _run(L, j, dfeats=torch.zeros((2, 70, 4), device="cuda"))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, dict(i, dout=i["dout"][:, :, :48]), layers=R.make_layers(1, 9, [48]))
    with pytest.raises(L.AmpnetError, match="layers"):
        _run(L, dict(i, dout=i["dout"][:, :, :32]), layers=R.make_layers(1, 9, [32, 32, 32, 32]))
    with pytest.raises(L.AmpnetError, match="nsample"):
        _run(L, i, group_idx=np.zeros((2, 9, 65), np.int32))
    with pytest.raises(L.AmpnetError, match="320"):
        _run(L, dict(i, dout=i["dout"][:, :, :32]), layers=R.make_layers(1, 321, [32]), feats=np.zeros((2, 70, 318), np.float32))
    # the LDS limit: nsample = 64 (two row tiles) with cin_0 = 320 and [256, 256, 256] -- from both entry points
    wide = [256, 256, 256]
    with pytest.raises(L.AmpnetError, match="workspace_bytes.*LDS"):
        L.sa_backward_workspace_bytes(317, 2, 9, 64, wide)
    assert L.sa_backward_workspace_bytes(317, 2, 9, 32, wide) > 0                  # the same stack at nsample = 32 is accepted
    dummy = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(dummy.data_ptr())
    table = (ctypes.c_void_p * 18)(*[dummy.data_ptr()] * 18)
    gtable = (ctypes.c_void_p * 12)(*[dummy.data_ptr()] * 12)
    rc = L.lib().ampnet_sa_backward_f32(p, 2, 70, 3, p, 9, p, 64, p, 317, table, (ctypes.c_int * 3)(*wide), (ctypes.c_float * 3)(*[1e-5] * 3), 3,
                                        p, None, gtable, None, p, ctypes.c_size_t(dummy.numel() * 4), None)     # (refused before any launch)
    assert rc != 0
    with pytest.raises(L.AmpnetError, match="ampnet_sa_backward_f32.*LDS"):
        L.check(rc, "ampnet_sa_backward_f32")
