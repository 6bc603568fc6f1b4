"""The yardstick of the group_all set abstraction checked without a GPU: tests/sa_all_ref.py against torch's float64 composition
(Conv2d 1x1 + BatchNorm2d.eval() + ReLU per layer on [B, C, N, 1], then max; autograd for the backward); every seeded case settles and
shows what it is there for; the backward over the compacted winner chunks with the masked dout equals the full backward; and the host
side of the new entry points: the module constructs, the library exports the symbols, the workspace sizes answer, misuse is an error."""
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
import sa_all_ref as R                             # noqa: E402
import sa_bwd_ref                                  # noqa: E402

NAMES = [c[0] for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, tape, float64 argmax) of a case, computed once and shared (nobody writes to them)."""
    i = R.case_inputs(sub("synthetic"), name)
    tape, worst = R.forward_tape(i["xyz"], i["feats"], i["layers"], i["eps"])
    assert worst > R.RELU_MARGIN
    return i, tape, R.float64_argmax(tape, R.N_CLOUDS)


def _torch(i):
    """float64 torch layers on [B, C, N, 1] -> (out [B, cout_last], {name: gradient})."""
    d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    xyz = d(i["xyz"])
    feats = None if i["feats"] is None else d(i["feats"]).requires_grad_(True)
    x = (xyz if feats is None else torch.cat([xyz, feats], -1)).transpose(1, 2).unsqueeze(-1)       # [B, C, N, 1]
    mods = []
    for layer, e in zip(i["layers"], i["eps"]):
        cout, cin = layer[0].shape
        conv, bn = torch.nn.Conv2d(cin, cout, 1).double(), torch.nn.BatchNorm2d(cout, eps=float(np.float32(e))).double().eval()
        with torch.no_grad():
            conv.weight.copy_(d(layer[0]).reshape(cout, cin, 1, 1))
            conv.bias.copy_(d(layer[1]))
            bn.weight.copy_(d(layer[2]))
            bn.bias.copy_(d(layer[3]))
            bn.running_mean.copy_(d(layer[4]))
            bn.running_var.copy_(d(layer[5]))
        mods.append((conv, bn))
        x = torch.relu(bn(conv(x)))
    out = torch.max(x, 2)[0].squeeze(-1)                                                           # [B, cout_last]
    (out * d(i["dout"])).sum().backward()
    res = {} if feats is None else {"dfeats": feats.grad.numpy()}
    for l, (conv, bn) in enumerate(mods):
        res.update({f"dW{l}": conv.weight.grad.numpy().reshape(conv.weight.shape[:2]), f"dbias{l}": conv.bias.grad.numpy(),
                    f"dgamma{l}": bn.weight.grad.numpy(), f"dbeta{l}": bn.bias.grad.numpy()})
    return out.detach().numpy(), res


def _close(a, b):
    return np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", ["n1", "n5", "n33", "n65", "n150", "duplicates", "dead_channel"])
def test_restatement_agrees_with_float64_torch(name):
    i, tape, arg = _case(name)
    R.check_argmax(arg, tape, i["xyz"], i["feats"])
    out, bar = R.forward(i["xyz"], i["feats"], i["layers"], i["eps"])
    want_out, want = _torch(i)
    assert out.shape == want_out.shape == bar.shape and (bar >= 0).all() and _close(out, want_out)
    got = R.backward(i["xyz"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
    assert sorted(got) == sorted(want) == sorted(sa_bwd_ref.output_names(len(i["layers"]), i["feats"] is not None))
    for k, (v, b) in got.items():
        assert v.shape == want[k].shape and b.shape == v.shape and (b >= 0).all(), k
        w = want[k]
        if name == "duplicates" and k == "dfeats":          # torch may send a tie to either twin: compare the twins' sum
            assert (v[:, 35:] == 0).all()                   # the restatement, like the kernels, sends it to the lower row
            v, w = v[:, :35] + v[:, 35:], w[:, :35] + w[:, 35:]
        assert _close(v, w), k
        assert np.abs(w).max() > 0, k


@pytest.mark.parametrize("name", NAMES)
def test_every_case_settles_and_shows_its_point(name):
    i, tape, arg = _case(name)                              # (settle_betas and the ReLU-margin assertion run inside)
    n = i["xyz"].shape[1]
    R.check_argmax(arg, tape, i["xyz"], i["feats"])
    distinct = [len(np.unique(arg[b])) for b in range(R.N_CLOUDS)]
    if name == "n5":
        assert max(distinct) <= 5 < R.CHUNK                 # fewer winners than one chunk
    if name == "wide":
        assert min(distinct) > R.CHUNK                      # several chunks
    if name == "n150_chunks":
        assert R.CHUNK < min(distinct) and max(distinct) <= 3 * R.CHUNK  # full, partly filled and empty chunks in one cloud
    if name == "duplicates":
        assert (arg < 35).all() and (i["xyz"][:, 35:] == i["xyz"][:, :35]).all()
        twin = arg.copy()
        twin[0, 0] += 35                                    # the same value, but not the lowest row that has it
        with pytest.raises(AssertionError, match="duplicate"):
            R.check_argmax(twin, tape, i["xyz"], i["feats"])
    if name == "dead_channel":
        out, _ = R.forward(i["xyz"], i["feats"], i["layers"], i["eps"])
        assert (tape[-1][5][:, R.DEAD] < 0).all() and (out[:, R.DEAD] == 0).all() and (arg[:, R.DEAD] == 0).all()
        got = R.backward(i["xyz"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
        L = len(i["layers"])
        assert all(got[f"{k}{L - 1}"][0][R.DEAD].max() == 0 == got[f"{k}{L - 1}"][0][R.DEAD].min() for k in ("dW", "dbias", "dgamma", "dbeta"))
    out_of_range = arg.copy()
    out_of_range[0, 0] = n
    with pytest.raises(AssertionError, match="nsample"):
        R.check_argmax(out_of_range, tape, i["xyz"], i["feats"])


@pytest.mark.parametrize("name", NAMES)
def test_backward_over_the_compacted_winners_equals_the_full_backward(name):
    i, tape, arg = _case(name)
    n = i["xyz"].shape[1]
    full = R.backward(i["xyz"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
    got, winners, ctape, gi, arg_k = R.backward_compacted(i["xyz"], i["feats"], i["layers"], i["eps"], i["dout"], arg)
    B, K, C = arg_k.shape
    assert K == C // R.CHUNK and gi.shape == (B, K, R.CHUNK)
    dout_k = R.compact(arg, i["dout"], n)[2]
    assert np.array_equal(dout_k.sum(1), i["dout"]) and ((dout_k != 0).sum(1) <= 1).all()      # every column's dout in exactly one chunk
    for b in range(B):
        w = winners[b]
        assert (np.diff(w) > 0).all() and set(w) == set(arg[b])                  # distinct, ascending, all of them
        flat = gi[b].reshape(-1)
        assert np.array_equal(flat[:len(w)], w)                                  # compacted: the real members come first, in order
        for k in range(K):
            members = w[R.CHUNK * k:R.CHUNK * (k + 1)]
            assert (gi[b, k, len(members):] == (members[0] if len(members) else w[0])).all()
    # inside a chunk the recomputed max of a column whose winner is there is that winner again (lowest row of the chunk that attains it)
    v = np.maximum(ctape[-1][5], 0.0).reshape(B, K, R.CHUNK, C)
    local = v.argmax(2)
    here = dout_k != 0
    assert np.array_equal(local[here], arg_k[here])
    assert np.array_equal(np.take_along_axis(gi, local, 2)[here], np.broadcast_to(arg[:, None, :], here.shape)[here])
    assert sorted(got) == sorted(full)
    for k, (val, _) in full.items():
        assert got[k][0].shape == val.shape and _close(got[k][0], val), k
    if i["feats"] is not None:
        for b in range(B):
            losers = np.setdiff1d(np.arange(n), winners[b])
            assert (got["dfeats"][0][b, losers] == 0).all()                      # zero outside the winners


# ---- what fails before group_all is built: the module, the symbols, the host-side answers -----------------------------------------------
SYMBOLS = ("ampnet_sa_all_forward_workspace_bytes", "ampnet_sa_all_forward_f32", "ampnet_sa_all_backward_workspace_bytes",
           "ampnet_sa_all_backward_f32")


def test_group_all_block_constructs():
    M = sub("pointNet.model.pointnet2_utils")
    sa = M.PointNetSetAbstraction(None, None, None, 12, [32], True, device="cpu")
    assert sa.group_all is True
    assert list(sa.state_dict()) == ["mlp_convs.0.weight", "mlp_convs.0.bias", "mlp_bns.0.weight", "mlp_bns.0.bias", "mlp_bns.0.running_mean",
                                     "mlp_bns.0.running_var", "mlp_bns.0.num_batches_tracked"]
    assert tuple(sa.mlp_convs[0].weight.shape) == (32, 12, 1, 1)
    with pytest.raises(NotImplementedError, match="group_all.*train mode"):
        M.PointNetSetAbstraction(None, None, None, 12, [32], True, device="cpu", batch_stats=True)
    with pytest.raises(NotImplementedError, match="group_all"):
        M.PointNetSetAbstraction(None, None, None, 12, [48], True, device="cpu")
    with pytest.raises(NotImplementedError, match="group_all"):
        M.PointNetSetAbstraction(None, None, None, 2, [32], True, device="cpu")
    assert M.PointNetSetAbstraction(16, 0.2, 32, 12, [32], False, device="cpu").group_all is False


def test_library_exports_the_group_all_entry_points():
    L = sub("_lib")
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s + "(" in header, s
    assert lib.ampnet_abi_version() == L.ABI_VERSION == 18      # the entry points above arrived within ABI 17; the baseline probe made it 18


def test_workspace_sizes_answer_on_the_host():
    L = sub("_lib")
    fwd, bwd = L.sa_all_forward_workspace_bytes, L.sa_all_backward_workspace_bytes
    small = fwd(6, 2, 70, [32, 64])
    assert small >= L.SA_WORKSPACE_BYTES + 2 * 3 * 64 * 8                        # the fold and ceil(70 / 32) = 3 partial rows per cloud
    assert fwd(6, 2, 64, [32, 64]) < small < fwd(6, 2, 150, [32, 64])
    assert fwd(6, 2, 1 << 20, [32, 64]) == fwd(6, 2, 1 << 22, [32, 64])          # at most 256 runs per cloud, whatever N
    assert fwd(317, 2, 5, [256, 256, 256]) > 0                                   # every stack of the ball-query forward, any N
    # the backward works on the winners alone: its workspace does not grow with N, and it holds the inner backward's
    assert bwd(6, 2, 70, [32, 64]) == bwd(6, 2, 1 << 20, [32, 64]) > L.sa_backward_workspace_bytes(6, 2, 2, 32, [32, 64])
    assert bwd(317, 2, 70, [256, 256, 256]) > 0
    for fn in (fwd, bwd):
        with pytest.raises(L.AmpnetError, match="multiple of 32"):
            fn(6, 2, 70, [32, 48])
        with pytest.raises(L.AmpnetError, match="multiple of 32"):
            fn(6, 2, 70, [288])
        with pytest.raises(L.AmpnetError, match="layers"):
            fn(6, 2, 70, [32, 32, 32, 32])
        with pytest.raises(L.AmpnetError, match="320"):
            fn(318, 2, 70, [32])
        with pytest.raises(L.AmpnetError, match="n=0"):
            fn(6, 2, 0, [32])
        with pytest.raises(L.AmpnetError, match="2\\^31"):
            fn(6, 1 << 16, 1 << 16, [32])


def test_null_pointers_and_bad_shapes_are_errors_not_crashes():
    """Every check runs on the host before any launch: host memory stands in for the device pointers, nothing is dereferenced."""
    L = sub("_lib")
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    table, gtable = (ctypes.c_void_p * 6)(*[p.value] * 6), (ctypes.c_void_p * 4)(*[p.value] * 4)
    couts, eps = (ctypes.c_int * 1)(32), (ctypes.c_float * 1)(1e-5)
    big = ctypes.c_size_t(1 << 30)

    def fwd(xyz=p, n_clouds=2, n=70, ld=3, feats=p, D=6, table=table, couts=couts, L_=1, out=p, ws=p, ws_bytes=big):
        return lib.ampnet_sa_all_forward_f32(xyz, n_clouds, n, ld, feats, D, table, couts, eps, L_, out, None, ws, ws_bytes, None)

    def bwd(xyz=p, n_clouds=2, n=70, ld=3, feats=p, D=6, table=table, couts=couts, L_=1, arg=p, dout=p, dfeats=None, gtable=gtable, ws=p,
            ws_bytes=big):
        return lib.ampnet_sa_all_backward_f32(xyz, n_clouds, n, ld, feats, D, table, couts, eps, L_, arg, dout, dfeats, gtable, ws, ws_bytes, None)

    def refused(rc, name, pattern):
        assert rc == -1
        with pytest.raises(L.AmpnetError, match=name + ".*" + pattern):
            L.check(rc, name)

    for fn, name in ((fwd, "ampnet_sa_all_forward_f32"), (bwd, "ampnet_sa_all_backward_f32")):
        refused(fn(xyz=None), name, "null pointer")
        refused(fn(table=None), name, "null pointer")
        refused(fn(couts=None), name, "null pointer")
        refused(fn(n=0), name, "n=0")
        refused(fn(n_clouds=0), name, "n_clouds=0")
        refused(fn(ld=2), name, "ld=2")
        refused(fn(feats=None), name, "feats must be NULL exactly when D = 0")
        refused(fn(D=0), name, "feats must be NULL exactly when D = 0")
        refused(fn(D=318), name, "320")
        refused(fn(L_=0), name, "layers")
        refused(fn(couts=(ctypes.c_int * 1)(48)), name, "multiple of 32")
        refused(fn(n_clouds=1 << 16, n=1 << 16), name, "2\\^31")
        refused(fn(ws=None), name, "workspace")
        refused(fn(ws_bytes=ctypes.c_size_t(1024)), name, "workspace of 1024 bytes, need")
        refused(fn(table=(ctypes.c_void_p * 6)(p.value, p.value, None, p.value, p.value, p.value)), name, "null parameter 2 of layer 0")
    refused(fwd(out=None), "ampnet_sa_all_forward_f32", "null pointer")
    refused(bwd(arg=None), "ampnet_sa_all_backward_f32", "null pointer")
    refused(bwd(dout=None), "ampnet_sa_all_backward_f32", "null pointer")
    refused(bwd(gtable=None), "ampnet_sa_all_backward_f32", "null pointer")
    refused(bwd(gtable=(ctypes.c_void_p * 4)(p.value, None, p.value, p.value)), "ampnet_sa_all_backward_f32", "null gradient pointer 1 of layer 0")
    refused(bwd(feats=None, D=0, dfeats=p), "ampnet_sa_all_backward_f32", "dfeats must be NULL when D = 0")
