"""The group_all set-abstraction forward (include/ampnet_hip.h: ampnet_sa_all_forward_f32) against the float64 restatement
tests/sa_all_ref.py (the bar is sa_ref.sa_forward's, derived there), and bit for bit against ampnet_sa_forward_f32 on the same rows around
a centre at the origin.  The worst error / bar ratio of every case is printed.  The row the max selects (`arg`) is also compared with the
one ampnet_sa_backward_f32 reports for the same rows as one group: the arg-max walks of the entry points must agree."""
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
from sa_all_run import case as _case, run_forward, to_gpu as _t   # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in R.CASES]


def _ball_forward(L, xyz, feats, layers, centres, group_idx):
    out = torch.full((xyz.shape[0], centres.shape[1], layers[-1][0].shape[0]), float("nan"), device="cuda")
    L.sa_forward_f32(_t(xyz), _t(centres), _t(group_idx), _t(feats), [tuple(_t(a) for a in layer) for layer in layers],
                     [R.BN_EPS] * len(layers), out, torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda"))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_sa_all_forward_within_the_derived_bar(name):
    L = sub("_lib")
    i, tape = _case(name)
    got, arg = run_forward(L, i)                                   # everything starts as NaN / -1: every element must be written
    assert np.isfinite(got).all() and (arg >= 0).all(), name
    again, arg2 = run_forward(L, i, prefill=-7.0)
    assert np.array_equal(got, again) and np.array_equal(arg, arg2), name       # bitwise the same on a second run
    with L.precision_scope("bf16"):
        scoped, arg3 = run_forward(L, i)
    assert np.array_equal(got, scoped) and np.array_equal(arg, arg3), name      # exact fp32 whatever the precision scope
    assert np.array_equal(run_forward(L, i, want_arg=False)[0], got), name      # arg_out = NULL changes nothing else
    want, bar = R.forward(i["xyz"], i["feats"], i["layers"], i["eps"])
    assert want.shape == got.shape and (want > 0).mean() > 0.2
    worst = float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(bar, 1e-300)))
    print(f"sa_all_forward {name}: worst error / bar = {worst:.3f}")
    R.check_argmax(arg, tape, i["xyz"], i["feats"])
    if name == "duplicates":
        assert (arg < 35).all()                                    # rows 35 .. 69 repeat rows 0 .. 34: the lowest row wins
    if name == "dead_channel":
        assert (got[:, R.DEAD] == 0).all() and (arg[:, R.DEAD] == 0).all()
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_sa_all_forward_equals_the_ball_query_kernel_bit_for_bit(name):
    """Point 0 of each cloud at the origin and used as every centre: ampnet_sa_forward_f32 on the 64-row chunks of arange(N) (the tail
    padded with the chunk's first index), max over the chunks, gives the same bits; on every row as a group of its own it gives the float32
    relu(y) per row, whose max is `out` and whose lowest maximal row is `arg_out`, exactly."""
    L = sub("_lib")
    i, _ = _case(name)
    xyz = i["xyz"].copy()
    xyz[:, 0] = 0.0
    B, n = xyz.shape[:2]
    got, arg = run_forward(L, i, xyz=xyz)
    chunks = -(-n // 64)
    gi = np.zeros((B, chunks, 64), np.int32)
    for k in range(chunks):
        members = np.arange(64 * k, min(n, 64 * k + 64))
        gi[:, k] = members[0]
        gi[:, k, :len(members)] = members
    by_chunk = _ball_forward(L, xyz, i["feats"], i["layers"], np.zeros((B, chunks), np.int32), gi)
    assert np.array_equal(by_chunk.max(1), got), name
    rows32 = _ball_forward(L, xyz, i["feats"], i["layers"], np.zeros((B, n), np.int32), np.tile(np.arange(n, dtype=np.int32)[None, :, None], (B, 1, 1)))
    assert np.array_equal(rows32.max(1), got), name
    assert np.array_equal(rows32.argmax(1), arg), name


def test_sa_all_forward_ignores_extra_xyz_columns():
    L = sub("_lib")
    i, _ = _case("n65")
    base = run_forward(L, i)
    wide = np.concatenate([i["xyz"], 50.0 + i["xyz"]], -1)         # ld = 6
    got = run_forward(L, i, xyz=wide)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


def test_sa_all_forward_many_tiles_per_run():
    """N = 32 * 256 * 2 + 5: more tiles than runs, so a wave walks several tiles and merges them into its own partial row; the winners are
    planted in the first and the last tile of a run, at a run's border and in the ragged last tile."""
    L = sub("_lib")
    i, _ = _case("n33")                                            # D = 0, [32]
    n = 32 * 256 * 2 + 5
    xyz = np.tile(i["xyz"][:, :1], (1, n, 1))                      # every row is row 0 ..
    plant = np.array([1, 63, 64, 32 * 300 + 7, n - 1])             # .. but these, which take rows of the seeded cloud
    xyz[:, plant] = i["xyz"][:, 1:6]
    got, arg = run_forward(L, i, xyz=xyz)
    small = np.ascontiguousarray(xyz[:, np.concatenate([[0], plant])])
    want, warg = run_forward(L, i, xyz=small)
    assert np.array_equal(got, want)
    assert np.array_equal(arg, np.concatenate([[0], plant])[warg])
    assert len(np.unique(arg)) >= 3                                # (several of the planted rows do win)


def test_sa_all_forward_refusals():
    """Every misuse is an AmpnetError that says what is wrong: there is no other path."""
    L = sub("_lib")
    i, _ = _case("n32")                                            # n 32, D 6, [32, 64]
    with pytest.raises(L.AmpnetError, match="workspace"):
        run_forward(L, i, ws_short=1)
    with pytest.raises(L.AmpnetError, match="out"):
        run_forward(L, i, out_shape=(2, 32))
    with pytest.raises(L.AmpnetError, match="out"):
        run_forward(L, i, out_shape=(2, 1, 64))
    with pytest.raises(L.AmpnetError, match="arg_out"):
        run_forward(L, i, arg_shape=(2, 32))
    with pytest.raises(L.AmpnetError, match="layer 0"):
        run_forward(L, i, feats=i["feats"][:, :, :5])              # weight [32, 9] against cin_0 = 3 + 5
    with pytest.raises(L.AmpnetError, match="layer 0"):
        run_forward(L, i, feats=None)
    with pytest.raises(L.AmpnetError, match="feats"):
        run_forward(L, i, feats=i["feats"][:, :31])
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        run_forward(L, i, layers=R.sa_ref.make_layers(1, 9, [32, 48]))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        run_forward(L, i, layers=R.sa_ref.make_layers(1, 9, [288]))
    with pytest.raises(L.AmpnetError, match="layers"):
        run_forward(L, i, layers=R.sa_ref.make_layers(1, 9, [32, 32, 32, 32]))
    with pytest.raises(L.AmpnetError, match="320"):
        run_forward(L, i, layers=R.sa_ref.make_layers(1, 321, [32]), feats=np.zeros((2, 32, 318), np.float32))
    with pytest.raises(L.AmpnetError, match="GPU"):
        L.sa_all_forward_f32(torch.zeros(2, 32, 3), None, [], [], torch.zeros(2, 32), torch.zeros(8, dtype=torch.uint8))


@pytest.mark.parametrize("n, repeat_from", [(8, 4), (40, 32), (1, None)])
def test_sa_all_arg_equals_the_grouped_backward_arg(n, repeat_from):
    """The same rows through both arg-max walks: as ONE group (group_idx = arange(n), the centre a point at the exact origin) through
    ampnet_sa_backward_f32(..., arg_out), and as a whole cloud through ampnet_sa_all_forward_f32(..., arg_out).  The rows from
    `repeat_from` on repeat the first rows bit for bit, so every column's maximum is attained twice: n = 8 ties rows r and r + 4, which
    sit in the two lane halves of one accumulator; n = 40 ties rows r and r + 32, which sit in two row tiles (two tiles of one group
    there, two runs of one cloud here).  The lowest row must win in both, and `out` must be ampnet_sa_forward_f32's on that group."""
    L = sub("_lib")
    B, D, widths = 2, 6, [32, 64]
    rng = np.random.default_rng(9100 + n)
    xyz = rng.uniform(-1.0, 1.0, (B, n, 3)).astype(np.float32)
    feats = rng.uniform(-1.0, 1.0, (B, n, D)).astype(np.float32)
    xyz[:, 0] = 0.0                                                # the centre: x - 0 is exact
    if repeat_from is not None:
        xyz[:, repeat_from:] = xyz[:, :n - repeat_from]
        feats[:, repeat_from:] = feats[:, :n - repeat_from]
    layers = R.sa_ref.make_layers(9200 + n, 3 + D, widths)
    i = {"xyz": xyz, "feats": feats, "layers": layers}
    out_all, arg_all = run_forward(L, i)
    centres = np.zeros((B, 1), np.int32)
    group_idx = np.tile(np.arange(n, dtype=np.int32), (B, 1, 1))
    out_ball = _ball_forward(L, xyz, feats, layers, centres, group_idx)
    glayers = [tuple(_t(a) for a in layer) for layer in layers]
    grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in glayers]
    arg_bwd = torch.full((B, 1, widths[-1]), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.sa_backward_workspace_bytes(D, B, 1, n, widths), dtype=torch.uint8, device="cuda")
    L.sa_backward_f32(_t(xyz), _t(centres), _t(group_idx), _t(feats), glayers, [R.BN_EPS] * len(layers),
                      torch.ones((B, 1, widths[-1]), device="cuda"), None, grads, ws, arg_out=arg_bwd)
    torch.cuda.synchronize()
    assert torch.equal(arg_bwd[:, 0].cpu(), torch.from_numpy(arg_all)), (n, arg_bwd[:, 0].cpu(), arg_all)
    assert np.array_equal(out_all, out_ball[:, 0]), n
    assert (arg_all >= 0).all() and (arg_all < (n if repeat_from is None else repeat_from)).all(), n   # a repeated row never wins
