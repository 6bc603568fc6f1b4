"""Layer-local float64 parity of the BatchNorm / pooling glue kernels (csrc/pw_misc.hip, the small kernels of csrc/bwd_misc.hip, reduce_windows
of csrc/pw_bwd.hip): the kernels that turn a layer's partials into the numbers every later kernel consumes.

Each case launches ONE kernel (or one host entry point) through ampnet_probe_bn_f32 (include/ampnet_hip.h, "test hooks") on inputs built here
and holds every output to the float64 restatement of tests/bn_probe.py (itself held to torch in tests/test_bn_refs_cpu.py), at the project's one
bar 8 eps sqrt(K) mag + 2 eps |x64| (K = 1 where the kernel sums in double).  Every case also checks: outputs pre-filled with NaN (-7 for int32)
are finite where the contract writes and keep the sentinel bits where it does not (tails past the extent, padding columns of ld > cols, partial
slots past the plan); a second run on re-poisoned outputs is bitwise identical; the worst error/bar of each kernel family is printed at teardown.
Inputs the contract says are not read (the sums of zero-row partials, the values of empty pool chunks) hold NaN.

Cases and the branch each is for
  pw_input      windows [1, 3, 4, 5, 255, 256, 257, 513, 700], 3 slots, chunk_rows 512: waves with no row, the 256-row staging boundary, a second
                chunk; modes 0 / 1 / 1 with slot-major T, fp32 / bf16 Z, three grids: per-chunk without partials (eval), per-chunk with partials,
                persistent with part_rows.  `many`: Q = 1100 windows of 1 .. 9 rows, 9 slots, persistent: more items than lanes (lanes walk
                several items, heavy lanes first, the trailing part_rows = 0).  `offset`: xyz + 100, mean^2 >> variance (the shifted sums).
  bn_finalize   C in {40, 64, 256}, optional outputs present / NULL.  `ragged2` / `ragged3`: per-chunk partials from a ragged win_off with an
                empty window and trailing empty chunks, chunks 2 (shift shortcut) and 3 (division); `uniform`: uniform_rows; `rows`: explicit
                part_rows with zero-row partials, a slot with exactly one row (unbiased variance = M2) and a slot with none (mean 0,
                invstd 1 / sqrt(eps)); `two_stage`: 1 slot, 208 partials, with and without merge_ws; `gathered`: bn_finalize_gathered, 3 ranks,
                2 slots, one rank with no row in a slot.
  bn_fold, bn_running_update, bn_param_grads   lists of 1, 3, 24 items with C cycling through {9, 64, 256, 1024} (the stride loop past 256
                threads), 25 refused; n_slots in {1, 3, 12}.
  pool_finalize plain kernel: chunks 1 / 3, C 256 / 40, out_slot_major 0 / 1, arg / zext present / NULL; negative and exactly-zero scales;
                equal extremes in chunks 0 and 2 (the earlier wins); a window with no row (arg -1, pooled relu(shift)); the eval form without
                part_amax (empty chunks hold the matching infinity).  In-kernel BatchNorm form (C 256): pfin_parts / n_slots in {1, 57, 70}
                (70: past one trip of the 64-wide loop, not a multiple of 4), zero-row partials, Q / n_slots = 6 (the early return), a
                large-mean channel; its BatchNorm outputs also against bn_finalize on the same partials.
  bn_bwd_finalize  <64>: 3 slots, C 128 / 40, chunks 1 / 3, win_off / uniform_rows, part_Q 0 / > 0, a slot with no row (P2 = P3 = 0); <16>: 1
                slot, C 64, part_Q 600.  Which instantiation runs is the rule of kernels.h (BnBwdFinalize), restated in bwd_cpb(): each case
                asserts it is on the intended side.
  fc_bn_bwd     per in {1, 2, 8, 63, 64, 65, 200}, 3 slots, C in {40, 256, 512}; dead rows with da set.  fc_act, fc_act_pair (= two fc_act
                calls bitwise), colsum rows {1, 7, 8, 25, 32, 33, 1000} x C {1, 31, 32, 33, 256}.
  reduce_windows  Q in {1, 7, 8, 57, 64, 65, 121, 600} (the edges of qi + 56 < Q), accumulate 0 / 1, ld_part > cols, ld_dst > cols, rows * cols
                not a multiple of 32; reduce_windows_multi: 12 items, each bitwise the single launch, 13 refused.  transpose64_slot_major:
                Q 12, 3 slots, chunks {1, 3, 8, 9}, by_workgroup 0 / 1, add NULL / present.  add_identity (k 3, 64), fill_i32_ramp: exact.
  test_probe_refuses_short_buffers: every buffer of every op one element short -> AMPNET_E_ARG, nothing written.

Left out: sync_bn_bwd_constants and sync_bn_fc_apply read buffers that only a collective exchange fills; the two-rank layer tests of
tests/test_syncbn_layers_gpu.py cover them (ops 1, 6 and 10 of the probe run with a collective installed, the others refuse).

Observed worst error/bar on the MI355X: pw_input Z 0.16 (bf16 Z 0.50: half an ulp of bf16 against the 2 EPS16 |z| term), slot mean 0.02, variance 0.01
(offset case included); bn_finalize scale 0.18, shift 0.13, mean / invstd / stat_mean / stat_uvar 0.10; its two-stage form invstd 0.39, stat_uvar 0.62
(the merged sub-slots pass through fp32), two- against one-stage 0.54; bn_fold scale 0.25, shift 0.13; bn_running_update 0.13 / 0.16; pool_finalize
pooled 0.09 (arg and zext exact); pool_finalize_bn scale 0.18, shift 0.11, pooled 0.10, the other outputs 0.10, against bn_finalize on the same partials
0.0000; bn_bwd_finalize<64> 0.10 on all four outputs, <16> P1 0.09, P2 / P3 / slot_ab 0.01; bn_param_grads 0.12; fc_act 0.10; fc_bn_bwd g 0.14, slot_ab
0.19; colsum 0.09; reduce_windows 0.07 (+= 0.07, multi 0.08); transpose64 0.13.
"""
import numpy as np
import pytest
import torch

import bn_probe as B
import pw_probe as PP
from pw_probe import EPS16, EPS32

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
TAIL = 8
WORST = {}
f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
cdiv = lambda a, b: (a + b - 1) // b


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[bn glue] worst error/bar {k}: {WORST[k]:.4f}")


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    assert r <= 1.0, f"{family}: error at {r:.3f} of the bar"
    return r


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device="cuda", dtype=dtype or t.dtype)


def host(t):
    return t.detach().cpu().numpy()


def out(n, tail=TAIL, dtype=torch.float32):
    """an output of n elements (+ `tail` more that nothing may write), poisoned."""
    t = torch.empty(int(n) + tail, dtype=dtype, device="cuda")
    poison(t)
    return t


def poison(t):
    if t.dtype == torch.int32:
        t.fill_(-7)
    elif t.dtype == torch.bfloat16:
        t.view(torch.int16).fill_(0x7FC0)
    else:
        t.fill_(float("nan"))


def sentinel(a):
    """elementwise: still the poison bits."""
    if a.dtype == torch.int32:
        return host(a) == -7
    if a.dtype == torch.bfloat16:
        return host(a.view(torch.int16)) == 0x7FC0
    return host(a.view(torch.int32)) == NAN_BITS


def bits(t):
    t = t.detach().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == torch.bfloat16 else t)


def launch(d, outs, restore=None):
    """run, snapshot, re-poison (or restore the in-place operands), run again: bitwise equal.  The outputs hold the second run."""
    rc, names = B.run(d)
    assert rc == 0, PP.last_error()
    assert names == [], names
    first = {k: bits(v).clone() for k, v in outs.items() if v is not None}
    for k, v in outs.items():
        if v is None:
            continue
        if restore and k in restore:
            v.copy_(restore[k])
        else:
            poison(v)
    rc, _ = B.run(d)
    assert rc == 0, PP.last_error()
    for k, v in first.items():
        assert torch.equal(v, bits(outs[k])), f"{k}: second run differs bitwise"


def written(t, n, what):
    """the first n elements written (no sentinel), the tail untouched; returns them as numpy."""
    s = sentinel(t)
    assert not s[:n].any(), f"{what}: sentinel left where the contract writes"
    assert s[n:].all(), f"{what}: written past its extent"
    a = host(t.float() if t.dtype == torch.bfloat16 else t)[:n]
    return a


def offsets(win):
    return np.concatenate([[0], np.cumsum(win)]).astype(np.int32)


# =====================================================================================================================================
# pw_input
# =====================================================================================================================================
WIN_A = [1, 3, 4, 5, 255, 256, 257, 513, 700]
INPUT_CASES = [("A", mode, sm, zb, grid, 0) for (mode, sm) in ((0, 0), (1, 0), (1, 1)) for zb in (0, 1) for grid in ("eval", "chunk", "persist")] + \
              [("many", 0, 0, 0, "persist", 0), ("many", 1, 0, 0, "persist", 0)] + \
              [("A", mode, sm, 0, grid, 1) for (mode, sm) in ((0, 0), (1, 1)) for grid in ("chunk", "persist")]
_INPUT_CACHE = {}


def input_data(name, mode, sm, offset):
    """inputs and their float64 reference, computed once per (shape, mode) and shared by the grids / Z formats."""
    key = (name, mode, sm, offset)
    if key not in _INPUT_CACHE:
        rng = np.random.default_rng(sum(map(ord, name)) + 10 * mode + 100 * sm + 1000 * offset)
        if name == "A":
            win, S, chunks = WIN_A, 3, 2
        else:
            win, S, chunks = list(rng.integers(1, 10, 1100)), 9, 1
        wo = offsets(win)
        x = f32(rng.standard_normal((int(wo[-1]), 9)))
        if offset:
            x[:, :3] += 100.0
        W = f32(rng.standard_normal((64, 12 if mode else 3)) * 0.5)
        T = f32(np.eye(3)[None] + 0.3 * rng.standard_normal((len(win), 3, 3))) if mode else None
        Z, M, K = B.input_ref(x, W, T, mode, wo, S, sm)
        _INPUT_CACHE[key] = dict(win=win, S=S, chunks=chunks, wo=wo, x=x, W=W, T=T, Z=Z, M=M, K=K, z32={})
    return _INPUT_CACHE[key]


def build_input(c, mode, sm, zb, grid, tail=TAIL):
    Q, S, chunks, rows = len(c["win"]), c["S"], c["chunks"], int(c["wo"][-1])
    d = B.new("pw_input", mode=mode, perwin_slot_major=sm, n_slots=S, z_bf16=zb, Q=Q, chunk_rows=512, chunks=chunks)
    outs = {"Z": out(rows * 64, tail, torch.bfloat16 if zb else torch.float32)}
    lanes = parts = 0
    if grid == "chunk":
        outs["part_sum"], outs["part_sq"] = out(Q * chunks * 64, tail), out(Q * chunks * 64, tail)
    elif grid == "persist":
        p = B.plan(Q, chunks, S)
        lanes, parts = p.input_stat_lanes, p.input_stat_parts
        d.stat_lanes = lanes
        outs["part_sum"], outs["part_sq"], outs["part_rows"] = out(parts * 64, tail), out(parts * 64, tail), out(parts, tail, torch.int32)
    ins = dict(x=dev(c["x"]), W=dev(c["W"]), T=dev(c["T"]) if mode else None, win_off=dev(c["wo"]))
    B.set_tensors(d, **ins, **outs)
    return d, ins, outs, lanes, parts


@pytest.mark.parametrize("name,mode,sm,zb,grid,offset", INPUT_CASES)
def test_pw_input(name, mode, sm, zb, grid, offset):
    c = input_data(name, mode, sm, offset)
    Q, S, chunks, rows, wo = len(c["win"]), c["S"], c["chunks"], int(c["wo"][-1]), c["wo"]
    d, ins, outs, lanes, parts = build_input(c, mode, sm, zb, grid)
    launch(d, outs)
    Z = written(outs["Z"], rows * 64, "Z").reshape(rows, 64)
    fam = f"pw_input mode {mode}"
    if zb:
        b = 8 * EPS32 * np.sqrt(c["K"]) * c["M"] + 2 * EPS16 * np.abs(c["Z"])          # the stored value: the bf16 unit roundoff on |z|
        note(fam + " Z bf16", PP.err_ratio(Z, c["Z"], b))
        if grid in c["z32"]:                                                             # and exactly the fp32 result rounded to nearest even
            assert torch.equal(c["z32"][grid].to(torch.bfloat16).view(torch.int16), bits(outs["Z"])[:rows * 64])
    else:
        note(fam + " Z", PP.ratio(Z, c["Z"], c["M"], c["K"]))
        c["z32"][grid] = outs["Z"].detach().cpu()[:rows * 64].clone()
    if grid == "eval":
        return
    slot_of_row = PP.win_of_rows(wo) % S
    if grid == "chunk":
        n = B.chunk_rows_of(wo, chunks, 512).reshape(-1)
        ps = written(outs["part_sum"], Q * chunks * 64, "part_sum").reshape(-1, 64)
        pq = written(outs["part_sq"], Q * chunks * 64, "part_sq").reshape(-1, 64)
        slots = B.slot_of_partial(Q * chunks, chunks, S)
    else:
        # lanes are dealt to the slots, lanes // S each and one more for the first lanes % S (kernels.h: StatLane); partial (slot, j) sits
        # at slot + j * S; a slot with fewer lanes than the others gets rows = 0 in its last partial, whose sums stay unwritten
        assert parts == cdiv(lanes, S) * S
        n = written(outs["part_rows"], parts, "part_rows")
        has_lane = np.array([(p // S) < lanes // S + (1 if p % S < lanes % S else 0) for p in range(parts)])
        assert np.all(n[~has_lane] == 0)
        for k in ("part_sum", "part_sq"):
            s = sentinel(outs[k])[:parts * 64].reshape(parts, 64)
            assert not s[has_lane].any() and s[~has_lane].all() and sentinel(outs[k])[parts * 64:].all(), k
        ps, pq = (np.nan_to_num(host(outs[k])[:parts * 64].reshape(parts, 64)) for k in ("part_sum", "part_sq"))
        slots = np.arange(parts) % S
    assert np.all(np.isfinite(ps)) and np.all(np.isfinite(pq)) and np.all(pq >= 0)
    for s in range(S):
        sel = np.nonzero(slots == s)[0]
        assert int(n[sel].sum()) == int((slot_of_row == s).sum()), f"slot {s}: rows of the partials"
        N, mean, m2 = PP.chan_merge([ps[p] for p in sel], [pq[p] for p in sel], [n[p] for p in sel])
        mu, var, bmean, bvar = PP.moment_bars(c["Z"][slot_of_row == s], c["M"][slot_of_row == s], c["K"])
        note(fam + " mean", PP.err_ratio(mean, mu, bmean))
        note(fam + " var", PP.err_ratio(m2 / N, var, bvar))


# =====================================================================================================================================
# bn_finalize
# =====================================================================================================================================
def make_partials(rng, rows, C):
    """fp32 (mean, M2) [P, C] for partials of `rows` [P] rows; zero-row partials hold NaN (never read); a large-mean channel."""
    rows = np.asarray(rows)
    mean = f32(rng.standard_normal((len(rows), C)) * 0.3 + 2.0 * rng.standard_normal(C))
    mean[:, min(7, C - 1)] += 1000.0
    m2 = f32(np.maximum(rows - 1, 0)[:, None] * (0.5 + rng.random((len(rows), C))))
    mean[rows == 0] = np.nan
    m2[rows == 0] = np.nan
    return mean, m2


def fin_case(name, C):
    rng = np.random.default_rng(C + sum(map(ord, "stage" if name.endswith("_stage") else name)))      # two_stage / one_stage: the same inputs
    k = dict(chunk_rows=512, chunks=1, uniform_rows=0, merge=False, win=None, part_rows=False, gather=0)
    if name in ("ragged2", "ragged3"):
        k["chunks"] = 2 if name == "ragged2" else 3
        k["win"] = [5, 0, 700, 3, 1000 if name == "ragged2" else 1030, 17, 512, 1, 40]
        k["S"], k["Q"] = 3, 9
        rows = B.chunk_rows_of(offsets(k["win"]), k["chunks"], 512).reshape(-1)
    elif name == "uniform":
        k.update(S=3, Q=7, chunks=2, uniform_rows=700)
        rows = np.tile([512, 188], 7)
    elif name == "rows":
        k.update(S=4, Q=4 * 57, part_rows=True)
        rows = rng.integers(0, 40, k["Q"])
        rows[rng.random(k["Q"]) < 0.2] = 0
        rows[1::4] = 0
        rows[1 + 4 * 11] = 1                      # slot 1: exactly one row
        rows[2::4] = 0                            # slot 2: no row
    elif name in ("two_stage", "one_stage"):
        k.update(S=1, Q=208, part_rows=True, merge=name == "two_stage")
        rows = rng.integers(0, 300, 208)
    else:                                         # gathered: 3 ranks x 2 slots, partial (rank, slot); rank 1 has no row in slot 0
        k.update(S=2, Q=6, gather=3)
        rows = np.array([30, 12, 0, 25, 17, 1])
    mean, m2 = make_partials(rng, rows, C)
    if name == "rows":
        m2[1 + 4 * 11] = f32(0.5 + rng.random(C))   # the one-row slot: stat_uvar must be this M2 itself
    if name == "gathered":
        mean, m2 = np.nan_to_num(mean), np.nan_to_num(m2)    # a rank with no row sends zeros
    k.update(rows=rows.astype(np.int32), mean=mean, m2=m2, gamma=f32(rng.standard_normal(C)), beta=f32(rng.standard_normal(C) * 0.5), C=C)
    k["slots"] = np.arange(len(rows)) % k["S"] if k["chunks"] == 1 else B.slot_of_partial(len(rows), k["chunks"], k["S"])
    return k


FIN_OUT = ("scale", "shift", "mean", "invstd", "stat_mean", "stat_uvar")


def build_finalize(k, opt, tail=TAIL):
    S, C = k["S"], k["C"]
    outs = {n: out(S * C, tail) if (opt or n in ("scale", "shift")) else None for n in FIN_OUT}
    ins = dict(gamma=dev(k["gamma"]), beta=dev(k["beta"]))
    if k["gather"]:
        body, seg = S * (2 * C + 1), S * (2 * C + 1) + 5
        buf = np.full((k["gather"] - 1) * seg + body, np.nan, dtype=np.float32)
        for r in range(k["gather"]):
            p = slice(r * S, (r + 1) * S)
            buf[r * seg:r * seg + S * C] = k["mean"][p].reshape(-1)
            buf[r * seg + S * C:r * seg + 2 * S * C] = k["m2"][p].reshape(-1)
            buf[r * seg + 2 * S * C:r * seg + body] = k["rows"][p].view(np.float32)
        d = B.new("bn_finalize_gathered", n_slots=S, C=C, gather_ranks=k["gather"], gather_seg=seg)
        ins["part_sum"] = dev(buf)
    else:
        d = B.new("bn_finalize", n_slots=S, C=C, Q=k["Q"], chunks=k["chunks"], chunk_rows=k["chunk_rows"], uniform_rows=k["uniform_rows"])
        ins.update(part_sum=dev(k["mean"]), part_sq=dev(k["m2"]))
        if k["part_rows"]:
            ins["part_rows"] = dev(k["rows"])
        elif k["win"] is not None:
            ins["win_off"] = dev(offsets(k["win"]))
        if k["merge"]:
            outs["merge_ws"] = out(B.plan(k["Q"], 1, S, C).merge_floats, tail)
    B.set_tensors(d, **ins, **outs)
    return d, ins, outs


def check_finalize(k, outs, fam):
    S, C = k["S"], k["C"]
    ref = B.finalize_ref(np.nan_to_num(k["mean"]), np.nan_to_num(k["m2"]), k["rows"], k["slots"], S, k["gamma"], k["beta"])
    got = {}
    for n in FIN_OUT:
        if outs[n] is not None:
            got[n] = written(outs[n], S * C, n).reshape(S, C)
            note(f"{fam} {n}", B.worst(got[n], ref[n]))
    return ref, got


@pytest.mark.parametrize("opt", [1, 0])
@pytest.mark.parametrize("C", [40, 64, 256])
@pytest.mark.parametrize("name", ["ragged2", "ragged3", "uniform", "rows", "gathered"])
def test_bn_finalize(name, C, opt):
    k = fin_case(name, C)
    d, ins, outs = build_finalize(k, opt)
    launch(d, outs)
    ref, got = check_finalize(k, outs, "bn_finalize")
    if name == "rows" and opt:
        assert ref["N"][1, 0] == 1 and ref["N"][2, 0] == 0
        one = k["m2"][1 + 4 * 11].astype(np.float64)
        assert np.array_equal(got["stat_uvar"][1], f32(one)), "one row: the unbiased variance falls back to M2"
        assert np.all(got["mean"][2] == 0) and np.all(got["stat_uvar"][2] == 0)
        assert np.array_equal(got["invstd"][2], np.full(C, np.float32(1.0 / np.sqrt(B.BN_EPS))))


@pytest.mark.parametrize("C", [40, 64, 256])
def test_bn_finalize_two_stage(C):
    res = {}
    for name in ("two_stage", "one_stage"):
        k = fin_case(name, C)
        assert k["Q"] >= 208 and k["Q"] * k["chunks"] // k["S"] > 192 and k["S"] * 16 <= k["Q"]      # the host entry point's rule for the two-stage form
        d, ins, outs = build_finalize(k, 1)
        launch(d, outs)
        ref, res[name] = check_finalize(k, {n: outs[n] for n in FIN_OUT}, "bn_finalize " + name)
        if name == "two_stage":                   # stage one ran: it left its 16 merged sub-slots in the scratch
            ws = written(outs["merge_ws"], 16 * (2 * C + 1), "merge_ws")
            assert int(ws[32 * C:].view(np.int32).sum()) == int(k["rows"].sum())
    for n in FIN_OUT:
        note("bn_finalize two- vs one-stage", PP.err_ratio(res["two_stage"][n], res["one_stage"][n].astype(np.float64), ref[n][1]))


# =====================================================================================================================================
# bn_fold, bn_running_update, bn_param_grads
# =====================================================================================================================================
ITEM_C = (9, 64, 256, 1024)


def build_items(op, n, S, tail=TAIL, seed=0):
    rng = np.random.default_rng(100 * n + S + seed)
    Cs = [ITEM_C[(i + n) % 4] for i in range(n)]
    tot = sum(Cs)
    d = B.new(op, n_items=n, n_slots=S)
    for i, c in enumerate(Cs):
        d.it_C[i] = c
    h = dict(Cs=Cs, tot=tot)
    if op == "bn_fold":
        h.update(gamma=f32(rng.standard_normal(tot)), beta=f32(rng.standard_normal(tot)), rmean=f32(rng.standard_normal(tot) * 3), rvar=f32(rng.random(tot) * 2 + 1e-3))
        ins = {k: dev(h[k]) for k in ("gamma", "beta", "rmean", "rvar")}
        outs = dict(scale=out(tot, tail), shift=out(tot, tail))
    elif op == "bn_running_update":
        h.update(stat_mean=f32(rng.standard_normal(S * tot) * 3), stat_uvar=f32(rng.random(S * tot) * 2), rmean=f32(rng.standard_normal(tot)), rvar=f32(rng.random(tot) + 0.5))
        ins = {k: dev(h[k]) for k in ("stat_mean", "stat_uvar")}
        outs = dict(rmean=out(tot, tail), rvar=out(tot, tail))
        h["restore"] = {k: dev(np.concatenate([h[k], np.full(tail, np.nan, dtype=np.float32)])) for k in ("rmean", "rvar")}
        for k in outs:
            outs[k].copy_(h["restore"][k])
    else:
        h["slot_ab"] = f32(rng.standard_normal(2 * S * tot))
        ins = dict(slot_ab=dev(h["slot_ab"]))
        outs = dict(dgamma=out(tot, tail), dbeta=out(tot, tail))
    B.set_tensors(d, **ins, **outs)
    return d, h, ins, outs


def item_slices(h, per=1):
    o = 0
    for c in h["Cs"]:
        yield slice(per * o, per * (o + c)), c
        o += c


@pytest.mark.parametrize("n", [1, 3, 24])
def test_bn_fold(n):
    d, h, ins, outs = build_items("bn_fold", n, 1)
    launch(d, outs)
    ref = B.fold_ref(h["gamma"], h["beta"], h["rmean"], h["rvar"])
    for k in ("scale", "shift"):
        note("bn_fold " + k, B.worst(written(outs[k], h["tot"], k), ref[k]))


@pytest.mark.parametrize("S", [1, 3, 12])
@pytest.mark.parametrize("n", [1, 3, 24])
def test_bn_running_update(n, S):
    d, h, ins, outs = build_items("bn_running_update", n, S)
    launch(d, outs, restore=h["restore"])
    got = {k: written(outs[k], h["tot"], k) for k in ("rmean", "rvar")}
    for (sl, c), (ssl, _) in zip(item_slices(h), item_slices(h, S)):
        ref = B.running_ref(h["rmean"][sl], h["rvar"][sl], h["stat_mean"][ssl].reshape(S, c), h["stat_uvar"][ssl].reshape(S, c))
        for k in ("rmean", "rvar"):
            note("bn_running_update " + k, B.worst(got[k][sl], ref[k]))


@pytest.mark.parametrize("S", [1, 3, 12])
@pytest.mark.parametrize("n", [1, 24])
def test_bn_param_grads(n, S):
    d, h, ins, outs = build_items("bn_param_grads", n, S)
    launch(d, outs)
    got = {k: written(outs[k], h["tot"], k) for k in ("dgamma", "dbeta")}
    for (sl, c), (ssl, _) in zip(item_slices(h), item_slices(h, 2 * S)):
        ref = B.param_grads_ref(h["slot_ab"][ssl].reshape(S, c, 2))
        for k in ("dgamma", "dbeta"):
            note("bn_param_grads " + k, B.worst(got[k][sl], ref[k]))


@pytest.mark.parametrize("op", ["bn_fold", "bn_running_update", "bn_param_grads"])
def test_item_lists_refuse_25(op):
    d, h, ins, outs = build_items(op, 25, 3)
    before = {k: bits(v).clone() for k, v in outs.items()}
    rc, names = B.run(d)
    assert rc == B.AMPNET_E_ARG and names == [], (rc, PP.last_error())
    assert "25 items" in PP.last_error()
    assert all(torch.equal(before[k], bits(v)) for k, v in outs.items())


# =====================================================================================================================================
# pool_finalize
# =====================================================================================================================================
def pool_case(chunks, C, seed=0, Q=6, S=3, tracked=True):
    """windows of up to chunks * 16 rows, one of them empty; negative and zero scales; equal extremes in chunks 0 and 2 of window 2."""
    rng = np.random.default_rng(10 * chunks + C + seed)
    base = [5, 0, 40, 16, 33, 48] if chunks == 3 else ([5, 0, 16, 1, 9, 12] if chunks == 1 else [5, 0, 30, 16, 32, 17])
    win = (base * cdiv(Q, 6))[:Q]
    wo = offsets(win)
    z = f32(rng.standard_normal((int(wo[-1]), C)) * 2)
    gamma = f32(rng.standard_normal(C))
    gamma[::5] = -np.abs(gamma[::5]) - 0.1
    gamma[3], gamma[5], gamma[11] = 0.7, -0.7, 0.0
    if chunks == 3:
        r0 = int(wo[2])
        for c, v in ((3, 50.0), (5, -50.0), (11, 50.0)):       # the extreme of the window, twice: rows 2 (chunk 0) and 35 (chunk 2)
            z[r0 + 2, c] = z[r0 + 35, c] = v
    pmax, amax = B.pool_partials(z, wo, chunks, 16, gamma, track=tracked)
    if tracked:
        pmax[amax < 0] = np.nan                                # an empty chunk's value is not read when rows are tracked
    return dict(win=win, wo=wo, z=z, gamma=gamma, pmax=pmax, amax=amax, Q=Q, S=S, C=C, chunks=chunks)


def build_pool(k, scale, shift, slot_major, opt, tail=TAIL):
    Q, C = k["Q"], k["C"]
    d = B.new("pool_finalize", mode=0, Q=Q, n_slots=k["S"], C=C, chunks=k["chunks"], out_slot_major=slot_major)
    outs = dict(pooled=out(Q * C, tail), arg=out(Q * C, tail, torch.int32) if opt and k["amax"] is not None else None, zext=out(Q * C, tail) if opt else None)
    ins = dict(part_max=dev(k["pmax"]), scale=dev(scale), shift=dev(shift))
    if k["amax"] is not None:
        ins.update(part_amax=dev(k["amax"]), win_off=dev(k["wo"]))
    B.set_tensors(d, **ins, **outs)
    return d, ins, outs


def check_pool(k, ref, outs, fam):
    Q, C = k["Q"], k["C"]
    note(fam + " pooled", B.worst(written(outs["pooled"], Q * C, "pooled").reshape(Q, C), ref["pooled"]))
    if outs.get("zext") is not None:
        assert np.array_equal(written(outs["zext"], Q * C, "zext").reshape(Q, C), f32(ref["zext"][0])), "zext is the extreme itself"
    if outs.get("arg") is not None:
        assert np.array_equal(written(outs["arg"], Q * C, "arg").reshape(Q, C), ref["arg"]), "arg"


@pytest.mark.parametrize("opt", [1, 0])
@pytest.mark.parametrize("slot_major", [0, 1])
@pytest.mark.parametrize("C", [256, 40])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("tracked", [True, False])
def test_pool_finalize(tracked, chunks, C, slot_major, opt):
    k = pool_case(chunks, C, tracked=tracked)
    rng = np.random.default_rng(C + chunks)
    scale = f32(k["gamma"][None, :] * (0.5 + rng.random((k["S"], C))))
    shift = f32(rng.standard_normal((k["S"], C)))
    d, ins, outs = build_pool(k, scale, shift, slot_major, opt)
    launch(d, outs)
    ref = B.pool_ref(k["pmax"], k["amax"], scale, shift, k["Q"], chunks, k["S"], slot_major)
    check_pool(k, ref, outs, "pool_finalize" + ("" if tracked else " eval"))
    # the contract's corners, read off the reference: the empty window, the tie, negative and zero scales all occur
    orow1 = (1 % k["S"]) * (k["Q"] // k["S"]) + 1 // k["S"] if slot_major else 1
    assert np.array_equal(ref["pooled"][0][orow1], np.maximum(scale[1 % k["S"]].astype(np.float64) * 0 + shift[1 % k["S"]], 0))
    if tracked:
        assert np.all(ref["arg"][1] == -1)
        if chunks == 3:
            assert np.all(ref["arg"][2][[3, 5, 11]] == k["wo"][2] + 2)


def build_pool_bn(k, pk, tail=TAIL):
    Q, S = k["Q"], k["S"]
    d = B.new("pool_finalize", mode=1, Q=Q, n_slots=S, C=256, chunks=k["chunks"], out_slot_major=1, pfin_parts=len(pk["rows"]))
    outs = dict(pooled=out(Q * 256, tail), arg=out(Q * 256, tail, torch.int32), zext=out(Q * 256, tail), **{n: out(S * 256, tail) for n in FIN_OUT})
    ins = dict(part_max=dev(k["pmax"]), part_amax=dev(k["amax"]), win_off=dev(k["wo"]), part_sum=dev(pk["mean"]), part_sq=dev(pk["m2"]),
               part_rows=dev(pk["rows"]), gamma=dev(k["gamma"]), beta=dev(pk["beta"]))
    B.set_tensors(d, **ins, **outs)
    return d, ins, outs


def pool_bn_case(per_slot):
    k = pool_case(2, 256, seed=per_slot, Q=18)
    rng = np.random.default_rng(per_slot)
    rows = rng.integers(1, 60, 3 * per_slot).astype(np.int32)
    if per_slot > 1:
        rows[rng.random(len(rows)) < 0.25] = 0
        rows[0] = 9
    mean, m2 = make_partials(rng, rows, 256)
    return k, dict(rows=rows, mean=mean, m2=m2, beta=f32(rng.standard_normal(256) * 0.5))


@pytest.mark.parametrize("per_slot", [1, 57, 70])
def test_pool_finalize_bn(per_slot):
    k, pk = pool_bn_case(per_slot)
    Q, S = k["Q"], k["S"]
    assert (Q // S) % 4 != 0
    d, ins, outs = build_pool_bn(k, pk)
    launch(d, outs)
    fref = B.finalize_ref(np.nan_to_num(pk["mean"]), np.nan_to_num(pk["m2"]), pk["rows"], np.arange(len(pk["rows"])) % S, S, k["gamma"], pk["beta"])
    got = {}
    for n in FIN_OUT:
        got[n] = written(outs[n], S * 256, n).reshape(S, 256)
        note("pool_finalize_bn " + n, B.worst(got[n], fref[n]))
    ref = B.pool_ref(k["pmax"], k["amax"], fref["scale"][0], fref["shift"][0], Q, 2, S, 1, fref["scale"][1], fref["shift"][1])
    check_pool(k, ref, outs, "pool_finalize_bn")
    # the same partials through bn_finalize (two-pass variance) agree with the raw-second-moment form within the bar
    fk = dict(S=S, C=256, gather=0, Q=len(pk["rows"]), chunks=1, chunk_rows=512, uniform_rows=0, part_rows=True, win=None, merge=False,
              mean=pk["mean"], m2=pk["m2"], rows=pk["rows"], gamma=k["gamma"], beta=pk["beta"])
    d2, _, o2 = build_finalize(fk, 1)
    rc, _ = B.run(d2)
    assert rc == 0, PP.last_error()
    for n in FIN_OUT:
        note("pool_finalize_bn vs bn_finalize", PP.err_ratio(got[n], host(o2[n])[:S * 256].reshape(S, 256).astype(np.float64), fref[n][1]))


# =====================================================================================================================================
# bn_bwd_finalize
# =====================================================================================================================================
def bwd_cpb(S, C, Q, part_Q, chunks):
    """kernels.h (BnBwdFinalize): 16 channels x 64 groups per block when few blocks face many partials, else 64 x 16."""
    return 16 if S * cdiv(C, 64) < 8 and cdiv(part_Q if part_Q > 0 else Q, S) * chunks >= 512 else 64


def build_bn_bwd(S, C, chunks, uniform, part_Q, win, tail=TAIL, seed=0):
    rng = np.random.default_rng(C + 10 * chunks + uniform + part_Q + seed)
    Q = len(win)
    P = (part_Q if part_Q > 0 else Q) * chunks
    wo = offsets(win)
    slot_rows = np.array([sum(win[q] for q in range(s, Q, S)) for s in range(S)])
    pslot = B.slot_of_partial(P, chunks, S)
    h = dict(part_a=f32(rng.standard_normal((P, C))), part_b=f32(rng.standard_normal((P, C)) * 3), gamma=f32(rng.standard_normal(C)),
             mean=f32(rng.standard_normal((S, C)) * 2), invstd=f32(0.2 + rng.random((S, C)) * 3), slots=pslot, slot_rows=slot_rows)
    dead = slot_rows[pslot] == 0
    h["part_a"][dead] = 0.0                                     # a slot with no row has no gradient either
    h["part_b"][dead] = 0.0
    d = B.new("bn_bwd_finalize", Q=Q, n_slots=S, C=C, chunks=chunks, uniform_rows=uniform, part_Q=part_Q)
    ins = {n: dev(h[n]) for n in ("part_a", "part_b", "gamma", "mean", "invstd")}
    if not uniform:
        ins["win_off"] = dev(wo)
    outs = dict(P1=out(S * C, tail), P2=out(S * C, tail), P3=out(S * C, tail), slot_ab=out(2 * S * C, tail))
    B.set_tensors(d, **ins, **outs)
    return d, h, ins, outs


def check_bn_bwd(h, outs, S, C, fam):
    ref = B.bn_bwd_finalize_ref(h["part_a"], h["part_b"], h["slots"], h["slot_rows"], h["gamma"], h["mean"], h["invstd"], S)
    for n in ("P1", "P2", "P3", "slot_ab"):
        got = written(outs[n], ref[n][0].size, n).reshape(ref[n][0].shape)
        note(f"{fam} {n}", B.worst(got, ref[n]))
    return ref


@pytest.mark.parametrize("part_Q", [0, 13])
@pytest.mark.parametrize("uniform", [0, 300])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("C", [128, 40])
def test_bn_bwd_finalize_64(C, chunks, uniform, part_Q):
    win = [300] * 7 if uniform else [5, 0, 700, 3, 0, 17, 512]           # ragged: slot 1 (windows 1 and 4) has no row
    assert bwd_cpb(3, C, len(win), part_Q, chunks) == 64
    d, h, ins, outs = build_bn_bwd(3, C, chunks, uniform, part_Q, win)
    launch(d, outs)
    check_bn_bwd(h, outs, 3, C, "bn_bwd_finalize<64>")
    if not uniform:
        assert h["slot_rows"][1] == 0
        P2, P3 = (host(outs[n])[:3 * C].reshape(3, C) for n in ("P2", "P3"))
        assert np.all(P2[1] == 0) and np.all(P3[1] == 0), "a slot with no row: P2 = P3 = 0"


def test_bn_bwd_finalize_16():
    win = [40, 7, 300, 5]
    assert bwd_cpb(1, 64, len(win), 600, 1) == 16 and bwd_cpb(1, 64, len(win), 511, 1) == 64
    d, h, ins, outs = build_bn_bwd(1, 64, 1, 0, 600, win)
    launch(d, outs)
    check_bn_bwd(h, outs, 1, 64, "bn_bwd_finalize<16>")


# =====================================================================================================================================
# fc_act, fc_act_pair, fc_bn_bwd, colsum
# =====================================================================================================================================
def build_fc_bn_bwd(c, tail=TAIL):
    S, per, C = c["n_slots"], c["per"], c["C"]
    d = B.new("fc_bn_bwd", n_slots=S, per=per, C=C)
    ins = {n: dev(c[n]) for n in ("z", "da", "scale", "shift", "mean", "invstd")}
    outs = dict(g=out(S * per * C, tail), slot_ab=out(2 * S * C, tail))
    B.set_tensors(d, **ins, **outs)
    return d, ins, outs


@pytest.mark.parametrize("C", B.FC_C)
@pytest.mark.parametrize("per", B.FC_PER)
def test_fc_bn_bwd(per, C):
    c = B.make_fc_bn_bwd(per, C)
    ref = B.fc_bn_bwd_ref(c["da"], c["z"], c["scale"], c["shift"], c["mean"], c["invstd"], 3, per)
    assert ref["sure"].all()
    d, ins, outs = build_fc_bn_bwd(c)
    launch(d, outs)
    note("fc_bn_bwd g", B.worst(written(outs["g"], 3 * per * C, "g").reshape(3 * per, C), ref["g"]))
    note("fc_bn_bwd slot_ab", B.worst(written(outs["slot_ab"], 6 * C, "slot_ab").reshape(3, C, 2), ref["slot_ab"]))
    ab = host(outs["slot_ab"])[:6 * C].reshape(3, C, 2)
    assert np.all(ab[:, 0, :] == 0), "a column the ReLU kills everywhere: da is ignored"


def build_fc_act(pair, tail=TAIL, rows=13, per=5, C=256, C1=128):
    rng = np.random.default_rng(rows + C)
    G = cdiv(rows, per)
    h = dict(z=f32(rng.standard_normal((rows, C))), scale=f32(rng.standard_normal((G, C))), shift=f32(rng.standard_normal((G, C))),
             z1=f32(rng.standard_normal((rows, C1))), s1=f32(rng.standard_normal((G, C1))), t1=f32(rng.standard_normal((G, C1))))
    d = B.new("fc_act_pair" if pair else "fc_act", rows=rows, per=per, C=C, C1=C1 if pair else 0)
    names = ("z", "scale", "shift", "z1", "s1", "t1") if pair else ("z", "scale", "shift")
    ins = {n: dev(h[n]) for n in names}
    outs = dict(act=out(rows * C, tail), **({"act1": out(rows * C1, tail)} if pair else {}))
    B.set_tensors(d, **ins, **outs)
    return d, h, ins, outs


def test_fc_act_and_pair():
    d, h, ins, outs = build_fc_act(True)
    launch(d, outs)
    rows, per = 13, 5
    a0 = written(outs["act"], rows * 256, "act").reshape(rows, 256)
    a1 = written(outs["act1"], rows * 128, "act1").reshape(rows, 128)
    note("fc_act", B.worst(a0, B.fc_act_ref(h["z"], h["scale"], h["shift"], per)["act"]))
    note("fc_act", B.worst(a1, B.fc_act_ref(h["z1"], h["s1"], h["t1"], per)["act"]))
    for z, s, t, C, want in (("z", "scale", "shift", 256, a0), ("z1", "s1", "t1", 128, a1)):
        d1 = B.new("fc_act", rows=rows, per=per, C=C)
        o = dict(act=out(rows * C))
        B.set_tensors(d1, z=ins[z], scale=ins[s], shift=ins[t], **o)
        launch(d1, o)
        assert np.array_equal(written(o["act"], rows * C, "act").view(np.int32), want.reshape(-1).view(np.int32)), "fc_act_pair = two fc_act calls, bitwise"


def build_colsum(rows, C, tail=TAIL):
    x = f32(np.random.default_rng(rows * 1000 + C).standard_normal((rows, C)))
    d = B.new("colsum", rows=rows, C=C)
    ins, outs = dict(src=dev(x)), dict(dst=out(C, tail))
    B.set_tensors(d, **ins, **outs)
    return d, x, ins, outs


@pytest.mark.parametrize("C", [1, 31, 32, 33, 256])
@pytest.mark.parametrize("rows", [1, 7, 8, 25, 32, 33, 1000])
def test_colsum(rows, C):
    d, x, ins, outs = build_colsum(rows, C)
    launch(d, outs)
    note("colsum", B.worst(written(outs["dst"], C, "dst"), B.colsum_ref(x)["out"]))


# =====================================================================================================================================
# reduce_windows, reduce_windows_multi, transpose64_slot_major, add_identity, fill_i32_ramp
# =====================================================================================================================================
def reduce_geometry(Q, rows, cols):
    ld_part, ld_dst = cols + 3, cols + 2
    stride = rows * ld_part + 5
    return ld_part, ld_dst, stride, (Q - 1) * stride + (rows - 1) * ld_part + cols, (rows - 1) * ld_dst + cols


def build_reduce(Q, rows, cols, accumulate, tail=TAIL):
    rng = np.random.default_rng(Q * 100 + rows * cols + accumulate)
    ld_part, ld_dst, stride, n_src, n_dst = reduce_geometry(Q, rows, cols)
    src = f32(rng.standard_normal(n_src))
    d = B.new("reduce_windows", Q=Q, rows=rows, cols=cols, ld_part=ld_part, ld_dst=ld_dst, accumulate=accumulate)
    d.stride = stride
    ins, outs = dict(src=dev(src)), dict(dst=out(n_dst, tail))
    dst0 = np.full(n_dst + tail, np.nan, dtype=np.float32)
    idx = (np.arange(rows)[:, None] * ld_dst + np.arange(cols)[None, :]).reshape(-1)
    dst0[idx] = rng.standard_normal(rows * cols)
    restore = None
    if accumulate:
        restore = dict(dst=dev(dst0))
        outs["dst"].copy_(restore["dst"])
    B.set_tensors(d, **ins, **outs)
    part = np.stack([np.stack([src[q * stride + r * ld_part:q * stride + r * ld_part + cols] for r in range(rows)]) for q in range(Q)])
    return d, ins, outs, restore, part, dst0[idx].reshape(rows, cols), idx


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,cols", [(3, 7), (5, 9)])
@pytest.mark.parametrize("Q", [1, 7, 8, 57, 64, 65, 121, 600])
def test_reduce_windows(Q, rows, cols, accumulate):
    assert (rows * cols) % 32 != 0
    d, ins, outs, restore, part, dst0, idx = build_reduce(Q, rows, cols, accumulate)
    launch(d, outs, restore)
    s = sentinel(outs["dst"])
    keep = np.ones(len(s), dtype=bool)
    keep[idx] = False
    assert not s[idx].any() and s[keep].all(), "dst: the padding columns of ld_dst and the tail stay untouched"
    got = host(outs["dst"])[idx].reshape(rows, cols)
    note("reduce_windows" + (" +=" if accumulate else ""), B.worst(got, B.reduce_ref(part, dst0 if accumulate else None)["dst"]))


MULTI = [(1, 3, 7), (7, 5, 9), (8, 1, 1), (57, 3, 7), (64, 2, 33), (65, 5, 9), (121, 1, 40), (600, 3, 7), (9, 64, 64), (2, 12, 3), (33, 7, 5), (12, 1, 31)]


def build_reduce_multi(n, tail=TAIL):
    items = (MULTI + MULTI[:1])[:n]
    rng = np.random.default_rng(n)
    d = B.new("reduce_windows_multi", n_items=n)
    po = do = 0
    geo = []
    for i, (Q, rows, cols) in enumerate(items):
        ld_part, ld_dst, stride, n_src, n_dst = reduce_geometry(Q, rows, cols)
        d.it_Q[i], d.it_rows[i], d.it_cols[i], d.it_ld_part[i], d.it_ld_dst[i] = Q, rows, cols, ld_part, ld_dst
        d.it_stride[i], d.it_part_off[i], d.it_dst_off[i] = stride, po, do
        geo.append((po, n_src, do, n_dst))
        po, do = po + n_src, do + n_dst
    src = f32(rng.standard_normal(po))
    ins, outs = dict(src=dev(src)), dict(dst=out(do, tail))
    B.set_tensors(d, **ins, **outs)
    return d, items, geo, src, ins, outs


def test_reduce_windows_multi():
    d, items, geo, src, ins, outs = build_reduce_multi(12)
    launch(d, outs)
    multi = bits(outs["dst"])
    for (Q, rows, cols), (po, n_src, do, n_dst) in zip(items, geo):
        ld_part, ld_dst, stride, _, _ = reduce_geometry(Q, rows, cols)
        d1 = B.new("reduce_windows", Q=Q, rows=rows, cols=cols, ld_part=ld_part, ld_dst=ld_dst, accumulate=0)
        d1.stride = stride
        o = dict(dst=out(n_dst, 0))
        B.set_tensors(d1, src=dev(src[po:po + n_src]), **o)
        rc, _ = B.run(d1)
        assert rc == 0, PP.last_error()
        assert torch.equal(bits(o["dst"]), multi[do:do + n_dst]), f"item {(Q, rows, cols)}: not the bits of the single launch (padding included)"
        idx = (np.arange(rows)[:, None] * ld_dst + np.arange(cols)[None, :]).reshape(-1)
        part = np.stack([np.stack([src[po + q * stride + r * ld_part:po + q * stride + r * ld_part + cols] for r in range(rows)]) for q in range(Q)])
        note("reduce_windows_multi", B.worst(host(o["dst"])[idx].reshape(rows, cols), B.reduce_ref(part)["dst"]))
    assert sentinel(outs["dst"])[geo[-1][2] + geo[-1][3]:].all()
    d, items, geo, src, ins, outs = build_reduce_multi(13)
    rc, names = B.run(d)
    assert rc == B.AMPNET_E_ARG and names == [] and "13 items" in PP.last_error(), (rc, PP.last_error())
    assert sentinel(outs["dst"]).all()


def build_transpose(chunks, by_workgroup, with_add, tail=TAIL, Q=12, S=3):
    rng = np.random.default_rng(chunks * 4 + by_workgroup * 2 + with_add)
    src = f32(rng.standard_normal((Q * chunks, 64, 64)))
    add = f32(rng.standard_normal((Q, 64, 64))) if with_add else None
    d = B.new("transpose64", Q=Q, n_slots=S, chunks=chunks, by_workgroup=by_workgroup)
    ins, outs = dict(src=dev(src), add=dev(add) if with_add else None), dict(dst=out(Q * 4096, tail))
    B.set_tensors(d, **ins, **outs)
    return d, src, add, ins, outs


@pytest.mark.parametrize("with_add", [0, 1])
@pytest.mark.parametrize("by_workgroup", [0, 1])
@pytest.mark.parametrize("chunks", [1, 3, 8, 9])
def test_transpose64(chunks, by_workgroup, with_add):
    d, src, add, ins, outs = build_transpose(chunks, by_workgroup, with_add)
    launch(d, outs)
    got = written(outs["dst"], 12 * 4096, "dst").reshape(12, 64, 64)
    note("transpose64", B.worst(got, B.transpose64_ref(src, 12, 3, chunks, by_workgroup, add)["dst"]))


def build_add_identity(k, tail=TAIL, Q=5):
    T = f32(np.random.default_rng(k).standard_normal(Q * k * k))
    d = B.new("add_identity", Q=Q, k=k)
    outs = dict(dst=out(Q * k * k, tail))
    restore = dict(dst=dev(np.concatenate([T, np.full(tail, np.nan, dtype=np.float32)])))
    outs["dst"].copy_(restore["dst"])
    B.set_tensors(d, **outs)
    return d, T, outs, restore


@pytest.mark.parametrize("k", [3, 64])
def test_add_identity(k):
    d, T, outs, restore = build_add_identity(k)
    launch(d, outs, restore)
    want = T.reshape(5, k, k) + np.eye(k, dtype=np.float32)[None]
    assert np.array_equal(written(outs["dst"], 5 * k * k, "T").reshape(5, k, k), want)


def build_ramp(n, step, tail=TAIL):
    d = B.new("fill_i32_ramp", rows=n, step=step)
    outs = dict(idst=out(n, tail, torch.int32))
    B.set_tensors(d, **outs)
    return d, outs


@pytest.mark.parametrize("n,step", [(1, 5), (256, 1), (257, 300), (1000, 4096)])
def test_fill_i32_ramp(n, step):
    d, outs = build_ramp(n, step)
    launch(d, outs)
    assert np.array_equal(written(outs["idst"], n, "ramp"), np.arange(n, dtype=np.int32) * step)


# =====================================================================================================================================
def test_probe_refuses_short_buffers():
    """A wrong test gets AMPNET_E_ARG, not an out-of-bounds access: every buffer of every op, one element short.  The descriptors are built
    with no spare element (tail 0), so each extent is exactly what the op touches; nothing is launched (the outputs keep their poison)."""
    cA = input_data("A", 1, 1, 0)
    kb, pb = pool_bn_case(57)
    pick = lambda r, *idx: tuple(r[i] for i in idx)            # (descriptor, inputs, outputs) of a builder's result
    builds = {
        "pw_input chunk": lambda: pick(build_input(cA, 1, 1, 0, "chunk", 0), 0, 1, 2),
        "pw_input persist": lambda: pick(build_input(cA, 1, 1, 1, "persist", 0), 0, 1, 2),
        "bn_finalize win_off": lambda: build_finalize(fin_case("ragged3", 40), 1, 0),
        "bn_finalize rows + merge_ws": lambda: build_finalize(fin_case("two_stage", 40), 1, 0),
        "bn_finalize_gathered": lambda: build_finalize(fin_case("gathered", 40), 1, 0),
        "bn_fold": lambda: pick(build_items("bn_fold", 3, 1, 0), 0, 2, 3),
        "bn_running_update": lambda: pick(build_items("bn_running_update", 3, 3, 0), 0, 2, 3),
        "bn_param_grads": lambda: pick(build_items("bn_param_grads", 3, 3, 0), 0, 2, 3),
        "pool_finalize": lambda: build_pool(pool_case(3, 40), f32(np.ones((3, 40))), f32(np.zeros((3, 40))), 1, 1, 0),
        "pool_finalize bn": lambda: build_pool_bn(kb, pb, 0),
        "bn_bwd_finalize": lambda: pick(build_bn_bwd(3, 40, 3, 0, 13, [5, 0, 700, 3, 0, 17, 512], 0), 0, 2, 3),
        "fc_bn_bwd": lambda: build_fc_bn_bwd(B.make_fc_bn_bwd(8, 40), 0),
        "fc_act": lambda: pick(build_fc_act(False, 0), 0, 2, 3),
        "fc_act_pair": lambda: pick(build_fc_act(True, 0), 0, 2, 3),
        "colsum": lambda: pick(build_colsum(7, 33, 0), 0, 2, 3),
        "reduce_windows": lambda: pick(build_reduce(9, 3, 7, 0, 0), 0, 1, 2),
        "reduce_windows_multi": lambda: pick(build_reduce_multi(12, 0), 0, 4, 5),
        "transpose64": lambda: pick(build_transpose(3, 1, 1, 0), 0, 3, 4),
        "add_identity": lambda: (lambda r: (r[0], {}, r[2]))(build_add_identity(3, 0)),
        "fill_i32_ramp": lambda: (lambda r: (r[0], {}, r[1]))(build_ramp(9, 2, 0)),
    }
    assert {B.OPS[w.split()[0]] for w in builds} == set(B.OPS.values()), "an op without a refusal case"
    n_checked = 0
    for what, make in builds.items():
        d, ins, outs = make()
        names = [n for n, t in {**ins, **outs}.items() if t is not None]
        assert names
        before = {n: bits(t).clone() for n, t in outs.items() if t is not None}
        for n in names:
            full = getattr(d, n + "_n")
            assert full == {**ins, **outs}[n].numel(), (what, n)
            setattr(d, n + "_n", full - 1)
            rc, launched = B.run(d)
            assert rc == B.AMPNET_E_ARG and launched == [], f"{what}: {n} one element short was not refused ({rc}, {PP.last_error()})"
            setattr(d, n + "_n", full)
            n_checked += 1
        assert all(torch.equal(before[n], bits(outs[n])) for n in before), f"{what}: a refused call wrote"
        rc, _ = B.run(d)                               # and the descriptor itself is a valid one
        assert rc == 0, (what, PP.last_error())
    assert n_checked >= 100
