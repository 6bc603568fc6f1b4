"""The bf16 side of tests/pw_probe.py, without a GPU: bf16_rne is held bit-equal to torch's float32 -> bfloat16 (random data, exact ties,
one fp32 ulp either side of a tie); the rounded-operand reference gemm_ref(operands="bf16") equals the fp32 one where every operand is
already a bf16 value; the ambiguity mask and widening are zero without a prologue and mark exactly the prologue outputs within 2^-22 |v| of
a rounding midpoint; bf16_bracket rejects a truncated store.

Negative controls, on the c128_128 data of tests/test_pw_layers_gpu.py: a simulated correct kernel (the float64 contract value rounded once
to fp32 = the accumulator, stored round-to-nearest-even, statistics of the accumulator) passes the tier-2 comparison; the same with a
TRUNCATING store, with statistics of the STORED value, or with a truncated weight image lands outside the tier-2 bar -- and inside the
tier-1 (project) bar, which separates none of them."""
import ctypes

import numpy as np
import torch

import pw_probe as PP
import test_pw_layers_gpu as T


def torch_bf16(x32):
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).bfloat16().float().numpy().astype(np.float64)


def trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (toward zero)."""
    return (np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def test_probe_mirror_appends_the_bf16_flags():
    """a_bf16 / z_bf16 are the last two fields; nothing before them moved (pfin_out_n ended the descriptor before)."""
    P = PP.PwGemmProbe
    assert P.a_bf16.offset == P.pfin_out_n.offset + 8 and P.z_bf16.offset == P.a_bf16.offset + 4
    assert ctypes.sizeof(P) == P.z_bf16.offset + 4 and ctypes.sizeof(P) % 8 == 0
    # the word that says whether they are there is the former pad0 (0 in every caller of the shorter descriptor); this mirror sets it
    assert P.tail.offset == P.pfin_parts.offset + 4 and P.pfin_gamma.offset == P.tail.offset + 4 and P().tail == 1


def test_bf16_rne_is_torch_bfloat16():
    g = np.random.default_rng(7)
    x = (g.standard_normal(1 << 18) * np.exp2(g.integers(-20, 21, 1 << 18))).astype(np.float32)
    assert np.array_equal(PP.bf16_rne(x.astype(np.float64)), torch_bf16(x))
    # exact ties between two neighbouring bf16 values (both parities of the lower one), and one fp32 ulp either side
    lo = torch_bf16(x[:4096])
    lo = lo[lo != 0.0]
    tie = (lo + np.sign(lo) * 0.5 * PP.ulp_bf16(lo)).astype(np.float32)
    assert np.array_equal(tie.astype(np.float64), lo + np.sign(lo) * 0.5 * PP.ulp_bf16(lo)), "a tie is an fp32 value"
    bits = lo.astype(np.float32).view(np.uint32) >> 16
    assert (bits & 1).min() == 0 and (bits & 1).max() == 1
    for v in (tie, np.nextafter(tie, np.float32(np.inf)), np.nextafter(tie, np.float32(-np.inf))):
        assert np.array_equal(PP.bf16_rne(v.astype(np.float64)), torch_bf16(v))
    r = PP.bf16_rne(tie.astype(np.float64))
    assert np.all((r.astype(np.float32).view(np.uint32) >> 16) & 1 == 0), "ties go to the even neighbour"
    assert np.array_equal(PP.bf16_rne(r), r) and PP.bf16_rne(0.0) == 0.0


def bf16_operands(g, rows, cin, cout):
    A = torch_bf16(g.standard_normal((rows, cin)))
    W = torch_bf16(g.uniform(-1, 1, (cout, cin)) / 8)
    return A, W


def test_rounded_reference_equals_the_fp32_one_on_bf16_operands():
    g = np.random.default_rng(11)
    wo = T.offsets([5, 1, 33, 12])
    A, W = bf16_operands(g, int(wo[-1]), 64, 40)
    bias = g.uniform(-0.5, 0.5, 40)
    Z, M = PP.gemm_ref(A, 64, 40, W, wo, 2, bias=bias, identity_k=3)
    Zr, Mr, amb = PP.gemm_ref(A, 64, 40, W, wo, 2, bias=bias, identity_k=3, operands="bf16")
    assert np.array_equal(Z, Zr) and np.array_equal(M, Mr)
    assert not amb["mask"].any() and not amb["wid"].any() and amb["share"] == 0.0        # no prologue: nothing is ambiguous
    # a prologue whose output is a bf16 value again (s = 1 or -1, t = 0), per-window weights, a per-window bias
    Wp = torch_bf16(g.uniform(-1, 1, (4, 64, 40)) / 8)
    bw = g.uniform(-0.5, 0.5, (4, 40))
    pro = (np.where(g.random((2, 64)) < 0.3, -1.0, 1.0), np.zeros((2, 64)))
    kw = dict(pro=pro, bias=bw, bias_win_stride=40, w_win_stride=64 * 40, slot_major=1)
    Z, M = PP.gemm_ref(A, 64, 40, Wp, wo, 2, **kw)
    Zr, Mr, amb = PP.gemm_ref(A, 64, 40, Wp, wo, 2, operands="bf16", **kw)
    assert np.array_equal(Z, Zr) and np.all(Mr <= M)
    assert not amb["mask"].any() and not amb["wid"].any()                               # bf16 values are no midpoints


def test_ambiguity_mask_and_widening():
    g = np.random.default_rng(13)
    b = torch_bf16(np.abs(g.standard_normal(512)) + 0.01)
    mid = b + 0.5 * PP.ulp_bf16(b)
    for f in (0.0, 2.0 ** -23, -2.0 ** -23):
        assert PP.ambiguous_bf16(mid * (1.0 + f)).all()
    for f in (2.0 ** -20, -2.0 ** -20):
        assert not PP.ambiguous_bf16(mid * (1.0 + f)).any()
    assert not PP.ambiguous_bf16(np.array([0.0, -0.75])).any()
    # one ambiguous element in a row moves each output by one bf16 step of it times the rounded weight
    s, t = np.ones((1, 64)), np.zeros((1, 64))
    A = torch_bf16(np.abs(g.standard_normal((3, 64))) + 0.5)
    A[1, 17] = 1.00390625                                         # 1 + 2^-8: the midpoint between 1 and 1 + 2^-7
    W = g.uniform(-1, 1, (40, 64)) / 8
    Zr, Mr, amb = PP.gemm_ref(A, 64, 40, W, T.offsets([3]), 1, pro=(s, t), operands="bf16")
    want = np.zeros((3, 64), dtype=bool)
    want[1, 17] = True
    assert np.array_equal(amb["mask"], want)
    wid = np.zeros((3, 40))
    wid[1] = 2.0 ** -7 * np.abs(PP.bf16_rne(W[:, 17]))
    assert np.array_equal(amb["wid"], wid) and amb["share"] == 1.0 / (3 * 64)
    assert np.array_equal(amb["wid"], PP.ambiguity_widening(amb["mask"], amb["v"], PP.bf16_rne(W).T))
    # on random prologue outputs the share is the window over the midpoint spacing: 2^-14 .. 2^-13
    v = np.abs(g.standard_normal(1 << 22)) * g.uniform(0.5, 1.5, 1 << 22)
    share = PP.ambiguous_bf16(v).mean()
    print(f"[pw refs] ambiguous share of {v.size} random prologue outputs: {share:.3e}")
    assert 2.0 ** -15 < share < 2.0 ** -12


def test_bracket_rejects_a_truncated_store():
    z64 = (1.0 + 2.0 ** -7) * (1.0 - 2.0 ** -12)                    # just below the bf16 value 1 + 2^-7: it rounds up, truncation gives 1
    lo, hi = PP.bf16_bracket(z64, 2.0 ** -20)
    assert lo == hi == 1.0 + 2.0 ** -7
    assert trunc_bf16(np.float32(z64)) == 1.0 < lo
    lo, hi = PP.bf16_bracket(1.0 + 2.0 ** -8, 2.0 ** -20)          # the bar straddles a midpoint: both neighbours are right
    assert (lo, hi) == (1.0, 1.0 + 2.0 ** -7)
    assert T.bracket_ratio(np.array([1.0 + 2.0 ** -7]), np.array([z64]), np.array([2.0 ** -20])) == 0.0625
    assert T.bracket_ratio(np.array([1.0]), np.array([z64]), np.array([2.0 ** -20])) == 2.0


def slot_stats_ratio(Zs, Z64r, Mr, slot, S, cin):
    """worst error / moment_bars(eps = 2^-24) of the per-slot mean and variance of Zs against those of the unrounded contract value."""
    worst = 0.0
    for sl in range(S):
        r = slot == sl
        mu, var, bmean, bvar = PP.moment_bars(Z64r[r], Mr[r], cin, PP.EPS32)
        z = Zs[r]
        worst = max(worst, PP.err_ratio(z.mean(0), mu, bmean), PP.err_ratio(((z - z.mean(0)) ** 2).mean(0), var, bvar))
    return worst


def test_negative_controls_on_the_c128_128_data():
    c = T.FWD["c128_128"]
    cin, cout, S = c["cin"], c["cout"], c["S"]
    host = T.gemm_host(c, 1234 + len("c128_128"), a_bf16=1)
    Z64, M = PP.gemm_ref(host["A"], cin, cout, host["W"], host["win_off"], S, pro=host["pro"])
    Z64r, Mr, amb = PP.gemm_ref(host["A"], cin, cout, host["W"], host["win_off"], S, pro=host["pro"], operands="bf16")
    print(f"[pw refs] c128_128: ambiguous share {amb['share']:.3e}, largest widening / bar "
          f"{np.max(amb['wid'] / PP.bar(Mr, Z64r, cin)):.1f}")
    assert 0.0 < amb["share"] < 2.0 ** -10
    b2 = PP.bar(Mr, Z64r, cin, PP.EPS32) + amb["wid"]
    b1 = PP.bar(M, Z64, cin, PP.EPS16) + 2 * PP.EPS16 * np.abs(Z64)
    slot = PP.win_of_rows(host["win_off"]) % S
    acc = Z64r.astype(np.float32)                                   # a correct kernel's accumulator: the contract value, rounded once
    good, trunc = torch_bf16(acc), trunc_bf16(acc)
    # the correct kernel passes both tiers
    assert T.bracket_ratio(good, Z64r, b2) <= 1.0 and PP.err_ratio(good, Z64, b1) <= 1.0
    assert slot_stats_ratio(acc.astype(np.float64), Z64r, Mr, slot, S, cin) <= 1.0
    # a truncating store: outside tier 2, inside tier 1
    assert T.bracket_ratio(trunc, Z64r, b2) == 2.0
    outside = np.mean((trunc < PP.bf16_bracket(Z64r, b2)[0]) | (trunc > PP.bf16_bracket(Z64r, b2)[1]))
    r1 = PP.err_ratio(trunc, Z64, b1)
    assert r1 <= 1.0
    # statistics of the stored (rounded) value instead of the accumulator: outside tier 2, inside tier 1
    r2 = slot_stats_ratio(good, Z64r, Mr, slot, S, cin)
    r1s = 0.0
    for sl in range(S):
        r = slot == sl
        mu, var, bmean, bvar = PP.moment_bars(Z64[r], M[r], cin, PP.EPS16)
        r1s = max(r1s, PP.err_ratio(good[r].mean(0), mu, bmean), PP.err_ratio(((good[r] - good[r].mean(0)) ** 2).mean(0), var, bvar))
    assert r2 > 1.0 and r1s <= 1.0
    # a wrong weight image (truncated instead of rounded): outside tier 2, inside tier 1
    u = PP.bf16_rne(np.maximum(host["A"].astype(np.float64) * host["pro"][0][slot] + host["pro"][1][slot], 0.0))
    wrong = torch_bf16((u @ trunc_bf16(host["W"]).T).astype(np.float32))
    r3, r13 = T.bracket_ratio(wrong, Z64r, b2), PP.err_ratio(wrong, Z64, b1)
    assert r3 == 2.0 and r13 <= 1.0
    print(f"[pw refs] negative controls: truncating store outside the bracket at {outside:.1%} of the elements (tier 1: {r1:.3f} of its bar); "
          f"statistics of the stored z at {r2:.1f} x the tier-2 bar (tier 1: {r1s:.3f}); truncated weights: tier 1 {r13:.3f}")
