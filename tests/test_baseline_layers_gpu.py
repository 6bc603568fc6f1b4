"""Layer-local float64 parity of the baseline single-window PointNet's kernels (csrc/baseline.hip: 5 bl_* kernels; csrc/baseline_train.hip: 20
bt_* kernels and the composed fwd_layer / bwd_layer).

Each case is ONE launch through ampnet_probe_baseline_f32 (include/ampnet_hip.h, "test hooks"), which goes through the launch wrappers of
csrc/baseline.h that the product entry points call, on inputs of tests/baseline_probe.py, and holds every output to the float64 restatement
there at the bars of that module's docstring (none derived from a kernel).  Every case also checks: outputs pre-filled with NaN (-7 for int32)
with 8 tail elements are finite where the contract writes and keep their sentinel bits elsewhere; inputs the contract does not read hold NaN; a
second run on re-poisoned outputs (in-place operands restored) is bitwise identical; the probe recorded the intended kernel.

Cases and the branch each is for
  bt_bias       bias / add / both; C in {1, 5, 64, 100}; M C never a multiple of 256 (the `i >= n` lanes); per in {1, 7, M}.  One addend: bitwise.
  bt_stats      M in {2, 3, 4, 5, 16, 513} (fewer rows than the 4 row groups, one past, many) x C in {4, 64, 65, 130} (`c >= C` lanes of the last
                block); column 0 with mean^2 >> variance, column 1 constant (invstd = 1 / sqrt(eps)); rm / rv updated in place from non-trivial
                values (unbiased variance).  bt_running_stats, bt_bn_act (ReLU decision rule) on the same C set.
  bt_bn_bwd     M in {2, 5, 513} x C in {40, 64, 65}; dead rows carry da; `apply` on the dg / dbe of the float64 reference (an error in `sums`
                cannot mask one in `apply`), and the pair chained on the kernel's own sums.
  rowmax        N in {1, 2, 3, 4, 5, 7, 513} x C in {1, 64, 65, 256} x B in {1, 3}: values exact, arg == np.argmax (first maximum); all-zero
                columns; small-integer ties; the maximum at rows 1 and 4 (low row in group 1, higher in group 0) and at rows 4 and 5 (the other
                way round); bl_rowmax bitwise the bt_ values.  bt_pool_scatter on a zeroed d_a, B C in {1, 255, 256, 257, 3 x 65}: exact.
  mix           k in {2, 3}, R in {1, 255, 256, 257} with N = 100 (not dividing 256); columns k .. 8 bitwise copies; bl_mix bitwise bt_mix.
                bt_mix_bwd k in {2, 3}, B = 3, N in {1, 255, 256, 257, 600} (K = 1: double sums).  bt_segsum N in {1, 3, 4, 5, 513} x C in
                {1, 64, 65}, B = 3.
  logits        bt_logits both ways and bl_logits exact, the round trip the identity, N = 1 and C = 1 included.  bt_fill, bt_add n in {1, 255,
                256, 257}: exact / one rounding.  bt_dropout p in {0.3, 0.5, 0.999}: the oracle's keep_mask, kept values the fp32 product, and
                the in-place form (out == a) the classification backward uses.
  log_softmax   B in {1, 63, 64, 65} x C in {1, 2, 40, 64} x logits shifted by {0, +80, -80}; exp(out) sums to 1 within the bar; C = 65 refused.
  bl_fold / bl_affine   bias x BatchNorm present or NULL; add / per; relu 0 / 1 with the decision rule.
  fwd_layer / bwd_layer   composition only: bit for bit the same kernels one at a time through the probe with the GEMMs through
                ampnet_small_gemm_f32 (and colsum through ampnet_probe_bn_f32): K in {2, 3, 9, 64} at lda = 9 / 64, w0 = 24 with ldw = 88,
                accumulate 0 / 1 on dA, dA NULL, a layer without BatchNorm, train and running statistics.
  refusals      every buffer of every op one element short, C = 65 for the log_softmax pair, a pooling index outside its window, k = 4: AMPNET_E_ARG
                with every output still at its sentinel; the backward entry points refuse the shapes their train forward refuses.

Observed worst error/bar on the MI355X (the teardown lines of this file's run; 340 cases, 3.3 s): bt_bias 0.16, bt_add 0.10 (and bitwise the one
fp32 addition).  bt_stats mean 0.10, invstd 0.23, rm 0.13, rv 0.10; bt_running_stats invstd 0.13; bt_bn_act 0.24.  bt_bn_bwd_sums dg 0.19, dbe 0.10;
bt_bn_bwd_apply 0.31 on the reference's sums and 0.31 chained.  bt_mix 0.14, bl_mix 0.14 (bitwise equal); bt_mix_bwd 0.08; bt_segsum 0.10.
bt_log_softmax 0.32, bt_log_softmax_bwd 0.49 (head_probe's EXP_ULP = 4, no new constant).  bl_fold scale 0.17, shift 0.11; bl_affine 0.16.
fwd_layer z 0.10, bwd_layer dW 0.10, dA 0.11 against float64 (beside the bit-for-bit composition).  rowmax, pool_scatter, logits, fill and dropout
are exact.  Every family is under 1.0; no kernel was found wrong.
Scratch-build mutations of csrc/baseline_train.hip (not committed), all five in one library, 101 of the 340 cases failing:
(a) `zh * dg[c] / (M - 1)` in bt_bn_bwd_apply_kernel: all 9 test_bt_bn_bwd cases; (b) the running variance from m2 / M in bt_stats_kernel: all 24
test_bt_stats_and_bn_act cases; (c) the cross-group tie rule dropped from bt_rowmax_kernel (`rv[k] > m` alone): 46 of the `ties` and `low_late` cases
of test_rowmax with N >= 5 (`low_first` passes, as it must: group 0 holds the lower row there); (d) i and j swapped in bt_mix_bwd_kernel: all 10
test_bt_mix_bwd cases; (e) row group 3 dropped from bt_segsum_kernel's final sum: the 12 test_bt_segsum cases with N >= 3.
"""
import ctypes

import numpy as np
import pytest
import torch

import bn_probe as BN
import baseline_probe as P
import pw_probe as PP

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
TAIL = 8
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[baseline layers] worst error/bar {k}: {WORST[k]:.4f}")


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def nanbuf(n):
    """n elements the contract may write + TAIL it must not."""
    return torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")


def ibuf(n):
    return torch.full((n + TAIL,), -7, dtype=torch.int32, device="cuda")


def unread(n):
    """an input the contract does not read"""
    return torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device="cuda")


def is_sentinel(t):
    if t.dtype == torch.int32:
        return bool((t == -7).all())
    return bool((t.detach().cpu().view(torch.int32) == NAN_BITS).all())


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def inplace(x):
    """a device copy of x followed by a NaN tail, and its pristine clone"""
    t = torch.cat([dev(P.f32(x)).reshape(-1), torch.full((TAIL,), float("nan"), device="cuda")])
    return t, t.clone()


def host(t, n=None, shape=None):
    a = t.detach().cpu().numpy()
    a = a if n is None else a[:n]
    return a if shape is None else a.reshape(shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def launch(d, outs, restore=()):
    """run, check the recorded kernel, re-poison the outputs (and restore the in-place operands), run again: bitwise equal.  outs: {name: (tensor,
    written elements, or None for an output written with gaps, which the caller checks)}; restore: [(tensor, original)].  Checks finite where
    written and the tail's sentinel.  The buffers hold the second run."""
    rc, names = P.run(d)
    assert rc == 0, PP.last_error()
    if d.op not in P.COMPOSED:
        assert names == [P.KERNEL[d.op]], (names, P.KERNEL[d.op])
    every = list(outs.items()) + [(f"in-place {i}", (t, t.numel() - TAIL)) for i, (t, _) in enumerate(restore)]
    first = {k: v.detach().cpu().clone() for k, (v, _) in every}
    for v, _ in outs.values():
        v.fill_(-7 if v.dtype == torch.int32 else float("nan"))
    for t, orig in restore:
        t.copy_(orig)
    rc, _ = P.run(d)
    assert rc == 0, PP.last_error()
    for k, (v, n) in every:
        now = v.detach().cpu()
        assert torch.equal(first[k].view(torch.int32), now.view(torch.int32)), f"{k}: second run differs bitwise"
        if n is None:
            continue
        assert v.dtype == torch.int32 or bool(torch.isfinite(v[:n]).all()), f"{k}: non-finite where the contract writes"
        assert is_sentinel(v[n:]), f"{k}: written past its extent"


# ---- bt_bias, bt_add, bt_fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,per,kind", P.BIAS_CASES)
def test_bt_bias(M, C, per, kind):
    c = P.make_bias(M, C, per, kind)
    r = P.bias_ref(c["z"], c["bias"], c["add"], per)
    z, z0 = inplace(c["z"])
    d = P.new("bt_bias", M=M, C=C, per=per)
    P.set_tensors(d, z=z, bias=None if c["bias"] is None else dev(c["bias"]), add=None if c["add"] is None else dev(c["add"]))
    launch(d, {}, restore=[(z, z0)])
    got = host(z, M * C, (M, C))
    assert note("bt_bias", P.worst(got, r["z"])) <= 1.0
    if kind != "both":
        assert np.array_equal(bits(got), bits(P.bias_ref(c["z"], c["bias"], c["add"], per, dt=np.float32)["z"][0])), "one addend is one rounding"


@pytest.mark.parametrize("n", P.FLAT_N)
def test_bt_fill_and_add(n):
    z = nanbuf(n)
    d = P.new("bt_fill", n=n)
    d.value = 0.37
    P.set_tensors(d, z=z)
    launch(d, dict(z=(z, n)))
    assert np.all(host(z, n) == np.float32(0.37))
    g = np.random.default_rng(n)
    y, x = P.f32(g.standard_normal(n)), P.f32(g.standard_normal(n))
    yt, y0 = inplace(y)
    d = P.new("bt_add", n=n)
    P.set_tensors(d, z=yt, x=dev(x))
    launch(d, {}, restore=[(yt, y0)])
    assert np.array_equal(bits(host(yt, n)), bits(y + x)), "one fp32 addition"
    note("bt_add", P.worst(host(yt, n), P.add_ref(y, x)["z"]))


# ---- BatchNorm forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", P.STATS_C)
@pytest.mark.parametrize("M", P.STATS_M)
def test_bt_stats_and_bn_act(M, C):
    c = P.make_stats(M, C)
    r = P.stats_ref(c["z"], c["rm"], c["rv"])
    mean, invstd = nanbuf(C), nanbuf(C)
    (rm, rm0), (rv, rv0) = inplace(c["rm"]), inplace(c["rv"])
    zt = dev(c["z"])
    d = P.new("bt_stats", M=M, C=C)
    P.set_tensors(d, z=zt, mean=mean, invstd=invstd, rm=rm, rv=rv)
    launch(d, dict(mean=(mean, C), invstd=(invstd, C)), restore=[(rm, rm0), (rv, rv0)])
    for k, t in (("mean", mean), ("invstd", invstd), ("rm", rm), ("rv", rv)):
        assert note(f"bt_stats {k}", P.worst(host(t, C), r[k])) <= 1.0, k
    assert host(invstd, C)[1] == np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5)))), "the constant column: variance exactly 0"
    assert host(mean, C)[1] == np.float32(2.5)
    # bt_bn_act on the kernel's own statistics
    m_, i_ = host(mean, C).copy(), host(invstd, C).copy()
    ra = P.bn_act_ref(c["z"], m_, i_, c["gamma"], c["beta"])
    a = nanbuf(M * C)
    d = P.new("bt_bn_act", M=M, C=C)
    P.set_tensors(d, z=zt, mean=mean[:C].clone(), invstd=invstd[:C].clone(), gamma=dev(c["gamma"]), beta=dev(c["beta"]), a=a)
    launch(d, dict(a=(a, M * C)))
    assert (~ra["sure"]).sum() <= 0.01 * M * C
    got = host(a, M * C, (M, C))
    assert note("bt_bn_act", P.worst_relu(got, ra["pre"], ra["sure"])) <= 1.0
    assert (got >= 0).all()


@pytest.mark.parametrize("C", P.STATS_C)
def test_bt_running_stats(C):
    c = P.make_stats(5, C)
    r = P.running_stats_ref(c["rm"], c["rv"])
    mean, invstd = nanbuf(C), nanbuf(C)
    rm, rv = dev(c["rm"]), dev(c["rv"])
    d = P.new("bt_running_stats", C=C)
    P.set_tensors(d, rm=rm, rv=rv, mean=mean, invstd=invstd)
    launch(d, dict(mean=(mean, C), invstd=(invstd, C)))
    assert np.array_equal(bits(host(mean, C)), bits(c["rm"])), "the mean is the running mean"
    assert note("bt_running_stats invstd", P.worst(host(invstd, C), r["invstd"])) <= 1.0
    assert np.array_equal(bits(host(rm)), bits(c["rm"])) and np.array_equal(bits(host(rv)), bits(c["rv"])), "eval mode touched the running statistics"


# ---- BatchNorm + ReLU backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", P.BWD_C)
@pytest.mark.parametrize("M", P.BWD_M)
def test_bt_bn_bwd(M, C):
    c = P.make_bn_bwd(M, C)
    args = (c["da"], c["a"], c["z"], c["mean"], c["invstd"])
    rs = P.bn_bwd_sums_ref(*args)
    common = dict(a=dev(c["a"]), z=dev(c["z"]), mean=dev(c["mean"]), invstd=dev(c["invstd"]))
    dg, dbe = nanbuf(C), nanbuf(C)
    d = P.new("bt_bn_bwd_sums", M=M, C=C)
    P.set_tensors(d, da=dev(c["da"]), dg=dg, dbe=dbe, **common)
    launch(d, dict(dg=(dg, C), dbe=(dbe, C)))
    assert note("bt_bn_bwd_sums dg", P.worst(host(dg, C), rs["dg"])) <= 1.0
    assert note("bt_bn_bwd_sums dbe", P.worst(host(dbe, C), rs["dbe"])) <= 1.0
    # apply on the reference's sums, then on the kernel's own (the chained pair)
    for name, dg_h, dbe_h in (("reference sums", P.f32(rs["dg"][0]), P.f32(rs["dbe"][0])), ("chained", host(dg, C).copy(), host(dbe, C).copy())):
        ra = P.bn_bwd_apply_ref(*args, c["gamma"], dg_h, dbe_h)
        da, da0 = inplace(c["da"])
        d = P.new("bt_bn_bwd_apply", M=M, C=C)
        P.set_tensors(d, da=da, gamma=dev(c["gamma"]), dg=dev(dg_h), dbe=dev(dbe_h), **common)
        launch(d, {}, restore=[(da, da0)])
        assert note(f"bt_bn_bwd_apply ({name})", P.worst(host(da, M * C, (M, C)), ra["dz"])) <= 1.0, name


# ---- pooling ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C,kind", P.POOL_CASES)
def test_rowmax(B, N, C, kind):
    a = P.make_pool(B, N, C, kind)
    r = P.rowmax_ref(a, B, N, C)
    at = dev(a)
    out, arg, out2 = nanbuf(B * C), ibuf(B * C), nanbuf(B * C)
    d = P.new("bt_rowmax", B=B, N=N, C=C)
    P.set_tensors(d, a=at, out=out, arg=arg)
    launch(d, dict(out=(out, B * C), arg=(arg, B * C)))
    assert np.array_equal(bits(host(out, B * C, (B, C))), bits(r["out"])), "the maximum is exact"
    assert np.array_equal(host(arg, B * C, (B, C)), r["arg"]), "arg is the FIRST maximum"
    d = P.new("bl_rowmax", B=B, N=N, C=C)
    P.set_tensors(d, a=at, out=out2, arg=None)
    launch(d, dict(out=(out2, B * C)))
    assert np.array_equal(bits(host(out2, B * C)), bits(host(out, B * C))), "bl_rowmax differs from bt_rowmax"


@pytest.mark.parametrize("B,C", P.SCATTER_BC)
def test_bt_pool_scatter(B, C):
    N = 7
    g = np.random.default_rng(B * 1000 + C)
    arg = g.integers(0, N, (B, C)).astype(np.int32)
    arg.reshape(-1)[0], arg.reshape(-1)[-1] = N - 1, 0
    dp = P.f32(g.standard_normal((B, C)) + 3.0)
    n = B * N * C
    da = torch.cat([torch.zeros(n, device="cuda"), torch.full((TAIL,), float("nan"), device="cuda")])
    d = P.new("bt_pool_scatter", B=B, N=N, C=C)
    P.set_tensors(d, x=dev(dp), arg=dev(arg), a=da)
    launch(d, {}, restore=[(da, da.clone())])
    assert np.array_equal(bits(host(da, n, (B, N, C))), bits(P.pool_scatter_ref(dp, arg, B, N, C))), "exact, every other element still +0"


# ---- the mix, its backward, the window sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", P.MIX_R)
@pytest.mark.parametrize("k", P.MIX_K)
def test_mix(k, R):
    N = 100
    c = P.make_mix(R, N, k)
    r = P.mix_ref(c["x"], c["T"], N, k)
    x, T = dev(c["x"]), dev(c["T"])
    got = {}
    for op in ("bt_mix", "bl_mix"):
        out = nanbuf(R * 9)
        d = P.new(op, M=R, N=N, k=k)
        P.set_tensors(d, x=x, T=T, out=out)
        launch(d, dict(out=(out, R * 9)))
        got[op] = host(out, R * 9, (R, 9)).copy()
        assert note(op, P.worst(got[op][:, :k], r["head"])) <= 1.0
        assert np.array_equal(bits(got[op][:, k:]), bits(c["x"][:, k:])), "columns k .. 8 are copies"
    assert np.array_equal(bits(got["bt_mix"]), bits(got["bl_mix"])), "the two kernels differ"


@pytest.mark.parametrize("N", P.MIX_BWD_N)
@pytest.mark.parametrize("k", P.MIX_K)
def test_bt_mix_bwd(k, N):
    B = 3
    c = P.make_mix(B * N, N, k, seed=5)
    dx = P.f32(np.random.default_rng(N + k).standard_normal((B * N, 9)))
    dx[:, k:] = np.nan                                                       # columns the contract does not read
    xin = c["x"].copy()
    xin[:, k:] = np.nan
    r = P.mix_bwd_ref(np.nan_to_num(xin), np.nan_to_num(dx), B, N, k)
    out = nanbuf(B * k * k)
    d = P.new("bt_mix_bwd", B=B, N=N, k=k)
    P.set_tensors(d, x=dev(xin), da=dev(dx), out=out)
    launch(d, dict(out=(out, B * k * k)))
    assert note("bt_mix_bwd", P.worst(host(out, B * k * k, (B, k, k)), r["dT"])) <= 1.0


@pytest.mark.parametrize("C", P.SEG_C)
@pytest.mark.parametrize("N", P.SEG_N)
def test_bt_segsum(N, C):
    B = 3
    dz = P.f32(np.random.default_rng(N * 100 + C).standard_normal((B * N, C)))
    out = nanbuf(B * C)
    d = P.new("bt_segsum", B=B, N=N, C=C)
    P.set_tensors(d, da=dev(dz), out=out)
    launch(d, dict(out=(out, B * C)))
    assert note("bt_segsum", P.worst(host(out, B * C, (B, C)), P.segsum_ref(dz, B, N, C)["out"])) <= 1.0


# ---- transposes, dropout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", P.LOGITS_BNC)
def test_logits_both_ways(B, N, C):
    n = B * N * C
    z = P.f32(np.random.default_rng(n).standard_normal((B * N, C)))
    want = P.logits_ref(z, B, N, C)
    zt = dev(z)
    for op in ("bt_logits", "bl_logits"):
        out = nanbuf(n)
        d = P.new(op, B=B, N=N, C=C)
        P.set_tensors(d, z=zt, out=out)
        launch(d, dict(out=(out, n)))
        assert np.array_equal(bits(host(out, n)), bits(want.reshape(-1))), op
    back = nanbuf(n)
    d = P.new("bt_logits_to_rows", B=B, N=N, C=C)
    P.set_tensors(d, z=back, out=dev(want))
    launch(d, dict(z=(back, n)))
    assert np.array_equal(bits(host(back, n)), bits(z.reshape(-1))), "the round trip is the identity"


@pytest.mark.parametrize("p", P.DROP_P)
@pytest.mark.parametrize("n", (1, 257, 4099))
def test_bt_dropout(n, p):
    seed = 1234 + n
    a = P.f32(np.random.default_rng(n).standard_normal(n) + 0.1)
    r = P.dropout_ref(a, seed, p)
    out = nanbuf(n)
    d = P.new("bt_dropout", n=n)
    d.drop_p, d.drop_seed = p, seed
    P.set_tensors(d, a=dev(a), out=out)
    launch(d, dict(out=(out, n)))
    got = host(out, n)
    assert np.array_equal(got != 0, r["keep"]), "the keep decisions are the oracle's keep_mask"
    assert np.array_equal(bits(got), bits(r["out"])), "a kept value is a * (1 / (1 - p)) in fp32, a dropped one +0"
    at, a0 = inplace(a)                                                      # in place, as the classification backward calls it
    P.set_tensors(d, a=at, out=at)
    launch(d, {}, restore=[(at, a0)])
    assert np.array_equal(bits(host(at, n)), bits(r["out"])), "the in-place form differs"


# ---- log_softmax ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", P.LSM_SHIFT)
@pytest.mark.parametrize("C", P.LSM_C)
@pytest.mark.parametrize("B", P.LSM_B)
def test_bt_log_softmax_and_bwd(B, C, shift):
    c = P.make_lsm(B, C, shift)
    r, rb = P.log_softmax_ref(c["z"]), P.log_softmax_bwd_ref(c["z"], c["d"])
    z = dev(c["z"])
    out, dz = nanbuf(B * C), nanbuf(B * C)
    d = P.new("bt_log_softmax", B=B, C=C)
    P.set_tensors(d, z=z, out=out)
    launch(d, dict(out=(out, B * C)))
    got = host(out, B * C, (B, C))
    assert note("bt_log_softmax", P.worst(got, r["out"])) <= 1.0
    tot = np.exp(got.astype(np.float64)).sum(1)
    assert np.all(np.abs(tot - 1.0) <= (np.exp(r["out"][0]) * r["out"][1]).sum(1) * 1.01 + 1e-15), "exp(out) sums to 1 within the bar"
    d = P.new("bt_log_softmax_bwd", B=B, C=C)
    P.set_tensors(d, z=z, da=dev(c["d"]), out=dz)
    launch(d, dict(out=(dz, B * C)))
    assert note("bt_log_softmax_bwd", P.worst(host(dz, B * C, (B, C)), rb["dz"])) <= 1.0


# ---- the eval fold ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("C", P.FOLD_C)
def test_bl_fold_and_affine(C, bias, bn):
    c = P.make_fold(C, bias, bn)
    r = P.fold_ref(c["bias"], c["gamma"], c["beta"], c["rm"], c["rv"], C)
    scale, shift = nanbuf(C), nanbuf(C)
    d = P.new("bl_fold", C=C)
    bnin = {k: dev(c[k]) if bn else unread(C) for k in ("beta", "rm", "rv")}
    P.set_tensors(d, bias=dev(c["bias"]) if bias else None, gamma=dev(c["gamma"]) if bn else None, scale=scale, shift=shift, **bnin)
    launch(d, dict(scale=(scale, C), shift=(shift, C)))
    sc, sh = host(scale, C).copy(), host(shift, C).copy()
    assert note("bl_fold scale", P.worst(sc, r["scale"])) <= 1.0 and note("bl_fold shift", P.worst(sh, r["shift"])) <= 1.0
    if not bn:
        assert np.all(sc == 1.0) and np.array_equal(bits(sh), bits(c["bias"] if bias else np.zeros(C, dtype=np.float32)))
    M, per = 13, 5
    g = np.random.default_rng(C + bias + 2 * bn)
    zin, add = P.f32(g.standard_normal((M, C))), P.f32(g.standard_normal(((M - 1) // per + 1, C)))
    for relu in (0, 1):
        for ad in (None, add):
            ra = P.affine_ref(zin, sc, sh, ad, per)
            z, z0 = inplace(zin)
            d = P.new("bl_affine", M=M, C=C, per=per if ad is not None else 0, relu=relu)
            P.set_tensors(d, z=z, scale=scale[:C].clone(), shift=shift[:C].clone(), add=None if ad is None else dev(ad))
            launch(d, {}, restore=[(z, z0)])
            got = host(z, M * C, (M, C))
            assert (~ra["sure"]).sum() <= 0.01 * M * C
            ratio = P.worst_relu(got, ra["pre"], ra["sure"]) if relu else P.worst(got, ra["pre"])
            assert note("bl_affine", ratio) <= 1.0, (relu, ad is not None)


# ---- fwd_layer, bwd_layer: the composition, bit for bit ----------------------------------------------------------------------------------------------
def small_gemm(ta, tb, M, N, K, A, lda, Bm, ldb, Cm, ldc, acc):
    lib = PP.L.lib()
    vp = ctypes.c_void_p
    rc = lib.ampnet_small_gemm_f32(int(ta), int(tb), M, N, K, vp(A), lda, vp(Bm), ldb, vp(Cm), ldc, int(acc), None, None, PP.L.stream_ptr())
    assert rc == 0, PP.last_error()
    torch.cuda.synchronize()


def one(op, ints=None, **tensors):
    d = P.new(op, **(ints or {}))
    P.set_tensors(d, **tensors)
    rc, _ = P.run(d)
    assert rc == 0, PP.last_error()


@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("c", P.LAYER_CASES, ids=lambda c: f"K{c['K']}_w{c['w0']}_bn{c['bn']}_dA{c['dA']}")
def test_layer_composition_is_its_kernels(c, train):
    M, C, K, lda, ldw, w0 = (c[k] for k in ("M", "C", "K", "lda", "ldw", "w0"))
    t = P.make_layer(c)
    bn = c["bn"]
    A, W = dev(t["A"]), dev(t["W"])
    bias, add = (None if t[k] is None else dev(t[k]) for k in ("bias", "add"))
    gamma = dev(t["gamma"]) if bn else None
    beta, rm0, rv0 = (dev(t[k]) if bn else None for k in ("beta", "rm", "rv"))
    n = M * C
    # ---- forward: composed
    z, a, mean, invstd = nanbuf(n), nanbuf(n), nanbuf(C), nanbuf(C)
    (rm, _), (rv, _) = (inplace(t["rm"]), inplace(t["rv"])) if bn else ((None, None), (None, None))
    d = P.new("fwd_layer", M=M, C=C, K=K, lda=lda, ldw=ldw, w0=w0, per=t["per"] if add is not None else 0, train=train)
    P.set_tensors(d, A=A, W=W, bias=bias, add=add, gamma=gamma, beta=beta, rm=rm, rv=rv, z=z, a=a if bn else None, mean=mean if bn else None,
                  invstd=invstd if bn else None)
    launch(d, dict(z=(z, n), a=(a, n if bn else 0), mean=(mean, C if bn else 0), invstd=(invstd, C if bn else 0)),
           restore=[(rm, inplace(t["rm"])[1]), (rv, inplace(t["rv"])[1])] if bn else ())
    # ---- forward: one kernel at a time
    z1, a1, mean1, invstd1 = nanbuf(n), nanbuf(n), nanbuf(C), nanbuf(C)
    small_gemm(0, 1, M, C, K, A.data_ptr(), lda, W.data_ptr() + 4 * w0, ldw, z1.data_ptr(), C, 0)
    if bias is not None or add is not None:
        one("bt_bias", dict(M=M, C=C, per=t["per"] if add is not None else 0), z=z1, bias=bias, add=add)
    if bn:
        rm1, rv1 = inplace(t["rm"])[0], inplace(t["rv"])[0]
        if train:
            one("bt_stats", dict(M=M, C=C), z=z1, mean=mean1, invstd=invstd1, rm=rm1, rv=rv1)
        else:
            one("bt_running_stats", dict(C=C), rm=rm1, rv=rv1, mean=mean1, invstd=invstd1)
        one("bt_bn_act", dict(M=M, C=C), z=z1, mean=mean1, invstd=invstd1, gamma=gamma, beta=beta, a=a1)
        for k, u, v in (("a", a, a1), ("mean", mean, mean1), ("invstd", invstd, invstd1), ("rm", rm, rm1), ("rv", rv, rv1)):
            assert np.array_equal(bits(host(u)), bits(host(v))), f"forward {k}: composed != one at a time"
        if not train:
            assert np.array_equal(bits(host(rm, C)), bits(t["rm"])) and np.array_equal(bits(host(rv, C)), bits(t["rv"])), "running statistics moved in eval"
    assert np.array_equal(bits(host(z)), bits(host(z1))), "forward z: composed != one at a time"
    if not train:
        return
    # ---- backward: composed
    want_dA, acc = c["dA"] > 0, int(c["dA"] == 2)
    ld_dA = K + 2
    (da, da0), (dA, dA0) = inplace(t["da"]), inplace(t["dA0"])
    dW, db, dg, dbe = nanbuf(C * ldw), nanbuf(C), nanbuf(C), nanbuf(C)
    tape = dict(z=z[:n].clone(), a=a[:n].clone() if bn else None, mean=mean[:C].clone() if bn else None, invstd=invstd[:C].clone() if bn else None)
    d = P.new("bwd_layer", M=M, C=C, K=K, lda=lda, ldw=ldw, w0=w0, ld_dA=ld_dA, accumulate=acc)
    P.set_tensors(d, da=da, A=A, W=W, gamma=gamma, dW=dW, db=db if c["bias"] else None, dg=dg if bn else None, dbe=dbe if bn else None,
                  dA=dA if want_dA else None, **tape)
    launch(d, dict(dW=(dW, None), db=(db, C if c["bias"] else 0), dg=(dg, C if bn else 0), dbe=(dbe, C if bn else 0)), restore=[(da, da0), (dA, dA0)])
    # ---- backward: one kernel at a time
    da1, dA1 = da0.clone(), dA0.clone()
    dW1, db1, dg1, dbe1 = nanbuf(C * ldw), nanbuf(C), nanbuf(C), nanbuf(C)
    if bn:
        one("bt_bn_bwd_sums", dict(M=M, C=C), da=da1, dg=dg1, dbe=dbe1, **tape)
        one("bt_bn_bwd_apply", dict(M=M, C=C), da=da1, gamma=gamma, dg=dg1, dbe=dbe1, **tape)
    small_gemm(1, 0, C, K, M, da1.data_ptr(), C, A.data_ptr(), lda, dW1.data_ptr() + 4 * w0, ldw, 0)
    if c["bias"]:
        dc = BN.new("colsum", rows=M, C=C)
        BN.set_tensors(dc, src=da1, dst=db1)
        rc, _ = BN.run(dc)
        assert rc == 0, PP.last_error()
    if want_dA:
        small_gemm(0, 0, M, K, C, da1.data_ptr(), C, W.data_ptr() + 4 * w0, ldw, dA1.data_ptr(), ld_dA, acc)
    for k, u, v in (("dz", da, da1), ("dW", dW, dW1), ("db", db, db1), ("dg", dg, dg1), ("dbe", dbe, dbe1), ("dA", dA, dA1)):
        assert np.array_equal(bits(host(u)), bits(host(v))), f"backward {k}: composed != one at a time"
    # what the composed call left alone: the columns of dW outside [w0, w0 + K), the pad columns of dA, all of dA when NULL
    assert is_sentinel(dW[C * ldw:])
    w = host(dW, C * ldw, (C, ldw))
    assert np.isfinite(w[:, w0:w0 + K]).all() and np.isnan(np.delete(w, np.s_[w0:w0 + K], 1)).all(), "dW: written exactly at columns w0 .. w0 + K"
    g = host(dA, M * ld_dA, (M, ld_dA))
    assert np.array_equal(bits(g[:, K:]), bits(t["dA0"][:, K:])), "dA: the pad columns moved"
    if not want_dA:
        assert np.array_equal(bits(g), bits(t["dA0"])), "dA == NULL was written"
    # against float64: dA and dW of the kernel's own dz
    dz = host(da, n, (M, C)).astype(np.float64)
    Wk, Ak = t["W"][:, w0:w0 + K].astype(np.float64), t["A"][:, :K].astype(np.float64)
    assert note("bwd_layer dW", P.worst(w[:, w0:w0 + K], (dz.T @ Ak, PP.bar(np.abs(dz).T @ np.abs(Ak), dz.T @ Ak, M)))) <= 1.0
    if want_dA:
        ref = dz @ Wk + (acc * t["dA0"][:, :K].astype(np.float64))
        assert note("bwd_layer dA", P.worst(g[:, :K], (ref, PP.bar(np.abs(dz) @ np.abs(Wk) + acc * np.abs(t["dA0"][:, :K]), ref, C + 1)))) <= 1.0
    zf = t["A"][:, :K].astype(np.float64) @ Wk.T
    mag = np.abs(Ak) @ np.abs(Wk).T
    for extra in (t["bias"], None if t["add"] is None else t["add"][np.arange(M) // t["per"]]):
        if extra is not None:
            zf, mag = zf + extra, mag + np.abs(extra)
    assert note("fwd_layer z", P.worst(host(z, n, (M, C)), (zf, PP.bar(mag, zf, K + 2)))) <= 1.0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def sizes(op, B=2, N=3, M=5, C=4, K=3, k=2, n=5, per=2, lda=4, ldw=5, w0=1, ld_dA=4):
    MC, BC, BNC, adds = M * C, B * C, B * N * C, ((M - 1) // per + 1) * C
    Wn = (C - 1) * ldw + w0 + K
    return {"bt_bias": dict(z=MC, bias=C, add=adds), "bt_stats": dict(z=MC, mean=C, invstd=C, rm=C, rv=C),
            "bt_running_stats": dict(rm=C, rv=C, mean=C, invstd=C), "bt_bn_act": dict(z=MC, a=MC, mean=C, invstd=C, gamma=C, beta=C),
            "bt_bn_bwd_sums": dict(da=MC, a=MC, z=MC, mean=C, invstd=C, dg=C, dbe=C),
            "bt_bn_bwd_apply": dict(da=MC, a=MC, z=MC, mean=C, invstd=C, gamma=C, dg=C, dbe=C),
            "bt_rowmax": dict(a=BNC, out=BC, arg=BC), "bl_rowmax": dict(a=BNC, out=BC), "bt_pool_scatter": dict(x=BC, arg=BC, a=BNC),
            "bt_mix": dict(x=M * 9, T=((M - 1) // N + 1) * k * k, out=M * 9), "bl_mix": dict(x=M * 9, T=((M - 1) // N + 1) * k * k, out=M * 9),
            "bt_mix_bwd": dict(x=B * N * 9, da=B * N * 9, out=B * k * k), "bt_segsum": dict(da=BNC, out=BC),
            "bt_logits": dict(z=BNC, out=BNC), "bt_logits_to_rows": dict(z=BNC, out=BNC), "bl_logits": dict(z=BNC, out=BNC),
            "bt_fill": dict(z=n), "bt_add": dict(z=n, x=n), "bt_dropout": dict(a=n, out=n),
            "bt_log_softmax": dict(z=BC, out=BC), "bt_log_softmax_bwd": dict(z=BC, da=BC, out=BC),
            "bl_fold": dict(bias=C, gamma=C, beta=C, rm=C, rv=C, scale=C, shift=C), "bl_affine": dict(z=MC, scale=C, shift=C, add=adds),
            "fwd_layer": dict(A=(M - 1) * lda + K, W=Wn, bias=C, add=adds, gamma=C, beta=C, rm=C, rv=C, z=MC, a=MC, mean=C, invstd=C),
            "bwd_layer": dict(da=MC, a=MC, z=MC, mean=C, invstd=C, gamma=C, W=Wn, A=(M - 1) * lda + K, dW=Wn, db=C, dg=C, dbe=C,
                              dA=(M - 1) * ld_dA + K)}[op]


WRITTEN = {"bt_bias": ("z",), "bt_stats": ("mean", "invstd", "rm", "rv"), "bt_running_stats": ("mean", "invstd"), "bt_bn_act": ("a",),
           "bt_bn_bwd_sums": ("dg", "dbe"), "bt_bn_bwd_apply": ("da",), "bt_rowmax": ("out", "arg"), "bl_rowmax": ("out",), "bt_pool_scatter": ("a",),
           "bt_mix": ("out",), "bl_mix": ("out",), "bt_mix_bwd": ("out",), "bt_segsum": ("out",), "bt_logits": ("out",), "bt_logits_to_rows": ("z",),
           "bl_logits": ("out",), "bt_fill": ("z",), "bt_add": ("z",), "bt_dropout": ("out",), "bt_log_softmax": ("out",), "bt_log_softmax_bwd": ("out",),
           "bl_fold": ("scale", "shift"), "bl_affine": ("z",), "fwd_layer": ("z", "a", "mean", "invstd", "rm", "rv"),
           "bwd_layer": ("da", "dW", "db", "dg", "dbe", "dA")}


def test_probe_refuses_bad_baseline_descriptors():
    """Every buffer of every op one element short, C = 65 for the log_softmax pair, k = 4, a zero dimension, a pooling index outside its window:
    AMPNET_E_ARG, nothing launched, every buffer an op could write (in-place operands included) still at its sentinel."""
    dims = dict(B=2, N=3, M=5, C=4, K=3, k=2, per=2, lda=4, ldw=5, w0=1, ld_dA=4)

    def attempt(op, short=None, arg_fill=-7, **over):
        full = sizes(op, **{k: v for k, v in over.items() if k in ("C", "k") and v > 0})
        bufs = {}
        for name, cnt in full.items():
            cnt = max(cnt - (name == short), 1)
            bufs[name] = torch.full((cnt,), arg_fill, dtype=torch.int32, device="cuda") if name == "arg" else \
                torch.full((cnt,), float("nan"), dtype=torch.float32, device="cuda")
        d = P.new(op, **{**dims, "n": 5, "train": 1, **over})
        d.drop_p = 0.3
        P.set_tensors(d, **bufs)
        if short is not None and full[short] == 1:
            setattr(d, short + "_n", 0)                         # a one-element buffer "one short": extent 0 on a live pointer
        rc, names = P.run(d)
        assert rc == P.AMPNET_E_ARG and names == [], (op, short, over, rc, names)
        for name in WRITTEN[op]:
            t = bufs[name]
            assert bool((t == arg_fill).all()) if name == "arg" else is_sentinel(t), (op, short, name)

    for op in P.OPS:
        for short in sizes(op):
            attempt(op, short, arg_fill=1)
        zero = "n" if op in ("bt_fill", "bt_add", "bt_dropout") else "C" if op in ("bt_running_stats", "bl_fold") else \
            "M" if op in ("bt_mix", "bl_mix") else "B" if "B" in _dims_of(op) else "M"
        attempt(op, arg_fill=1, **{zero: 0})
    for op in ("bt_log_softmax", "bt_log_softmax_bwd"):
        attempt(op, C=65)                                       # buffers sized for C = 65: only the limit refuses
    for op in ("bt_mix", "bl_mix", "bt_mix_bwd"):
        attempt(op, k=4)
        attempt(op, k=1)
    attempt("bt_pool_scatter", arg_fill=3)                      # N = 3: rows 0 .. 2
    attempt("bt_pool_scatter", arg_fill=-1)
    d = P.BaselineProbe()
    d.op = 25
    assert P.run(d) == (P.AMPNET_E_ARG, [])
    d.op = -1
    assert P.run(d) == (P.AMPNET_E_ARG, [])
    for which, B, N, C, rc, msg in P.backward_shape_refusals():
        assert rc == P.AMPNET_E_ARG and "bad shape" in msg, (which, B, N, C, rc, msg)


def _dims_of(op):
    return "BNC" if op in ("bt_rowmax", "bl_rowmax", "bt_pool_scatter", "bt_mix_bwd", "bt_segsum", "bt_logits", "bt_logits_to_rows", "bl_logits",
                           "bt_log_softmax", "bt_log_softmax_bwd") else "MC"
