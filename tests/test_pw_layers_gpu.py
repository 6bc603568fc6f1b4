"""Layer-local float64 parity of the per-point layer kernels: pw_gemm (csrc/pw_gemm.hip) and the fused backward pw_bwd_fused with the split
(pw_bwd_x3.hip) and bf16 (pw_bwd_bf16.hip) kernels it dispatches to.

Each case launches ONE kernel through the test hook (include/ampnet_hip.h, "test hooks") on inputs chosen here and holds every output to a
float64 restatement of the same operation on the same fp32 inputs (tests/pw_probe.py), with the bar of pw_probe.bar:
    |x - x64| <= 8 eps sqrt(K) (|u| |v|) + 2 eps |x64|,   eps = 2^-24 (fp32, f32x3) or 2^-8 (bf16 operands)
Nothing upstream feeds these inputs, so the chaotic network-level gradients (tests/diagnostics/README.md) cannot move the bar.
Every case also checks: outputs pre-filled with NaN are finite where the contract writes and keep their sentinel bits where it does not
(padding columns, partial slots past the plan); a second run is bitwise identical; the kernel that ran is the instantiation the case is
meant for (profile names: " x3" in f32x3 for every split-eligible shape, " bf16" in the bf16 modes).

The forward in the bf16 modes is held in TWO tiers (check_gemm).  Tier 1, the project bar: the reference above on the operands as given
(a bf16 A: its rounded values), eps = 2^-8, a bf16 Z with 2 eps |z64| more.  Tier 2, the contract bar (families "pw_gemm t2 ..."): the
reference on the bf16-ROUNDED prologue output and weights (pw_probe.gemm_ref(operands="bf16")), eps = 2^-24 -- fp32 accumulation is the
only error left; a bf16 Z must be the round-to-nearest-even of a value within the bar (pw_probe.bf16_bracket); the statistics, fin_*
constants and pool extremes follow the UNROUNDED accumulator.  The reference forms the prologue in float64, the kernel in fp32: a prologue
output within 2^-22 |v| of a bf16 rounding midpoint may round either way ("ambiguous"; asserted < 2^-10 of the positive ones per case,
observed 3.6e-5 .. 3.1e-4), and each output carries sum_k [ambiguous] ulp_bf16(v_k) |w'_jk| on top of its bar (families "... amb";
outputs, slots and extremes that no ambiguous element reaches keep the plain bar and are reported apart).  tests/test_pw_refs_cpu.py
shows on the c128_128 data that a truncating store, statistics of the stored z and a truncated weight image each land outside tier 2
and inside tier 1.
Observed on the MI355X, worst error/bar, bf16_train / bf16_store: tier 1 Z 0.007 / 0.011, statistics 0.001 / 0.001, pool 0.002 / 0.003;
tier 2 Z 0.077 / 0.0625 (bf16 Z: the lowest rung of bracket_ratio's ladder), statistics 0.027 / 0.013, pool 0.032 / 0.023; tier 2 with an
ambiguous element in reach: Z 0.998 / 1.0 (rung (1/2, 1]), statistics 0.51 / 0.12.  The two above 0.5 are the reference's own ambiguity,
not accumulation error: where an ambiguous element did round the other way the output is off by exactly its widening, i.e. at
widening / (bar + widening), just under 1 (every output beyond the plain bar had an ambiguous element: 118 of 118 on ones160, 246 of 246
on c128_128, against 0.014 / 0.035 on the others); see tier_moment_bars for the statistics.

Cases, from the dispatch of pw_gemm / launch_pw / launch_pw_x and pw_bwd_fused / launch_fused / pw_bwd_fused_x3 / pw_bwd_fused_bf16:
  forward (fp32, f32x3, bf16_train: every case, pool_eval there asserted as pw_gemm's refusal, chunk512 skipped; bf16_store: the
  (a_bf16, z_bf16) pairs of FWD_STORE; c64_64, c128_128, pool, c64_40 and drop128 in fp32 with AMPNET_PW_PIPE=1 and =0)
    c64_64    cin 64 -> 64, no prologue, per-workgroup statistics, ragged windows, 3 slots
    c64_128   cin 64 -> 128, BN+ReLU prologue, statistics; Q = 576, 9 slots, 300 rows (the persistent loop wraps)
    c128_128  cin 128 -> 128 BN+ReLU, Z + statistics (split-eligible), 12 slots, windows of 1 .. 700 rows
    pool      cin 128 -> 256 BN+ReLU, pool with argmax + statistics, negative gammas (split-eligible); Q = 576, 9 slots, 300 rows
    pool_eval cin 128 -> 256, pool without argmax (the eval form), 1 slot
    pool_z    cin 128 -> 256, pool with argmax AND a stored Z, negative gammas, a window of identical rows (tie rule)
    c256_fc   cin 256 -> 256 FC rows: bias, uniform_rows, direct in-kernel BatchNorm finalize (fin_*), tiny-problem NT narrowing
    c256_fc2  cin 256 -> 128 FC rows with B > 128 per slot: per-workgroup partials (two-stage path)
    fc3       cin 128 -> 9 FC: bias + identity_k = 3
    bmm       cin 64 -> 64 per-window weights ([cin][cout] k-major, slot-major pidx), 3 slots
    drop128   cin 128 -> 64, BN+ReLU+dropout prologue
    drop64    cin 64 -> 32, BN+ReLU+dropout prologue
    c64_40    cin 64 -> 40 (not a multiple of 32), ldz 48 (padding columns)
    c128_200  cin 128 -> 200 (not a multiple of 128: not split-eligible), ldz 208
    pfin      cin 128 -> 128 with the consumer-side finalize of the input's BatchNorm (pfin_*)
    chunk512  the split-eligible c128_128 shape handed chunk_rows 512 (the non-split chunking): refused or correct
    conv2     cin 64 -> 128, no prologue, a per-window bias (bias_win_stride), 1 slot: the head's conv_2
    ones      cin 128 -> 128 BN+ReLU, 40 windows of ONE row, 4 slots: every prefetch crosses a window (narrowed to 32 columns)
    ones160   the same with 160 windows: the 128-column instantiations (split-eligible)
    bf16_store only: drop128 with a bias (the head's conv_3), drop64 with a bias, cout 5, ldz 8 (the head's conv_4)
    refusals  a bf16 A or Z in fp32 / f32x3, a bf16 A with lda 68: pw_gemm's own checks, outputs left at their sentinels
  backward (fp32, f32x3, bf16_train, bf16_store)
    b128_128 dense / b128_gram Gram / b128_64 act / b128_64lin / b64_64 act / b64_64add act+add / b64_64lin lin+add / b64_128 /
    b64_128drop dropout / bmm64 per-window weights + items_per_block / slotw Gram with w_slot_stride + bias_slot /
    fin128_64 in-kernel BatchNorm-backward constants (fin_*; fp32 kernels only) / wrap128 Q = 576, 9 slots, 300 rows.
The unfused pw_dgrad / pw_wgrad (probe kinds 1 and 2) and the max-pooled layers' backward are tests/test_pooled_bwd_gpu.py.
Pool tie rule (pw_gemm.hip: strict compare in ascending rows, lower row on equal merges): the FIRST row of a chunk among equal extremes.
"""
import os

import numpy as np
import pytest
import torch

import pw_probe as PP

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[pw layers] worst error/bar {k}: {WORST[k]:.4f}")


def note(family, mode, r):
    key = f"{family} {mode}"
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


class precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        PP.L.set_matrix_precision(self.mode)

    def __exit__(self, *a):
        PP.L.set_matrix_precision("fp32")


def nanbuf(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -7, dtype=torch.int32, device="cuda")
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def is_sentinel(t):
    a = t.detach().cpu()
    if a.dtype == torch.int32:
        return bool((a == -7).all())
    if a.dtype == torch.bfloat16:
        return bool((a.contiguous().view(torch.int16) == NAN_BITS >> 16).all())
    return bool((a.view(torch.int32) == NAN_BITS).all())


def rng(seed):
    return np.random.default_rng(seed)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)


def offsets(sizes, base=0):
    return np.concatenate([[base], base + np.cumsum(sizes)]).astype(np.int32)


def snap(d):
    return {k: v.detach().cpu().clone() for k, v in d.items() if torch.is_tensor(v)}


def bitwise_equal(a, b):
    for k in a:
        x, y = a[k], b[k]
        if x.dtype in (torch.float32,):
            x, y = x.view(torch.int32), y.view(torch.int32)
        elif x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        assert torch.equal(x, y), f"{k}: second run differs bitwise"


# ================================================================================================================================
# forward
# ================================================================================================================================
FWD = {
    # name: cin, cout, ldz, window sizes, n_slots, pro (0/1/2), pool (None/"arg"/"noarg"), Z, stats ("wg"/None), extras
    "c64_64": dict(cin=64, cout=64, sizes=[1, 4, 31, 33, 127, 129, 255, 257, 700], S=3, pro=0, stats="wg"),
    "c64_128": dict(cin=64, cout=128, sizes=[300] * 576, S=9, pro=1, stats="wg"),
    "c128_128": dict(cin=128, cout=128, sizes=[1, 4, 31, 33, 127, 129, 255, 257, 700, 64, 128, 5] * 2, S=12, pro=1, stats="wg"),
    "pool": dict(cin=128, cout=256, sizes=[300] * 576, S=9, pro=1, pool="arg", stats="wg", neg=True, Z=False),
    "pool_eval": dict(cin=128, cout=256, sizes=[129, 31, 700, 257], S=1, pro=1, pool="noarg", Z=False, neg=True),
    "pool_z": dict(cin=128, cout=256, sizes=[257, 40, 129, 700], S=2, pro=1, pool="arg", neg=True, dup=1),
    "c256_fc": dict(cin=256, cout=256, uniform=8, Q=3, S=3, pro=0, bias=True, stats="fin"),
    "c256_fc2": dict(cin=256, cout=128, uniform=200, Q=2, S=2, pro=1, bias=True, stats="wg", fc=True),
    "fc3": dict(cin=128, cout=9, uniform=8, Q=1, S=1, pro=1, bias=True, identity_k=3),
    "bmm": dict(cin=64, cout=64, sizes=[33, 129, 4, 257, 31, 127], S=3, pro=1, perwin=True),
    "drop128": dict(cin=128, cout=64, sizes=[255, 33, 700, 1], S=2, pro=2),
    "drop64": dict(cin=64, cout=32, sizes=[127, 129, 31], S=3, pro=2),
    "c64_40": dict(cin=64, cout=40, ldz=48, sizes=[31, 33, 257], S=3, pro=1, stats="wg"),
    "c128_200": dict(cin=128, cout=200, ldz=208, sizes=[129, 255, 4], S=3, pro=1, stats="wg"),
    "pfin": dict(cin=128, cout=128, sizes=[127, 129, 255, 257, 31, 33] * 8, S=3, pro=1, stats="wg", pfin=True),
    "chunk512": dict(cin=128, cout=128, sizes=[700, 257, 129, 1] * 16, S=2, pro=1, stats="wg", chunk512=True),
    "conv2": dict(cin=64, cout=128, sizes=[33, 1, 257, 127, 700, 31], S=1, pro=0, stats="wg", biaswin=True),
    "ones": dict(cin=128, cout=128, sizes=[1] * 40, S=4, pro=1, stats="wg"),
    "ones160": dict(cin=128, cout=128, sizes=[1] * 160, S=4, pro=1, stats="wg"),
}
# bf16_store: the (a_bf16, z_bf16) pairs the product launches each shape with (csrc/encoder.hip, head.hip), and what the head's layers add
FWD_STORE = {
    "c64_64": [(1, 1), (0, 1)], "c64_128": [(1, 1)], "c128_128": [(1, 1)], "pool": [(1, 0)], "pool_z": [(1, 1)], "drop128": [(1, 1)],
    "drop64": [(1, 0)], "c64_40": [(1, 1)], "c128_200": [(1, 1)], "pfin": [(1, 1)], "bmm": [(1, 1)], "conv2": [(0, 1)], "ones": [(1, 1)],
    "ones160": [(1, 1)],
}
FWD_STORE_EXTRA = {"drop128": dict(bias=True),                        # as the head's conv_3
                   "drop64": dict(bias=True, cout=5, ldz=8)}          # as the head's conv_4
FWD_MODES = ["fp32", "f32x3", "bf16_train", "bf16_store"]
POOL_EVAL_REFUSAL = "the pool epilogue without argmax rows is the fp32 eval form"


def fwd_case(name, mode):
    return dict(FWD[name], **FWD_STORE_EXTRA.get(name, {})) if mode == "bf16_store" else FWD[name]


def fwd_params():
    ps = [pytest.param(name, mode, None, id=f"{name}-{mode}") for mode in FWD_MODES[:3] for name in FWD]
    return ps + [pytest.param(name, "bf16_store", pair, id=f"{name}-bf16_store-a{pair[0]}z{pair[1]}") for name in FWD_STORE for pair in FWD_STORE[name]]


def fwd_x3_expected(c, mode, n_blocks):
    """pw_gemm.hip launch_pw_x: the split kernels serve cin 128, > 64 columns in whole blocks of 128, BN+ReLU prologue, no bias / identity /
    per-window weights / uniform rows, Z or the pool (not both), statistics only per workgroup -- and (pw_gemm) a problem that is not
    narrowed to 32 / 64-column blocks: the pool, or at least 128 workgroups of (blocks of rows) x (128-column blocks)."""
    if mode != "f32x3":
        return False
    if not c.get("pool") and n_blocks * -(-c["cout"] // 128) < 128:
        return False
    return (c["cin"] == 128 and c["cout"] > 64 and c["cout"] % 128 == 0 and c.get("pro") == 1 and not c.get("bias") and not c.get("identity_k")
            and not c.get("perwin") and not c.get("uniform") and (bool(c.get("pool")) != c.get("Z", True)) and c.get("stats") != "chunk")


def fwd_name(c, n_blocks, split, mode="fp32"):
    """The profile name of the instantiation pw_gemm picks (pw_gemm.hip: pw_gemm's NT choice and tiny-problem narrowing, launch_pw_y's name)."""
    cout = c["cout"]
    nt = 4 if cout > 64 else (2 if cout > 32 else 1)
    while nt > 1 and not c.get("pool") and c.get("pro") != 2 and n_blocks * -(-cout // (32 * nt)) < 128:
        nt //= 2
    return (f"pw_gemm<{c['cin']},{32 * nt}>" + ("+store" if c.get("Z", True) else "") + ("+pool" if c.get("pool") else "")
            + (" x3" if split else (" bf16" if mode.startswith("bf16") else "")))


def gemm_host(c, seed, a_bf16=0):
    """The host side of a forward case: every input as numpy fp32 (no GPU, no library).  a_bf16: A holds bf16 values (rounded here, so
    that the float64 references read what the kernel reads)."""
    g = rng(seed)
    cin, cout, S = c["cin"], c["cout"], c["S"]
    uniform = c.get("uniform", 0)
    if uniform:
        Q = c["Q"]
        sizes = [uniform] * Q
    else:
        sizes = c["sizes"]
        Q = len(sizes)
    wo = offsets(sizes)
    rows = int(wo[-1])
    A = f32(g.standard_normal((rows, cin)))
    if c.get("dup"):
        A[wo[c["dup"]]:wo[c["dup"] + 1]] = A[wo[c["dup"]]]          # a window of identical rows
    if a_bf16:
        A = torch.from_numpy(A).bfloat16().float().numpy()
    W = f32(g.uniform(-1, 1, (cout, cin)) / np.sqrt(cin))
    host = dict(A=A, W=W, win_off=wo, rows=rows, Q=Q, S=S, max_rows=max(sizes))
    if c.get("perwin"):
        host["W"] = f32(g.uniform(-1, 1, (Q, cin, cout)) / np.sqrt(cin))
    if c.get("bias"):
        host["bias"] = f32(g.uniform(-0.5, 0.5, cout))
    if c.get("biaswin"):
        host["bias"] = f32(g.uniform(-0.5, 0.5, (Q, cout)))        # one row per window (bias_win_stride = cout)
    if c.get("pro"):
        s = f32(g.uniform(0.5, 1.5, (S, cin)) * np.where(g.random((S, cin)) < 0.1, -1, 1))
        host["pro"] = (s, f32(g.uniform(-0.5, 0.5, (S, cin))))
    if c.get("pro") == 2:
        host["drop"] = (0.3, (seed, 7))
    if c.get("stats") == "fin":
        host["fin"] = (f32(g.uniform(0.5, 1.5, cout)), f32(g.uniform(-0.3, 0.3, cout)))
    if c.get("pool") and c.get("neg"):
        host["gamma"] = f32(g.uniform(0.5, 1.5, cout) * np.where(np.arange(cout) % 3 == 1, -1, 1))
    if c.get("pfin"):
        P = 2 * S
        pm = f32(g.uniform(-1, 1, (P, cin)))
        prow = (g.integers(50, 400, P)).astype(np.int32)
        prow[-1] = 0                                         # an empty partial slot
        pq = f32(g.uniform(0.5, 2.0, (P, cin)) * prow[:, None])
        host["pfin"] = (pm, pq, prow, f32(g.uniform(0.5, 1.5, cin)), f32(g.uniform(-0.3, 0.3, cin)))
    return host


def make_gemm(name, c, mode, seed, pair=None):
    a_bf16, z_bf16 = pair or (0, 0)
    host = gemm_host(c, seed, a_bf16)
    cin, cout, S = c["cin"], c["cout"], c["S"]
    ldz = c.get("ldz", cout)
    uniform = c.get("uniform", 0)
    A, W, wo, rows, Q, max_rows = (host[k] for k in ("A", "W", "win_off", "rows", "Q", "max_rows"))
    sh = PP.plan(Q, S, max_rows, cin, cout)
    chunk_rows, chunks = (sh.x_chunk_rows, sh.x_chunks) if (mode == "f32x3" and cin == 128 and cout > 64 and cout % 128 == 0) else (sh.chunk_rows, sh.chunks)
    if uniform:
        chunk_rows, chunks = sh.fc_chunk_rows, -(-uniform // sh.fc_chunk_rows)
    if c.get("chunk512"):
        chunk_rows, chunks = sh.chunk_rows, sh.chunks
    split = fwd_x3_expected(c, mode, Q * chunks)
    d = PP.PwGemmProbe()
    d.lda, d.cin, d.ldw, d.n_slots, d.cout, d.ldz = cin, cin, cin, S, cout, ldz
    d.Q, d.chunk_rows, d.chunks, d.uniform_rows, d.identity_k, d.fin_eps = Q, chunk_rows, chunks, uniform, c.get("identity_k", 0), 1e-5
    d.a_bf16, d.z_bf16 = a_bf16, z_bf16
    t = dict(A=dev(A, torch.bfloat16 if a_bf16 else torch.float32), win_off=dev(wo, torch.int32), W=dev(W))
    host.update(chunk_rows=chunk_rows, chunks=chunks, name=fwd_name(c, Q * chunks, split, mode))
    if c.get("perwin"):
        d.w_win_stride, d.perwin_slot_major = cin * cout, 1
    if "bias" in host:
        t["bias"] = dev(host["bias"])
        d.bias_win_stride = cout if c.get("biaswin") else 0
    if c.get("pro"):
        t["pro_scale"], t["pro_shift"] = dev(host["pro"][0]), dev(host["pro"][1])
    if c.get("pro") == 2:
        d.drop_p = 0.3
        d.drop_seed = PP.drop_base(seed, 7)
    if c.get("Z", True):
        t["Z"] = nanbuf(rows, ldz, dtype=torch.bfloat16 if z_bf16 else torch.float32)
    if c.get("stats") == "wg":
        lanes = PP.plan(Q, S, max_rows, cin, cout, chunks).stat_lanes      # the orchestration's plan (lane cap of the kernel family)
        parts = -(-lanes // S) * S
        d.stat_lanes = lanes
        t["part_sum"], t["part_sq"] = nanbuf(parts + S, cout), nanbuf(parts + S, cout)
        t["part_rows"] = nanbuf(parts + S, dtype=torch.int32)
        host["parts"] = parts
    if c.get("stats") == "fin":
        lanes = S
        d.stat_lanes = lanes
        t["part_sum"], t["part_sq"] = nanbuf(S, cout), nanbuf(S, cout)
        t["part_rows"] = nanbuf(S, dtype=torch.int32)
        t["fin_gamma"], t["fin_beta"] = dev(host["fin"][0]), dev(host["fin"][1])
        for k in ("scale", "shift", "mean", "invstd", "smean", "suvar"):
            t["fin_" + k] = nanbuf(S, cout)
    if c.get("pool"):
        n = Q * chunks
        t["part_max"] = nanbuf(n + 1, cout)
        if c["pool"] == "arg":
            t["part_amax"] = nanbuf(n + 1, cout, dtype=torch.int32)
        if c.get("neg"):
            t["pool_gamma"] = dev(host["gamma"])
    if c.get("pfin"):
        pm, pq, prow = host["pfin"][:3]
        t["pfin_sum"], t["pfin_sq"], t["pfin_rows"] = dev(pm), dev(pq), dev(prow, torch.int32)
        t["pfin_gamma"], t["pfin_beta"] = dev(host["pfin"][3]), dev(host["pfin"][4])
        d.pfin_parts = len(prow)
        for k in ("scale", "shift", "mean", "invstd", "smean", "suvar"):
            t["pfin_" + k] = nanbuf(S, cin)
    PP.set_tensors(d, PP.GEMM_EXTENTS, **t)
    return d, t, host, split


def bracket_ratio(Z, Z64, b):
    """A stored bf16 Z against PP.bf16_bracket: the smallest s of (1/16, 1/4, 1/2, 1) at which EVERY element lies in the bracket of s * b
    (2.0: not even at the bar itself).  Elements that pass at one s pass at every larger one and are not looked at again."""
    assert np.all(np.isfinite(Z)), "non-finite where the contract writes"
    z, z64, b = Z.reshape(-1), Z64.reshape(-1), np.broadcast_to(b, Z64.shape).reshape(-1)
    for s in (0.0625, 0.25, 0.5, 1.0):
        lo, hi = PP.bf16_bracket(z64, s * b)
        bad = (z < lo) | (z > hi)
        if not bad.any():
            return s
        z, z64, b = z[bad], z64[bad], b[bad]
    return 2.0


def tier_moment_bars(z64, mag, cin, eps, wid):
    """PP.moment_bars, and the family suffix.  Tier 2 (wid = the ambiguity widening of these rows): a slot none of whose rows has an
    ambiguous element keeps exactly that bar (suffix ""); in any other the REFERENCE's moments are only known up to the flips -- each row
    moves by at most wid, so the mean by at most mean(wid) and the variance by at most mean(2 |dz| w + w^2) + mean(w) (2 mean|dz| +
    mean(w)) -- and that is added (suffix " amb").  Measured on ones160 / bf16_train, slot 0 (40 rows, one flipped element): the kernel's
    mean is 8.631e-06 from the reference's, which is exactly wid / 40 of that row, its variance 1.61 x the plain bar from it, and both equal the
    moments of the kernel's own fp32 Z to 1e-16; the plain bar alone would hold the reference's ambiguity against the kernel."""
    mu, var, bmean, bvar = PP.moment_bars(z64, mag, cin, eps)
    if wid is None or not wid.any():
        return mu, var, bmean, bvar, ""
    dz = np.abs(z64 - mu)
    wm = wid.mean(0)
    return mu, var, bmean + wm, bvar + (2 * dz * wid + wid * wid).mean(0) + wm * (2 * dz.mean(0) + wm), " amb"


def check_gemm(name, c, mode, d, t, host, split, names):
    """Tier 1 (every mode): the float64 reference on the operands as given, the bar at the mode's eps.  Tier 2 (bf16 modes, families
    "pw_gemm t2 ..."): the float64 reference on the bf16-ROUNDED operands, the bar at eps = 2^-24 plus the ambiguity widening -- fp32
    accumulation is the only error left; a bf16 Z must lie in PP.bf16_bracket; statistics and pool extremes follow the UNROUNDED z."""
    bf = mode.startswith("bf16")
    cin, cout = c["cin"], c["cout"]
    S = host["S"]
    assert names == [host["name"]], (names, host["name"])          # the intended instantiation, x3 or bf16 or neither, ran
    pro = pfin_constants(c, mode, t, host)
    kw = dict(pro=pro, drop=host.get("drop"), bias=host.get("bias"), bias_win_stride=d.bias_win_stride, w_win_stride=d.w_win_stride,
              slot_major=d.perwin_slot_major, identity_k=c.get("identity_k", 0))
    Z64, M = PP.gemm_ref(host["A"], cin, cout, host["W"], host["win_off"], S, **kw)
    worst = check_gemm_tier("", c, mode, d, t, host, Z64, M, PP.EPS16 if bf else PP.EPS32, None)
    if bf:
        del Z64, M
        Z64r, Mr, amb = PP.gemm_ref(host["A"], cin, cout, host["W"], host["win_off"], S, operands="bf16", **kw)
        print(f"[pw layers] {name} {mode}: ambiguous share of the positive prologue outputs {amb['share']:.3e}")
        assert amb["share"] < 2.0 ** -10, amb["share"]
        assert pro is not None or not amb["wid"].any()
        worst = max(worst, check_gemm_tier(" t2", c, mode, d, t, host, Z64r, Mr, PP.EPS32, amb["wid"]))
    return worst


def pfin_constants(c, mode, t, host):
    """The prologue constants of the case; pfin: the kernel's own pfin_scale / pfin_shift, held to float64 here."""
    fam = "pw_gemm"
    S = host["S"]
    pro = host.get("pro")
    if c.get("pfin"):
        pm, pq, prow, gam, bet = host["pfin"]
        sc = t["pfin_scale"].cpu().numpy().astype(np.float64)
        shf = t["pfin_shift"].cpu().numpy().astype(np.float64)
        for sl in range(S):
            idx = np.arange(sl, len(prow), S)
            n, mean, m2 = PP.chan_merge(pm[idx], pq[idx], prow[idx])
            var = m2 / n
            inv = 1.0 / np.sqrt(var + 1e-5)
            note(fam + " pfin", mode, PP.ratio(t["pfin_mean"].cpu().numpy()[sl], mean, np.abs(mean) + np.sqrt(var), len(idx)))
            note(fam + " pfin", mode, PP.ratio(t["pfin_invstd"].cpu().numpy()[sl], inv, inv, len(idx)))
            note(fam + " pfin", mode, PP.ratio(sc[sl], gam * inv, np.abs(gam * inv), len(idx)))
            note(fam + " pfin", mode, PP.ratio(shf[sl], bet - mean * gam * inv, np.abs(bet) + np.abs(mean * gam * inv), len(idx)))
            note(fam + " pfin", mode, PP.ratio(t["pfin_suvar"].cpu().numpy()[sl], m2 / (n - 1), m2 / (n - 1), len(idx)))
        pro = (f32(sc), f32(shf))                      # the prologue the kernel staged: its own outputs, held to float64 above
    return pro


def check_gemm_tier(tier, c, mode, d, t, host, Z64, M, eps, wid):
    """Every output against one float64 reference (Z64, magnitudes M) at `eps`; wid [rows, cout]: the ambiguity widening of tier 2."""
    fam = "pw_gemm" + tier
    cin, cout = c["cin"], c["cout"]
    S, Q, rows = host["S"], host["Q"], host["rows"]
    zbf = bool(d.z_bf16)
    worst = 0.0
    if "Z" in t:
        Zt = t["Z"].cpu()
        Z = Zt.float().numpy().astype(np.float64)[:rows, :cout]                 # (bf16 -> float64 is exact)
        zb = PP.bar(M, Z64, cin, eps)
        if not tier:                                                # (a bf16 Z, tier 1: its rounding on top, the rule of test_bn_glue_gpu.py)
            worst = max(worst, note(fam, mode, PP.err_ratio(Z, Z64, zb + (2 * PP.EPS16 * np.abs(Z64) if zbf else 0.0))))
        else:
            # outputs no ambiguous element feeds carry the plain bar (family "t2"); the others the bar plus the widening ("t2 amb": one that
            # did flip sits at widening / (bar + widening), just under 1, by construction).  A bf16 Z: the RNE rounding of a value in the bar
            for sub, sel in (("", wid == 0.0), (" amb", wid > 0.0)):
                if sel.any():
                    z, z64, b = Z[sel], Z64[sel], (zb + wid)[sel]
                    worst = max(worst, note(fam + sub, mode, bracket_ratio(z, z64, b) if zbf else PP.err_ratio(z, z64, b)))
        if d.ldz > cout:
            assert is_sentinel(Zt[:, cout:]), "padding columns of Z were written"
    q = PP.win_of_rows(host["win_off"])
    slot = q % S
    if c.get("stats") == "wg":
        parts = host["parts"]
        ps, pq, pr = (t[k].cpu().numpy() for k in ("part_sum", "part_sq", "part_rows"))
        assert is_sentinel(t["part_sum"][parts:]) and is_sentinel(t["part_rows"][parts:]), "partials past the plan were written"
        for sl in range(S):
            idx = np.arange(sl, parts, S)
            live = pr[idx] > 0
            assert np.all(pr[idx] >= 0), "a partial slot inside the plan was left unwritten"
            assert np.all(np.isfinite(ps[idx][live])) and np.all(np.isfinite(pq[idx][live]))
            n, mean, m2 = PP.chan_merge(ps[idx][live], pq[idx][live], pr[idx][live])
            r = slot == sl
            assert n == r.sum(), (sl, n, r.sum())
            mu, var, bmean, bvar, sub = tier_moment_bars(Z64[r], M[r], cin, eps, None if wid is None else wid[r])
            worst = max(worst, note(fam + " stats" + sub, mode, PP.err_ratio(mean, mu, bmean)))
            worst = max(worst, note(fam + " stats" + sub, mode, PP.err_ratio(m2 / n, var, bvar)))
    if c.get("stats") == "fin":
        gam, bet = host["fin"]
        for sl in range(S):
            r = slot == sl if not d.uniform_rows else (np.arange(rows) // d.uniform_rows) % S == sl
            K = r.sum()
            mu, var, bmean, bvar, _ = tier_moment_bars(Z64[r], M[r], cin, eps, None if wid is None else wid[r])
            inv = 1.0 / np.sqrt(var + 1e-5)
            binv = 0.5 * inv ** 3 * bvar + 4 * eps * inv
            got = {k: t["fin_" + k].cpu().numpy()[sl].astype(np.float64) for k in ("scale", "shift", "mean", "invstd", "suvar")}
            for k, want, b in (("mean", mu, bmean), ("invstd", inv, binv), ("scale", gam * inv, np.abs(gam) * binv + 4 * eps * np.abs(gam * inv)),
                               ("shift", bet - mu * gam * inv, np.abs(mu * gam) * binv + np.abs(gam * inv) * bmean + 4 * eps * (np.abs(bet) + np.abs(mu * gam * inv))),
                               ("suvar", var * K / (K - 1), bvar * K / (K - 1) + 4 * eps * var)):
                worst = max(worst, note(fam + " stats", mode, PP.err_ratio(got[k], want, b)))
    if c.get("pool"):
        pmx = t["part_max"].cpu().numpy()
        am = t["part_amax"].cpu().numpy() if "part_amax" in t else None
        n = Q * host["chunks"]
        assert is_sentinel(t["part_max"][n:]), "pool partials past Q * chunks were written"
        gam = host.get("gamma", np.ones(cout, np.float32))
        sg = np.where(gam < 0, -1.0, 1.0)
        cr = host["chunk_rows"]
        Zk = t["Z"].float().cpu().numpy() if "Z" in t and not tier else None      # (the kernel against its own Z: once)
        # a bf16 Z is the rounding of the fp32 value the extreme was taken from; rounding is monotone, so the extremes agree after it
        own = (lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()) if zbf else (lambda x: x)
        for qq in range(Q):
            for ch in range(host["chunks"]):
                i = qq * host["chunks"] + ch
                r0 = host["win_off"][qq] + ch * cr
                r1 = min(host["win_off"][qq + 1], r0 + cr)
                if r1 <= r0:
                    assert np.all(np.isinf(pmx[i])) and (am is None or np.all(am[i] == -1)), "empty chunk"
                    continue
                z64 = Z64[r0:r1] * sg
                ext64 = z64.max(0) * sg
                b = PP.bar(M[r0:r1].max(0), ext64, cin, eps)
                assert np.all(np.isfinite(pmx[i]))
                # tier 2: every row's z' is known up to its own widening w, so the extreme lies in [max(z' - w), max(z' + w)] (the column
                # maximum itself where no ambiguous row comes near it)
                w = np.zeros_like(z64) if wid is None else wid[r0:r1]
                elo, ehi = (z64 - w).max(0), (z64 + w).max(0)
                x = pmx[i] * sg
                worst = max(worst, note(fam + " pool", mode, float(np.max(np.maximum(np.maximum(elo - x, x - ehi), 0.0) / b))))
                if am is not None:
                    a = am[i]
                    assert np.all((a >= r0) & (a < r1)), "argmax row outside its chunk"
                    at = z64[a - r0, np.arange(cout)] + w[a - r0, np.arange(cout)]
                    worst = max(worst, note(fam + " pool", mode, float(np.max(np.maximum(elo - at, 0.0) / (2 * b)))))
                    if Zk is not None:
                        zk = Zk[r0:r1, :cout] * sg
                        assert np.array_equal(own(pmx[i]), Zk[a, np.arange(cout)]), "extreme != the kernel's own Z at its row"
                        assert np.array_equal(own(pmx[i]) * sg, zk.max(0)), "extreme is not the extreme of the kernel's own Z"
                    if c.get("dup") == qq:
                        assert np.all(a == r0), "tie rule: the first row of the chunk among equal extremes"
    return worst


def outputs_of(t):
    return {k: v for k, v in t.items() if k in ("Z",) or k.startswith(("part_", "fin_s", "fin_m", "fin_i", "pfin_s", "pfin_m", "pfin_i")) and k not in ("pfin_sum", "pfin_sq")}


def assert_refused(d, t, message):
    """AMPNET_E_ARG with `message`, nothing launched, every output still at its sentinel."""
    rc, names = PP.run_gemm(d)
    assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
    assert message in PP.last_error(), PP.last_error()
    for k, v in outputs_of(t).items():
        assert is_sentinel(v), f"{k} was written by a refused launch"


@pytest.mark.parametrize("name,mode,pair", fwd_params())
def test_pw_gemm_layer(name, mode, pair):
    c = fwd_case(name, mode)
    if c.get("chunk512") and mode.startswith("bf16"):
        pytest.skip("chunk512 hands the split-eligible shape the non-split chunking: there is no split kernel to refuse it outside f32x3")
    if c.get("pool") == "noarg" and mode.startswith("bf16"):
        with precision(mode):
            d, t, host, split = make_gemm(name, c, mode, 1234 + len(name), pair)
            assert_refused(d, t, POOL_EVAL_REFUSAL)
        return
    pipes = ["1", "0"] if mode == "fp32" and name in ("c64_64", "c128_128", "pool", "c64_40", "drop128") else [None]
    old = os.environ.get("AMPNET_PW_PIPE")
    try:
        for pipe in pipes:
            if pipe is not None:
                os.environ["AMPNET_PW_PIPE"] = pipe
            with precision(mode):
                d, t, host, split = make_gemm(name, c, mode, 1234 + len(name), pair)
                rc, names = PP.run_gemm(d)
                if c.get("chunk512") and rc == PP.AMPNET_E_ARG:
                    print(f"[pw layers] chunk512 {mode}: refused ({PP.last_error()})")
                    continue
                assert rc == 0, PP.last_error()
                first = snap(t)
                for v in outputs_of(t).values():                     # second run on re-poisoned outputs
                    v.copy_(nanbuf(*v.shape, dtype=v.dtype))
                rc2, _ = PP.run_gemm(d)
                assert rc2 == 0, PP.last_error()
                bitwise_equal(first, snap(t))
                w = check_gemm(name, c, mode, d, t, host, split, names)
                print(f"[pw layers] {name} {mode} pair={pair} pipe={pipe}: {names[0]}, worst error/bar {w:.4f}")
                assert w <= 1.0
    finally:
        if old is None:
            os.environ.pop("AMPNET_PW_PIPE", None)
        else:
            os.environ["AMPNET_PW_PIPE"] = old


def test_pw_gemm_bf16_tensor_refusals():
    """pw_gemm's own argument checks are the gate of the bf16 tensors (the hook adds none): a bf16 A or Z outside the bf16 modes, and a
    bf16 A whose rows are not 16-byte aligned (lda = 68), get AMPNET_E_ARG with pw_gemm's message and leave the outputs alone."""
    c = FWD["c64_64"]
    for mode in ("fp32", "f32x3"):
        for pair in ((1, 0), (0, 1)):
            with precision(mode):
                d, t, host, _ = make_gemm("c64_64", c, mode, 5, pair)
                assert_refused(d, t, "pw_gemm: bf16 tensors need a bf16 precision mode")
    with precision("bf16_store"):
        d, t, host, _ = make_gemm("c64_64", c, "bf16_store", 5, (1, 1))
        A68 = torch.zeros(host["rows"], 68, dtype=torch.bfloat16, device="cuda")
        A68[:, :64] = t["A"]
        d.A, d.A_n, d.lda = A68.data_ptr(), A68.numel(), 68
        assert_refused(d, t, "pw_gemm: bf16 A needs lda % 8 == 0")


def test_pw_gemm_probe_descriptor_without_the_tail():
    """A caller built against the descriptor that ended at pfin_out_n has tail (its pad0) == 0 and whatever memory follows its struct where
    a_bf16 / z_bf16 now are: the hook must not read them.  tail == 0 with both words set runs the fp32 kernel and gives the bits of the
    plain run; any other tail but 0 and 1 is refused."""
    c = FWD["c64_64"]
    with precision("fp32"):
        d, t, host, _ = make_gemm("c64_64", c, "fp32", 5)
        rc, names = PP.run_gemm(d)
        assert rc == 0 and names == [host["name"]], (rc, names, PP.last_error())
        first = snap(outputs_of(t))
        for v in outputs_of(t).values():
            v.copy_(nanbuf(*v.shape, dtype=v.dtype))
        d.tail, d.a_bf16, d.z_bf16 = 0, 0x5A5A5A5A, -1
        rc, names = PP.run_gemm(d)
        assert rc == 0 and names == [host["name"]], (rc, names, PP.last_error())
        bitwise_equal(first, snap(outputs_of(t)))
        for v in outputs_of(t).values():
            v.copy_(nanbuf(*v.shape, dtype=v.dtype))
        d.tail, d.a_bf16, d.z_bf16 = 2, 0, 0
        assert_refused(d, t, "probe_pw_gemm: tail = 2")


# ================================================================================================================================
# backward
# ================================================================================================================================
BWD = {
    # CX, CY, form: dense / gram / lin (prev without activation); add, drop, per-window, slot weights, fin
    "b128_128": dict(CX=128, CY=128, sizes=[1, 4, 31, 33, 127, 129, 255, 257, 700], S=3),
    "b128_gram": dict(CX=128, CY=128, gram=True, sizes=[257, 129, 31, 700, 4, 33], S=3),
    "b128_64": dict(CX=128, CY=64, sizes=[255, 257, 1, 127, 33, 700], S=3),
    "b128_64lin": dict(CX=128, CY=64, lin=True, sizes=[255, 31, 129], S=3),
    "b64_64": dict(CX=64, CY=64, sizes=[127, 129, 4, 700], S=2),
    "b64_64add": dict(CX=64, CY=64, add=True, sizes=[33, 257, 31, 255], S=2),
    "b64_64lin": dict(CX=64, CY=64, lin=True, add=True, sizes=[129, 1, 257, 31], S=2),
    "b64_128": dict(CX=64, CY=128, sizes=[255, 257, 33, 31], S=12 // 6),
    "b64_128drop": dict(CX=64, CY=128, drop=0.3, sizes=[129, 700, 4], S=3),
    "bmm64": dict(CX=64, CY=64, perwin=True, add=True, sizes=[512] * 6, S=3),
    "slotw": dict(CX=128, CY=128, gram=True, slotw=True, sizes=[127, 129, 255, 257, 31, 33, 4, 1, 700], S=9),
    "fin128_64": dict(CX=128, CY=64, fin=True, sizes=[255, 257, 129, 127], S=2),
    "wrap128": dict(CX=128, CY=128, sizes=[300] * 576, S=9),
}
BWD_MODES = ["fp32", "f32x3", "bf16_train", "bf16_store"]


def bwd_x3_expected(c):
    """pw_bwd_x3.hip pw_bwd_x3_supported, restated: 128 x 128 dense or Gram with an activated input, 128 x 64 dense, 64 x 64 dense with an
    activated input or an addend (no dropout), 64 x 128 dense with an activated input; per-window weights only on 64 x 64."""
    if c.get("slotw"):
        return True
    CX, CY = c["CX"], c["CY"]
    if c.get("perwin"):
        return CX == 64 and CY == 64
    if CX == 128 and CY == 128:
        return not c.get("lin")
    if CX == 128 and CY == 64:
        return not c.get("gram")
    if CX == 64 and CY == 64:
        return not c.get("gram") and not c.get("drop") and (not c.get("lin") or c.get("add"))
    return not c.get("gram") and not c.get("lin")


def bwd_name(c, mode):
    """The profile name of the kernel pw_bwd_fused dispatches to (launch_fused_x / launch_x3 / launch_x3n / launch_bf16_z)."""
    base = f"pw_bwd<{c['CX']},{c['CY']}>" + ("+gram" if c.get("gram") else "")
    if mode.startswith("bf16"):
        return base + " bf16"
    tail = (" lin" if c.get("lin") else "") + ("+add" if c.get("add") else "") + ("+drop" if c.get("drop") else "")
    return base + tail + (" x3" if mode == "f32x3" and bwd_x3_expected(c) else "")


def make_bwd(name, c, mode, seed):
    g = rng(seed)
    CX, CY, S = c["CX"], c["CY"], c["S"]
    sizes = c["sizes"]
    Q = len(sizes)
    wo = offsets(sizes)
    rows, max_rows = int(wo[-1]), max(sizes)
    zb = mode == "bf16_store"
    h = dict(CX=CX, CY=CY, n_slots=S, win_off=wo, act=1 if c.get("gram") else 0)
    rnd = lambda *s: f32(g.standard_normal(s))
    pz = rnd(rows, CY)
    gz = pz if c.get("gram") else rnd(rows, CX)
    if zb:                                                      # the float64 reference reads the bf16-rounded z tensors
        pz = torch.from_numpy(pz).bfloat16().float().numpy()
        gz = pz if c.get("gram") else torch.from_numpy(gz).bfloat16().float().numpy()
    h["pz"], h["gz"] = pz, gz
    if not c.get("gram"):
        h["dy"] = rnd(rows, CX)
        h["P1"] = f32(g.uniform(0.5, 1.5, (S, CX)))
        h["P2"] = f32(g.uniform(-0.2, 0.2, (S, CX)))
        h["P3"] = f32(g.uniform(-0.2, 0.2, (S, CX)))
    if not c.get("lin"):
        gam = f32(g.uniform(0.5, 1.5, (S, CY)))
        mean = f32(g.uniform(-0.2, 0.2, (S, CY)))
        inv = f32(g.uniform(0.8, 1.2, (S, CY)))
        beta = f32(g.uniform(-0.2, 0.2, (S, CY)))
        s = f32(gam * inv)
        h["ps"], h["pt"] = s, f32(beta - mean * s)
        h["prev_mean"], h["prev_invstd"] = mean, inv
        if c.get("gram"):                                     # Gram: x and y are the same activated tensor relu(z s + t)
            h["P2"], h["P3"] = h["ps"], h["pt"]
    if c.get("drop"):
        h["drop_p"], h["drop_key"] = c["drop"], (seed, 5)
    d = PP.PwBwdProbe()
    d.kind, d.CX, d.CY, d.act, d.Q, d.n_slots, d.max_rows = 0, CX, CY, h["act"], Q, S, max_rows
    pl = PP.plan(Q, S, max_rows)
    if c.get("perwin"):
        ws = CY * CX
        h["W"] = f32(g.uniform(-1, 1, (Q, CY, CX)) / np.sqrt(CX))
        h["w_win_stride"], h["perwin_slot_major"] = ws, 1
        d.w_win_stride, d.perwin_slot_major = ws, 1
        cpw = -(-max_rows // pl.bwd_item_rows)
        d.items_per_block = 1
        d.blocks_per_slot = (Q // S) * cpw
    elif c.get("slotw"):
        h["W"] = f32(g.uniform(-1, 1, (S, CX, CY)) / np.sqrt(CX))
        h["ldw"], h["w_slot_stride"] = CY, CX * CY
        d.ldw, d.w_slot_stride = CY, CX * CY
        h["bias_slot"] = f32(g.uniform(-0.3, 0.3, (S, CY)))
        d.blocks_per_slot = pl.bwd_blocks
    else:
        h["W"] = f32(g.uniform(-1, 1, (CX, CY)) / np.sqrt(CX))
        h["ldw"] = CY
        d.ldw = CY
        d.blocks_per_slot = pl.bwd_blocks
    if c.get("add"):
        h["add"] = rnd(rows, CY)
    d.drop_p = c.get("drop", 0.0)
    if c.get("drop"):
        d.drop_seed = PP.drop_base(*h["drop_key"])
    grid = d.blocks_per_slot * S
    zdt = torch.bfloat16 if zb else torch.float32
    t = dict(gz=dev(h["gz"], zdt), pz=dev(h["pz"], zdt), W=dev(h["W"]), win_off=dev(wo, torch.int32),
             out=nanbuf(rows, CY), dWpart=nanbuf(grid + S, CX, CY), dbpart=nanbuf(grid + S, CX))
    if c.get("gram"):
        t["gz"] = t["pz"]
    d.g_z_bf16 = d.prev_z_bf16 = 1 if zb else 0
    for k in ("dy", "P1", "P2", "P3", "ps", "pt", "prev_mean", "prev_invstd", "bias_slot", "add"):
        if h.get(k) is not None:
            t[k] = dev(h[k])
    if h.get("prev_mean") is not None:
        t["part_a"], t["part_b"] = nanbuf(grid + S, CY), nanbuf(grid + S, CY)
    if c.get("fin"):
        P = 3 * S
        fa, fb = rnd(P, CX) * 10, rnd(P, CX) * 10
        fg = f32(g.uniform(0.5, 1.5, CX))
        fm, fi = f32(g.uniform(-0.2, 0.2, (S, CX))), f32(g.uniform(0.8, 1.2, (S, CX)))
        n_slot_rows = [int(sum(sizes[q] for q in range(Q) if q % S == sl)) for sl in range(S)]
        assert len(set(n_slot_rows)) == 1
        h["fin"] = (fa, fb, fg, fm, fi, n_slot_rows[0])
        fg_pad = np.zeros((S, CX), np.float32)                 # (one extent covers gamma [CX] and mean / invstd [n_slots, CX])
        fg_pad[0] = fg
        t.update(fin_part_a=dev(fa), fin_part_b=dev(fb), fin_gamma=dev(fg_pad), fin_mean=dev(fm), fin_invstd=dev(fi))
        for k in ("P1", "P2", "P3"):
            t["fin_" + k] = nanbuf(S, CX, 2)
        t["fin_slot_ab"] = nanbuf(S, CX, 2)
        d.fin_parts, d.fin_rows = P, n_slot_rows[0]
        t.pop("P1"), t.pop("P2"), t.pop("P3")
        t["P1"], t["P2"], t["P3"] = nanbuf(S, CX), nanbuf(S, CX), nanbuf(S, CX)    # outputs then (kernels.h: PwBwd.fin_*)
    PP.set_tensors(d, PP.BWD_EXTENTS, **t)
    return d, t, h, grid


def check_bwd(name, c, mode, d, t, h, grid, names):
    fam = "pw_bwd"
    eps = PP.EPS16 if mode.startswith("bf16") else PP.EPS32
    S, CX, CY = c["S"], c["CX"], c["CY"]
    assert names == [bwd_name(c, mode)], (names, bwd_name(c, mode))   # the intended instantiation ran
    if mode == "f32x3":                                             # and the library's own predicate agrees with the restatement
        assert bwd_x3_expected(c) == (PP.plan(d.Q, S, d.max_rows, bwd=d).bwd_x3 == 1)
    worst = 0.0
    if c.get("fin"):
        fa, fb, fg, fm, fi, n = h["fin"]
        for sl in range(S):
            A_, B_ = fa[sl::S].astype(np.float64).sum(0), fb[sl::S].astype(np.float64).sum(0)
            sv = fg.astype(np.float64) * fi[sl]
            p2 = -sv * fi[sl] * B_ / n
            p3 = -sv * A_ / n - p2 * fm[sl]
            K = len(fa[sl::S])
            ma = np.abs(fa[sl::S]).sum(0)
            mb = np.abs(fb[sl::S]).sum(0)
            ab = t["fin_slot_ab"].cpu().numpy()[sl]
            worst = max(worst, note(fam + " fin", mode, PP.ratio(ab[:, 0], A_, ma, K)))
            worst = max(worst, note(fam + " fin", mode, PP.ratio(ab[:, 1], B_, mb, K)))
            got = {k: t["fin_" + k].cpu().numpy().reshape(-1)[sl * CX:(sl + 1) * CX] for k in ("P1", "P2", "P3")}
            worst = max(worst, note(fam + " fin", mode, PP.ratio(got["P1"], sv, np.abs(sv), 1)))
            worst = max(worst, note(fam + " fin", mode, PP.ratio(got["P2"], p2, np.abs(sv * fi[sl]) * mb / n, K)))
            worst = max(worst, note(fam + " fin", mode, PP.ratio(got["P3"], p3, np.abs(sv) * ma / n + np.abs(sv * fi[sl]) * mb / n * np.abs(fm[sl]), K)))
        # the data path then runs on the constants the kernel formed: its own outputs, held to float64 above
        h = dict(h)
        for k in ("P1", "P2", "P3"):
            h[k] = t["fin_" + k].cpu().numpy().reshape(-1)[:S * CX].reshape(S, CX)
    ref = PP.bwd_ref(h)
    rows = len(PP.win_of_rows(h["win_off"]))
    out = t["out"].cpu().numpy()
    worst = max(worst, note(fam, mode, PP.ratio(out, ref["out"], ref["out_m"], CX, eps)))
    assert is_sentinel(t["dWpart"][grid:]) and is_sentinel(t["dbpart"][grid:]), "partials past the grid were written"
    dW = PP.slot_sums(t["dWpart"].cpu().numpy()[:grid], S, (CX, CY))
    for sl in range(S):
        K = ref["rows"][sl]
        worst = max(worst, note(fam + " dW", mode, PP.ratio(dW[sl], ref["dW"][sl], ref["dW_m"][sl], K, eps)))
    db = PP.slot_sums(t["dbpart"].cpu().numpy()[:grid], S, (CX,))
    worst = max(worst, note(fam + " db", mode, max(PP.ratio(db[sl], ref["db"][sl], ref["db_m"][sl], ref["rows"][sl], eps) for sl in range(S))))
    if "part_a" in t:
        assert is_sentinel(t["part_a"][grid:]), "partials past the grid were written"
        pa = PP.slot_sums(t["part_a"].cpu().numpy()[:grid], S, (CY,))
        pb = PP.slot_sums(t["part_b"].cpu().numpy()[:grid], S, (CY,))
        for sl in range(S):
            K = ref["rows"][sl] * CX
            worst = max(worst, note(fam + " bnsums", mode, PP.ratio(pa[sl], ref["pa"][sl], ref["pa_m"][sl], K, eps)))
            worst = max(worst, note(fam + " bnsums", mode, PP.ratio(pb[sl], ref["pb"][sl], ref["pb_m"][sl], K, eps)))
    del rows
    return worst


@pytest.mark.parametrize("mode", BWD_MODES)
@pytest.mark.parametrize("name", list(BWD))
def test_pw_bwd_layer(name, mode):
    c = BWD[name]
    if c.get("fin") and mode.startswith("bf16"):
        pytest.skip("in-kernel BatchNorm-backward constants are built for the fp32 kernels only (pw_bwd_fused refuses them in bf16)")
    with precision(mode):
        w = run_bwd_case(name, c, mode, 4321 + len(name))
    assert w <= 1.0


def run_bwd_case(name, c, mode, seed):
    """One fused-backward case in the CURRENT matrix precision `mode`: run, re-poison, run again (bitwise equal), check; the worst
    error / bar."""
    d, t, h, grid = make_bwd(name, c, mode, seed)
    rc, names = PP.run_bwd(d)
    assert rc == 0, PP.last_error()
    first = snap(t)
    for k in ("out", "dWpart", "dbpart", "part_a", "part_b", "fin_P1", "fin_P2", "fin_P3", "fin_slot_ab"):
        if k in t:
            t[k].copy_(nanbuf(*t[k].shape))
    if c.get("fin"):
        for k in ("P1", "P2", "P3"):
            t[k].copy_(nanbuf(*t[k].shape))
    rc2, _ = PP.run_bwd(d)
    assert rc2 == 0, PP.last_error()
    bitwise_equal(first, snap(t))
    w = check_bwd(name, c, mode, d, t, h, grid, names)
    print(f"[pw layers] {name} {mode}: {names[0]}, worst error/bar {w:.4f}")
    return w


def test_probe_refuses_short_buffers():
    """A wrong test gets AMPNET_E_ARG, not an out-of-bounds access: Z one row short, dWpart one workgroup short, win_off descending,
    the previous layer's scale without its shift, pfin_rows one partial short."""
    with precision("fp32"):
        d, t, host, _ = make_gemm("c64_64", FWD["c64_64"], "fp32", 5)
        d.Z_n = d.Z_n - d.ldz
        rc, names = PP.run_gemm(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        d, t, h, grid = make_bwd("b64_64", BWD["b64_64"], "fp32", 5)
        d.dW_n = d.dW_n - (d.dW_n - (grid - 1) * 64 * 64)
        rc, names = PP.run_bwd(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        d, t, h, grid = make_bwd("b64_64", BWD["b64_64"], "fp32", 5)
        t["win_off"][1] = int(t["win_off"][2]) + 1
        rc, names = PP.run_bwd(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        d, t, h, grid = make_bwd("b64_64", BWD["b64_64"], "fp32", 5)
        d.pt = None                                               # prev scale without its shift: every fused kernel would read it
        rc, names = PP.run_bwd(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        d, t, host, _ = make_gemm("pfin", FWD["pfin"], "fp32", 5)
        d.pfin_rows_n = d.pfin_parts - 1
        rc, names = PP.run_gemm(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
