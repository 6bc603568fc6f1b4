"""Layer-local float64 parity of the max-pooled layers' backward (csrc/bwd_misc.hip: pool_bwd, slot_mats, sparse_scatter, sparse_rows,
sparse_fix, pooled_wgrad, reduce_slots / reduce_slots2), of the unfused pw_dgrad / pw_wgrad (csrc/pw_bwd.hip) and of the input layers'
weight gradient (pw_input_wgrad, input_param_grads).

Each kernel is launched ONCE through a test hook (include/ampnet_hip.h, "test hooks": ampnet_probe_pooled_bwd_f32, ampnet_probe_pw_bwd_f32
kinds 1 / 2, ampnet_probe_input_wgrad_f32) and every output is held to a float64 restatement of its contract (kernels.h / bwd_misc.h) on the
fp32 inputs it read -- bf16-rounded where it reads a bf16 z -- with pw_probe.bar and K = that output's own contraction length.  Every case
also checks NaN sentinels where the contract does not write, a bitwise-identical second run, and the path that ran: profile names where the
product instruments the launch (pw_dgrad / pw_wgrad, the small-GEMM launches of slot_mats for n_slots <= 9 and of pooled_wgrad with wgram);
slot_mats_kernel and pooled_wgrad's Gram-row walk show as the absence of that launch; sparse_scatter_kernel<true> is told from <false> by
its result (a bf16 z_prev read as fp32 is garbage, far outside the bar).

Layer cases compose the kernels in the order EncBwd::pooled_layer (csrc/encoder_bwd.hip) launches them, fused and unfused, and hold the
result to pooled_layer_ref (torch float64 autograd of the whole layer).  Their bar is propagated by a magnitude pass: the same float64
restatement on the absolute values of every operand, with K = the sum of the contraction lengths along the path and the constant of
pw_probe.bar (8 eps sqrt(K) |.| + 2 eps |x|), the same for every case.

Every family also runs its check against a reference with one small realistic defect and must report error / bar > 1 there: a window or a
row left out of a sum (pool_bwd's slot sums, the Gram and column sums, reduce_slots' partials, pw_wgrad, pw_input_wgrad, input_param_grads'
dW), P1 from the neighbouring slot, one output row scaled by (1 + 1e-4) (the Gram launch's and pw_dgrad's data gradient; 1 + 1e-3 for
slot_mats' G), a merged channel's contribution dropped (sparse_rows, sparse_scatter, sparse_fix) or one window's share of the BatchNorm sums
dropped, the P3 (x) asum term left out (pooled_wgrad), dT written at window q instead of its slot-major row, and the tie rule flipped to the
last row (the whole layer).  The families whose bar takes the bf16 unit roundoff in the bf16 modes (the Gram launch, the Gram and column
sums, the whole layer) run their defect checks in fp32 and f32x3 only: there the bar of a K ~ 1e4 contraction is wider than any one row or
window.

Not covered (no caller): the sparse GradSrc (arg / dpool) of pw_dgrad / pw_wgrad -- EncBwd::sparse() has no call site -- and
PwDgrad.rowmap / srows, which nothing in csrc/ sets.  Global-batch BatchNorm (sync_bn_bwd_constants inside pool_bwd) needs a process group:
tests/test_syncbn_layers_gpu.py holds it to pool_bwd_global_ref below on two ranks.
"""
import numpy as np
import pytest
import torch

import pw_probe as PP
from test_pw_layers_gpu import bitwise_equal, dev, f32, is_sentinel, nanbuf, offsets, precision, snap

pytestmark = pytest.mark.gpu
WORST = {}
C, CP = 256, 128


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[pooled bwd] worst error/bar {k}: {WORST[k]:.4f}")


def note(family, mode, r):
    key = f"{family} {mode}"
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def teeth(x, want_bad, mag, K, eps=PP.EPS32):
    """the check of a family against a reference with one defect must fail it"""
    r = PP.ratio(x, want_bad, mag, K, eps)
    assert r > 1.0, f"the bar does not see the defect (error/bar {r:.3f})"


def prow_of(q, Q, S, slot_major):
    return (q % S) * (Q // S) + q // S if slot_major else q


# ================================================================================================================================
# inputs of one max-pooled layer: z_prev [rows, 128] -> relu(bn_prev) -> W [256, 128] -> BN (per-slot batch statistics) -> ReLU -> max
# ================================================================================================================================
POOL = {
    # sizes: window rows; S slots; sm slot_major; zero: an empty window; one: one-row windows (all 256 channels on one row);
    # share: a few channels share a row among many distinct rows; tie: identical rows (exact ties); dead: channels zero over a window
    "s1": dict(sizes=[1, 4, 33, 257, 700, 129], S=1, sm=0, share=True),
    "s9": dict(sizes=[300] * 594, S=9, sm=1),                                 # 66 windows per slot; Q > 128 and not a multiple of 128
    "s10": dict(sizes=([1, 40, 700, 3, 129] * 2) * 13, S=10, sm=0, one=True, tie=True),    # 13 windows per slot
    "s12": dict(sizes=[31, 1, 200, 64, 700, 5, 17, 129, 2, 300, 77, 33] * 6, S=12, sm=1, dead=True, zero=True),
}


def pool_inputs(c, seed, zb=False):
    g = np.random.default_rng(seed)
    sizes, S = list(c["sizes"]), c["S"]
    Q = len(sizes)
    if c.get("zero"):
        sizes[5] = 0
    wo = offsets(sizes)
    rows = int(wo[-1])
    win = PP.win_of_rows(wo)
    slot = win % S
    zp = f32(g.standard_normal((rows, CP)))
    if c.get("tie"):                                            # window 1: rows 0 .. 5 identical, window 2: two identical rows
        zp[wo[1]:wo[1] + 6] = zp[wo[1]]
        zp[wo[2] + 3] = zp[wo[2] + 10]
    if zb:
        zp = torch.from_numpy(zp).bfloat16().float().numpy()
    gam_p, inv_p = f32(g.uniform(0.5, 1.5, (S, CP))), f32(g.uniform(0.8, 1.2, (S, CP)))
    mean_p, beta_p = f32(g.uniform(-0.2, 0.2, (S, CP))), f32(g.uniform(-0.2, 0.2, (S, CP)))
    s_p = f32(gam_p * inv_p)
    t_p = f32(beta_p - mean_p * s_p)
    W = f32(g.uniform(-1, 1, (C, CP)) / np.sqrt(CP))
    a = np.maximum(zp.astype(np.float64) * s_p[slot] + t_p[slot], 0.0)
    z32 = f32(a @ W.astype(np.float64).T)
    gamma = g.uniform(0.5, 1.5, C)
    gamma[::7] *= -1.0                                           # negative gamma: the argmax is the minimum
    beta = g.uniform(-0.3, 0.3, C)
    if c.get("dead"):
        beta[3::40] = -50.0                                      # relu(bn(z)) = 0 over every window: dpm = 0
    mean, invstd = np.zeros((S, C)), np.zeros((S, C))
    for s in range(S):
        zz = z32[slot == s].astype(np.float64)
        mean[s] = zz.mean(0)
        invstd[s] = 1.0 / np.sqrt(zz.var(0) + 1e-5)
    scale = f32(gamma * invstd)
    shift = f32(beta - mean * scale)
    arg = np.full((Q, C), -1, np.int32)
    zext = np.zeros((Q, C), np.float32)
    for q in range(Q):
        if sizes[q] == 0:
            continue
        zz = z32[wo[q]:wo[q + 1]]
        neg = scale[q % S] < 0
        i_max, i_min = zz.argmax(0), zz.argmin(0)                # numpy: the first index among equal values
        arg[q] = wo[q] + np.where(neg, i_min, i_max)
        zext[q] = z32[arg[q], np.arange(C)]
    if c.get("one"):
        assert sizes[0] == 1 and np.all(arg[0] == wo[0])
    if c.get("share"):
        # window 4 (700 rows): channels 10..13 and 200 share one row, 50 and 51 another, the rest distinct rows
        q = 4
        for chans, r in (([10, 11, 12, 13, 200], wo[q] + 5), ([50, 51], wo[q] + 600)):
            for ch in chans:
                arg[q, ch] = r
                zext[q, ch] = z32[r, ch]
    d_pooled = f32(g.standard_normal((Q, C)))
    return dict(sizes=sizes, S=S, Q=Q, sm=c["sm"], wo=wo, rows=rows, win=win, slot=slot, zp=zp, s_p=s_p, t_p=t_p, mean_p=mean_p,
                inv_p=inv_p, W=W, z32=z32, gamma=gamma, beta=beta, scale=scale, shift=shift, mean=f32(mean), invstd=f32(invstd),
                arg=arg, zext=zext, d_pooled=d_pooled, zb=zb)


def pool_ranks(cfgs, seeds, exact=False):
    """pool_inputs of every rank (its own windows and seed) under ONE BatchNorm: gamma and beta of rank 0 and the statistics of the ranks' rows
    together, per slot (every rank's window count is a multiple of S, so window q of any rank belongs to slot q % S of the whole batch).
    The sign of a channel's scale is the sign of its gamma, the same for every seed, so each rank's arg / zext stay the extremes the forward
    would have kept.  exact: the constants stay float64 (the CPU tests against autograd); otherwise fp32, as the kernels get them."""
    hs = [pool_inputs(c, s) for c, s in zip(cfgs, seeds)]
    S = hs[0]["S"]
    assert all(h["S"] == S and h["Q"] % S == 0 for h in hs)
    z, slot = np.concatenate([h["z32"] for h in hs]).astype(np.float64), np.concatenate([h["slot"] for h in hs])
    gamma, beta = hs[0]["gamma"], hs[0]["beta"]
    mean = np.stack([z[slot == s].mean(0) for s in range(S)])
    invstd = np.stack([1.0 / np.sqrt(z[slot == s].var(0) + 1e-5) for s in range(S)])
    scale = gamma * invstd
    cast =(lambda x: x) if exact else f32
    for h in hs:
        assert np.array_equal(h["scale"] < 0, scale < 0)
        h.update(gamma=gamma, beta=beta, scale=cast(scale), shift=cast(beta - mean * cast(scale)), mean=cast(mean), invstd=cast(invstd))
    return hs


# ---- float64 restatements ------------------------------------------------------------------------------------------------------
def pool_bwd_ref(h, neighbour_p1=False, skip_window=None):
    """pool_bwd (kernels.h: PoolBwd): dpm[prow(q)] = d_pooled[prow(q)] where arg >= 0 and fmaf(zext, s, t) > 0 (exact in float64 as
    z s + t > 0); per slot A = sum dpm, Bs = sum dpm (zext - mean) invstd over the slot's windows, n = its rows; P1 = s, P2 = -s invstd Bs / n,
    P3 = -s A / n - P2 mean."""
    Q, S = h["Q"], h["S"]
    sc, sh, mu, inv = (h[k].astype(np.float64) for k in ("scale", "shift", "mean", "invstd"))
    dpm = np.zeros((Q, C))
    A, Bs, Am, Bm = (np.zeros((S, C)) for _ in range(4))
    n = np.zeros(S)
    for q in range(Q):
        s, pr = q % S, prow_of(q, Q, S, h["sm"])
        n[s] += h["sizes"][q]
        live = (h["arg"][q] >= 0) & (h["zext"][q] * sc[s] + sh[s] > 0)
        d = np.where(live, h["d_pooled"][pr], 0.0)
        dpm[pr] = d
        if q == skip_window:                                     # the defect: one window left out of the slot sums
            continue
        zh = (h["zext"][q] - mu[s]) * inv[s]
        A[s] += d
        Bs[s] += d * zh
        Am[s] += np.abs(d)
        Bm[s] += np.abs(d) * (np.abs(h["zext"][q]) + np.abs(mu[s])) * inv[s]
    nn = np.maximum(n, 1)[:, None]
    P1 = sc
    P2 = -sc * inv * Bs / nn
    P3 = -sc * A / nn - P2 * mu
    if neighbour_p1:
        P1 = np.roll(P1, 1, axis=0) if S > 1 else P1 * (1 + 1e-4)
    P2m = np.abs(sc * inv) * Bm / nn
    P3m = np.abs(sc) * Am / nn + P2m * np.abs(mu)
    return dict(dpm=dpm, P1=P1, P2=P2, P3=P3, A=A, Bs=Bs, Am=Am, Bm=Bm, P2m=P2m, P3m=P3m, n=n)


def pool_bwd_global_ref(hs):
    """pool_bwd under a collective (bwd_misc.hip: pool_bwd -> sync_bn_bwd_constants): hs = the ranks' pool_inputs, with the SAME forward
    constants (scale, shift, mean, invstd) on every rank.  dpm and slot_ab are each rank's own (`ranks` = the ranks' pool_bwd_ref); P1, P2, P3
    come from A, Bs and the window rows summed over the ranks, with bn_probe's bars of the exchange (allreduced, global_bwd_constants)."""
    import bn_probe as B
    assert all(np.array_equal(h[k], hs[0][k]) for h in hs for k in ("scale", "shift", "mean", "invstd"))
    ranks = [pool_bwd_ref(h) for h in hs]
    A = B.allreduced([r["A"] for r in ranks], [r["Am"] for r in ranks])
    Bs = B.allreduced([r["Bs"] for r in ranks], [r["Bm"] for r in ranks])
    res = B.global_bwd_constants(A, Bs, sum(r["n"] for r in ranks), hs[0]["scale"], hs[0]["invstd"], hs[0]["mean"])
    res["ranks"] = ranks
    return res


def act_prev(h, zp=None):
    zp = h["zp"] if zp is None else zp
    return np.maximum(zp.astype(np.float64) * h["s_p"][h["slot"]] + h["t_p"][h["slot"]], 0.0)


def sparse_ref(h, dpm, P1, drop_merged=False):
    """the scattered rows (kernels.h, SparseScatter / SparseRows + SparseFix): out[row] += mask(row) * sum over the channels c whose argmax
    is `row` of P1[c] dpm[c] W[c][:], and per window part_a = sum of the added values, part_b = sum of added * (z_prev - mean) invstd."""
    Q, S, W = h["Q"], h["S"], h["W"].astype(np.float64)
    add, addm = np.zeros((h["rows"], CP)), np.zeros((h["rows"], CP))
    pa, pb, pam, pbm = (np.zeros((Q, CP)) for _ in range(4))
    zp = h["zp"].astype(np.float64)
    for q in range(Q):
        s, pr = q % S, prow_of(q, Q, S, h["sm"])
        coef = P1[s] * dpm[pr]
        seen = set()
        for ch in range(C):
            r = h["arg"][q, ch]
            if r < 0:
                continue
            if drop_merged and r in seen:
                continue
            seen.add(r)
            add[r] += coef[ch] * W[ch]
            addm[r] += np.abs(coef[ch] * W[ch])
        rows = sorted(seen)
        if rows:
            rr = np.array(rows)
            m = zp[rr] * h["s_p"][s] + h["t_p"][s] > 0
            add[rr] = np.where(m, add[rr], 0.0)
            addm[rr] = np.where(m, addm[rr], 0.0)
            zh = (zp[rr] - h["mean_p"][s]) * h["inv_p"][s]
            zhm = (np.abs(zp[rr]) + np.abs(h["mean_p"][s])) * h["inv_p"][s]
            pa[q], pb[q] = add[rr].sum(0), (add[rr] * zh).sum(0)
            pam[q], pbm[q] = addm[rr].sum(0), (addm[rr] * zhm).sum(0)
    return dict(add=add, addm=addm, pa=pa, pb=pb, pam=pam, pbm=pbm)


def gram_ref(h, zp=None):
    a = act_prev(h, zp)
    S = h["S"]
    return (np.stack([a[h["slot"] == s].T @ a[h["slot"] == s] for s in range(S)]),
            np.stack([a[h["slot"] == s].sum(0) for s in range(S)]), a)


def pooled_wgrad_ref(h, P1, P2, P3, dpm, gram, asum, drop_p3=False):
    """dW = sum_s diag(P2[s]) W Gram[s] + P3[s] (x) asum[s] + sum_q P1 dpm (x) a[arg] (kernels.h, PooledWgrad)."""
    Q, S, W = h["Q"], h["S"], h["W"].astype(np.float64)
    dW, dWm = np.zeros((C, CP)), np.zeros((C, CP))
    for s in range(S):
        dW += P2[s][:, None] * (W @ gram[s]) + (0 if drop_p3 else P3[s][:, None] * asum[s][None, :])
        dWm += np.abs(P2[s])[:, None] * (np.abs(W) @ np.abs(gram[s])) + np.abs(P3[s])[:, None] * np.abs(asum[s])[None, :]
    a = act_prev(h)
    for q in range(Q):
        s, pr = q % S, prow_of(q, Q, S, h["sm"])
        ok = h["arg"][q] >= 0
        coef = np.where(ok, P1[s] * dpm[pr], 0.0)
        rows = np.where(ok, h["arg"][q], 0)
        dW += coef[:, None] * a[rows]
        dWm += np.abs(coef)[:, None] * a[rows]
    return dW, dWm


def dense_dgrad_ref(h, G, c0, mag=False):
    """out = (a G[slot] + c0[slot]) masked by relu(bn_prev)."""
    a = act_prev(h)
    sl = h["slot"]
    if mag:
        v = np.einsum("rj,rjk->rk", a, np.abs(G)[sl]) + np.abs(c0)[sl]
    else:
        v = np.einsum("rj,rjk->rk", a, G[sl]) + c0[sl]
    m = h["zp"].astype(np.float64) * h["s_p"][sl] + h["t_p"][sl] > 0
    return np.where(m, v, 0.0)


def bn_sums(h, out, outm):
    """per-slot (sum dy, sum dy zhat_prev) of dy_prev and their magnitudes."""
    S, sl = h["S"], h["slot"]
    zp = h["zp"].astype(np.float64)
    zh = (zp - h["mean_p"][sl]) * h["inv_p"][sl]
    zhm = (np.abs(zp) + np.abs(h["mean_p"][sl])) * h["inv_p"][sl]
    f = lambda x: np.stack([x[sl == s].sum(0) for s in range(S)])
    return f(out), f(out * zh), f(outm), f(outm * zhm)


# ---- whole layer ------------------------------------------------------------------------------------------------------------------
def pooled_layer_ref(h, flip_ties=False):
    """torch float64 autograd of  z = relu(bn_prev(z_prev)) W^T;  pooled = maxpool_window(relu(bn(z)));  L = sum d_pooled . pooled.
    bn: per-slot batch statistics (biased variance, eps 1e-5); bn_prev: the fixed affine (s_prev, t_prev).  The argmax is the forward's
    (pool_finalize_kernel, csrc/pw_misc.hip): extreme z, the max for scale >= 0 and the min otherwise, the first row among equal values, -1
    for an empty window; z carries the fp32 values the kernels saw (z32) and the masks are the kernels' (z s + t > 0, exact in float64).
    Returns dW [256, 128], dy_prev [rows, 128] (masked), dy_prev's per-slot (sum dy, sum dy zhat_prev), and dgamma / dbeta of bn."""
    Q, S, sl = h["Q"], h["S"], torch.from_numpy(h["slot"])
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    zp = t(h["zp"])
    y_prev = (zp * t(h["s_p"])[sl] + t(h["t_p"])[sl]).requires_grad_(True)
    W = t(h["W"]).requires_grad_(True)
    gamma, beta = t(h["gamma"]).requires_grad_(True), t(h["beta"]).requires_grad_(True)
    a = torch.relu(y_prev)
    z = a @ W.T
    z = z + (t(h["z32"]) - z).detach()
    y = torch.zeros_like(z)
    for s in range(S):
        r = sl == s
        mu = z[r].mean(0)
        var = ((z[r] - mu) ** 2).mean(0)
        y[r] = (z[r] - mu) / torch.sqrt(var + 1e-5) * gamma + beta
    mask = torch.from_numpy(h["z32"].astype(np.float64) * h["scale"][h["slot"]] + h["shift"][h["slot"]] > 0)
    y = torch.where(mask, y, torch.zeros_like(y))
    arg = h["arg"].astype(np.int64).copy()
    if flip_ties:                                               # the defect: the LAST row among equal extremes
        for q in range(Q):
            if h["sizes"][q] == 0:
                continue
            zz = h["z32"][h["wo"][q]:h["wo"][q + 1]]
            ext = zz[arg[q] - h["wo"][q], np.arange(C)]
            last = len(zz) - 1 - np.argmax((zz == ext)[::-1], axis=0)
            arg[q] = h["wo"][q] + last
    L = torch.zeros((), dtype=torch.float64)
    for q in range(Q):
        ok = torch.from_numpy(arg[q] >= 0)
        rows = torch.from_numpy(np.where(arg[q] >= 0, arg[q], 0))
        pooled = torch.where(ok, y[rows, torch.arange(C)], torch.zeros(C, dtype=torch.float64))
        L = L + (t(h["d_pooled"][prow_of(q, Q, S, h["sm"])]) * pooled).sum()
    L.backward()
    dy = y_prev.grad.numpy()
    zh = (h["zp"].astype(np.float64) - h["mean_p"][h["slot"]]) * h["inv_p"][h["slot"]]
    sa = np.stack([dy[h["slot"] == s].sum(0) for s in range(S)])
    sb = np.stack([(dy * zh)[h["slot"] == s].sum(0) for s in range(S)])
    return dict(dW=W.grad.numpy(), dy=dy, sa=sa, sb=sb, dgamma=gamma.grad.numpy(), dbeta=beta.grad.numpy())


def layer_mags(h, pr):
    """the magnitude pass of the whole layer: the float64 restatement on absolute operands -- dz = P1 dy_sparse + P2 z + P3 per row with
    |z| = |a| |W|^T and |P2|, |P3| the magnitudes of their own sums (pool_bwd_ref: P2m, P3m), dW = |dz|^T |a|, dy_prev = |dz| |W| masked,
    and the sums over those -- and K = the sum of the contraction lengths (rows of the largest slot + C + cp + windows per slot).  The
    bar is then pw_probe.bar with its constant 8 and these magnitudes, unchanged for every case and mode."""
    sl = h["slot"]
    a = act_prev(h)
    W = np.abs(h["W"].astype(np.float64))
    zm = a @ W.T
    dzm = pr["P2m"][sl] * zm + pr["P3m"][sl]
    sp = np.zeros((h["rows"], C))
    for q in range(h["Q"]):
        ok = h["arg"][q] >= 0
        sp[h["arg"][q][ok], np.arange(C)[ok]] += np.abs(h["scale"][q % h["S"]][ok] * pr["dpm"][prow_of(q, h["Q"], h["S"], h["sm"])][ok])
    dzm = dzm + sp
    m = h["zp"].astype(np.float64) * h["s_p"][sl] + h["t_p"][sl] > 0
    dym = np.where(m, dzm @ W, 0.0)
    _, _, sam, sbm = bn_sums(h, dym, dym)
    K = max(np.bincount(sl, minlength=h["S"])) + C + CP + h["Q"] // h["S"]
    return dict(dW=dzm.T @ a, dy=dym, sa=sam, sb=sbm, dgamma=pr["Bm"].sum(0), dbeta=pr["Am"].sum(0), K=K)


# ================================================================================================================================
# the probe launches
# ================================================================================================================================
def pdesc(h, op, **t):
    d = PP.PooledBwdProbe()
    d.op, d.Q, d.n_slots, d.C, d.cp, d.slot_major, d.z_bf16 = op, h["Q"], h["S"], C, CP, h["sm"], 1 if h["zb"] else 0
    PP.set_tensors(d, PP.POOL_EXTENTS, **t)
    return d


def launch(d, outs, fn=PP.run_pooled):
    """run, re-poison the outputs, run again: bitwise equal; the kernel names of the first run"""
    before = {k: v.clone() for k, v in outs.items()}
    rc, names = fn(d)
    assert rc == 0, PP.last_error()
    first = snap(outs)
    for k, v in outs.items():
        v.copy_(before[k])
    rc2, _ = fn(d)
    assert rc2 == 0, PP.last_error()
    bitwise_equal(first, snap(outs))
    return names


def run_pool_bwd(h, t):
    S, Q = h["S"], h["Q"]
    o = dict(dpm=nanbuf(Q, C), P1=nanbuf(S, C), P2=nanbuf(S, C), P3=nanbuf(S, C), slot_ab=nanbuf(S, C, 2))
    d = pdesc(h, 0, win_off=t["win_off"], arg=t["arg"], zext=t["zext"], d_pooled=t["d_pooled"], scale=t["scale"], shift=t["shift"],
              mean=t["mean"], invstd=t["invstd"], **o)
    names = launch(d, o)
    assert names == [], names
    return {k: v.cpu().numpy().astype(np.float64) for k, v in o.items()}


def check_pool_bwd(h, k, mode="fp32"):
    pr = pool_bwd_ref(h)
    assert np.array_equal(k["dpm"], pr["dpm"]), "dpm differs from the masked pooled gradient"
    K = h["Q"] // h["S"]
    w = 0.0
    w = max(w, PP.ratio(k["slot_ab"][..., 0], pr["A"], pr["Am"], K), PP.ratio(k["slot_ab"][..., 1], pr["Bs"], pr["Bm"], K))
    w = max(w, PP.ratio(k["P1"], pr["P1"], np.abs(pr["P1"]), 1))
    w = max(w, PP.ratio(k["P2"], pr["P2"], pr["P2m"], K), PP.ratio(k["P3"], pr["P3"], pr["P3m"], K))
    teeth(k["P1"], pool_bwd_ref(h, neighbour_p1=True)["P1"], np.abs(pr["P1"]), 1)
    q0 = next(q for q in range(h["Q"]) if np.any(pr["dpm"][prow_of(q, h["Q"], h["S"], h["sm"])] != 0))
    bad = pool_bwd_ref(h, skip_window=q0)
    teeth(k["slot_ab"][..., 0], bad["A"], pr["Am"], K)
    teeth(k["slot_ab"][..., 1], bad["Bs"], pr["Bm"], K)
    teeth(k["P2"], bad["P2"], pr["P2m"], K)
    teeth(k["P3"], bad["P3"], pr["P3m"], K)
    return note("pool_bwd", mode, w), pr


def dev_inputs(h):
    zdt = torch.bfloat16 if h["zb"] else torch.float32
    return dict(win_off=dev(h["wo"], torch.int32), arg=dev(h["arg"], torch.int32), zext=dev(h["zext"]), d_pooled=dev(h["d_pooled"]),
                scale=dev(h["scale"]), shift=dev(h["shift"]), mean=dev(h["mean"]), invstd=dev(h["invstd"]), W=dev(h["W"]),
                z_prev=dev(h["zp"], zdt), s_prev=dev(h["s_p"]), t_prev=dev(h["t_p"]), mean_prev=dev(h["mean_p"]), invstd_prev=dev(h["inv_p"]))


def run_slot_mats(h, t, P):
    S = h["S"]
    o = dict(G=nanbuf(S + 1, CP, CP), c0=nanbuf(S + 1, CP))
    d = pdesc(h, 1, W=t["W"], P2=P["P2"], P3=P["P3"], **o)
    d.G_n, d.c0_n = S * CP * CP, S * CP
    names = launch(d, o)
    assert names == (["sgemm_mfma"] if S <= 9 else []), names          # the small-GEMM launch, or slot_mats_kernel (uninstrumented)
    assert is_sentinel(o["G"][S:]) and is_sentinel(o["c0"][S:])
    G, c0 = o["G"][:S].cpu().numpy().astype(np.float64), o["c0"][:S].cpu().numpy().astype(np.float64)
    W, P2, P3 = h["W"].astype(np.float64), P["P2h"], P["P3h"]
    Gr = np.stack([W.T @ (P2[s][:, None] * W) for s in range(S)])
    Gm = np.stack([np.abs(W).T @ (np.abs(P2[s])[:, None] * np.abs(W)) for s in range(S)])
    w = max(PP.ratio(G, Gr, Gm, C), PP.ratio(c0, P3 @ W, np.abs(P3) @ np.abs(W), C))
    teeth(G, Gr * np.where(np.arange(CP) == 7, 1 + 1e-3, 1.0)[None, :, None], Gm, C)
    return note("slot_mats", "fp32", w), G, c0, Gm


# ================================================================================================================================
# the whole layer, in EncBwd::pooled_layer's order (csrc/encoder_bwd.hip, pooled_layer: pool_bwd; fused: slot_mats -> Gram pw_bwd_fused ->
# reduce_slots2 -> pooled_wgrad -> sparse_scatter; unfused: sparse_rows -> slot_mats -> pw_wgrad -> reduce_slots x2 -> pooled_wgrad ->
# pw_dgrad -> sparse_fix)
# ================================================================================================================================
def scale_row(want, mag, f=1e-4):
    """the defect 'one output row scaled by (1 + f)': the row where the value stands out most against its magnitude"""
    bad = want.copy()
    r = int(np.argmax(np.max(np.abs(want) / np.maximum(mag, 1e-300), axis=1)))
    bad[r] *= 1 + f
    return bad


def check_reduce(dWpart, dbpart, part_slot, gram, asum, S, mode):
    """reduce_slots / reduce_slots2: out[s] = the float64 sum of the partials that belong to slot s; the defect: one partial left out"""
    w = 0.0
    for part, got in ((dWpart.cpu().numpy(), gram), (dbpart.cpu().numpy(), asum)):
        p = part.astype(np.float64)
        want = np.stack([p[part_slot == s].sum(0) for s in range(S)])
        mag = np.stack([np.abs(p[part_slot == s]).sum(0) for s in range(S)])
        K = int(np.bincount(part_slot, minlength=S).max())
        w = max(w, PP.ratio(got, want, mag, K))
        i0 = max(np.nonzero(part_slot == 0)[0], key=lambda i: np.abs(p[i]).sum())
        bad = want.copy()
        bad[0] -= p[i0]
        teeth(got, bad, mag, K)
    return note("reduce_slots", mode, w)


def check_gram(h, gram, asum, gr, asr, a, fam, mode, eps):
    """per-slot Gram and column sums of a = relu(bn_prev(z_prev)) (a >= 0: each is its own magnitude); the defect: one window of slot 0
    left out (checked at the fp32 bar: with bf16 operands the bar of K ~ 2e4 rows is wider than any one window)"""
    S = h["S"]
    rows_s = np.bincount(h["slot"], minlength=S)
    w = max(max(PP.ratio(gram[s], gr[s], gr[s], rows_s[s], eps), PP.ratio(asum[s], asr[s], asr[s], rows_s[s], eps)) for s in range(S))
    if eps == PP.EPS32:
        q0 = max(range(0, h["Q"], S), key=lambda q: h["sizes"][q])
        aw = a[h["wo"][q0]:h["wo"][q0 + 1]]
        teeth(gram[0], gr[0] - aw.T @ aw, gr[0], rows_s[0])
        teeth(asum[0], asr[0] - aw.sum(0), asr[0], rows_s[0])
    return note(fam, mode, w)


def layer(name, mode, fused, seed, wgram=True):
    c = POOL[name]
    eps = PP.EPS16 if mode.startswith("bf16") else PP.EPS32
    h = pool_inputs(c, seed, zb=mode == "bf16_store")
    S, Q, rows = h["S"], h["Q"], h["rows"]
    t = dev_inputs(h)
    kp = run_pool_bwd(h, t)
    w_pool, pr = check_pool_bwd(h, kp, mode)
    P = {k: dev(kp[k].astype(np.float32)) for k in ("P1", "P2", "P3")}
    P.update(P2h=kp["P2"], P3h=kp["P3"])
    dpm = dev(kp["dpm"].astype(np.float32))
    sa = dev(kp["slot_ab"].astype(np.float32))
    w_sm, G, c0, Gm = run_slot_mats(h, t, P)
    worst = {"pool_bwd": w_pool, "slot_mats": w_sm}
    Gt, c0t = dev(G.astype(np.float32)), dev(c0.astype(np.float32))
    gr, asr, a = gram_ref(h)
    out = nanbuf(rows, CP)
    if fused:
        # the Gram pw_bwd_fused (encoder_bwd.hip: pooled_layer, "if (fused)")
        d = PP.PwBwdProbe()
        pl = PP.plan(Q, S, max(h["sizes"]))
        d.kind, d.CX, d.CY, d.act, d.Q, d.n_slots, d.max_rows = 0, CP, CP, 1, Q, S, max(h["sizes"])
        d.ldw, d.w_slot_stride, d.blocks_per_slot = CP, CP * CP, pl.bwd_blocks
        d.g_z_bf16 = d.prev_z_bf16 = 1 if h["zb"] else 0
        nblk = d.blocks_per_slot * S
        bt = dict(gz=t["z_prev"], pz=t["z_prev"], P2=t["s_prev"], P3=t["t_prev"], ps=t["s_prev"], pt=t["t_prev"], prev_mean=t["mean_prev"],
                  prev_invstd=t["invstd_prev"], W=Gt, bias_slot=c0t, win_off=t["win_off"], out=out, dWpart=nanbuf(nblk, CP, CP),
                  dbpart=nanbuf(nblk, CP), part_a=nanbuf(nblk + Q, CP), part_b=nanbuf(nblk + Q, CP))
        PP.set_tensors(d, PP.BWD_EXTENTS, **bt)
        d.pab_n = nblk * CP
        names = launch(d, {k: bt[k] for k in ("out", "dWpart", "dbpart", "part_a", "part_b")}, PP.run_bwd)
        assert len(names) == 1 and names[0].startswith("pw_bwd<128,128>+gram"), names
        dense = out.cpu().numpy().astype(np.float64)
        want = dense_dgrad_ref(h, G, c0)
        wm = dense_dgrad_ref(h, Gm, np.abs(c0), mag=True)
        worst["gram_bwd out"] = note("gram pw_bwd out", mode, PP.ratio(dense, want, wm, CP, eps))
        if eps == PP.EPS32:
            teeth(dense, scale_row(want, wm), wm, CP)
        # reduce_slots2: Gram and column sums per slot
        o = dict(gram=nanbuf(S, CP, CP), asum=nanbuf(S, CP))
        d2 = pdesc(h, 7, red_part0=bt["dWpart"], red_part1=bt["dbpart"], red_out0=o["gram"], red_out1=o["asum"])
        d2.chunks, d2.red_n0, d2.red_n1 = 1, CP * CP, CP
        d2.Q = nblk                                             # the partials of the persistent grid: index % n_slots = slot
        launch(d2, o)
        gram, asum = o["gram"].cpu().numpy().astype(np.float64), o["asum"].cpu().numpy().astype(np.float64)
        worst["reduce_slots"] = check_reduce(bt["dWpart"], bt["dbpart"], np.arange(nblk) % S, gram, asum, S, mode)
        worst["gram"] = check_gram(h, gram, asum, gr, asr, a, "gram", mode, eps)
        gpa, gpb = bt["part_a"], bt["part_b"]
        pa_off = nblk
    else:
        # sparse_rows (before slot_mats in the product; independent of it)
        so = dict(srows=nanbuf(Q * C, CP), srow_row=nanbuf(Q * C, dtype=torch.int32), srow_cnt=nanbuf(Q, dtype=torch.int32))
        d3 = pdesc(h, 3, arg=t["arg"], dpm=dpm, P1=P["P1"], W=t["W"], win_off=t["win_off"], **so)
        launch(d3, so)
        check_sparse_rows(h, kp, so)
        # pw_wgrad (Gram + column sums of a per window chunk), then reduce_slots x2
        chunk_rows, chunks = 256, -(-max(h["sizes"]) // 256)
        wt, wn = run_wgrad_gram(h, t, chunk_rows, chunks)
        worst["pw_wgrad"] = wn
        o = dict(gram=nanbuf(S, CP, CP))
        d2 = pdesc(h, 6, red_part0=wt["dWpart"], red_out0=o["gram"])
        d2.chunks, d2.red_n0 = chunks, CP * CP
        launch(d2, o)
        o2 = dict(asum=nanbuf(S, CP))
        d2b = pdesc(h, 6, red_part0=wt["dbpart"], red_out0=o2["asum"])
        d2b.chunks, d2b.red_n0 = chunks, CP
        launch(d2b, o2)
        gram, asum = o["gram"].cpu().numpy().astype(np.float64), o2["asum"].cpu().numpy().astype(np.float64)
        worst["reduce_slots"] = check_reduce(wt["dWpart"], wt["dbpart"], np.repeat(np.arange(Q), chunks) % S, gram, asum, S, mode)
        worst["gram"] = check_gram(h, gram, asum, gr, asr, a, "gram unfused", mode, eps)
        o.update(o2)
    # pooled_wgrad
    ow = dict(dW=nanbuf(C, CP))
    extra = dict(wgram=nanbuf(S, C, CP)) if wgram else {}
    d4 = pdesc(h, 5, W=t["W"], P1=P["P1"], P2=P["P2"], P3=P["P3"], gram=o["gram"], asum=o["asum"], arg=t["arg"], dpm=dpm,
               z_prev=t["z_prev"], s_prev=t["s_prev"], t_prev=t["t_prev"], win_off=t["win_off"], **ow, **extra)
    names = launch(d4, ow)
    assert names == (["sgemm_mfma"] if wgram else []), names
    dWk = ow["dW"].cpu().numpy().astype(np.float64)
    want, wm = pooled_wgrad_ref(h, kp["P1"], kp["P2"], kp["P3"], kp["dpm"], gram, asum)
    Kw = CP + S + Q
    worst["pooled_wgrad"] = note("pooled_wgrad" + (" wgram" if wgram else " walk"), mode, PP.ratio(dWk, want, wm, Kw))
    teeth(dWk, pooled_wgrad_ref(h, kp["P1"], kp["P2"], kp["P3"], kp["dpm"], gram, asum, drop_p3=True)[0], wm, Kw)
    sp = sparse_ref(h, kp["dpm"], kp["P1"])
    if fused:
        before = out.cpu().numpy().astype(np.float64)
        d5 = pdesc(h, 2, arg=t["arg"], dpm=dpm, P1=P["P1"], W=t["W"], z_prev=t["z_prev"], s_prev=t["s_prev"], t_prev=t["t_prev"],
                   mean_prev=t["mean_prev"], invstd_prev=t["invstd_prev"], win_off=t["win_off"], out=out,
                   part_a=gpa[pa_off:], part_b=gpb[pa_off:])
        d5.part_chunks, d5.slot_idx = 1, 0
        o5 = dict(out=out, pa=gpa, pb=gpb)
        launch(d5, o5)
        check_scatter(h, sp, before, out, gpa[pa_off:], gpb[pa_off:], 1, 0, mode, fused=True)
        pa_all = PP.slot_sums(gpa.cpu().numpy(), S, (CP,))
        pb_all = PP.slot_sums(gpb.cpu().numpy(), S, (CP,))
    else:
        chunks_d = -(-max(h["sizes"]) // 512)
        pc = chunks_d + 1
        pa_t, pb_t = nanbuf(Q * pc, CP), nanbuf(Q * pc, CP)
        d6 = PP.PwBwdProbe()
        d6.kind, d6.CX, d6.CY, d6.act, d6.Q, d6.n_slots, d6.max_rows = 1, CP, CP, 1, Q, S, max(h["sizes"])
        d6.ldw, d6.w_slot_stride, d6.cp, d6.part_chunks, d6.chunk_rows, d6.chunks = CP, CP * CP, CP, pc, 512, chunks_d
        bt = dict(gz=t["z_prev"], P2=t["s_prev"], P3=t["t_prev"], pz=t["z_prev"], ps=t["s_prev"], pt=t["t_prev"],
                  prev_mean=t["mean_prev"], prev_invstd=t["invstd_prev"], W=Gt, bias_slot=c0t, win_off=t["win_off"], out=out,
                  part_a=pa_t, part_b=pb_t)
        PP.set_tensors(d6, PP.BWD_EXTENTS, **bt)
        names = launch(d6, dict(out=out, pa=pa_t, pb=pb_t), PP.run_bwd)
        assert names == ["pw_dgrad<128,128>+act"], names
        dense = out.cpu().numpy().astype(np.float64)
        want = dense_dgrad_ref(h, G, c0)
        wm = dense_dgrad_ref(h, Gm, np.abs(c0), mag=True)
        worst["pw_dgrad out"] = note("pw_dgrad", mode, PP.ratio(dense, want, wm, CP))
        assert is_sentinel(pa_t.view(Q, pc, CP)[:, chunks_d]), "pw_dgrad wrote sparse_fix's partial slot"
        o7 = dict(out=out, pa=pa_t, pb=pb_t)
        d7 = pdesc(h, 4, srows=so["srows"], srow_row=so["srow_row"], srow_cnt=so["srow_cnt"], z_prev=t["z_prev"], s_prev=t["s_prev"],
                   t_prev=t["t_prev"], mean_prev=t["mean_prev"], invstd_prev=t["invstd_prev"], win_off=t["win_off"], out=out,
                   part_a=pa_t, part_b=pb_t)
        d7.part_chunks, d7.slot_idx = pc, chunks_d
        before = dense
        launch(d7, o7)
        check_scatter(h, sp, before, out, pa_t, pb_t, pc, chunks_d, mode, fused=False)
        q_of = np.repeat(np.arange(Q), pc)
        pa_np, pb_np = pa_t.cpu().numpy(), pb_t.cpu().numpy()
        pa_all = np.stack([pa_np[(q_of % S) == s].astype(np.float64).sum(0) for s in range(S)])
        pb_all = np.stack([pb_np[(q_of % S) == s].astype(np.float64).sum(0) for s in range(S)])
    # the whole layer against torch autograd, with the propagated bar
    ref = pooled_layer_ref(h)
    mg = layer_mags(h, pr)
    K = mg["K"]
    dyk = out.cpu().numpy().astype(np.float64)
    lw = 0.0
    lw = max(lw, PP.ratio(dWk, ref["dW"], mg["dW"], K, eps), PP.ratio(dyk, ref["dy"], mg["dy"], K, eps))
    lw = max(lw, PP.ratio(pa_all, ref["sa"], mg["sa"], K, eps), PP.ratio(pb_all, ref["sb"], mg["sb"], K, eps))
    slab = sa.cpu().numpy().astype(np.float64)
    lw = max(lw, PP.ratio(slab[..., 1].sum(0), ref["dgamma"], mg["dgamma"], K), PP.ratio(slab[..., 0].sum(0), ref["dbeta"], mg["dbeta"], K))
    worst["layer"] = note("layer " + ("fused" if fused else "unfused"), mode, lw)
    if c.get("tie") and eps == PP.EPS32:                       # (with bf16 operands and K ~ 1e4 the layer bar is too wide for one row)
        teeth(dyk, pooled_layer_ref(h, flip_ties=True)["dy"], mg["dy"], K, eps)
    return worst, dict(dW=dWk, dy=dyk, mdW=mg["dW"], mdy=mg["dy"], K=K)


def check_sparse_rows(h, kp, so):
    Q, S = h["Q"], h["S"]
    cnt = so["srow_cnt"].cpu().numpy()
    rr = so["srow_row"].cpu().numpy().reshape(Q, C)
    sr = so["srows"].cpu().numpy().reshape(Q, C, CP).astype(np.float64)
    W = h["W"].astype(np.float64)
    w, merged = 0.0, []
    for q in range(Q):
        s, pr_ = q % S, prow_of(q, Q, S, h["sm"])
        a = h["arg"][q]
        owners = [r for i, r in enumerate(a) if r >= 0 and r not in a[:i]]
        assert cnt[q] == len(owners) and list(rr[q, :cnt[q]]) == owners, f"window {q}: merged rows"
        assert np.all(rr[q, cnt[q]:] == -7), "srow_row written past srow_cnt"
        coef = kp["P1"][s] * kp["dpm"][pr_]
        for i, r in enumerate(owners):
            chs = np.nonzero(a == r)[0]
            want = (coef[chs][:, None] * W[chs]).sum(0)
            mag = (np.abs(coef[chs])[:, None] * np.abs(W[chs])).sum(0)
            w = max(w, PP.ratio(sr[q, i], want, mag, len(chs)))
            if len(chs) > 1 and np.any(coef[chs[-1]] != 0) and not merged:      # the defect: a merged channel's contribution dropped
                merged.append((sr[q, i], want - coef[chs[-1]] * W[chs[-1]], mag, len(chs)))
    note("sparse_rows", "fp32", w)
    assert w <= 1.0
    assert merged, "no window merges channels"
    teeth(*merged[0])


def check_scatter(h, sp, before, out, pa, pb, pc, idx, mode, fused):
    fam = "sparse_scatter" if fused else "sparse_fix"
    Q = h["Q"]
    # out + add: the added rows carry the bar of their own contraction (C channels at most), the one fp32 addition to the dense value
    # `before` one more rounding of it
    after = out.cpu().numpy().astype(np.float64)
    b = PP.bar(sp["addm"], before + sp["add"], C) + 2 * PP.EPS32 * np.abs(before)
    w = PP.err_ratio(after, before + sp["add"], b)
    pan = pa.cpu().numpy().reshape(Q, pc, CP)[:, idx].astype(np.float64)
    pbn = pb.cpu().numpy().reshape(Q, pc, CP)[:, idx].astype(np.float64)
    w = max(w, PP.ratio(pan, sp["pa"], sp["pam"], C), PP.ratio(pbn, sp["pb"], sp["pbm"], C))
    note(fam, mode, w)
    assert w <= 1.0, (fam, w)
    assert any(len(set(h["arg"][q][h["arg"][q] >= 0])) < (h["arg"][q] >= 0).sum() for q in range(Q)), "no window merges channels"
    pr = pool_bwd_ref(h)
    bad = sparse_ref(h, pr["dpm"], pr["P1"], drop_merged=True)             # the defect: a merged channel's contribution dropped
    r = PP.err_ratio(after, before + bad["add"], b)
    assert r > 1.0, f"the bar does not see the defect (error/bar {r:.3f})"
    q0 = int(np.argmax(np.abs(sp["pa"]).sum(1)))                           # the defect: one window's share of the sums dropped
    bad_pa = sp["pa"].copy()
    bad_pa[q0] = 0.0
    teeth(pan, bad_pa, sp["pam"], C)


def run_wgrad_gram(h, t, chunk_rows, chunks):
    """pw_wgrad with x = y = relu(bn_prev(z_prev)) (the unfused pooled layer's Gram), per (window, chunk) partials + column sums"""
    Q, S = h["Q"], h["S"]
    d = PP.PwBwdProbe()
    d.kind, d.CX, d.CY, d.act, d.Q, d.n_slots, d.max_rows = 2, CP, CP, 1, Q, S, max(h["sizes"])
    d.ldp, d.chunk_rows, d.chunks = CP, chunk_rows, chunks
    wt = dict(gz=t["z_prev"], P2=t["s_prev"], P3=t["t_prev"], pz=t["z_prev"], ps=t["s_prev"], pt=t["t_prev"], win_off=t["win_off"],
              dWpart=nanbuf(Q * chunks, CP, CP), dbpart=nanbuf(Q * chunks, CP))
    PP.set_tensors(d, PP.BWD_EXTENTS, **wt)
    names = launch(d, {k: wt[k] for k in ("dWpart", "dbpart")}, PP.run_bwd)
    assert names == ["pw_wgrad<128,128>+gram"], names
    a = act_prev(h)
    parts = wt["dWpart"].cpu().numpy().reshape(Q, chunks, CP, CP).astype(np.float64)
    db = wt["dbpart"].cpu().numpy().reshape(Q, chunks, CP).astype(np.float64)
    w = 0.0
    for q in range(Q):
        for ch in range(chunks):
            r0 = h["wo"][q] + ch * chunk_rows
            r1 = min(h["wo"][q + 1], r0 + chunk_rows)
            aa = a[r0:r1] if r1 > r0 else np.zeros((0, CP))
            g = aa.T @ aa
            w = max(w, PP.ratio(parts[q, ch], g, g, max(r1 - r0, 1)), PP.ratio(db[q, ch], aa.sum(0), aa.sum(0), max(r1 - r0, 1)))
            if q == 0 and ch == 0:                              # the defect: the chunk's last row left out
                teeth(parts[q, ch], aa[:-1].T @ aa[:-1], g, max(r1 - r0, 1))
    return wt, note("pw_wgrad gram", "fp32", w)


LAYER = [("s1", True), ("s9", True), ("s10", True), ("s12", True), ("s1", False), ("s10", False), ("s12", False)]


@pytest.mark.parametrize("name,fused", LAYER)
def test_pooled_layer_fp32(name, fused):
    with precision("fp32"):
        worst, _ = layer(name, "fp32", fused, 77 + len(name), wgram=POOL[name]["S"] <= 10)
    print(f"[pooled bwd] {name} {'fused' if fused else 'unfused'} fp32: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mode", ["f32x3", "bf16_train", "bf16_store"])
@pytest.mark.parametrize("name", ["s10"])
def test_pooled_layer_fused_modes(name, mode):
    with precision(mode):
        worst, _ = layer(name, mode, True, 91 + len(name))
    print(f"[pooled bwd] {name} fused {mode}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_pooled_wgrad_walk_and_fused_unfused_agree():
    """pooled_wgrad without wgram (the Gram-row walk) at n_slots 10; the fused and unfused forms agree within their combined bar."""
    with precision("fp32"):
        wf, f = layer("s10", "fp32", True, 5, wgram=False)
        wu, u = layer("s10", "fp32", False, 5, wgram=True)
    assert max(wf.values()) <= 1.0 and max(wu.values()) <= 1.0
    r = max(PP.err_ratio(f["dW"], u["dW"], 2 * PP.bar(f["mdW"], u["dW"], f["K"])),
            PP.err_ratio(f["dy"], u["dy"], 2 * PP.bar(f["mdy"], u["dy"], f["K"])))
    print(f"[pooled bwd] fused vs unfused s10: {r:.4f}")
    assert r <= 1.0


# ================================================================================================================================
# unfused pw_dgrad / pw_wgrad at the shapes the product falls back to, and K in {64, 128, 256} with cp not a multiple of 32
# ================================================================================================================================
UNF = {
    # head conv_2 (csrc/head_bwd.hip, the `bpw > wch` branch at max_rows 1537 .. 1792): g dense with the BatchNorm constants, W [128, 320]
    # (columns 0 .. 63 used), no previous layer in pw_dgrad (unmasked output), pw_wgrad y = the linear local features, one slot, chunks of
    # 1024 rows
    "head_c2": dict(CX=128, CY=64, sizes=[1700, 1537, 900, 1792], S=1, lin=True, ldw=320, noprev=True, wg_chunk_rows=1024),
    # the bmm transform's backward (encoder_bwd.hip, `ipb == 0` at max_rows 2561 .. 2816): g = d_local dense WITHOUT BatchNorm constants
    # (P1 == nullptr), per-window slot-major T, 64 -> 64; pw_dgrad has no previous layer, pw_wgrad's y = relu(bn(z_c2))
    "bmm": dict(CX=64, CY=64, sizes=[2700, 2561, 1000, 2816, 5, 2700], S=3, perwin=True, nobn=True, noprev=True),
    "k64_drop": dict(CX=64, CY=64, sizes=[33, 257, 700, 1, 129, 31], S=3, drop=0.3),
    "k128_40": dict(CX=128, CY=40, sizes=[127, 129, 255, 4], S=2, slotw=True, add=True),
    "k256_72": dict(CX=256, CY=72, sizes=[300, 31, 513, 64], S=4),
    "k128_gram": dict(CX=128, CY=128, sizes=[300] * 140, S=10, gram=True, slotw=True),
}


def unf_inputs(c, seed):
    g = np.random.default_rng(seed)
    CX, CY, S, sizes = c["CX"], c["CY"], c["S"], c["sizes"]
    Q, wo = len(sizes), offsets(sizes)
    rows = int(wo[-1])
    rnd = lambda *s: f32(g.standard_normal(s))
    h = dict(CX=CX, CY=CY, n_slots=S, win_off=wo, act=1 if c.get("gram") else 0)
    h["pz"] = rnd(rows, CY)
    if c.get("gram"):
        assert CX == CY
        h["gz"] = h["pz"]
    elif c.get("nobn"):
        h["dy"] = rnd(rows, CX)
    else:
        h["gz"], h["dy"] = rnd(rows, CX), rnd(rows, CX)
        h["P1"], h["P2"], h["P3"] = f32(g.uniform(0.5, 1.5, (S, CX))), f32(g.uniform(-0.2, 0.2, (S, CX))), f32(g.uniform(-0.2, 0.2, (S, CX)))
    if not c.get("lin"):
        gam, inv = f32(g.uniform(-1.5, 1.5, (S, CY))), f32(g.uniform(0.8, 1.2, (S, CY)))
        mean, beta = f32(g.uniform(-0.2, 0.2, (S, CY))), f32(g.uniform(-0.2, 0.2, (S, CY)))
        h["ps"] = f32(gam * inv)
        h["pt"] = f32(beta - mean * h["ps"])
        h["prev_mean"], h["prev_invstd"] = mean, inv
        if c.get("gram"):
            h["P2"], h["P3"] = h["ps"], h["pt"]
    if c.get("perwin"):
        h["W"] = f32(g.uniform(-1, 1, (Q, CY, CX)) / np.sqrt(CX))
        h["w_win_stride"], h["perwin_slot_major"] = CY * CX, 1
    elif c.get("slotw"):
        h["W"] = f32(g.uniform(-1, 1, (S, CX, CY)) / np.sqrt(CX))
        h["ldw"], h["w_slot_stride"] = CY, CX * CY
        h["bias_slot"] = f32(g.uniform(-0.3, 0.3, (S, CY)))
    else:
        h["ldw"] = c.get("ldw", CY)
        h["W"] = f32(g.uniform(-1, 1, (CX, h["ldw"])) / np.sqrt(CX))
    if c.get("add"):
        h["add"] = rnd(rows, CY)
    if c.get("drop"):
        h["drop_p"], h["drop_key"] = c["drop"], (seed, 3)
    return h


def unf_tensors(h):
    t = dict(win_off=dev(h["win_off"], torch.int32))
    for k in ("dy", "gz", "P1", "P2", "P3", "pz", "ps", "pt", "prev_mean", "prev_invstd", "W", "bias_slot", "add"):
        if h.get(k) is not None:
            t[k] = dev(h[k])
    if h["act"]:
        t["gz"] = t["pz"]
    return t


@pytest.mark.parametrize("name", list(UNF))
def test_pw_dgrad(name):
    c = UNF[name]
    h = unf_inputs(c, 600 + len(name))
    CX, CY, S = c["CX"], c["CY"], c["S"]
    Q, rows, max_rows = len(c["sizes"]), int(h["win_off"][-1]), max(c["sizes"])
    chunk_rows = 512
    chunks = -(-max_rows // chunk_rows)
    pc = chunks + 1
    t = unf_tensors(h)
    if c.get("noprev"):                                         # as the product launches it: no previous layer, an unmasked output
        h = {k: v for k, v in h.items() if k not in ("ps", "pt", "prev_mean", "prev_invstd")}
        for k in ("pz", "ps", "pt", "prev_mean", "prev_invstd"):
            t.pop(k, None)
    o = dict(out=nanbuf(rows, CY))
    if h.get("ps") is not None:
        o.update(part_a=nanbuf(Q * pc, CY), part_b=nanbuf(Q * pc, CY))
    d = PP.PwBwdProbe()
    d.kind, d.CX, d.CY, d.act, d.Q, d.n_slots, d.max_rows = 1, CX, CY, h["act"], Q, S, max_rows
    d.ldw, d.w_slot_stride, d.w_win_stride, d.perwin_slot_major = h.get("ldw", 0), h.get("w_slot_stride", 0), h.get("w_win_stride", 0), h.get("perwin_slot_major", 0)
    d.cp, d.part_chunks, d.chunk_rows, d.chunks = CY, pc, chunk_rows, chunks
    d.drop_p = c.get("drop", 0.0)
    if c.get("drop"):
        d.drop_seed = PP.drop_base(*h["drop_key"])
    PP.set_tensors(d, PP.BWD_EXTENTS, **t, **o)
    with precision("fp32"):
        names = launch(d, o, PP.run_bwd)
    NT = 4 if CY > 64 else (2 if CY > 32 else 1)
    want_name = f"pw_dgrad<{CX},{32 * NT}>" + ("+act" if h["act"] else "")
    assert names == [want_name], (names, want_name)
    ref = PP.bwd_ref(h)
    out = o["out"].cpu().numpy()
    w = PP.ratio(out, ref["out"], ref["out_m"], CX)
    teeth(out, scale_row(ref["out"], ref["out_m"]), ref["out_m"], CX)     # the defect: one output row scaled by (1 + 1e-4)
    if "part_a" in o:
        pa = o["part_a"].cpu().numpy().reshape(Q, pc, CY)
        assert is_sentinel(o["part_a"].view(Q, pc, CY)[:, chunks]), "partial slot past chunks written"
        for s in range(S):
            K = ref["rows"][s] * CX
            w = max(w, PP.ratio(pa[s::S, :chunks].astype(np.float64).sum((0, 1)), ref["pa"][s], ref["pa_m"][s], K))
            pb = o["part_b"].cpu().numpy().reshape(Q, pc, CY)
            w = max(w, PP.ratio(pb[s::S, :chunks].astype(np.float64).sum((0, 1)), ref["pb"][s], ref["pb_m"][s], K))
    note("pw_dgrad", "fp32", w)
    print(f"[pooled bwd] pw_dgrad {name}: {names[0]}, worst error/bar {w:.4f}")
    assert w <= 1.0


@pytest.mark.parametrize("name", list(UNF))
def test_pw_wgrad(name):
    c = UNF[name]
    if c.get("perwin"):
        c = dict(c, perwin=False)                               # (pw_wgrad reads no weights)
    h = unf_inputs(c, 700 + len(name))
    CX, CY, S = c["CX"], c["CY"], c["S"]
    Q, max_rows = len(c["sizes"]), max(c["sizes"])
    chunk_rows = c.get("wg_chunk_rows", 256)
    chunks = -(-max_rows // chunk_rows) + 1                     # one chunk more than needed: empty chunks write zero partials
    ldp = CY + 8                                                # ldp > y.C: padding columns keep their sentinels
    t = unf_tensors(h)
    o = dict(dWpart=nanbuf(Q * chunks, CX, ldp), dbpart=nanbuf(Q * chunks, CX))
    d = PP.PwBwdProbe()
    d.kind, d.CX, d.CY, d.act, d.Q, d.n_slots, d.max_rows = 2, CX, CY, h["act"], Q, S, max_rows
    d.ldp, d.chunk_rows, d.chunks = ldp, chunk_rows, chunks
    d.drop_p = c.get("drop", 0.0)
    if c.get("drop"):
        d.drop_seed = PP.drop_base(*h["drop_key"])
    t.pop("W", None), t.pop("bias_slot", None), t.pop("add", None), t.pop("prev_mean", None), t.pop("prev_invstd", None)
    PP.set_tensors(d, PP.BWD_EXTENTS, **t, **o)
    with precision("fp32"):
        names = launch(d, o, PP.run_bwd)
    assert names == [f"pw_wgrad<{CX},{CY}>" + ("+gram" if h["act"] else "")], names
    dWp = o["dWpart"].cpu().numpy().reshape(Q, chunks, CX, ldp)
    assert np.all(dWp[..., CY:].view(np.int32) == PP_NAN), "padding columns written"
    h2 = dict(h)
    h2["W"] = np.zeros((CX, CY), np.float32)
    h2["ldw"], h2["w_slot_stride"], h2["w_win_stride"] = CY, 0, 0
    for k in ("prev_mean", "add", "bias_slot"):                # (data-gradient inputs: not read by pw_wgrad)
        h2.pop(k, None)
    w = 0.0
    dbp = o["dbpart"].cpu().numpy().reshape(Q, chunks, CX)
    def window_ref(q, r0, r1):
        """window q's rows r0 .. r1 alone: the restatement on a one-window problem with the slot's own constants"""
        hq = {k: v for k, v in h2.items()}
        sl = q % S
        for k in ("P1", "P2", "P3", "ps", "pt"):
            if hq.get(k) is not None:
                hq[k] = hq[k][sl:sl + 1]
        for k in ("dy", "gz", "pz"):
            if hq.get(k) is not None:
                hq[k] = hq[k][r0:r1]
        if h["act"]:
            hq["gz"] = hq["pz"]
        hq["n_slots"], hq["win_off"] = 1, np.array([0, r1 - r0])
        if c.get("drop"):
            keep = PP.keep_elems(h["drop_key"], int(h["win_off"][-1]), CY, c["drop"])[r0:r1]
            hq["drop_p"] = 0.0
            hq["_keep"] = keep
        return PP.bwd_ref(hq) if not c.get("drop") else drop_wgrad_ref(hq, keep, c["drop"])

    for q in range(Q):
        r0, r1 = int(h["win_off"][q]), int(h["win_off"][q + 1])
        ref = window_ref(q, r0, r1)
        got = dWp[q, :, :, :CY].astype(np.float64).sum(0)
        w = max(w, PP.ratio(got, ref["dW"][0], ref["dW_m"][0], max(r1 - r0, 1)))
        w = max(w, PP.ratio(dbp[q].astype(np.float64).sum(0), ref["db"][0], ref["db_m"][0], max(r1 - r0, 1)))
        if q == 1:                                              # the defect: the window's last row left out
            teeth(got, window_ref(q, r0, r1 - 1)["dW"][0], ref["dW_m"][0], max(r1 - r0, 1))
    note("pw_wgrad", "fp32", w)
    print(f"[pooled bwd] pw_wgrad {name}: {names[0]}, worst error/bar {w:.4f}")
    assert w <= 1.0


PP_NAN = 0x7FC00000


def drop_wgrad_ref(hq, keep, p):
    h = dict(hq)
    h.pop("_keep")
    h["drop_p"] = 0.0
    r = PP.bwd_ref(h)
    # rebuild with the dropout mask on the activation: a = keep * relu(z s + t) / (1 - p)
    s, tt = h["ps"][0].astype(np.float64), h["pt"][0].astype(np.float64)
    pz = h["pz"].astype(np.float64)
    ds = PP.dscale32(p)
    a = np.where(keep, np.maximum(pz * s + tt, 0) * ds, 0.0)
    am = np.where(keep, (np.abs(pz * s) + np.abs(tt)) * ds, 0.0)
    dy, gz = h["dy"].astype(np.float64), h["gz"].astype(np.float64)
    P1, P2, P3 = (h[k][0].astype(np.float64) for k in ("P1", "P2", "P3"))
    g = dy * P1 + gz * P2 + P3
    gm = np.abs(dy * P1) + np.abs(gz * P2) + np.abs(P3)
    r["dW"] = (g.T @ a)[None]
    r["dW_m"] = (gm.T @ am)[None]
    return r


# ================================================================================================================================
# the input layers: pw_input_wgrad (dWeff per window) and input_param_grads (dW; dT at the slot-major row)
# ================================================================================================================================
@pytest.mark.parametrize("mode,fin", [(0, False), (1, False), (1, True)])
def test_input_wgrad(mode, fin):
    g = np.random.default_rng(11 + mode + 2 * fin)
    S = 3
    sizes = [300] * 12 if fin else [1, 255, 257, 700, 31, 129, 4, 513, 64]
    Q, wo = len(sizes), offsets(sizes)
    rows = int(wo[-1])
    x = f32(g.standard_normal((rows, 9)))
    dy = f32(g.standard_normal((rows, 64)))
    W = f32(g.uniform(-1, 1, (64, 12 if mode else 3)))
    T = f32(np.eye(3)[None] + 0.3 * g.standard_normal((Q, 3, 3)))
    P1, P2, P3 = f32(g.uniform(0.5, 1.5, (S, 64))), f32(g.uniform(-0.2, 0.2, (S, 64))), f32(g.uniform(-0.2, 0.2, (S, 64)))
    t = dict(x=dev(x), dy=dev(dy), W=dev(W), win_off=dev(wo, torch.int32))
    if mode:
        t["T"] = dev(T)
    d = PP.InputWgradProbe()
    d.op, d.mode, d.perwin_slot_major, d.Q, d.n_slots = 0, mode, 1, Q, S
    o = dict(dWeff=nanbuf(Q, 64, 9))
    if fin:
        nP = 4 * S
        fa, fb = f32(g.standard_normal((nP, 64)) * 10), f32(g.standard_normal((nP, 64)) * 10)
        fg, fm, fi = f32(g.uniform(-1.5, 1.5, 64)), f32(g.uniform(-0.2, 0.2, (S, 64))), f32(g.uniform(0.8, 1.2, (S, 64)))
        n = sum(sizes[::S])
        d.fin_parts, d.fin_rows = nP, n
        t.update(fin_part_a=dev(fa), fin_part_b=dev(fb), fin_gamma=dev(fg), fin_mean=dev(fm), fin_invstd=dev(fi))
        o.update(fin_P1=nanbuf(S, 64, 2), fin_P2=nanbuf(S, 64, 2), fin_P3=nanbuf(S, 64, 2), fin_slot_ab=nanbuf(S, 64, 2))
    else:
        t.update(P1=dev(P1), P2=dev(P2), P3=dev(P3))
    PP.set_tensors(d, PP.INPUT_EXTENTS, **t, **o)
    with precision("fp32"):
        names = launch(d, o, PP.run_input)
    assert names == [], names
    w = 0.0
    if fin:
        got = {k: o["fin_" + k].cpu().numpy().reshape(-1)[:S * 64].reshape(S, 64).astype(np.float64) for k in ("P1", "P2", "P3")}
        for sl in range(S):
            A_, B_ = fa[sl::S].astype(np.float64).sum(0), fb[sl::S].astype(np.float64).sum(0)
            sv = fg.astype(np.float64) * fi[sl]
            p2 = -sv * fi[sl] * B_ / n
            p3 = -sv * A_ / n - p2 * fm[sl]
            K = len(fa[sl::S])
            ma, mb = np.abs(fa[sl::S]).sum(0), np.abs(fb[sl::S]).sum(0)
            ab = o["fin_slot_ab"].cpu().numpy()[sl]
            w = max(w, PP.ratio(ab[:, 0], A_, ma, K), PP.ratio(ab[:, 1], B_, mb, K))
            w = max(w, PP.ratio(got["P1"][sl], sv, np.abs(sv), 1), PP.ratio(got["P2"][sl], p2, np.abs(sv * fi[sl]) * mb / n, K))
            w = max(w, PP.ratio(got["P3"][sl], p3, np.abs(sv) * ma / n + np.abs(sv * fi[sl]) * mb / n * np.abs(fm[sl]), K))
        assert is_sentinel(o["fin_P1"].view(-1)[S * 64:]), "fin_P1 written past [n_slots, 64]"
        P1, P2, P3 = got["P1"], got["P2"], got["P3"]
    # dWeff[q][c][f] = sum_rows g[row][c] x[row][f], g = dy P1 + z P2 + P3, z = x Weff^T (kernels.h: PwInput)
    X, DY = x.astype(np.float64), dy.astype(np.float64)
    P1, P2, P3 = (np.asarray(v, dtype=np.float64) for v in (P1, P2, P3))
    q_big = int(np.argmax(sizes))
    pidx = np.array([(q % S) * (Q // S) + q // S for q in range(Q)])
    dWeff_ref = np.zeros((Q, 64, 9))
    dWeff_m = np.zeros((Q, 64, 9))
    for q in range(Q):
        r = slice(wo[q], wo[q + 1])
        if mode == 0:
            Weff = np.zeros((64, 9))
            Weff[:, :3] = W
        else:
            Weff = W[:, 3:].astype(np.float64).copy()
            Weff[:, :3] += W[:, :3].astype(np.float64) @ T[pidx[q]].astype(np.float64).T
        s = q % S
        z = X[r] @ Weff.T
        zm = np.abs(X[r]) @ np.abs(Weff).T
        gg = DY[r] * P1[s] + z * P2[s] + P3[s]
        gm = np.abs(DY[r] * P1[s]) + zm * np.abs(P2[s]) + np.abs(P3[s])
        dWeff_ref[q] = gg.T @ X[r]
        dWeff_m[q] = gm.T @ np.abs(X[r])
        if q == q_big:                                          # the defect: the window's last row left out
            bad_eff = dWeff_ref.copy()
            bad_eff[q] -= np.outer(gg[-1], X[r][-1])
    dWeff = o["dWeff"].cpu().numpy().astype(np.float64)
    K = max(sizes) + 9
    w = max(w, PP.ratio(dWeff, dWeff_ref, dWeff_m, K))
    teeth(dWeff, bad_eff, dWeff_m, K)
    note("pw_input_wgrad", f"mode{mode}", w)
    # input_param_grads on the kernel's own dWeff
    nw = 12 if mode else 3
    o2 = dict(dW=nanbuf(64 * nw + 4), dT=nanbuf(Q + 1, 9))
    d2 = PP.InputWgradProbe()
    d2.op, d2.mode, d2.perwin_slot_major, d2.Q, d2.n_slots = 1, mode, 1, Q, S
    PP.set_tensors(d2, PP.INPUT_EXTENTS, dWeff=o["dWeff"], W=t["W"], T=t.get("T"), dW=o2["dW"], dT=o2["dT"] if mode else None)
    with precision("fp32"):
        launch(d2, o2, PP.run_input)
    assert is_sentinel(o2["dW"][64 * nw:]), "dW written past [64, nw]"
    dW = o2["dW"][:64 * nw].cpu().numpy().reshape(64, nw).astype(np.float64)
    if mode == 0:
        dW_ref, dW_m = dWeff[:, :, :3].sum(0), np.abs(dWeff[:, :, :3]).sum(0)
        bad_dW = dW_ref - dWeff[Q - 1, :, :3]                  # the defect: the last window left out
        assert is_sentinel(o2["dT"]), "mode 0 wrote dT"
    else:
        dW_ref, dW_m = np.zeros((64, 12)), np.zeros((64, 12))
        dW_ref[:, 3:], dW_m[:, 3:] = dWeff.sum(0), np.abs(dWeff).sum(0)
        Tp = T[pidx].astype(np.float64)                         # T of window q at its slot-major row
        dW_ref[:, :3] = np.einsum("qid,qci->cd", Tp, dWeff[:, :, :3])
        dW_m[:, :3] = np.einsum("qid,qci->cd", np.abs(Tp), np.abs(dWeff[:, :, :3]))
        bad_dW = dW_ref.copy()                                  # the defect: the last window left out
        bad_dW[:, 3:] -= dWeff[Q - 1]
        bad_dW[:, :3] -= dWeff[Q - 1, :, :3] @ Tp[Q - 1]
        dT = o2["dT"][:Q].cpu().numpy().reshape(Q, 3, 3).astype(np.float64)
        assert is_sentinel(o2["dT"][Q:]), "dT written past Q"
        dT_ref = np.zeros((Q, 3, 3))
        dT_m = np.zeros((Q, 3, 3))
        Wd = W[:, :3].astype(np.float64)
        for q in range(Q):
            dT_ref[pidx[q]] = dWeff[q, :, :3].T @ Wd
            dT_m[pidx[q]] = np.abs(dWeff[q, :, :3]).T @ np.abs(Wd)
        w2 = PP.ratio(dT, dT_ref, dT_m, 64)
        bad = np.zeros_like(dT_ref)
        for q in range(Q):
            bad[q] = dWeff[q, :, :3].T @ Wd                     # the defect: dT written at window q, not its slot-major row
        teeth(dT, bad, dT_m, 64)
        w = max(w, note("input_param_grads dT", f"mode{mode}", w2))
    w = max(w, note("input_param_grads dW", f"mode{mode}", PP.ratio(dW, dW_ref, dW_m, Q * 3)))
    teeth(dW, bad_dW, dW_m, Q * 3)
    print(f"[pooled bwd] input wgrad mode {mode} fin {fin}: worst error/bar {w:.4f}")
    assert w <= 1.0


# ================================================================================================================================
# refusals
# ================================================================================================================================
def test_probe_refuses_bad_pooled_descriptors():
    """AMPNET_E_ARG before any launch: an arg entry outside its window, a wgram one slot short, part_chunks too small for slot_idx,
    pw_wgrad's dWpart one chunk short."""
    c = POOL["s12"]
    h = pool_inputs(c, 3)
    t = dev_inputs(h)
    S, Q = h["S"], h["Q"]
    with precision("fp32"):
        kp = run_pool_bwd(h, t)
        dpm = dev(kp["dpm"].astype(np.float32))
        P = {k: dev(kp[k].astype(np.float32)) for k in ("P1", "P2", "P3")}
        bad = h["arg"].copy()
        bad[3, 17] = h["wo"][4]                                    # the first row of the NEXT window
        d = pdesc(h, 2, arg=dev(bad, torch.int32), dpm=dpm, P1=P["P1"], W=t["W"], z_prev=t["z_prev"], s_prev=t["s_prev"], t_prev=t["t_prev"],
                  mean_prev=t["mean_prev"], invstd_prev=t["invstd_prev"], win_off=t["win_off"], out=nanbuf(h["rows"], CP),
                  part_a=nanbuf(Q, CP), part_b=nanbuf(Q, CP))
        d.part_chunks, d.slot_idx = 1, 0
        rc, names = PP.run_pooled(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        d.arg = t["arg"].data_ptr()
        d.slot_idx = 1                                             # part_chunks 1 has no slot 1
        rc, names = PP.run_pooled(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        h10 = pool_inputs(POOL["s10"], 3)
        t10 = dev_inputs(h10)
        kp10 = run_pool_bwd(h10, t10)
        S10 = h10["S"]
        P10 = {k: dev(kp10[k].astype(np.float32)) for k in ("P1", "P2", "P3")}
        d = pdesc(h10, 5, W=t10["W"], P1=P10["P1"], P2=P10["P2"], P3=P10["P3"], gram=nanbuf(S10, CP, CP), asum=nanbuf(S10, CP), arg=t10["arg"],
                  dpm=dev(kp10["dpm"].astype(np.float32)), z_prev=t10["z_prev"], s_prev=t10["s_prev"], t_prev=t10["t_prev"],
                  win_off=t10["win_off"], dW=nanbuf(C, CP), wgram=nanbuf(S10 - 1, C, CP))
        rc, names = PP.run_pooled(d)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
        c = UNF["k64_drop"]
        hh = unf_inputs(c, 9)
        tt = unf_tensors(hh)
        Qn = len(c["sizes"])
        dd = PP.PwBwdProbe()
        dd.kind, dd.CX, dd.CY, dd.Q, dd.n_slots, dd.max_rows = 2, 64, 64, Qn, c["S"], max(c["sizes"])
        dd.ldp, dd.chunk_rows, dd.chunks = 64, 256, 3
        PP.set_tensors(dd, PP.BWD_EXTENTS, dy=tt["dy"], gz=tt["gz"], P1=tt["P1"], P2=tt["P2"], P3=tt["P3"], pz=tt["pz"], ps=tt["ps"],
                       pt=tt["pt"], win_off=tt["win_off"], dWpart=nanbuf(Qn * 3 - 1, 64, 64))
        rc, names = PP.run_bwd(dd)
        assert rc == PP.AMPNET_E_ARG and names == [], (rc, names)
