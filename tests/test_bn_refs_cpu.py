"""The float64 restatements of tests/bn_probe.py against torch in float64, so that a wrong restatement cannot pass a wrong kernel: the finalize
against F.batch_norm(training=True) on the concatenated rows of a slot, the running update against a double nn.BatchNorm1d fed the slots in order,
the pool against max_pool1d(relu(bn(z))) (channels with negative gamma included), bn_bwd_finalize / fc_bn_bwd / bn_param_grads against autograd
through relu(batch_norm(z)), the input layers against conv_1 of cat(xyz T, x), and the committed fc_bn_bwd inputs for ReLU decisions outside
the fp32 bar.  The global-batch restatements (two ranks with uneven shares, a slot one rank holds no row of, a slot no rank holds a row of)
against the same torch operations on the ranks' rows TOGETHER, within 1e-12, and each against its single-process restatement for one rank.
No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import bn_probe as B

RTOL = 1e-11
EPS = 1e-5


def close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    assert float(np.abs(a - b).max() if a.size else 0.0) <= rtol * scale, (what, float(np.abs(a - b).max()), scale)


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))


def make_layer(seed, win, C, n_slots, chunks, chunk_rows):
    rng = np.random.default_rng(seed)
    win_off = np.concatenate([[0], np.cumsum(win)]).astype(np.int64)
    z = rng.standard_normal((int(win_off[-1]), C)) * (0.5 + rng.random(C)) + 3.0 * rng.standard_normal(C)
    gamma = rng.standard_normal(C)
    gamma[::5] = -np.abs(gamma[::5]) - 0.1
    beta = rng.standard_normal(C) * 0.5
    q = B.PP.win_of_rows(win_off)
    return z, win_off, gamma, beta, q % n_slots


def slot_constants(z, win_off, gamma, beta, n_slots, chunks, chunk_rows, eps=EPS):
    mean, m2, rows = B.chunk_partials(z, win_off, chunks, chunk_rows)
    return B.finalize_ref(mean, m2, rows, B.slot_of_partial(len(rows), chunks, n_slots), n_slots, gamma, beta, eps)


def test_finalize_ref_matches_batch_norm():
    for seed, win, C, S, chunks, cr in ((0, [5, 0, 9, 17, 4, 30, 1, 2, 8], 7, 3, 2, 16), (1, [40, 3, 11, 64], 5, 2, 3, 24), (2, [6], 4, 1, 1, 8)):
        z, win_off, gamma, beta, slot = make_layer(seed, win, C, S, chunks, cr)
        r = slot_constants(z, win_off, gamma, beta, S, chunks, cr)
        for s in range(S):
            zs = t64(z[slot == s])
            rm, rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
            y = F.batch_norm(zs, rm, rv, t64(gamma), t64(beta), training=True, momentum=1.0, eps=EPS)
            close(z[slot == s] * r["scale"][0][s] + r["shift"][0][s], y.numpy(), f"y slot {s}")
            close(r["mean"][0][s], rm.numpy(), "mean")                    # momentum 1: the running buffers ARE the batch statistics
            close(r["stat_mean"][0][s], rm.numpy(), "stat_mean")
            close(r["stat_uvar"][0][s], rv.numpy(), "unbiased variance")
            close(r["invstd"][0][s], 1.0 / np.sqrt(zs.numpy().var(0) + EPS), "invstd")
            close(r["scale"][0][s], gamma / np.sqrt(zs.numpy().var(0) + EPS), "scale")
            assert r["N"][s, 0] == (slot == s).sum()


def test_finalize_ref_one_row_and_no_row():
    gamma, beta = np.array([2.0, -1.0]), np.array([0.5, 0.25])
    means, m2s = np.array([[1.0, 2.0], [7.0, 7.0]]), np.array([[4.0, 9.0], [5.0, 5.0]])
    r = B.finalize_ref(means, m2s, np.array([1, 0]), np.array([0, 1]), 3, gamma, beta, EPS)
    close(r["stat_uvar"][0][0], [4.0, 9.0], "one row: the unbiased variance falls back to M2")
    close(r["invstd"][0][0], 1.0 / np.sqrt(np.array([4.0, 9.0]) + EPS), "one row: biased variance M2 / 1")
    for s in (1, 2):                                                     # zero-row partial only; no partial at all
        close(r["mean"][0][s], [0.0, 0.0], "no row: mean")
        close(r["invstd"][0][s], [1.0 / np.sqrt(EPS)] * 2, "no row: invstd")
        close(r["shift"][0][s], beta, "no row: shift")
        close(r["stat_uvar"][0][s], [0.0, 0.0], "no row: variance")


def test_running_ref_matches_batchnorm1d():
    z, win_off, gamma, beta, slot = make_layer(3, [9, 4, 12, 7, 5, 30, 3, 8, 6, 10, 2, 14], 6, 12, 1, 64)
    for S in (1, 3, 12):
        sl = B.PP.win_of_rows(win_off) % S
        r = slot_constants(z, win_off, gamma, beta, S, 1, 64)
        bn = torch.nn.BatchNorm1d(6, eps=EPS, momentum=0.1).double().train()
        rng = np.random.default_rng(S)
        rm0, rv0 = rng.standard_normal(6), rng.random(6) + 0.5
        with torch.no_grad():
            bn.running_mean.copy_(t64(rm0))
            bn.running_var.copy_(t64(rv0))
            for s in range(S):
                bn(t64(z[sl == s]))
        got = B.running_ref(rm0, rv0, r["stat_mean"][0], r["stat_uvar"][0], momentum=0.1)
        close(got["rmean"][0], bn.running_mean.numpy(), f"running_mean, {S} slots")
        close(got["rvar"][0], bn.running_var.numpy(), f"running_var, {S} slots")


def test_fold_ref_matches_eval_batch_norm():
    rng = np.random.default_rng(4)
    C = 9
    gamma, beta, rm, rv = rng.standard_normal(C), rng.standard_normal(C), rng.standard_normal(C), rng.random(C) + 0.1
    x = rng.standard_normal((5, C))
    r = B.fold_ref(gamma, beta, rm, rv, EPS)
    y = F.batch_norm(t64(x), t64(rm), t64(rv), t64(gamma), t64(beta), training=False, eps=EPS)
    close(x * r["scale"][0] + r["shift"][0], y.numpy(), "eval-mode affine")


def test_pool_ref_matches_max_pool1d():
    for seed, win, C, S, chunks, cr, slot_major in ((5, [5, 3, 9, 17, 4, 30], 10, 3, 3, 16, 1), (6, [40, 3, 11, 48], 6, 2, 1, 64, 0), (7, [4, 20, 6], 5, 3, 2, 16, 0)):
        z, win_off, gamma, beta, slot = make_layer(seed, win, C, S, chunks, cr)
        z = z.astype(np.float32).astype(np.float64)                      # pool partials hold fp32 values
        gamma[1] = 0.0                                                  # scale exactly 0
        r = slot_constants(z, win_off, gamma, beta, S, chunks, cr)
        scale, shift = r["scale"][0], r["shift"][0]
        pmax, amax = B.pool_partials(z, win_off, chunks, cr, gamma)
        Q = len(win)
        for am in (amax, None):
            p = B.pool_ref(pmax, am, scale, shift, Q, chunks, S, slot_major)
            for q in range(Q):
                zq = t64(z[win_off[q]:win_off[q + 1]])
                y = torch.relu(zq * t64(scale[q % S]) + t64(shift[q % S]))
                want = F.max_pool1d(y.T[None], kernel_size=zq.shape[0])[0, :, 0].numpy()
                orow = (q % S) * (Q // S) + q // S if slot_major else q
                close(p["pooled"][0][orow], want, f"pooled window {q}")
                if am is not None:
                    a = p["arg"][q]
                    assert np.all((a >= win_off[q]) & (a < win_off[q + 1]))
                    close(z[a, np.arange(C)], p["zext"][0][q], "zext is z at the argmax row")
                    # the FIRST row of the extreme (chunks ascend in row order, each chunk names its first)
                    ext = np.where(scale[q % S] >= 0, zq.numpy().max(0), zq.numpy().min(0))
                    first = np.array([np.nonzero(zq.numpy()[:, c] == ext[c])[0][0] for c in range(C)]) + win_off[q]
                    assert np.array_equal(a, first)


def test_pool_ref_ties_and_empty_windows():
    # two chunks hold the same extreme: the earlier chunk's row; a window with no non-empty chunk: arg -1, zext 0, relu(shift)
    pmax = np.array([[2.0, -3.0], [1.0, 0.0], [2.0, -3.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], dtype=np.float32)
    amax = np.array([[4, 5], [9, 9], [20, 21], [-1, -1], [-1, -1], [-1, -1]], dtype=np.int32)
    p = B.pool_ref(pmax, amax, np.array([[1.0, -1.0]]), np.array([[0.5, -0.25]]), 2, 3, 1, 0)
    assert np.array_equal(p["arg"], [[4, 5], [-1, -1]])
    close(p["zext"][0], [[2.0, -3.0], [0.0, 0.0]], "zext")
    close(p["pooled"][0], [[2.5, 2.75], [0.5, 0.0]], "pooled")
    pinf = np.array([[2.0, np.inf], [-np.inf, -3.0], [2.0, -3.0], [-np.inf, np.inf], [-np.inf, np.inf], [-np.inf, np.inf]], dtype=np.float32)
    p = B.pool_ref(pinf, None, np.array([[1.0, -1.0]]), np.array([[0.5, -0.25]]), 2, 3, 1, 0)
    close(p["pooled"][0], [[2.5, 2.75], [0.5, 0.0]], "pooled, eval form")


def _autograd(z, da, gamma, beta, slot, S):
    zt, g, b = t64(z).requires_grad_(True), t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
    loss = 0.0
    for s in range(S):
        idx = torch.from_numpy(np.nonzero(slot == s)[0])
        y = torch.relu(F.batch_norm(zt[idx], None, None, g, b, training=True, eps=EPS))
        loss = loss + (y * t64(da)[idx]).sum()
    loss.backward()
    return zt.grad.numpy(), g.grad.numpy(), b.grad.numpy()


def test_bn_bwd_finalize_ref_matches_autograd():
    for seed, win, C, S, chunks, cr in ((8, [5, 3, 9, 17, 4, 30], 6, 3, 2, 16), (9, [40, 7, 11, 48, 2], 5, 2, 3, 16), (10, [12], 4, 1, 1, 16)):
        z, win_off, gamma, beta, slot = make_layer(seed, win, C, S, chunks, cr)
        da = np.random.default_rng(seed + 100).standard_normal(z.shape)
        r = slot_constants(z, win_off, gamma, beta, S, chunks, cr)
        scale, shift, mean, invstd = (r[k][0] for k in ("scale", "shift", "mean", "invstd"))
        dy = np.where(z * scale[slot] + shift[slot] > 0, da, 0.0)
        zh = (z - mean[slot]) * invstd[slot]
        n = B.chunk_rows_of(win_off, chunks, cr)
        Q = len(win)
        pa, pb = np.zeros((Q * chunks, C)), np.zeros((Q * chunks, C))
        for q in range(Q):
            for ch in range(chunks):
                rr = slice(win_off[q] + ch * cr, win_off[q] + ch * cr + n[q, ch])
                pa[q * chunks + ch], pb[q * chunks + ch] = dy[rr].sum(0), (dy[rr] * zh[rr]).sum(0)
        rows = np.array([(slot == s).sum() for s in range(S)])
        f = B.bn_bwd_finalize_ref(pa, pb, B.slot_of_partial(Q * chunks, chunks, S), rows, gamma, mean, invstd, S)
        dz, dgamma, dbeta = _autograd(z, da, gamma, beta, slot, S)
        close(f["P1"][0][slot] * dy + f["P2"][0][slot] * z + f["P3"][0][slot], dz, "dz = P1 dy + P2 z + P3")
        pg = B.param_grads_ref(f["slot_ab"][0])
        close(pg["dgamma"][0], dgamma, "dgamma")
        close(pg["dbeta"][0], dbeta, "dbeta")
    # a slot with no row: finite constants, P2 = P3 = 0
    f = B.bn_bwd_finalize_ref(np.zeros((2, 3)), np.zeros((2, 3)), np.array([0, 0]), np.array([4, 0]), np.ones(3), np.zeros((2, 3)), np.ones((2, 3)), 2)
    assert np.all(f["P2"][0][1] == 0) and np.all(f["P3"][0][1] == 0) and all(np.all(np.isfinite(f[k][0])) for k in ("P1", "P2", "P3", "slot_ab"))


def test_fc_bn_bwd_ref_matches_autograd_and_cases_are_decided():
    for per in B.FC_PER:
        for C in B.FC_C:
            c = B.make_fc_bn_bwd(per, C)
            r = B.fc_bn_bwd_ref(c["da"], c["z"], c["scale"], c["shift"], c["mean"], c["invstd"], 3, per)
            assert r["sure"].all(), f"per {per}, C {C}: a ReLU decision inside the fp32 bar"
            alive = (B.f64(c["z"]) * B.f64(c["scale"]).repeat(per, 0) + B.f64(c["shift"]).repeat(per, 0)) > 0
            assert not alive[:, 0].any() and alive[:, 1].all() and 0.2 < alive[:, 2:].mean() < 0.8
    # the formulas, on constants that are the slots' statistics in float64
    per, C, S = 9, 6, 3
    c = B.make_fc_bn_bwd(per, C)
    z, da = B.f64(c["z"]), B.f64(c["da"])
    zz = z.reshape(S, per, C)
    mean, invstd = zz.mean(1), 1.0 / np.sqrt(zz.var(1) + EPS)
    scale = c["gamma"][None, :] * invstd
    shift = c["beta"][None, :] - mean * scale
    r = B.fc_bn_bwd_ref(da, z, scale, shift, mean, invstd, S, per)
    slot = np.arange(S * per) // per
    dz, dgamma, dbeta = _autograd(z, da, c["gamma"], c["beta"], slot, S)
    close(r["g"][0], dz, "g")
    pg = B.param_grads_ref(r["slot_ab"][0])
    close(pg["dgamma"][0], dgamma, "dgamma")
    close(pg["dbeta"][0], dbeta, "dbeta")
    # da on dead elements is ignored
    da2 = np.where(z * scale[slot] + shift[slot] > 0, da, 1e6)
    close(B.fc_bn_bwd_ref(da2, z, scale, shift, mean, invstd, S, per)["g"][0], dz, "g with da set on dead elements")
    a = B.fc_act_ref(z, scale, shift, per)["act"][0]
    close(a, torch.relu(t64(z * scale[slot] + shift[slot])).numpy(), "fc_act")


def test_input_ref_matches_conv_of_transformed_points():
    rng = np.random.default_rng(11)
    win = [4, 1, 7, 3, 5, 2]
    win_off = np.concatenate([[0], np.cumsum(win)])
    x = rng.standard_normal((int(win_off[-1]), 9))
    W3, W12, T = rng.standard_normal((64, 3)), rng.standard_normal((64, 12)), rng.standard_normal((6, 3, 3))
    q = B.PP.win_of_rows(win_off)
    Z, M, K = B.input_ref(x, W3, None, 0, win_off, 3)
    close(Z, F.conv1d(t64(x[:, :3]).T[None], t64(W3)[:, :, None])[0].T.numpy(), "mode 0")
    assert K == 3 and np.all(M >= np.abs(Z))
    for sm in (0, 1):
        pidx = (q % 3) * 2 + q // 3 if sm else q
        feat = np.concatenate([np.einsum("rf,rfd->rd", x[:, :3], T[pidx]), x], 1)       # cat(xyz T, x)
        Z, M, K = B.input_ref(x, W12, T, 1, win_off, 3, sm)
        close(Z, F.conv1d(t64(feat).T[None], t64(W12)[:, :, None])[0].T.numpy(), f"mode 1, slot_major {sm}")
        assert K == 12 and np.all(M >= np.abs(Z) * (1 - 1e-12))


def test_small_refs():
    rng = np.random.default_rng(12)
    x = rng.standard_normal((7, 5))
    close(B.colsum_ref(x)["out"][0], t64(x).sum(0).numpy(), "colsum")
    p = rng.standard_normal((4, 3, 5))
    close(B.reduce_ref(p)["dst"][0], p.sum(0), "reduce")
    close(B.reduce_ref(p, x[:3])["dst"][0], p.sum(0) + x[:3], "reduce, accumulate")
    Q, S, chunks = 6, 3, 2
    src, add = rng.standard_normal((Q * chunks, 64, 64)), rng.standard_normal((Q, 64, 64))
    got = B.transpose64_ref(src, Q, S, chunks, 0, add)["dst"][0]
    wg = B.transpose64_ref(src, Q, S, chunks, 1)["dst"][0]
    for q in range(Q):
        p = (q % S) * (Q // S) + q // S
        close(got[p], (src[2 * q] + src[2 * q + 1]).T + add[p], "window-major partials")
        j = q // S
        close(wg[p], (src[(j * chunks) * S + q % S] + src[(j * chunks + 1) * S + q % S]).T, "workgroup-major partials")


# ---- the global-batch forms (two ranks with uneven shares) ---------------------------------------------------------------------------------
GTOL = 1e-12


def _two_rank_layer(seed, wins, C, S, chunks, cr):
    """make_layer on the ranks' windows one after the other (rank 0 holds a multiple of S windows, so every window keeps its slot) and the
    row ranges of the ranks."""
    assert len(wins[0]) % S == 0
    z, win_off, gamma, beta, slot = make_layer(seed, wins[0] + wins[1], C, S, chunks, cr)
    cut = int(win_off[len(wins[0])])
    offs = [win_off[:len(wins[0]) + 1], win_off[len(wins[0]):] - cut]
    return z, gamma, beta, slot, [slice(0, cut), slice(cut, None)], offs


def _rank_partials(z, offs, S, chunks, cr):
    mean, m2, rows = B.chunk_partials(z, offs, chunks, cr)
    return mean, m2, rows, B.slot_of_partial(len(rows), chunks, S)


# rank 1: not a multiple of S windows, no row of slot 2 (3 slots) -- and, last, no row of slot 1 on either rank
GLOBAL_LAYERS = ((20, ([5, 0, 9, 17, 4, 30], [7, 12, 0, 3]), 7, 3, 2, 16), (21, ([40, 3], [11, 64, 2]), 5, 2, 3, 24), (22, ([6, 1], [9]), 4, 1, 1, 16),
                 (23, ([5, 0, 9, 17, 0, 30], [7, 0, 3, 2]), 6, 3, 2, 16))


def test_finalize_global_ref_matches_batch_norm_on_the_concatenated_rows():
    for seed, wins, C, S, chunks, cr in GLOBAL_LAYERS:
        z, gamma, beta, slot, rows_of, offs = _two_rank_layer(seed, wins, C, S, chunks, cr)
        ranks = [_rank_partials(z[rows_of[r]], offs[r], S, chunks, cr) for r in range(2)]
        g = B.finalize_global_ref(ranks, S, gamma, beta, EPS)
        if seed == 20:
            assert not any(n > 0 and s == 2 for n, s in zip(ranks[1][2], ranks[1][3])) and g["N"][2, 0] > 0      # slot 2: rank 0's rows only
        for s in range(S):
            zs = t64(z[slot == s])
            if zs.shape[0] == 0:
                assert seed == 23 and s == 1
                close(g["mean"][0][s], np.zeros(C), "no row anywhere: mean")
                close(g["invstd"][0][s], np.full(C, 1.0 / np.sqrt(EPS)), "no row anywhere: invstd")
                close(g["stat_uvar"][0][s], np.zeros(C), "no row anywhere: variance")
                continue
            rm, rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
            y = F.batch_norm(zs, rm, rv, t64(gamma), t64(beta), training=True, momentum=1.0, eps=EPS)
            close(z[slot == s] * g["scale"][0][s] + g["shift"][0][s], y.numpy(), f"y slot {s}", GTOL)
            close(g["mean"][0][s], rm.numpy(), "mean", GTOL)
            close(g["stat_mean"][0][s], rm.numpy(), "stat_mean", GTOL)
            close(g["stat_uvar"][0][s], rv.numpy(), "unbiased variance", GTOL)
            close(g["invstd"][0][s], 1.0 / np.sqrt(zs.numpy().var(0) + EPS), "invstd", GTOL)
            assert g["N"][s, 0] == (slot == s).sum()
        # per-rank statistics are NOT the global ones, and the bars of the exchange only add to finalize_ref's
        own = B.finalize_ref(*ranks[0], S, gamma, beta, EPS)
        assert np.abs(own["mean"][0] - g["mean"][0]).max() > 1e-3
        whole = B.finalize_ref(*B.concat_ranks(ranks), S, gamma, beta, EPS)
        for k in ("scale", "shift", "mean", "invstd", "stat_mean", "stat_uvar"):
            assert np.array_equal(g[k][0], whole[k][0]) and np.all(g[k][1] >= whole[k][1]) and np.all(np.isfinite(g[k][1])), k
        one = B.finalize_global_ref(ranks[:1], S, gamma, beta, EPS)                       # one rank: the single-process restatement
        for k in ("scale", "shift", "mean", "invstd", "stat_mean", "stat_uvar"):
            assert np.array_equal(one[k][0], own[k][0]) and np.array_equal(one[k][1], own[k][1]), k


def _rank_bwd_partials(dy, zh, offs, S, chunks, cr):
    n = B.chunk_rows_of(offs, chunks, cr)
    Q = len(offs) - 1
    pa, pb = np.zeros((Q * chunks, dy.shape[1])), np.zeros((Q * chunks, dy.shape[1]))
    for q in range(Q):
        for ch in range(chunks):
            rr = slice(offs[q] + ch * cr, offs[q] + ch * cr + n[q, ch])
            pa[q * chunks + ch], pb[q * chunks + ch] = dy[rr].sum(0), (dy[rr] * zh[rr]).sum(0)
    rows = np.array([n[s::S].sum() for s in range(S)])
    return pa, pb, B.slot_of_partial(Q * chunks, chunks, S), rows


def test_bn_bwd_finalize_global_ref_matches_autograd_on_the_concatenated_rows():
    for seed, wins, C, S, chunks, cr in GLOBAL_LAYERS:
        z, gamma, beta, slot, rows_of, offs = _two_rank_layer(seed, wins, C, S, chunks, cr)
        da = np.random.default_rng(seed + 100).standard_normal(z.shape)
        fw = B.finalize_global_ref([_rank_partials(z[rows_of[r]], offs[r], S, chunks, cr) for r in range(2)], S, gamma, beta, EPS)
        scale, shift, mean, invstd = (fw[k][0] for k in ("scale", "shift", "mean", "invstd"))
        dy = np.where(z * scale[slot] + shift[slot] > 0, da, 0.0)
        zh = (z - mean[slot]) * invstd[slot]
        ranks = [_rank_bwd_partials(dy[rows_of[r]], zh[rows_of[r]], offs[r], S, chunks, cr) for r in range(2)]
        f = B.bn_bwd_finalize_global_ref(ranks, gamma, mean, invstd, S)
        dz, dgamma, dbeta = _autograd(z, da, gamma, beta, slot, S)
        close(f["P1"][0][slot] * dy + f["P2"][0][slot] * z + f["P3"][0][slot], dz, "dz = P1 dy + P2 z + P3", GTOL)
        pg = [B.param_grads_ref(ab[0]) for ab in f["slot_ab"]]                         # the gradient all-reduce adds the ranks' own
        close(pg[0]["dgamma"][0] + pg[1]["dgamma"][0], dgamma, "dgamma", GTOL)
        close(pg[0]["dbeta"][0] + pg[1]["dbeta"][0], dbeta, "dbeta", GTOL)
        own = B.bn_bwd_finalize_ref(*ranks[0], gamma, mean, invstd, S)
        assert np.abs(own["P3"][0] - f["P3"][0]).max() > 1e-4                          # per-rank constants are not the global ones
        one = B.bn_bwd_finalize_global_ref(ranks[:1], gamma, mean, invstd, S)
        for k in ("P1", "P2", "P3"):
            assert np.array_equal(one[k][0], own[k][0]) and np.all(one[k][1] >= own[k][1]), k
        assert np.array_equal(one["slot_ab"][0][0], own["slot_ab"][0]) and np.array_equal(one["slot_ab"][0][1], own["slot_ab"][1])
        if seed == 23:                                                               # a slot with no row on any rank
            assert np.all(f["P2"][0][1] == 0) and np.all(f["P3"][0][1] == 0) and np.all(f["P2"][1][1] == 0) and np.all(f["P3"][1][1] == 0)
            assert np.all(np.isfinite(f["P1"][0])) and all(np.all(np.isfinite(f[k][i])) for k in ("P1", "P2", "P3") for i in (0, 1))


def test_fc_bn_bwd_global_ref_matches_autograd_and_cases_are_decided():
    for pers in B.FC_PERS:
        for C in B.FC_C:
            for S in B.FC_SLOTS:
                rk = B.make_fc_bn_bwd_ranks(pers, C, S)
                r = B.fc_bn_bwd_global_ref([c["da"] for c in rk], [c["z"] for c in rk], rk[0]["scale"], rk[0]["shift"], rk[0]["mean"], rk[0]["invstd"], S, pers)
                assert all(s.all() for s in r["sure"]), f"per {pers}, C {C}, {S} slots: a ReLU decision inside the fp32 bar"
    pers, C, S = (5, 3), 6, 3
    rk = B.make_fc_bn_bwd_ranks(pers, C, S)
    whole = B.make_fc_bn_bwd(sum(pers), C, S, 1)                                      # (the seed make_fc_bn_bwd_ranks uses)
    z, da = B.f64(whole["z"]), B.f64(whole["da"])
    zz = z.reshape(S, sum(pers), C)
    mean, invstd = zz.mean(1), 1.0 / np.sqrt(zz.var(1) + EPS)
    scale = whole["gamma"][None, :] * invstd
    shift = whole["beta"][None, :] - mean * scale
    r = B.fc_bn_bwd_global_ref([c["da"] for c in rk], [c["z"] for c in rk], scale, shift, mean, invstd, S, pers)
    slot = np.arange(S * sum(pers)) // sum(pers)
    dz, dgamma, dbeta = _autograd(z, da, whole["gamma"], whole["beta"], slot, S)
    dzz, o = dz.reshape(S, sum(pers), C), 0
    for i, per in enumerate(pers):
        close(r["g"][i][0], dzz[:, o:o + per].reshape(S * per, C), f"g of rank {i}", GTOL)
        o += per
    pg = [B.param_grads_ref(ab[0]) for ab in r["slot_ab"]]
    close(pg[0]["dgamma"][0] + pg[1]["dgamma"][0], dgamma, "dgamma", GTOL)
    close(pg[0]["dbeta"][0] + pg[1]["dbeta"][0], dbeta, "dbeta", GTOL)
    own = B.fc_bn_bwd_ref(rk[0]["da"], rk[0]["z"], scale, shift, mean, invstd, S, pers[0])
    assert np.abs(own["g"][0] - r["g"][0][0]).max() > 1e-3                             # the rank's own means are not the global ones
    one = B.fc_bn_bwd_global_ref([rk[0]["da"]], [rk[0]["z"]], scale, shift, mean, invstd, S, pers[:1])
    for k in ("g", "slot_ab"):
        assert np.array_equal(one[k][0][0], own[k][0]) and np.array_equal(one[k][0][1], own[k][1]), k


def test_pool_bwd_global_ref_matches_autograd_on_the_concatenated_rows():
    import test_pooled_bwd_gpu as PB
    C = PB.C
    for sm in (0, 1):
        hs = PB.pool_ranks([dict(sizes=[5, 3, 9, 4, 7, 2], S=3, sm=sm), dict(sizes=[6, 1, 8], S=3, sm=sm)], (31, 32), exact=True)
        g = PB.pool_bwd_global_ref(hs)
        z = np.concatenate([h["z32"] for h in hs]).astype(np.float64)
        slot = np.concatenate([h["slot"] for h in hs])
        zt, gm, bt = t64(z).requires_grad_(True), t64(hs[0]["gamma"]), t64(hs[0]["beta"])
        y = torch.zeros_like(zt)
        for s in range(3):
            idx = torch.from_numpy(np.nonzero(slot == s)[0])
            y = y.index_copy(0, idx, torch.relu(F.batch_norm(zt[idx], None, None, gm, bt, training=True, eps=EPS)))
        loss, dys, row0 = 0.0, np.zeros_like(z), 0
        for h, r in zip(hs, g["ranks"]):
            for q in range(h["Q"]):
                pr = PB.prow_of(q, h["Q"], 3, sm)
                rows = torch.from_numpy(h["arg"][q].astype(np.int64) + row0)
                loss = loss + (y[rows, torch.arange(C)] * t64(h["d_pooled"][pr])).sum()
                dys[h["arg"][q] + row0, np.arange(C)] += r["dpm"][pr]
            row0 += h["rows"]
        loss.backward()
        close(g["P1"][0][slot] * dys + g["P2"][0][slot] * z + g["P3"][0][slot], zt.grad.numpy(), f"dz, slot_major {sm}", GTOL)
        assert np.abs(g["ranks"][1]["P3"] - g["P3"][0]).max() > 1e-5                       # the rank's own constants are not the global ones
        one = PB.pool_bwd_global_ref(hs[:1])
        for k in ("P1", "P2", "P3"):
            assert np.array_equal(one[k][0], one["ranks"][0][k]), k
