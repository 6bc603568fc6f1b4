"""CPU restatement of the train-mode (batch-statistics) feature propagation, forward and backward, written from the spec in
include/ampnet_hip.h (ampnet_fp_train_forward_f32, ampnet_fp_train_backward_f32), in float64, with a derived float32 error bar per output
element; and the seeded cases of tests/test_fp_train_gpu.py, so that the CPU test (tests/test_fp_train_ref_cpu.py) can check the yardstick
and the seeds without a GPU.  Test infrastructure: no GPU, no library."""
import numpy as np

import fp_ref
from fp_bwd_ref import BN_EPS, C_WEIGHT, RELU_MARGIN, input_rows
from sa_ref import EPS32, make_layers

MOMENTUM = 0.1

# The restatement cases: every one is compared element by element, none left out.
#         name              clouds  n    s   D1   D2   widths       seed
CASES = [("tail_tile",       2,     70,  9,  16,  32,  [32, 64],    0),
         ("two_layers",      2,     70,  9,  16,  32,  [64, 32],    0),
         ("negative_gamma",  2,     70,  9,  16,  32,  [32, 64],    0),
         ("odd_cin",         2,     70,  9,  13,  32,  [64],        0),
         ("two_coarse",      2,     70,  2,  8,   32,  [32, 32],    0),
         ("one_coarse",      2,     40,  1,  8,   32,  [32],        0),
         ("unpicked",        2,     70,  12, 8,   32,  [32, 32],    0),
         ("offset",          2,     70,  9,  16,  32,  [64],        0),
         ("dead_channel",    2,     70,  9,  16,  32,  [32, 64],    0),
         ("fp3_l0",          2,     64,  8,  128, 256, [256],       0),
         ("fp2_l0",          2,     64,  16, 64,  256, [256],       0),
         ("fp1_l0",          2,     96,  12, 0,   128, [128],       0),
         ("widest_l0",       2,     40,  4,  256, 256, [256],       0),
         ("many_tiles",      1026,  2,   2,  8,   32,  [32],        0)]
# Depth and width beyond what the bars can settle (batch normalisation re-amplifies a carried bar by its |x^| / relative-spread factor per
# layer): compared by composition in the GPU test, an L-layer call against L chained one-layer calls, bit for bit.
COMPOSE = [("three_layers",    2,  96,  12, 0,   128, [128, 128, 128],  0),
           ("fp3_form",        2,  64,  8,  128, 256, [256, 256],       0),
           ("fp2_form",        2,  64,  16, 64,  256, [256, 128],       0),
           ("widest",          2,  40,  4,  256, 256, [256, 256, 256],  0),
           ("negative_gamma3", 2,  70,  9,  16,  32,  [32, 64, 32],     0),
           # more tiles than workgroups with every phase of the backward in play: a workgroup carries its sums over several tiles
           ("many_tiles3",     1026, 2, 2,  8,   32,  [32, 32, 32],     0)]
# The dead channel of `dead_channel`: one whose seeded beta is negative.  Its output is relu(beta) in every row; with beta > 0 torch's float64
# gradient of the conv bias for it is a cancelling sum of terms of size gamma / sqrt(eps) |dy| ~ 400, whose own rounding (0.2e-12 .. 1.1e-12
# over the 32 candidate rows, moving with the machine's reduction order) sits on the 1e-12 absolute bound the CPU test holds a zero to; with
# beta < 0 the channel's gradient terms are exact zeros in every implementation, and var = 0, invstd = 1 / sqrt(eps) and the
# running-statistics update are exercised all the same.
DEAD_ROW = 1


def case_inputs(synth, name, seed=None):
    """The seeded inputs of case `name` (CASES or COMPOSE) as a dict of numpy arrays: points1 [B, n, D1] or None, points2 [B, s, D2],
    idx / dist2 [B, n, k] (fp_ref.three_nn on seeded clouds whose coarse points are a subset of the fine ones), layers (seeded; for CASES
    then settle_betas), eps, dout [B, n, cout_last], unpicked (per cloud the coarse points that are nobody's neighbour)."""
    table = CASES + COMPOSE
    _, B, n, s, D1, D2, widths, table_seed = next(c for c in table if c[0] == name)
    seed = table_seed if seed is None else seed             # (another seed: only to look for one that keeps the ReLU margin)
    base = 3000 + 97 * seed + 7 * [c[0] for c in table].index(name)
    fine = synth.clouds(base, B, n)
    pick = np.arange(s) * (n // s) + (1 if n // s > 1 else 0)
    coarse = np.ascontiguousarray(fine[:, pick])
    if name == "unpicked":
        coarse[:, -3:, :] += np.float32(50.0)              # three coarse points far from every fine point
    p1 = synth.uniform(base * 16 + 5, (B, n, D1), -1.0, 1.0) if D1 else None
    p2 = synth.uniform(base * 16 + 6, (B, s, D2), -1.0, 1.0)
    if name == "offset":
        p1, p2 = p1 + np.float32(8.0), p2 + np.float32(8.0)
    dout = synth.uniform(base * 16 + 7, (B, n, widths[-1]), -1.0, 1.0)
    idx, d2 = (np.stack(a) for a in zip(*(fp_ref.three_nn(fine[c], coarse[c]) for c in range(B))))
    layers = make_layers(base + 1, D1 + D2, widths, negative_gamma=name.startswith("negative_gamma"))
    if name.startswith("negative_gamma"):
        assert all((layer[2] < 0).any() and (layer[2] > 0).any() for layer in layers)
        layers[0][2][1] = 0.0                               # one gamma exactly 0
    if name == "dead_channel":
        layers[0][0][DEAD_ROW] = 0.0                        # a = 0 in every row: var = 0, invstd = 1 / sqrt(eps)
        assert layers[0][3][DEAD_ROW] < -0.1
    eps = [BN_EPS] * len(widths)
    if name in [c[0] for c in CASES]:
        settle_betas(p1, p2, idx, d2, layers, eps)
    unpicked = [np.setdiff1d(np.arange(s), idx[c]) for c in range(B)]
    if name == "unpicked":
        assert all(len(u) >= 2 for u in unpicked)
    else:
        assert (d2[:, pick, 0] == 0).all()                  # the fine clouds contain the coarse points
    return dict(points1=p1, points2=p2, idx=idx, dist2=d2, layers=layers, dout=dout, unpicked=unpicked, eps=eps)


def forward_layer(x, bx, layer, e, unbiased=True):
    """One train-mode layer on rows x [M, cin] with bar bx -> a dict of float64 values and bars (b_*); see fp_train's docstring."""
    W, b, gamma, beta, rmean, rvar = (np.asarray(v, dtype=np.float64) for v in layer)
    M = x.shape[0]
    sq = np.sqrt(M)
    a = x @ W.T
    b_a = bx @ np.abs(W).T + 8.0 * EPS32 * np.sqrt(W.shape[1]) * (np.abs(x) @ np.abs(W).T) + 2.0 * EPS32 * np.abs(a)
    mu = a.mean(0)
    b_mu = b_a.mean(0) + 8.0 * EPS32 * sq * np.abs(a).mean(0) + 2.0 * EPS32 * np.abs(mu)
    d = a - mu
    b_d = b_a + b_mu + 2.0 * EPS32 * np.abs(d)
    var = (d * d).mean(0)
    b_var = (2.0 * np.abs(d) * b_d + b_d * b_d).mean(0) + 8.0 * EPS32 * sq * var + 2.0 * EPS32 * var
    ve = var + np.float64(np.float32(e))
    assert (b_var < 0.5 * ve).all(), "the bar of a variance reaches var + eps: choose other inputs"
    inv = 1.0 / np.sqrt(ve)
    b_inv = 0.5 * b_var * (ve - b_var) ** -1.5 + 3.0 * EPS32 * inv
    scale = gamma * inv
    b_scale = np.abs(gamma) * b_inv + 2.0 * EPS32 * np.abs(scale)
    pre = d * scale                                                          # y = pre + beta
    b_pre = (b_a + b_mu) * np.abs(scale) + np.abs(d) * b_scale + (b_a + b_mu) * b_scale + 2.0 * EPS32 * (np.abs(mu * scale) + np.abs(pre))
    y = pre + beta
    b_y = b_pre + 4.0 * EPS32 * np.abs(beta)
    m = np.float64(np.float32(MOMENTUM))
    unb = var * M / (M - 1.0) if unbiased else var
    new_rm = (1.0 - m) * rmean + m * (mu + b)
    b_rm = m * b_mu + 4.0 * EPS32 * (np.abs(m * (mu + b)) + np.abs((1.0 - m) * rmean))
    new_rv = (1.0 - m) * rvar + m * unb
    b_rv = m * b_var * M / (M - 1.0) + 4.0 * EPS32 * (np.abs(m * unb) + np.abs((1.0 - m) * rvar))
    return dict(x=x, bx=bx, W=W, a=a, b_a=b_a, mu=mu, b_mu=b_mu, d=d, b_d=b_d, var=var, inv=inv, b_inv=b_inv, scale=scale, b_scale=b_scale,
                pre=pre, b_pre=b_pre, y=y, b_y=b_y, rm=(new_rm, b_rm), rv=(new_rv, b_rv))


def settle_betas(points1, points2, idx, dist2, layers, eps, margin=2.0 * RELU_MARGIN, step=2.0 ** -10):
    """Moves BatchNorm biases (beta) of `layers`, in place, until no ReLU input of any layer lies within `margin` x its bar of zero
    (fp_bwd_ref.settle_betas's trick: a channel's beta shifts all its inputs together; a layer's batch statistics do not depend on its
    beta).  Twice the margin fp_train asserts is asked here, so that the assertion does not hang on a rounding."""
    x, bx, _, _ = input_rows(points1, points2, idx, dist2)
    for layer, e in zip(layers, eps):
        beta = layer[3]
        f = forward_layer(x, bx, layer, e)                                   # (pre and b_pre do not depend on beta)
        for c in range(len(beta)):
            b0 = np.float32(beta[c])
            for j in range(4096):
                beta[c] = b0 + np.float32(((j + 1) // 2) * (step if j % 2 else -step))
                if (np.abs(f["pre"][:, c] + np.float64(beta[c])) > margin * (f["b_pre"][:, c] + 4.0 * EPS32 * abs(np.float64(beta[c])))).all():
                    break
            else:
                raise AssertionError(f"no beta near {b0} clears channel {c}")
        f = forward_layer(x, bx, layer, e)
        assert (np.abs(f["y"]) > margin * f["b_y"]).all()
        x, bx = np.maximum(f["y"], 0.0), f["b_y"]


def output_names(L, has_points1):
    return (["out"] + [f"{k}{l}" for l in range(L) for k in ("save_mean", "save_invstd", "running_mean", "running_var")]
            + (["dpoints1"] if has_points1 else []) + ["dpoints2"] + [f"{k}{l}" for l in range(L) for k in ("dW", "dbias", "dgamma", "dbeta")])


def fp_train(points1, points2, idx, dist2, layers, eps, dout, margin=RELU_MARGIN, mutate=None):
    """points1 [B, n, D1] float32 or None, points2 [B, s, D2], idx / dist2 [B, n, k] (taken as exact), layers as sa_ref.make_layers (the last
    two entries: running_mean and running_var BEFORE the call), eps per layer, dout [B, n, cout_last] -> ({name: (value, bar)}, worst) with
    the names of output_names(): float64 values and float32 error bars of the outputs of ampnet_fp_train_forward_f32 and
    ampnet_fp_train_backward_f32 (momentum MOMENTUM); worst = the smallest |y| / bar(y) over every ReLU input y of every layer.
    mutate: None, or a deliberate mistake for the test of the test -- "biased" (running_var from the biased variance), "no_xhat" (dz without
    its x^ dgamma / M term).

    Values.  Rows x_0 as in fp_bwd_ref.  Per layer over the M = B n rows: a = x W^T, mu = mean a, d = a - mu, var = mean d^2,
    inv = 1 / sqrt(var + eps), scale = gamma inv, y = d scale + beta, x_{l+1} = relu(y); running_mean' = (1 - m) running_mean + m (mu + b),
    running_var' = (1 - m) running_var + m var M / (M - 1).  Backward from dx_L = dout: dy = dx [y > 0], dbeta = sum dy, G = sum dy a,
    dgamma = inv (G - mu dbeta), dz = scale (dy - dbeta / M - d inv dgamma / M), dW = dz^T x, dx_l = dz W, dbias = 0; dpoints1 / dpoints2
    from dx_0 as in fp_bwd_ref.

    ReLU.  As in fp_bwd_ref: the mask is a step, so |y| > margin * bar(y) (margin = 4) is asserted for every element of every layer and
    the cases are built to keep it (settle_betas).  No element is ever left out of a comparison.

    Bars, e = 2^-24.  The one rule is tests/pw_probe.py::bar: a float32 sum of K products u v has |err| <= 8 e sqrt(K) sum |u| |v| +
    2 e |result|, on top of what the operands' bars carry in: sum (b_u |v| + |u| b_v + b_u b_v).  A quantity formed by r roundings of its
    own gets (r + 1) e times the magnitudes of its terms (one spare).
      * a: b_a = b_x |W|^T + 8 e sqrt(cin) |x| |W|^T + 2 e |a|  (b_x of layer 0: fp_ref's C_INTERP rule; later layers: b_y).
      * mu, a sum of M terms a 1 divided by M (the kernel's tile means and Chan merges are a pairwise form of that sum, well inside the
        sqrt(M) rule):  b_mu = mean b_a + 8 e sqrt(M) mean |a| + 2 e |mu|.
      * d = a - mu, one rounding:  b_d = b_a + b_mu + 2 e |d|.
      * var, a sum of M products d d divided by M (centred in the kernel too: every term is a square, nothing cancels):
        b_var = mean (2 |d| b_d + b_d^2) + 8 e sqrt(M) var + 2 e var.
      * inv = 1 / sqrt(var + eps) is convex and decreasing: |inv(v') - inv(v)| <= (1/2) b_var (var + eps - b_var)^(-3/2) for
        |v' - v| <= b_var (asserted < (var + eps) / 2), plus its own sum, sqrt and quotient:  b_inv = that + 3 e inv.
      * scale = gamma inv:  b_scale = |gamma| b_inv + 2 e |scale|.
      * y = fma(a, scale, shift), shift = fma(-mu, scale, beta): the two fmas round shift and y once each, and the exact value is
        (a - mu) scale + beta, so the errors of a and mu enter through scale only and that of scale through d:
        b_y = (b_a + b_mu) |scale| + |d| b_scale + (b_a + b_mu) b_scale + 2 e (|mu scale| + |d scale| + 2 |beta|)
        (|shift| <= |mu scale| + |beta|, |y| <= |d scale| + |beta|).  out = relu(y) carries b_y.
      * running_mean' = fma(m, mu + b, (1 - m) running_mean): m b_mu + 4 e (|m (mu + b)| + |(1 - m) running_mean|);
        running_var' likewise with var M / (M - 1): m b_var M / (M - 1) + 4 e (|m var M / (M - 1)| + |(1 - m) running_var|).
      * dy = dx [y > 0]: b_dy = b_dx [y > 0] (dout is exact).  dbeta and G as in fp_bwd_ref:
        b_dbeta = sum b_dy + 8 e sqrt(M) sum |dy| + 2 e |dbeta|;  b_G = sum (b_dy |a| + |dy| b_a + b_dy b_a) + 8 e sqrt(M) sum |dy a| + 2 e |G|.
      * t = fma(-mu, dbeta, G):  b_t = b_G + |mu| b_dbeta + b_mu |dbeta| + b_mu b_dbeta + 2 e (|G| + |mu dbeta|);
        dgamma = inv t:  b_dgamma = inv b_t + |t| b_inv + b_t b_inv + 2 e |dgamma|.
      * c1 = dbeta / M:  b_c1 = b_dbeta / M + 2 e |c1|;   c2 = dgamma inv / M:  b_c2 = (b_dgamma inv + |dgamma| b_inv + b_dgamma b_inv) / M
        + 4 e |c2|.
      * dz = scale fma(-d, c2, dy - c1):  u = dy - c1, b_u = b_dy + b_c1 + 2 e |u|;  w = u - d c2,
        b_w = b_u + b_d |c2| + |d| b_c2 + b_d b_c2 + 2 e (|u| + |d c2|);  b_dz = |scale| b_w + |w| b_scale + b_w b_scale + 2 e |dz|.
      * dW = dz^T x over M rows, dx_l = dz W over cout, dpoints1, dpoints2: fp_bwd_ref's rules.  A coarse point with no term has value 0
        and bar 0: it must come back as exact zeros.  dbias: value 0, bar 0 -- exact zeros."""
    x, bx, w, idx = input_rows(points1, points2, idx, dist2)
    B, n, k = idx.shape
    s, D2 = points2.shape[1:]
    D1 = 0 if points1 is None else points1.shape[2]
    M = B * n
    tape, worst, out = [], np.inf, {}
    for l, (layer, e) in enumerate(zip(layers, eps)):
        f = forward_layer(x, bx, layer, e, unbiased=mutate != "biased")
        worst = min(worst, float((np.abs(f["y"]) / np.maximum(f["b_y"], 1e-300)).min()))
        tape.append(f)
        out[f"save_mean{l}"] = (f["mu"], f["b_mu"])
        out[f"save_invstd{l}"] = (f["inv"], f["b_inv"])
        out[f"running_mean{l}"] = f["rm"]
        out[f"running_var{l}"] = f["rv"]
        x, bx = np.maximum(f["y"], 0.0), f["b_y"]
    assert worst > margin, f"a ReLU input lies within {margin} x its bar of zero (|y| / bar = {worst:.3g}): choose other inputs"
    out["out"] = (x.reshape(B, n, -1), bx.reshape(B, n, -1))
    dx, bdx = np.asarray(dout, dtype=np.float64).reshape(M, -1), np.zeros((M, dout.shape[-1]))
    sq = np.sqrt(M)
    for l in range(len(layers) - 1, -1, -1):
        f = tape[l]
        x, bx, W, a, b_a, mu, b_mu, d, b_d = (f[q] for q in ("x", "bx", "W", "a", "b_a", "mu", "b_mu", "d", "b_d"))
        inv, b_inv, scale, b_scale = (f[q] for q in ("inv", "b_inv", "scale", "b_scale"))
        mask = f["y"] > 0.0
        dy, bdy = dx * mask, bdx * mask
        dbeta = dy.sum(0)
        b_dbeta = bdy.sum(0) + 8.0 * EPS32 * sq * np.abs(dy).sum(0) + 2.0 * EPS32 * np.abs(dbeta)
        G = (dy * a).sum(0)
        b_G = (bdy * np.abs(a) + np.abs(dy) * b_a + bdy * b_a).sum(0) + 8.0 * EPS32 * sq * np.abs(dy * a).sum(0) + 2.0 * EPS32 * np.abs(G)
        t = G - mu * dbeta
        b_t = b_G + np.abs(mu) * b_dbeta + b_mu * np.abs(dbeta) + b_mu * b_dbeta + 2.0 * EPS32 * (np.abs(G) + np.abs(mu * dbeta))
        dgamma = inv * t
        b_dgamma = inv * b_t + np.abs(t) * b_inv + b_t * b_inv + 2.0 * EPS32 * np.abs(dgamma)
        out[f"dbeta{l}"] = (dbeta, b_dbeta)
        out[f"dgamma{l}"] = (dgamma, b_dgamma)
        out[f"dbias{l}"] = (np.zeros_like(dbeta), np.zeros_like(dbeta))
        c1 = dbeta / M
        b_c1 = b_dbeta / M + 2.0 * EPS32 * np.abs(c1)
        c2 = dgamma * inv / M
        b_c2 = (b_dgamma * inv + np.abs(dgamma) * b_inv + b_dgamma * b_inv) / M + 4.0 * EPS32 * np.abs(c2)
        u = dy - c1
        b_u = bdy + b_c1 + 2.0 * EPS32 * np.abs(u)
        if mutate == "no_xhat":
            c2 = np.zeros_like(c2)
        wv = u - d * c2
        b_w = b_u + b_d * np.abs(c2) + np.abs(d) * b_c2 + b_d * b_c2 + 2.0 * EPS32 * (np.abs(u) + np.abs(d * c2))
        dz = scale * wv
        bdz = np.abs(scale) * b_w + np.abs(wv) * b_scale + b_w * b_scale + 2.0 * EPS32 * np.abs(dz)
        dW = dz.T @ x
        out[f"dW{l}"] = (dW, bdz.T @ np.abs(x) + np.abs(dz).T @ bx + bdz.T @ bx + 8.0 * EPS32 * sq * (np.abs(dz).T @ np.abs(x))
                         + 2.0 * EPS32 * np.abs(dW))
        dx = dz @ W
        bdx = bdz @ np.abs(W) + 8.0 * EPS32 * np.sqrt(W.shape[0]) * (np.abs(dz) @ np.abs(W)) + 2.0 * EPS32 * np.abs(dx)
    dx, bdx = dx.reshape(B, n, -1), bdx.reshape(B, n, -1)
    if points1 is not None:
        out["dpoints1"] = (dx[..., :D1], bdx[..., :D1])
    g, bg = dx[..., D1:], bdx[..., D1:]
    dp2, b_carry, mag = (np.zeros((B, s, D2)) for _ in range(3))
    cnt = np.zeros((B, s, 1))
    for c in range(B):
        for q in range(k):
            wq = w[c, :, q, None]
            np.add.at(dp2[c], idx[c, :, q], wq * g[c])
            np.add.at(b_carry[c], idx[c, :, q], wq * bg[c] + C_WEIGHT * EPS32 * np.abs(wq * g[c]))
            np.add.at(mag[c], idx[c, :, q], np.abs(wq * g[c]))
            np.add.at(cnt[c], idx[c, :, q], 1.0)
    out["dpoints2"] = (dp2, b_carry + 8.0 * EPS32 * np.sqrt(cnt) * mag + 2.0 * EPS32 * np.abs(dp2))
    return out, worst
