"""CPU restatement of the feature-propagation backward, written from the spec in include/ampnet_hip.h (ampnet_fp_backward_f32), in
float64, with a derived float32 error bar per output element; and the seeded cases of tests/test_fp_backward_gpu.py, so that the CPU test
(tests/test_fp_bwd_ref_cpu.py) can check the yardstick and the seeds without a GPU.  Test infrastructure: no GPU, no library."""
import numpy as np

import fp_ref
from sa_ref import EPS32, make_layers

BN_EPS = 1e-5
RELU_MARGIN = 4.0
C_WEIGHT = 8.0      # roundings of one interpolation weight: 7 (fp_ref.fp_forward), (1 + e)^7 - 1 < 8 e

#         name               n    s   D1   D2   widths            seed
CASES = [("tail_tile",       70,  9,  16,  32,  [32, 64],         0),
         ("odd_cin",         70,  9,  13,  32,  [64],             0),
         ("three_layers",    96,  12, 0,   128, [128, 128, 128],  0),
         ("fp3_form",        64,  8,  128, 256, [256, 256],       0),
         ("fp2_form",        64,  16, 64,  256, [256, 128],       0),
         ("two_coarse",      70,  2,  8,   32,  [32, 32],         0),
         ("one_coarse",      40,  1,  8,   32,  [32],             0),
         ("negative_gamma",  70,  9,  16,  32,  [32, 64, 32],     0),
         ("unpicked",        70,  12, 8,   32,  [32, 32],         0),
         # beyond the issue's table: the one shape family whose tiles do not fit the LDS side by side (x_0 is built twice)
         ("widest",          40,  4,  256, 256, [256, 256, 256],  0)]
N_CLOUDS = 2


def case_inputs(synth, name, seed=None):
    """The seeded inputs of case `name` as a dict of numpy arrays: points1 [2, n, D1] or None, points2 [2, s, D2], idx / dist2 [2, n, k]
    (fp_ref.three_nn on two seeded clouds whose coarse points are a subset of the fine ones), layers (seeded, then settle_betas), dout
    [2, n, cout_last], unpicked (per cloud the coarse points that are nobody's neighbour)."""
    _, n, s, D1, D2, widths, table_seed = next(c for c in CASES if c[0] == name)
    seed = table_seed if seed is None else seed             # (another seed: only to look for one that keeps the ReLU margin)
    base = 1000 + 97 * seed + 7 * [c[0] for c in CASES].index(name)
    fine = synth.clouds(base, N_CLOUDS, n)
    pick = np.arange(s) * (n // s) + 1
    coarse = np.ascontiguousarray(fine[:, pick])
    if name == "unpicked":
        coarse[:, -3:, :] += np.float32(50.0)              # three coarse points far from every fine point
    p1 = synth.uniform(base * 16 + 5, (N_CLOUDS, n, D1), -1.0, 1.0) if D1 else None
    p2 = synth.uniform(base * 16 + 6, (N_CLOUDS, s, D2), -1.0, 1.0)
    dout = synth.uniform(base * 16 + 7, (N_CLOUDS, n, widths[-1]), -1.0, 1.0)
    idx, d2 = (np.stack(a) for a in zip(*(fp_ref.three_nn(fine[c], coarse[c]) for c in range(N_CLOUDS))))
    layers = make_layers(base + 1, D1 + D2, widths, negative_gamma=name == "negative_gamma")
    if name == "negative_gamma":
        assert all((layer[2] < 0).any() and (layer[2] > 0).any() for layer in layers)
        layers[0][2][1] = 0.0                               # one gamma exactly 0
    eps = [BN_EPS] * len(widths)
    settle_betas(p1, p2, idx, d2, layers, eps)
    unpicked = [np.setdiff1d(np.arange(s), idx[c]) for c in range(N_CLOUDS)]
    if name == "unpicked":
        assert all(len(u) >= 2 for u in unpicked)
    else:
        assert (d2[:, pick, 0] == 0).all()                  # the fine clouds contain the coarse points
    return dict(points1=p1, points2=p2, idx=idx, dist2=d2, layers=layers, dout=dout, unpicked=unpicked, eps=eps)


def input_rows(points1, points2, idx, dist2):
    """-> (x_0 [B n, D1 + D2] float64, its float32 bar (fp_ref.fp_forward's rule), the weights w [B, n, k], the clamped idx)."""
    p2 = np.asarray(points2, dtype=np.float64)
    B, s, _ = p2.shape
    idx = np.clip(np.asarray(idx), 0, s - 1)
    d = np.asarray(dist2, dtype=np.float64)
    r = 1.0 / (d + np.float64(np.float32(1e-8)))
    w = r / r.sum(-1, keepdims=True)                                            # [B, n, k]
    terms = w[..., None] * np.stack([p2[c][idx[c]] for c in range(B)])          # [B, n, k, D2]
    x = terms.sum(2)
    bx = fp_ref.C_INTERP * EPS32 * np.abs(terms).sum(2)
    if points1 is not None:
        p1 = np.asarray(points1, dtype=np.float64)
        x = np.concatenate([p1, x], -1)
        bx = np.concatenate([np.zeros_like(p1), bx], -1)
    M = x.shape[0] * x.shape[1]
    return x.reshape(M, -1), bx.reshape(M, -1), w, idx


def forward_layer(x, bx, layer, e):
    """One layer on rows x with bar bx -> (a, b_a, y, b_y, W, scale, inv, b - mean) in float64 (sa_ref.mlp_chain's rule for the bars)."""
    W, b, gamma, beta, mean, var = (np.asarray(v, dtype=np.float64) for v in layer)
    a = x @ W.T
    ba = bx @ np.abs(W).T + 8.0 * EPS32 * np.sqrt(W.shape[1]) * (np.abs(x) @ np.abs(W).T) + 2.0 * EPS32 * np.abs(a)
    inv = 1.0 / np.sqrt(var + np.float64(np.float32(e)))
    scale = gamma * inv
    y = (a + b - mean) * scale + beta
    by = np.abs(scale) * ba + 6.0 * EPS32 * (np.abs(a * scale) + np.abs((b - mean) * scale) + np.abs(beta))
    return a, ba, y, by, W, scale, inv, b - mean


def settle_betas(points1, points2, idx, dist2, layers, eps, margin=2.0 * RELU_MARGIN, step=2.0 ** -10):
    """Moves BatchNorm biases (beta) of `layers`, in place, until no ReLU input of any layer lies within `margin` x its bar of zero.

    With tens of thousands of ReLU inputs per layer and bars of 1e-6 .. 1e-4 of their spread, no seed alone clears every element of the
    larger cases (forty were tried for each).  A channel's beta shifts all its inputs together, and the rows of these cases forbid only a
    sliver of its range: layer by layer, channel by channel, beta is stepped by +-step, +-2 step, .. (float32 values) to the nearest value
    at which the channel is clear.  Twice the margin fp_backward asserts is asked here, so that the assertion does not hang on a rounding.
    Everything else about the case stays as seeded."""
    x, bx, _, _ = input_rows(points1, points2, idx, dist2)
    for layer, e in zip(layers, eps):
        beta = layer[3]
        a, ba, _, _, _, scale, _, bm = forward_layer(x, bx, layer, e)         # (none of these depends on beta)
        pre, fixed = (a + bm) * scale, np.abs(scale) * ba + 6.0 * EPS32 * (np.abs(a * scale) + np.abs(bm * scale))
        for c in range(len(beta)):
            b0 = np.float32(beta[c])
            for j in range(4096):
                beta[c] = b0 + np.float32(((j + 1) // 2) * (step if j % 2 else -step))
                if (np.abs(pre[:, c] + np.float64(beta[c])) > margin * (fixed[:, c] + 6.0 * EPS32 * abs(np.float64(beta[c])))).all():
                    break
            else:
                raise AssertionError(f"no beta near {b0} clears channel {c}")
        _, _, y, by, *_ = forward_layer(x, bx, layer, e)
        assert (np.abs(y) > margin * by).all()
        x, bx = np.maximum(y, 0.0), by


def output_names(L, has_points1):
    return (["dpoints1"] if has_points1 else []) + ["dpoints2"] + [f"{k}{l}" for l in range(L) for k in ("dW", "dbias", "dgamma", "dbeta")]


def fp_backward(points1, points2, idx, dist2, layers, eps, dout, margin=RELU_MARGIN):
    """points1 [B, n, D1] float32 or None, points2 [B, s, D2], idx / dist2 [B, n, k] (taken as exact), layers as sa_ref.make_layers, eps per
    layer, dout [B, n, cout_last] -> ({name: (value, bar)}, worst) with the names of output_names(): float64 values and float32 error
    bars of ampnet_fp_backward_f32's outputs; worst = the smallest |y| / bar(y) over every ReLU input y of every layer.

    Values.  Rows x_0 = [points1[i], sum_q w_q points2[idx_q]], w_q = r_q / sum r, r_q = 1 / (dist2_q + float32(1e-8)).  Per layer
    a = x W^T, scale = gamma / sqrt(var + eps), y = (a + b - mean) scale + beta, x_{l+1} = relu(y).  Backward from dx_L = dout:
    dy = dx [y > 0], dbeta = sum_rows dy, G = sum_rows dy a, dgamma = (G + (b - mean) dbeta) / sqrt(var + eps), dz = dy scale,
    dbias = scale dbeta, dW = dz^T x_l, dx_l = dz W.  dpoints1 = dx_0[:, :D1]; dpoints2[j] = sum over (i, q) with idx[i, q] = j of
    w_q(i) dx_0[i, D1:] (indices clamped into [0, s)).  Sums over rows run over all B clouds.

    ReLU.  The mask [y > 0] is a step: where the float32 y and the float64 y disagree in sign the gradient differs by a whole term and
    no bar covers it.  So the restatement refuses inputs that come near: it asserts |y| > margin * bar(y) (margin = 4) for every element
    of every layer, bar(y) the forward's bar (sa_ref.mlp_chain's rule).  The cases are built so that this holds (settle_betas); no element
    is ever left out of a comparison.  With the mask exact, every output is a smooth function of rounded quantities and the bars follow.

    Bars, e = 2^-24.  The one rule is tests/pw_probe.py::bar: a float32 sum of K products u v has |err| <= 8 e sqrt(K) sum |u| |v| +
    2 e |result|, on top of what the operands' own bars (b_u, b_v) carry in: sum (b_u |v| + |u| b_v + b_u b_v).
      * forward, per layer (kept per element, as mlp_chain does): b_a = b_x |W|^T + 8 e sqrt(cin) |x| |W|^T + 2 e |a|;
        b_y = |scale| b_a + 6 e (|a scale| + |(b - mean) scale| + |beta|); b_relu = b_y.  b_x of layer 0: fp_ref.fp_forward's C_INTERP rule.
      * dy = dx [y > 0]: b_dy = b_dx [y > 0] (dout is exact).
      * dbeta: a sum of M = B n terms dy 1:  sum b_dy + 8 e sqrt(M) sum |dy| + 2 e |dbeta|.
      * G: terms dy a:  sum (b_dy |a| + |dy| b_a + b_dy b_a) + 8 e sqrt(M) sum |dy a| + 2 e |G|.
      * dgamma = fma(b - mean, dbeta, G) / sqrt(var + eps): the bars of G and dbeta times their factors, times inv = 1 / sqrt(var + eps);
        the roundings of its own (var + eps, sqrt, b - mean, the fma, the quotient: <= 5 on either term) as
        6 e inv (|G| + |(b - mean) dbeta|).
      * dz = dy scale: scale carries <= 3 e (sum, sqrt, quotient), the product one more: b_dz = b_dy |scale| + 4 e |dz|.
      * dbias = scale dbeta: |scale| b_dbeta + 4 e |dbias|.
      * dW = dz^T x over M rows:  b_dz^T |x| + |dz|^T b_x + b_dz^T b_x + 8 e sqrt(M) |dz|^T |x| + 2 e |dW|.
      * dx_l = dz W over cout:  b_dz |W| + 8 e sqrt(cout) |dz| |W| + 2 e |dx|.
      * dpoints1: dx_0's own.  dpoints2[j]: a sum of c_j terms w dx_0, w with relative error C_WEIGHT e (7 roundings, fp_ref.fp_forward):
        sum (|w| b_dx0 + C_WEIGHT e |w dx_0|) + 8 e sqrt(c_j) sum |w dx_0| + 2 e |dpoints2|.  A coarse point with no term has value 0 and
        bar 0: it must come back as exact zeros."""
    x, bx, w, idx = input_rows(points1, points2, idx, dist2)
    B, n, k = idx.shape
    s, D2 = points2.shape[1:]
    D1 = 0 if points1 is None else points1.shape[2]
    M = B * n
    # forward, keeping every layer's input, accumulator and bars
    tape, worst = [], np.inf
    for layer, e in zip(layers, eps):
        a, ba, y, by, W, scale, inv, bm = forward_layer(x, bx, layer, e)
        worst = min(worst, float((np.abs(y) / np.maximum(by, 1e-300)).min()))
        tape.append((x, bx, W, a, ba, y, scale, inv, bm))
        x, bx = np.maximum(y, 0.0), by
    assert worst > margin, f"a ReLU input lies within {margin} x its bar of zero (|y| / bar = {worst:.3g}): choose other inputs"
    out = {}
    dx, bdx = np.asarray(dout, dtype=np.float64).reshape(M, -1), np.zeros((M, dout.shape[-1]))
    sq = np.sqrt(M)
    for l in range(len(layers) - 1, -1, -1):
        x, bx, W, a, ba, y, scale, inv, bm = tape[l]
        mask = y > 0.0
        dy, bdy = dx * mask, bdx * mask
        dbeta = dy.sum(0)
        b_dbeta = bdy.sum(0) + 8.0 * EPS32 * sq * np.abs(dy).sum(0) + 2.0 * EPS32 * np.abs(dbeta)
        G = (dy * a).sum(0)
        b_G = (bdy * np.abs(a) + np.abs(dy) * ba + bdy * ba).sum(0) + 8.0 * EPS32 * sq * np.abs(dy * a).sum(0) + 2.0 * EPS32 * np.abs(G)
        out[f"dbeta{l}"] = (dbeta, b_dbeta)
        out[f"dgamma{l}"] = ((G + bm * dbeta) * inv,
                             inv * (b_G + np.abs(bm) * b_dbeta) + 6.0 * EPS32 * inv * (np.abs(G) + np.abs(bm * dbeta)))
        out[f"dbias{l}"] = (scale * dbeta, np.abs(scale) * b_dbeta + 4.0 * EPS32 * np.abs(scale * dbeta))
        dz = dy * scale
        bdz = bdy * np.abs(scale) + 4.0 * EPS32 * np.abs(dz)
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
