"""CPU restatement of the fused segmentation head and its backward, written from the spec in include/ampnet_hip.h
(ampnet_seg_head_forward_f32, ampnet_seg_head_backward_f32), in float64, with a derived float32 error bar per output element; and the seeded
cases of tests/test_seg_head_gpu.py, so that the CPU test (tests/test_seg_head_ref_cpu.py) can check the yardstick and the seeds without a
GPU.  Test infrastructure: no GPU, no library.

Values.  Per row x:  a = W1 x,  scale = gamma / sqrt(var + eps),  y = (a + b1 - mean) scale + beta,  h = relu(y),  z = W2 h + b2,
lse = m + log(sum_c exp(z_c - m)) with m = max_c z_c,  logp = z - lse,  pred = the lowest c with z_c = m.  Backward from g = dlogp:
dz_c = g_c - exp(logp_c) sum_j g_j,  db2 = sum_rows dz,  dW2 = dz^T h,  dh = dz W2, then conv1 as one layer of fp_bwd_ref.fp_backward:
dy = dh [y > 0], dbeta = sum_rows dy, G = sum_rows dy a, dgamma = (G + (b1 - mean) dbeta) / sqrt(var + eps), db1 = scale dbeta,
dz1 = dy scale, dW1 = dz1^T x, dx = dz1 W1.

Bars, e = 2^-24.  The one rule for a float32 sum of K products u v is tests/pw_probe.py::bar: |err| <= 8 e sqrt(K) sum |u| |v| + 2 e |result|,
on top of what the operands' own bars carry in.
  * h: sa_ref.mlp_chain's rule for one layer (fp_bwd_ref.forward_layer), the input rows exact: bar 0 going in.
  * z: one more linear layer of `hidden` products, the bias taken into the magnitude (its one addition is a term of the sum):
    b_z = b_h |W2|^T + 8 e sqrt(hidden) (|h| |W2|^T + |b2|) + 2 e |z|.
  * logp_c = (z_c - m) - logf(S), S = sum over c of expf(z_c - m):
      - what z carries in: b_z[c] + max_j b_z[j] -- the log-sum-exp is 1-Lipschitz in the max norm (its gradient is a probability vector);
      - the subtraction d_c = z_c - m: e |d_c|;
      - expf(d_c): relative error head_probe.exp_rel(d_c) = (2 |d_c| + 4) e, the bound the project measured the device's expf and logf
        against (tests/test_head_layers_gpu.py::test_exp_log_sweep: 0.24 and 0.48 of it);
      - S: the terms are positive, so its relative error is sum_c p_c exp_rel(d_c), p = softmax(z), plus (C - 1) e for the C - 1 additions;
      - logf(S): the relative error of S is an absolute error of the logarithm, plus head_probe.exp_rel(S) |log S| for the function;
      - the last subtraction: e |logp_c|.
  * pred: compared where the reference's arg-max cannot flip: see admitted().
  * dz_c = fma(-expf(logp_c), sg, g_c), sg = sum_j g_j over j ascending:  p_c = expf(logp_c) carries p_c (b_logp[c] + exp_rel(logp_c));
    sg carries (C - 1) e sum_j |g_j| (g is exact);  b_dz = b_p |sg| + p b_sg + b_p b_sg + e |dz|  (one rounding, the fma's).
  * db2: a sum of M terms dz 1:  sum b_dz + 8 e sqrt(M) sum |dz| + 2 e |db2|.
  * dW2 = dz^T h over M rows:  b_dz^T |h| + |dz|^T b_h + b_dz^T b_h + 8 e sqrt(M) |dz|^T |h| + 2 e |dW2|.
  * dh = dz W2 over the classes (the kernel pads them to 32 with zeros, whose products add exactly nothing):
    b_dz |W2| + 8 e sqrt(C) |dz| |W2| + 2 e |dh|.
  * dbeta, G, dgamma, db1, dz1, dW1, dx: fp_bwd_ref.fp_backward's rules, term by term, with dx_{l+1} = dh and its bar.
ReLU.  As in fp_bwd_ref: the restatement refuses inputs whose conv1 pre-activation y comes within RELU_MARGIN x bar(y) of zero, and the cases
are built so that none does (settle_beta moves bn1's bias, channel by channel, to the nearest float32 value that clears twice the margin)."""
import numpy as np

from fp_bwd_ref import BN_EPS, RELU_MARGIN, forward_layer
from sa_ref import EPS32, make_layers

EXP_ULP = 4.0       # head_probe.EXP_ULP: exp_rel below is head_probe.exp_rel (that module imports torch and the library; this one must not)

#         name                  M                     cin  hidden  C   seed
CASES = [("tail",               70,                   128, 128,    5,  0),
         ("one_row",            1,                    9,   32,     2,  0),
         ("odd_cin",            33,                   13,  64,     13, 0),
         ("full_tile_classes",  64,                   32,  32,     32, 0),
         ("widest",             40,                   256, 256,    31, 1),     # (seed 0 leaves 1 of the 40 rows out of the pred check)
         ("negative_gamma",     70,                   16,  64,     5,  0),
         ("walk",               32 * 4 * 1024 + 70,   32,  32,     5,  0),
         ("ties",               64,                   8,   32,     4,  0)]
NAMES = [c[0] for c in CASES]
OUTPUTS = ("dx", "dW1", "db1", "dgamma", "dbeta", "dW2", "db2")
MAX_LEFT_OUT = 0.01     # share of a case's rows admitted() may leave out: a condition on the seeds, asserted by the CPU test


def exp_rel(x, ulp=EXP_ULP):
    """head_probe.exp_rel: the relative error bound of a float32 exp / log of the rounded argument x."""
    return (2.0 * np.abs(x) + ulp) * EPS32


def settle_beta(x, layer, e, margin=2.0 * RELU_MARGIN, step=2.0 ** -10):
    """fp_bwd_ref.settle_betas for the head's one BatchNorm layer on exact rows x: moves beta, in place, channel by channel to the nearest
    float32 value b0 +- j step, j < 2048, at which no pre-activation of the channel lies within `margin` x its bar of zero.  With 131 142
    rows (the `walk` case) trying the candidates one by one takes half a minute, so every row strikes out the candidates it forbids at
    once -- an interval around -pre, its half-width taken with the largest |beta| among the candidates -- and the nearest survivor is
    checked against the rule itself."""
    x = np.asarray(x, dtype=np.float64)
    beta = layer[3]
    a, ba, _, _, _, scale, _, bm = forward_layer(x, np.zeros_like(x), layer, e)           # (none of these depends on beta)
    pre, fixed = (a + bm) * scale, np.abs(scale) * ba + 6.0 * EPS32 * (np.abs(a * scale) + np.abs(bm * scale))
    js = np.arange(-2048, 2048)
    for c in range(len(beta)):
        b0 = np.float32(beta[c])
        cands = (b0 + (js * step).astype(np.float32)).astype(np.float64)                   # ascending float32 values
        half = margin * (fixed[:, c] + 6.0 * EPS32 * np.abs(cands).max()) * (1.0 + 1e-9)
        struck = np.zeros(len(cands) + 1)
        np.add.at(struck, np.searchsorted(cands, -pre[:, c] - half, "left"), 1.0)
        np.add.at(struck, np.searchsorted(cands, -pre[:, c] + half, "right"), -1.0)
        free = np.flatnonzero(np.cumsum(struck)[:-1] == 0)
        assert len(free), f"no beta near {b0} clears channel {c}"
        beta[c] = np.float32(cands[free[np.argmin(np.abs(js[free]))]])
        assert (np.abs(pre[:, c] + np.float64(beta[c])) > margin * (fixed[:, c] + 6.0 * EPS32 * abs(np.float64(beta[c])))).all()


def case_inputs(synth, name, seed=None):
    """The seeded inputs of case `name` as a dict of numpy float32 arrays: x [M, cin], params (W1, b1, gamma, beta, running_mean,
    running_var, W2, b2), dlogp [M, C], eps."""
    _, M, cin, hidden, C, table_seed = next(c for c in CASES if c[0] == name)
    seed = table_seed if seed is None else seed             # (another seed: only to look for one that meets the conditions)
    base = 5000 + 97 * seed + 7 * NAMES.index(name)
    x = synth.uniform(base * 16 + 1, (M, cin), -1.0, 1.0)
    layer = make_layers(base + 1, cin, [hidden], negative_gamma=name == "negative_gamma")[0]
    if name == "negative_gamma":
        assert (layer[2] < 0).any() and (layer[2] > 0).any()
        layer[2][1] = 0.0                                   # one gamma exactly 0
    settle_beta(x, layer, BN_EPS)
    k = 1.0 / np.sqrt(hidden)
    # (logits a few units apart, as a trained head's are: with weights of 1 / sqrt(hidden) alone the classes would lie closer together
    # than the bars of a 256-wide head tell apart)
    W2 = synth.uniform(base * 16 + 2, (C, hidden), -4.0 * k, 4.0 * k)
    b2 = synth.uniform(base * 16 + 3, (C,), -1.0, 1.0)
    if name == "ties":
        W2[1], b2[1] = W2[0], b2[0]                         # classes 0 and 1 tie exactly in every row
    dlogp = synth.uniform(base * 16 + 4, (M, C), -1.0, 1.0)
    return dict(x=x, params=tuple(layer) + (W2, b2), dlogp=dlogp, eps=BN_EPS)


def duplicates(params):
    """The classes whose W2 row and b2 equal those of a LOWER class: their logits tie with that class in every row, by construction."""
    W2, b2 = params[6], params[7]
    return [c for c in range(len(b2)) if any((W2[c] == W2[j]).all() and b2[c] == b2[j] for j in range(c))]


def seg_forward(x, params, eps, margin=RELU_MARGIN):
    """x [M, cin] float32, params the 8 float32 arrays, eps -> dict: logp (value, bar), pred (int64 [M], the lowest arg-max), z (value, bar),
    worst (the smallest |y| / bar(y) over conv1's pre-activations), tape (what seg_backward needs)."""
    x = np.asarray(x, dtype=np.float64)
    a, ba, y, by, W1, scale, inv, bm = forward_layer(x, np.zeros_like(x), params[:6], eps)
    worst = float((np.abs(y) / np.maximum(by, 1e-300)).min())
    assert worst > margin, f"a ReLU input lies within {margin} x its bar of zero (|y| / bar = {worst:.3g}): choose other inputs"
    h, bh = np.maximum(y, 0.0), by
    W2, b2 = (np.asarray(v, dtype=np.float64) for v in params[6:])
    C, hidden = W2.shape
    z = h @ W2.T + b2
    for c in duplicates(params):                            # (equal rows of W2: equal logits, whatever order the BLAS adds in)
        j = next(j for j in range(c) if (params[6][c] == params[6][j]).all() and params[7][c] == params[7][j])
        z[:, c] = z[:, j]
    bz = bh @ np.abs(W2).T + 8.0 * EPS32 * np.sqrt(hidden) * (np.abs(h) @ np.abs(W2).T + np.abs(b2)) + 2.0 * EPS32 * np.abs(z)
    m = z.max(1, keepdims=True)
    d = z - m
    ex = np.exp(d)
    S = ex.sum(1, keepdims=True)
    logp = d - np.log(S)
    rel_S = (ex / S * exp_rel(d)).sum(1, keepdims=True) + (C - 1) * EPS32
    blogp = bz + bz.max(1, keepdims=True) + EPS32 * np.abs(d) + rel_S + exp_rel(S) * np.abs(np.log(S)) + EPS32 * np.abs(logp)
    return dict(logp=(logp, blogp), pred=z.argmax(1).astype(np.int64), z=(z, bz), worst=worst,
                tape=(x, a, ba, y, W1, scale, inv, bm, h, bh, W2))


def admitted(fwd, params):
    """The rows whose pred is compared with the reference's: a row is LEFT OUT when the gap between its two largest logits is under twice
    the row's bar (the largest b_z of the row), for then a float32 evaluation inside its bars may rank them the other way.  Classes that
    duplicate a lower class (duplicates()) tie with it exactly in the kernel too -- the same operations on the same numbers -- and the lowest
    wins there as here, so they are not counted as a second logit."""
    z, bz = fwd["z"]
    keep = [c for c in range(z.shape[1]) if c not in duplicates(params)]
    top = np.sort(z[:, keep], 1)
    gap = top[:, -1] - top[:, -2] if len(keep) > 1 else np.full(len(z), np.inf)
    return gap >= 2.0 * bz.max(1)


def seg_backward(x, params, eps, dlogp, margin=RELU_MARGIN):
    """-> ({name: (value, bar)} for OUTPUTS, the forward's dict): float64 values and float32 error bars of ampnet_seg_head_backward_f32's
    outputs (the module docstring)."""
    fwd = seg_forward(x, params, eps, margin)
    x, a, ba, y, W1, scale, inv, bm, h, bh, W2 = fwd["tape"]
    logp, blogp = fwd["logp"]
    g = np.asarray(dlogp, dtype=np.float64)
    M, C = g.shape
    sq = np.sqrt(M)
    p = np.exp(logp)
    bp = p * (blogp + exp_rel(logp))
    sg = g.sum(1, keepdims=True)
    bsg = (C - 1) * EPS32 * np.abs(g).sum(1, keepdims=True)
    dz = g - p * sg
    bdz = bp * np.abs(sg) + p * bsg + bp * bsg + EPS32 * np.abs(dz)
    out = {}
    db2 = dz.sum(0)
    out["db2"] = (db2, bdz.sum(0) + 8.0 * EPS32 * sq * np.abs(dz).sum(0) + 2.0 * EPS32 * np.abs(db2))
    dW2 = dz.T @ h
    out["dW2"] = (dW2, bdz.T @ np.abs(h) + np.abs(dz).T @ bh + bdz.T @ bh + 8.0 * EPS32 * sq * (np.abs(dz).T @ np.abs(h))
                  + 2.0 * EPS32 * np.abs(dW2))
    dh = dz @ W2
    bdh = bdz @ np.abs(W2) + 8.0 * EPS32 * np.sqrt(C) * (np.abs(dz) @ np.abs(W2)) + 2.0 * EPS32 * np.abs(dh)
    # conv1: one layer of fp_bwd_ref.fp_backward
    mask = y > 0.0
    dy, bdy = dh * mask, bdh * mask
    dbeta = dy.sum(0)
    b_dbeta = bdy.sum(0) + 8.0 * EPS32 * sq * np.abs(dy).sum(0) + 2.0 * EPS32 * np.abs(dbeta)
    G = (dy * a).sum(0)
    b_G = (bdy * np.abs(a) + np.abs(dy) * ba + bdy * ba).sum(0) + 8.0 * EPS32 * sq * np.abs(dy * a).sum(0) + 2.0 * EPS32 * np.abs(G)
    out["dbeta"] = (dbeta, b_dbeta)
    out["dgamma"] = ((G + bm * dbeta) * inv, inv * (b_G + np.abs(bm) * b_dbeta) + 6.0 * EPS32 * inv * (np.abs(G) + np.abs(bm * dbeta)))
    out["db1"] = (scale * dbeta, np.abs(scale) * b_dbeta + 4.0 * EPS32 * np.abs(scale * dbeta))
    dz1 = dy * scale
    bdz1 = bdy * np.abs(scale) + 4.0 * EPS32 * np.abs(dz1)
    dW1 = dz1.T @ x
    out["dW1"] = (dW1, bdz1.T @ np.abs(x) + 8.0 * EPS32 * sq * (np.abs(dz1).T @ np.abs(x)) + 2.0 * EPS32 * np.abs(dW1))     # (b_x = 0)
    dx = dz1 @ W1
    out["dx"] = (dx, bdz1 @ np.abs(W1) + 8.0 * EPS32 * np.sqrt(W1.shape[0]) * (np.abs(dz1) @ np.abs(W1)) + 2.0 * EPS32 * np.abs(dx))
    return out, fwd


def compose(x, params, eps, dlogp, dt):
    """The same formulas in numpy of dtype dt, nothing else shared with the functions above (BLAS / pairwise summation orders, not the
    kernels'): -> {logp, pred, and OUTPUTS}.  float64 is compared with torch, float32 must stay inside every bar."""
    x, W1, b1, gamma, beta, mean, var, W2, b2, g = (np.asarray(v, dtype=dt) for v in (x,) + tuple(params) + (dlogp,))
    inv = dt(1.0) / np.sqrt(var + dt(np.float32(eps)))
    scale = gamma * inv
    a = x @ W1.T
    y = a * scale + ((b1 - mean) * scale + beta)
    h = np.maximum(y, dt(0.0))
    z = h @ W2.T + b2
    d = z - z.max(1, keepdims=True)
    logp = d - np.log(np.exp(d).sum(1, keepdims=True))
    dz = g - np.exp(logp) * g.sum(1, keepdims=True)
    dy = (dz @ W2) * (y > 0)
    dbeta, G = dy.sum(0), (dy * a).sum(0)
    dz1 = dy * scale
    return dict(logp=logp, pred=z.argmax(1).astype(np.int64), dx=dz1 @ W1, dW1=dz1.T @ x, db1=scale * dbeta,
                dgamma=(G + (b1 - mean) * dbeta) * inv, dbeta=dbeta, dW2=dz.T @ h, db2=dz.sum(0))


_REFERENCES = {}


def reference(synth, name):
    """(inputs, {output: (value, bar)}, the forward's dict) of a case, computed once per process and shared: nobody writes to them."""
    if name not in _REFERENCES:
        i = case_inputs(synth, name)
        out, fwd = seg_backward(i["x"], i["params"], i["eps"], i["dlogp"])
        _REFERENCES[name] = (i, out, fwd)
    return _REFERENCES[name]
