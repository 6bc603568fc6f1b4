"""CPU restatement of the segmentation head in TRAIN mode, forward and backward, written from the spec in include/ampnet_hip.h
(ampnet_seg_head_train_forward_f32, ampnet_seg_head_train_backward_f32), in float64, with a derived float32 error bar per output element;
and the seeded cases of tests/test_seg_head_train_gpu.py, so that the CPU test (tests/test_seg_head_train_ref_cpu.py) can check the
yardstick and the seeds without a GPU.  Test infrastructure: no GPU, no library.

Values.  Over the M rows x:  a = W1 x,  mu = mean a,  d = a - mu,  var = mean d^2,  inv = 1 / sqrt(var + eps),  scale = gamma inv,
y = d scale + beta,  h = relu(y);  running_mean' = (1 - m) running_mean + m (mu + b1),  running_var' = (1 - m) running_var + m var M / (M - 1)
(fp_train_ref.forward_layer).  hd = keep ? h dscale : 0 with keep_mask() below and dscale the float32 value 1 / (1 - p) as the host forms
it (an exact constant here).  z = W2 hd + b2, logp = log_softmax(z) as in seg_head_ref.  Backward from g = dlogp:  dz_c = g_c - exp(logp_c)
sum_j g_j,  db2 = sum_rows dz,  dW2 = dz^T hd,  dh = dz W2,  dh' = keep ? dh dscale : 0,  dy = dh' [y > 0],  dbeta = sum dy,  G = sum dy a,
dgamma = inv (G - mu dbeta),  db1 = 0,  dz1 = scale (dy - dbeta / M - d inv dgamma / M),  dW1 = dz1^T x,  dx = dz1 W1.

Bars, e = 2^-24.  The one rule for a float32 sum of K products u v is tests/pw_probe.py::bar: |err| <= 8 e sqrt(K) sum |u| |v| + 2 e |result|,
on top of what the operands' own bars carry in.
  * a, mu, d, var, inv, scale, y and the running statistics: fp_train_ref.forward_layer, term by term, the input rows exact (bar 0).
  * hd = h dscale where kept, one rounding (one spare):  b_hd = keep (b_y dscale + 2 e |hd|); a dropped element is an exact zero, bar 0.
    The mask is not a matter of rounding: a wrong keep bit moves a logit by about |W2| |h| dscale, orders of magnitude above b_z.
  * z, logp, dz, db2, dW2, dh: seg_head_ref's rules with hd and b_hd in place of h and b_h.
  * dh' = dh dscale where kept:  b_dh' = keep (b_dh dscale + 2 e |dh'|).
  * dy, dbeta, G, dgamma, c1, c2, dz1, dW1, dx: fp_train_ref.fp_train's rules for one layer with dx_{l+1} = dh' and b_x = 0.  db1: value 0,
    bar 0 -- exact zeros.
ReLU.  As in fp_train_ref: the restatement refuses inputs whose pre-activation y comes within RELU_MARGIN x bar(y) of zero, and the cases are
built so that none does (settle_beta moves bn1's bias against the BATCH-statistics pre-activation, which does not depend on beta)."""
import numpy as np

from fp_bwd_ref import BN_EPS, RELU_MARGIN
from fp_train_ref import MOMENTUM, forward_layer
from sa_ref import EPS32, make_layers
from seg_head_ref import exp_rel

#         name                  M                     cin  hidden  C   p    seed
CASES = [("two_rows",           2,                    9,   32,     2,  0.5, 0),     # the minimum the statistics accept
         ("tail",               70,                   128, 128,    5,  0.5, 0),     # a 6-row last tile
         ("odd_cin",            33,                   13,  64,     13, 0.3, 0),     # a one-row tile
         ("full_tile_classes",  64,                   32,  32,     32, 0.5, 0),
         ("widest",             40,                   256, 256,    31, 0.5, 0),
         ("negative_gamma",     70,                   16,  64,     5,  0.5, 0),     # one gamma exactly 0
         ("no_drop",            70,                   32,  64,     5,  0.0, 0),
         ("stats_walk",         32 * 1024 + 70,       32,  32,     5,  0.5, 0),     # partial rows that merge two tiles
         ("walk",               32 * 4096 + 70,       32,  32,     5,  0.5, 0)]     # the backward's grid wraps
NAMES = [c[0] for c in CASES]
FORWARD = ("logp", "save_mean", "save_invstd", "running_mean", "running_var")
BACKWARD = ("dx", "dW1", "db1", "dgamma", "dbeta", "dW2", "db2")
DROP_SEED = 0x6A09E667
WALK_POOL = 67          # distinct input rows of the cases with more than 4096 rows (case_inputs)


def _mix32(x):
    x = x & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def keep_mask(seed, M, hidden, p):
    """bool [M, hidden]: keep(r hidden + c) = mix32(i ^ drop_base(seed, 0)) >= drop_threshold(p) -- csrc/kernels.h restated; p is the float
    the C ABI takes, so the threshold is that of the float32-rounded value.  p == 0 keeps everything."""
    if p == 0:
        return np.ones((M, hidden), dtype=bool)
    base = _mix32(np.array([seed & 0xFFFFFFFF], dtype=np.uint64))[0]           # (stream 0)
    t = float(np.float32(p)) * 4294967296.0
    thr = np.uint64(0xFFFFFFFF if t >= 4294967295.0 else int(t))
    i = np.arange(M * hidden, dtype=np.uint64)
    return (_mix32(i ^ base) >= thr).reshape(M, hidden)


def drop_scale(p):
    """1.0f / (1.0f - p) as the host forms it in float32, as an exact float64 constant."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def settle_beta(x, layer, e, margin=2.0 * RELU_MARGIN, step=2.0 ** -10):
    """seg_head_ref.settle_beta against the batch-statistics pre-activation: moves beta, in place, channel by channel to the nearest float32
    value b0 +- j step, j < 2048, at which no y = pre + beta of the channel lies within `margin` x its bar of zero.  pre and its bar do not
    depend on beta (fp_train_ref.forward_layer); every row strikes out the candidates it forbids at once."""
    x = np.asarray(x, dtype=np.float64)
    beta = layer[3]
    f = forward_layer(x, np.zeros_like(x), layer, e)
    pre, fixed = f["pre"], f["b_pre"]
    js = np.arange(-2048, 2048)
    for c in range(len(beta)):
        b0 = np.float32(beta[c])
        cands = (b0 + (js * step).astype(np.float32)).astype(np.float64)                   # ascending float32 values
        half = margin * (fixed[:, c] + 4.0 * EPS32 * np.abs(cands).max()) * (1.0 + 1e-9)
        struck = np.zeros(len(cands) + 1)
        np.add.at(struck, np.searchsorted(cands, -pre[:, c] - half, "left"), 1.0)
        np.add.at(struck, np.searchsorted(cands, -pre[:, c] + half, "right"), -1.0)
        free = np.flatnonzero(np.cumsum(struck)[:-1] == 0)
        assert len(free), f"no beta near {b0} clears channel {c}"
        beta[c] = np.float32(cands[free[np.argmin(np.abs(js[free]))]])
        assert (np.abs(pre[:, c] + np.float64(beta[c])) > margin * (fixed[:, c] + 4.0 * EPS32 * abs(np.float64(beta[c])))).all()


def case_inputs(synth, name, seed=None):
    """The seeded inputs of case `name` as a dict: x [M, cin], params (W1, b1, gamma, beta, running_mean, running_var, W2, b2) float32
    (the running statistics BEFORE the call), dlogp [M, C], eps, p, drop_seed."""
    _, M, cin, hidden, C, p, table_seed = next(c for c in CASES if c[0] == name)
    seed = table_seed if seed is None else seed             # (another seed: only to look for one that meets the conditions)
    base = 7000 + 97 * seed + 7 * NAMES.index(name)
    if M > 4096:
        # Tens of thousands of independent rows leave no beta that clears them all: the bar of the batch mean grows with sqrt(M), every row
        # forbids an interval of 16 bars around -pre, and together they cover the whole range (at M = 32 838 about three times over).  The
        # long cases therefore cycle through WALK_POOL distinct rows -- coprime with the 32 rows of a tile, so consecutive tiles start at
        # different places of the pool: a channel then has WALK_POOL distinct pre-activations, while the mask and dlogp differ row by row.
        x = np.ascontiguousarray(synth.uniform(base * 16 + 1, (WALK_POOL, cin), -1.0, 1.0)[np.arange(M) % WALK_POOL])
    else:
        x = synth.uniform(base * 16 + 1, (M, cin), -1.0, 1.0)
    layer = make_layers(base + 1, cin, [hidden], negative_gamma=name == "negative_gamma")[0]
    if name == "negative_gamma":
        assert (layer[2] < 0).any() and (layer[2] > 0).any()
        layer[2][1] = 0.0                                   # one gamma exactly 0
    settle_beta(x, layer, BN_EPS)
    k = 1.0 / np.sqrt(hidden)
    W2 = synth.uniform(base * 16 + 2, (C, hidden), -4.0 * k, 4.0 * k)          # (logits a few units apart: seg_head_ref.case_inputs)
    b2 = synth.uniform(base * 16 + 3, (C,), -1.0, 1.0)
    dlogp = synth.uniform(base * 16 + 4, (M, C), -1.0, 1.0)
    return dict(x=x, params=tuple(layer) + (W2, b2), dlogp=dlogp, eps=BN_EPS, p=p, drop_seed=DROP_SEED + NAMES.index(name))


def seg_train(x, params, eps, p, drop_seed, dlogp, margin=RELU_MARGIN, keep=None):
    """-> ({name: (value, bar)} for FORWARD + BACKWARD, worst): float64 values and float32 error bars of the outputs of the two train entry
    points (momentum MOMENTUM); worst = the smallest |y| / bar(y) over conv1's pre-activations.  keep: None, or a mask to use in place of
    keep_mask (the test of the test)."""
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[0]
    sq = np.sqrt(M)
    f = forward_layer(x, np.zeros_like(x), params[:6], eps)
    a, b_a, mu, b_mu, d, b_d, inv, b_inv, scale, b_scale, y, b_y = (f[q] for q in ("a", "b_a", "mu", "b_mu", "d", "b_d", "inv", "b_inv", "scale",
                                                                                   "b_scale", "y", "b_y"))
    worst = float((np.abs(y) / np.maximum(b_y, 1e-300)).min())
    assert worst > margin, f"a ReLU input lies within {margin} x its bar of zero (|y| / bar = {worst:.3g}): choose other inputs"
    out = dict(save_mean=(mu, b_mu), save_invstd=(inv, b_inv), running_mean=f["rm"], running_var=f["rv"])
    W1 = f["W"]
    W2, b2 = (np.asarray(v, dtype=np.float64) for v in params[6:])
    C, hidden = W2.shape
    keep = keep_mask(drop_seed, M, hidden, p) if keep is None else keep
    ds = drop_scale(p) if p else 1.0
    nr = 2.0 * EPS32 if p else 0.0                                             # (p == 0: no multiplication, no rounding)
    hd = np.maximum(y, 0.0) * keep * ds
    b_hd = keep * (b_y * ds + nr * np.abs(hd))
    z = hd @ W2.T + b2
    bz = b_hd @ np.abs(W2).T + 8.0 * EPS32 * np.sqrt(hidden) * (np.abs(hd) @ np.abs(W2).T + np.abs(b2)) + 2.0 * EPS32 * np.abs(z)
    dm = z - z.max(1, keepdims=True)
    ex = np.exp(dm)
    S = ex.sum(1, keepdims=True)
    logp = dm - np.log(S)
    rel_S = (ex / S * exp_rel(dm)).sum(1, keepdims=True) + (C - 1) * EPS32
    blogp = bz + bz.max(1, keepdims=True) + EPS32 * np.abs(dm) + rel_S + exp_rel(S) * np.abs(np.log(S)) + EPS32 * np.abs(logp)
    out["logp"] = (logp, blogp)
    # the backward: seg_head_ref's rules down to dh
    g = np.asarray(dlogp, dtype=np.float64)
    pr = np.exp(logp)
    bp = pr * (blogp + exp_rel(logp))
    sg = g.sum(1, keepdims=True)
    bsg = (C - 1) * EPS32 * np.abs(g).sum(1, keepdims=True)
    dz = g - pr * sg
    bdz = bp * np.abs(sg) + pr * bsg + bp * bsg + EPS32 * np.abs(dz)
    db2 = dz.sum(0)
    out["db2"] = (db2, bdz.sum(0) + 8.0 * EPS32 * sq * np.abs(dz).sum(0) + 2.0 * EPS32 * np.abs(db2))
    dW2 = dz.T @ hd
    out["dW2"] = (dW2, bdz.T @ np.abs(hd) + np.abs(dz).T @ b_hd + bdz.T @ b_hd + 8.0 * EPS32 * sq * (np.abs(dz).T @ np.abs(hd))
                  + 2.0 * EPS32 * np.abs(dW2))
    dh = dz @ W2
    bdh = bdz @ np.abs(W2) + 8.0 * EPS32 * np.sqrt(C) * (np.abs(dz) @ np.abs(W2)) + 2.0 * EPS32 * np.abs(dh)
    dhd = dh * keep * ds
    bdhd = keep * (bdh * ds + nr * np.abs(dhd))
    # conv1 through the statistics: fp_train_ref.fp_train's rules for one layer
    mask = y > 0.0
    dy, bdy = dhd * mask, bdhd * mask
    dbeta = dy.sum(0)
    b_dbeta = bdy.sum(0) + 8.0 * EPS32 * sq * np.abs(dy).sum(0) + 2.0 * EPS32 * np.abs(dbeta)
    G = (dy * a).sum(0)
    b_G = (bdy * np.abs(a) + np.abs(dy) * b_a + bdy * b_a).sum(0) + 8.0 * EPS32 * sq * np.abs(dy * a).sum(0) + 2.0 * EPS32 * np.abs(G)
    t = G - mu * dbeta
    b_t = b_G + np.abs(mu) * b_dbeta + b_mu * np.abs(dbeta) + b_mu * b_dbeta + 2.0 * EPS32 * (np.abs(G) + np.abs(mu * dbeta))
    dgamma = inv * t
    b_dgamma = inv * b_t + np.abs(t) * b_inv + b_t * b_inv + 2.0 * EPS32 * np.abs(dgamma)
    out["dbeta"] = (dbeta, b_dbeta)
    out["dgamma"] = (dgamma, b_dgamma)
    out["db1"] = (np.zeros_like(dbeta), np.zeros_like(dbeta))
    c1 = dbeta / M
    b_c1 = b_dbeta / M + 2.0 * EPS32 * np.abs(c1)
    c2 = dgamma * inv / M
    b_c2 = (b_dgamma * inv + np.abs(dgamma) * b_inv + b_dgamma * b_inv) / M + 4.0 * EPS32 * np.abs(c2)
    u = dy - c1
    b_u = bdy + b_c1 + 2.0 * EPS32 * np.abs(u)
    wv = u - d * c2
    b_w = b_u + b_d * np.abs(c2) + np.abs(d) * b_c2 + b_d * b_c2 + 2.0 * EPS32 * (np.abs(u) + np.abs(d * c2))
    dz1 = scale * wv
    bdz1 = np.abs(scale) * b_w + np.abs(wv) * b_scale + b_w * b_scale + 2.0 * EPS32 * np.abs(dz1)
    dW1 = dz1.T @ x
    out["dW1"] = (dW1, bdz1.T @ np.abs(x) + 8.0 * EPS32 * sq * (np.abs(dz1).T @ np.abs(x)) + 2.0 * EPS32 * np.abs(dW1))     # (b_x = 0)
    dx = dz1 @ W1
    out["dx"] = (dx, bdz1 @ np.abs(W1) + 8.0 * EPS32 * np.sqrt(W1.shape[0]) * (np.abs(dz1) @ np.abs(W1)) + 2.0 * EPS32 * np.abs(dx))
    return out, worst


def compose(x, params, eps, p, drop_seed, dlogp, dt):
    """The same formulas in numpy of dtype dt, nothing else shared with seg_train but the mask (BLAS / pairwise summation orders, not the
    kernels'): -> {FORWARD + BACKWARD}.  float32 must stay inside every bar."""
    x, W1, b1, gamma, beta, rmean, rvar, W2, b2, g = (np.asarray(v, dtype=dt) for v in (x,) + tuple(params) + (dlogp,))
    M = x.shape[0]
    a = x @ W1.T
    mu = a.mean(0, dtype=dt)
    d = a - mu
    var = (d * d).mean(0, dtype=dt)
    inv = dt(1.0) / np.sqrt(var + dt(np.float32(eps)))
    scale = gamma * inv
    y = d * scale + beta
    m = dt(np.float32(MOMENTUM))
    keep = keep_mask(drop_seed, M, W1.shape[0], p).astype(dt) * dt(drop_scale(p) if p else 1.0)
    hd = np.maximum(y, dt(0.0)) * keep
    z = hd @ W2.T + b2
    dm = z - z.max(1, keepdims=True)
    logp = dm - np.log(np.exp(dm).sum(1, keepdims=True))
    dz = g - np.exp(logp) * g.sum(1, keepdims=True)
    dy = (dz @ W2) * keep * (y > 0)
    dbeta, G = dy.sum(0), (dy * a).sum(0)
    dgamma = inv * (G - mu * dbeta)
    dz1 = scale * (dy - dbeta / dt(M) - d * (dgamma * inv / dt(M)))
    return dict(logp=logp, save_mean=mu, save_invstd=inv, running_mean=(dt(1.0) - m) * rmean + m * (mu + b1),
                running_var=(dt(1.0) - m) * rvar + m * (var * dt(M) / dt(M - 1)), dx=dz1 @ W1, dW1=dz1.T @ x, db1=np.zeros_like(dbeta),
                dgamma=dgamma, dbeta=dbeta, dW2=dz.T @ hd, db2=dz.sum(0))


_REFERENCES = {}


def reference(synth, name):
    """(inputs, {output: (value, bar)}, worst) of a case, computed once per process and shared: nobody writes to them."""
    if name not in _REFERENCES:
        i = case_inputs(synth, name)
        out, worst = seg_train(i["x"], i["params"], i["eps"], i["p"], i["drop_seed"], i["dlogp"])
        _REFERENCES[name] = (i, out, worst)
    return _REFERENCES[name]
