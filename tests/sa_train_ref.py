"""CPU restatement of the train-mode (batch-statistics) set abstraction, forward and backward, written from the spec in
include/ampnet_hip.h (ampnet_sa_train_forward_f32, ampnet_sa_train_backward_f32), in float64, with a derived float32 error bar per output
element; the seeded cases of tests/test_sa_train_gpu.py; the layer-local checker that reads the backward's own tape; and a float32 numpy
emulation of the path, so that the CPU test (tests/test_sa_train_ref_cpu.py) can check the yardstick, the seeds and the checker without a
GPU.  Test infrastructure: no GPU, no library."""
import numpy as np

import sa_bwd_ref
import sa_ref
from fp_bwd_ref import BN_EPS, RELU_MARGIN
from sa_bwd_ref import input_rows
from sa_ref import EPS32, make_layers

MOMENTUM = 0.1
N_CLOUDS = 2
UNDECIDED_BARS = 4.0            # a ReLU input within this many bars of zero is undecided for the layer-local checker
UNDECIDED_CAP = 1e-3            # .. and at most this share of a layer's elements may be

# The restatement cases: every one is compared element by element, none left out.  `base` seeds the clouds, the features and the layers;
# the cases that tests/sa_bwd_ref.py has under the same name keep its base, so that what it asserts of their balls holds here too.
# full64's cloud is scaled by 0.625, as there.
#         name               n     s     nsample  D    widths       radius  base
CASES = [("tail_group",      70,   9,    20,      6,   [32, 64],    0.35,   3000),       # repeated slots and padding rows
         ("no_feats",        70,   9,    32,      0,   [32],        0.35,   3007),       # no dfeats
         ("two_tiles",       150,  5,    48,      13,  [32, 64],    0.6,    3014),       # R = 64 with padding
         ("full64",          150,  5,    64,      16,  [64],        0.9,    3021),
         ("sparse_ball",     70,   9,    16,      8,   [32, 32],    0.12,   3049),       # some count == 1: all slots, not distinct members
         ("unpicked",        70,   9,    16,      8,   [32, 32],    0.12,   3056),       # exact-zero dfeats rows, and written
         ("negative_gamma",  70,   9,    20,      16,  [32, 64],    0.35,   3042),       # one gamma exactly 0
         ("dead_channel",    70,   9,    20,      6,   [32, 64],    0.35,   3070),       # as in fp_train_ref
         ("sa2_l0",          96,   6,    32,      64,  [64],        0.5,    3028),
         ("sa3_l0",          64,   4,    32,      128, [128],       0.6,    3035),
         ("widest_l0",       64,   3,    32,      317, [256],       0.6,    3063),
         # 2200 groups: more than the 1024 partial rows of the statistics passes and than the 2048 workgroups of the backward, so a wave
         # carries its statistics and its sums over several groups
         ("many_groups",     2200, 1100, 2,       8,   [32],        0.05,   3077)]
# Depth and width beyond what the bars of a chained restatement can settle (batch normalisation re-amplifies a carried bar by its |x^| /
# relative-spread factor per layer, fp_train_ref.COMPOSE): checked layer by layer on the kernel's own tape (check_layers below).
LOCAL = [("sa1_form",        96,   8,    32,      9,   [32, 32, 64],     0.4,   3084),
         ("sa2_form",        96,   6,    32,      64,  [64, 64, 128],    0.5,   3028),
         ("sa3_form",        64,   4,    32,      128, [128, 128, 256],  0.6,   3035),
         # (base: 3063, 3091 and 3098 put 1.1e-3 .. 1.3e-3 of one layer's ReLU inputs within four bars of zero, above check_layers' cap)
         ("widest",          64,   3,    32,      317, [256, 256, 256],  0.6,   3105),
         ("negative_gamma3", 70,   9,    20,      16,  [32, 64, 32],     0.35,  3042),
         ("many_groups3",    2200, 1100, 2,       8,   [32, 32, 32],     0.05,  3077)]


def case_inputs(synth, name):
    """The seeded inputs of case `name` (CASES or LOCAL) as a dict of numpy arrays: xyz [2, n, 3], centres [2, s] int32
    (arange(s) * (n // s) + 1), group_idx [2, s, nsample] int32 and count [2, s] (sa_ref.ball_query), feats [2, n, D] or None, layers
    (seeded; for CASES then settle_betas), eps, dout [2, s, cout_last], unpicked (per cloud the points that are in no group)."""
    _, n, s, nsample, D, widths, radius, base = next(c for c in CASES + LOCAL if c[0] == name)
    xyz = synth.clouds(base, N_CLOUDS, n)
    if name == "full64":
        xyz = xyz * np.float32(0.625)
    centres = np.tile((np.arange(s) * (n // s) + 1).astype(np.int32), (N_CLOUDS, 1))
    group_idx, count = (np.stack(a) for a in zip(*(sa_ref.ball_query(xyz[c], centres[c], radius, nsample) for c in range(N_CLOUDS))))
    feats = synth.uniform(base * 16 + 5, (N_CLOUDS, n, D), -1.0, 1.0) if D else None
    dout = synth.uniform(base * 16 + 7, (N_CLOUDS, s, widths[-1]), -1.0, 1.0)
    layers = make_layers(base + 1, 3 + D, widths, negative_gamma=name.startswith("negative_gamma"))
    dead_row = None
    if name.startswith("negative_gamma"):
        assert all((layer[2] < 0).any() and (layer[2] > 0).any() for layer in layers)
        layers[0][2][1] = 0.0                               # one gamma exactly 0
    if name == "dead_channel":
        dead_row = int(np.flatnonzero(layers[0][3] < -0.1)[0])     # a channel whose seeded beta is negative (fp_train_ref.DEAD_ROW's reason)
        layers[0][0][dead_row] = 0.0                        # a = 0 in every row: var = 0, invstd = 1 / sqrt(eps)
    eps = [BN_EPS] * len(widths)
    if name in [c[0] for c in CASES]:
        x, bx = input_rows(xyz, centres, group_idx, feats)
        settle_betas(x, bx, layers, eps)
    unpicked = [np.setdiff1d(np.arange(n), group_idx[c]) for c in range(N_CLOUDS)]
    if name == "unpicked":
        assert all(len(u) >= 2 for u in unpicked)
    if name == "sparse_ball":
        assert (count == 1).any() and count.max() <= 3      # some ball holds its centre alone: 15 of its 16 rows are repeats
    if name == "full64":
        assert (count == nsample).all()                     # every slot a distinct member
    if name in ("tail_group", "two_tiles"):
        assert (count < nsample).any()                      # repeated slots
    if name.startswith("many_groups"):
        assert N_CLOUDS * s > 2048
    return dict(xyz=xyz, centres=centres, group_idx=group_idx, count=count, feats=feats, layers=layers, eps=eps, dout=dout,
                unpicked=unpicked, nsample=nsample, dead_row=dead_row)


def forward_layer(x, bx, layer, e, unbiased=True, stat_rows=None):
    """One train-mode layer on rows x [M, cin] with bar bx -> a dict of float64 values and bars (b_*): fp_train_ref.forward_layer, whose
    docstring derives every bar.  stat_rows: None, or (the test of the test) a boolean row mask the statistics are restricted to."""
    W, b, gamma, beta, rmean, rvar = (np.asarray(v, dtype=np.float64) for v in layer)
    a = x @ W.T
    b_a = bx @ np.abs(W).T + 8.0 * EPS32 * np.sqrt(W.shape[1]) * (np.abs(x) @ np.abs(W).T) + 2.0 * EPS32 * np.abs(a)
    sa_, sb_a = (a, b_a) if stat_rows is None else (a[stat_rows], b_a[stat_rows])
    M = sa_.shape[0]
    sq = np.sqrt(M)
    mu = sa_.mean(0)
    b_mu = sb_a.mean(0) + 8.0 * EPS32 * sq * np.abs(sa_).mean(0) + 2.0 * EPS32 * np.abs(mu)
    d = a - mu
    b_d = b_a + b_mu + 2.0 * EPS32 * np.abs(d)
    sd, sb_d = (d, b_d) if stat_rows is None else (d[stat_rows], b_d[stat_rows])
    var = (sd * sd).mean(0)
    b_var = (2.0 * np.abs(sd) * sb_d + sb_d * sb_d).mean(0) + 8.0 * EPS32 * sq * var + 2.0 * EPS32 * var
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


def settle_betas(x, bx, layers, eps, margin=2.0 * RELU_MARGIN, step=2.0 ** -10):
    """fp_train_ref.settle_betas on the rows (x, bx): moves BatchNorm biases (beta) of `layers`, in place, until no ReLU input of any
    layer lies within `margin` x its bar of zero (a channel's beta shifts all its inputs together; a layer's batch statistics do not
    depend on its beta).  Twice the margin sa_train asserts is asked here, so that the assertion does not hang on a rounding."""
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


def backward_layer(f, dx, bdx, mutate=None, undecided=None):
    """One layer of the backward through the statistics on the forward record f (forward_layer) from dx [M, cout] with bar bdx ->
    a dict: dbeta, dgamma (value, bar), dz, b_dz, dW (value, bar), dx (value, bar) of the layer's input, and for `undecided` (a boolean
    mask of the elements whose ReLU the float32 path may have decided the other way) dz_alt: dz with the other branch of those elements.
    The rules are fp_train_ref.fp_train's, M the number of rows.  An undecided element stays in every comparison; in its column it widens
    the bars of dbeta and G by |dx| + b_dx and (|dx| + b_dx)(|a| + b_a): either branch of it is then inside."""
    x, bx, W, a, b_a, mu, b_mu, d, b_d = (f[q] for q in ("x", "bx", "W", "a", "b_a", "mu", "b_mu", "d", "b_d"))
    inv, b_inv, scale, b_scale = (f[q] for q in ("inv", "b_inv", "scale", "b_scale"))
    M = x.shape[0]
    sq = np.sqrt(M)
    mask = f["y"] > 0.0
    dy, bdy = dx * mask, bdx * mask
    dbeta = dy.sum(0)
    b_dbeta = bdy.sum(0) + 8.0 * EPS32 * sq * np.abs(dy).sum(0) + 2.0 * EPS32 * np.abs(dbeta)
    G = (dy * a).sum(0)
    b_G = (bdy * np.abs(a) + np.abs(dy) * b_a + bdy * b_a).sum(0) + 8.0 * EPS32 * sq * np.abs(dy * a).sum(0) + 2.0 * EPS32 * np.abs(G)
    if undecided is not None:
        wide = (np.abs(dx) + bdx) * undecided
        b_dbeta = b_dbeta + wide.sum(0)
        b_G = b_G + (wide * (np.abs(a) + b_a)).sum(0)
    t = G - mu * dbeta
    b_t = b_G + np.abs(mu) * b_dbeta + b_mu * np.abs(dbeta) + b_mu * b_dbeta + 2.0 * EPS32 * (np.abs(G) + np.abs(mu * dbeta))
    dgamma = inv * t
    b_dgamma = inv * b_t + np.abs(t) * b_inv + b_t * b_inv + 2.0 * EPS32 * np.abs(dgamma)
    c1 = dbeta / M
    b_c1 = b_dbeta / M + 2.0 * EPS32 * np.abs(c1)
    c2 = dgamma * inv / M
    b_c2 = (b_dgamma * inv + np.abs(dgamma) * b_inv + b_dgamma * b_inv) / M + 4.0 * EPS32 * np.abs(c2)
    if mutate == "no_xhat":
        c2 = np.zeros_like(c2)

    def form(dy, bdy):
        u = dy - c1
        b_u = bdy + b_c1 + 2.0 * EPS32 * np.abs(u)
        wv = u - d * c2
        b_w = b_u + b_d * np.abs(c2) + np.abs(d) * b_c2 + b_d * b_c2 + 2.0 * EPS32 * (np.abs(u) + np.abs(d * c2))
        dz = scale * wv
        return dz, np.abs(scale) * b_w + np.abs(wv) * b_scale + b_w * b_scale + 2.0 * EPS32 * np.abs(dz)

    dz, bdz = form(dy, bdy)
    res = dict(dbeta=(dbeta, b_dbeta), dgamma=(dgamma, b_dgamma), dz=dz, b_dz=bdz)
    if undecided is not None:
        res["dz_alt"], res["b_dz_alt"] = form(dx * (mask ^ undecided), bdx * (mask ^ undecided))
    dW = dz.T @ x
    res["dW"] = (dW, bdz.T @ np.abs(x) + np.abs(dz).T @ bx + bdz.T @ bx + 8.0 * EPS32 * sq * (np.abs(dz).T @ np.abs(x)) + 2.0 * EPS32 * np.abs(dW))
    res["dx"] = dgrad(dz, bdz, W)
    return res


def dgrad(dz, bdz, W):
    """dx = dz W over cout terms -> (value, bar)."""
    dx = dz @ W
    return dx, bdz @ np.abs(W) + 8.0 * EPS32 * np.sqrt(W.shape[0]) * (np.abs(dz) @ np.abs(W)) + 2.0 * EPS32 * np.abs(dx)


def gather_dfeats(dx, bdx, group_idx, n):
    """dfeats [B, n, D] = the sum over the entries with group_idx = j (clamped) of dx_0[entry, 3:], a plain sum of its c_j terms:
    bar sum b_dx0 + 8 e sqrt(c_j) sum |dx_0| + 2 e |dfeats| (sa_bwd_ref.sa_backward).  A point in no group: value 0, bar 0."""
    idx = np.clip(np.asarray(group_idx), 0, n - 1)
    B, s, nsample = idx.shape
    D = dx.shape[1] - 3
    g, bg = dx[:, 3:].reshape(B, s * nsample, D), bdx[:, 3:].reshape(B, s * nsample, D)
    df, carry, mag = (np.zeros((B, n, D)) for _ in range(3))
    cnt = np.zeros((B, n, 1))
    for c in range(B):
        flat = idx[c].reshape(-1)
        np.add.at(df[c], flat, g[c])
        np.add.at(carry[c], flat, bg[c])
        np.add.at(mag[c], flat, np.abs(g[c]))
        np.add.at(cnt[c], flat, 1.0)
    return df, carry + 8.0 * EPS32 * np.sqrt(cnt) * mag + 2.0 * EPS32 * np.abs(df)


def select_dout(arg, dout, nsample):
    """dx_L [M, cout_last]: dout[g, c] at row arg[g, c] of group g, 0 elsewhere (an exact selection: bar 0)."""
    B, s, cl = np.asarray(dout).shape
    dx4 = np.zeros((B, s, nsample, cl))
    np.put_along_axis(dx4, np.asarray(arg).astype(np.int64)[:, :, None, :], np.asarray(dout, dtype=np.float64)[:, :, None, :], 2)
    return dx4.reshape(B * s * nsample, cl)


def output_names(L, has_feats):
    return (["out"] + [f"{k}{l}" for l in range(L) for k in ("save_mean", "save_invstd", "running_mean", "running_var")]
            + (["dfeats"] if has_feats else []) + [f"{k}{l}" for l in range(L) for k in ("dW", "dbias", "dgamma", "dbeta")])


def forward_tape(xyz, centres, group_idx, feats, layers, eps, margin=RELU_MARGIN, mutate=None):
    """-> (tape, worst): per layer the record of forward_layer on the M = B s nsample rows (every slot a row, repeated or not); asserts
    the ReLU margin on every ReLU input of every layer.  mutate "biased": running_var from the biased variance; "distinct": the statistics
    over the first occurrence of every member only (the repeated slots left out)."""
    x, bx = input_rows(xyz, centres, group_idx, feats)
    stat_rows = None
    if mutate == "distinct":
        idx = np.asarray(group_idx)
        first = np.ones(idx.shape, bool)
        for t in range(1, idx.shape[2]):
            first[:, :, t] = (idx[:, :, :t] != idx[:, :, t:t + 1]).all(-1)
        stat_rows = first.reshape(-1)
    tape, worst = [], np.inf
    for layer, e in zip(layers, eps):
        f = forward_layer(x, bx, layer, e, unbiased=mutate != "biased", stat_rows=stat_rows)
        worst = min(worst, float((np.abs(f["y"]) / np.maximum(f["b_y"], 1e-300)).min()))
        tape.append(f)
        x, bx = np.maximum(f["y"], 0.0), f["b_y"]
    assert worst > margin, f"a ReLU input lies within {margin} x its bar of zero (|y| / bar = {worst:.3g}): choose other inputs"
    return tape, worst


def float64_argmax(tape, group_idx):
    """The lowest row of every (group, column) that attains the float64 maximum of relu(y): [B, s, cout_last] int32 (for the CPU tests;
    the GPU test takes the kernel's own choice)."""
    idx = np.asarray(group_idx)
    B, s, nsample = idx.shape
    v = np.maximum(tape[-1]["y"], 0.0).reshape(B, s, nsample, -1).copy()
    for t in range(1, nsample):                             # a repeated slot is its first member again: a matrix product may still round
        v[:, :, t][(idx[:, :, :t] == idx[:, :, t:t + 1]).any(-1)] = -1.0      # the two rows differently, so it is kept from winning
    return v.argmax(2).astype(np.int32)


def check_argmax(arg, f_last, group_idx):
    """sa_bwd_ref.check_argmax on the last layer's record: `arg` is in range, within the two bars of the float64 maximum, and the first
    occurrence of its source point."""
    sa_bwd_ref.check_argmax(arg, [(None, None, None, None, None, f_last["y"], f_last["b_y"])], group_idx)


def sa_train(xyz, centres, group_idx, feats, layers, eps, dout, arg, tape=None, mutate=None):
    """xyz [B, n, >= 3] float32, centres [B, s], group_idx [B, s, nsample] (taken as exact), feats [B, n, D] float32 or None, layers as
    sa_ref.make_layers (the last two entries: running_mean and running_var BEFORE the call), eps per layer, dout [B, s, cout_last], arg
    [B, s, cout_last] the row the max selected (an INPUT, as in sa_bwd_ref.sa_backward; check_argmax says whether a choice is admissible)
    -> {name: (value, bar)} with the names of output_names(): float64 values and float32 error bars of the outputs of
    ampnet_sa_train_forward_f32 and ampnet_sa_train_backward_f32 (momentum MOMENTUM).
    mutate: None, or a deliberate mistake for the test of the test -- "biased", "distinct" (forward_tape), "no_xhat" (dz without its
    x^ dgamma / M term).

    Values.  Rows x_0 = [xyz[idx_t] - xyz[centre], feats[idx_t]], M = B s nsample of them: a slot that repeats the group's first member is
    a row like any other.  Per layer over the M rows: a = x W^T, mu = mean a, d = a - mu, var = mean d^2, inv = 1 / sqrt(var + eps),
    scale = gamma inv, y = d scale + beta, x_{l+1} = relu(y); running_mean' = (1 - m) running_mean + m (mu + b), running_var' =
    (1 - m) running_var + m var M / (M - 1); out[g, c] = relu(y) of the last layer at row arg[g, c].  Backward: dx_L[(g, t), c] =
    dout[g, c] at t = arg[g, c], 0 elsewhere; dy = dx [y > 0], dbeta = sum dy, G = sum dy a, dgamma = inv (G - mu dbeta),
    dz = scale (dy - dbeta / M - d inv dgamma / M) for every row, dW = dz^T x, dx_l = dz W, dbias = 0; dfeats[j] = sum over the entries
    with group_idx = j (clamped) of dx_0[entry, 3:].

    Bars, e = 2^-24: fp_train_ref.fp_train's rules with M = B s nsample, and, as in sa_bwd_ref.sa_backward, x_0: e |dx| on the three
    coordinate differences, the features exact; the last layer's dx an exact selection of dout: bar 0; dfeats: gather_dfeats.  out: the bar
    of y at the selected row.  dbias: value 0, bar 0 -- exact zeros.  The ReLU margin |y| > 4 bar(y) is asserted for every element of
    every layer (settle_betas builds the cases to keep it); no element is ever left out of a comparison."""
    if tape is None:
        tape, _ = forward_tape(xyz, centres, group_idx, feats, layers, eps, mutate=mutate)
    B, s, nsample = np.asarray(group_idx).shape
    n = np.asarray(xyz).shape[1]
    out = {}
    for l, f in enumerate(tape):
        out[f"save_mean{l}"] = (f["mu"], f["b_mu"])
        out[f"save_invstd{l}"] = (f["inv"], f["b_inv"])
        out[f"running_mean{l}"] = f["rm"]
        out[f"running_var{l}"] = f["rv"]
    pick = np.asarray(arg).astype(np.int64)[:, :, None, :]
    y4, by4 = (tape[-1][k].reshape(B, s, nsample, -1) for k in ("y", "b_y"))
    out["out"] = (np.maximum(np.take_along_axis(y4, pick, 2)[:, :, 0], 0.0), np.take_along_axis(by4, pick, 2)[:, :, 0])
    dx, bdx = select_dout(arg, dout, nsample), 0.0
    bdx = np.zeros_like(dx)
    for l in range(len(layers) - 1, -1, -1):
        r = backward_layer(tape[l], dx, bdx, mutate=mutate)
        out[f"dbeta{l}"], out[f"dgamma{l}"], out[f"dW{l}"] = r["dbeta"], r["dgamma"], r["dW"]
        out[f"dbias{l}"] = (np.zeros_like(r["dbeta"][0]), np.zeros_like(r["dbeta"][0]))
        dx, bdx = r["dx"]
    if feats is not None:
        out["dfeats"] = gather_dfeats(dx, bdx, group_idx, n)
    return out


# ---- layer-local: every layer alone, on the kernel's own x_l and dz_l -------------------------------------------------------------------
def check_layers(i, got):
    """The depth-and-width check.  i: case inputs; got: what the kernels returned as numpy arrays -- out, arg [B, s, cout_last], dfeats (or
    absent), and per layer l: x{l} [M, >= cin_l] and dz{l} [M, cout_l] read from the backward's tape, save_mean{l}, save_invstd{l},
    running_mean{l}, running_var{l}, dW{l}, dgamma{l}, dbeta{l}.  Every layer is checked ALONE, its float32 x_l and dz_l (and dz_{l+1})
    taken as exact inputs, against one-layer bars (forward_layer with b_x = 0, backward_layer, dgrad):
      save_mean_l, save_invstd_l, running statistics from x_l;  x_{l+1} = relu(bn(x_l W^T)) (the ReLU is continuous: no mask), for the last
      layer out[g, c] at arg and check_argmax;  dW_l = dz_l^T x_l;  dx_l = dz_{l+1} W_{l+1} (dx_L from arg and dout) and from it dbeta_l,
      dgamma_l and dz_l;  dfeats against the gather of dx_0 = dz_0 W_0.
    An element whose float64 |y| is within UNDECIDED_BARS bars of zero is undecided: it is not excluded, its dz must match one of the two
    branches, and it widens its column's bars (backward_layer).  At most UNDECIDED_CAP of a layer's elements may be undecided.
    -> {name: worst error / bar, and undecided{l}: the undecided share of layer l / UNDECIDED_CAP}; asserts nothing but the cap, the shapes
    and check_argmax."""
    layers, eps = i["layers"], i["eps"]
    L = len(layers)
    B, s, nsample = i["group_idx"].shape
    n = i["xyz"].shape[1]
    M = B * s * nsample
    ratios = {}

    def ratio(name, v, want, bar):
        assert v.shape == want.shape, (name, v.shape, want.shape)
        err = np.abs(v.astype(np.float64) - want)
        ratios[name] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())

    dzs = [got[f"dz{l}"].astype(np.float64) for l in range(L)]
    for l in range(L - 1, -1, -1):
        cin = layers[l][0].shape[1]
        x = got[f"x{l}"].astype(np.float64)
        assert x.shape[0] == M and (x[:, cin:] == 0).all(), f"x{l}: the padded columns are not zero"
        f = forward_layer(x[:, :cin], np.zeros((M, cin)), layers[l], eps[l])
        ratio(f"save_mean{l}", got[f"save_mean{l}"], f["mu"], f["b_mu"])
        ratio(f"save_invstd{l}", got[f"save_invstd{l}"], f["inv"], f["b_inv"])
        ratio(f"running_mean{l}", got[f"running_mean{l}"], *f["rm"])
        ratio(f"running_var{l}", got[f"running_var{l}"], *f["rv"])
        if l == L - 1:
            check_argmax(got["arg"], f, i["group_idx"])
            pick = got["arg"].astype(np.int64)[:, :, None, :]
            y4, by4 = (f[k].reshape(B, s, nsample, -1) for k in ("y", "b_y"))
            ratio("out", got["out"], np.maximum(np.take_along_axis(y4, pick, 2)[:, :, 0], 0.0), np.take_along_axis(by4, pick, 2)[:, :, 0])
            dx = select_dout(got["arg"], i["dout"], nsample)
            bdx = np.zeros_like(dx)
        else:
            cout = layers[l][0].shape[0]
            ratio(f"x{l + 1}", got[f"x{l + 1}"][:, :cout], np.maximum(f["y"], 0.0), f["b_y"])
            dx, bdx = dgrad(dzs[l + 1], np.zeros_like(dzs[l + 1]), np.asarray(layers[l + 1][0], dtype=np.float64))
        und = np.abs(f["y"]) <= UNDECIDED_BARS * f["b_y"]
        share = float(und.mean())
        ratios[f"undecided{l}"] = share / UNDECIDED_CAP
        assert share <= UNDECIDED_CAP, f"layer {l}: {share:.3g} of the ReLU inputs lie within {UNDECIDED_BARS} bars of zero"
        r = backward_layer(f, dx, bdx, undecided=und)
        ratio(f"dbeta{l}", got[f"dbeta{l}"], *r["dbeta"])
        ratio(f"dgamma{l}", got[f"dgamma{l}"], *r["dgamma"])
        e_main = np.abs(dzs[l] - r["dz"]) / np.maximum(r["b_dz"], 1e-300)
        e_alt = np.abs(dzs[l] - r["dz_alt"]) / np.maximum(r["b_dz_alt"], 1e-300)
        e = np.where(und, np.minimum(e_main, e_alt), e_main)
        ratios[f"dz{l}"] = float(np.where(dzs[l] == r["dz"], 0.0, e).max())
        dW = dzs[l].T @ x[:, :cin]
        ratio(f"dW{l}", got[f"dW{l}"], dW, 8.0 * EPS32 * np.sqrt(M) * (np.abs(dzs[l]).T @ np.abs(x[:, :cin])) + 2.0 * EPS32 * np.abs(dW))
    if i["feats"] is not None:
        dx0, bdx0 = dgrad(dzs[0], np.zeros_like(dzs[0]), np.asarray(layers[0][0], dtype=np.float64))
        ratio("dfeats", got["dfeats"], *gather_dfeats(dx0, bdx0, i["group_idx"], n))
    return ratios


def emulate_f32(i):
    """The path of the two entry points in float32 numpy (numpy's own summation orders) -> the dict check_layers takes, plus dbias{l}.  It
    stands in for the kernel where there is no GPU: tests/test_sa_train_ref_cpu.py runs check_layers on it."""
    f32 = np.float32
    xyz, group_idx, centres = i["xyz"], i["group_idx"], i["centres"]
    B, s, nsample = group_idx.shape
    n = xyz.shape[1]
    M = B * s * nsample
    rows = np.stack([xyz[c][group_idx[c]] - xyz[c][centres[c]][:, None, :] for c in range(B)]).astype(f32)
    if i["feats"] is not None:
        rows = np.concatenate([rows, np.stack([i["feats"][c][group_idx[c]] for c in range(B)])], -1)
    x = np.ascontiguousarray(rows.reshape(M, -1), dtype=f32)
    got, tape = {}, []
    m = f32(MOMENTUM)
    for l, ((W, b, gamma, beta, rm, rv), e) in enumerate(zip(i["layers"], i["eps"])):
        a = x @ W.T
        mu = a.mean(0, dtype=f32)
        d = a - mu
        var = (d * d).mean(0, dtype=f32)
        inv = (f32(1.0) / np.sqrt(var + f32(e))).astype(f32)
        scale = gamma * inv
        y = a * scale + (beta - mu * scale)
        got.update({f"x{l}": x, f"save_mean{l}": mu, f"save_invstd{l}": inv, f"running_mean{l}": m * (mu + b) + (f32(1.0) - m) * rm,
                    f"running_var{l}": m * (var * f32(M) / f32(M - 1)) + (f32(1.0) - m) * rv})
        tape.append((x, W, a, mu, inv, scale, y))
        x = np.maximum(y, f32(0.0))
    v = x.reshape(B, s, nsample, -1)
    got["arg"] = v.argmax(2).astype(np.int32)
    got["out"] = v.max(2)
    dx = select_dout(got["arg"], i["dout"], nsample).astype(f32)
    for l in range(len(tape) - 1, -1, -1):
        x, W, a, mu, inv, scale, y = tape[l]
        dy = np.where(y > 0, dx, f32(0.0))
        dbeta = dy.sum(0, dtype=f32)
        dgamma = inv * ((dy * a).sum(0, dtype=f32) - mu * dbeta)
        dz = (scale * ((dy - dbeta / f32(M)) - (a - mu) * (dgamma * inv / f32(M)))).astype(f32)
        got.update({f"dz{l}": dz, f"dbeta{l}": dbeta, f"dgamma{l}": dgamma, f"dbias{l}": np.zeros_like(dbeta), f"dW{l}": dz.T @ x})
        dx = dz @ W
    if i["feats"] is not None:
        D = i["feats"].shape[2]
        df = np.zeros((B, n, D), f32)
        g = dx[:, 3:].reshape(B, s * nsample, D)
        for c in range(B):
            np.add.at(df[c], np.clip(group_idx[c].reshape(-1), 0, n - 1), g[c])
        got["dfeats"] = df
    return got
