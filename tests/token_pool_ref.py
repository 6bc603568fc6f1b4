"""CPU restatement of the window token (include/ampnet_hip.h: ampnet_token_pool_forward_f32, ampnet_token_pool_backward_f32) in float64
with float32 bars from tests/pw_probe.py::bar, and the seeded cases of tests/test_token_pool_gpu.py.
    forward    y[r, c] = W[c, :] . x[r, :] + bias[c];  out[q, c] = max over cloud q's rows;  arg = the LOWEST row attaining it
    backward   given arg: dx (zero outside the winners), dW, db
Test infrastructure: no GPU, no library."""
import numpy as np

from pw_probe import bar


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def row_values(rows, W, bias):
    """-> (y64 [total, cout], b [total, cout]): every row's float64 value and its bar, bar(|W| |x| + |bias|, y64, K = cin)."""
    x, w, bb = np.asarray(rows, np.float64), np.asarray(W, np.float64), np.asarray(bias, np.float64)
    y = x @ w.T + bb
    mag = np.abs(x) @ np.abs(w).T + np.abs(bb)
    return y, bar(mag, y, x.shape[1])


def forward(rows, sizes, W, bias):
    """-> (out64 [Q, cout], arg [Q, cout] int32: the lowest row inside its cloud attaining the float64 max, bar_out [Q, cout] = the largest
    row bar of the cloud: max is 1-Lipschitz in the sup norm)."""
    y, b = row_values(rows, W, bias)
    off = offsets(sizes)
    out = np.stack([y[off[q]:off[q + 1]].max(0) for q in range(len(sizes))])
    arg = np.stack([y[off[q]:off[q + 1]].argmax(0) for q in range(len(sizes))]).astype(np.int32)
    bar_out = np.stack([b[off[q]:off[q + 1]].max(0) for q in range(len(sizes))])
    return out, arg, bar_out


def check_arg(arg, rows, sizes, W, bias):
    """`arg` [Q, cout] lies inside its cloud and its float64 value attains the float64 max within twice the cloud's bar."""
    y, _ = row_values(rows, W, bias)
    out, _, bar_out = forward(rows, sizes, W, bias)
    off = offsets(sizes)
    arg = np.asarray(arg)
    for q, n in enumerate(sizes):
        assert ((arg[q] >= 0) & (arg[q] < n)).all(), f"cloud {q}: arg outside [0, {n})"
        got = y[off[q] + arg[q], np.arange(y.shape[1])]
        assert (got >= out[q] - 2 * bar_out[q]).all(), f"cloud {q}: arg does not attain the max"


def backward(rows, sizes, W, arg, dout):
    """Given arg (clamped into its cloud) -> {name: (value float64, bar)} for dx [total, cin], dW [cout, cin], db [cout].  The bars: `bar`
    with the float64 product of the absolute operands and K = the number of summed terms -- the channels a row won for dx, Q for dW, db."""
    x, w, g = np.asarray(rows, np.float64), np.asarray(W, np.float64), np.asarray(dout, np.float64)
    off = offsets(sizes)
    Q, cout = g.shape
    dx, mdx, kdx = np.zeros_like(x), np.zeros_like(x), np.zeros(x.shape[0])
    dW, mdW = np.zeros_like(w), np.zeros_like(w)
    for q, n in enumerate(sizes):
        a = np.clip(np.asarray(arg)[q], 0, n - 1) + off[q]
        for c in range(cout):
            dx[a[c]] += g[q, c] * w[c]
            mdx[a[c]] += abs(g[q, c]) * np.abs(w[c])
            kdx[a[c]] += 1
        dW += g[q][:, None] * x[a]
        mdW += np.abs(g[q])[:, None] * np.abs(x[a])
    db, mdb = g.sum(0), np.abs(g).sum(0)
    return {"dx": (dx, bar(mdx, dx, kdx[:, None])), "dW": (dW, bar(mdW, dW, Q)), "db": (db, bar(mdb, db, Q))}


def winner_rows(arg, sizes):
    """bool [total]: the rows some channel's arg names."""
    off = offsets(sizes)
    hit = np.zeros(off[-1], bool)
    for q, n in enumerate(sizes):
        hit[off[q] + np.clip(np.asarray(arg)[q], 0, n - 1)] = True
    return hit


# ---- the cases of tests/test_token_pool_gpu.py -----------------------------------------------------------------------------------------
G_TILES = 32 * 256 * 2 + 5            # many_tiles: 513 tiles of one cloud, then a cloud of one row
#         name          sizes                 cin  cout
CASES = [("model",      [64, 64, 64],         128, 128),
         ("n1",         [1, 1, 1],            32,  32),
         ("borders",    [31, 32, 33, 1, 65],  32,  64),
         ("wide",       [40, 40],             256, 256),
         ("duplicates", [70],                 64,  32),
         ("negative",   [33, 5],              32,  32),
         ("many_tiles", [G_TILES, 1],         32,  32),
         # beyond the cases the feature was specified with: more tiles than items, so an item is a run of SEVERAL tiles (the merge of a
         # later tile into a run's partial), clouds that start and end inside items, and one that spans three
         ("long_runs",  [4096 * 32 * 2 + 7, 3, 40, 200, 1], 32, 32)]
NAMES = [c[0] for c in CASES]


def planted_rows(name, sizes):
    """The rows of cloud 0 that get a planted winner: the first tile, tile and run borders in mid-cloud, the last full tile and the ragged
    tail (many_tiles: every tile is a run; long_runs: a run is three tiles)."""
    n = sizes[0]
    t = (n + 31) // 32
    if name == "many_tiles":
        return [3, 32 * 256 - 1, 32 * 256, 32 * 257 + 9, 32 * (t - 1) - 1, n - 2]
    if name == "long_runs":
        return [5, 32 * 3 - 1, 32 * 3, 32 * 3 * (t // 6) + 1, 32 * (t - 2) + 4, n - 3]
    return []


def case_inputs(synth, name):
    """-> dict(rows [total, cin], sizes, W, bias, dout [Q, cout]) float32, seeded."""
    _, sizes, cin, cout = next(c for c in CASES if c[0] == name)
    base = 9100 + 11 * NAMES.index(name)
    total = sum(sizes)
    W = synth.uniform(base + 1, (cout, cin), -1.0, 1.0) / np.float32(np.sqrt(cin))
    bias = synth.uniform(base + 2, (cout,), -0.5, 0.5)
    if name in ("many_tiles", "long_runs"):
        # constant rows (every row ties: row 0 would win everything), with winners planted: the i-th planted row is the constant row plus
        # a step along W[i, :] that lifts channel i by 4, more than the other planted rows lift it, so it wins channel i at least
        one = synth.uniform(base + 3, (1, cin), 0.5, 1.0)
        rows = np.repeat(one, total, 0)
        for i, p in enumerate(planted_rows(name, sizes)):
            rows[p] = one[0] + np.float32(4.0) * W[i] / np.float32(W[i] @ W[i])
        off = offsets(sizes)
        rows[off[1]:] = synth.uniform(base + 4, (total - sizes[0], cin), -1.0, 1.0)
    else:
        rows = synth.uniform(base + 3, (total, cin), -1.0, 1.0)
    if name == "duplicates":
        rows[35:] = rows[:35]
    if name == "negative":
        bias = np.full((cout,), -50.0, np.float32)
    dout = synth.uniform(base + 5, (len(sizes), cout), -1.0, 1.0)
    return dict(rows=np.ascontiguousarray(rows, np.float32), sizes=list(sizes), W=W.astype(np.float32), bias=bias.astype(np.float32), dout=dout)


def hand_args(sizes, cout):
    """Two hand-made args.  The first: in cloud 0 (of three rows or more) the last row wins ONE channel and the row before it TWO, the
    other channels and clouds are spread over the rows.  The second: in every cloud one row wins ALL channels."""
    spread = np.stack([np.arange(cout) % n for n in sizes]).astype(np.int32)
    n0 = sizes[0]
    if n0 >= 3:
        spread[0] = np.arange(cout) % (n0 - 2)
        spread[0, 0] = n0 - 1
        spread[0, 1] = spread[0, 2] = n0 - 2
    every = np.stack([np.full(cout, n // 2) for n in sizes]).astype(np.int32)
    return [spread, every]

