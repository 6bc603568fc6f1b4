"""CPU restatement of set abstraction over ONE group of all points (include/ampnet_hip.h: ampnet_sa_all_forward_f32,
ampnet_sa_all_backward_f32) in float64 with derived float32 bars, built from tests/sa_ref.py and tests/sa_bwd_ref.py: an origin point is
appended to every cloud and used as the single centre, with group_idx = arange(N), so the values and the bars are the ball-query
restatement's.  Also the winner compaction of the backward restated in numpy, and the seeded cases of tests/test_sa_all_gpu.py and
tests/test_sa_all_backward_gpu.py.  Test infrastructure: no GPU, no library."""
import numpy as np

import sa_bwd_ref
import sa_ref
from fp_bwd_ref import BN_EPS, RELU_MARGIN

CHUNK = 32
N_CLOUDS = 2
#         name            n    D    widths
CASES = [("n1",           1,   6,   [32]),
         ("n5",           5,   0,   [32, 64]),              # fewer winners than one chunk
         ("n31",          31,  13,  [32, 32, 64]),
         ("n32",          32,  6,   [32, 64]),
         ("n33",          33,  0,   [32]),
         ("n64",          64,  13,  [32, 64]),
         ("n65",          65,  6,   [32, 32, 64]),
         ("n70",          70,  0,   [32, 32, 64]),
         ("n150",         150, 13,  [32, 32, 64]),
         ("n150_one",     150, 6,   [32]),
         ("n150_chunks",  150, 6,   [32, 128]),             # more than 32 distinct winners: two chunks are used, two are empty
         ("duplicates",   70,  6,   [32, 64]),              # rows 35 .. 69 repeat rows 0 .. 34: every tie goes to the lower row
         ("dead_channel", 33,  6,   [32, 64]),              # channel 3 of the last layer is negative on every row: max 0, row 0, no gradient
         ("wide",         70,  256, [256, 256, 256])]       # more than 32 distinct winners: several chunks
DEAD = 3


def as_group(xyz, feats):
    """The cloud with an origin point appended, that point as the single centre and all N real points as its group ->
    (xyz1 [B, N + 1, 3], feats1 [B, N + 1, D] or None, centres [B, 1], group_idx [B, 1, N])."""
    xyz = np.asarray(xyz)[..., :3]
    B, N = xyz.shape[:2]
    xyz1 = np.concatenate([xyz, np.zeros((B, 1, 3), xyz.dtype)], 1)
    feats1 = None if feats is None else np.concatenate([feats, np.zeros((B, 1, feats.shape[2]), feats.dtype)], 1)
    return xyz1, feats1, np.full((B, 1), N, np.int32), np.tile(np.arange(N, dtype=np.int32), (B, 1, 1))


def case_inputs(synth, name):
    """The seeded inputs of case `name`: xyz [2, n, 3], feats [2, n, D] or None, layers (seeded, then sa_bwd_ref.settle_betas), eps,
    dout [2, cout_last]."""
    _, n, D, widths = next(c for c in CASES if c[0] == name)
    base = 5000 + 7 * [c[0] for c in CASES].index(name)
    xyz = synth.clouds(base, N_CLOUDS, n)
    feats = synth.uniform(base * 16 + 5, (N_CLOUDS, n, D), -1.0, 1.0) if D else None
    if name == "duplicates":
        xyz[:, 35:] = xyz[:, :35]
        feats[:, 35:] = feats[:, :35]
    dout = synth.uniform(base * 16 + 7, (N_CLOUDS, widths[-1]), -1.0, 1.0)
    layers = sa_ref.make_layers(base + 1, 3 + D, widths)
    if name == "dead_channel":
        layers[-1][2][DEAD] = 0.0                           # scale 0: y = beta on every row
        layers[-1][3][DEAD] = -1.0
    eps = [BN_EPS] * len(widths)
    x, bx = _rows(xyz, feats)
    sa_bwd_ref.settle_betas(x, bx, layers, eps)
    return dict(xyz=xyz, feats=feats, layers=layers, eps=eps, dout=dout)


def _rows(xyz, feats):
    xyz1, feats1, cen, gi = as_group(xyz, feats)
    return sa_bwd_ref.input_rows(xyz1, cen, gi, feats1)


def forward(xyz, feats, layers, eps):
    """-> (out [B, cout_last] float64, bar): sa_ref.sa_forward on the one group of every cloud."""
    xyz1, feats1, cen, gi = as_group(xyz, feats)
    res = [sa_ref.sa_forward(xyz1[c], cen[c], gi[c], None if feats1 is None else feats1[c], layers, eps) for c in range(xyz1.shape[0])]
    return np.stack([r[0][0] for r in res]), np.stack([r[1][0] for r in res])


def forward_tape(xyz, feats, layers, eps):
    """sa_bwd_ref.forward_tape on the B N rows (its ReLU-margin assertion included) -> (tape, worst)."""
    xyz1, feats1, cen, gi = as_group(xyz, feats)
    return sa_bwd_ref.forward_tape(xyz1, cen, gi, feats1, layers, eps)


def float64_argmax(tape, B):
    """[B, cout_last] int32: the lowest row of every (cloud, column) that attains the float64 maximum of relu(y)."""
    v = np.maximum(tape[-1][5], 0.0)
    return v.reshape(B, -1, v.shape[1]).argmax(1).astype(np.int32)


def check_argmax(arg, tape, xyz, feats):
    """sa_bwd_ref.check_argmax restated for one group of N rows: `arg` [B, cout_last] is in [0, N), attains the float64 maximum within the
    two bars, and is the LOWEST of the rows whose inputs [xyz, feats] are bit-identical to its own (identical rows give identical bits)."""
    xyz = np.asarray(xyz)[..., :3]
    B, N = xyz.shape[:2]
    arg = np.asarray(arg)
    sa_bwd_ref.check_argmax(arg[:, None, :], tape, np.tile(np.arange(N, dtype=np.int32), (B, 1, 1)))
    rows = xyz if feats is None else np.concatenate([xyz, feats], -1)
    for b in range(B):
        first = np.array([int(np.flatnonzero((rows[b] == rows[b, j]).all(-1))[0]) for j in range(N)])
        assert (first[arg[b]] == arg[b]).all(), "arg is a duplicate of a lower row"


def backward(xyz, feats, layers, eps, dout, arg, tape=None):
    """-> {name: (value, bar)} with sa_bwd_ref.output_names(): sa_bwd_ref.sa_backward on the one group per cloud, the origin point's row
    of dfeats (it is in no group: exact zeros) dropped."""
    xyz1, feats1, cen, gi = as_group(xyz, feats)
    out = sa_bwd_ref.sa_backward(xyz1, cen, gi, feats1, layers, eps, np.asarray(dout)[:, None, :], np.asarray(arg)[:, None, :], tape)
    if feats is not None:
        v, bar = out["dfeats"]
        assert (v[:, -1] == 0).all() and (bar[:, -1] == 0).all()
        out["dfeats"] = (v[:, :-1], bar[:, :-1])
    return out


def compact(arg, dout, n):
    """The backward's winner compaction.  arg, dout [B, C] -> (winners: per cloud the distinct values of arg (clamped to [0, n)) ascending;
    group_idx [B, K, 32]: chunk k holds winners 32 k .. 32 k + 31 as ROW NUMBERS of the cloud, padded with the chunk's first member, an
    empty chunk with winner 0; dout_k [B, K, C]: dout where arg's winner lies in chunk k, 0 elsewhere; slot [B, C]: the place of column c's
    winner inside its chunk), K = C / 32."""
    arg = np.clip(np.asarray(arg), 0, n - 1)
    B, C = arg.shape
    K = C // CHUNK
    winners, gi = [], np.zeros((B, K, CHUNK), np.int32)
    dout_k, slot = np.zeros((B, K, C), np.asarray(dout).dtype), np.zeros((B, C), np.int32)
    for b in range(B):
        w = np.unique(arg[b])                               # sorted, distinct
        winners.append(w)
        rank = np.searchsorted(w, arg[b])
        for k in range(K):
            members = w[CHUNK * k:CHUNK * (k + 1)]
            head = members[0] if len(members) else w[0]
            gi[b, k] = head
            gi[b, k, :len(members)] = members
            here = rank // CHUNK == k
            dout_k[b, k, here] = np.asarray(dout)[b, here]
        slot[b] = rank % CHUNK
    return winners, gi, dout_k, slot


def backward_compacted(xyz, feats, layers, eps, dout, arg):
    """The backward over the compacted chunks alone, as the kernels run it: sa_bwd_ref.sa_backward on K groups of 32 rows per cloud around
    the origin point with the masked dout_k.  In a chunk, a column whose winner is there takes that winner's slot; every other column has
    dout_k = 0 and takes slot 0.  -> ({name: (value, bar)}, winners, chunk tape, group_idx, slot)."""
    xyz1, feats1, _, _ = as_group(xyz, feats)
    B, N = np.asarray(xyz).shape[:2]
    winners, gi, dout_k, slot = compact(arg, dout, N)
    K = gi.shape[1]
    cen = np.full((B, K), N, np.int32)
    rank_chunk = np.stack([np.searchsorted(winners[b], np.clip(np.asarray(arg)[b], 0, N - 1)) // CHUNK for b in range(B)])
    arg_k = np.where(rank_chunk[:, None, :] == np.arange(K)[None, :, None], slot[:, None, :], 0).astype(np.int32)
    tape, _ = sa_bwd_ref.forward_tape(xyz1, cen, gi, feats1, layers, eps)
    out = sa_bwd_ref.sa_backward(xyz1, cen, gi, feats1, layers, eps, dout_k, arg_k, tape)
    if feats is not None:
        v, bar = out["dfeats"]
        out["dfeats"] = (v[:, :-1], bar[:, :-1])
    return out, winners, tape, gi, arg_k
