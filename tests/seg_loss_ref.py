"""The yardstick of the loss kernel behind the segmentation head (csrc/seg_loss.hip, include/ampnet_hip.h: ampnet_seg_nll_forward_f32): a
float64 numpy restatement of the masked, weighted NLL, the predictions and the confusion counts, and the seeded cases the GPU test runs.
Test infrastructure; tests/test_seg_loss_ref_cpu.py checks it against torch's float64 F.nll_loss.

The bars of tests/test_seg_loss_gpu.py are derived, not measured:
  sums   the kernel adds float64 terms that are exact (w[t] * -logp is a product of two float32 values), so its only error is the
         additions'.  Its longest chain: a thread's rows (at most 2 at the sizes here), 6 shuffle steps, 4 waves, at most 1024 partial rows
         -- below 2^12 additions of non-negative terms, each within 2^-53 relative of its exact value: 2^12 * 2^-53 < 1e-12 of the sum
         (math.fsum gives the reference sums correctly rounded);
  loss   the float64 quotient is within 1e-12 relative of the reference's, far inside the float32 grid; one rounding to float32: 1 ulp;
  dlogp  2 ulp of the float64 formula.  The kernel forms -(w[t] g) / sums[1] in float64 and rounds once (half an ulp).  A float32
         statement -(w[t] g) / (float)sums[1] -- the rounding of sums[1], of the product and of the quotient, with mantissas m_W, m_P, m_Q --
         is (m_Q / m_W + m_Q / m_P + 1) / 2 ulp off in the worst case, up to 2.5: it measured 2.04 ulp at M = 257, C = 32, weighted, and
         missed the bar, which is why the kernel does not compute it that way;
  preds, counts   integers: exact."""
import functools
import math

import numpy as np

ROWS = (1, 63, 64, 65, 257, 4099, 256 * 1024 + 3)      # one wave less one, one wave, one more, two workgroups, odd, the grid-stride loop
CLASSES = (2, 5, 32)
GRAD = np.float32(0.73)                                # the upstream gradient of the backward checks


def nll(logp, target, w):
    """float64 statement of the forward: logp [M, C], target [M] int64, w [C] or None
    -> dict(sums [2], loss, preds [M], counts [C * C + 1], live [M] bool)."""
    M, C = logp.shape
    lp = logp.astype(np.float64)
    w64 = np.ones(C) if w is None else w.astype(np.float64)
    live = (target >= 0) & (target < C)
    t = np.where(live, target, 0)
    wt = np.where(live, w64[t], 0.0)
    num, den = math.fsum(wt * -lp[np.arange(M), t]), math.fsum(wt)      # correctly rounded sums
    preds = lp.argmax(1).astype(np.int64)                               # numpy: the FIRST of equal maxima, i.e. the lowest class
    counts = np.zeros(C * C + 1, dtype=np.int64)
    np.add.at(counts, t[live] * C + preds[live], 1)
    counts[C * C] = int((~live).sum())
    return dict(sums=np.array([num, den]), loss=num / den if den != 0.0 else float("nan"), preds=preds, counts=counts, live=live)


def nll_backward(target, w, den, g, C):
    """float64 statement of the backward for the upstream gradient g: dlogp [M, C], -(w[t] g) / den at (m, t) of a live row, 0 elsewhere."""
    M = target.shape[0]
    w64 = np.ones(C) if w is None else w.astype(np.float64)
    live = (target >= 0) & (target < C)
    d = np.zeros((M, C))
    rows = np.arange(M)[live]
    d[rows, target[live]] = -(w64[target[live]] * float(g)) / den
    return d


@functools.lru_cache(maxsize=None)
def case(M, C, weighted):
    """The seeded inputs of one (M, C, weighted) case and their reference, computed once and shared: logp a float32 log_softmax of seeded
    logits with the two largest entries of 5 % of the rows made equal (the tie rule), about 20 % of the targets -1, the targets drawn from
    [0, C - 1) so that class C - 1 never occurs, and -- from 3 rows on -- one target out of range on the far side (C + 3) in the middle
    row.  M = 1 is a single live row."""
    from conftest import sub
    synth = sub("synthetic")
    seed = 7000 + 37 * M % 1000 + 11 * C + int(weighted)
    z = synth.uniform(seed, (M, C), -4.0, 4.0).astype(np.float64)
    z -= z.max(1, keepdims=True)
    logp = (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)
    tie = synth.uniform01(seed + 1, (M,)) < 0.05
    order = np.argsort(logp, axis=1, kind="stable")
    top, second = order[:, -1], order[:, -2]
    rows = np.arange(M)[tie]
    logp[rows, second[tie]] = logp[rows, top[tie]]
    target = synth.randint(seed + 2, (M,), 0, C - 1)
    if M > 1:
        target[synth.uniform01(seed + 3, (M,)) < 0.2] = -1
        target[0] = 0                                                   # (at least one live row whatever the draws)
    if M >= 3:
        target[M // 2] = C + 3
    w = synth.uniform(seed + 4, (C,), 0.5, 2.0) if weighted else None
    ref = nll(logp, target, w)
    for a in (logp, target) + (() if w is None else (w,)):
        a.setflags(write=False)
    return logp, target, w, ref
