"""A plain torch restatement of the WHOLE pointnet_2 / pointnet_2_seg network (pointNet/model/pointnetAtt.py), differentiated by torch's
own autograd and parameterised by dtype: float64 is the yardstick of tests/test_pn2_model_parity_gpu.py, float32 measures what a correct
float32 implementation may differ by (tests/test_pn2_model_ref_cpu.py).  Written from the PointNet++ definitions and the docstrings of
pointnet2_utils.py / pointnetAtt.py; it shares no code with the package and uses elementary torch ops only (matmul, index gather, max(dim),
mean, relu, log_softmax, F.nll_loss) -- no nn.BatchNorm*, so batch statistics, biased / unbiased variance and momentum stand written out.
Test infrastructure: no GPU, no library.

Wiring.
  set abstraction `sa1`..`sa3`:  rows [xyz[group] - xyz[centre], features[group]] -> (1x1 conv, BatchNorm, ReLU) per layer -> max over the
      group; sa1's features are all 9 input columns; the next level's coordinates are the centres' own.
  feature propagation `fp3`, `fp2`, `fp1`:  the given 3 neighbours, weights r_k / sum r, r_k = 1 / (d_k^2 + 1e-8) from the coordinates in
      the model's dtype; rows [points1, interpolated] (fp1: interpolated alone) -> (1x1 conv, BatchNorm, ReLU) per layer.
      fp3(l2 <- l3) replaces l2's features, fp2(l1 <- l2) l1's, fp1(l0 <- l1) gives the 128 features per input point.
  head (pointnet_2_seg):  conv1, bn1, ReLU, drop1 (keep mask * 1 / (1 - p)), conv2, log_softmax over the classes.
  pointnet_2:  conv1 (with its bias) on the 128 features and the max over the points.
  BatchNorm in train mode:  mean and BIASED variance of the rows of the call; running_mean' = (1 - m) running_mean + m mean,
      running_var' = (1 - m) running_var + m var M / (M - 1), m = 0.1; num_batches_tracked + 1.  Eval mode: the running statistics, frozen.
  encoder_grad=False:  the three set-abstraction outputs are detached where the decoder takes them.

Discrete choices are INPUTS (`Indices`): per level the centres, the ball-query groups and the 3-NN indices, and the dropout keep mask.
The ReLU signs and the max winners are not: each dtype decides its own, and the bars below absorb the ones that fall the other way.

Error measure (errors()): gradients, running statistics and feature tensors  |got - ref64|_2 / |ref64|_2 per tensor;  log_probs  max abs;
loss  relative.  A `kind` is a state_dict key without its layer number ("sa2.mlp_convs.weight"): a bar covers the layers of a block.

BARS: per (mode, case) and kind the worst error of the float32 restatement against the float64 one over the parameter seeds SEEDS (both
steps in mode T), on identical indices and masks, on one thread, rounded up to three digits.  The bar of the GPU test is GPU_FACTOR x that
value and may not exceed CAP.
Regenerate with:  python tests/pn2_model_ref.py        (prints the table; a quarter of a minute on one CPU core)"""
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

import fp_ref
import sa_ref
import seg_head_train_ref

BN_EPS = float(np.float32(1e-5))              # the values the float32 ABI hands the kernels
MOMENTUM = float(np.float32(0.1))
INTERP_EPS = float(np.float32(1e-8))
HIDDEN, P_DROP, HEAD_SEED, SEED_STRIDE = 128, 0.5, 0x6A09E667, 0x632BE5AB
NUM_CLASSES = 5
CLASS_W = (1.0, 2.0, 2.0, 1.0, 1.0)
NSAMPLE = 32
SEEDS = (8, 9, 11, 13, 14, 15, 17, 19)        # parameter seeds of the measurement (PASSED_OVER: the ones left out); the GPU test runs the first
GPU_FACTOR = 4.0
CAP = 0.05

#        B  N    centres        radii              seed of the input
CASES = {"A": dict(B=2, N=512, npoint=(128, 32, 8), radius=(0.2, 0.4, 0.8), seed=55),      # pn2_finetune_util's reduced model and input
         "B": dict(B=3, N=200, npoint=(48, 12, 3), radius=(0.25, 0.5, 1.0), seed=57)}     # tails: N % 64 != 0, fp3 from 3 points, sa3 padded

#        train-mode BatchNorm in: encoder decoder head    gradient into the encoder    the model
MODES = {"T": dict(train=(True, True, True), encoder_grad=True, seg=True),      # pointnet_2_seg, all five flags, .train()
         "E": dict(train=(False, False, False), encoder_grad=True, seg=True),   # decoder_grad, encoder_grad, eval mode
         "D": dict(train=(False, False, False), encoder_grad=False, seg=True),  # decoder_grad alone
         "G": dict(train=(True, True, False), encoder_grad=True, seg=False)}    # pointnet_2, its four flags, .train()
STEPS = {"T": 2, "E": 1, "D": 1, "G": 1}
ENCODER, DECODER = ("sa1", "sa2", "sa3"), ("fp3", "fp2", "fp1")
TAPS = ("l1_sa2", "l1_fp2", "l2_sa3", "l2_fp3")          # the four consumers at the two fan-in points
FAULTS = ("fp2_skip_detached", "fp3_skip_detached", "fp2_concat_swapped", "biased_running_var", "next_steps_mask", "sa2_not_recentred",
          "ignored_rows_in_denominator")


# ---- the state -------------------------------------------------------------------------------------------------------------------------
def state_shapes(seg=True):
    """The state_dict of pointnet_2_seg(5) (seg) or pointnet_2(5) as {key: shape}, in the modules' order."""
    shapes = {}

    def block(name, cin, widths, tail):
        last = cin
        for l, c in enumerate(widths):
            shapes[f"{name}.mlp_convs.{l}.weight"] = (c, last) + tail
            shapes[f"{name}.mlp_convs.{l}.bias"] = (c,)
            last = c
        for l, c in enumerate(widths):
            bn(f"{name}.mlp_bns.{l}", c)

    def bn(name, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.{k}"] = (c,)
        shapes[f"{name}.num_batches_tracked"] = ()

    block("sa1", 9 + 3, (32, 32, 64), (1, 1))
    block("sa2", 64 + 3, (64, 64, 128), (1, 1))
    block("sa3", 128 + 3, (128, 128, 256), (1, 1))
    block("fp3", 128 + 256, (256, 256), (1,))
    block("fp2", 64 + 256, (256, 128), (1,))
    block("fp1", 128, (128, 128, 128), (1,))
    shapes["conv1.weight"], shapes["conv1.bias"] = (HIDDEN, 128, 1), (HIDDEN,)
    if seg:
        bn("bn1", HIDDEN)
        shapes["conv2.weight"], shapes["conv2.bias"] = (NUM_CLASSES, HIDDEN, 1), (NUM_CLASSES,)
    return shapes


def random_state(seed, seg=True):
    """Seeded values for every key, by the rule of pn2_finetune_util.randomise: num_batches_tracked 3, running_var and the blocks' BatchNorm
    weights in [0.5, 1.5), everything else centred, +-0.3 for vectors and +-1 / sqrt(fan-in) for matrices."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_shapes(seg).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var") or ("mlp_bns" in k and k.endswith("weight")):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        else:
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * (0.6 if len(shape) == 1 else 2.0 / shape[1] ** 0.5)
    return sd


# ---- the seeded inputs and the discrete choices ------------------------------------------------------------------------------------------
def case_inputs(synth, name):
    """-> dict: x [B, N, 9] float32 (xyz and six feature columns), target int64 [B, N] with about 10 % of them -1 and class 4 absent, and for
    pointnet_2's loss r [B, 128, N], q [B, 128]."""
    c = CASES[name]
    B, N, s = c["B"], c["N"], c["seed"]
    x = np.concatenate([synth.clouds(s, B, N), synth.uniform(s + 1, (B, N, 6), -1.0, 1.0)], -1)
    target = synth.randint(s + 10, (B, N), 0, NUM_CLASSES - 1)
    target[synth.uniform01(s + 11, (B, N)) < 0.1] = -1
    assert (target == -1).any() and not (target == NUM_CLASSES - 1).any()
    return dict(x=x, target=target, r=synth.uniform(s + 12, (B, 128, N), -0.5, 0.5), q=synth.uniform(s + 13, (B, 128), -0.5, 0.5))


class Indices:
    """The discrete choices of one input: centres[l] int64 [B, npoint_l], groups[l] int64 [B, npoint_l, nsample] (l = 0, 1, 2 for
    sa1..sa3) and nn3[name] int64 [B, n, k] for fp3, fp2, fp1."""

    def __init__(self, centres, groups, nn3):
        as_long = lambda a: torch.as_tensor(np.asarray(a.cpu() if torch.is_tensor(a) else a)).long()
        self.centres = [as_long(a) for a in centres]
        self.groups = [as_long(a) for a in groups]
        self.nn3 = {k: as_long(a) for k, a in nn3.items()}


def indices_cpu(x, case):
    """Indices from the suite's CPU restatements of the three searches: oracle/fps_oracle.fps_indices_c, sa_ref.ball_query, fp_ref.three_nn."""
    from oracle import fps_oracle
    c = CASES[case]
    levels, centres, groups = [np.ascontiguousarray(x[..., :3])], [], []
    for npoint, radius in zip(c["npoint"], c["radius"]):
        cur = levels[-1]
        cen = np.stack([fps_oracle.fps_indices_c(cloud, npoint) for cloud in cur])
        groups.append(np.stack([sa_ref.ball_query(cloud, ce, radius, NSAMPLE)[0] for cloud, ce in zip(cur, cen)]))
        centres.append(cen)
        levels.append(np.stack([cloud[ce] for cloud, ce in zip(cur, cen)]))
    nn3 = {name: np.stack([fp_ref.three_nn(f, co)[0] for f, co in zip(levels[i], levels[i + 1])]) for name, i in zip(DECODER, (2, 1, 0))}
    return Indices(centres, groups, nn3)


def head_seed(seed, step):
    """PointNetSegHead.next_seed()."""
    return (seed + SEED_STRIDE * step) & 0xFFFFFFFF


def dropout_mask(seed, step, rows, dtype):
    """keep * 1 / (1 - p) of the head's call number `step`, [rows, HIDDEN]."""
    keep = seg_head_train_ref.keep_mask(head_seed(seed, step), rows, HIDDEN, P_DROP)
    return torch.from_numpy(keep.astype(np.float64) * seg_head_train_ref.drop_scale(P_DROP)).to(dtype)


# ---- the network -----------------------------------------------------------------------------------------------------------------------
class Restatement:
    """The network on a state_dict of the package's model: params (tensors of `dtype` that require grad), buffers (running statistics,
    replaced by every train-mode forward) and counts (num_batches_tracked as ints), all under the state_dict's keys."""

    def __init__(self, state, dtype, seg=True):
        self.dtype, self.seg = dtype, seg
        self.params, self.buffers, self.counts = {}, {}, {}
        for k, v in state.items():
            v = v.detach().cpu()
            if k.endswith("num_batches_tracked"):
                self.counts[k] = int(v)
            elif k.endswith(("running_mean", "running_var")):
                self.buffers[k] = v.to(dtype).clone()
            else:
                self.params[k] = v.to(dtype).clone().requires_grad_(True)
        self.faults = ()

    def _bn(self, name, z, train):
        """BatchNorm over the rows z [M, C]."""
        if train:
            M = z.shape[0]
            mean = z.mean(0)
            d = z - mean
            var = (d * d).mean(0)
            with torch.no_grad():
                unbiased = var if "biased_running_var" in self.faults else var * M / (M - 1.0)
                self.buffers[name + ".running_mean"] = (1.0 - MOMENTUM) * self.buffers[name + ".running_mean"] + MOMENTUM * mean
                self.buffers[name + ".running_var"] = (1.0 - MOMENTUM) * self.buffers[name + ".running_var"] + MOMENTUM * unbiased
            self.counts[name + ".num_batches_tracked"] += 1
        else:
            mean, var = self.buffers[name + ".running_mean"], self.buffers[name + ".running_var"]
            d = z - mean
        return d / torch.sqrt(var + BN_EPS) * self.params[name + ".weight"] + self.params[name + ".bias"]

    def _mlp(self, name, rows, train):
        """The shared MLP of a block on rows [M, cin] -> [M, cout_last]."""
        l = 0
        while f"{name}.mlp_convs.{l}.weight" in self.params:
            W = self.params[f"{name}.mlp_convs.{l}.weight"]
            z = rows @ W.reshape(W.shape[0], W.shape[1]).T + self.params[f"{name}.mlp_convs.{l}.bias"]
            rows = torch.relu(self._bn(f"{name}.mlp_bns.{l}", z, train))
            l += 1
        return rows

    def set_abstraction(self, name, xyz, feats, centres, group, train):
        """xyz [B, n, 3], feats [B, n, D], centres [B, s], group [B, s, nsample] -> (new_xyz [B, s, 3], new_points [B, s, cout])."""
        B, s, nsample = group.shape
        b1, b2 = torch.arange(B)[:, None], torch.arange(B)[:, None, None]
        new_xyz = xyz[b1, centres]
        rel = xyz[b2, group]
        if not (name == "sa2" and "sa2_not_recentred" in self.faults):
            rel = rel - new_xyz[:, :, None, :]
        rows = torch.cat([rel, feats[b2, group]], -1)
        out = self._mlp(name, rows.reshape(B * s * nsample, -1), train)
        return new_xyz, out.reshape(B, s, nsample, -1).max(2).values

    def feature_propagation(self, name, xyz1, xyz2, points1, points2, nn3, train):
        """xyz1 [B, n, 3] fine, xyz2 [B, s, 3] coarse, points1 [B, n, D1] or None, points2 [B, s, D2], nn3 [B, n, k] -> [B, n, cout]."""
        B, n, _ = nn3.shape
        b2 = torch.arange(B)[:, None, None]
        d = xyz1[:, :, None, :] - xyz2[b2, nn3]
        sq = d * d
        recip = 1.0 / (((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + INTERP_EPS)
        w = recip / recip.sum(-1, keepdim=True)
        interpolated = (w[..., None] * points2[b2, nn3]).sum(2)
        if points1 is None:
            rows = interpolated
        elif name == "fp2" and "fp2_concat_swapped" in self.faults:
            rows = torch.cat([interpolated, points1], -1)
        else:
            rows = torch.cat([points1, interpolated], -1)
        return self._mlp(name, rows.reshape(B * n, -1), train).reshape(B, n, -1)

    def forward(self, x, idx, train=(False, False, False), encoder_grad=True, mask=None):
        """x [B, N, 9] of self.dtype -> log_probs [B, N, classes] (seg) or (global feature [B, 128], l0_points [B, 128, N]).
        train: BatchNorm (and dropout) in train mode in the encoder, the decoder, the head; mask: dropout_mask() for a train-mode head.
        self.taps: the four tensors the fan-in consumers take (copies of l1_points / l2_points, for torch.autograd.grad)."""
        train_enc, train_dec, train_head = train
        l0_xyz = x[..., :3]
        l1_xyz, l1 = self.set_abstraction("sa1", l0_xyz, x, idx.centres[0], idx.groups[0], train_enc)
        l1_sa2, l1_fp2 = l1.clone(), l1.clone()
        l2_xyz, l2 = self.set_abstraction("sa2", l1_xyz, l1_sa2, idx.centres[1], idx.groups[1], train_enc)
        l2_sa3, l2_fp3 = l2.clone(), l2.clone()
        l3_xyz, l3 = self.set_abstraction("sa3", l2_xyz, l2_sa3, idx.centres[2], idx.groups[2], train_enc)
        self.taps = dict(l1_sa2=l1_sa2, l1_fp2=l1_fp2, l2_sa3=l2_sa3, l2_fp3=l2_fp3)
        if not encoder_grad:
            l1_fp2, l2_fp3, l3 = l1_fp2.detach(), l2_fp3.detach(), l3.detach()
        if "fp3_skip_detached" in self.faults:
            l2_fp3 = l2_fp3.detach()
        if "fp2_skip_detached" in self.faults:
            l1_fp2 = l1_fp2.detach()
        l2_new = self.feature_propagation("fp3", l2_xyz, l3_xyz, l2_fp3, l3, idx.nn3["fp3"], train_dec)
        l1_new = self.feature_propagation("fp2", l1_xyz, l2_xyz, l1_fp2, l2_new, idx.nn3["fp2"], train_dec)
        l0 = self.feature_propagation("fp1", l0_xyz, l1_xyz, None, l1_new, idx.nn3["fp1"], train_dec)
        B, N, _ = l0.shape
        self.trace = dict(xyz=(l0_xyz, l1_xyz, l2_xyz, l3_xyz), l1=l1, l2=l2, l3=l3, l2_new=l2_new, l1_new=l1_new, l0=l0)
        if not self.seg:
            return self._conv1(l0.reshape(B * N, -1)).reshape(B, N, -1).max(1).values, l0.transpose(1, 2)
        return self.head(l0.reshape(B * N, -1), train_head, mask).reshape(B, N, -1)

    def _conv1(self, rows):
        W1 = self.params["conv1.weight"]
        return rows @ W1.reshape(W1.shape[0], W1.shape[1]).T + self.params["conv1.bias"]

    def head(self, rows, train, mask=None):
        """The per-point classifier on rows [M, 128] -> log-probabilities [M, classes]; mask [M, HIDDEN] in train mode."""
        h = torch.relu(self._bn("bn1", self._conv1(rows), train))
        if train:
            h = h * mask
        W2 = self.params["conv2.weight"]
        logits = h @ W2.reshape(W2.shape[0], W2.shape[1]).T + self.params["conv2.bias"]
        return torch.log_softmax(logits, -1)

    def loss(self, log_probs, target):
        """The weighted NLL over the rows whose target is not -1."""
        C = log_probs.shape[-1]
        w = torch.tensor(CLASS_W, dtype=self.dtype)
        lp, t = log_probs.reshape(-1, C), torch.as_tensor(target).reshape(-1)
        if "ignored_rows_in_denominator" in self.faults:
            live = t >= 0
            return F.nll_loss(lp, t, weight=w, ignore_index=-1, reduction="sum") / (w[t[live]].sum() + (~live).sum())
        return F.nll_loss(lp, t, weight=w, ignore_index=-1)


def run(state, inputs, idx, mode, dtype, faults=(), head_seed0=HEAD_SEED, first_step=0):
    """STEPS[mode] forward + backward passes of `mode` on one state, the way the GPU test drives the package: no optimiser between the steps,
    the running statistics carried on, the head's dropout step advancing.  -> a list with one dict per step:
      out      log_probs and loss (seg) or l0_points and glob (pointnet_2);
      grads    {key: gradient or None}; buffers {key: running statistic}; counts {key: num_batches_tracked};
      taps     {TAPS name: the gradient that consumer alone sends back} (encoder_grad modes)."""
    m = MODES[mode]
    net = Restatement(state, dtype, seg=m["seg"])
    net.faults = tuple(faults)
    x = torch.from_numpy(inputs["x"]).to(dtype)
    results = []
    for step in range(first_step, first_step + STEPS[mode]):
        mask = None
        if m["train"][2]:
            mask = dropout_mask(head_seed0, step + (1 if "next_steps_mask" in faults else 0), x.shape[0] * x.shape[1], dtype)
        if m["seg"]:
            log_probs = net.forward(x, idx, m["train"], m["encoder_grad"], mask)
            loss = net.loss(log_probs, inputs["target"])
            out = dict(log_probs=log_probs.detach(), loss=loss.detach())
        else:
            glob, l0 = net.forward(x, idx, m["train"], m["encoder_grad"])
            loss = (l0 * torch.from_numpy(inputs["r"]).to(dtype)).sum() + (glob * torch.from_numpy(inputs["q"]).to(dtype)).sum()
            out = dict(l0_points=l0.detach(), glob=glob.detach())
        keys = list(net.params)
        taps = list(TAPS) if m["encoder_grad"] else []
        g = torch.autograd.grad(loss, [net.params[k] for k in keys] + [net.taps[k] for k in taps], allow_unused=True)
        results.append(dict(out=out, grads=dict(zip(keys, g[:len(keys)])), taps=dict(zip(taps, g[len(keys):])),
                            buffers=dict(net.buffers), counts=dict(net.counts)))
    return results


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------
def kind(key):
    """A state_dict key without its layer number."""
    return re.sub(r"\.\d+\.", ".", key)


def zero_by_construction(key, mode):
    """A conv bias in front of a batch-statistics BatchNorm: its true gradient is zero."""
    enc, dec, head = MODES[mode]["train"]
    if "mlp_convs" in key and key.endswith(".bias"):
        return enc if key.startswith(ENCODER) else dec
    return key == "conv1.bias" and head


def trains(key, mode):
    """Whether the BatchNorm that owns `key` is in train mode."""
    enc, dec, head = MODES[mode]["train"]
    return enc if key.startswith(ENCODER) else dec if key.startswith(DECODER) else head


def rel_l2(got, ref):
    """|got - ref|_2 / |ref|_2; a missing gradient (None) counts as zeros."""
    got = torch.zeros_like(ref) if got is None else got
    got, ref = (torch.as_tensor(t).detach().cpu().double() for t in (got, ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / ref.norm())


def errors(got, ref, mode):
    """One step's results (run()'s dict; `got` may hold GPU float32 tensors) against the float64 ones -> {kind: the worst error}.
    Gradients that are zero by construction or None on both sides are left to the caller."""
    e = {}

    def put(k, v):
        e[k] = max(e.get(k, 0.0), v)

    for k, r in ref["out"].items():
        g = torch.as_tensor(got["out"][k]).detach().cpu().double()
        if k == "log_probs":
            put(k, float((g - r.double()).abs().max()))
        elif k == "loss":
            put(k, abs(float(g) - float(r)) / abs(float(r)))
        else:
            put(k, rel_l2(g, r))
    for k, r in ref["grads"].items():
        if r is None or zero_by_construction(k, mode):
            continue
        put("grad." + kind(k), rel_l2(got["grads"][k], r))
    for k, r in ref["buffers"].items():
        if trains(k, mode):                                          # (frozen statistics: bit-unchanged, the caller's torch.equal)
            put(kind(k), rel_l2(got["buffers"][k], r))
    for k, r in ref["taps"].items():
        if k in got["taps"]:                                         # (the GPU test takes them in a test of their own)
            put("tap." + k, rel_l2(got["taps"][k], r))
    return e


def measure(synth, mode, case, seeds, faults=(), ref64=None):
    """The float32 restatement (with `faults`) against the float64 one (without) on identical indices and masks
    -> {kind: worst error over the seeds and the steps}."""
    inputs = case_inputs(synth, case)
    idx = indices_cpu(inputs["x"], case)
    worst = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # float32 sums depend on how a product is split over threads: the table is one thread's
    try:
        for seed in seeds:
            state = random_state(seed, MODES[mode]["seg"])
            want = ref64[seed] if ref64 is not None else run(state, inputs, idx, mode, torch.float64)
            for g, r in zip(run(state, inputs, idx, mode, torch.float32, faults), want):
                for k, v in errors(g, r, mode).items():
                    worst[k] = max(worst.get(k, 0.0), v)
    finally:
        torch.set_num_threads(threads)
    return worst


def round_up(v):
    """v rounded UP to three significant digits, as the table holds it."""
    if v == 0.0:
        return 0.0
    e = int(np.floor(np.log10(v)))
    return float(f"{np.ceil(v / 10.0 ** e * 100.0 - 1e-9) / 100.0:.2f}e{e}")


def bar(mode, case, k):
    """The GPU test's bar of kind k."""
    return GPU_FACTOR * BARS[(mode, case)][k]


def ratios(err, mode, case):
    """{kind: error / bar}; an exact result is inside any bar."""
    return {k: 0.0 if v == 0.0 else v / bar(mode, case, k) if bar(mode, case, k) else float("inf") for k, v in err.items()}


def summary(rat):
    """One line: the worst error / bar per block and tensor kind."""
    return "  ".join(f"{k} {v:.2g}" for k, v in sorted(rat.items()))


# Seeds of 8..23 left out of SEEDS, with the worst float32 error of a gradient tensor that excluded them.  One ReLU decision that falls the
# other way near the loss moves EVERY gradient tensor behind it by about 1 / sqrt(active elements), 3e-3 .. 4e-2 here, while a run without one
# stays below 1e-5: the distribution is bimodal, and whether a state has a ReLU input within rounding of zero is a property of the state, so
# it holds for every float32 implementation.  A seed whose float32 restatement alone exceeds CAP / GPU_FACTOR = 1.25e-2 in some mode and
# case cannot give a bar inside the cap and is passed over.
PASSED_OVER = {10: ("T B", 1.72e-2), 12: ("G A", 2.58e-2), 16: ("T B", 4.25e-2), 18: ("T B", 1.40e-2), 20: ("T A", 1.37e-2), 22: ("G B", 1.44e-2)}

BARS = {
    ('T', 'A'): {
        'log_probs': 5.29e-06, 'loss': 1.24e-07, 'grad.sa1.mlp_convs.weight': 6.04e-03, 'grad.sa1.mlp_bns.weight': 7.68e-03,
        'grad.sa1.mlp_bns.bias': 8.48e-03, 'grad.sa2.mlp_convs.weight': 6.55e-03, 'grad.sa2.mlp_bns.weight': 6.51e-03,
        'grad.sa2.mlp_bns.bias': 6.73e-03, 'grad.sa3.mlp_convs.weight': 6.04e-03, 'grad.sa3.mlp_bns.weight': 6.54e-03,
        'grad.sa3.mlp_bns.bias': 7.14e-03, 'grad.fp3.mlp_convs.weight': 6.04e-03, 'grad.fp3.mlp_bns.weight': 5.60e-03,
        'grad.fp3.mlp_bns.bias': 5.93e-03, 'grad.fp2.mlp_convs.weight': 5.60e-03, 'grad.fp2.mlp_bns.weight': 4.00e-03,
        'grad.fp2.mlp_bns.bias': 5.51e-03, 'grad.fp1.mlp_convs.weight': 3.88e-03, 'grad.fp1.mlp_bns.weight': 2.85e-03,
        'grad.fp1.mlp_bns.bias': 4.95e-03, 'grad.conv1.weight': 7.56e-06, 'grad.bn1.weight': 2.87e-06, 'grad.bn1.bias': 1.05e-07,
        'grad.conv2.weight': 1.04e-06, 'grad.conv2.bias': 8.95e-08, 'sa1.mlp_bns.running_mean': 9.68e-08,
        'sa1.mlp_bns.running_var': 8.86e-08, 'sa2.mlp_bns.running_mean': 8.93e-08, 'sa2.mlp_bns.running_var': 8.96e-08,
        'sa3.mlp_bns.running_mean': 1.49e-07, 'sa3.mlp_bns.running_var': 8.84e-08, 'fp3.mlp_bns.running_mean': 3.85e-07,
        'fp3.mlp_bns.running_var': 8.92e-08, 'fp2.mlp_bns.running_mean': 1.17e-07, 'fp2.mlp_bns.running_var': 8.99e-08,
        'fp1.mlp_bns.running_mean': 1.44e-07, 'fp1.mlp_bns.running_var': 9.02e-08, 'bn1.running_mean': 1.20e-07,
        'bn1.running_var': 8.96e-08, 'tap.l1_sa2': 5.99e-03, 'tap.l1_fp2': 6.41e-03, 'tap.l2_sa3': 6.29e-03, 'tap.l2_fp3': 6.09e-03,
    },
    ('T', 'B'): {
        'log_probs': 4.72e-06, 'loss': 1.39e-07, 'grad.sa1.mlp_convs.weight': 1.11e-03, 'grad.sa1.mlp_bns.weight': 1.19e-03,
        'grad.sa1.mlp_bns.bias': 1.52e-03, 'grad.sa2.mlp_convs.weight': 1.11e-03, 'grad.sa2.mlp_bns.weight': 1.02e-03,
        'grad.sa2.mlp_bns.bias': 1.04e-03, 'grad.sa3.mlp_convs.weight': 1.02e-03, 'grad.sa3.mlp_bns.weight': 1.05e-03,
        'grad.sa3.mlp_bns.bias': 1.16e-03, 'grad.fp3.mlp_convs.weight': 9.25e-04, 'grad.fp3.mlp_bns.weight': 1.01e-03,
        'grad.fp3.mlp_bns.bias': 1.05e-03, 'grad.fp2.mlp_convs.weight': 1.02e-03, 'grad.fp2.mlp_bns.weight': 9.51e-04,
        'grad.fp2.mlp_bns.bias': 1.02e-03, 'grad.fp1.mlp_convs.weight': 1.25e-03, 'grad.fp1.mlp_bns.weight': 1.87e-03,
        'grad.fp1.mlp_bns.bias': 1.21e-03, 'grad.conv1.weight': 1.09e-03, 'grad.bn1.weight': 9.73e-03, 'grad.bn1.bias': 2.60e-03,
        'grad.conv2.weight': 1.63e-06, 'grad.conv2.bias': 9.42e-08, 'sa1.mlp_bns.running_mean': 1.05e-07,
        'sa1.mlp_bns.running_var': 9.02e-08, 'sa2.mlp_bns.running_mean': 1.15e-07, 'sa2.mlp_bns.running_var': 8.70e-08,
        'sa3.mlp_bns.running_mean': 1.98e-07, 'sa3.mlp_bns.running_var': 9.59e-08, 'fp3.mlp_bns.running_mean': 7.05e-07,
        'fp3.mlp_bns.running_var': 1.08e-07, 'fp2.mlp_bns.running_mean': 1.46e-07, 'fp2.mlp_bns.running_var': 8.99e-08,
        'fp1.mlp_bns.running_mean': 1.50e-07, 'fp1.mlp_bns.running_var': 9.64e-08, 'bn1.running_mean': 1.49e-07,
        'bn1.running_var': 8.80e-08, 'tap.l1_sa2': 9.99e-04, 'tap.l1_fp2': 9.11e-04, 'tap.l2_sa3': 1.04e-03, 'tap.l2_fp3': 1.06e-03,
    },
    ('E', 'A'): {
        'log_probs': 2.31e-07, 'loss': 1.28e-07, 'grad.sa1.mlp_convs.weight': 3.02e-07, 'grad.sa1.mlp_convs.bias': 2.52e-07,
        'grad.sa1.mlp_bns.weight': 3.02e-07, 'grad.sa1.mlp_bns.bias': 2.38e-07, 'grad.sa2.mlp_convs.weight': 2.72e-07,
        'grad.sa2.mlp_convs.bias': 2.61e-07, 'grad.sa2.mlp_bns.weight': 3.31e-07, 'grad.sa2.mlp_bns.bias': 2.59e-07,
        'grad.sa3.mlp_convs.weight': 3.00e-07, 'grad.sa3.mlp_convs.bias': 2.70e-07, 'grad.sa3.mlp_bns.weight': 3.06e-07,
        'grad.sa3.mlp_bns.bias': 2.73e-07, 'grad.fp3.mlp_convs.weight': 2.55e-07, 'grad.fp3.mlp_convs.bias': 2.34e-07,
        'grad.fp3.mlp_bns.weight': 2.27e-07, 'grad.fp3.mlp_bns.bias': 2.28e-07, 'grad.fp2.mlp_convs.weight': 3.26e-07,
        'grad.fp2.mlp_convs.bias': 2.22e-07, 'grad.fp2.mlp_bns.weight': 2.67e-07, 'grad.fp2.mlp_bns.bias': 2.07e-07,
        'grad.fp1.mlp_convs.weight': 2.42e-07, 'grad.fp1.mlp_convs.bias': 1.80e-07, 'grad.fp1.mlp_bns.weight': 1.92e-07,
        'grad.fp1.mlp_bns.bias': 1.60e-07, 'grad.conv1.weight': 1.88e-07, 'grad.conv1.bias': 9.19e-08, 'grad.bn1.weight': 1.14e-07,
        'grad.bn1.bias': 7.80e-08, 'grad.conv2.weight': 2.07e-07, 'grad.conv2.bias': 1.01e-07, 'tap.l1_sa2': 4.81e-07,
        'tap.l1_fp2': 4.31e-07, 'tap.l2_sa3': 3.99e-07, 'tap.l2_fp3': 4.42e-07,
    },
    ('E', 'B'): {
        'log_probs': 2.46e-07, 'loss': 5.08e-08, 'grad.sa1.mlp_convs.weight': 3.84e-07, 'grad.sa1.mlp_convs.bias': 3.59e-07,
        'grad.sa1.mlp_bns.weight': 4.61e-07, 'grad.sa1.mlp_bns.bias': 2.86e-07, 'grad.sa2.mlp_convs.weight': 3.36e-07,
        'grad.sa2.mlp_convs.bias': 3.23e-07, 'grad.sa2.mlp_bns.weight': 3.35e-07, 'grad.sa2.mlp_bns.bias': 3.38e-07,
        'grad.sa3.mlp_convs.weight': 3.46e-07, 'grad.sa3.mlp_convs.bias': 3.39e-07, 'grad.sa3.mlp_bns.weight': 3.76e-07,
        'grad.sa3.mlp_bns.bias': 3.12e-07, 'grad.fp3.mlp_convs.weight': 2.64e-07, 'grad.fp3.mlp_convs.bias': 2.33e-07,
        'grad.fp3.mlp_bns.weight': 2.39e-07, 'grad.fp3.mlp_bns.bias': 2.38e-07, 'grad.fp2.mlp_convs.weight': 2.97e-07,
        'grad.fp2.mlp_convs.bias': 2.37e-07, 'grad.fp2.mlp_bns.weight': 2.08e-07, 'grad.fp2.mlp_bns.bias': 2.20e-07,
        'grad.fp1.mlp_convs.weight': 2.81e-07, 'grad.fp1.mlp_convs.bias': 2.00e-07, 'grad.fp1.mlp_bns.weight': 2.17e-07,
        'grad.fp1.mlp_bns.bias': 2.20e-07, 'grad.conv1.weight': 2.01e-07, 'grad.conv1.bias': 6.97e-08, 'grad.bn1.weight': 8.62e-08,
        'grad.bn1.bias': 7.28e-08, 'grad.conv2.weight': 2.21e-07, 'grad.conv2.bias': 7.38e-08, 'tap.l1_sa2': 5.30e-07,
        'tap.l1_fp2': 4.17e-07, 'tap.l2_sa3': 4.31e-07, 'tap.l2_fp3': 4.21e-07,
    },
    ('D', 'A'): {
        'log_probs': 2.31e-07, 'loss': 1.28e-07, 'grad.fp3.mlp_convs.weight': 2.55e-07, 'grad.fp3.mlp_convs.bias': 2.34e-07,
        'grad.fp3.mlp_bns.weight': 2.27e-07, 'grad.fp3.mlp_bns.bias': 2.28e-07, 'grad.fp2.mlp_convs.weight': 3.26e-07,
        'grad.fp2.mlp_convs.bias': 2.22e-07, 'grad.fp2.mlp_bns.weight': 2.67e-07, 'grad.fp2.mlp_bns.bias': 2.07e-07,
        'grad.fp1.mlp_convs.weight': 2.42e-07, 'grad.fp1.mlp_convs.bias': 1.80e-07, 'grad.fp1.mlp_bns.weight': 1.92e-07,
        'grad.fp1.mlp_bns.bias': 1.60e-07, 'grad.conv1.weight': 1.88e-07, 'grad.conv1.bias': 9.19e-08, 'grad.bn1.weight': 1.14e-07,
        'grad.bn1.bias': 7.80e-08, 'grad.conv2.weight': 2.07e-07, 'grad.conv2.bias': 1.01e-07,
    },
    ('D', 'B'): {
        'log_probs': 2.46e-07, 'loss': 5.08e-08, 'grad.fp3.mlp_convs.weight': 2.64e-07, 'grad.fp3.mlp_convs.bias': 2.33e-07,
        'grad.fp3.mlp_bns.weight': 2.39e-07, 'grad.fp3.mlp_bns.bias': 2.38e-07, 'grad.fp2.mlp_convs.weight': 2.97e-07,
        'grad.fp2.mlp_convs.bias': 2.37e-07, 'grad.fp2.mlp_bns.weight': 2.08e-07, 'grad.fp2.mlp_bns.bias': 2.20e-07,
        'grad.fp1.mlp_convs.weight': 2.81e-07, 'grad.fp1.mlp_convs.bias': 2.00e-07, 'grad.fp1.mlp_bns.weight': 2.17e-07,
        'grad.fp1.mlp_bns.bias': 2.20e-07, 'grad.conv1.weight': 2.01e-07, 'grad.conv1.bias': 6.97e-08, 'grad.bn1.weight': 8.62e-08,
        'grad.bn1.bias': 7.28e-08, 'grad.conv2.weight': 2.21e-07, 'grad.conv2.bias': 7.38e-08,
    },
    ('G', 'A'): {
        'l0_points': 5.73e-06, 'glob': 2.83e-06, 'grad.sa1.mlp_convs.weight': 5.00e-03, 'grad.sa1.mlp_bns.weight': 5.50e-03,
        'grad.sa1.mlp_bns.bias': 5.65e-03, 'grad.sa2.mlp_convs.weight': 5.11e-03, 'grad.sa2.mlp_bns.weight': 5.01e-03,
        'grad.sa2.mlp_bns.bias': 5.72e-03, 'grad.sa3.mlp_convs.weight': 4.69e-03, 'grad.sa3.mlp_bns.weight': 5.12e-03,
        'grad.sa3.mlp_bns.bias': 5.45e-03, 'grad.fp3.mlp_convs.weight': 4.78e-03, 'grad.fp3.mlp_bns.weight': 4.28e-03,
        'grad.fp3.mlp_bns.bias': 4.82e-03, 'grad.fp2.mlp_convs.weight': 4.19e-03, 'grad.fp2.mlp_bns.weight': 3.71e-03,
        'grad.fp2.mlp_bns.bias': 6.99e-03, 'grad.fp1.mlp_convs.weight': 3.46e-03, 'grad.fp1.mlp_bns.weight': 2.30e-03,
        'grad.fp1.mlp_bns.bias': 6.71e-03, 'grad.conv1.weight': 5.29e-06, 'grad.conv1.bias': 0.00e+00, 'sa1.mlp_bns.running_mean': 5.92e-08,
        'sa1.mlp_bns.running_var': 5.35e-08, 'sa2.mlp_bns.running_mean': 5.67e-08, 'sa2.mlp_bns.running_var': 4.86e-08,
        'sa3.mlp_bns.running_mean': 9.09e-08, 'sa3.mlp_bns.running_var': 4.90e-08, 'fp3.mlp_bns.running_mean': 2.42e-07,
        'fp3.mlp_bns.running_var': 4.93e-08, 'fp2.mlp_bns.running_mean': 6.64e-08, 'fp2.mlp_bns.running_var': 4.73e-08,
        'fp1.mlp_bns.running_mean': 7.37e-08, 'fp1.mlp_bns.running_var': 5.30e-08, 'tap.l1_sa2': 4.58e-03, 'tap.l1_fp2': 5.23e-03,
        'tap.l2_sa3': 4.96e-03, 'tap.l2_fp3': 4.12e-03,
    },
    ('G', 'B'): {
        'l0_points': 5.93e-06, 'glob': 3.42e-06, 'grad.sa1.mlp_convs.weight': 1.13e-03, 'grad.sa1.mlp_bns.weight': 1.08e-03,
        'grad.sa1.mlp_bns.bias': 1.16e-03, 'grad.sa2.mlp_convs.weight': 1.11e-03, 'grad.sa2.mlp_bns.weight': 1.34e-03,
        'grad.sa2.mlp_bns.bias': 1.04e-03, 'grad.sa3.mlp_convs.weight': 1.18e-03, 'grad.sa3.mlp_bns.weight': 1.12e-03,
        'grad.sa3.mlp_bns.bias': 1.24e-03, 'grad.fp3.mlp_convs.weight': 1.08e-03, 'grad.fp3.mlp_bns.weight': 1.07e-03,
        'grad.fp3.mlp_bns.bias': 1.11e-03, 'grad.fp2.mlp_convs.weight': 1.03e-03, 'grad.fp2.mlp_bns.weight': 9.96e-04,
        'grad.fp2.mlp_bns.bias': 1.20e-03, 'grad.fp1.mlp_convs.weight': 1.16e-03, 'grad.fp1.mlp_bns.weight': 1.05e-03,
        'grad.fp1.mlp_bns.bias': 2.26e-03, 'grad.conv1.weight': 5.21e-06, 'grad.conv1.bias': 2.34e-08, 'sa1.mlp_bns.running_mean': 6.15e-08,
        'sa1.mlp_bns.running_var': 5.46e-08, 'sa2.mlp_bns.running_mean': 6.85e-08, 'sa2.mlp_bns.running_var': 4.73e-08,
        'sa3.mlp_bns.running_mean': 1.16e-07, 'sa3.mlp_bns.running_var': 5.33e-08, 'fp3.mlp_bns.running_mean': 4.45e-07,
        'fp3.mlp_bns.running_var': 5.70e-08, 'fp2.mlp_bns.running_mean': 8.19e-08, 'fp2.mlp_bns.running_var': 5.01e-08,
        'fp1.mlp_bns.running_mean': 8.35e-08, 'fp1.mlp_bns.running_var': 5.25e-08, 'tap.l1_sa2': 1.05e-03, 'tap.l1_fp2': 9.43e-04,
        'tap.l2_sa3': 1.10e-03, 'tap.l2_fp3': 1.09e-03,
    },
}


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    from conftest import sub
    print("BARS = {")
    for mode_ in MODES:
        for case_ in CASES:
            w = measure(sub("synthetic"), mode_, case_, SEEDS)
            print(f"    ({mode_!r}, {case_!r}): {{")
            line = "       "
            for k_, v_ in w.items():
                item = f" {k_!r}: {round_up(v_):.2e},"
                if len(line) + len(item) > 140:
                    print(line)
                    line = "       "
                line += item
            print(line + "\n    },")
    print("}")
