"""The ragged wiring of pointnet_2_seg (forward_ragged on clouds of UNEQUAL size packed back to back) on top of the plain torch restatement
tests/pn2_model_ref.py, which is imported and not edited: its Restatement's blocks, head, loss and error measure, in float64 (the yardstick
of tests/test_pn2_ragged_train_gpu.py) and float32 (what a correct float32 implementation may differ by, tests/test_pn2_ragged_ref_cpu.py).
Test infrastructure: no GPU, no library.

Wiring.
  sa1 and fp1 run on the packed array [1, total, .] as ONE cloud with GLOBAL centres, groups and 3-NN indices (a row of the packed array;
      for fp1 the coarse point b * npoint + j of the Q * npoint centres of all clouds);
  the middle of the network -- sa2, sa3, fp3, fp2 -- runs on [Q, npoint, .], every cloud having sa1's npoint centres;
  BatchNorm in train mode runs over ALL rows of the call (Restatement._bn on the flattened rows: Q * npoint * nsample for sa1, total for
      fp1 and the head), the dropout mask covers `total` rows, and the loss is the weighted NLL over the rows whose target is not -1.
The discrete choices are inputs (pn2_model_ref.Indices): indices_cpu_ragged takes them from the suite's CPU restatements cloud by cloud
(fps_oracle, sa_ref.ball_query, fp_ref.three_nn) plus the offsets; the GPU test hands over the package's own.

BARS: per mode and kind the worst error of the float32 restatement against the float64 one over the parameter seeds SEEDS (both steps in
mode T) on identical indices and masks, on one thread, rounded up to three digits; the GPU test's bar is pn2_model_ref.GPU_FACTOR (4) x
that and may not exceed pn2_model_ref.CAP (0.05).  A seed at which float32 alone exceeds CAP / GPU_FACTOR = 0.0125 in some mode cannot give
a bar inside the cap and is passed over (PASSED_OVER, with its figure): pn2_model_ref's docstring says why the distribution is bimodal.
FAULT_FACTORS: the two planted wiring faults, each as the largest error / bar over the kinds (test_pn2_ragged_ref_cpu.py recomputes them).
Regenerate with:  python tests/pn2_ragged_ref.py        (prints SEEDS, PASSED_OVER, BARS and FAULT_FACTORS)"""
import os
import sys

import numpy as np
import torch

import fp_ref
import pn2_model_ref as R
import sa_ref

SIZES = (128, 129, 200, 200, 511)             # npoint itself, one more, two equal clouds, no multiple of a 32-row tile
NPOINT, RADIUS = (128, 32, 8), (0.2, 0.4, 0.8)                 # pn2_finetune_util's reduced model
INPUT_SEED = 61
MODE_NAMES = ("T", "E", "D")                  # pn2_model_ref.MODES: all five flags in train mode, two steps; eval with both grads; decoder alone
CANDIDATES = tuple(range(8, 24))
FAULTS = ("sa1_local_indices", "bn_per_cloud")


def case_inputs(synth):
    """-> dict: x [total, 9] float32 (the clouds back to back: xyz and six feature columns), target int64 [total] with about 10 % of them
    -1 and class 4 absent."""
    total = sum(SIZES)
    xyz = np.concatenate([synth.clouds(INPUT_SEED + b, 1, n)[0] for b, n in enumerate(SIZES)])
    x = np.concatenate([xyz, synth.uniform(INPUT_SEED + 20, (total, 6), -1.0, 1.0)], -1).astype(np.float32)
    target = synth.randint(INPUT_SEED + 30, (total,), 0, R.NUM_CLASSES - 1)
    target[synth.uniform01(INPUT_SEED + 31, (total,)) < 0.1] = -1
    assert (target == -1).any() and not (target == R.NUM_CLASSES - 1).any()
    return dict(x=x, target=target)


def pack_indices(centres, groups, nn3, sizes=SIZES):
    """The choices of every cloud ALONE -- centres[l] [Q, npoint_l] and groups[l] [Q, npoint_l, nsample] relative to the level's cloud, nn3
    as pn2_model_ref.Indices with nn3['fp1'] a list of [n_b, 3] -- as the ragged wiring takes them: level 0 global and as one cloud."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Q, S = len(sizes), np.asarray(centres[0]).shape[1]
    c0 = (np.asarray(centres[0]) + off[:-1, None]).reshape(1, Q * S)
    g0 = (np.asarray(groups[0]) + off[:-1, None, None]).reshape(1, Q * S, -1)
    fp1 = np.concatenate([np.asarray(a) + b * S for b, a in enumerate(nn3["fp1"])])[None]
    return R.Indices([c0, centres[1], centres[2]], [g0, groups[1], groups[2]], dict(fp3=nn3["fp3"], fp2=nn3["fp2"], fp1=fp1))


def choices_cpu(x, sizes=SIZES):
    """(centres, groups, nn3) of every cloud alone, from the suite's CPU restatements of the three searches."""
    from oracle import fps_oracle
    off = np.concatenate([[0], np.cumsum(sizes)])
    clouds = [np.ascontiguousarray(x[off[b]:off[b + 1], :3]) for b in range(len(sizes))]
    levels, centres, groups = [clouds], [], []
    for npoint, radius in zip(NPOINT, RADIUS):
        cen = [fps_oracle.fps_indices_c(c, npoint) for c in levels[-1]]
        groups.append(np.stack([sa_ref.ball_query(c, ce, radius, R.NSAMPLE)[0] for c, ce in zip(levels[-1], cen)]))
        centres.append(np.stack(cen))
        levels.append([c[ce] for c, ce in zip(levels[-1], cen)])
    nn3 = {name: [fp_ref.three_nn(f, co)[0] for f, co in zip(levels[i], levels[i + 1])] for name, i in zip(R.DECODER, (2, 1, 0))}
    nn3["fp3"], nn3["fp2"] = np.stack(nn3["fp3"]), np.stack(nn3["fp2"])
    return centres, groups, nn3


def indices_cpu_ragged(x, sizes=SIZES, sa1_local=False):
    """pn2_model_ref.Indices of the ragged wiring.  sa1_local (the planted fault): sa1's centres and groups stay relative to their cloud,
    so every cloud after the first reads rows of the first."""
    centres, groups, nn3 = choices_cpu(x, sizes)
    idx = pack_indices(centres, groups, nn3, sizes)
    if sa1_local:
        Q, S = len(sizes), centres[0].shape[1]
        idx.centres[0] = torch.from_numpy(np.asarray(centres[0]).reshape(1, Q * S)).long()
        idx.groups[0] = torch.from_numpy(np.asarray(groups[0]).reshape(1, Q * S, -1)).long()
    return idx


class RaggedRestatement(R.Restatement):
    """pn2_model_ref.Restatement with forward() wired for packed clouds.  per_cloud (the planted fault "bn_per_cloud"): every train-mode
    BatchNorm of sa1, fp1 and the head takes its statistics cloud by cloud -- what running forward_rows once per cloud would do."""

    def __init__(self, state, dtype, sizes=SIZES, per_cloud=False):
        super().__init__(state, dtype, seg=True)
        self.sizes, self.per_cloud, self._segments = tuple(sizes), per_cloud, None

    def _bn(self, name, z, train):
        if not (train and self.per_cloud and self._segments is not None):
            return super()._bn(name, z, train)
        parts = []
        for rows in torch.split(z, self._segments):                 # (the running statistics end as the last cloud left them)
            parts.append(super()._bn(name, rows, train))
            self.counts[name + ".num_batches_tracked"] -= 1
        self.counts[name + ".num_batches_tracked"] += 1
        return torch.cat(parts)

    def forward(self, x, idx, train=(False, False, False), encoder_grad=True, mask=None):
        """x [total, 9] of self.dtype -> log_probs [total, classes]."""
        train_enc, train_dec, train_head = train
        Q = len(self.sizes)
        S = idx.centres[0].shape[1] // Q
        nsample = idx.groups[0].shape[2]
        packed = x[None]
        l0_xyz = packed[..., :3]
        self._segments = [S * nsample] * Q
        l1_xyz, l1 = self.set_abstraction("sa1", l0_xyz, packed, idx.centres[0], idx.groups[0], train_enc)
        self._segments = None
        l1_xyz, l1 = l1_xyz.reshape(Q, S, 3), l1.reshape(Q, S, -1)
        l2_xyz, l2 = self.set_abstraction("sa2", l1_xyz, l1, idx.centres[1], idx.groups[1], train_enc)
        l3_xyz, l3 = self.set_abstraction("sa3", l2_xyz, l2, idx.centres[2], idx.groups[2], train_enc)
        l1_fp2, l2_fp3 = l1, l2
        if not encoder_grad:
            l1_fp2, l2_fp3, l3 = l1.detach(), l2.detach(), l3.detach()
        l2_new = self.feature_propagation("fp3", l2_xyz, l3_xyz, l2_fp3, l3, idx.nn3["fp3"], train_dec)
        l1_new = self.feature_propagation("fp2", l1_xyz, l2_xyz, l1_fp2, l2_new, idx.nn3["fp2"], train_dec)
        self._segments = list(self.sizes)
        l0 = self.feature_propagation("fp1", l0_xyz, l1_xyz.reshape(1, Q * S, 3), None, l1_new.reshape(1, Q * S, -1), idx.nn3["fp1"], train_dec)
        out = self.head(l0[0], train_head, mask)
        self._segments = None
        return out


def run(state, inputs, idx, mode, dtype, faults=(), first_step=0):
    """pn2_model_ref.run for the ragged wiring: STEPS[mode] forward + backward passes on one state, no optimiser between them, the running
    statistics carried on, the head's dropout step advancing -> one dict per step (out, grads, taps = {}, buffers, counts)."""
    m = R.MODES[mode]
    net = RaggedRestatement(state, dtype, per_cloud="bn_per_cloud" in faults)
    x = torch.from_numpy(inputs["x"]).to(dtype)
    results = []
    for step in range(first_step, first_step + R.STEPS[mode]):
        mask = R.dropout_mask(R.HEAD_SEED, step, x.shape[0], dtype) if m["train"][2] else None
        log_probs = net.forward(x, idx, m["train"], m["encoder_grad"], mask)
        loss = net.loss(log_probs, inputs["target"])
        keys = list(net.params)
        g = torch.autograd.grad(loss, [net.params[k] for k in keys], allow_unused=True)
        results.append(dict(out=dict(log_probs=log_probs.detach(), loss=loss.detach()), grads=dict(zip(keys, g)), taps={},
                            buffers=dict(net.buffers), counts=dict(net.counts)))
    return results


def measure(synth, mode, seeds, faults=()):
    """The float32 restatement (with `faults`) against the float64 one (without) on identical indices and masks, on one thread
    -> {seed: {kind: worst error over the steps}}."""
    inputs = case_inputs(synth)
    idx = indices_cpu_ragged(inputs["x"])
    idx32 = indices_cpu_ragged(inputs["x"], sa1_local=True) if "sa1_local_indices" in faults else idx
    per_seed = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # float32 sums depend on how a product is split over threads: the table is one thread's
    try:
        for seed in seeds:
            state = R.random_state(seed)
            worst = {}
            for g, r in zip(run(state, inputs, idx32, mode, torch.float32, faults), run(state, inputs, idx, mode, torch.float64)):
                for k, v in R.errors(g, r, mode).items():
                    worst[k] = max(worst.get(k, 0.0), v)
            per_seed[seed] = worst
    finally:
        torch.set_num_threads(threads)
    return per_seed


def worst_over(per_seed, seeds):
    out = {}
    for s in seeds:
        for k, v in per_seed[s].items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def bar(mode, k):
    """The GPU test's bar of kind k."""
    return R.GPU_FACTOR * BARS[mode][k]


def ratios(err, mode):
    """{kind: error / bar}; an exact result is inside any bar."""
    return {k: 0.0 if v == 0.0 else v / bar(mode, k) if bar(mode, k) else float("inf") for k, v in err.items()}


def fault_factor(synth, fault, mode="T", seed=None):
    """The largest error / bar over the kinds when the float32 restatement carries `fault` (seed: SEEDS[0])."""
    seed = SEEDS[0] if seed is None else seed
    return max(ratios(measure(synth, mode, [seed], (fault,))[seed], mode).values())


# Measured on one CPU thread.  Of the candidates 8, 9, .. the first eight whose float32 restatement stays within CAP / GPU_FACTOR in every mode;
# PASSED_OVER: the candidates before the eighth that do not, as seed: (mode, the worst float32 error of a gradient tensor).
SEEDS = (8, 9, 11, 12, 13, 14, 16, 17)
PASSED_OVER = {10: ('T', 0.0184), 15: ('T', 0.0212)}
BARS = {
    'T': {
        'log_probs': 3.75e-06, 'loss': 1.71e-07, 'grad.sa1.mlp_convs.weight': 5.68e-03, 'grad.sa1.mlp_bns.weight': 5.95e-03,
        'grad.sa1.mlp_bns.bias': 5.94e-03, 'grad.sa2.mlp_convs.weight': 5.40e-03, 'grad.sa2.mlp_bns.weight': 5.44e-03,
        'grad.sa2.mlp_bns.bias': 5.19e-03, 'grad.sa3.mlp_convs.weight': 4.89e-03, 'grad.sa3.mlp_bns.weight': 5.80e-03,
        'grad.sa3.mlp_bns.bias': 5.39e-03, 'grad.fp3.mlp_convs.weight': 5.43e-03, 'grad.fp3.mlp_bns.weight': 6.01e-03,
        'grad.fp3.mlp_bns.bias': 4.95e-03, 'grad.fp2.mlp_convs.weight': 5.89e-03, 'grad.fp2.mlp_bns.weight': 5.18e-03,
        'grad.fp2.mlp_bns.bias': 8.49e-03, 'grad.fp1.mlp_convs.weight': 5.36e-03, 'grad.fp1.mlp_bns.weight': 5.95e-03,
        'grad.fp1.mlp_bns.bias': 7.18e-03, 'grad.conv1.weight': 6.76e-06, 'grad.bn1.weight': 2.46e-06, 'grad.bn1.bias': 9.98e-08,
        'grad.conv2.weight': 9.48e-07, 'grad.conv2.bias': 1.02e-07, 'sa1.mlp_bns.running_mean': 9.51e-08,
        'sa1.mlp_bns.running_var': 9.45e-08, 'sa2.mlp_bns.running_mean': 1.06e-07, 'sa2.mlp_bns.running_var': 8.52e-08,
        'sa3.mlp_bns.running_mean': 1.19e-07, 'sa3.mlp_bns.running_var': 8.70e-08, 'fp3.mlp_bns.running_mean': 2.17e-07,
        'fp3.mlp_bns.running_var': 8.71e-08, 'fp2.mlp_bns.running_mean': 1.03e-07, 'fp2.mlp_bns.running_var': 8.55e-08,
        'fp1.mlp_bns.running_mean': 1.62e-07, 'fp1.mlp_bns.running_var': 9.34e-08, 'bn1.running_mean': 1.02e-07,
        'bn1.running_var': 8.99e-08,
    },
    'E': {
        'log_probs': 2.44e-07, 'loss': 8.93e-08, 'grad.sa1.mlp_convs.weight': 5.92e-07, 'grad.sa1.mlp_convs.bias': 3.60e-07,
        'grad.sa1.mlp_bns.weight': 3.61e-07, 'grad.sa1.mlp_bns.bias': 3.44e-07, 'grad.sa2.mlp_convs.weight': 2.52e-06,
        'grad.sa2.mlp_convs.bias': 2.45e-06, 'grad.sa2.mlp_bns.weight': 2.42e-06, 'grad.sa2.mlp_bns.bias': 3.00e-06,
        'grad.sa3.mlp_convs.weight': 2.97e-07, 'grad.sa3.mlp_convs.bias': 2.97e-07, 'grad.sa3.mlp_bns.weight': 2.77e-07,
        'grad.sa3.mlp_bns.bias': 2.71e-07, 'grad.fp3.mlp_convs.weight': 3.14e-07, 'grad.fp3.mlp_convs.bias': 2.68e-07,
        'grad.fp3.mlp_bns.weight': 2.73e-07, 'grad.fp3.mlp_bns.bias': 2.40e-07, 'grad.fp2.mlp_convs.weight': 2.83e-07,
        'grad.fp2.mlp_convs.bias': 2.13e-07, 'grad.fp2.mlp_bns.weight': 2.61e-07, 'grad.fp2.mlp_bns.bias': 2.05e-07,
        'grad.fp1.mlp_convs.weight': 2.41e-07, 'grad.fp1.mlp_convs.bias': 1.89e-07, 'grad.fp1.mlp_bns.weight': 2.53e-07,
        'grad.fp1.mlp_bns.bias': 1.80e-07, 'grad.conv1.weight': 1.70e-07, 'grad.conv1.bias': 8.42e-08, 'grad.bn1.weight': 9.33e-08,
        'grad.bn1.bias': 7.34e-08, 'grad.conv2.weight': 2.34e-07, 'grad.conv2.bias': 1.39e-07,
    },
    'D': {
        'log_probs': 2.44e-07, 'loss': 8.93e-08, 'grad.fp3.mlp_convs.weight': 3.14e-07, 'grad.fp3.mlp_convs.bias': 2.68e-07,
        'grad.fp3.mlp_bns.weight': 2.73e-07, 'grad.fp3.mlp_bns.bias': 2.40e-07, 'grad.fp2.mlp_convs.weight': 2.83e-07,
        'grad.fp2.mlp_convs.bias': 2.13e-07, 'grad.fp2.mlp_bns.weight': 2.61e-07, 'grad.fp2.mlp_bns.bias': 2.05e-07,
        'grad.fp1.mlp_convs.weight': 2.41e-07, 'grad.fp1.mlp_convs.bias': 1.89e-07, 'grad.fp1.mlp_bns.weight': 2.53e-07,
        'grad.fp1.mlp_bns.bias': 1.80e-07, 'grad.conv1.weight': 1.70e-07, 'grad.conv1.bias': 8.42e-08, 'grad.bn1.weight': 9.33e-08,
        'grad.bn1.bias': 7.34e-08, 'grad.conv2.weight': 2.34e-07, 'grad.conv2.bias': 1.39e-07,
    },
}
FAULT_FACTORS = {'sa1_local_indices': 376000.0, 'bn_per_cloud': 3050000.0}


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    from conftest import sub
    synth_ = sub("synthetic")
    per_mode = {m_: measure(synth_, m_, CANDIDATES) for m_ in MODE_NAMES}
    limit = R.CAP / R.GPU_FACTOR
    passed, seeds_ = {}, []
    for s_ in CANDIDATES:
        bad = [(max(per_mode[m_][s_].values()), m_) for m_ in MODE_NAMES if max(per_mode[m_][s_].values()) > limit]
        if bad and len(seeds_) < 8:
            passed[s_] = (max(bad)[1], float(f"{max(bad)[0]:.2e}"))
        elif len(seeds_) < 8:
            seeds_.append(s_)
    print(f"SEEDS = {tuple(seeds_)!r}")
    print(f"PASSED_OVER = {passed!r}")
    print("BARS = {")
    for m_ in MODE_NAMES:
        print(f"    {m_!r}: {{")
        line = "       "
        for k_, v_ in worst_over(per_mode[m_], seeds_).items():
            item = f" {k_!r}: {R.round_up(v_):.2e},"
            if len(line) + len(item) > 140:
                print(line)
                line = "       "
            line += item
        print(line + "\n    },")
    print("}")
    SEEDS, BARS = tuple(seeds_), {m_: {k_: R.round_up(v_) for k_, v_ in worst_over(per_mode[m_], seeds_).items()} for m_ in MODE_NAMES}
    print("FAULT_FACTORS = {" + ", ".join(f"{f_!r}: {float(f'{fault_factor(synth_, f_):.3g}')!r}" for f_ in FAULTS) + "}")
