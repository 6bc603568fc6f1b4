"""pointnet_2 / pointnet_2_seg as a WHOLE against the plain float64 restatement tests/pn2_model_ref.py: forward, loss, every parameter's
gradient and every BatchNorm's running statistics of a step, in the model's real modes, at reduced sizes.  The layer tests hold every
kernel to float64 on its own inputs and the model tests compare the model with the C ABI bit for bit; this file is the one that holds the
WIRING -- which tensor goes where, in which layout, with which saved state, and what comes back along both branches of a skip connection
-- to something independent of the package.

The discrete choices (centres, ball-query groups, 3-NN indices from utils.fps_indices / ball_query / three_nn on the same coordinates, and
the dropout keep mask from the head's seed and step) are handed to the restatement; ReLU signs and max winners are its own.  The bars are
4 x the worst error of the float32 restatement against the float64 one (pn2_model_ref.BARS, measured in test_pn2_model_ref_cpu.py), none
above 0.05; the conv biases in front of a batch-statistics BatchNorm are exact zeros.

Cases (pn2_model_ref.CASES): A = pn2_finetune_util's reduced model (B 2, N 512, centres 128 / 32 / 8); B = tails and padding (B 3, N 200,
centres 48 / 12 / 3: N no multiple of 64, fp3 from exactly three coarse points, sa3's groups mostly repeats).  No size had to be moved.
Modes: T pointnet_2_seg with all five flags in train mode, two steps;  E decoder_grad + encoder_grad in eval mode;  D decoder_grad alone;
G pointnet_2 with its four flags in train mode.  The float64 restatement runs on the CPU: 0.02 .. 0.08 s per forward + backward; every
test takes under a second but the first train-mode call of a process (2.9 s).

Observed on an MI355X (worst error / bar per test; then the worst among the gradients of the six blocks, whose bars carry a ReLU decision
that the kernels did not flip here, so they sit four orders below them in the train modes):
  T A  step 0: 0.44 grad.bn1.bias,  step 1: 0.40 grad.conv2.bias;  blocks 5.7e-4 (fp1.mlp_bns.weight);  running statistics <= 0.27
  T B  step 0: 0.40 grad.conv2.bias, step 1: 0.38 grad.conv2.bias;  blocks 1.2e-3 (fp2.mlp_bns.weight);  log_probs 0.23, loss 0.19
  E A  0.53 grad.bn1.bias;   blocks 0.36 (fp1.mlp_bns.bias);    log_probs 0.39, loss 0.18
  E B  0.71 grad.conv1.bias; blocks 0.32 (fp1.mlp_bns.weight);  log_probs 0.34, loss 0.13
  D A, D B  the figures of E A, E B for the decoder and the head (the same kernels on the same values); the encoder's gradients None
  G A  0.26 sa2.mlp_bns.running_mean; blocks 6.1e-4;  l0_points 0.22, glob 0.22
  G B  0.25 grad.conv1.bias;          blocks 1.4e-3;  l0_points 0.21, glob 0.20
  fan-in, T A:  l1 = sa2's + fp2's and l2 = sa3's + fp3's contribution bit for bit;  each alone 7.8e-5 .. 1.3e-4 of its bar
No defect found: the worst ratio is 0.71, at conv1.bias of mode E / D, case B."""
import functools
import os
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_finetune_util as PU                     # noqa: E402
import pn2_model_ref as R                          # noqa: E402

pytestmark = pytest.mark.gpu

SEED = R.SEEDS[0]
FLAGS = {"T": dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True, head_batch_stats=True),
         "E": dict(decoder_grad=True, encoder_grad=True),
         "D": dict(decoder_grad=True),
         "G": dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True)}
CASE_NAMES = sorted(R.CASES)


def _model(mode, case):
    """The package's model of `mode` at the sizes of `case`, seeded (pn2_finetune_util.randomise), in the mode's train / eval state."""
    A = sub("pointNet.model.pointnetAtt")
    seg = R.MODES[mode]["seg"]
    net = (A.pointnet_2_seg if seg else A.pointnet_2)(R.NUM_CLASSES, **FLAGS[mode]).eval()
    c = R.CASES[case]
    for sa, npoint, radius in zip((net.sa1, net.sa2, net.sa3), c["npoint"], c["radius"]):
        sa.npoint, sa.radius = npoint, radius
        assert sa.nsample == R.NSAMPLE
    PU.randomise(net, SEED)
    assert list(net.state_dict()) == list(R.state_shapes(seg))        # the restatement's keys are the model's
    if any(R.MODES[mode]["train"]):
        assert net.train() is net
    if seg:
        assert (net._head.seed, net._head._step, net.drop1.p, net._head.training) == (R.HEAD_SEED, 0, R.P_DROP, R.MODES[mode]["train"][2])
    return net


@functools.lru_cache(maxsize=None)
def _case(case):
    """(inputs, x [B, N, 9] on the GPU, the discrete choices of the package's own searches on it), computed once and shared."""
    U = sub("utils.utils")
    inputs = R.case_inputs(sub("synthetic"), case)
    x = torch.from_numpy(inputs["x"]).cuda()
    c = R.CASES[case]
    levels, centres, groups = [x[..., :3].contiguous()], [], []
    for npoint, radius in zip(c["npoint"], c["radius"]):
        centres.append(U.fps_indices(levels[-1], npoint))
        groups.append(U.ball_query(levels[-1], centres[-1], radius, R.NSAMPLE))
        levels.append(U.gather_rows(levels[-1], centres[-1]))
    nn3 = {name: U.three_nn(levels[i], levels[i + 1])[0] for name, i in zip(R.DECODER, (2, 1, 0))}
    assert nn3["fp3"].shape[2] == 3
    return inputs, x, R.Indices(centres, groups, nn3)


@functools.lru_cache(maxsize=None)
def _reference(mode, case):
    """The float64 restatement's STEPS[mode] steps on the seeded state: computed once, shared, never written to."""
    inputs, _, idx = _case(case)
    t0 = time.perf_counter()
    ref = R.run(R.random_state(SEED, R.MODES[mode]["seg"]), inputs, idx, mode, torch.float64)
    print(f"pn2 parity {mode} {case}: float64 restatement {(time.perf_counter() - t0) / R.STEPS[mode]:.2f} s per forward + backward")
    return ref


def _step(net, mode, case):
    """One forward + backward of the package's model, as pn2_step drives it -> the dict of pn2_model_ref.run()."""
    P = sub("pointNet.model.pointnet2_utils")
    inputs, x, _ = _case(case)
    for p in net.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    if R.MODES[mode]["seg"]:
        log_probs = net.forward_rows(x)
        loss, _, _ = P.seg_nll_loss(log_probs, torch.from_numpy(inputs["target"]).cuda(), torch.tensor(R.CLASS_W, device="cuda"))
        out = dict(log_probs=log_probs.detach(), loss=loss.detach())
    else:
        glob, l0 = net(x.transpose(1, 2).contiguous())
        loss = (l0 * torch.from_numpy(inputs["r"]).cuda()).sum() + (glob * torch.from_numpy(inputs["q"]).cuda()).sum()
        out = dict(l0_points=l0.detach(), glob=glob.detach())
    loss.backward()
    assert x.grad is None                                            # the input receives no gradient
    return dict(out=out, grads={k: p.grad for k, p in net.named_parameters()}, taps={},
                buffers={k: v.clone() for k, v in net.named_buffers() if not k.endswith("num_batches_tracked")},
                counts={k: int(v) for k, v in net.named_buffers() if k.endswith("num_batches_tracked")})


def _compare(got, ref, mode, case, what):
    """Asserts one step against the restatement's and prints the worst error / bar per block and tensor kind."""
    rat = R.ratios(R.errors(got, ref, mode), mode, case)
    print(f"pn2 parity {mode} {case} {what}: " + R.summary(rat))
    assert sorted(got["grads"]) == sorted(ref["grads"]) and sorted(got["buffers"]) == sorted(ref["buffers"])
    for k, r in ref["grads"].items():
        g = got["grads"][k]
        if r is None:
            assert g is None, k
            continue
        assert g is not None and tuple(g.shape) == tuple(r.shape) and bool(torch.isfinite(g).all()), k
        if R.zero_by_construction(k, mode):
            assert bool((g == 0).all()), k
    assert got["counts"] == ref["counts"]
    worst = max(rat, key=rat.get)
    assert rat[worst] <= 1.0, (worst, rat[worst])
    return rat


def _frozen(net, before):
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("case", CASE_NAMES)
def test_training_from_scratch_two_steps(case):
    """Mode T: all 17 BatchNorms on batch statistics, dropout from the head's seed; then a second step on the same model, against the
    restatement advanced the same way (its own new running statistics, the mask of _step = 1)."""
    net = _model("T", case)
    ref = _reference("T", case)
    assert sum(k.endswith("num_batches_tracked") for k in net.state_dict()) == 17
    for step in range(2):
        assert net._head._step == step
        _compare(_step(net, "T", case), ref[step], "T", case, f"step {step}")
    assert all(int(v) == 5 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("case", CASE_NAMES)
def test_fine_tuning_with_frozen_statistics(case):
    """Mode E: the whole model differentiable in eval mode; the buffers stay bit-unchanged."""
    net = _model("E", case)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    _compare(_step(net, "E", case), _reference("E", case)[0], "E", case, "step 0")
    _frozen(net, before)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_decoder_only(case):
    """Mode D: the encoder's gradients are None, the decoder's and the head's those of the restatement with the boundary detached."""
    net = _model("D", case)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    got = _step(net, "D", case)
    assert all((g is None) == k.startswith(R.ENCODER) for k, g in got["grads"].items())
    _compare(got, _reference("D", case)[0], "D", case, "step 0")
    _frozen(net, before)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_pointnet_2_backbone_in_train_mode(case):
    """Mode G: l0_points and the global feature (conv1 and the max over the points, the torch part), gradients and statistics."""
    _compare(_step(_model("G", case), "G", case), _reference("G", case)[0], "G", case, "step 0")


def test_both_branches_of_the_two_fan_in_points():
    """l1_points feeds sa2 and fp2's skip input, l2_points sa3 and fp3's: each consumer takes its features through a .clone() (the same
    bits, an identity backward), so a hook on the clone sees that consumer's contribution alone."""
    case = "A"
    plain = _model("T", case)
    _, x, _ = _case(case)
    with torch.no_grad():
        want = plain.forward_rows(x)
    net = _model("T", case)
    seen = {}

    def tap(block, pos, name, total):
        inner = block._forward_rows

        def wrapped(*args):
            args = list(args)
            if total not in seen:
                seen[total] = None
                args[pos].register_hook(lambda g: seen.__setitem__(total, g.detach().clone()))
            args[pos] = args[pos].clone()
            args[pos].register_hook(lambda g: seen.__setitem__(name, g.detach().clone()))
            return inner(*args)

        block._forward_rows = wrapped

    tap(net.sa2, 1, "l1_sa2", "l1")
    tap(net.fp2, 2, "l1_fp2", "l1")
    tap(net.sa3, 1, "l2_sa3", "l2")
    tap(net.fp3, 2, "l2_fp3", "l2")
    got = _step(net, "T", case)
    assert torch.equal(got["out"]["log_probs"], want)                # the wrapped model computes the unwrapped one's bits
    assert sorted(seen) == sorted(R.TAPS + ("l1", "l2")) and all(v is not None for v in seen.values())      # every hook fired
    for total, a, b in (("l1", "l1_sa2", "l1_fp2"), ("l2", "l2_sa3", "l2_fp3")):
        assert torch.equal(seen[total], seen[a] + seen[b]), total     # the float32 sum of the two contributions, bit for bit
    ref = _reference("T", case)[0]
    rat = {k: R.rel_l2(seen[k], ref["taps"][k]) / R.bar("T", case, "tap." + k) for k in R.TAPS}
    print(f"pn2 parity fan-in T {case}: " + R.summary(rat))
    assert max(rat.values()) <= 1.0, rat
