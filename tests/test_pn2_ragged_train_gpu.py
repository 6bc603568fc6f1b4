"""pointnet_2_seg training and fine-tuning on clouds of UNEQUAL size (forward_ragged with a graph and in train mode,
pn2_step.train_loop_clouds) as a WHOLE against the float64 restatement tests/pn2_ragged_ref.py: forward, loss, every parameter's gradient,
every running statistic and every num_batches_tracked of a step, in modes T (all five flags, .train(), two steps), E (eval, decoder and
encoder grad) and D (decoder grad alone), on the reduced model of tests/pn2_finetune_util.py (128 / 32 / 8 centres) and clouds of 128, 129,
200, 200 and 511 points, some targets -1.

The discrete choices -- centres, groups and 3-NN indices of the package's own searches, ragged at level 0, and the dropout keep mask from
the head's seed and step -- are handed to the restatement; ReLU signs and max winners are its own.  The bars are 4 x the worst error of
the float32 restatement against the float64 one (pn2_ragged_ref.BARS, measured in test_pn2_ragged_ref_cpu.py), none above 0.05; the conv
biases in front of a batch-statistics BatchNorm are exact zeros.  Then: after training steps the .eval() forward_ragged still equals
forward_rows cloud by cloud, bit for bit; a default model keeps refusing train mode and never builds a graph; train_loop_clouds.

Observed on an MI355X (worst error / bar per test; then the worst among the gradients of the six blocks, whose train-mode bars carry a ReLU
decision that the kernels did not flip here):
  T  step 0: 0.39 grad.bn1.bias,  step 1: 0.44 grad.bn1.bias;  blocks 2.4e-4 (fp1.mlp_bns.weight);  running statistics <= 0.24;
     log_probs 0.20, loss 0.11
  E  0.66 grad.bn1.bias;  blocks 0.34 (fp1.mlp_bns.bias);  log_probs 0.40, loss 0.18
  D  the figures of E for the decoder and the head (the same kernels on the same values); the encoder's gradients None
No defect found.  The float64 restatement runs on the CPU; every test takes under two seconds."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_finetune_util as PU                     # noqa: E402
import pn2_model_ref as R                          # noqa: E402
import pn2_ragged_ref as G                         # noqa: E402

pytestmark = pytest.mark.gpu

SEED = G.SEEDS[0]
SIZES = list(G.SIZES)
SMALL = 90                                         # below sa1.npoint: train_loop_clouds pads it
FLAGS = {"T": dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True, head_batch_stats=True),
         "E": dict(decoder_grad=True, encoder_grad=True),
         "D": dict(decoder_grad=True)}


def _model(mode=None, **flags):
    """The package's pointnet_2_seg of `mode` (or of `flags`) at the reduced sizes, seeded, in the mode's train / eval state."""
    A = sub("pointNet.model.pointnetAtt")
    net = A.pointnet_2_seg(R.NUM_CLASSES, **(FLAGS[mode] if mode else flags)).eval()
    for sa, npoint, radius in zip((net.sa1, net.sa2, net.sa3), G.NPOINT, G.RADIUS):
        sa.npoint, sa.radius = npoint, radius
        assert sa.nsample == R.NSAMPLE
    PU.randomise(net, SEED)
    assert list(net.state_dict()) == list(R.state_shapes())           # the restatement's keys are the model's
    if mode and any(R.MODES[mode]["train"]):
        assert net.train() is net
    return net


@functools.lru_cache(maxsize=None)
def _case():
    """(inputs, rows [total, 9] on the GPU, the discrete choices of the package's own searches on them), computed once and shared."""
    U = sub("utils.utils")
    inputs = G.case_inputs(sub("synthetic"))
    rows = torch.from_numpy(inputs["x"]).cuda()
    xyz = rows[:, :3].contiguous()
    layout = U.ragged_layout("test", xyz, SIZES)
    c0 = torch.stack(U.fps_indices_ragged(xyz, SIZES, G.NPOINT[0]))                   # [Q, 128], relative to their cloud
    g0 = U.ball_query_ragged(xyz, layout, c0, G.RADIUS[0], R.NSAMPLE)
    levels = [None, xyz[(c0 + layout.off[:-1].unsqueeze(1)).long()].contiguous()]     # [Q, 128, 3]
    centres, groups = [c0], [g0]
    for npoint, radius in zip(G.NPOINT[1:], G.RADIUS[1:]):
        centres.append(U.fps_indices(levels[-1], npoint))
        groups.append(U.ball_query(levels[-1], centres[-1], radius, R.NSAMPLE))
        levels.append(U.gather_rows(levels[-1], centres[-1]))
    cpu = lambda t: t.cpu().numpy()
    nn3 = dict(fp3=cpu(U.three_nn(levels[2], levels[3])[0]), fp2=cpu(U.three_nn(levels[1], levels[2])[0]),
               fp1=[cpu(t) for t in U.three_nn_ragged(xyz, layout, levels[1])[0].split(SIZES)])
    assert nn3["fp3"].shape[2] == 3
    return inputs, rows, G.pack_indices([cpu(c) for c in centres], [cpu(g) for g in groups], nn3)


@functools.lru_cache(maxsize=None)
def _reference(mode):
    """The float64 restatement's STEPS[mode] steps on the seeded state: computed once, shared, never written to."""
    inputs, _, idx = _case()
    return G.run(R.random_state(SEED), inputs, idx, mode, torch.float64)


def _step(net):
    """One forward + backward of the package's model through forward_ragged, as train_loop_clouds drives it -> the dict of pn2_ragged_ref.run()."""
    P = sub("pointNet.model.pointnet2_utils")
    inputs, rows, _ = _case()
    for p in net.parameters():
        p.grad = None
    x = rows.clone().requires_grad_(True)
    log_probs = net.forward_ragged(x, SIZES)
    assert tuple(log_probs.shape) == (sum(SIZES), R.NUM_CLASSES) and log_probs.requires_grad
    loss, _, _ = P.seg_nll_loss(log_probs, torch.from_numpy(inputs["target"]).cuda(), torch.tensor(R.CLASS_W, device="cuda"))
    loss.backward()
    assert x.grad is None                                            # the input receives no gradient
    return dict(out=dict(log_probs=log_probs.detach(), loss=loss.detach()), grads={k: p.grad for k, p in net.named_parameters()}, taps={},
                buffers={k: v.clone() for k, v in net.named_buffers() if not k.endswith("num_batches_tracked")},
                counts={k: int(v) for k, v in net.named_buffers() if k.endswith("num_batches_tracked")})


def _compare(got, ref, mode, what):
    """Prints the worst error / bar per block and tensor kind of one step against the restatement's, then asserts it."""
    rat = G.ratios(R.errors(got, ref, mode), mode)
    print(f"pn2 ragged parity {mode} {what}: " + R.summary(rat))
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


def _frozen(net, before):
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(v, before[k]), k


def _eval_ragged_equals_rows(net):
    _, rows, _ = _case()
    net.eval()
    with torch.no_grad():
        logp = net.forward_ragged(rows, SIZES)
        off = 0
        for n in SIZES:
            assert torch.equal(logp[off:off + n], net.forward_rows(rows[off:off + n][None].contiguous())[0]), n
            off += n
    preds = net.predict_ragged(rows, SIZES)                          # an eval operation without a graph for every model, grad mode on
    assert preds.dtype == torch.int64 and not preds.requires_grad and torch.equal(preds, logp.argmax(1))


def test_training_from_scratch_two_steps_then_eval_bits():
    """Mode T: all 17 BatchNorms on the statistics of the whole call, dropout over `total` rows; a second step on the same model against
    the restatement advanced the same way.  Then the parameters move (a plain gradient step) and .eval() forward_ragged equals
    forward_rows cloud by cloud, bit for bit."""
    net = _model("T")
    ref = _reference("T")
    for step in range(2):
        assert net._head._step == step
        _compare(_step(net), ref[step], "T", f"step {step}")
    assert all(int(v) == 5 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))       # 3, and once per forward
    with torch.no_grad():
        for p in net.parameters():
            p.sub_(0.05 * p.grad)
    _, rows, _ = _case()
    with pytest.raises(NotImplementedError, match="eval"):
        net.predict_ragged(rows, SIZES)                              # train mode: the predict calls stay eval operations
    _eval_ragged_equals_rows(net)


def test_fine_tuning_with_frozen_statistics():
    """Mode E: the whole model differentiable in eval mode through forward_ragged; the buffers stay bit-unchanged."""
    net = _model("E")
    before = {k: v.clone() for k, v in net.state_dict().items()}
    got = _step(net)
    _compare(got, _reference("E")[0], "E", "step 0")
    _frozen(net, before)
    _eval_ragged_equals_rows(net)
    assert torch.equal(got["out"]["log_probs"], _model().forward_ragged(_case()[1], SIZES))     # a graph does not change a forward value
    with pytest.raises(NotImplementedError, match="eval"):
        _, rows, _ = _case()
        net.train().forward_ragged(rows, SIZES)                      # no batch-statistics flags: train mode is not built
    net.eval()


def test_decoder_only():
    """Mode D: the encoder's gradients are None, the decoder's and the head's those of the restatement with the boundary detached."""
    net = _model("D")
    before = {k: v.clone() for k, v in net.state_dict().items()}
    got = _step(net)
    assert all((g is None) == k.startswith(R.ENCODER) for k, g in got["grads"].items())
    _compare(got, _reference("D")[0], "D", "step 0")
    _frozen(net, before)


def test_a_default_model_is_unchanged():
    """Without the flags: no graph in eval mode even with grad mode on and parameters that require grad, the bits of the flagged model's
    eval forward, and NotImplementedError mentioning "eval" from all three ragged calls in train mode."""
    net = _model()
    _, rows, _ = _case()
    assert torch.is_grad_enabled() and all(p.requires_grad for p in net.parameters())
    logp = net.forward_ragged(rows, SIZES)
    assert not logp.requires_grad and logp.grad_fn is None
    with torch.no_grad():
        assert torch.equal(logp, _model("E").forward_ragged(rows, SIZES))
    clouds = list(rows.split(SIZES))
    net.train()
    try:
        for call in (lambda: net.forward_ragged(rows, SIZES), lambda: net.predict_ragged(rows, SIZES), lambda: net.predict_clouds(clouds)):
            with pytest.raises(NotImplementedError, match="eval"):
                call()
    finally:
        net.eval()
    small = rows[:SMALL + 128].contiguous()
    with pytest.raises(sub("_lib").AmpnetError, match="at least sa1.npoint=128 points, cloud 0 has 90"):
        _model("T").forward_ragged(small, [SMALL, 128])               # every cloud still needs sa1.npoint points


def _cluster(synth, seed, n):
    """[n, 10] float32 on the CPU as a cluster file holds it: nine feature columns and the ASPRS class code."""
    x = np.concatenate([synth.clouds(seed, 1, n)[0], synth.uniform(seed + 1000, (n, 6), -1.0, 1.0)], -1)
    codes = np.array([1, 15, 14, 3, 4, 5, 7], dtype=np.float32)[synth.randint(seed + 2000, (n,), 0, 7)]
    return torch.from_numpy(np.concatenate([x, codes[:, None]], -1).astype(np.float32))


def test_train_loop_clouds(synth):
    """The five clouds plus one of 90 points: train=True moves every trainable parameter that has a gradient (the conv biases in front of a
    batch-statistics BatchNorm have an exactly zero one and stay), returns preds / targets of sum(n_i) rows without the padding, and
    train=False is seg_nll_loss on forward_ragged under no_grad."""
    S, T, P, U = sub("pointNet.pn2_step"), sub("trainer"), sub("pointNet.model.pointnet2_utils"), sub("utils.utils")
    A = sub("pointNet.amp_test")
    sizes = SIZES + [SMALL]
    clouds = [_cluster(synth, 700 + i, n) for i, n in enumerate(sizes)]
    class_w = torch.tensor(R.CLASS_W, device="cuda")
    net = _model("T")
    # train=False first: the loss of the padded batch, the padding rows with target -1
    metrics, tg, preds, counts = S.train_loop_clouds(clouds, None, class_w, net, train=False)
    assert not net.training and tuple(tg.shape) == tuple(preds.shape) == (sum(sizes),) and tg.is_cuda and preds.dtype == torch.int64
    rows, want_t, _ = A._upload_clusters(clouds, torch.device("cuda"))
    assert torch.equal(tg, want_t) and len(set(tg.tolist())) == 5
    padded, _, gather, keep = U.pad_cloud_sizes(sizes, 128)
    assert padded == SIZES + [128]
    gather, keep = torch.from_numpy(gather).cuda(), torch.from_numpy(keep).cuda()
    pt = torch.full((sum(padded),), -1, dtype=torch.int64, device="cuda")
    pt[keep] = want_t
    with torch.no_grad():
        logp = net.forward_ragged(rows[gather].contiguous(), padded)
        loss, want_p, want_c = P.seg_nll_loss(logp, pt, class_w, want_preds=True, want_counts=True)
    assert torch.equal(metrics["loss"], loss) and torch.equal(preds, want_p[keep]) and torch.equal(counts, want_c)
    assert int(counts[-1]) == 128 - SMALL                            # the padding rows are the ignored ones
    # train=True
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    stats = {k: v.clone() for k, v in net.named_buffers()}
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    metrics, tg2, preds2, _ = S.train_loop_clouds(clouds, opt, class_w, net, train=True)
    assert net.training and torch.equal(tg2, want_t) and tuple(preds2.shape) == (sum(sizes),)
    assert torch.isfinite(metrics["loss"]) and not metrics["loss"].requires_grad
    for k, p in net.named_parameters():
        assert torch.equal(p, before[k]) == R.zero_by_construction(k, "T"), k
    for k, v in net.named_buffers():
        assert not torch.equal(v, stats[k]), k                       # every running statistic moved, every counter counted
    host = S.train_loop_clouds(clouds, opt, class_w, net, train=False, device_outputs=False)
    assert all(not t.is_cuda for t in host[1:]) and tuple(host[2].shape) == (sum(sizes),)
