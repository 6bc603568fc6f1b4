"""The test of the test, without a GPU: the whole-network restatement tests/pn2_model_ref.py
  * block by block against the numpy float64 restatements the layer tests already trust (sa_ref, fp_ref, sa_train_ref, fp_train_ref,
    seg_head_train_ref, seg_loss_ref) on the tensors of case A, to 1e-12 of each output's scale;
  * its table of bars: two of the measured seeds recomputed (float32 restatement against float64 on identical indices and masks) and still
    under the table, and no bar of the GPU test above CAP = 0.05;
  * the conv biases in front of a batch-statistics BatchNorm, whose true gradient is zero: below 1e-12 of their layer's dW norm in float64;
  * seven planted faults of the wiring, in the float32 restatement only: each must push at least one tensor to 10 x its GPU bar or more.

Measured: the float64 restatement takes 0.08 s for a forward + backward at case A and 0.04 s at case B; the file about 10 s.
The planted faults in mode T at (case A, case B), worst error / GPU bar and the tensor that shows it (all seven reach 10 x; none is a
finding about the bars):
  fp2_skip_detached            39, 274            tap.l1_fp2 (that contribution is missing: error 1)
  fp3_skip_detached            41, 236            tap.l2_fp3
  fp2_concat_swapped           6.1e5, 4.3e5       fp2.mlp_bns.running_mean
  biased_running_var           1.4e3, 2.9e3       fp3.mlp_bns.running_var
  next_steps_mask              4.7e5, 5.3e4       grad.bn1.bias, grad.conv2.weight
  sa2_not_recentred            3.3e5, 4.8e4       grad.bn1.bias, fp3.mlp_bns.running_mean
  ignored_rows_in_denominator  1.7e5, 1.7e5       grad.conv2.bias
The two detached skip inputs reach 10 x at the fan-in contributions; the parameter gradients behind them (sa1, sa2) move by 5 x their bars
at case A and 29 .. 83 x at case B -- a failure of the GPU test either way, but that is why tests/test_pn2_model_parity_gpu.py checks the
four contributions directly."""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import fp_ref                                      # noqa: E402
import fp_train_ref                                # noqa: E402
import pn2_model_ref as R                          # noqa: E402
import sa_ref                                      # noqa: E402
import sa_train_ref                                # noqa: E402
import seg_head_train_ref                          # noqa: E402
import seg_loss_ref                                # noqa: E402

SEED = R.SEEDS[0]
PAIRS = [(m, c) for m in R.MODES for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _case(case):
    inputs = R.case_inputs(sub("synthetic"), case)
    return inputs, R.indices_cpu(inputs["x"], case)


@functools.lru_cache(maxsize=None)
def _ref64(mode, case, seed):
    """The float64 run of (mode, case, seed), computed once and shared: nobody writes to it."""
    inputs, idx = _case(case)
    return R.run(R.random_state(seed, R.MODES[mode]["seg"]), inputs, idx, mode, torch.float64)


def _layers(state, name):
    """A block's parameters as the numpy restatements take them: per layer (W [cout, cin], b, gamma, beta, running_mean, running_var)."""
    out, l = [], 0
    while f"{name}.mlp_convs.{l}.weight" in state:
        W = state[f"{name}.mlp_convs.{l}.weight"]
        out.append(tuple(np.ascontiguousarray(t.numpy()) for t in (
            W.reshape(W.shape[0], W.shape[1]), state[f"{name}.mlp_convs.{l}.bias"], state[f"{name}.mlp_bns.{l}.weight"],
            state[f"{name}.mlp_bns.{l}.bias"], state[f"{name}.mlp_bns.{l}.running_mean"], state[f"{name}.mlp_bns.{l}.running_var"])))
        l += 1
    return out


def _close(got, want, what, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= tol * scale, (what, err, scale)


def _network(train):
    """One float64 forward of pointnet_2_seg at case A -> (net, state, inputs, idx, the traced tensors as numpy, log_probs)."""
    inputs, idx = _case("A")
    state = R.random_state(SEED)
    net = R.Restatement(state, torch.float64)
    x = torch.from_numpy(inputs["x"]).double()
    rows = x.shape[0] * x.shape[1]
    with torch.no_grad():
        logp = net.forward(x, idx, (train,) * 3, True, R.dropout_mask(R.HEAD_SEED, 0, rows, torch.float64) if train else None)
    t = {k: v.numpy() for k, v in net.trace.items() if k != "xyz"}
    t["xyz"] = [v.numpy().astype(np.float32) for v in net.trace["xyz"]]          # (exact: every level's coordinates are input values)
    t["l0_in"] = inputs["x"]
    return net, state, inputs, idx, t, logp.numpy()


#             block  level of xyz  its features   its output
SA_BLOCKS = (("sa1", 0, "l0_in", "l1"), ("sa2", 1, "l1", "l2"), ("sa3", 2, "l2", "l3"))
#             block  fine, coarse   points1   points2    its output
FP_BLOCKS = (("fp3", 2, 3, "l2", "l3", "l2_new"), ("fp2", 1, 2, "l1", "l2_new", "l1_new"), ("fp1", 0, 1, None, "l1_new", "l0"))


def _exact_dist2(fine, coarse, nn3):
    """The squared distances to the given neighbours in float64 from the float32 coordinates."""
    d = fine.astype(np.float64)[:, :, None, :] - np.stack([c.astype(np.float64)[i] for c, i in zip(coarse, nn3)])
    return (d * d).sum(-1)


def _train_chain(ref, x, layers):
    """The train-mode layers of a block on its input rows x through ref.forward_layer, one after the other -> the records per layer.  Only
    the float64 values are used: the carried float32 bars (which batch normalisation re-amplifies layer by layer) are left at zero."""
    tape = []
    for layer in layers:
        tape.append(ref.forward_layer(x, np.zeros_like(x), layer, R.BN_EPS))
        x = np.maximum(tape[-1]["y"], 0.0)
    return tape


def test_eval_blocks_equal_the_numpy_restatements():
    net, state, inputs, idx, t, logp = _network(train=False)
    eps = [R.BN_EPS] * 3
    for name, lvl, feats, out in SA_BLOCKS:
        layers = _layers(state, name)
        for b in range(inputs["x"].shape[0]):
            want, _ = sa_ref.sa_forward(t["xyz"][lvl][b], idx.centres[lvl][b].numpy(), idx.groups[lvl][b].numpy(), t[feats][b], layers, eps)
            _close(t[out][b], want, (name, b))
    for name, fine, coarse, p1, p2, out in FP_BLOCKS:
        layers = _layers(state, name)
        nn3 = idx.nn3[name].numpy()
        d2 = _exact_dist2(t["xyz"][fine], t["xyz"][coarse], nn3)
        for b in range(inputs["x"].shape[0]):
            want, _ = fp_ref.fp_forward(None if p1 is None else t[p1][b], t[p2][b], nn3[b], d2[b], layers, eps)
            _close(t[out][b], want, (name, b))
    for k, v in net.buffers.items():                                  # eval mode: nothing moves
        assert torch.equal(v, state[k].double()), k
    assert all(v == 3 for v in net.counts.values())


def test_train_blocks_and_loss_equal_the_numpy_restatements():
    net, state, inputs, idx, t, logp = _network(train=True)
    B = inputs["x"].shape[0]
    for name, lvl, feats, out in SA_BLOCKS:
        layers = _layers(state, name)
        group = idx.groups[lvl].numpy()
        tape = _train_chain(sa_train_ref, sa_train_ref.input_rows(t["xyz"][lvl], idx.centres[lvl].numpy(), group, t[feats])[0], layers)
        _close(t[out], np.maximum(tape[-1]["y"], 0.0).reshape(group.shape + (-1,)).max(2), name)
        for l, f in enumerate(tape):
            _close(net.buffers[f"{name}.mlp_bns.{l}.running_mean"].numpy(), f["rm"][0], (name, l, "running_mean"))
            _close(net.buffers[f"{name}.mlp_bns.{l}.running_var"].numpy(), f["rv"][0], (name, l, "running_var"))
    for name, fine, coarse, p1, p2, out in FP_BLOCKS:
        layers = _layers(state, name)
        nn3 = idx.nn3[name].numpy()
        d2 = _exact_dist2(t["xyz"][fine], t["xyz"][coarse], nn3)
        tape = _train_chain(fp_train_ref, fp_train_ref.input_rows(None if p1 is None else t[p1], t[p2], nn3, d2)[0], layers)
        _close(t[out], np.maximum(tape[-1]["y"], 0.0).reshape(t[out].shape), name)
        for l, f in enumerate(tape):
            _close(net.buffers[f"{name}.mlp_bns.{l}.running_mean"].numpy(), f["rm"][0], (name, l, "running_mean"))
            _close(net.buffers[f"{name}.mlp_bns.{l}.running_var"].numpy(), f["rv"][0], (name, l, "running_var"))
    # the head, forward and backward, from the gradient of the loss at its log-probabilities
    rows = t["l0"].reshape(-1, 128)
    target = inputs["target"].reshape(-1)
    w = np.asarray(R.CLASS_W, dtype=np.float32)
    nll = seg_loss_ref.nll(logp.reshape(-1, R.NUM_CLASSES), target, w)
    dlogp = seg_loss_ref.nll_backward(target, w, nll["sums"][1], 1.0, R.NUM_CLASSES)
    params = tuple(np.ascontiguousarray(state[k].numpy().reshape(state[k].shape[:2]) if state[k].dim() == 3 else state[k].numpy())
                   for k in ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "conv2.weight", "conv2.bias"))
    want, _ = seg_head_train_ref.seg_train(rows, params, R.BN_EPS, R.P_DROP, R.head_seed(R.HEAD_SEED, 0), dlogp, margin=-1.0)
    _close(logp.reshape(-1, R.NUM_CLASSES), want["logp"][0], "log_probs")
    _close(net.buffers["bn1.running_mean"].numpy(), want["running_mean"][0], "bn1.running_mean")
    _close(net.buffers["bn1.running_var"].numpy(), want["running_var"][0], "bn1.running_var")
    assert all(v == 4 for v in net.counts.values()) and len(net.counts) == 17
    step = _ref64("T", "A", SEED)[0]
    _close(float(step["out"]["loss"]), nll["loss"], "loss")
    _close(step["out"]["log_probs"].numpy().reshape(-1, R.NUM_CLASSES), want["logp"][0], "log_probs of run()")
    for key, name in (("conv1.weight", "dW1"), ("bn1.weight", "dgamma"), ("bn1.bias", "dbeta"), ("conv2.weight", "dW2"), ("conv2.bias", "db2")):
        _close(step["grads"][key].numpy().reshape(want[name][0].shape), want[name][0], key, tol=1e-10)
    assert B == 2


def test_state_shapes_and_seeds():
    for seg, bns in ((True, 17), (False, 16)):
        shapes = R.state_shapes(seg)
        assert sum(k.endswith("num_batches_tracked") for k in shapes) == bns
        state = R.random_state(SEED, seg)
        assert list(state) == list(shapes) and all(tuple(state[k].shape) == tuple(s) for k, s in shapes.items())
    assert len(R.SEEDS) == 8 and not set(R.SEEDS) & set(R.PASSED_OVER)
    assert all(worst > R.CAP / R.GPU_FACTOR for _, worst in R.PASSED_OVER.values())
    inputs, idx = _case("B")
    assert inputs["x"].shape == (3, 200, 9) and idx.nn3["fp3"].shape == (3, 12, 3) and idx.groups[2].shape == (3, 3, 32)
    members = [len(set(g.tolist())) for cloud in idx.groups[2] for g in cloud]
    assert max(members) <= 12                                        # sa3's groups at case B: at least 20 of the 32 slots repeat a member


def test_no_bar_exceeds_the_cap():
    assert sorted(R.BARS) == sorted(PAIRS)
    for key, table in R.BARS.items():
        for k, v in table.items():
            assert R.GPU_FACTOR * v <= R.CAP, (key, k, v)


@pytest.mark.parametrize("mode,case", PAIRS)
def test_table_dominates_two_recomputed_seeds(mode, case):
    inputs, idx = _case(case)
    t0 = time.perf_counter()
    R.run(R.random_state(R.SEEDS[2], R.MODES[mode]["seg"]), inputs, idx, mode, torch.float64)
    t64 = (time.perf_counter() - t0) / R.STEPS[mode]
    want = {seed: _ref64(mode, case, seed) for seed in R.SEEDS[:2]}
    got = R.measure(sub("synthetic"), mode, case, R.SEEDS[:2], ref64=want)
    table = R.BARS[(mode, case)]
    assert sorted(got) == sorted(table)
    worst = max(got, key=lambda k: got[k] / table[k] if table[k] else 0.0)
    print(f"pn2 restatement {mode} {case}: float64 forward + backward {t64:.2f} s; worst float32 error / table "
          f"{got[worst] / table[worst] if table[worst] else 0.0:.2f} at {worst}")
    for k, v in got.items():
        assert v <= table[k], (k, v, table[k])


@pytest.mark.parametrize("mode,case", [p for p in PAIRS if any(R.MODES[p[0]]["train"])])
def test_bias_gradients_in_front_of_batch_statistics_are_zero(mode, case):
    for step in _ref64(mode, case, SEED):
        zero = [k for k in step["grads"] if R.zero_by_construction(k, mode)]
        assert len(zero) == (17 if mode == "T" else 16)
        for k in zero:
            dW = step["grads"][k.replace(".bias", ".weight")]
            assert float(step["grads"][k].norm()) <= 1e-12 * float(dW.norm()), (k, float(step["grads"][k].norm()), float(dW.norm()))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_caught(fault):
    """The float32 restatement WITH the fault against the float64 one without, the comparison the GPU test makes of the package: at least one
    tensor at 10 x its bar or more, in both cases.  Next to it the unplanted float32 run's error of the same tensor."""
    for case in R.CASES:
        want = {SEED: _ref64("T", case, SEED)}
        clean = R.measure(sub("synthetic"), "T", case, [SEED], ref64=want)
        rat = R.ratios(R.measure(sub("synthetic"), "T", case, [SEED], faults=(fault,), ref64=want), "T", case)
        k = max(rat, key=rat.get)
        print(f"planted {fault} at case {case}: {k} at {rat[k]:.3g} x its bar (unplanted: {clean[k] / R.bar('T', case, k):.3g})")
        assert rat[k] >= 10.0, (fault, case, k, rat[k])
        assert max(R.ratios(clean, "T", case).values()) <= 1.0 / R.GPU_FACTOR
