"""The test of the test, without a GPU: the ragged wiring tests/pn2_ragged_ref.py on top of pn2_model_ref.Restatement
  * on clouds of ONE size it is pn2_model_ref's own uniform wiring: forward, loss, every gradient, every running statistic to 1e-12;
  * its table of bars: two of the measured seeds recomputed in every mode (float32 restatement against float64 on identical indices and
    masks) and still under the table, no bar of the GPU test above CAP = 0.05, eight seeds, every seed passed over listed with a figure
    above CAP / GPU_FACTOR;
  * two planted faults of the wiring, in the float32 restatement only -- sa1's indices of the clouds after the first left relative to their
    cloud, and the BatchNorm statistics of sa1, fp1 and the head taken cloud by cloud -- each must push a tensor past its GPU bar.

Measured, mode T, worst error / GPU bar (pn2_ragged_ref.FAULT_FACTORS): sa1_local_indices 3.8e5, bn_per_cloud 3.1e6 -- the running
statistics and the head's gradients have bars of 1e-7 .. 1e-5, and either fault moves them by a tenth of their size."""
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
import pn2_model_ref as R                          # noqa: E402
import pn2_ragged_ref as G                         # noqa: E402


@functools.lru_cache(maxsize=None)
def _synth():
    return sub("synthetic")


def test_the_table_is_complete_and_inside_the_cap():
    assert len(G.SEEDS) == 8 and len(set(G.SEEDS)) == 8 and not set(G.SEEDS) & set(G.PASSED_OVER)
    assert sorted(G.SEEDS + tuple(G.PASSED_OVER)) == list(range(min(G.SEEDS), max(G.SEEDS) + 1))     # the first eight that qualify
    assert all(mode in G.MODE_NAMES and fig > R.CAP / R.GPU_FACTOR for mode, fig in G.PASSED_OVER.values())
    assert sorted(G.BARS) == sorted(G.MODE_NAMES)
    for mode in G.MODE_NAMES:
        assert all(0.0 < G.bar(mode, k) <= R.CAP for k in G.BARS[mode]), mode
        grads = {k for k in G.BARS[mode] if k.startswith("grad.")}
        want = {"grad." + R.kind(k) for k in R.state_shapes() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))
                and not R.zero_by_construction(k, mode) and (R.MODES[mode]["encoder_grad"] or not k.startswith(R.ENCODER))}
        assert grads == want, (mode, grads ^ want)
    assert sum(k.endswith(("running_mean", "running_var")) for k in G.BARS["T"]) == 14            # every running statistic, per block kind


@pytest.mark.parametrize("mode", G.MODE_NAMES)
def test_two_seeds_recomputed_stay_under_the_table(mode):
    seeds = (G.SEEDS[0], G.SEEDS[5])
    per_seed = G.measure(_synth(), mode, seeds)
    for seed in seeds:
        assert sorted(per_seed[seed]) == sorted(G.BARS[mode]), (mode, seed)
        for k, v in per_seed[seed].items():
            assert v <= G.BARS[mode][k], (mode, seed, k, v, G.BARS[mode][k])


@pytest.mark.parametrize("mode", G.MODE_NAMES)
def test_on_clouds_of_one_size_the_ragged_wiring_is_the_uniform_one(mode):
    """Case B of pn2_model_ref (3 clouds of 200 points) through both wirings in float64: the same numbers."""
    inputs = R.case_inputs(_synth(), "B")
    B, N = inputs["x"].shape[:2]
    uniform = R.indices_cpu(inputs["x"], "B")
    nn3 = {k: v.numpy() for k, v in uniform.nn3.items()}
    nn3["fp1"] = list(nn3["fp1"])
    idx = G.pack_indices([c.numpy() for c in uniform.centres], [g.numpy() for g in uniform.groups], nn3, sizes=(N,) * B)
    state = R.random_state(G.SEEDS[0])
    want = R.run(state, inputs, uniform, mode, torch.float64)
    m = R.MODES[mode]
    net = G.RaggedRestatement(state, torch.float64, sizes=(N,) * B)
    x = torch.from_numpy(inputs["x"]).double().reshape(B * N, 9)
    for step in range(R.STEPS[mode]):
        mask = R.dropout_mask(R.HEAD_SEED, step, B * N, torch.float64) if m["train"][2] else None
        log_probs = net.forward(x, idx, m["train"], m["encoder_grad"], mask)
        loss = net.loss(log_probs, inputs["target"])
        keys = list(net.params)
        grads = dict(zip(keys, torch.autograd.grad(loss, [net.params[k] for k in keys], allow_unused=True)))
        ref = want[step]
        assert float((log_probs.detach().reshape(B, N, -1) - ref["out"]["log_probs"]).abs().max()) <= 1e-12
        assert abs(float(loss.detach()) - float(ref["out"]["loss"])) <= 1e-12 * abs(float(ref["out"]["loss"]))
        for k, r in ref["grads"].items():
            assert (grads[k] is None) == (r is None), k
            if r is not None and not R.zero_by_construction(k, mode):
                assert R.rel_l2(grads[k], r) <= 1e-10, (mode, step, k)
        for k, r in ref["buffers"].items():
            assert R.rel_l2(net.buffers[k], r) <= 1e-12, (mode, step, k)
        assert net.counts == ref["counts"]


@pytest.mark.parametrize("fault", G.FAULTS)
def test_a_planted_wiring_fault_exceeds_a_bar(fault):
    factor = G.fault_factor(_synth(), fault)
    print(f"pn2 ragged ref, planted {fault}: worst error / GPU bar {factor:.3g} (recorded {G.FAULT_FACTORS[fault]:.3g})")
    assert factor > 10.0, (fault, factor)
    assert 0.5 <= factor / G.FAULT_FACTORS[fault] <= 2.0, (fault, factor)
