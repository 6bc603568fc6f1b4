"""bench.py --dump-outputs, host side: which arrays a step's result becomes, and how they are written (dtype, size cap, sample)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_step_outputs_names_every_returned_tensor_and_the_module_state():
    b = _bench()
    out = dict(logits=torch.randn(2, 5, 3), preds=torch.arange(6), ce=torch.tensor([1.5, 2.0]), targets_pc=torch.zeros(6), B=2,
               grad_bufs=(torch.ones(4), torch.zeros(2)), pending={}, feat=None)
    bn = torch.nn.BatchNorm1d(3)
    got = b.step_outputs(out, (("bn", bn),))
    assert sorted(got) == ["bn_state", "ce", "grad_bufs_0", "grad_bufs_1", "logits", "preds"]
    assert np.array_equal(got["logits"], out["logits"].numpy())
    # weight, bias, running_mean, running_var in state_dict order; the integer num_batches_tracked is not an output
    assert np.array_equal(got["bn_state"], np.concatenate([np.ones(3), np.zeros(3), np.zeros(3), np.ones(3)]).astype(np.float32))


def test_write_outputs_keeps_float32_widens_the_rest_and_samples_over_the_cap(tmp_path):
    b = _bench()
    arrays = {"big": np.arange(3_000_000, dtype=np.float32), "idx": np.arange(1_000_000, dtype=np.int64), "small": np.ones(7, np.float32)}
    for run in ("a", "b"):
        b.write_outputs(str(tmp_path / run), arrays, limit=4_000_000)
    data = sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "idx.npy", "small.npy"] and data <= 4_000_000
    small, idx, big = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("small", "idx", "big"))
    assert small.dtype == np.float32 and np.array_equal(small, arrays["small"])          # under its share: whole
    assert idx.dtype == np.float64 and big.dtype == np.float32
    for a in (idx, big):                                                                  # over it: a sorted sample of the elements
        assert 0 < a.size and np.all(np.diff(a) > 0) and a[-1] < 3_000_000
    for n in ("small", "idx", "big"):                                                     # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))
    b.write_outputs(str(tmp_path / "whole"), arrays)                                      # the default cap holds all of it
    assert np.array_equal(np.load(tmp_path / "whole" / "idx.npy"), np.arange(1_000_000, dtype=np.float64))
