"""pointnet_2_seg on clouds of unequal size in one launch sequence (forward_ragged / predict_ragged / predict_clouds, pointNet/pn2_infer.py):
cloud by cloud the bits of the uniform path on that cloud alone.  The reduced model of tests/pn2_finetune_util.py (128 / 32 / 8 centres)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_finetune_util as F                      # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [128, 129, 200, 200, 511]                  # npoint itself, one more, two equal clouds, no multiple of a 32-row tile
SMALL = 90                                         # below sa1.npoint: predict_clouds pads it


@pytest.fixture(scope="module")
def net():
    M = sub("pointNet.model.pointnetAtt")
    net = M.pointnet_2_seg(5).eval()
    for sa, npoint, radius in ((net.sa1, 128, 0.2), (net.sa2, 32, 0.4), (net.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    F.randomise(net, 8)
    return net


def _cloud(synth, seed, n, cols=9):
    """[n, cols] float32: coordinates of synth.clouds, features in [-1, 1]; column 9 (when asked for) holds ASPRS class codes."""
    x = np.concatenate([synth.clouds(seed, 1, n)[0], synth.uniform(seed + 1000, (n, 6), -1.0, 1.0)], -1)
    if cols == 10:
        codes = np.array([1, 15, 14, 3, 4, 5, 7], dtype=np.float32)[synth.randint(seed + 2000, (n,), 0, 7)]
        x = np.concatenate([x, codes[:, None]], -1)
    return torch.from_numpy(x.astype(np.float32))


@pytest.fixture(scope="module")
def clouds(synth):
    return [_cloud(synth, 300 + i, n).cuda() for i, n in enumerate(SIZES)]


@pytest.fixture(scope="module")
def alone(net, clouds):
    """The reference, once: forward_rows / predict_rows on every cloud alone."""
    return [(net.forward_rows(c[None].contiguous())[0], net.predict_rows(c[None].contiguous())[0]) for c in clouds]


def test_forward_and_predict_ragged_equal_the_uniform_path_cloud_by_cloud(net, clouds, alone):
    rows = torch.cat(clouds).contiguous()
    logp = net.forward_ragged(rows, SIZES)
    preds = net.predict_ragged(rows, SIZES)
    assert tuple(logp.shape) == (sum(SIZES), 5) and logp.dtype == torch.float32 and not logp.requires_grad
    assert tuple(preds.shape) == (sum(SIZES),) and preds.dtype == torch.int64
    off = 0
    for b, n in enumerate(SIZES):
        assert torch.equal(logp[off:off + n], alone[b][0]), (b, n)
        assert torch.equal(preds[off:off + n], alone[b][1]), (b, n)
        off += n
    assert len(torch.unique(logp, dim=0)) > sum(SIZES) // 2                            # (the answer follows the point)
    # two identical calls return the same bits; the order of the clouds does not reach a cloud's result
    assert torch.equal(net.forward_ragged(rows, SIZES), logp) and torch.equal(net.predict_ragged(rows, SIZES), preds)
    back = net.forward_ragged(torch.cat(clouds[::-1]).contiguous(), SIZES[::-1])
    assert torch.equal(back[:SIZES[-1]], alone[-1][0]) and torch.equal(back[-SIZES[0]:], alone[0][0])


def test_predict_clouds_pads_a_small_cloud_and_drops_the_padding(net, synth, clouds, alone):
    small = _cloud(synth, 400, SMALL, cols=10)                                        # on the CPU, with a tenth column: both are accepted
    out = net.predict_clouds([small] + clouds)
    assert [tuple(p.shape) for p in out] == [(SMALL,)] + [(n,) for n in SIZES] and all(p.dtype == torch.int64 and p.is_cuda for p in out)
    padded = small[torch.arange(net.sa1.npoint) % SMALL, :9].cuda()[None].contiguous()
    assert torch.equal(out[0], net.predict_rows(padded)[0, :SMALL])
    for b in range(len(SIZES)):
        assert torch.equal(out[1 + b], alone[b][1]), b
    assert net.predict_clouds([]) == []


def test_refusals(net, clouds):
    L = sub("_lib")
    rows = torch.cat(clouds).contiguous()
    net.train()
    try:
        for call in (lambda: net.forward_ragged(rows, SIZES), lambda: net.predict_ragged(rows, SIZES), lambda: net.predict_clouds(clouds)):
            with pytest.raises(NotImplementedError, match="eval"):
                call()
    finally:
        net.eval()
    small = rows[:SMALL + 128].contiguous()
    with pytest.raises(L.AmpnetError, match="at least sa1.npoint=128 points, cloud 0 has 90"):
        net.forward_ragged(small, [SMALL, 128])
    with pytest.raises(L.AmpnetError, match="do not tile"):
        net.forward_ragged(rows, SIZES[:-1])
    with pytest.raises(L.AmpnetError, match="packed rows"):
        net.forward_ragged(rows[None], SIZES)
    with pytest.raises(L.AmpnetError, match="must live on the GPU"):
        net.forward_ragged(rows.cpu(), SIZES)


@pytest.fixture(scope="module")
def files(synth):
    """Three files of clusters [n_i, 10] on the CPU, as the cluster files hold them; the first has a cluster below sa1.npoint and two of
    equal size (which pn2_train.segment_file puts into one call)."""
    sizes = ([SMALL, 200, 131, 200], [128, 511], [300])
    return [[_cloud(synth, 500 + 10 * f + i, n, cols=10) for i, n in enumerate(s)] for f, s in enumerate(sizes)]


def test_the_driver_equals_pn2_train_segment_file_and_files_do_not_reach_each_other(net, files):
    """The seeded state answers class 1 for every point, which would make equal predictions a weak statement: for this test conv2's bias is
    moved by the mean log-probabilities of one cluster, so that the arg-max follows the point (asserted), and put back afterwards."""
    I, T = sub("pointNet.pn2_infer"), sub("pointNet.pn2_train")
    bias = net.conv2.bias.detach().clone()
    with torch.no_grad():
        net.conv2.bias.sub_(net.forward_rows(files[1][1][None, :, :9].cuda().contiguous())[0].mean(0))
    try:
        per_file = []
        for cl in files:
            want_p, want_t = T.segment_file(net, cl, "cuda")
            got_p, got_t = I.segment_file(net, cl, "cuda")
            assert not got_p.is_cuda and got_p.dtype == torch.int64 and got_t.dtype == torch.int64
            assert torch.equal(got_p, want_p) and torch.equal(got_t, want_t)
            dev_p, dev_t = I.segment_file(net, cl, "cuda", device_outputs=True)
            assert dev_p.is_cuda and dev_t.is_cuda and torch.equal(dev_p.cpu(), want_p) and torch.equal(dev_t.cpu(), want_t)
            per_file.append((want_p, want_t))
        assert all(len(set(p.tolist())) >= 3 for p, _ in per_file)                    # the predictions follow the point
        assert len(set(per_file[0][1].tolist())) == 5                                 # every label occurs: the table is exercised
        together = I.segment_files(net, files, "cuda")
        assert len(together) == 3
        for (p, t), (want_p, want_t) in zip(together, per_file):
            assert torch.equal(p, want_p) and torch.equal(t, want_t)
        on_dev = I.segment_files(net, files, "cuda", device_outputs=True)
        assert all(p.is_cuda and torch.equal(p.cpu(), w[0]) and torch.equal(t.cpu(), w[1]) for (p, t), w in zip(on_dev, per_file))
        assert I.segment_files(net, [], "cuda") == []
    finally:
        with torch.no_grad():
            net.conv2.bias.copy_(bias)
