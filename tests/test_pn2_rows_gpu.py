"""pointnet_2_seg.forward_rows / predict_rows on the GPU: the model on point-major [Q, N, 9] rows gives the bits of forward / predict on
[Q, 9, N] -- in eval mode and, with all five flags, in train mode (log-probabilities, every gradient, every running statistic) -- and
forward() itself still gives the bits of the blocks composed one by one through their public, channel-major forwards.  The reduced model
of tests/pn2_finetune_util.py (128 / 32 / 8 centres, B = 2, N = 512)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_finetune_util as PU                     # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True, head_batch_stats=True)


def _seg_model(**kwargs):
    """pointnet_2_seg(5) in eval mode at the reduced sizes of pn2_finetune_util.model, seeded."""
    A = sub("pointNet.model.pointnetAtt")
    net = A.pointnet_2_seg(5, **kwargs).eval()
    for sa, npoint, radius in ((net.sa1, 128, 0.2), (net.sa2, 32, 0.4), (net.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    PU.randomise(net, 8)
    return net


def _rows(x):
    return x.transpose(1, 2).contiguous()                            # [B, N, 9]


def test_eval_rows_equal_forward_and_predict_bit_for_bit(synth):
    x = PU.model_input(synth)
    seg = _seg_model()
    log_probs, l0 = seg(x)
    rows = seg.forward_rows(_rows(x))
    assert rows.shape == (PU.B, PU.N, 5) and not rows.requires_grad and torch.equal(rows, log_probs)
    pred = seg.predict_rows(_rows(x))
    assert pred.dtype == torch.int64 and pred.shape == (PU.B, PU.N) and torch.equal(pred, seg.predict(x))
    # with a graph (eval mode, frozen statistics): the same bits, and a graph
    tuned = _seg_model(decoder_grad=True, encoder_grad=True)
    out = tuned.forward_rows(_rows(x))
    assert out.requires_grad and torch.equal(out.detach(), log_probs)
    with torch.no_grad():
        assert not tuned.forward_rows(_rows(x)).requires_grad
    # the input's contract: point-major, float32, contiguous, on the GPU
    L = sub("_lib")
    for bad in (x, _rows(x).double(), _rows(x)[:, ::2], _rows(x)[:, :, :8]):
        with pytest.raises(L.AmpnetError, match="point-major rows"):
            seg.forward_rows(bad)
    with pytest.raises(L.AmpnetError, match="must live on the GPU"):
        seg.forward_rows(_rows(x).cpu())
    with pytest.raises(NotImplementedError, match="eval mode"):
        seg.train().forward_rows(_rows(x))                           # the mode checks are forward()'s
    with pytest.raises(NotImplementedError):
        _seg_model(**FLAGS).train().predict_rows(_rows(x))           # an eval operation


def test_forward_still_equals_the_blocks_composed_one_by_one(synth):
    x = PU.model_input(synth)
    seg = _seg_model()
    l0_xyz = x[:, :3].contiguous()
    l1_xyz, l1_points = seg.sa1(l0_xyz, x)
    l2_xyz, l2_points = seg.sa2(l1_xyz, l1_points)
    l3_xyz, l3_points = seg.sa3(l2_xyz, l2_points)
    l2_points = seg.fp3(l2_xyz, l3_xyz, l2_points, l3_points)
    l1_points = seg.fp2(l1_xyz, l2_xyz, l1_points, l2_points)
    l0 = seg.fp1(l0_xyz, l1_xyz, None, l1_points)
    log_probs, l0_points = seg(x)
    assert torch.equal(l0_points, l0) and torch.equal(log_probs, seg._head(l0))
    backbone = PU.model(state={k: v for k, v in seg.state_dict().items() if k.split(".")[0] not in ("bn1", "conv2")})
    assert torch.equal(backbone(x)[1], l0)                           # pointnet_2 shares _backbone: its bits have not moved either


def test_train_mode_rows_equal_forward_in_outputs_gradients_and_statistics(synth):
    x = PU.model_input(synth)
    target = torch.from_numpy(synth.randint(78, (PU.B * PU.N,), 0, 5)).cuda()
    one, two = _seg_model(**FLAGS), _seg_model(**FLAGS)
    assert one._head.seed == two._head.seed and one._head._step == two._head._step == 0
    one.train(), two.train()
    a, l0 = one(x)
    b = two.forward_rows(_rows(x))
    assert a.requires_grad and b.requires_grad and l0 is not None
    assert torch.equal(a.detach(), b.detach())
    F.nll_loss(a.reshape(-1, 5), target).backward()
    F.nll_loss(b.reshape(-1, 5), target).backward()
    grads = dict(two.named_parameters())
    for k, p in one.named_parameters():
        assert p.grad is not None and grads[k].grad is not None and torch.equal(p.grad, grads[k].grad), k
    buffers = dict(two.named_buffers())
    fresh = dict(_seg_model(**FLAGS).named_buffers())
    for k, v in one.named_buffers():
        assert torch.equal(v, buffers[k]), k
        assert not torch.equal(v, fresh[k]), k                       # (and every one of them did move: statistics and counters)
    assert int(one.bn1.num_batches_tracked) == int(two.bn1.num_batches_tracked) == 4
    assert one._head._step == two._head._step == 1
    # a second step from the same state: still the same bits (the dropout step advanced alike)
    assert torch.equal(one(x)[0].detach(), two.forward_rows(_rows(x)).detach())
