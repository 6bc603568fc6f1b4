"""ClassificationWithAttention on the HIP path (pointNet/model/pointnetAtt.py:115-151) against the reference module's own
outputs and autograd gradients (tests/golden/cls.npz, made by tests/golden/make_golden.py:sec_cls).  Bars: outputs / attention weights
1e-4; gradients 5e-3 of each tensor's norm against the reference's fp32 autograd (BatchNorm over B = 16 rows)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu


def _net(synth, params, g, dropout=0.0):
    Wn, B, C = [int(v) for v in g["meta"]]
    M = sub("pointNet.model.pointnetAtt")
    net = M.ClassificationWithAttention(256, 8, num_classes=C, dropout=dropout, num_w=Wn, device="cuda")
    table = params.cls_head_params(C, Wn)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(9, table).items()}
    sd.update({k: torch.from_numpy(v) for k, v in synth.make_buffers(9, params.CLS_HEAD_BUFFERS).items()})
    r = net.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and all(k.endswith("num_batches_tracked") for k in r.missing_keys)
    assert list(dict(net.named_parameters()).keys()) == list(table.keys())
    gl = torch.from_numpy(synth.uniform(91, (Wn, B, 256), 0.0, 2.0)).cuda()
    mask = torch.zeros(B, Wn, dtype=torch.bool)
    mask[1, 3:] = True
    mask[7, 4] = True
    return net, gl, mask.cuda(), (Wn, B, C)


def test_cls_head_eval_matches_reference(golden, synth, params):
    g = golden("cls")
    net, gl, mask, _ = _net(synth, params, g)
    net.eval()
    with torch.no_grad():
        out, aw = net(gl, None, mask)
    np.testing.assert_allclose(out.cpu().numpy(), g["eval_out"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(aw.cpu().numpy(), g["eval_weights"], rtol=1e-4, atol=1e-6)
    with pytest.raises(Exception):
        net(gl.cpu(), None, None)


def test_cls_head_train_step_matches_reference(golden, synth, params):
    g = golden("cls")
    net, gl, mask, (Wn, B, C) = _net(synth, params, g)
    net.train()
    glg = gl.clone().requires_grad_(True)
    out, aw = net(glg, None, mask)
    tgt = torch.from_numpy(synth.randint(92, (B,), 0, C)).cuda()
    loss = torch.nn.functional.cross_entropy(out, tgt)
    loss.backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["train_out"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(aw.cpu().numpy(), g["train_weights"], rtol=1e-4, atol=1e-6)
    assert abs(loss.item() - g["loss"].item()) <= 1e-4 * abs(g["loss"].item())
    ref = g["d_gl"].astype(np.float64)                       # [W, B, 256]
    got = glg.grad.double().cpu().numpy()
    assert np.linalg.norm(got - ref) <= 5e-3 * np.linalg.norm(ref)
    worst = 0.0
    gtot = np.sqrt(sum(float((g[f"grad/{k}"].astype(np.float64) ** 2).sum()) for k, _ in net.named_parameters()))
    for k, p in net.named_parameters():                      # fc_2.bias (in front of bn_2) has an analytically zero gradient
        ref = g[f"grad/{k}"].astype(np.float64)
        err = np.linalg.norm(p.grad.double().cpu().numpy().reshape(ref.shape) - ref)
        worst = max(worst, err / (np.linalg.norm(ref) + 1e-3 * gtot))
        assert err <= 5e-3 * np.linalg.norm(ref) + 1e-5 * gtot, (k, err, np.linalg.norm(ref), gtot)
    print(f"classification head: worst relative gradient error vs the reference's autograd {worst:.2e}")
    sd = net.state_dict()
    for k in sd:
        if "running" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), g[f"buf/{k}"], rtol=1e-4, atol=1e-5, err_msg=k)
    assert int(net.bn_2.num_batches_tracked) == 1


def test_cls_head_dropout_matches_oracle_masks(golden, synth, params):
    """Attention dropout 0.3: the HIP forward / backward equal the oracle evaluated with the same keep-mask."""
    from oracle import ampnet_oracle as O
    from helpers import torch_params
    g = golden("cls")
    net, gl, mask, (Wn, B, C) = _net(synth, params, g, dropout=0.3)
    net.train()
    seed = net.seed
    glg = gl.clone().requires_grad_(True)
    out, aw = net(glg, None, mask)
    tgt = torch.from_numpy(synth.randint(92, (B,), 0, C)).cuda()
    torch.nn.functional.cross_entropy(out, tgt).backward()
    keep = torch.from_numpy(O.keep_mask(seed, 0, B * 8 * Wn * Wn, 0.3)).double().reshape(B * 8, Wn, Wn)
    p = {k: v.double().requires_grad_(True) for k, v in torch_params(synth.make_params(9, params.cls_head_params(C, Wn))).items()}
    b = {k: v.double() for k, v in torch_params(synth.make_buffers(9, params.CLS_HEAD_BUFFERS)).items()}
    gl64 = gl.double().cpu().requires_grad_(True)
    o64, a64 = O.cls_head(p, b, gl64, mask.cpu(), True, drop_p=0.3, drop_mask=keep)
    torch.nn.functional.cross_entropy(o64, tgt.cpu()).backward()
    assert (out.detach().double().cpu() - o64.detach()).abs().max().item() <= 1e-4
    assert (aw.double().cpu() - a64.detach()).abs().max().item() <= 1e-5
    gtot64 = float(np.sqrt(sum(float(v.grad.pow(2).sum()) for v in p.values())))
    for k, v in net.named_parameters():
        ref = p[k].grad
        assert float((v.grad.double().cpu().reshape(ref.shape) - ref).norm()) <= 5e-3 * float(ref.norm()) + 1e-5 * gtot64, k
    assert float((glg.grad.double().cpu() - gl64.grad).norm()) <= 5e-3 * float(gl64.grad.norm())


def _cls_oracle(O, table_p, table_b, gl, mask, tgt, dt, train, relu_shift=0.0):
    """(out, attention weights, parameter gradients, d gl, running statistics) of O.cls_head evaluated in dt, as float64 tensors; relu_shift
    moves every BatchNorm output by that amount before its ReLU (what an activation switching side of the kink costs)."""
    orig = O.batchnorm_rows
    if relu_shift:
        O.batchnorm_rows = lambda *a, **k: orig(*a, **k) + relu_shift
    try:
        p = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in table_p.items()}
        b = {k: v.to(dt).clone() for k, v in table_b.items()}
        g = gl.detach().to(dt).clone().requires_grad_(True)
        out, aw = O.cls_head(p, b, g, mask, train)
        if not train:
            return out.detach().double(), aw.detach().double(), None, None, None
        torch.nn.functional.cross_entropy(out, tgt).backward()
        return out.detach().double(), aw.detach().double(), {k: v.grad.double() for k, v in p.items()}, g.grad.double(), {k: v.double() for k, v in b.items()}
    finally:
        O.batchnorm_rows = orig


@pytest.mark.parametrize("B,W,C", [(2, 1, 2), (3, 2, 5), (4, 6, 16), (7, 5, 5), (5, 32, 8)])
def test_cls_head_edge_shapes_match_oracle(synth, params, B, W, C):
    """B < W, B not coprime to W, W = 1 and W = 32, C = 2 .. 16 through the module, against the float64 oracle, in eval mode and in train mode
    with backward; a key-padding mask that leaves sample 0 a single valid key (no sample fully masked: the reference defines nothing there).
    Yardstick of every tensor: 3 x the oracle's own fp32-vs-float64 difference + 2e-4 of its norm (gradients: + 1e-5 of the oracle's total
    gradient norm + 1.5 x the ReLU-kink allowance); running statistics: 3 x that difference + 1e-5 of the tensor's norm."""
    from oracle import ampnet_oracle as O
    from helpers import torch_params
    M = sub("pointNet.model.pointnetAtt")
    net = M.ClassificationWithAttention(256, 8, num_classes=C, dropout=0.0, num_w=W, device="cuda")
    tp = torch_params(synth.make_params(9, params.cls_head_params(C, W)))
    tb = torch_params(synth.make_buffers(9, params.CLS_HEAD_BUFFERS))
    r = net.load_state_dict({**tp, **tb}, strict=False)
    assert not r.unexpected_keys and all(k.endswith("num_batches_tracked") for k in r.missing_keys)
    gl = torch.from_numpy(synth.uniform(95, (W, B, 256), 0.0, 2.0))
    mask = torch.zeros(B, W, dtype=torch.bool)
    mask[0, 1:] = True
    if W > 1:
        mask[B - 1, W - 1] = True
    assert not mask.all(1).any()
    tgt = torch.from_numpy(synth.randint(96, (B,), 0, C))

    def held(got, w64, w32, extra, what):
        err = float((got.double().cpu().reshape(w64.shape) - w64).norm())
        allowed = 3.0 * float((w32 - w64).norm()) + 2e-4 * float(w64.norm()) + extra
        assert err <= allowed, (what, err, allowed, float(w64.norm()))
        return err / allowed

    net.eval()
    with torch.no_grad():
        out, aw = net(gl.cuda(), None, mask.cuda())
    o64, a64, _, _, _ = _cls_oracle(O, tp, tb, gl, mask, tgt, torch.float64, False)
    o32, a32, _, _, _ = _cls_oracle(O, tp, tb, gl, mask, tgt, torch.float32, False)
    assert out.shape == (B, C) and aw.shape == (B, W, W)
    held(out, o64, o32, 0.0, "eval out")
    held(aw, a64, a32, 0.0, "eval weights")
    assert not aw.cpu()[mask.reshape(B, 1, W).expand(B, W, W)].any(), "masked keys get weight exactly 0"

    net.train()
    glg = gl.cuda().requires_grad_(True)
    out, aw = net(glg, None, mask.cuda())
    torch.nn.functional.cross_entropy(out, tgt.cuda()).backward()
    o64, a64, w64, g64, b64 = _cls_oracle(O, tp, tb, gl, mask, tgt, torch.float64, True)
    o32, a32, w32, g32, b32 = _cls_oracle(O, tp, tb, gl, mask, tgt, torch.float32, True)
    kink = {k: 0.0 for k in w64}
    kink_gl, kink_out = 0.0, 0.0
    for sft in (1e-5, -1e-5):
        os_, _, ws, gs, _ = _cls_oracle(O, tp, tb, gl, mask, tgt, torch.float64, True, relu_shift=sft)
        kink_gl, kink_out = max(kink_gl, float((gs - g64).norm())), max(kink_out, float((os_ - o64).norm()))
        for k in w64:
            kink[k] = max(kink[k], float((ws[k] - w64[k]).norm()))
    gtot = float(np.sqrt(sum(float(w.pow(2).sum()) for w in w64.values())))
    held(out.detach(), o64, o32, 1.5 * kink_out, "train out")
    held(aw, a64, a32, 0.0, "train weights")
    worst = held(glg.grad, g64, g32, 1e-5 * gtot + 1.5 * kink_gl, "d gl")
    assert len(w64) == 12
    for k, p in net.named_parameters():
        worst = max(worst, held(p.grad, w64[k], w32[k], 1e-5 * gtot + 1.5 * kink[k], k))
    print(f"classification head edge shapes B={B} W={W} C={C}: worst gradient error / allowance {worst:.3f}")
    sd = net.state_dict()
    for k in b64:
        err = float((sd[k].double().cpu() - b64[k]).norm())
        assert err <= 3.0 * float((b32[k] - b64[k]).norm()) + 1e-5 * float(b64[k].norm()), (k, err)
    assert int(net.bn_2.num_batches_tracked) == 1
