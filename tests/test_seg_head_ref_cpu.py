"""The yardstick of the fused segmentation head, checked without a GPU: tests/seg_head_ref.py against torch's float64 composition, a float32
numpy composition against its bars, the conditions its seeds have to meet, and the host side of the feature -- the C symbols, their refusals
(every one happens on the host before any launch, so bogus non-null pointers are never followed), the constructors' limits and the
state_dict keys."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import seg_head_ref as R                           # noqa: E402

AMPNET_E_ARG = -1


def _case(name):
    return R.reference(sub("synthetic"), name)


def _torch_head(params, eps, dtype):
    W1, b1, gamma, beta, mean, var, W2, b2 = (torch.from_numpy(np.ascontiguousarray(p)).to(dtype) for p in params)
    conv1 = torch.nn.Conv1d(W1.shape[1], W1.shape[0], 1).to(dtype)
    bn1 = torch.nn.BatchNorm1d(W1.shape[0], eps=float(np.float32(eps))).to(dtype).eval()
    conv2 = torch.nn.Conv1d(W2.shape[1], W2.shape[0], 1).to(dtype)
    with torch.no_grad():
        conv1.weight.copy_(W1[:, :, None]), conv1.bias.copy_(b1), bn1.weight.copy_(gamma), bn1.bias.copy_(beta)
        bn1.running_mean.copy_(mean), bn1.running_var.copy_(var), conv2.weight.copy_(W2[:, :, None]), conv2.bias.copy_(b2)
    return conv1, bn1, conv2


@pytest.mark.parametrize("name", R.NAMES)
def test_reference_equals_torch_float64(name):
    """Conv1d, BatchNorm1d.eval(), ReLU, Conv1d, log_softmax in float64 with autograd for the backward: 1e-12 of each output's scale."""
    i, want, fwd = _case(name)
    conv1, bn1, conv2 = _torch_head(i["params"], i["eps"], torch.float64)
    x = torch.from_numpy(i["x"]).double().t()[None].contiguous().requires_grad_(True)       # [1, cin, M]
    logp = torch.log_softmax(conv2(torch.relu(bn1(conv1(x)))), dim=1).permute(0, 2, 1)     # [1, M, C]
    logp.backward(torch.from_numpy(i["dlogp"]).double()[None])
    got = dict(logp=logp[0], dx=x.grad[0].t(), dW1=conv1.weight.grad[:, :, 0], db1=conv1.bias.grad, dgamma=bn1.weight.grad,
               dbeta=bn1.bias.grad, dW2=conv2.weight.grad[:, :, 0], db2=conv2.bias.grad)
    for k, t in got.items():
        v = fwd["logp"][0] if k == "logp" else want[k][0]
        err = float(np.abs(t.detach().numpy() - v).max())
        assert err <= 1e-12 * max(1.0, float(np.abs(v).max())), (name, k, err)
    # the float64 numpy composition says the same: compose() is a restatement too
    c64 = R.compose(i["x"], i["params"], i["eps"], i["dlogp"], np.float64)
    for k in ("logp",) + R.OUTPUTS:
        v = fwd["logp"][0] if k == "logp" else want[k][0]
        assert float(np.abs(c64[k] - v).max()) <= 1e-12 * max(1.0, float(np.abs(v).max())), (name, k)


@pytest.mark.parametrize("name", R.NAMES)
def test_float32_numpy_stays_inside_every_bar(name):
    i, want, fwd = _case(name)
    c32 = R.compose(i["x"], i["params"], i["eps"], i["dlogp"], np.float32)
    ratios = {}
    for k in ("logp",) + R.OUTPUTS:
        v, bar = fwd["logp"] if k == "logp" else want[k]
        assert c32[k].dtype == np.float32 and c32[k].shape == v.shape, (name, k)
        assert (bar > 0).all() or k != "logp", (name, k)
        ratios[k] = float((np.abs(c32[k].astype(np.float64) - v) / np.maximum(bar, 1e-300)).max())
    print(f"seg_head float32 numpy {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", R.NAMES)
def test_seeds_keep_the_relu_margin_and_the_pred_condition(name):
    """Conditions on the seeded cases, met by the reference alone: every conv1 pre-activation RELU_MARGIN bars away from zero, and at most
    1 % of a case's rows left out of the pred comparison."""
    i, _, fwd = _case(name)
    assert fwd["worst"] > R.RELU_MARGIN, (name, fwd["worst"])
    keep = R.admitted(fwd, i["params"])
    share = 1.0 - float(keep.mean())
    print(f"seg_head {name}: smallest |y| / bar {fwd['worst']:.1f}, rows left out of the pred check {share:.4%} ({int((~keep).sum())} of {len(keep)})")
    assert share <= R.MAX_LEFT_OUT, (name, share)
    # on the admitted rows a float32 evaluation ranks the classes as the reference does (classes that duplicate a lower one count as it)
    c32 = R.compose(i["x"], i["params"], i["eps"], i["dlogp"], np.float32)
    canon = np.arange(len(i["params"][7]))
    for c in R.duplicates(i["params"]):
        canon[c] = next(j for j in range(c) if (i["params"][6][c] == i["params"][6][j]).all())
    assert np.array_equal(canon[c32["pred"][keep]], fwd["pred"][keep]), name
    if name == "ties":
        z = fwd["z"][0]
        assert R.duplicates(i["params"]) == [1] and (z[:, 0] == z[:, 1]).all()
        tied_on_top = z[:, 0] == z.max(1)
        assert tied_on_top.sum() >= 8 and (fwd["pred"][tied_on_top] == 0).all()             # the case does exercise the rule
    if name == "negative_gamma":
        gamma = i["params"][2]
        assert (gamma < 0).any() and (gamma > 0).any() and (gamma == 0).sum() == 1


def test_symbols_exist_and_the_abi_is_17():
    lib = sub("_lib").lib()
    assert lib.ampnet_abi_version() == 18      # the symbols arrived within ABI 17; the baseline probe made it 18
    for s in ("ampnet_seg_head_forward_f32", "ampnet_seg_head_forward_workspace_bytes", "ampnet_seg_head_backward_f32",
              "ampnet_seg_head_backward_workspace_bytes"):
        assert hasattr(lib, s), s


# ---- the host refusals of the C ABI ------------------------------------------------------------------------------------------------------
_BOGUS = ctypes.create_string_buffer(64)           # a non-null address nobody follows: every refusal comes before any launch


def _c_call(L, backward, **over):
    """One call of the C entry point with valid arguments but for `over`; -> (return code, ampnet_last_error)."""
    lib = L.lib()
    p = ctypes.cast(_BOGUS, ctypes.c_void_p)
    a = dict(x=p, ld=16, M=70, cin=16, hidden=64, n_classes=5, params=[p.value] * 8, eps=1e-5, out=p, opt=p, grads=[p.value] * 6, ws=p,
             ws_bytes=None)
    a.update(over)
    size = lib.ampnet_seg_head_backward_workspace_bytes if backward else lib.ampnet_seg_head_forward_workspace_bytes
    size.restype = ctypes.c_size_t
    if a["ws_bytes"] is None:
        a["ws_bytes"] = size(16, 64, 5, ctypes.c_longlong(70))
        assert a["ws_bytes"] > 0
    table = None if a["params"] is None else (ctypes.c_void_p * 8)(*a["params"])
    head = (a["x"], a["ld"], ctypes.c_longlong(a["M"]), a["cin"], a["hidden"], a["n_classes"], table, ctypes.c_float(a["eps"]), a["out"], a["opt"])
    tail = (a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
    if backward:
        gtable = None if a["grads"] is None else (ctypes.c_void_p * 6)(*a["grads"])
        rc = lib.ampnet_seg_head_backward_f32(*head, gtable, *tail)
    else:
        rc = lib.ampnet_seg_head_forward_f32(*head, *tail)
    return rc, (lib.ampnet_last_error() or b"").decode()


REFUSALS = [("x", dict(x=None), "null pointer"), ("params", dict(params=None), "null pointer"),
            ("a parameter", dict(params=[1] * 6 + [0, 1]), "null parameter 6"), ("out", dict(out=None), "null pointer"),
            ("workspace", dict(ws=None), "workspace"), ("short workspace", dict(ws_bytes=63), "workspace"),
            ("cin 0", dict(cin=0, ld=16), "cin=0"), ("cin 257", dict(cin=257, ld=257), "cin=257"), ("ld < cin", dict(ld=15), "ld=15"),
            ("hidden 0", dict(hidden=0), "hidden=0"), ("hidden 48", dict(hidden=48), "hidden=48"), ("hidden 288", dict(hidden=288), "hidden=288"),
            ("one class", dict(n_classes=1), "n_classes=1"), ("33 classes", dict(n_classes=33), "n_classes=33"),
            ("no rows", dict(M=0), "M=0"), ("too many rows", dict(M=0x7fff0000 * 32 + 1), "rows")]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("what,over,says", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_without_a_gpu(backward, what, over, says):
    L = sub("_lib")
    rc, msg = _c_call(L, backward, **over)
    name = "ampnet_seg_head_backward_f32" if backward else "ampnet_seg_head_forward_f32"
    assert rc == AMPNET_E_ARG and msg.startswith(name) and says in msg, (what, rc, msg)


def test_backward_refuses_its_own_null_pointers():
    L = sub("_lib")
    for over, says in ((dict(grads=None), "null pointer"), (dict(grads=[1, 1, 0, 1, 1, 1]), "null gradient pointer 2"),
                       (dict(grads=[1, 1, 1, 1, 1, 0]), "dW2, db2")):
        rc, msg = _c_call(L, True, **over)
        assert rc == AMPNET_E_ARG and says in msg, (over, msg)


def test_workspace_bytes_answer_on_the_host():
    L = sub("_lib")
    assert L.seg_head_forward_workspace_bytes(128, 128, 5, 70) == 256 * 4
    small, large = L.seg_head_backward_workspace_bytes(128, 128, 5, 70), L.seg_head_backward_workspace_bytes(128, 128, 5, 32768)
    assert 0 < small < large
    assert L.seg_head_backward_workspace_bytes(256, 256, 32, 1) > 0 and L.seg_head_backward_workspace_bytes(1, 32, 2, 0x7fff0000 * 32) > 0
    for bad, says in (((257, 128, 5, 70), "cin=257"), ((128, 96 + 16, 5, 70), "multiple of 32"), ((128, 128, 33, 70), "n_classes=33"),
                      ((128, 128, 5, 0), "M=0")):
        for fn in (L.seg_head_forward_workspace_bytes, L.seg_head_backward_workspace_bytes):
            with pytest.raises(L.AmpnetError, match=says):
                fn(*bad)


@pytest.mark.parametrize("name", ["seg_head_forward", "seg_head_backward"])
def test_wrappers_name_themselves_and_the_argument(name):
    """CPU tensors and a missing tensor are AmpnetErrors that open with the wrapper's name, as for the other PointNet++ wrappers."""
    L = sub("_lib")
    i, _, _ = _case("negative_gamma")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = dict(x=t(i["x"]), params=[t(p) for p in i["params"]], eps=i["eps"], workspace=torch.zeros(64, dtype=torch.uint8))
    if name == "seg_head_forward":
        args.update(logp=torch.zeros(70, 5), preds=None)
    else:
        args.update(dlogp=t(i["dlogp"]), dx=None, grads=[torch.zeros_like(t(i["params"][q])) for q in (0, 1, 1, 1, 6, 7)])
    with pytest.raises(L.AmpnetError, match=f"^{name}: x must be .*GPU"):
        getattr(L, name + "_f32")(**args)
    with pytest.raises(L.AmpnetError, match=f"^{name}: x is None"):
        getattr(L, name + "_f32")(**dict(args, x=None))


# ---- the modules -------------------------------------------------------------------------------------------------------------------------
def test_constructor_refuses_what_is_outside_the_limits():
    U = sub("pointNet.model.pointnet2_utils")
    U.PointNetSegHead(256, 256, 32, device="cpu")
    U.PointNetSegHead(1, 32, 2, device="cpu")
    for bad in ((0, 128, 5), (257, 128, 5), (128, 0, 5), (128, 48, 5), (128, 288, 5), (128, 128, 1), (128, 128, 33)):
        with pytest.raises(NotImplementedError, match="segmentation head is built for"):
            U.PointNetSegHead(*bad, device="cpu")
    with pytest.raises(TypeError):
        U.PointNetSegHead(128, 128, 5, device="cpu", precision="bf16")             # the head is fp32: there is no such keyword


def _torch_seg_head(cin, hidden, classes):
    m = torch.nn.Module()
    m.conv1, m.bn1, m.drop1, m.conv2 = (torch.nn.Conv1d(cin, hidden, 1), torch.nn.BatchNorm1d(hidden), torch.nn.Dropout(0.5),
                                        torch.nn.Conv1d(hidden, classes, 1))
    return m


def test_state_dict_keys_and_shapes_are_a_torch_heads():
    U = sub("pointNet.model.pointnet2_utils")
    ours, theirs = U.PointNetSegHead(128, 128, 5, device="cpu"), _torch_seg_head(128, 128, 5)
    a, b = ours.state_dict(), theirs.state_dict()
    assert list(a) == list(b)
    assert {k: (tuple(v.shape), v.dtype) for k, v in a.items()} == {k: (tuple(v.shape), v.dtype) for k, v in b.items()}
    ours.load_state_dict(b, strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    assert all(torch.equal(ours.state_dict()[k], theirs.state_dict()[k]) for k in a)


def test_pointnet_2_seg_keys_are_the_references_with_its_lines_restored():
    A = sub("pointNet.model.pointnetAtt")
    seg, backbone = A.pointnet_2_seg(5, device="cpu"), A.pointnet_2(5, device="cpu")
    keys, base = list(seg.state_dict()), list(backbone.state_dict())
    head = [k for k in keys if k.split(".")[0] in ("conv1", "bn1", "conv2")]
    assert [k for k in keys if k not in head] == [k for k in base if not k.startswith("conv1.")]
    assert sorted(head) == sorted(["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"]
                                  + ["bn1." + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")])
    assert {k.split(".")[0] for k in keys} == {"sa1", "sa2", "sa3", "fp3", "fp2", "fp1", "conv1", "bn1", "conv2"}
    assert tuple(seg.state_dict()["conv1.weight"].shape) == (128, 128, 1) and tuple(seg.state_dict()["conv2.weight"].shape) == (5, 128, 1)
    res = seg.load_state_dict(backbone.state_dict(), strict=False)
    assert not res.unexpected_keys and sorted({k.split(".")[0] for k in res.missing_keys}) == ["bn1", "conv2"]
    assert torch.equal(seg.conv1.weight, backbone.conv1.weight)
    # the flag rules are pointnet_2's; the head stays in eval mode whatever the model's mode is
    with pytest.raises(ValueError):
        A.pointnet_2_seg(5, device="cpu", encoder_grad=True)
    trainable = A.pointnet_2_seg(5, device="cpu", decoder_grad=True, decoder_batch_stats=True)
    trainable.train()
    assert trainable.training and trainable.fp1.training and not trainable.sa1.training
    assert not trainable._head.training and not trainable.bn1.training and not trainable.drop1.training
    with pytest.raises(NotImplementedError):
        seg.set_precision("bf16")
