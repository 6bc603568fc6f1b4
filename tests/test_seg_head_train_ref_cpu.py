"""The yardstick of the train-mode segmentation head, checked without a GPU: tests/seg_head_train_ref.py against torch's float64
composition (Conv1d, BatchNorm1d.train(), ReLU, the mask, Conv1d, log_softmax), a float32 numpy composition against its bars, the
conditions its seeds have to meet, the numpy keep mask against the oracle's, and the host side of the feature -- the four C symbols, their
refusals (every one happens on the host before any launch, so bogus non-null pointers are never followed) and the constructors' rules."""
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
from oracle import ampnet_oracle as O              # noqa: E402
import seg_head_train_ref as R                     # noqa: E402

AMPNET_E_ARG = -1
ALL = R.FORWARD + R.BACKWARD


def _case(name):
    return R.reference(sub("synthetic"), name)


@pytest.mark.parametrize("name", R.NAMES)
def test_reference_equals_torch_float64(name):
    """1e-12 of each output's scale, the running statistics included."""
    i, want, _ = _case(name)
    W1, b1, gamma, beta, rmean, rvar, W2, b2 = (torch.from_numpy(np.ascontiguousarray(p)).double() for p in i["params"])
    hidden, cin = W1.shape
    conv1 = torch.nn.Conv1d(cin, hidden, 1).double()
    bn1 = torch.nn.BatchNorm1d(hidden, eps=float(np.float32(i["eps"])), momentum=float(np.float32(R.MOMENTUM))).double().train()
    conv2 = torch.nn.Conv1d(hidden, W2.shape[0], 1).double()
    with torch.no_grad():
        conv1.weight.copy_(W1[:, :, None]), conv1.bias.copy_(b1), bn1.weight.copy_(gamma), bn1.bias.copy_(beta)
        bn1.running_mean.copy_(rmean), bn1.running_var.copy_(rvar), conv2.weight.copy_(W2[:, :, None]), conv2.bias.copy_(b2)
    M = i["x"].shape[0]
    mask = R.keep_mask(i["drop_seed"], M, hidden, i["p"]).astype(np.float64) * (R.drop_scale(i["p"]) if i["p"] else 1.0)
    x = torch.from_numpy(i["x"]).double().t()[None].contiguous().requires_grad_(True)       # [1, cin, M]
    pre = conv1(x)
    pre.retain_grad()
    h = torch.relu(bn1(pre)) * torch.from_numpy(mask).t()[None]
    logp = torch.log_softmax(conv2(h), dim=1).permute(0, 2, 1)                              # [1, M, C]
    logp.backward(torch.from_numpy(i["dlogp"]).double()[None])
    a = (pre[0] - b1[:, None]).detach()                                                     # the raw accumulator, [hidden, M]
    got = dict(logp=logp[0], save_mean=a.mean(1), save_invstd=1.0 / torch.sqrt(a.var(1, unbiased=False) + bn1.eps),
               running_mean=bn1.running_mean, running_var=bn1.running_var, dx=x.grad[0].t(), dW1=conv1.weight.grad[:, :, 0],
               db1=conv1.bias.grad, dgamma=bn1.weight.grad, dbeta=bn1.bias.grad, dW2=conv2.weight.grad[:, :, 0], db2=conv2.bias.grad)
    assert sorted(got) == sorted(want) == sorted(ALL)
    for k, t in got.items():
        v = want[k][0]
        err = float(np.abs(t.detach().numpy() - v).max())
        # (db1 is 0 here and a cancelling sum of the rows' dz1 in torch: the scale of ITS rounding is the sum of their magnitudes)
        scale = float(pre.grad.abs().sum(2).max()) if k == "db1" else float(np.abs(v).max())
        assert err <= 1e-12 * max(1.0, scale), (name, k, err)
    assert int(bn1.num_batches_tracked) == 1


@pytest.mark.parametrize("name", R.NAMES)
def test_float32_numpy_stays_inside_every_bar(name):
    i, want, _ = _case(name)
    c32 = R.compose(i["x"], i["params"], i["eps"], i["p"], i["drop_seed"], i["dlogp"], np.float32)
    ratios = {}
    for k in ALL:
        v, bar = want[k]
        assert c32[k].dtype == np.float32 and c32[k].shape == v.shape, (name, k)
        err = np.abs(c32[k].astype(np.float64) - v)
        ratios[k] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())
    print(f"seg_head_train float32 numpy {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", R.NAMES)
def test_seeds_keep_the_relu_margin(name):
    """A condition on the seeded cases, met by the reference alone; and the bars do pin the mask: one flipped keep bit leaves them."""
    i, want, worst = _case(name)
    print(f"seg_head_train {name}: smallest |y| / bar {worst:.1f}")
    assert worst > R.RELU_MARGIN, (name, worst)
    if name == "negative_gamma":
        gamma = i["params"][2]
        assert (gamma < 0).any() and (gamma > 0).any() and (gamma == 0).sum() == 1
    if name == "tail":
        M, hidden = i["x"].shape[0], i["params"][0].shape[0]
        keep = R.keep_mask(i["drop_seed"], M, hidden, i["p"])
        y_pos = R.forward_layer(i["x"].astype(np.float64), np.zeros(i["x"].shape), i["params"][:6], i["eps"])["y"] > 0
        r, c = np.argwhere(y_pos)[0]                                   # a live activation: its keep bit matters
        keep[r, c] = ~keep[r, c]
        flipped, _ = R.seg_train(i["x"], i["params"], i["eps"], i["p"], i["drop_seed"], i["dlogp"], keep=keep)
        v, bar = want["logp"]
        assert (np.abs(flipped["logp"][0][r] - v[r]) > 100.0 * bar[r]).any()


@pytest.mark.parametrize("name", R.NAMES)
def test_numpy_mask_is_the_oracles(name):
    _, M, _, hidden, _, p, _ = next(c for c in R.CASES if c[0] == name)
    seed = R.DROP_SEED + R.NAMES.index(name)
    keep = R.keep_mask(seed, M, hidden, p)
    assert np.array_equal(keep.reshape(-1), O.keep_mask(seed, 0, M * hidden, p))
    n = M * hidden
    sigma = np.sqrt(p * (1.0 - p) / n)
    assert abs(float(keep.mean()) - (1.0 - p)) <= 4.0 * sigma, (name, float(keep.mean()))
    assert R.drop_scale(0.5) == 2.0 and np.float32(R.drop_scale(0.3)) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))


def test_symbols_exist_within_abi_18():
    lib = sub("_lib").lib()
    assert lib.ampnet_abi_version() == 18
    for s in ("ampnet_seg_head_train_forward_f32", "ampnet_seg_head_train_forward_workspace_bytes", "ampnet_seg_head_train_backward_f32",
              "ampnet_seg_head_train_backward_workspace_bytes"):
        assert hasattr(lib, s), s


# ---- the host refusals of the C ABI ------------------------------------------------------------------------------------------------------
_BOGUS = ctypes.create_string_buffer(64)           # a non-null address nobody follows: every refusal comes before any launch


def _c_call(L, backward, **over):
    """One call of the C entry point with valid arguments but for `over`; -> (return code, ampnet_last_error)."""
    lib = L.lib()
    p = ctypes.cast(_BOGUS, ctypes.c_void_p)
    a = dict(x=p, ld=16, M=70, cin=16, hidden=64, n_classes=5, params=[p.value] * 8, eps=1e-5, momentum=0.1, drop_p=0.5, seed=7, out=p,
             save_mean=p, save_invstd=p, dx=p, grads=[p.value] * 6, ws=p, ws_bytes=None)
    a.update(over)
    size = lib.ampnet_seg_head_train_backward_workspace_bytes if backward else lib.ampnet_seg_head_train_forward_workspace_bytes
    size.restype = ctypes.c_size_t
    if a["ws_bytes"] is None:
        a["ws_bytes"] = size(16, 64, 5, ctypes.c_longlong(70))
        assert a["ws_bytes"] > 0
    table = None if a["params"] is None else (ctypes.c_void_p * 8)(*a["params"])
    head = (a["x"], a["ld"], ctypes.c_longlong(a["M"]), a["cin"], a["hidden"], a["n_classes"], table, ctypes.c_float(a["eps"]))
    drop = (ctypes.c_float(a["drop_p"]), ctypes.c_uint32(a["seed"]))
    tail = (a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
    if backward:
        gtable = None if a["grads"] is None else (ctypes.c_void_p * 6)(*a["grads"])
        rc = lib.ampnet_seg_head_train_backward_f32(*head, *drop, a["save_mean"], a["save_invstd"], a["out"], a["dx"], gtable, *tail)
    else:
        rc = lib.ampnet_seg_head_train_forward_f32(*head, ctypes.c_float(a["momentum"]), *drop, a["out"], a["save_mean"], a["save_invstd"], *tail)
    return rc, (lib.ampnet_last_error() or b"").decode()


# (`out` is logp in the forward and dlogp in the backward)
REFUSALS = [("x", dict(x=None), "null pointer"), ("params", dict(params=None), "null pointer"),
            ("a parameter", dict(params=[1] * 6 + [0, 1]), "null parameter 6"), ("out", dict(out=None), "null pointer"),
            ("save_mean", dict(save_mean=None), "save_mean"), ("save_invstd", dict(save_invstd=None), "save_invstd"),
            ("workspace", dict(ws=None), "workspace"), ("short workspace", dict(ws_bytes=63), "workspace"),
            # the eval head's limits
            ("cin 0", dict(cin=0, ld=16), "cin=0"), ("cin 257", dict(cin=257, ld=257), "cin=257"), ("ld < cin", dict(ld=15), "ld=15"),
            ("hidden 0", dict(hidden=0), "hidden=0"), ("hidden 48", dict(hidden=48), "hidden=48"), ("hidden 288", dict(hidden=288), "hidden=288"),
            ("one class", dict(n_classes=1), "n_classes=1"), ("33 classes", dict(n_classes=33), "n_classes=33"),
            ("no rows", dict(M=0), "M=0"),
            # the batch statistics' and the dropout's
            ("one row", dict(M=1), ">= 2 rows"), ("2^24 + 1 rows", dict(M=(1 << 24) + 1), "exceed 16777216"),
            ("drop_p 1", dict(drop_p=1.0), "drop_p=1"), ("drop_p < 0", dict(drop_p=-0.1), "drop_p=-0.1"),
            ("drop_p nan", dict(drop_p=float("nan")), "drop_p="), ("drop_p inf", dict(drop_p=float("inf")), "drop_p=")]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("what,over,says", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_without_a_gpu(backward, what, over, says):
    L = sub("_lib")
    rc, msg = _c_call(L, backward, **over)
    name = "ampnet_seg_head_train_backward_f32" if backward else "ampnet_seg_head_train_forward_f32"
    assert rc == AMPNET_E_ARG and msg.startswith(name) and says in msg, (what, rc, msg)


def test_each_entry_point_refuses_its_own_arguments():
    L = sub("_lib")
    for m in (-0.1, 1.5, float("nan")):
        rc, msg = _c_call(L, False, momentum=m)
        assert rc == AMPNET_E_ARG and msg.startswith("ampnet_seg_head_train_forward_f32") and "momentum" in msg, (m, msg)
    for over, says in ((dict(grads=None), "null pointer"), (dict(grads=[1, 1, 0, 1, 1, 1]), "null gradient pointer 2"),
                       (dict(grads=[1, 1, 1, 1, 1, 0]), "dW2, db2")):
        rc, msg = _c_call(L, True, **over)
        assert rc == AMPNET_E_ARG and msg.startswith("ampnet_seg_head_train_backward_f32") and says in msg, (over, msg)


def test_workspace_bytes_answer_on_the_host():
    L = sub("_lib")
    # the eval sizes did not change: the fold alone, and the train sizes lie behind them
    assert L.seg_head_forward_workspace_bytes(128, 128, 5, 70) == 256 * 4
    assert L.seg_head_train_forward_workspace_bytes(128, 128, 5, 70) == (256 + 3 * 3 * 128) * 4             # 3 tiles: 3 partial rows
    assert L.seg_head_train_backward_workspace_bytes(128, 128, 5, 70) == L.seg_head_backward_workspace_bytes(128, 128, 5, 70) + 256 * 4
    for fn in (L.seg_head_train_forward_workspace_bytes, L.seg_head_train_backward_workspace_bytes):
        assert fn(256, 256, 32, 2) > 0 and fn(1, 32, 2, 1 << 24) > 0
        for bad, says in (((257, 128, 5, 70), "cin=257"), ((128, 112, 5, 70), "multiple of 32"), ((128, 128, 33, 70), "n_classes=33"),
                          ((128, 128, 5, 0), "M=0"), ((128, 128, 5, 1), ">= 2 rows"), ((128, 128, 5, (1 << 24) + 1), "exceed 16777216")):
            with pytest.raises(L.AmpnetError, match=says):
                fn(*bad)


# ---- the modules -------------------------------------------------------------------------------------------------------------------------
def test_constructor_rules():
    U, A = sub("pointNet.model.pointnet2_utils"), sub("pointNet.model.pointnetAtt")
    head = U.PointNetSegHead(128, 128, 5, device="cpu", grad=True, batch_stats=True)
    assert head.batch_stats and head.seed == 0x6A09E667 and head._step == 0
    assert not U.PointNetSegHead(128, 128, 5, device="cpu").batch_stats
    for bad in ((0, 128, 5), (128, 48, 5), (128, 128, 33)):
        with pytest.raises(NotImplementedError, match="segmentation head is built for"):
            U.PointNetSegHead(*bad, device="cpu", batch_stats=True)
    # seeds: eval mode does not advance the step, train mode does
    head.eval()
    assert head.next_seed() == 0x6A09E667 and head._step == 0
    head.train()
    assert head.next_seed() == 0x6A09E667 and head.next_seed() == (0x6A09E667 + 0x632BE5AB) & 0xFFFFFFFF and head._step == 2
    # the refusals of a train-mode call come before anything touches the GPU
    x = torch.zeros(2, 128, 35)
    with pytest.raises(NotImplementedError, match="eval mode"):
        U.PointNetSegHead(128, 128, 5, device="cpu").train()(x)
    with pytest.raises(NotImplementedError, match="predict is an eval operation"):
        head.predict(x)
    full = U.PointNetSegHead(128, 128, 5, dropout=1.0, device="cpu", batch_stats=True).train()
    with pytest.raises(NotImplementedError, match="0 <= p < 1"):
        full._train_rows(torch.zeros(70, 128))
    cumulative = U.PointNetSegHead(128, 128, 5, device="cpu", batch_stats=True).train()
    cumulative.bn1.momentum = None
    with pytest.raises(NotImplementedError, match="momentum=None"):
        cumulative._train_rows(torch.zeros(70, 128))
    # the model's flag
    with pytest.raises(ValueError, match="head_batch_stats=True needs decoder_batch_stats=True"):
        A.pointnet_2_seg(5, device="cpu", decoder_grad=True, head_batch_stats=True)
    frozen = A.pointnet_2_seg(5, device="cpu", decoder_grad=True, decoder_batch_stats=True).train()
    assert frozen.fp1.training and not frozen._head.training and not frozen.bn1.training
    model = A.pointnet_2_seg(5, device="cpu", decoder_grad=True, decoder_batch_stats=True, head_batch_stats=True)
    assert model._head.batch_stats and not model._head.training
    model.train()
    assert model._head.training and model.bn1.training and model.drop1.training and model.fp1.training and not model.sa1.training
    model.eval()
    assert not model._head.training and not model.bn1.training
    assert list(model.state_dict()) == list(A.pointnet_2_seg(5, device="cpu").state_dict())
