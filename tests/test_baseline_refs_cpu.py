"""The float64 restatements of tests/baseline_probe.py, without a GPU: each is held to torch in float64 (nn.BatchNorm1d in train mode with its
running update and its autograd backward composed with ReLU, max_pool1d with return_indices, log_softmax and its backward, torch.bmm for the mix
and autograd for dT, the eval-mode fold), and each restatement evaluated in fp32 numpy stays inside its own bar, so the bars admit a correct fp32
implementation.  Two conditions on the committed inputs are asserted here, per case, on the reference alone: the ReLU cap (at most 1 % of a case
is left undecided by |pre-activation| > bar) and the presence of the edge a case is named for (ties across row groups, dead rows with da set, a
constant column, a column with mean^2 >> variance).  The backward entry points' shape refusals run here too: they are decided on the host."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import baseline_probe as P

T64 = dict(rtol=1e-9, atol=1e-11)
STATS = [(M, C) for M in P.STATS_M for C in P.STATS_C]
BWD = [(M, C) for M in P.BWD_M for C in P.BWD_C]


def t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def close(a, b, **kw):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), **(kw or T64))


def test_descriptor_mirror_has_the_headers_size():
    assert ctypes.sizeof(P.BaselineProbe) == 16 * 4 + 4 * 4 + 2 * 4 + 8 + 24 * 16
    assert len(P.OPS) == 25 and sorted(P.OPS.values()) == list(range(25))


# ---- BatchNorm, train mode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", STATS)
def test_stats_and_bn_act_equal_torch_batchnorm(M, C):
    c = P.make_stats(M, C)
    bn = torch.nn.BatchNorm1d(C, eps=P.BN_EPS, momentum=P.MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(t64(c["gamma"])), bn.bias.copy_(t64(c["beta"]))
        bn.running_mean.copy_(t64(c["rm"])), bn.running_var.copy_(t64(c["rv"]))
    y = torch.relu(bn(t64(c["z"])))
    r = P.stats_ref(c["z"], c["rm"], c["rv"])
    # the kernel's 1 - momentum is the fp32 difference 1.0f - 0.1f = 0.9f, torch's the float64 one: 2.4e-8 apart
    close(r["rm"][0], bn.running_mean.numpy(), rtol=1e-7, atol=1e-7)
    close(r["rv"][0], bn.running_var.numpy(), rtol=1e-7, atol=1e-7)
    act = P.bn_act_ref(c["z"], r["mean"][0], r["invstd"][0], c["gamma"], c["beta"])
    # column 0 (1000 +- 1): torch's own float64 variance carries ~1e-10 there
    close(act["a"][0], y.detach().numpy(), rtol=1e-7, atol=1e-9)
    # the edges the cases are named for
    assert np.all(r["invstd"][0][1] == 1.0 / np.sqrt(P.BN_EPS)), "column 1 is constant: variance exactly 0"
    var0 = 1.0 / r["invstd"][0][0] ** 2
    assert r["mean"][0][0] ** 2 > 1e4 * var0, "column 0: mean^2 >> variance"
    assert (~act["sure"]).sum() <= 0.01 * act["sure"].size, "ReLU cap"


@pytest.mark.parametrize("M,C", STATS)
def test_stats_fp32_evaluation_stays_inside_the_bars(M, C):
    c = P.make_stats(M, C)
    r, r32 = P.stats_ref(c["z"], c["rm"], c["rv"]), P.stats_ref(c["z"], c["rm"], c["rv"], dt=np.float32)
    for k in ("mean", "invstd", "rm", "rv"):
        assert r32[k][0].dtype == np.float32 and P.worst(r32[k][0], r[k]) <= 1.0, k
    mean, invstd = P.f32(r["mean"][0]), P.f32(r["invstd"][0])
    a, a32 = P.bn_act_ref(c["z"], mean, invstd, c["gamma"], c["beta"]), P.bn_act_ref(c["z"], mean, invstd, c["gamma"], c["beta"], dt=np.float32)
    assert P.worst(a32["pre"][0], a["pre"]) <= 1.0
    rs, rs32 = P.running_stats_ref(c["rm"], c["rv"]), P.running_stats_ref(c["rm"], c["rv"], dt=np.float32)
    assert P.worst(rs32["invstd"][0], rs["invstd"]) <= 1.0 and np.array_equal(rs32["mean"][0], c["rm"])
    close(rs["invstd"][0], 1.0 / np.sqrt(P.f64(c["rv"]) + P.BN_EPS))


@pytest.mark.parametrize("M,C", BWD)
def test_bn_backward_equals_autograd_through_relu(M, C):
    c = P.make_bn_bwd(M, C)
    # autograd on the float64 statistics of the same z: mean / invstd as float64 inputs of the restatement
    z = t64(c["z"]).requires_grad_(True)
    g, b = t64(c["gamma"]).requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    st = P.stats_ref(c["z"], np.zeros(C), np.ones(C))
    pre = F.batch_norm(z, None, None, g, b, True, 0.1, P.BN_EPS)
    a64 = torch.relu(pre)
    a64.backward(t64(c["da"]))
    a = a64.detach().numpy()
    s = P.bn_bwd_sums_ref(c["da"], a, c["z"], st["mean"][0], st["invstd"][0])
    close(s["dg"][0], g.grad.numpy(), rtol=1e-7, atol=1e-9)
    close(s["dbe"][0], b.grad.numpy(), rtol=1e-7, atol=1e-9)
    dz = P.bn_bwd_apply_ref(c["da"], a, c["z"], st["mean"][0], st["invstd"][0], c["gamma"], s["dg"][0], s["dbe"][0])
    # column 0 (mean^2 >> variance) and column 1 (invstd = 316): float64 itself carries ~1e-9 relative there
    close(dz["dz"][0], z.grad.numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("M,C", BWD)
def test_bn_backward_fp32_evaluation_and_its_edges(M, C):
    c = P.make_bn_bwd(M, C)
    args = (c["da"], c["a"], c["z"], c["mean"], c["invstd"])
    s, s32 = P.bn_bwd_sums_ref(*args), P.bn_bwd_sums_ref(*args, dt=np.float32)
    for k in ("dg", "dbe"):
        assert P.worst(s32[k][0], s[k]) <= 1.0, k
    dg, dbe = P.f32(s["dg"][0]), P.f32(s["dbe"][0])
    d, d32 = P.bn_bwd_apply_ref(*args, c["gamma"], dg, dbe), P.bn_bwd_apply_ref(*args, c["gamma"], dg, dbe, dt=np.float32)
    assert P.worst(d32["dz"][0], d["dz"]) <= 1.0
    dead = (c["a"] == 0) & (c["da"] != 0)
    assert dead.mean() > 0.2 and ((c["a"] > 0) & (c["da"] != 0)).mean() > 0.2, "dead rows with da set, and live ones"
    assert np.all(c["invstd"][1] == np.float32(1.0 / np.sqrt(P.BN_EPS))), "the constant column"


# ---- pooling ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C,kind", P.POOL_CASES)
def test_rowmax_is_max_pool1d_with_indices(B, N, C, kind):
    a = P.make_pool(B, N, C, kind)
    r = P.rowmax_ref(a, B, N, C)
    v, i = F.max_pool1d(torch.from_numpy(a).double().permute(0, 2, 1), N, return_indices=True)
    assert np.array_equal(r["out"].astype(np.float64), v[:, :, 0].numpy()) and np.array_equal(r["arg"], i[:, :, 0].numpy().astype(np.int32))
    assert not np.signbit(a).any() and (a >= 0).all()
    if kind == "relu":
        assert not a[:, :, ::5].any() and not r["out"][:, ::5].any() and not r["arg"][:, ::5].any(), "all-zero columns: value 0 at row 0"
    if kind in P.TIE_ROWS:
        lo, hi = P.TIE_ROWS[kind]
        assert np.all(r["arg"] == lo) and np.all(a[:, hi] == r["out"]) and lo % 4 != hi % 4, "an equal maximum in two row groups"
        assert (lo % 4 > hi % 4) == (kind == "low_late")
    if kind == "ties" and N >= 5 and C >= 64:
        eq = a == r["out"][:, None, :]
        groups = np.stack([eq[:, g::4].any(1) for g in range(4)], 0).sum(0)
        assert (groups > 1).mean() > 0.5, "maxima repeated across row groups"
    d_pool = P.f32(np.random.default_rng(N + C).standard_normal((B, C)))
    s = P.pool_scatter_ref(d_pool, r["arg"], B, N, C)
    x = torch.from_numpy(a).double().requires_grad_(True)
    F.max_pool1d(x.permute(0, 2, 1), N)[:, :, 0].backward(torch.from_numpy(d_pool).double())
    assert np.array_equal(s.astype(np.float64), x.grad.numpy())


# ---- the mix ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", P.MIX_K)
@pytest.mark.parametrize("N", P.MIX_BWD_N)
def test_mix_is_bmm_and_dT_its_autograd(N, k):
    B = 3
    c = P.make_mix(B * N, N, k)
    x = t64(c["x"]).reshape(B, N, 9)
    T = t64(c["T"]).requires_grad_(True)
    out = torch.cat([torch.bmm(x[:, :, :k], T), x[:, :, k:]], 2)
    r = P.mix_ref(c["x"], c["T"], N, k)
    close(np.concatenate([r["head"][0], r["tail"]], 1), out.detach().numpy().reshape(B * N, 9))
    d = P.f32(np.random.default_rng(N + k).standard_normal((B * N, 9)))
    out.backward(t64(d).reshape(B, N, 9))
    rb = P.mix_bwd_ref(c["x"], d, B, N, k)
    close(rb["dT"][0], T.grad.numpy())
    r32 = P.mix_ref(c["x"], c["T"], N, k, dt=np.float32)
    assert P.worst(r32["head"][0], r["head"]) <= 1.0 and np.array_equal(r32["tail"], c["x"][:, k:])
    assert P.worst(P.mix_bwd_ref(c["x"], d, B, N, k, dt=np.float32)["dT"][0], rb["dT"]) <= 1.0


@pytest.mark.parametrize("C", P.SEG_C)
@pytest.mark.parametrize("N", P.SEG_N)
def test_segsum_and_logits(N, C):
    B = 3
    dz = P.f32(np.random.default_rng(N * 100 + C).standard_normal((B * N, C)))
    r = P.segsum_ref(dz, B, N, C)
    close(r["out"][0], t64(dz).reshape(B, N, C).sum(1).numpy())
    assert P.worst(P.segsum_ref(dz, B, N, C, dt=np.float32)["out"][0], r["out"]) <= 1.0
    lg = P.logits_ref(dz, B, N, C)
    assert np.array_equal(lg, torch.from_numpy(dz).reshape(B, N, C).permute(0, 2, 1).contiguous().numpy())


# ---- log_softmax ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", P.LSM_SHIFT)
@pytest.mark.parametrize("C", P.LSM_C)
@pytest.mark.parametrize("B", P.LSM_B)
def test_log_softmax_and_backward_equal_torch(B, C, shift):
    c = P.make_lsm(B, C, shift)
    z = t64(c["z"]).requires_grad_(True)
    y = F.log_softmax(z, dim=1)
    y.backward(t64(c["d"]))
    r, rb = P.log_softmax_ref(c["z"]), P.log_softmax_bwd_ref(c["z"], c["d"])
    close(r["out"][0], y.detach().numpy(), rtol=1e-9, atol=1e-12)
    close(rb["dz"][0], z.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert P.worst(P.log_softmax_ref(c["z"], dt=np.float32)["out"][0], r["out"]) <= 1.0
    assert P.worst(P.log_softmax_bwd_ref(c["z"], c["d"], dt=np.float32)["dz"][0], rb["dz"]) <= 1.0
    close(np.exp(r["out"][0]).sum(1), np.ones(B), rtol=1e-12, atol=0)
    if shift:
        base = P.log_softmax_ref(P.f64(c["z"]) - shift)                     # shift invariance, in float64 on the same fp32 logits
        close(r["out"][0], base["out"][0], rtol=1e-9, atol=1e-12)


# ---- the eval fold ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("C", P.FOLD_C)
def test_fold_and_affine_equal_eval_batchnorm(C, bias, bn):
    c = P.make_fold(C, bias, bn)
    M, per = 13, 5
    g = np.random.default_rng(C + bias + 2 * bn)
    z, add = P.f32(g.standard_normal((M, C))), P.f32(g.standard_normal(((M - 1) // per + 1, C)))
    f = P.fold_ref(c["bias"], c["gamma"], c["beta"], c["rm"], c["rv"], C)
    v = t64(z) + t64(add)[torch.arange(M) // per] + (t64(c["bias"]) if bias else 0.0)
    want = F.batch_norm(v, t64(c["rm"]), t64(c["rv"]), t64(c["gamma"]), t64(c["beta"]), False, 0.1, P.BN_EPS) if bn else v
    a = P.affine_ref(z, f["scale"][0], f["shift"][0], add, per)
    close(a["pre"][0], want.numpy())
    f32_ = P.fold_ref(c["bias"], c["gamma"], c["beta"], c["rm"], c["rv"], C, dt=np.float32)
    assert P.worst(f32_["scale"][0], f["scale"]) <= 1.0 and P.worst(f32_["shift"][0], f["shift"]) <= 1.0
    sc, sh = P.f32(f["scale"][0]), P.f32(f["shift"][0])
    for ad in (None, add):
        a, a32 = P.affine_ref(z, sc, sh, ad, per), P.affine_ref(z, sc, sh, ad, per, dt=np.float32)
        assert P.worst(a32["pre"][0], a["pre"]) <= 1.0
        assert (~a["sure"]).sum() <= 0.01 * a["sure"].size, "ReLU cap"


# ---- bias, add, dropout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,per,kind", P.BIAS_CASES)
def test_bias_fp32_evaluation(M, C, per, kind):
    c = P.make_bias(M, C, per, kind)
    r = P.bias_ref(c["z"], c["bias"], c["add"], per)
    want = t64(c["z"]) + (t64(c["bias"]) if c["bias"] is not None else 0.0) + (t64(c["add"])[torch.arange(M) // per] if c["add"] is not None else 0.0)
    close(r["z"][0], want.numpy())
    assert P.worst(P.bias_ref(c["z"], c["bias"], c["add"], per, dt=np.float32)["z"][0], r["z"]) <= 1.0
    assert (M * C) % 256 != 0


@pytest.mark.parametrize("p", P.DROP_P)
def test_dropout_reference_keeps_about_one_minus_p(p):
    n = 1 << 16
    r = P.dropout_ref(np.ones(n, dtype=np.float32), 12345, p)
    assert abs(r["keep"].mean() - (1.0 - float(np.float32(p)))) < 4.0 * np.sqrt(p * (1 - p) / n) + 1e-4
    assert np.all(r["out"][r["keep"]] == np.float32(1.0) / (np.float32(1.0) - np.float32(p))) and not r["out"][~r["keep"]].any()


@pytest.mark.parametrize("c", P.LAYER_CASES, ids=lambda c: f"K{c['K']}_w{c['w0']}_bn{c['bn']}")
def test_layer_cases_keep_the_relu_margin(c):
    """the composed cases are compared bit for bit on the device; here only that their inputs exercise what they are named for"""
    t = P.make_layer(c)
    assert t["A"].shape == (c["M"], c["lda"]) and c["ldw"] >= c["w0"] + c["K"] and (c["w0"] == 0 or c["ldw"] > c["K"])
    assert (t["gamma"] is None) == (not c["bn"])


# ---- the backward entry points refuse what the train forward refuses ---------------------------------------------------------------------------
def test_backward_entry_points_repeat_the_forwards_shape_limits():
    for which, B, N, C, rc, msg in P.backward_shape_refusals():
        assert rc == P.AMPNET_E_ARG and "bad shape" in msg and f"ampnet_pointnet_{which}_bwd_f32" in msg, (which, B, N, C, rc, msg)
