"""Layer-local float64 parity of the segmentation head's own kernels: posenc_tokens, attention_core, attention_core_bwd, head_logits +
loss_finalize, head_out_bwd<fp32 / bf16 z3>, and the token path's sgemm_linear_bwd / sgemm_wgrad_bias.

Each case launches ONE kernel through ampnet_probe_head_f32 (include/ampnet_hip.h, "test hooks") on inputs of tests/head_probe.py and holds every
output to the float64 restatement there, at the bars of that module's docstring.  Every case also checks: outputs pre-filled with NaN are
finite where the contract writes and keep their sentinel where it does not; a second run on re-poisoned outputs is bitwise identical; the probe
recorded the kernel the case is meant for.

Precision modes: none of these kernels reads the matrix-precision switch (the attention / logits / head_out_bwd kernels are VALU fp32,
sgemm_linear_bwd / sgemm_wgrad_bias always run sgemm_mfma on the fp32 matrix pipe unless AMPNET_SGEMM_VALU=1 is set at process start); head_out_bwd
reads a bf16 z3 when the forward stored one (mode bf16_store), which the probe selects by z_bf16.  The small GEMMs are run in fp32 and f32x3 all the
same and must give the same bits.

Exponential sweep (test_exp_log_sweep): worst relative error of __expf / expf / logf against float64 divided by (2 |x| + c) eps, required <= 0.5.
c = 4 for expf and logf (measured 1.38 and 2.98 eps worst: 0.24 and 0.48).  __expf measured 0.59 with c = 4 (64.56 eps worst, growing as 1.23 |x| eps), so its constant was
replaced by the measured c = 21 (head_probe.FAST_EXP_ULP; the smallest the float64 sweep supports is 20.47): 0.50 now.
Observed worst error/bar on the MI355X: attention probs 0.96, ctx 0.02,
attention_bwd dq 0.04 / dk 0.04 / dv 0.17; posenc tok 0.11, hid 0.06; logits loss_part 0.10, ce 0.05; head_out_bwd dy3 0.18, dW4 0.17, db4 0.01, part_a 0.06,
part_b 0.10 (bf16 z3: 0.15, 0.15, 0.03, 0.05, 0.09); linear_bwd / wgrad_bias dW 0.15, dX 0.06, db 0.10 (identical in fp32 and f32x3).
Scratch-build mutations, each failing its test: dscale dropped in head_out_bwd (all 48 cases with drop_p = 0.3, dy3 at 1.8e5 .. 4.6e5 of the bar); sds[i][j] for
sds[j][i] in the dk sum (65 of the 75 cases with W > 1 that save probs, dk at >= 1.0e5 of the bar); >= in the argmax (all 60
cases with C > 1).
"""
import itertools

import numpy as np
import pytest
import torch

import head_probe as H
import pw_probe as PP

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[head layers] worst error/bar {k}: {WORST[k]:.4f}")


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def nanbuf(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def i64buf(*shape):
    return torch.full(shape, -77, dtype=torch.int64, device="cuda")


def poison(t):
    t.fill_(-77 if t.dtype == torch.int64 else float("nan"))


def is_sentinel(t):
    a = t.detach().cpu()
    return bool((a == -77).all()) if a.dtype == torch.int64 else bool((a.view(torch.int32) == NAN_BITS).all())


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device="cuda", dtype=dtype or t.dtype)


def host(t):
    return t.detach().cpu().numpy()


def launch(d, outs, want_names):
    """run, check the recorded kernels, re-poison, run again: bitwise equal.  Returns nothing: the outputs hold the second run."""
    rc, names = H.run(d)
    assert rc == 0, PP.last_error()
    assert names == want_names, (names, want_names)
    first = {k: v.detach().cpu().clone() for k, v in outs.items()}
    for v in outs.values():
        poison(v)
    rc, _ = H.run(d)
    assert rc == 0, PP.last_error()
    for k, v in outs.items():
        a, b = first[k], v.detach().cpu()
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), f"{k}: second run differs bitwise"


# ---- exp / log ---------------------------------------------------------------------------------------------------------------------
def test_exp_log_sweep():
    """The argument ranges of the cases: exp(s - m) with s - m in [-100, 0] (attention 'large', logits of std 3), log of a sum in [1, 8]."""
    xe = np.concatenate([-np.linspace(0, 87, 200001), -np.random.default_rng(0).random(100000) * 30]).astype(np.float32)
    xl = np.concatenate([np.linspace(1, 8, 200001), 1 + np.random.default_rng(1).random(100001) * 1e-3]).astype(np.float32)
    for x, cols in ((xe, (0, 1)), (xl, (2,))):
        d = H.HeadProbe()
        d.op, d.rows = 7, len(x)
        y = nanbuf(3, len(x))
        H.set_tensors(d, X=dev(x), dX=y)
        rc, names = H.run(d)
        assert rc == 0 and names == ["exp_log_sweep"], (PP.last_error(), names)
        got = host(y).astype(np.float64)
        x64 = x.astype(np.float64)
        for c in cols:
            want = np.log(x64) if c == 2 else np.exp(x64)
            ok = want > 2.0 ** -126 if c != 2 else np.ones_like(want, dtype=bool)
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.where(want != 0, np.abs(got[c] - want) / np.abs(want), np.abs(got[c]))
            k = H.FAST_EXP_ULP if c == 0 else H.EXP_ULP
            r = float((rel[ok] / ((2 * np.abs(x64[ok]) + k) * H.EPS)).max())
            r4 = float((rel[ok] / ((2 * np.abs(x64[ok]) + 4.0) * H.EPS)).max())
            ulp = float((rel[ok] / H.EPS).max())
            name = ("__expf", "expf", "logf")[c]
            print(f"[head layers] {name}: worst relative error {ulp:.3f} eps, {r4:.4f} of (2|x| + 4) eps, {r:.4f} of (2|x| + {k:g}) eps")
            note(f"sweep {name}", r)
            assert r <= 0.5, f"{name}: {r:.4f} of (2|x| + {k:g}) eps; the bars assume <= 0.5"
            below = ~ok
            assert np.all(np.abs(got[c][below]) <= 2.0 ** -126)


# ---- positional encoding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", H.POSENC_Q)
@pytest.mark.parametrize("train", [True, False])
def test_posenc_tokens(Q, train):
    c = H.make_posenc(Q)
    r = H.posenc_ref(*(c[k] for k in ("gl", "cent", "w1", "b1", "w2", "b2")))
    d = H.HeadProbe()
    d.op, d.Q = 0, Q
    tok, hid, slope = nanbuf(Q + 1, 256), nanbuf(Q + 1, 16), nanbuf(Q + 1, 16)
    H.set_tensors(d, **{k: dev(c[k]) for k in ("gl", "cent", "w1", "b1", "w2", "b2")}, tok=tok, hid=hid if train else None, slope=slope if train else None)
    launch(d, dict(tok=tok, hid=hid, slope=slope), ["posenc_tokens"])
    assert is_sentinel(tok[Q:]) and is_sentinel(hid[Q:]) and is_sentinel(slope[Q:])
    assert note("posenc tok", H.worst(host(tok[:Q]), r["tok"])) <= 1.0
    if train:
        # fc1's output is exact in fp32 by construction (tests/test_head_refs_cpu.py checks that): every decision, 0 included, is exact
        assert np.array_equal(host(slope[:Q]).astype(np.float64), np.where(r["slope"][0] == 1.0, 1.0, float(np.float32(0.01))))
        pos = r["hid"][0] > 0
        assert np.array_equal(host(hid[:Q])[pos].astype(np.float64), r["hid"][0][pos]), "a positive hidden unit is fc1's exact output"
        assert note("posenc hid", H.worst(host(hid[:Q]), r["hid"])) <= 1.0
        z = r["hid"][0] == 0
        assert z.any() and not host(hid[:Q])[z].any(), "a hidden unit exactly at 0 stays 0 (slope 0.01)"
    else:
        assert is_sentinel(hid) and is_sentinel(slope)


# ---- attention -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", H.ATT_VARIANTS)
@pytest.mark.parametrize("B", H.ATT_B)
@pytest.mark.parametrize("W", H.ATT_W)
def test_attention_core_and_bwd(W, B, variant):
    c = H.make_attention(W, B, variant)
    r = H.attention_ref(c["qkv"], c["mask"], B, W, c["drop_p"], c["key"])
    d = H.HeadProbe()
    d.op, d.B, d.W, d.drop_p = 1, B, W, c["drop_p"]
    d.drop_seed = PP.drop_base(*c["key"]) if c["drop_p"] > 0 else 0
    qkv = dev(c["qkv"])
    probs, ctx = nanbuf(B * 8 * W * W + 3), nanbuf(B * W + 1, 256)
    H.set_tensors(d, qkv=qkv, mask=None if c["mask"] is None else dev(c["mask"]), probs=probs if c["want_probs"] else None, ctx=ctx)
    launch(d, dict(probs=probs, ctx=ctx), ["attention_core"])
    assert is_sentinel(ctx[B * W:])
    assert note("attention ctx", H.worst(host(ctx[:B * W]), r["ctx"])) <= 1.0
    dead_rows = np.zeros(B * W, dtype=bool) if c["mask"] is None else np.repeat(c["mask"].all(1), W)
    assert not host(ctx[:B * W])[dead_rows].any(), "a sample with every key masked: zeros"
    if not c["want_probs"]:
        assert is_sentinel(probs)
        return
    assert is_sentinel(probs[B * 8 * W * W:])
    pg = host(probs[:B * 8 * W * W]).reshape(B, 8, W, W)
    assert note("attention probs", H.worst(pg, r["probs"])) <= 1.0
    if c["mask"] is not None:
        assert not pg[np.broadcast_to(c["mask"].astype(bool).reshape(B, 1, 1, W), pg.shape)].any(), "masked keys get probability exactly 0"
    # backward, from the probs the forward kernel saved (the kernel's own contract) and a chosen d(ctx)
    rb = H.attention_bwd_ref(c["qkv"], pg, c["dctx"], B, W, c["drop_p"], c["key"])
    d2 = H.HeadProbe()
    d2.op, d2.B, d2.W, d2.drop_p, d2.drop_seed = 2, B, W, c["drop_p"], d.drop_seed
    dqkv = nanbuf(B * W + 1, 768)
    H.set_tensors(d2, qkv=qkv, probs=probs, dctx=dev(c["dctx"]), dqkv=dqkv)
    launch(d2, dict(dqkv=dqkv), ["attention_core_bwd"])
    assert is_sentinel(dqkv[B * W:])
    g = host(dqkv[:B * W])
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(256 * i, 256 * (i + 1))
        assert note(f"attention_bwd {nm}", H.worst(g[:, sl], (rb["dqkv"][0][:, sl], rb["dqkv"][1][:, sl]))) <= 1.0
    assert not g[dead_rows].any(), "a sample with every key masked: zero gradients"


# ---- logits tail ---------------------------------------------------------------------------------------------------------------------
LOGIT_CASES = [(C, P, B, ld, cw) for C in H.LOGIT_C for P in H.LOGIT_P for B in H.LOGIT_B for ld, cw in ((C, True), (32, False))]


@pytest.mark.parametrize("C,P,B,ldz4,cw", LOGIT_CASES)
def test_head_logits_and_loss(C, P, B, ldz4, cw):
    c = H.make_logits(C, P, B, ldz4, cw)
    R = c["R"]
    r = H.logits_ref(c["z4"], R, P, C, c["targets"], c["class_w"])
    nb = -(-R // H.HL_ROWS)
    for form in ("loss", "preds_only", "bare"):
        d = H.HeadProbe()
        d.op, d.R, d.P, d.C, d.ldz4 = 3, R, P, C, ldz4
        logits, preds, part, loss = nanbuf(R * C + 5), i64buf(R + 3), nanbuf(nb + 1, 2), nanbuf(4)
        H.set_tensors(d, z4=dev(c["z4"]), logits=logits, preds=None if form == "bare" else preds,
                      targets=dev(c["targets"]) if form == "loss" else None,
                      class_w=dev(c["class_w"]) if (form == "loss" and cw) else None, loss_part=part, loss_out=loss if form == "loss" else None)
        launch(d, dict(logits=logits, preds=preds, part=part, loss=loss), ["head_logits", "loss_finalize"] if form == "loss" else ["head_logits"])
        assert is_sentinel(logits[R * C:]) and is_sentinel(preds[R:])
        # the transpose is a copy: bitwise (the NaN padding columns of z4 never reach it)
        assert np.array_equal(host(logits[:R * C]).view(np.int32), np.ascontiguousarray(r["logits"], dtype=np.float32).reshape(-1).view(np.int32))
        if form == "bare":
            assert is_sentinel(preds)
        else:
            assert np.array_equal(host(preds[:R]), r["preds"]), "first-maximum argmax (the logits are inputs: exact)"
        if form != "loss":
            assert is_sentinel(part) and is_sentinel(loss), "no targets: loss_part is not written"
            continue
        assert is_sentinel(part[nb:]) and is_sentinel(loss[2:])
        assert note("logits loss_part", H.worst(host(part[:nb]), r["loss_part"])) <= 1.0
        l2 = host(loss[:2])
        assert note("logits ce", H.worst(l2[:1], (r["loss2"][0][:1], r["loss2"][1][:1]))) <= 1.0
        assert float(l2[1]) == r["loss2"][0][1], "loss2[1] is the float64 weight sum (weights exact in fp32)"


# ---- conv_4 backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zb", [0, 1])
@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("C", H.HOB_C)
@pytest.mark.parametrize("R", H.HOB_R)
def test_head_out_bwd(R, C, drop_p, zb):
    c = H.make_head_out(R, C, drop_p, zb)
    r = H.head_out_bwd_ref(c["dlogits"], c["zread"], c["scale"], c["shift"], c["mean"], c["invstd"], c["w4"], c["P"], drop_p, c["key"])
    blocks = -(-R // H.HB_ROWS)
    d = H.HeadProbe()
    d.op, d.R, d.P, d.C, d.z_bf16, d.drop_p = 4, R, c["P"], C, zb, drop_p
    d.drop_seed = PP.drop_base(*c["key"]) if drop_p > 0 else 0
    dy3, pa, pb, w4p = nanbuf(R + 2, 64), nanbuf(blocks + 1, 64), nanbuf(blocks + 1, 64), nanbuf(blocks * (C * 64 + C) + 7)
    z3 = dev(c["z3"]).to(torch.bfloat16) if zb else dev(c["z3"])
    assert not zb or np.array_equal(z3.float().cpu().numpy(), c["zread"])
    d.z3, d.z3_n = z3.data_ptr(), z3.numel()
    H.set_tensors(d, dlogits=dev(c["dlogits"]), **{k: dev(c[k]) for k in ("scale", "shift", "mean", "invstd", "w4")}, dy3=dy3, part_a=pa, part_b=pb, w4part=w4p)
    launch(d, dict(dy3=dy3, pa=pa, pb=pb, w4p=w4p), ["head_out_bwd<bf16>" if zb else "head_out_bwd<f32>"])
    assert is_sentinel(dy3[R:]) and is_sentinel(pa[blocks:]) and is_sentinel(pb[blocks:]) and is_sentinel(w4p[blocks * (C * 64 + C):])
    got = host(dy3[:R]).astype(np.float64)
    sure = r["sure"]
    assert (~sure).sum() <= 1e-3 * R * 64
    fam = "head_out_bwd" + (" bf16" if zb else "")
    assert note(f"{fam} dy3", H.worst(np.where(sure, got, 0), (np.where(sure, r["dy3"][0], 0), r["dy3"][1]))) <= 1.0
    un = ~sure                                                     # undecided by the ReLU: 0 or within the bar of the unmasked value
    assert np.all((got[un] == 0) | (np.abs(got[un] - r["da3"][0][un]) <= r["da3"][1][un]))
    w = host(w4p[:blocks * (C * 64 + C)]).astype(np.float64).reshape(blocks, C * 64 + C).sum(0)
    assert note(f"{fam} dW4", H.worst(w[:C * 64].reshape(C, 64), r["dW4"])) <= 1.0
    assert note(f"{fam} db4", H.worst(w[C * 64:], r["db4"])) <= 1.0
    assert note(f"{fam} part_a", H.worst(host(pa[:blocks]).astype(np.float64).sum(0), r["part_a"])) <= 1.0
    assert note(f"{fam} part_b", H.worst(host(pb[:blocks]).astype(np.float64).sum(0), r["part_b"])) <= 1.0


# ---- the token path's small GEMMs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f32x3"])
@pytest.mark.parametrize("n_out,n_in", H.LIN_SHAPES)
@pytest.mark.parametrize("rows", H.LIN_ROWS)
def test_sgemm_linear_bwd_and_wgrad_bias(rows, n_out, n_in, mode):
    ldw = 320 if n_in == 256 else n_in                            # conv_2's token half: columns 64.. of a [128, 320] matrix
    c = H.make_linear(rows, n_out, n_in, ldw)
    W = c["Wl"][:, :n_in]
    PP.L.set_matrix_precision(mode)
    try:
        for db_on, mul_on in itertools.product((False, True), (False, True)):
            r = H.linear_bwd_ref(c["G"], c["X"], W, c["dx_mul"] if mul_on else None)
            d = H.HeadProbe()
            d.op, d.rows, d.n_out, d.n_in = 5, rows, n_out, n_in
            d.ldg, d.ldx, d.ldw, d.lddw, d.lddx = n_out, n_in, ldw, ldw, n_in
            Wd = dev(c["Wl"]).reshape(-1)[:(n_out - 1) * ldw + n_in]        # the matrix ends with its last used column
            dW, dX, db = nanbuf((n_out - 1) * ldw + n_in), nanbuf(rows + 1, n_in), nanbuf(n_out + 3)
            H.set_tensors(d, G=dev(c["G"]), X=dev(c["X"]), Wl=Wd, dW=dW, dX=dX, db=db if db_on else None, dx_mul=dev(c["dx_mul"]) if mul_on else None)
            launch(d, dict(dW=dW, dX=dX, db=db), ["sgemm_mfma"])
            gW = torch.cat([dW, nanbuf(ldw - n_in)]).reshape(n_out, ldw)
            assert is_sentinel(gW[:, n_in:]) and is_sentinel(dX[rows:]) and is_sentinel(db[n_out:] if db_on else db)
            assert note("linear_bwd dW", H.worst(host(gW[:, :n_in]), r["dW"])) <= 1.0
            assert note("linear_bwd dX", H.worst(host(dX[:rows]), r["dX"])) <= 1.0
            if db_on:
                assert note("linear_bwd db", H.worst(host(db[:n_out]), r["db"])) <= 1.0
        d = H.HeadProbe()
        d.op, d.rows, d.n_out, d.n_in, d.ldg, d.ldx, d.lddw = 6, rows, n_out, n_in, n_out, n_in, n_in
        dW, db = nanbuf(n_out * n_in + 1), nanbuf(n_out + 1)
        H.set_tensors(d, G=dev(c["G"]), X=dev(c["X"]), dW=dW, db=db)
        launch(d, dict(dW=dW, db=db), ["sgemm_mfma"])
        assert is_sentinel(dW[n_out * n_in:]) and is_sentinel(db[n_out:])
        assert note("wgrad_bias dW", H.worst(host(dW[:n_out * n_in]).reshape(n_out, n_in), r["dW"])) <= 1.0
        assert note("wgrad_bias db", H.worst(host(db[:n_out]), r["db"])) <= 1.0
    finally:
        PP.L.set_matrix_precision("fp32")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_probe_refuses_bad_head_descriptors():
    """A short buffer of each kind, W = 33, C = 9 and R % P != 0 get AMPNET_E_ARG and launch nothing (every output keeps its sentinel)."""
    def refused(d, outs, what):
        rc, names = H.run(d)
        assert rc == H.AMPNET_E_ARG and names == [], (what, rc, names)
        assert all(is_sentinel(o) for o in outs), what

    def base(op):
        d = H.HeadProbe()
        d.op = op
        return d

    def t(n, dtype=torch.float32):
        return torch.zeros(max(n, 1), dtype=dtype, device="cuda")

    # op 0
    Q = 3
    full = dict(gl=Q * 256, cent=Q * 2, w1=32, b1=16, w2=4096, b2=256, tok=Q * 256, hid=Q * 16, slope=Q * 16)
    for short in full:
        d = base(0)
        d.Q = Q
        bufs = {k: (nanbuf(n - (k == short)) if k in ("tok", "hid", "slope") else t(n - (k == short))) for k, n in full.items()}
        H.set_tensors(d, **bufs)
        refused(d, [bufs[k] for k in ("tok", "hid", "slope")], f"posenc {short}")
    # ops 1, 2
    B, W = 2, 3
    full = dict(qkv=B * W * 768, mask=B * W, probs=B * 8 * W * W, ctx=B * W * 256)
    for short, (b_, w_) in [(k, (B, W)) for k in full] + [(None, (B, 33)), (None, (B, 0))]:
        d = base(1)
        d.B, d.W = b_, w_
        bufs = {k: (nanbuf(n - (k == short)) if k in ("probs", "ctx") else t(n - (k == short), torch.uint8 if k == "mask" else torch.float32))
                for k, n in full.items()}
        if short is None:
            bufs = {k: (nanbuf(B * 33 * 768) if k in ("probs", "ctx") else t(B * 33 * 768, torch.uint8 if k == "mask" else torch.float32)) for k in full}
        H.set_tensors(d, **bufs)
        refused(d, [bufs["probs"], bufs["ctx"]], f"attention {short} W={w_}")
    full = dict(qkv=B * W * 768, probs=B * 8 * W * W, dctx=B * W * 256, dqkv=B * W * 768)
    for short, w_ in [(k, W) for k in full] + [(None, 33)]:
        d = base(2)
        d.B, d.W = B, w_
        bufs = {k: (nanbuf(n - (k == short)) if k == "dqkv" else t(n - (k == short))) for k, n in full.items()}
        if short is None:
            bufs = {k: (nanbuf(B * 33 * 33 * 8 * 3) if k == "dqkv" else t(B * 33 * 33 * 8 * 3)) for k in full}
        H.set_tensors(d, **bufs)
        refused(d, [bufs["dqkv"]], f"attention_bwd {short} W={w_}")
    # op 3
    R, P, C, ld = 300, 100, 5, 8
    full = dict(z4=(R - 1) * ld + C, logits=R * C, targets=R, class_w=C, preds=R, loss_part=4, loss_out=2)
    variants = [(k, R, P, C, ld) for k in full] + [(None, R, P, 9, 16), (None, R, P, 0, 8), (None, R, 7, C, ld), (None, R, P, C, 4)]
    for short, r_, p_, c_, ld_ in variants:
        d = base(3)
        d.R, d.P, d.C, d.ldz4 = r_, p_, c_, ld_
        big = short is None
        bufs = {}
        for k, n in full.items():
            n = 16 * R if big else n - (k == short)
            bufs[k] = i64buf(n) if k == "preds" else t(n, torch.int64) if k == "targets" else nanbuf(n) if k in ("logits", "loss_part", "loss_out") else t(n)
        H.set_tensors(d, **bufs)
        refused(d, [bufs[k] for k in ("logits", "preds", "loss_part", "loss_out")], f"head_logits {short} {r_} {p_} {c_} {ld_}")
    # op 4
    R, P, C = 1100, 550, 5
    full = dict(dlogits=R * C, z3=R * 64, scale=64, shift=64, mean=64, invstd=64, w4=C * 64, dy3=R * 64, part_a=128, part_b=128, w4part=2 * (C * 64 + C))
    for zb in (0, 1):
        for short, p_, c_ in [(k, P, C) for k in full] + [(None, P, 9), (None, 7, C)]:
            d = base(4)
            d.R, d.P, d.C, d.z_bf16 = R, p_, c_, zb
            bufs = {}
            for k, n in full.items():
                n = 16 * R * 64 if short is None else n - (k == short)
                bufs[k] = nanbuf(n) if k in ("dy3", "part_a", "part_b", "w4part") else t(n, torch.bfloat16 if (k == "z3" and zb) else torch.float32)
            H.set_tensors(d, **bufs)
            refused(d, [bufs[k] for k in ("dy3", "part_a", "part_b", "w4part")], f"head_out_bwd {short} P={p_} C={c_} zb={zb}")
    # ops 5, 6
    rows, no, ni, ldw = 5, 16, 8, 12
    full = dict(G=rows * no, X=rows * ni, Wl=(no - 1) * ldw + ni, dW=(no - 1) * ldw + ni, dX=rows * ni, db=no, dx_mul=rows * ni)
    for op in (5, 6):
        for short in full:
            if op == 6 and short in ("Wl", "dX", "dx_mul"):
                continue
            d = base(op)
            d.rows, d.n_out, d.n_in, d.ldg, d.ldx, d.ldw, d.lddw, d.lddx = rows, no, ni, no, ni, ldw, ldw, ni
            bufs = {k: (nanbuf(n - (k == short)) if k in ("dW", "dX", "db") else t(n - (k == short))) for k, n in full.items()}
            H.set_tensors(d, **bufs)
            refused(d, [bufs[k] for k in ("dW", "dX", "db")], f"sgemm op {op} {short}")
    d = base(8)
    refused(d, [], "op 8")
