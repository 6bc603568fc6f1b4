"""The float64 restatements of tests/head_probe.py against independent float64 computations (torch's multi_head_attention_forward and its
autograd, the oracle's head pieces, F.cross_entropy autograd, torch.optim.Adam), an fp32 numpy evaluation of every operation under every bar,
and the exclusion caps of the committed cases (masked elements and argmax rows: at most 0.1 % per case).  No GPU."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

import head_probe as H
from oracle import ampnet_oracle as O

RTOL = 1e-12


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    assert float(np.abs(a - b).max() if a.size else 0.0) <= RTOL * scale, what


def under(res32, res64, names, what):
    for n in names:
        r = H.worst(res32[n][0], res64[n])
        assert r <= 1.0, f"{what} {n}: fp32 numpy evaluation at {r:.3f} of the bar"


def t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


ATT_CPU = [(W, B, v) for W in H.ATT_W for B in (1, 5) for v in H.ATT_VARIANTS] + [(32, 64, "maskall"), (9, 64, "drop")]


def test_attention_refs_match_torch_mha():
    for W, B, variant in ATT_CPU:
        c = H.make_attention(W, B, variant)
        r = H.attention_ref(c["qkv"], c["mask"], B, W, c["drop_p"], c["key"])
        qkv = t64(c["qkv"]).requires_grad_(True)
        dead = c["mask"] is not None and bool(c["mask"].all(1).any())
        keep = t64(H.keep_flat(c["key"], B * 8 * W * W, c["drop_p"]).reshape(B * 8, W, W).astype(np.float64))
        # the oracle's attention core (sequence-first, identity projections) ...
        q, k, v = qkv.reshape(B, W, 3, 8, 32).permute(2, 0, 3, 1, 4).reshape(3, B * 8, W, 32)
        s = torch.bmm(q * H.QSCALE, k.transpose(1, 2))
        if c["mask"] is not None:
            s = s.masked_fill(torch.from_numpy(c["mask"].astype(bool)).reshape(B, 1, 1, W).expand(B, 8, W, W).reshape(B * 8, W, W), float("-inf"))
        a = torch.softmax(s, -1)
        a = torch.where(torch.isnan(a), torch.zeros_like(a), a)          # a fully masked row: zeros (attention.hip), where torch gives NaN
        ds = H.PP.dscale32(c["drop_p"]) if c["drop_p"] > 0 else 1.0
        ctx = torch.bmm(a * keep * ds, v).reshape(B, 8, W, 32).permute(0, 2, 1, 3).reshape(B * W, 256)
        close(r["probs"][0].reshape(B * 8, W, W), a.detach().numpy(), f"probs {W} {B} {variant}")
        close(r["ctx"][0], ctx.detach().numpy(), f"ctx {W} {B} {variant}")
        # ... and torch's own multi_head_attention_forward with identity projections (no dropout: its generator is not ours)
        if c["drop_p"] == 0 and not dead:
            x = t64(c["qkv"]).reshape(B, W, 3, 256)
            eye = torch.eye(256, dtype=torch.float64)
            out, wts = F.multi_head_attention_forward(
                x[:, :, 0].transpose(0, 1), x[:, :, 1].transpose(0, 1), x[:, :, 2].transpose(0, 1), 256, 8, None, None, None, None, False, 0.0,
                eye, torch.zeros(256, dtype=torch.float64), training=False,
                key_padding_mask=None if c["mask"] is None else torch.from_numpy(c["mask"].astype(bool)), need_weights=True,
                use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye, average_attn_weights=False)
            scale = H.QSCALE * math.sqrt(32.0)                          # the fp32 constant against torch's exact 1 / sqrt(32): rescale q
            if abs(scale - 1.0) < 1e-7:
                out2, _ = F.multi_head_attention_forward(
                    x[:, :, 0].transpose(0, 1) * scale, x[:, :, 1].transpose(0, 1), x[:, :, 2].transpose(0, 1), 256, 8, None, None, None, None,
                    False, 0.0, eye, torch.zeros(256, dtype=torch.float64), training=False,
                    key_padding_mask=None if c["mask"] is None else torch.from_numpy(c["mask"].astype(bool)), need_weights=False,
                    use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
                close(r["ctx"][0], out2.transpose(0, 1).reshape(B * W, 256).numpy(), f"mha ctx {W} {B} {variant}")
        # backward: autograd of the restated forward given the fp32-rounded probs is not the kernel's contract (it reads the saved probs);
        # with float64 probs the two coincide
        dctx = t64(c["dctx"])
        (g,) = torch.autograd.grad(ctx, qkv, dctx)
        rb = H.attention_bwd_ref(c["qkv"], r["probs"][0], c["dctx"], B, W, c["drop_p"], c["key"])
        close(rb["dqkv"][0], g.numpy(), f"dqkv {W} {B} {variant}")
        if dead:
            rows = np.repeat(c["mask"].all(1), W)
            assert not rb["dqkv"][0][rows].any() and not r["ctx"][0][rows].any() and np.isfinite(r["ctx"][0]).all()
        # fp32 numpy under the bars
        r32 = H.attention_ref(c["qkv"], c["mask"], B, W, c["drop_p"], c["key"], dt=np.float32)
        under(r32, r, ("probs", "ctx"), f"attention {W} {B} {variant}")
        p32 = r32["probs"][0]
        under(H.attention_bwd_ref(c["qkv"], p32, c["dctx"], B, W, c["drop_p"], c["key"], dt=np.float32),
              H.attention_bwd_ref(c["qkv"], p32, c["dctx"], B, W, c["drop_p"], c["key"]), ("dqkv",), f"attention_bwd {W} {B} {variant}")
        if variant == "large":
            assert np.abs(np.einsum("bhid,bhjd->bhij", *[x.astype(np.float64) for x in H._split(c["qkv"], B, W, np.float64)[:2]])).max() * H.QSCALE > (25 if W * B > 4 else 5)


def test_posenc_ref_matches_oracle_head_piece():
    for Q in H.POSENC_Q:
        c = H.make_posenc(Q)
        r = H.posenc_ref(c["gl"], c["cent"], c["w1"], c["b1"], c["w2"], c["b2"])
        cent, w1, b1, w2, b2 = (t64(c[k]) for k in ("cent", "w1", "b1", "w2", "b2"))
        pos = F.leaky_relu(cent @ w1.t() + b1, H.LEAK) @ w2.t() + b2          # oracle.head, pointnetAtt.py:183-185
        close(r["tok"][0], (t64(c["gl"]) + pos).numpy(), f"tok {Q}")
        v = c["cent"].astype(np.float64) @ c["w1"].astype(np.float64).T + c["b1"]
        assert (v == 0).any() and (v < 0).any() and (v > 0).any(), "the case must put hidden units at 0 and on both sides of it"
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "fc1's output must be exact in fp32 for this case"
        under(H.posenc_ref(c["gl"], c["cent"], c["w1"], c["b1"], c["w2"], c["b2"], dt=np.float32), r, ("tok", "hid"), f"posenc {Q}")


LOGIT_CASES = [(C, P, B, ld, cw) for C in H.LOGIT_C for P in H.LOGIT_P for B in H.LOGIT_B for ld, cw in ((C, True), (32, False))]


def test_logits_and_ce_refs_match_torch_cross_entropy():
    for C, P, B, ld, cw in LOGIT_CASES:
        c = H.make_logits(C, P, B, ld, cw)
        r = H.logits_ref(c["z4"], c["R"], P, C, c["targets"], c["class_w"])
        lg = t64(r["logits"]).requires_grad_(True)
        tt = torch.from_numpy(np.where(H.live_targets(c["targets"], C), c["targets"], -1)).reshape(B, P)
        w = None if c["class_w"] is None else t64(c["class_w"])
        ce = F.cross_entropy(lg, tt, weight=w, ignore_index=-1)
        close(r["loss2"][0][0], ce.item(), f"ce {C} {P} {B}")
        ce_o, _ = O.loss_terms(lg.detach(), tt, torch.eye(64, dtype=torch.float64)[None], class_w=tuple(np.ones(C) if w is None else w.numpy()))
        close(r["loss2"][0][0], ce_o.item(), f"oracle ce {C} {P} {B}")
        assert np.array_equal(r["preds"], O.predictions(lg.detach()).reshape(-1).numpy()), "first maximum"
        for gs in (1.0, 0.125):
            (g,) = torch.autograd.grad(ce * gs, lg, retain_graph=True)
            rb = H.ce_bwd_ref(r["logits"], c["targets"], c["class_w"], r["loss2"][0][1], gs)
            close(rb["dlogits"][0], g.numpy(), f"dlogits {C} {P} {B} {gs}")
            wsum32 = np.float32(r["loss2"][0][1])
            under(H.ce_bwd_ref(r["logits"], c["targets"], c["class_w"], wsum32, gs, dt=np.float32),
                  H.ce_bwd_ref(r["logits"], c["targets"], c["class_w"], wsum32, gs), ("dlogits",), f"ce_bwd {C} {P} {B}")
        r32 = H.logits_ref(c["z4"], c["R"], P, C, c["targets"], c["class_w"], dt=np.float32)
        under(r32, r, ("loss_part",), f"logits {C} {P} {B}")
        # argmax rows: the logits are inputs (bar 0), so no row is excluded -- the cap of 0.1 % holds with 0 rows
        assert np.array_equal(r32["preds"], r["preds"])
        assert r["loss2"][0][1] == float(np.float32(r["loss2"][0][1])), "the weight sum must be exact in fp32 for the consistency test"


HOB_CASES = list(itertools.product(H.HOB_R, H.HOB_C, (0.0, 0.3), (0, 1)))


def test_head_out_bwd_ref_matches_autograd_and_keeps_the_cap():
    for R, C, dp, zb in HOB_CASES:
        c = H.make_head_out(R, C, dp, zb)
        args = (c["dlogits"], c["zread"], c["scale"], c["shift"], c["mean"], c["invstd"], c["w4"], c["P"], dp, c["key"])
        r = H.head_out_bwd_ref(*args)
        excluded = (~r["sure"]).sum()
        assert excluded <= 1e-3 * R * 64, f"head_out {R} {C} {dp} {zb}: {excluded} undecided elements"
        # autograd of conv_4(dropout(relu(bn_3(z3)))) wrt the bn_3 output, W4 and b4 (oracle.head's last lines)
        y = (t64(c["zread"]) * t64(c["scale"]) + t64(c["shift"])).requires_grad_(True)
        w4 = t64(c["w4"]).requires_grad_(True)
        b4 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        keep = t64(H.keep_flat(c["key"], R * 64, dp).reshape(R, 64).astype(np.float64))
        ds = H.PP.dscale32(dp) if dp > 0 else 1.0
        out = (torch.relu(y) * keep * ds) @ w4.t() + b4
        d = t64(c["dlogits"]).transpose(1, 2).reshape(R, C)
        gy, gw, gb = torch.autograd.grad(out, (y, w4, b4), d)
        close(r["dy3"][0], gy.numpy(), "dy3")
        close(r["dW4"][0], gw.numpy(), "dW4")
        close(r["db4"][0], gb.numpy(), "db4")
        zh = (c["zread"].astype(np.float64) - c["mean"]) * c["invstd"]
        close(r["part_a"][0], gy.numpy().sum(0), "part_a")
        close(r["part_b"][0], (gy.numpy() * zh).sum(0), "part_b")
        r32 = H.head_out_bwd_ref(*args, dt=np.float32)
        s = r["sure"]
        assert H.worst(np.where(s, r32["dy3"][0], 0), (np.where(s, r["dy3"][0], 0), r["dy3"][1])) <= 1.0
        under(r32, r, ("dW4", "db4", "part_a", "part_b"), f"head_out {R} {C} {dp} {zb}")
        assert (c["scale"] < 0).any()


def test_linear_and_reg_refs():
    for rows, (no, ni) in itertools.product(H.LIN_ROWS, H.LIN_SHAPES):
        c = H.make_linear(rows, no, ni, 320 if ni == 256 else ni)
        W = c["Wl"][:, :ni]
        r = H.linear_bwd_ref(c["G"], c["X"], W, c["dx_mul"])
        x = t64(c["X"]).requires_grad_(True)
        w = t64(W).requires_grad_(True)
        b = torch.zeros(no, dtype=torch.float64, requires_grad=True)
        pre = x * 1.0
        y = pre @ w.t() + b
        gx, gw, gb = torch.autograd.grad(y, (pre, w, b), t64(c["G"]))
        close(r["dW"][0], gw.numpy(), "dW")
        close(r["db"][0], gb.numpy(), "db")
        close(r["dX"][0], (gx * t64(c["dx_mul"])).numpy(), "dX")
        under(H.linear_bwd_ref(c["G"], c["X"], W, c["dx_mul"], dt=np.float32), r, ("dW", "db", "dX"), f"linear {rows} {no} {ni}")
    for n, kind in ((1, "mixed"), (5, "mixed"), (64, "mixed"), (5, "zero")):
        Fm = H.make_reg(n, kind)
        r = H.reg_fwd_ref(Fm)
        ft = t64(Fm).requires_grad_(True)
        _, reg = O.loss_terms(torch.zeros(1, 2, 1, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.int64), ft, class_w=(1.0, 1.0))
        close(r["reg"][0], [reg.item()], f"reg {n} {kind}")
        if kind == "zero":
            assert r["reg"][0][0] == 0.0 and not H.reg_bwd_ref(Fm, r["G"][0], 0.0, 0.5)["dF"][0].any()
            continue
        assert n == 1 or not r["G"][0][-1].any(), "the last matrix is exactly orthogonal"
        (g,) = torch.autograd.grad(reg * 0.5, ft)
        close(H.reg_bwd_ref(Fm, r["G"][0], r["reg"][0][0], 0.5)["dF"][0], g.numpy(), "d reg")
        r32 = H.reg_fwd_ref(Fm, dt=np.float32)
        under(r32, r, ("G", "part", "reg"), f"reg {n}")
        dF0 = H.f32(np.random.default_rng(n).standard_normal(Fm.shape))
        a = (Fm, r32["G"][0], r32["reg"][0][0], 0.5, dF0)
        under(H.reg_bwd_ref(*a, dt=np.float32), H.reg_bwd_ref(*a), ("dF",), f"reg bwd {n}")


def test_adam_ref_matches_oracle_and_torch_adam():
    hy = {k: float(np.float32(v)) for k, v in H.ADAM_HYPER.items()}
    for step, gs in itertools.product(H.ADAM_STEPS, (1.0, 0.125)):
        for p, g, m, v in H.make_adam(7, seed=step, big_at=3):
            r = H.adam_ref(p, g, m, v, step, gscale=gs, **H.ADAM_HYPER)
            po, mo, vo = t64(p).clone(), t64(m).clone(), t64(v).clone()
            O.adam_step(po, t64(g) * gs, mo, vo, step, **hy)
            close(r["p"][0], po.numpy(), "oracle p")
            close(r["m"][0], mo.numpy(), "oracle m")
            close(r["v"][0], vo.numpy(), "oracle v")
            pt = torch.nn.Parameter(t64(p).clone())
            opt = torch.optim.Adam([pt], lr=hy["lr"], betas=(hy["b1"], hy["b2"]), eps=hy["eps"])
            pt.grad = t64(g) * gs
            opt.state[pt] = {"step": torch.tensor(float(step - 1)), "exp_avg": t64(m).clone(), "exp_avg_sq": t64(v).clone()}
            opt.step()
            close(r["p"][0], pt.detach().numpy(), "torch p")
            close(r["m"][0], opt.state[pt]["exp_avg"].numpy(), "torch m")
            close(r["v"][0], opt.state[pt]["exp_avg_sq"].numpy(), "torch v")
            # adam_kernel's own expression order in fp32 numpy
            f = np.float32
            gi = g * f(gs)
            mi = f(hy["b1"]) * m + (f(1) - f(hy["b1"])) * gi
            vi = f(hy["b2"]) * v + (f(1) - f(hy["b2"])) * gi * gi
            ss, isb = f(hy["lr"] / (1 - hy["b1"] ** step)), f(1 / math.sqrt(1 - hy["b2"] ** step))
            pn = p - ss * mi / (np.sqrt(vi) * isb + f(hy["eps"]))
            for name, x in (("p", pn), ("m", mi), ("v", vi)):
                assert H.worst(x, r[name]) <= 1.0, f"adam {name} step {step}: fp32 numpy over the bar"
            assert np.all(np.sign(m) * np.sign(g) >= 0), "m carries the sign of g (adam_ref)"


def test_pad_mask_cases():
    for W in H.PAD_W:
        for P in H.pad_P(W):
            assert P % W == 0 and P >= W
            t = H.make_pad_targets(3, P, W)
            m = H.pad_mask_ref(t, W)
            assert m[0, 0] == 1 and m[2].all() and (W == 1 or m[0, W - 1] == 0)
    assert any(P > 8192 for W in H.PAD_W for P in H.pad_P(W)) and any(P % 1024 for W in H.PAD_W for P in H.pad_P(W))
