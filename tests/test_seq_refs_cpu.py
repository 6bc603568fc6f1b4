"""The float64 restatements of tests/seq_probe.py against torch in float64 -- torch.nn.GRU(256 -> 64) and its autograd (ops 0 and 1), autograd of
the literal .view(-1, W, 256) + contraction (ops 2 and 6), a plain mean over the heads (op 3), F.batch_norm and its running update (op 4), F.linear
(op 5) -- then: every bar is positive, the fp32 numpy evaluation of every restatement stays inside its own bar on all the committed case inputs,
and the ReLU-undecided share of every case stays under 1 %.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import seq_probe as S

RTOL = 1e-11


def close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    assert float(np.abs(a - b).max() if a.size else 0.0) <= rtol * scale, (what, float(np.abs(a - b).max()), scale)


def under(res32, res64, names, what):
    for n in names:
        assert np.all(S.f64(res64[n][1]) >= 0), f"{what} {n}: negative bar"
        r = S.worst(res32[n][0], res64[n])
        assert r <= 1.0, f"{what} {n}: fp32 numpy evaluation at {r:.3f} of the bar"


def positive(res, names, what):
    for n in names:
        assert np.all(S.f64(res[n][1]) > 0), f"{what} {n}: a bar is not positive"


def t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def torch_gru(c, dH=None):
    """nn.GRU(256 -> 64, batch_first) in float64 fed x with W_ih x + b_ih = the case's gi (W_ih = [I_192 | 0], b_ih = 0, x = [gi | 0]): its output,
    and with dH its autograd gradients of the four parameters and of x (whose first 192 columns are d(gi))."""
    B, W = c["B"], c["W"]
    gru = torch.nn.GRU(256, S.H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.zero_()
        gru.weight_ih_l0[:, :S.G3] = torch.eye(S.G3, dtype=torch.float64)
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(t64(c["Whh"]))
        gru.bias_hh_l0.copy_(t64(c["bhh"]))
    x = torch.zeros(B, W, 256, dtype=torch.float64)
    x[:, :, :S.G3] = t64(c["gi"]).reshape(B, W, S.G3)
    x.requires_grad_(True)
    out, _ = gru(x)
    if dH is None:
        return out.detach().numpy(), None
    out.backward(t64(dH).reshape(B, W, S.H))
    return out.detach().numpy(), dict(x=x.grad.numpy(), wih=gru.weight_ih_l0.grad.numpy(), whh=gru.weight_hh_l0.grad.numpy(),
                                      bih=gru.bias_ih_l0.grad.numpy(), bhh=gru.bias_hh_l0.grad.numpy())


def manual_gru(c, dH):
    """The cell written with torch ops, gh = W_hh h + b_hh kept per step: autograd's gradient AT gh and at gi."""
    B, W = c["B"], c["W"]
    gi = t64(c["gi"]).reshape(B, W, S.G3).requires_grad_(True)
    Whh, bhh = t64(c["Whh"]), t64(c["bhh"])
    h = torch.zeros(B, S.H, dtype=torch.float64)
    ghs, hs = [], []
    for t in range(W):
        gh = (h @ Whh.t() + bhh).requires_grad_(True)
        gh.retain_grad()
        r = torch.sigmoid(gi[:, t, :S.H] + gh[:, :S.H])
        z = torch.sigmoid(gi[:, t, S.H:2 * S.H] + gh[:, S.H:2 * S.H])
        n = torch.tanh(gi[:, t, 2 * S.H:] + r * gh[:, 2 * S.H:])
        h = (1.0 - z) * n + z * h
        ghs.append(gh)
        hs.append(h)
    out = torch.stack(hs, 1)
    out.backward(t64(dH).reshape(B, W, S.H))
    return out.detach().numpy(), gi.grad.numpy().reshape(B * W, S.G3), torch.stack([g.grad for g in ghs], 1).numpy().reshape(B * W, S.G3)


def test_gru_forward_ref_matches_torch_gru():
    for B in S.GRU_B:
        for W in S.GRU_W:
            for variant in S.GRU_VARIANTS:
                c = S.make_gru(B, W, variant)
                r = S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W)
                out, _ = torch_gru(c)
                close(r["h"][0], out, f"gru h {B} {W} {variant}")
                positive(r, ("r", "z", "n", "ghn", "h"), f"gru {B} {W} {variant}")
                r32 = S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W, dt=np.float32)
                under(r32, r, ("r", "z", "n", "ghn", "h"), f"gru chained {B} {W} {variant}")
                # step-local from the fp32 evaluation's own states, as the GPU test does from the kernel's
                h32 = S.f32(r32["h"][0]).reshape(B * W, S.H)
                loc = S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W, h_given=h32)
                under(S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W, h_given=h32, dt=np.float32), loc, ("r", "z", "n", "ghn", "h"),
                      f"gru step-local {B} {W} {variant}")
                if variant == "saturated":
                    assert np.all(np.isfinite(r32["h"][0]))
                    big = np.abs(c["gi"].reshape(B, W, S.G3)[:, :, :21]) == 100.0
                    assert big.all() and np.all(np.isin(r32["r"][0][:, :, :21], (0.0, 1.0))), "fp32 sigmoid at +-100 (+- |gh| < 11) is exactly 0 or 1"
                    assert np.all(np.abs(r32["n"][0][:, :, :21]) == 1.0)


def test_gru_backward_ref_matches_torch_autograd():
    for B in S.GRU_B:
        for W in S.GRU_W:
            for variant in S.GRU_BWD_VARIANTS:
                c = S.make_gru_bwd(B, W, variant)
                fw = S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W)
                h_last = S.f64(fw["h"][0])[:, -1]
                assert (np.abs(h_last) > 0.5).mean() > 0.6, "the last hidden state of every sample is far from 0"
                if variant == "small_r":
                    assert S.f64(fw["r"][0]).max() < 0.25, "small_r: r far from 1 everywhere"
                # float64 gates and states (not rounded) into the restatement: equals autograd exactly
                g64 = np.concatenate([S.f64(fw[k][0]) for k in ("r", "z", "n", "ghn")], axis=2).reshape(B * W, 4 * S.H)
                h64 = S.f64(fw["h"][0]).reshape(B * W, S.H)
                r = S.gru_bwd_ref(c["dH"], g64, h64, c["Whh"], B, W)
                out, dgi, dgh = manual_gru(c, c["dH"])
                tout, tg = torch_gru(c, c["dH"])
                close(out, tout, f"manual cell vs nn.GRU {B} {W} {variant}")
                close(r["dgi"][0], dgi, f"dgi {B} {W} {variant}", 1e-10)
                close(r["dgh"][0], dgh, f"dgh {B} {W} {variant}", 1e-10)
                close(r["dgi"][0], tg["x"].reshape(B * W, 256)[:, :S.G3], f"dgi vs nn.GRU {B} {W} {variant}", 1e-10)
                close(r["dgi"][0].sum(0), tg["bih"], f"db_ih {B} {W} {variant}", 1e-10)
                close(r["dgh"][0].sum(0), tg["bhh"], f"db_hh {B} {W} {variant}", 1e-10)
                close(r["dgh"][0].T @ S.f64(r["hprev"][0]), tg["whh"], f"dW_hh {B} {W} {variant}", 1e-10)
                hp = S.f64(r["hprev"][0]).reshape(B, W, S.H)
                assert not hp[:, 0].any() and np.array_equal(hp[:, 1:], h64.reshape(B, W, S.H)[:, :-1])
                # the committed (fp32-rounded) tape: fp32 evaluation under the bars
                r64 = S.gru_bwd_ref(c["dH"], c["gates"], c["h_all"], c["Whh"], B, W)
                if variant != "last_only":
                    positive(r64, ("dgi", "dgh"), f"gru_bwd {B} {W} {variant}")
                under(S.gru_bwd_ref(c["dH"], c["gates"], c["h_all"], c["Whh"], B, W, dt=np.float32), r64, ("dgi", "dgh", "hprev"),
                      f"gru_bwd {B} {W} {variant}")
                if variant == "last_only" and W > 1:
                    assert np.abs(r64["dgi"][0].reshape(B, W, S.G3)[:, 0]).max() > 0, "the gradient reaches step 0 through the recurrence"


def test_sweep_refs_under_their_bars_in_fp32():
    x = S.sweep_points()
    assert 4000 <= len(x) <= 4200 and x.min() == -90.0 and x.max() == 90.0 and (np.abs(x) < 1e-3).sum() > 500
    s, bs = S.sigmoid_ref(x)
    n, bn = S.tanh_ref(x)
    close(s, torch.sigmoid(t64(x)).numpy(), "sigmoid")
    close(n, torch.tanh(t64(x)).numpy(), "tanh")
    assert np.all(bs > 0) and np.all(bn > 0)
    assert S.worst(S.sigmoid_ref(x, dt=np.float32)[0], (s, bs)) <= 1.0
    assert S.worst(S.tanh_ref(x, dt=np.float32)[0], (n, bn)) <= 1.0


def view_contract(o, cw, cb, B, W):
    """autograd of the literal reference lines: attn_output [W, B, 256] -> .view(-1, W, 256) -> conv_1 (Conv1d(W -> 1, 1)) -> relu."""
    o_t = t64(o).requires_grad_(True)                                         # [B * W, 256], token (b, w) at row b W + w
    cw_t, cb_t = t64(cw).requires_grad_(True), t64(cb).requires_grad_(True)
    attn_output = o_t.reshape(B, W, 256).transpose(0, 1).contiguous()         # sequence-first, as nn.MultiheadAttention returns it
    x = torch.relu(F.conv1d(attn_output.view(-1, W, 256), cw_t.reshape(1, W, 1), cb_t.reshape(1))).reshape(B, 256)
    return o_t, cw_t, cb_t, x


def test_cls_mix_refs_match_autograd_of_the_view():
    for B, W in S.CLS_BW:
        c = S.make_cls_mix(B, W)
        r = S.cls_mix_ref(c["o"], c["cw"], c["cb"], B, W)
        o_t, cw_t, cb_t, x = view_contract(c["o"], c["cw"], c["cb"], B, W)
        close(np.maximum(r["pre"][0], 0), x.detach().numpy(), f"cls_mix {B} {W}")
        assert (~r["sure"]).sum() <= 0.01 * B * 256, "ReLU-undecided share over 1 %"
        assert r["zero"][:, [5, 77]].all() == (B % 2 == 0) and np.all(r["pre"][0][r["zero"]] == 0)
        assert np.all(r["pre"][1][~r["zero"]] > 0)
        r32 = S.cls_mix_ref(c["o"], c["cw"], c["cb"], B, W, dt=np.float32)
        assert S.worst(r32["pre"][0], r["pre"]) <= 1.0
        # backward: the committed x is the rounded forward, so x > 0 decides as autograd's ReLU does
        assert np.array_equal(c["x"] > 0, x.detach().numpy() > 0)
        x.backward(t64(c["dx"]))
        rb = S.cls_mix_bwd_ref(c["dx"], c["x"], c["o"], c["cw"], B, W)
        close(rb["d_o"][0], o_t.grad.numpy(), f"d_o {B} {W}")
        close(rb["cwpart"][0][:, :W].sum(0), cw_t.grad.numpy(), f"d cw {B} {W}")
        close(rb["cwpart"][0][:, W].sum(), cb_t.grad.numpy()[0], f"d cb {B} {W}")
        under(S.cls_mix_bwd_ref(c["dx"], c["x"], c["o"], c["cw"], B, W, dt=np.float32), rb, ("d_o", "cwpart"), f"cls_mix_bwd {B} {W}")
        assert (c["x"] == 0).any() and (c["cw"] < 0).any() and (W == 1 or (c["cw"] == 0).any())


def test_cls_weights_ref_is_the_mean_over_heads():
    from oracle.ampnet_oracle import keep_mask
    for B, W in S.CLS_WEIGHTS_BW:
        c = S.make_cls_weights(B, W)
        assert W == 1 or (c["probs"] == 0).any()
        for p in (0.0, 0.3):
            r = S.cls_weights_ref(c["probs"], B, W, p, c["key"])
            a = t64(c["probs"])
            if p > 0:
                a = a * t64(keep_mask(c["key"][0], c["key"][1], a.numel(), p).reshape(a.shape).astype(np.float64)) * S.PP.dscale32(p)
            close(r["out"][0], a.mean(1).numpy(), f"cls_weights {B} {W} {p}")
            under(S.cls_weights_ref(c["probs"], B, W, p, c["key"], dt=np.float32), r, ("out",), f"cls_weights {B} {W} {p}")


def test_cls_bn_act_ref_matches_batch_norm():
    for B in S.BN_B:
        c = S.make_cls_bn(B)
        for train in (0, 1):
            r = S.cls_bn_act_ref(c["z"], c["b2"], c["gamma"], c["beta"], c["rmean"], c["rvar"], B, train)
            v = t64(r["v"][0])
            assert np.array_equal(r["v"][0], c["z"] + c["b2"][None, :]), "z + b2 with one fp32 rounding"
            rm, rv = t64(c["rmean"]).clone(), t64(c["rvar"]).clone()
            if train and B == 1:                      # F.batch_norm refuses one row in train mode: the definition by hand
                y = t64(c["beta"])[None, :].expand(1, -1)
                rm, rv = S.MOM9 * rm + S.MOM1 * v[0], S.MOM9 * rv
            else:
                y = F.batch_norm(v, rm, rv, t64(c["gamma"]), t64(c["beta"]), bool(train), S.MOM1, S.BN_EPS)
            close(np.maximum(r["pre"][0], 0), torch.relu(y).numpy(), f"act {B} {train}", 1e-9)
            # torch's running update is (1 - 0.1) r + 0.1 s in float64; the kernel's constants are 0.9f and 0.1f
            close(r["rmean"][0], rm.numpy(), f"rmean {B} {train}", 1e-7)
            close(r["rvar"][0], rv.numpy(), f"rvar {B} {train}", 1e-7)
            if train and B == 1:
                assert np.all(r["invstd"][0] == 1.0 / np.sqrt(1e-5)) and np.array_equal(r["rvar"][0], S.MOM9 * S.f64(c["rvar"]))
            names = ("scale", "shift", "mean", "invstd", "pre", "rmean", "rvar")
            for n in ("scale", "shift", "invstd", "pre"):
                nz = S.f64(r[n][0]) != 0
                assert np.all(np.broadcast_to(r[n][1], nz.shape)[nz] > 0), n
            under(S.cls_bn_act_ref(c["z"], c["b2"], c["gamma"], c["beta"], c["rmean"], c["rvar"], B, train, dt=np.float32), r, names, f"cls_bn_act {B} {train}")
            assert (~r["sure"]).sum() <= 0.01 * B * S.CLS_HID, "ReLU-undecided share over 1 %"
        z7 = S.f64(c["z"][:, 7] + c["b2"][7])
        assert B == 1 or z7.mean() ** 2 > 1e6 * z7.var()
        assert (c["gamma"] < 0).any() and c["gamma"][3] == 0


def test_cls_out_ref_is_linear():
    for B in S.OUT_B:
        for C in S.OUT_C:
            c = S.make_cls_out(B, C)
            r = S.cls_out_ref(c["act"], c["W3"], c["b3"])
            close(r["out"][0], F.linear(t64(c["act"]), t64(c["W3"]), t64(c["b3"])).numpy(), f"cls_out {B} {C}")
            positive(r, ("out",), f"cls_out {B} {C}")
            under(S.cls_out_ref(c["act"], c["W3"], c["b3"], dt=np.float32), r, ("out",), f"cls_out {B} {C}")
