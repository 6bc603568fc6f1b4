"""Layer-local float64 parity of the GRU recurrence (gru_seq_kernel, gru_seq_bwd_kernel) and of the classification head's own kernels
(cls_mix_kernel, cls_weights_kernel, cls_bn_act_kernel, cls_out_kernel, cls_mix_bwd_kernel).

Each case launches ONE kernel through ampnet_probe_seq_f32 (include/ampnet_hip.h, "test hooks"), which goes through the launch wrappers the product
entry points call, on inputs of tests/seq_probe.py and holds every output to the float64 restatement there, at the bars of that module's
docstring.  Every case also checks: outputs pre-filled with NaN (8 tail elements) are finite where the contract writes and keep their sentinel
bits elsewhere; a second run on re-poisoned outputs (in-place operands restored) is bitwise identical; the probe recorded the intended kernel.

The recurrence's forward is checked step-local (step t of the restatement starts from the kernel's own fp32 h_{t-1}: one-step bars for r, z, n,
gh_n, h) and chained from h = 0 with the bar carried step to step (the check that notices a drift); the backward chained only.

tanhf / sigmoid sweep (test_tanh_sigmoid_sweep, 4105 points of [-90, 90]): tanhf 1.76 eps worst relative error (at x = 0.655), 0.44 of its bar
TANH_ULP eps |n| + 2^-126 with the assumed TANH_ULP = 4: under 0.5, the 4 stands.  The kernel's sigmoid 1 / (1 + __expf(-x)): 63.6 eps worst
relative error (at x = -86.8, where s ~ e^x and the error is __expf's), 0.46 of its bar with head_probe.FAST_EXP_ULP = 21: stands too.
Observed worst error/bar on the MI355X: gru_seq step-local r 0.31, z 0.32, n 0.16, gh_n 0.06, h 0.22; chained r 0.15, z 0.10, n 0.16, gh_n 0.03,
h 0.12; gru_seq_bwd d(gi) r 0.45 / z 0.46 / n 0.48, d(gh) r 0.45 / z 0.46 / n 0.48; cls_mix x 0.08; cls_mix_bwd d_o 0.10, cwpart 0.006, bias column
0.003; cls_weights 0.13; cls_bn_act scale 0.08, shift 0.09, mean 0.09, invstd 0.10, act 0.06, rmean 0.54, rvar 0.47; cls_out 0.01.  No kernel finding.
Scratch-build mutations (not committed), each failing its tests here and in the entry-level edge-shape tests:
(a) h_{t-1} at t = 0 read from h_all[q - 1] (guarded for q = 0, which would read before the buffer): all 15 test_gru_seq_bwd cases with B = 3
    ("h_{t-1} at t = 0 is not +0"), and test_gru_head_edge_shapes_match_oracle for B > 1 (global_seq gradient 3e-2 .. 1.1e-1 against 2e-2);
(b) the n-third of d(gh) written as dnp: all 30 test_gru_seq_bwd cases (d(gh) n at 7.8e6 .. 3.8e9 of the bar) and every edge-shape case with a
    backward (weight_hh_l0 / bias_hh_l0 gradients at 40 .. 1100 x their allowance);
(c) rowmap returning (f / B) * W + f % B (taken modulo B W: as written it leaves the buffer where W > B): the 7 test_cls_mix_and_bwd cases other
    than (1, 1) (x at 2.5e5 .. 8.5e6 of the bar) and the 4 test_cls_head_edge_shapes_match_oracle cases with W > 1 (out 5 .. 340 x its allowance);
(d) q / B for q / (B - 1) in cls_bn_act's running variance: the 4 train cases with B > 1 of test_cls_bn_act (rvar at 3.3e4 .. 5.8e5 of the bar);
(e) sW[j * GRU_H + k] for sW[k * GRU_H + j] in the backward's r-gate term: the 24 test_gru_seq_bwd cases with W > 1 (d(gi) r at 570 .. 1.6e4 of the
    bar) and every edge-shape case with a backward (weight_ih_l0 and the recurrence's gradients).
"""
import numpy as np
import pytest
import torch

import pw_probe as PP
import seq_probe as S

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
TAIL = 8
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[gru cls layers] worst error/bar {k}: {WORST[k]:.4f}")


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def nanbuf(n):
    """n elements the contract may write + TAIL it must not."""
    return torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")


def is_sentinel(t):
    return bool((t.detach().cpu().view(torch.int32) == NAN_BITS).all())


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def launch(d, outs, restore=()):
    """run, check the recorded kernel, re-poison the outputs (and restore the in-place operands), run again: bitwise equal.  outs: {name: (tensor,
    written elements)}; restore: [(tensor, original)].  Checks finite where written and the tail's sentinel.  The outputs hold the second run."""
    want = [S.KERNEL[d.op]]
    rc, names = S.run(d)
    assert rc == 0, PP.last_error()
    assert names == want, (names, want)
    first = {k: v.detach().cpu().clone() for k, (v, _) in outs.items()}
    for v, _ in outs.values():
        v.fill_(float("nan"))
    for t, orig in restore:
        t.copy_(orig)
    rc, _ = S.run(d)
    assert rc == 0, PP.last_error()
    for k, (v, n) in outs.items():
        assert torch.equal(first[k].view(torch.int32), v.detach().cpu().view(torch.int32)), f"{k}: second run differs bitwise"
        assert bool(torch.isfinite(v[:n]).all()), f"{k}: non-finite where the contract writes"
        assert is_sentinel(v[n:]), f"{k}: written past its extent"


# ---- tanhf / sigmoid --------------------------------------------------------------------------------------------------------------------
def test_tanh_sigmoid_sweep():
    x = S.sweep_points()
    d = S.new("sweep", rows=len(x))
    y = nanbuf(2 * len(x))
    S.set_tensors(d, X=dev(x), Y=y)
    launch(d, dict(Y=(y, 2 * len(x))))
    got = host(y[:2 * len(x)]).astype(np.float64).reshape(2, -1)
    x64 = x.astype(np.float64)
    for row, (name, ref, c) in enumerate((("tanhf", S.tanh_ref, S.TANH_ULP), ("sigmoid", S.sigmoid_ref, S.FAST_EXP_ULP))):
        want, b = ref(x)
        r = S.worst(got[row], (want, b))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(np.abs(want) > 2.0 ** -126, np.abs(got[row] - want) / np.abs(want), 0.0)
        at = int(np.argmax(rel))
        print(f"[gru cls layers] {name}: worst error {r:.4f} of its bar (constant {c:g}); worst relative error {rel.max() / S.EPS:.3f} eps at x = {x64[at]:.6g}")
        note(f"sweep {name}", r)
        assert r <= 0.5, f"{name}: {r:.4f} of the bar; the bars assume <= 0.5"
    big = np.abs(x64) >= 89.0
    assert np.all(np.isin(got[1][big], (0.0, 1.0))), "|x| >= 89: __expf overflows or vanishes, the sigmoid is exactly 0 or 1"
    assert np.all(np.abs(got[0][np.abs(x64) >= 20.0]) == 1.0), "|x| >= 20: tanhf is exactly +-1"
    assert got[0][x64 == 0][0] == 0.0 and got[1][x64 == 0][0] == 0.5


# ---- the recurrence, forward -----------------------------------------------------------------------------------------------------------------
def run_gru(c, B, W, want_gates=True, rows=None):
    gi = c["gi"] if rows is None else c["gi"][rows]
    d = S.new("gru_seq", B=B, W=W)
    h, g = nanbuf(B * W * S.H), nanbuf(B * W * 4 * S.H)
    S.set_tensors(d, gi=dev(gi), Whh=dev(c["Whh"]), bhh=dev(c["bhh"]), h_out=h, gates=g if want_gates else None)
    launch(d, dict(h_out=(h, B * W * S.H), gates=(g, B * W * 4 * S.H if want_gates else 0)))
    return host(h[:B * W * S.H]).reshape(B * W, S.H), host(g[:B * W * 4 * S.H]).reshape(B, W, 4, S.H)


@pytest.mark.parametrize("variant", S.GRU_VARIANTS)
@pytest.mark.parametrize("W", S.GRU_W)
@pytest.mark.parametrize("B", S.GRU_B)
def test_gru_seq(B, W, variant):
    c = S.make_gru(B, W, variant)
    h, g = run_gru(c, B, W)
    got = dict(r=g[:, :, 0], z=g[:, :, 1], n=g[:, :, 2], ghn=g[:, :, 3], h=h.reshape(B, W, S.H))
    local = S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W, h_given=h)
    chained = S.gru_fwd_ref(c["gi"], c["Whh"], c["bhh"], B, W)
    for k in ("r", "z", "n", "ghn", "h"):
        assert note(f"gru_seq {k} step-local", S.worst(got[k], local[k])) <= 1.0, (k, "step-local")
        assert note(f"gru_seq {k} chained", S.worst(got[k], chained[k])) <= 1.0, (k, "chained")
    if variant == "saturated":
        gi = c["gi"].reshape(B, W, S.G3)
        for name, base in (("r", 0), ("z", S.H)):
            at100 = got[name][:, :, :21]
            assert np.array_equal(at100, (gi[:, :, base:base + 21] > 0).astype(np.float32)), f"{name} at +-100: exactly 0 or 1"
            at30 = got[name][:, :, 21:42]
            pos = gi[:, :, base + 21:base + 42] > 0
            assert np.all(at30[pos] == 1.0) and np.all((at30[~pos] >= 0) & (at30[~pos] < 1e-8)), f"{name} at +-30"
        assert np.array_equal(got["n"][:, :, :21], np.sign(gi[:, :, 2 * S.H:2 * S.H + 21])), "n at +-30: exactly +-1"
    # gates = NULL: the same h, bit for bit, and nothing written to gates (launch() checked its sentinel)
    h2, _ = run_gru(c, B, W, want_gates=False)
    assert np.array_equal(bits(h2), bits(h)), "h_out without gates differs from the run with gates"
    # every sample alone: the same bits (a sample starts from h = 0, not from its predecessor's last state)
    if B > 1:
        for b in range(B):
            hb, gb = run_gru(c, 1, W, rows=slice(b * W, (b + 1) * W))
            assert np.array_equal(bits(hb), bits(h[b * W:(b + 1) * W])) and np.array_equal(bits(gb[0]), bits(g[b])), f"sample {b} alone differs"


# ---- the recurrence, backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.GRU_BWD_VARIANTS)
@pytest.mark.parametrize("W", S.GRU_W)
@pytest.mark.parametrize("B", S.GRU_B)
def test_gru_seq_bwd(B, W, variant):
    c = S.make_gru_bwd(B, W, variant)
    Q = B * W
    d = S.new("gru_seq_bwd", B=B, W=W)
    dgi, dgh, hp = nanbuf(Q * S.G3), nanbuf(Q * S.G3), nanbuf(Q * S.H)
    S.set_tensors(d, dH=dev(c["dH"]), gates=dev(c["gates"]), h_all=dev(c["h_all"]), Whh=dev(c["Whh"]), dgi=dgi, dgh=dgh, hprev_out=hp)
    launch(d, dict(dgi=(dgi, Q * S.G3), dgh=(dgh, Q * S.G3), hprev_out=(hp, Q * S.H)))
    gi_, gh_, hp_ = host(dgi[:Q * S.G3]).reshape(Q, S.G3), host(dgh[:Q * S.G3]).reshape(Q, S.G3), host(hp[:Q * S.H]).reshape(B, W, S.H)
    # h_{t-1}: exactly 0 at t = 0 of EVERY sample (the previous sample's last state is far from 0), else the bits of h_all's previous row
    ha = c["h_all"].reshape(B, W, S.H)
    assert (np.abs(ha[:, -1]) > 0.5).mean() > 0.6
    assert not bits(hp_[:, 0]).any(), "h_{t-1} at t = 0 is not +0"
    assert np.array_equal(bits(hp_[:, 1:]), bits(ha[:, :-1])), "h_{t-1} is not h_all's previous row"
    r = S.gru_bwd_ref(c["dH"], c["gates"], c["h_all"], c["Whh"], B, W)
    assert np.array_equal(bits(gi_[:, :2 * S.H]), bits(gh_[:, :2 * S.H])), "the r- and z-thirds of d(gi) and d(gh) differ"
    for k, name, got in (("dgi", "d(gi)", gi_), ("dgh", "d(gh)", gh_)):
        for i, third in enumerate("rzn"):
            sl = slice(i * S.H, (i + 1) * S.H)
            assert note(f"gru_seq_bwd {name} {third}", S.worst(got[:, sl], (r[k][0][:, sl], r[k][1][:, sl]))) <= 1.0, (name, third)
    # the n-third of d(gh) is dnp r: one fp32 product of the kernel's own dnp
    rr = c["gates"].reshape(Q, 4, S.H)[:, 0].astype(np.float64)
    prod = gi_[:, 2 * S.H:].astype(np.float64) * rr
    assert np.all(np.abs(gh_[:, 2 * S.H:] - prod) <= S.EPS * np.abs(prod) + 2.0 ** -126), "the n-third of d(gh) is not dnp * r"
    if variant == "small_r":
        assert rr.max() < 0.25
    if variant == "last_only" and W > 1:
        assert np.abs(gi_.reshape(B, W, S.G3)[:, 0]).max() > 0, "the gradient did not reach step 0"


# ---- conv_1 over the re-viewed attention output ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,W", S.CLS_BW)
def test_cls_mix_and_bwd(B, W):
    c = S.make_cls_mix(B, W)
    r = S.cls_mix_ref(c["o"], c["cw"], c["cb"], B, W)
    d = S.new("cls_mix", B=B, W=W)
    x = nanbuf(B * 256)
    o, cw = dev(c["o"]), dev(c["cw"])
    S.set_tensors(d, o=o, cw=cw, cb=dev(c["cb"]), x=x)
    launch(d, dict(x=(x, B * 256)))
    got = host(x[:B * 256]).reshape(B, 256)
    assert (~r["sure"]).sum() <= 0.01 * B * 256
    assert note("cls_mix x", S.worst_relu(got, r["pre"], r["sure"])) <= 1.0
    assert not got[r["zero"]].any() and (B % 2 == 1 or r["zero"].any()), "a pre-activation of exactly 0 gives x == 0"
    rb = S.cls_mix_bwd_ref(c["dx"], c["x"], c["o"], c["cw"], B, W)
    d2 = S.new("cls_mix_bwd", B=B, W=W)
    d_o, part = nanbuf(B * W * 256), nanbuf(B * (W + 1))
    S.set_tensors(d2, dx=dev(c["dx"]), x=dev(c["x"]), o=o, cw=cw, d_o=d_o, cwpart=part)
    launch(d2, dict(d_o=(d_o, B * W * 256), cwpart=(part, B * (W + 1))))      # every element of d_o finite: the row map is a bijection
    assert note("cls_mix_bwd d_o", S.worst(host(d_o[:B * W * 256]).reshape(B * W, 256), rb["d_o"])) <= 1.0
    gp = host(part[:B * (W + 1)]).reshape(B, W + 1)
    assert note("cls_mix_bwd cwpart", S.worst(gp[:, :W], (rb["cwpart"][0][:, :W], rb["cwpart"][1][:, :W]))) <= 1.0
    assert note("cls_mix_bwd bias column", S.worst(gp[:, W], (rb["cwpart"][0][:, W], rb["cwpart"][1][:, W]))) <= 1.0


@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("B,W", S.CLS_WEIGHTS_BW)
def test_cls_weights(B, W, drop_p):
    c = S.make_cls_weights(B, W)
    r = S.cls_weights_ref(c["probs"], B, W, drop_p, c["key"])
    d = S.new("cls_weights", B=B, W=W)
    d.drop_p = drop_p
    d.drop_seed = PP.drop_base(*c["key"]) if drop_p > 0 else 0
    out = nanbuf(B * W * W)
    S.set_tensors(d, probs=dev(c["probs"]), wout=out)
    launch(d, dict(wout=(out, B * W * W)))
    got = host(out[:B * W * W]).reshape(B, W, W)
    assert note("cls_weights", S.worst(got, r["out"])) <= 1.0
    assert not got[r["out"][0] == 0].any(), "masked keys (and keys dropped in every head) get exactly 0"


# ---- fc_2's bias + bn_2 + ReLU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("B", S.BN_B)
def test_cls_bn_act(B, train):
    c = S.make_cls_bn(B)
    n = B * S.CLS_HID
    r = S.cls_bn_act_ref(c["z"], c["b2"], c["gamma"], c["beta"], c["rmean"], c["rvar"], B, train)
    d = S.new("cls_bn_act", B=B, train=train)
    z0 = torch.cat([dev(c["z"]).reshape(-1), torch.full((TAIL,), float("nan"), device="cuda")])
    rm0, rv0 = dev(c["rmean"]), dev(c["rvar"])
    z, rm, rv = z0.clone(), rm0.clone(), rv0.clone()
    outs = {k: nanbuf(S.CLS_HID) for k in ("scale", "shift", "mean", "invstd")}
    act = nanbuf(n)
    S.set_tensors(d, z=z, b2=dev(c["b2"]), gamma=dev(c["gamma"]), beta=dev(c["beta"]), rmean=rm, rvar=rv, act=act, **outs)
    launch(d, dict(act=(act, n), **{k: (v, S.CLS_HID) for k, v in outs.items()}), restore=[(z, z0), (rm, rm0), (rv, rv0)])
    assert is_sentinel(z[n:])
    assert np.array_equal(bits(host(z[:n])), bits(r["v"][0].reshape(-1))), "z afterwards is z + bias with one rounding"
    for k in ("scale", "shift", "mean", "invstd"):
        assert note(f"cls_bn_act {k}", S.worst(host(outs[k][:S.CLS_HID]), r[k])) <= 1.0, k
    assert (~r["sure"]).sum() <= 0.01 * n
    assert note("cls_bn_act act", S.worst_relu(host(act[:n]).reshape(B, S.CLS_HID), r["pre"], r["sure"])) <= 1.0
    if train:
        assert note("cls_bn_act rmean", S.worst(host(rm), r["rmean"])) <= 1.0
        assert note("cls_bn_act rvar", S.worst(host(rv), r["rvar"])) <= 1.0
    else:
        assert np.array_equal(bits(host(rm)), bits(c["rmean"])) and np.array_equal(bits(host(rv)), bits(c["rvar"])), "eval mode touched the running statistics"
    if train and B == 1:
        assert np.all(host(outs["invstd"][:S.CLS_HID]) == np.float32(1.0 / np.sqrt(1e-5))), "one row: variance 0"
        assert np.array_equal(host(rv), (np.float32(0.9) * c["rvar"]).astype(np.float32)), "one row: the running variance is updated with 0"
        assert np.array_equal(host(outs["mean"][:S.CLS_HID]), r["v"][0][0])


# ---- fc_3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", S.OUT_C)
@pytest.mark.parametrize("B", S.OUT_B)
def test_cls_out(B, C):
    c = S.make_cls_out(B, C)
    r = S.cls_out_ref(c["act"], c["W3"], c["b3"])
    d = S.new("cls_out", B=B, C=C)
    out = nanbuf(B * C)
    S.set_tensors(d, act=dev(c["act"]), W3=dev(c["W3"]), b3=dev(c["b3"]), out=out)
    launch(d, dict(out=(out, B * C)))
    assert note("cls_out", S.worst(host(out[:B * C]).reshape(B, C), r["out"])) <= 1.0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = {"gru_seq": ("h_out", "gates"), "gru_seq_bwd": ("dgi", "dgh", "hprev_out"), "cls_mix": ("x",), "cls_weights": ("wout",),
           "cls_bn_act": ("scale", "shift", "mean", "invstd", "act", "z", "rmean", "rvar"), "cls_out": ("out",), "cls_mix_bwd": ("d_o", "cwpart"),
           "sweep": ("Y",)}


def sizes(op, B, W, C, rows=5):
    Q = B * W
    return {"gru_seq": dict(gi=Q * 192, Whh=192 * 64, bhh=192, h_out=Q * 64, gates=Q * 256),
            "gru_seq_bwd": dict(dH=Q * 64, gates=Q * 256, h_all=Q * 64, Whh=192 * 64, dgi=Q * 192, dgh=Q * 192, hprev_out=Q * 64),
            "cls_mix": dict(o=Q * 256, cw=W, cb=1, x=B * 256),
            "cls_weights": dict(probs=B * 8 * W * W, wout=B * W * W),
            "cls_bn_act": dict(z=B * 128, b2=128, gamma=128, beta=128, rmean=128, rvar=128, scale=128, shift=128, mean=128, invstd=128, act=B * 128),
            "cls_out": dict(act=B * 128, W3=C * 128, b3=C, out=B * C),
            "cls_mix_bwd": dict(dx=B * 256, x=B * 256, o=Q * 256, cw=W, d_o=Q * 256, cwpart=B * (W + 1)),
            "sweep": dict(X=rows, Y=2 * rows)}[op]


def test_probe_refuses_bad_seq_descriptors():
    """Every buffer of every op one element short, W = 33 for a cls op, C = 17, W = 0 and B = 0 get AMPNET_E_ARG and nothing is written: every
    buffer an op could write (in-place operands included) keeps its sentinel."""
    def attempt(op, B, W, C, short=None, alloc=None, rows=5):
        full = sizes(op, *(alloc or (B, W, C)), rows)
        bufs = {k: torch.full((max(n - (k == short), 1),), float("nan"), dtype=torch.float32, device="cuda") for k, n in full.items()}
        d = S.new(op, B=B, W=W, C=C, rows=rows, train=1)
        S.set_tensors(d, **bufs)
        if short is not None and full[short] == 1:
            setattr(d, short + "_n", 0)                         # a one-element buffer "one short": extent 0 on a live pointer
        rc, names = S.run(d)
        assert rc == S.AMPNET_E_ARG and names == [], (op, B, W, C, short, rc, names)
        assert all(is_sentinel(bufs[k]) for k in OUTPUTS[op]), (op, short)

    B, W, C = 2, 3, 5
    for op in S.OPS:
        for short in sizes(op, B, W, C):
            attempt(op, B, W, C, short)
        attempt(op, 0, W, C, alloc=(B, W, C)) if op != "sweep" else attempt(op, B, W, C, rows=0)
    for op in ("cls_mix", "cls_weights", "cls_mix_bwd"):
        attempt(op, B, 33, C)                                   # buffers sized for W = 33: only the limit refuses
        attempt(op, B, 0, C, alloc=(B, W, C))
    for op in ("gru_seq", "gru_seq_bwd"):
        attempt(op, B, 0, C, alloc=(B, W, C))
    attempt("cls_out", B, W, 17)
    attempt("cls_out", B, W, 0, alloc=(B, W, C))
    d = S.SeqProbe()
    d.op = 8
    assert S.run(d) == (S.AMPNET_E_ARG, [])
