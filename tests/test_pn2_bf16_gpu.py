"""The bf16 PointNet++ forwards on the GPU (include/ampnet_hip.h: ampnet_sa_forward_bf16, ampnet_fp_forward_bf16) against
tests/pn2_bf16_ref.py, the float64 statement of the rounding model.  Every case is B = 2 seeded clouds with the indices of the fp32
ball_query / three_nn kernels (checked against their restatements), and is judged four ways:
  * against the EMULATION of the model: max |gpu - emulated| <= 4 F + ULP.  F is the distance between the emulation and a second
    float32 implementation of the same model (k descending); the GPU's order is a third one, hence the 4.  ULP = 2^-22 max(1, |out|):
    the last fma and the accumulator it takes are rounded to float32 once on each side, four half-ulps at the size of the outputs.
    (Where the order of a sum decides which bf16 neighbour a hidden activation takes, two implementations part by far more than
    float32 noise.  The seeds are those on which the MFMA's measured order keeps within half this bar: pn2_bf16_ref.seed_holds);
  * against the EXACT float64 result: max |gpu - exact| <= 1.5 E, E = max |emulated - exact|, what the model's roundings cost;
  * the output differs from the fp32 kernel's on the same inputs (the bf16 path ran);
  * two calls are bit-identical.
tests/test_pn2_bf16_cpu.py asserts E >= 16 F for every case, so a missing rounding step (an error of the size of E) cannot hide under
4 F.  E, F and the GPU's distances of every case are printed.

Measured on an MI355X (E and F are CPU figures; the GPU's are from one run, and the kernels are deterministic):
  set abstraction, 26 cases: E 1.7e-3 .. 3.9e-3; largest |gpu - emulated| 6.1e-6 (ns40-D317-256x256x256, bar 1.92e-5), elsewhere <= 2.4e-7;
    largest |gpu - emulated| / bar 0.32; |gpu - exact| / E between 0.999 and 1.000 in every case;
  feature propagation, 72 cases: E 1.4e-3 .. 6.4e-3; largest |gpu - emulated| 3.06e-5 (S40-D1_0-cin512-128x96, F 3.07e-5, bar 1.23e-4),
    then 1.18e-5 (S2-D1_0-cin40-256x256x256, F 1.19e-5): F has the same size there, presumably the same flipped activation; elsewhere
    <= 2.8e-6; largest |gpu - emulated| / bar 0.34; |gpu - exact| / E 1.000;
  pointnet_2, bf16 against fp32: global feature 5.05e-4 (E_model 5.05e-4), point features 2.24e-3 (E_model 2.24e-3).
F per case (case id F):
  set abstraction: ns8-D0-32 0.0e+00, ns8-D0-32x64 6.0e-08, ns8-D0-64x96x160 1.2e-07, ns8-D9-32 6.0e-08, ns8-D9-32x64 1.2e-07,
      ns8-D9-64x96x160 1.2e-07, ns8-D30-32 1.2e-07, ns8-D30-32x64 1.2e-07, ns8-D30-64x96x160 1.2e-07, ns8-D61-32 1.2e-07, ns8-D61-32x64
      6.0e-08, ns8-D61-64x96x160 1.2e-07, ns40-D0-32 0.0e+00, ns40-D0-32x64 6.0e-08, ns40-D0-64x96x160 1.2e-07, ns40-D9-32 1.2e-07,
      ns40-D9-32x64 1.2e-07, ns40-D9-64x96x160 1.2e-07, ns40-D30-32 2.4e-07, ns40-D30-32x64 1.2e-07, ns40-D30-64x96x160 1.2e-07,
      ns40-D61-32 1.2e-07, ns40-D61-32x64 1.2e-07, ns40-D61-64x96x160 1.2e-07, ns8-D317-256x256x256 2.4e-07, ns40-D317-256x256x256
      4.7e-06
  feature propagation: S1-D1_0-cin40-32 6.0e-08, S1-D1_0-cin40-128x96 6.0e-08, S1-D1_0-cin40-256x256x256 6.0e-08, S1-D1_0-cin128-32
      1.2e-07, S1-D1_0-cin128-128x96 6.0e-08, S1-D1_0-cin128-256x256x256 1.2e-07, S1-D1_0-cin512-32 1.5e-07, S1-D1_0-cin512-128x96
      6.0e-08, S1-D1_0-cin512-256x256x256 1.2e-07, S1-D1_7-cin40-32 1.2e-07, S1-D1_7-cin40-128x96 1.2e-07, S1-D1_7-cin40-256x256x256
      2.9e-05, S1-D1_7-cin128-32 1.2e-07, S1-D1_7-cin128-128x96 1.2e-07, S1-D1_7-cin128-256x256x256 1.8e-07, S1-D1_7-cin512-32 1.2e-07,
      S1-D1_7-cin512-128x96 1.2e-07, S1-D1_7-cin512-256x256x256 1.1e-04, S2-D1_0-cin40-32 1.2e-07, S2-D1_0-cin40-128x96 6.0e-08,
      S2-D1_0-cin40-256x256x256 1.2e-05, S2-D1_0-cin128-32 1.8e-07, S2-D1_0-cin128-128x96 1.2e-07, S2-D1_0-cin128-256x256x256 1.2e-07,
      S2-D1_0-cin512-32 2.7e-07, S2-D1_0-cin512-128x96 1.3e-06, S2-D1_0-cin512-256x256x256 5.7e-06, S2-D1_7-cin40-32 1.2e-07,
      S2-D1_7-cin40-128x96 1.2e-07, S2-D1_7-cin40-256x256x256 2.4e-07, S2-D1_7-cin128-32 1.2e-07, S2-D1_7-cin128-128x96 1.2e-07,
      S2-D1_7-cin128-256x256x256 2.9e-06, S2-D1_7-cin512-32 2.4e-07, S2-D1_7-cin512-128x96 1.2e-07, S2-D1_7-cin512-256x256x256 3.0e-05,
      S5-D1_0-cin40-32 1.2e-07, S5-D1_0-cin40-128x96 7.5e-08, S5-D1_0-cin40-256x256x256 2.4e-07, S5-D1_0-cin128-32 1.8e-07,
      S5-D1_0-cin128-128x96 1.2e-07, S5-D1_0-cin128-256x256x256 1.2e-07, S5-D1_0-cin512-32 2.4e-07, S5-D1_0-cin512-128x96 1.2e-07,
      S5-D1_0-cin512-256x256x256 2.7e-06, S5-D1_7-cin40-32 1.2e-07, S5-D1_7-cin40-128x96 8.9e-08, S5-D1_7-cin40-256x256x256 2.0e-04,
      S5-D1_7-cin128-32 1.2e-07, S5-D1_7-cin128-128x96 1.2e-07, S5-D1_7-cin128-256x256x256 5.0e-05, S5-D1_7-cin512-32 3.6e-07,
      S5-D1_7-cin512-128x96 1.2e-07, S5-D1_7-cin512-256x256x256 1.2e-07, S40-D1_0-cin40-32 1.2e-07, S40-D1_0-cin40-128x96 1.2e-07,
      S40-D1_0-cin40-256x256x256 1.2e-07, S40-D1_0-cin128-32 1.8e-07, S40-D1_0-cin128-128x96 1.2e-07, S40-D1_0-cin128-256x256x256
      1.2e-07, S40-D1_0-cin512-32 4.8e-07, S40-D1_0-cin512-128x96 3.1e-05, S40-D1_0-cin512-256x256x256 6.7e-06, S40-D1_7-cin40-32
      1.2e-07, S40-D1_7-cin40-128x96 1.2e-07, S40-D1_7-cin40-256x256x256 3.6e-07, S40-D1_7-cin128-32 1.2e-07, S40-D1_7-cin128-128x96
      1.4e-07, S40-D1_7-cin128-256x256x256 1.8e-07, S40-D1_7-cin512-32 3.6e-07, S40-D1_7-cin512-128x96 1.2e-07,
      S40-D1_7-cin512-256x256x256 1.8e-07
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_bf16_ref as R                           # noqa: E402
import sa_ref                                      # noqa: E402
import fp_ref                                      # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tl(layers):
    return [tuple(_t(a) for a in layer) for layer in layers]


def _ws(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def _judge(what, got, again, fp32, exact, emu, E, F):
    assert np.isfinite(got).all(), what                            # the output started as NaN: every element was written
    assert np.array_equal(got, again), what                        # reproducible, bit for bit
    assert not np.array_equal(got, fp32), what                     # the bf16 path ran
    g = got.astype(np.float64)
    d_emu, d_exact = float(np.abs(g - emu).max()), float(np.abs(g - exact).max())
    ulp = R.ulp_term(emu)
    print(f"{what}: E = {E:.3e}, F = {F:.3e}, |gpu - emulated| = {d_emu:.3e} (bar {4 * F + ulp:.3e}), |gpu - exact| = {d_exact:.3e} "
          f"(bar {1.5 * E:.3e}), |gpu - fp32 kernel| = {float(np.abs(g - fp32).max()):.3e}")
    assert d_emu <= 4.0 * F + ulp, (what, d_emu, F, ulp)
    assert d_exact <= 1.5 * E, (what, d_exact, E)


@pytest.mark.parametrize("case", R.SA_CASES, ids=R.sa_id)
def test_sa_forward_bf16(synth, case):
    L, U = sub("_lib"), sub("utils.utils")
    nsample, D, widths = case
    xyz, cent, grp, feats, layers = R.sa_case(synth, case)
    exact, emu, E, F, _ = R.sa_three(synth, case)
    x, c = _t(xyz), _t(cent)
    g = U.ball_query(x, c, R.SA_RADIUS, nsample)                   # the fp32 kernel's groups, which are the restatement's
    assert np.array_equal(g.cpu().numpy(), grp)
    count = np.array([[len(set(row)) for row in cl] for cl in grp])
    assert count.max() == nsample and (nsample == 8 or count.min() < nsample)          # full groups, and filler slots where nsample = 40
    args = (x, c, g, _t(feats), _tl(layers), [R.BN_EPS] * len(layers))
    need = L.sa_forward_bf16_workspace_bytes(D, R.B, R.SA_NPOINT, nsample, widths)
    outs = []
    for fn, nbytes, prefill in ((L.sa_forward_bf16, need, float("nan")), (L.sa_forward_bf16, need, -7.0),
                                (L.sa_forward_f32, L.SA_WORKSPACE_BYTES, float("nan"))):
        out = torch.full((R.B, R.SA_NPOINT, widths[-1]), prefill, dtype=torch.float32, device="cuda")
        fn(*args, out, _ws(nbytes))
        outs.append(out.cpu().numpy())
    _judge("sa " + R.sa_id(case), *outs, exact, emu, E, F)


@pytest.mark.parametrize("case", R.FP_CASES, ids=R.fp_id)
def test_fp_forward_bf16(synth, case):
    L, U = sub("_lib"), sub("utils.utils")
    S, D1, cin, widths = case
    fine, coarse, p1, p2, idx, d2, layers = R.fp_case(synth, case)
    exact, emu, E, F, _ = R.fp_three(synth, case)
    gi, gd = U.three_nn(_t(fine), _t(coarse))                      # the fp32 kernel's neighbours, which are the restatement's
    assert gi.cpu().numpy().tobytes() == idx.tobytes() and gd.cpu().numpy().tobytes() == d2.tobytes()
    args = (_t(p1), _t(p2), gi, gd, _tl(layers), [R.BN_EPS] * len(layers))
    need = L.fp_forward_bf16_workspace_bytes(D1, cin - D1, R.B, R.FP_N, widths)
    outs, rows, guard = [], R.B * R.FP_N, -1234.5
    for fn, nbytes, prefill in ((L.fp_forward_bf16, need, float("nan")), (L.fp_forward_bf16, need, -7.0),
                                (L.fp_forward_f32, L.FP_WORKSPACE_BYTES, float("nan"))):
        buf = torch.full((rows + 8, widths[-1]), prefill, dtype=torch.float32, device="cuda")          # 8 guard rows behind the output
        buf[rows:] = guard
        fn(*args, buf[:rows].view(R.B, R.FP_N, widths[-1]), _ws(nbytes))
        assert (buf[rows:] == guard).all(), "rows past the last cloud were written"
        outs.append(buf[:rows].view(R.B, R.FP_N, widths[-1]).cpu().numpy())
    _judge("fp " + R.fp_id(case), *outs, exact, emu, E, F)


def test_refusals_on_device_tensors(synth):
    """The limits of the fp32 entry points, and a workspace of the fp32 size is too small."""
    L = sub("_lib")
    xyz, cent, grp, feats, layers = R.sa_case(synth, (8, 9, [32, 64]))
    args = (_t(xyz), _t(cent), _t(grp), _t(feats))
    out = torch.zeros((R.B, R.SA_NPOINT, 64), device="cuda")
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.sa_forward_bf16(*args, _tl(layers), [R.BN_EPS] * 2, out, _ws(L.SA_WORKSPACE_BYTES))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        L.sa_forward_bf16(*args, _tl(sa_ref.make_layers(1, 12, [32, 48])), [R.BN_EPS] * 2, torch.zeros((R.B, R.SA_NPOINT, 48), device="cuda"),
                          _ws(1 << 16))
    _, _, p1, p2, idx, d2, layers = R.fp_case(synth, (5, 7, 40, [32]))
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.fp_forward_bf16(_t(p1), _t(p2), _t(idx), _t(d2), _tl(layers), [R.BN_EPS], torch.zeros((R.B, R.FP_N, 32), device="cuda"),
                          _ws(L.FP_WORKSPACE_BYTES))


# ---- the modules -----------------------------------------------------------------------------------------------------------------------
def _randomise(mod, seed):
    """Seeded values for every parameter and BatchNorm buffer (fresh running statistics would make bn_eval almost the identity)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in mod.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var") or ("mlp_bns" in k and k.endswith("weight")):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * (0.6 if v.dim() == 1 else 2.0 / v.shape[1] ** 0.5)
    mod.load_state_dict(sd)
    return sd


def _block_layers(block):
    M = sub("pointNet.model.pointnet2_utils")
    return M._mlp_tensors(block), [bn.eps for bn in block.mlp_bns]


def test_blocks_go_through_the_entry_point_their_precision_names(synth):
    """A precision='bf16' block is the direct bf16 call on its own centres, groups and neighbours, bit for bit; the precision=None
    block beside it is the fp32 call, also inside a bf16 precision scope."""
    M, L, U = sub("pointNet.model.pointnet2_utils"), sub("_lib"), sub("utils.utils")
    B, N, D, S = 2, 200, 9, 24
    xyz = _t(synth.clouds(71, B, N)).transpose(1, 2).contiguous()                                   # [B, 3, N]
    points = _t(synth.uniform(72, (B, N, D), -1.0, 1.0)).transpose(1, 2).contiguous()
    x, feats = xyz.transpose(1, 2).contiguous(), points.transpose(1, 2).contiguous()
    sa16 = M.PointNetSetAbstraction(S, 0.5, 40, D + 3, [32, 64], False, precision="bf16").eval()
    sa32 = M.PointNetSetAbstraction(S, 0.5, 40, D + 3, [32, 64], False).eval()
    _randomise(sa16, 9)
    sa32.load_state_dict(sa16.state_dict())
    cent = U.fps_indices(x, S)
    gi = U.ball_query(x, cent, 0.5, 40)
    layers, eps = _block_layers(sa16)
    want16, want32 = (torch.full((B, S, 64), float("nan"), device="cuda") for _ in range(2))
    L.sa_forward_bf16(x, cent, gi, feats, layers, eps, want16, _ws(L.sa_forward_bf16_workspace_bytes(D, B, S, 40, [32, 64])))
    L.sa_forward_f32(x, cent, gi, feats, layers, eps, want32, _ws(L.SA_WORKSPACE_BYTES))
    xyz16, out16 = sa16(xyz, points)
    xyz32, out32 = sa32(xyz, points)
    assert torch.equal(out16, want16.transpose(1, 2)) and torch.equal(out32, want32.transpose(1, 2)) and not torch.equal(out16, out32)
    assert torch.equal(xyz16, xyz32) and torch.equal(xyz16, U.gather_rows(x, cent).transpose(1, 2))
    with L.precision_scope("bf16"):
        assert torch.equal(sa32(xyz, points)[1], out32) and torch.equal(sa16(xyz, points)[1], out16)
    assert torch.equal(sa32.set_precision("bf16")(xyz, points)[1], out16)                            # the workspace grows with the request
    assert torch.equal(sa32.set_precision("fp32")(xyz, points)[1], out32)
    assert not out16.requires_grad

    D1 = 7
    p1 = _t(synth.uniform(73, (B, N, D1), -1.0, 1.0)).transpose(1, 2).contiguous()
    xyz2, p2 = xyz16, out16                                                                          # [B, 3, S], [B, 64, S]
    fp16 = M.PointNetFeaturePropagation(D1 + 64, [128, 96], precision="bf16").eval()
    fp32 = M.PointNetFeaturePropagation(D1 + 64, [128, 96]).eval()
    _randomise(fp16, 10)
    fp32.load_state_dict(fp16.state_dict())
    idx, d2 = U.three_nn(x, xyz2.transpose(1, 2).contiguous())
    layers, eps = _block_layers(fp16)
    r1, r2 = p1.transpose(1, 2).contiguous(), p2.transpose(1, 2).contiguous()
    want16, want32 = (torch.full((B, N, 96), float("nan"), device="cuda") for _ in range(2))
    L.fp_forward_bf16(r1, r2, idx, d2, layers, eps, want16, _ws(L.fp_forward_bf16_workspace_bytes(D1, 64, B, N, [128, 96])))
    L.fp_forward_f32(r1, r2, idx, d2, layers, eps, want32, _ws(L.FP_WORKSPACE_BYTES))
    out16, out32 = fp16(xyz, xyz2, p1, p2), fp32(xyz, xyz2, p1, p2)
    assert torch.equal(out16, want16.transpose(1, 2)) and torch.equal(out32, want32.transpose(1, 2)) and not torch.equal(out16, out32)
    with L.precision_scope("bf16"):
        assert torch.equal(fp32(xyz, xyz2, p1, p2), out32) and torch.equal(fp16(xyz, xyz2, p1, p2), out16)
    fp16.train()
    with pytest.raises(NotImplementedError, match="eval"):
        fp16(xyz, xyz2, p1, p2)


def test_pointnet_2_bf16_stays_within_the_model_error_of_the_fp32_model(synth):
    """pointnet_2(precision='bf16').eval() at B = 2, N = 512 (128 / 32 / 8 centres and larger balls, as the fp32 model's test): both
    outputs finite, of the right shapes, and within 1.5 E_model of the fp32 model's, E_model = max |emulated - exact| of the six blocks
    CHAINED on the CPU (conv1 and the max in float64 on both sides), on the model's own centres, groups and neighbours -- which are
    the same in both modes: they depend on the coordinates alone."""
    A, U = sub("pointNet.model.pointnetAtt"), sub("utils.utils")
    B, N = 2, 512
    m16, m32 = A.pointnet_2(5, precision="bf16").eval(), A.pointnet_2(5).eval()
    for m in (m16, m32):
        for sa, npoint, radius in ((m.sa1, 128, 0.2), (m.sa2, 32, 0.4), (m.sa3, 8, 0.8)):
            sa.npoint, sa.radius = npoint, radius
    sd = {k: v.cpu().numpy() for k, v in _randomise(m16, 8).items()}
    m32.load_state_dict(m16.state_dict())
    x_np = np.concatenate([synth.clouds(55, B, N), synth.uniform(56, (B, N, 6), -1.0, 1.0)], -1).astype(np.float32)     # [B, N, 9]
    x = _t(x_np).transpose(1, 2).contiguous()
    with torch.no_grad():
        g16, p16 = m16(x)
        g32, p32 = m32(x)
    assert g16.shape == (B, 128) and p16.shape == (B, 128, N) and torch.isfinite(g16).all() and torch.isfinite(p16).all()
    assert not torch.equal(p16, p32) and not p16.requires_grad

    def layers_of(name, n):
        return [(sd[f"{name}.mlp_convs.{i}.weight"].reshape(sd[f"{name}.mlp_convs.{i}.weight"].shape[:2]), sd[f"{name}.mlp_convs.{i}.bias"],
                 sd[f"{name}.mlp_bns.{i}.weight"], sd[f"{name}.mlp_bns.{i}.bias"], sd[f"{name}.mlp_bns.{i}.running_mean"],
                 sd[f"{name}.mlp_bns.{i}.running_var"]) for i in range(n)]

    def chain(mode, c):
        xyz0, feats, levels = x_np[c, :, :3], x_np[c], []
        xyz = xyz0
        for name, sa in (("sa1", m32.sa1), ("sa2", m32.sa2), ("sa3", m32.sa3)):
            cent = U.fps_indices(_t(xyz)[None], sa.npoint)[0].cpu().numpy()
            grp, _ = sa_ref.ball_query(xyz, cent, sa.radius, sa.nsample)
            feats = R.sa_forward(xyz, cent, grp, feats, layers_of(name, 3), [1e-5] * 3, mode)
            xyz = xyz[cent]
            levels.append((xyz, feats))
        (x1, f1), (x2, f2), (x3, f3) = levels
        for name, n, fine, coarse, skip in (("fp3", 2, x2, x3, f2), ("fp2", 2, x1, x2, f1), ("fp1", 3, xyz0, x1, None)):
            idx, d2 = fp_ref.three_nn(fine, coarse)
            f3 = R.fp_forward(skip, f3, idx, d2, layers_of(name, n), [1e-5] * n, mode)
        y = f3 @ sd["conv1.weight"][:, :, 0].astype(np.float64).T + sd["conv1.bias"].astype(np.float64)
        return y.max(0), f3                                                                            # [128], [N, 128]

    E_g = E_p = 0.0
    for c in range(B):
        (ge, pe), (gm, pm) = chain(R.EXACT, c), chain(R.EMULATED, c)
        E_g, E_p = max(E_g, float(np.abs(gm - ge).max())), max(E_p, float(np.abs(pm - pe).max()))
    d_g, d_p = float((g16 - g32).abs().max()), float((p16 - p32).abs().max())
    print(f"pointnet_2 bf16 against fp32: global feature {d_g:.3e} (E_model {E_g:.3e}), point features {d_p:.3e} (E_model {E_p:.3e})")
    assert 0.0 < d_g <= 1.5 * E_g and 0.0 < d_p <= 1.5 * E_p, (d_g, E_g, d_p, E_p)
