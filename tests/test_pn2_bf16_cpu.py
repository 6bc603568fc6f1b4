"""The host side of the bf16 PointNet++ forwards, without a GPU: the `precision` keyword of the two blocks and of pointnet_2 with its
refusals, the four new entry points within ABI 17, the workspace sizes answered on the host, and -- for every case of
tests/test_pn2_bf16_gpu.py -- that the inherent bf16 error E stands at least 16 times above F, the distance between two legitimate
implementations of the rounding model (tests/pn2_bf16_ref.py), so that the GPU bars (4 F against the emulation, 1.5 E against the exact
result) can tell a missing rounding step from noise; and that the summation order the MFMA was measured to use lies within half of
that bar (pn2_bf16_ref.seed_holds: the rule by which the seeds were chosen, on the CPU alone)."""
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_bf16_ref as R                           # noqa: E402

SYMBOLS = ("ampnet_sa_forward_bf16", "ampnet_fp_forward_bf16", "ampnet_sa_forward_bf16_workspace_bytes",
           "ampnet_fp_forward_bf16_workspace_bytes")
FP32_NAMES, BF16_NAMES, NOT_BUILT = (None, "fp32", "f32", "float32"), ("bf16", "bfloat16"), ("f32x3", "fp32_split", "bf16_train", "bf16_store")


def _sa(M, **kw):
    return M.PointNetSetAbstraction(16, 0.2, 8, 12, [32, 64], kw.pop("group_all", False), device="cpu", **kw)


def _fp(M, **kw):
    return M.PointNetFeaturePropagation(40, [32, 64], device="cpu", **kw)


def _model(A, **kw):
    return A.pointnet_2(5, device="cpu", **kw)


def test_the_three_constructors_take_keyword_only_precision_last():
    M, A = sub("pointNet.model.pointnet2_utils"), sub("pointNet.model.pointnetAtt")
    for cls in (M.PointNetSetAbstraction, M.PointNetFeaturePropagation, A.pointnet_2):
        par = list(inspect.signature(cls.__init__).parameters.values())
        assert par[-1].name == "precision" and par[-1].kind is inspect.Parameter.KEYWORD_ONLY and par[-1].default is None, cls
        assert callable(cls.set_precision) and cls.precision is None
    assert "precision" not in inspect.signature(M.PointNetSetAbstractionMsg.__init__).parameters          # not built in this block
    with pytest.raises(TypeError):
        M.PointNetFeaturePropagation(40, [32], "cpu", False, False, "bf16")


def test_none_and_fp32_construct_as_before():
    M, A = sub("pointNet.model.pointnet2_utils"), sub("pointNet.model.pointnetAtt")
    base_sa, base_fp, base_model = list(_sa(M).state_dict()), list(_fp(M).state_dict()), list(_model(A).state_dict())
    for mode in FP32_NAMES + BF16_NAMES:
        sa, fp, model = _sa(M, precision=mode), _fp(M, precision=mode), _model(A, precision=mode)
        assert (sa.precision, fp.precision, model.precision) == (mode,) * 3
        assert [m.precision for m in (model.sa1, model.sa2, model.sa3, model.fp3, model.fp2, model.fp1)] == [mode] * 6
        assert (list(sa.state_dict()), list(fp.state_dict()), list(model.state_dict())) == (base_sa, base_fp, base_model)
    # fp32 with every flag, as before
    for mode in FP32_NAMES:
        _sa(M, grad=True, batch_stats=True, precision=mode)
        _sa(M, group_all=True, grad=True, precision=mode)
        _fp(M, grad=True, batch_stats=True, precision=mode)
        _model(A, decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True, precision=mode)
    model = _model(A)
    assert model.set_precision("bf16") is model and model.fp1.precision == model.sa3.precision == "bf16"
    assert model.set_precision(None).fp1.precision is None


def test_the_refusal_matrix():
    M, A = sub("pointNet.model.pointnet2_utils"), sub("pointNet.model.pointnetAtt")
    for mode in BF16_NAMES:
        for kw in ({"grad": True}, {"batch_stats": True}, {"group_all": True}, {"grad": True, "batch_stats": True}):
            with pytest.raises(NotImplementedError, match="=True"):
                _sa(M, precision=mode, **kw)
            with pytest.raises(NotImplementedError, match="inference"):
                _sa(M, **kw).set_precision(mode)
        for kw in ({"grad": True}, {"batch_stats": True}):
            with pytest.raises(NotImplementedError, match="=True"):
                _fp(M, precision=mode, **kw)
            block = _fp(M, **kw)
            with pytest.raises(NotImplementedError, match="inference"):
                block.set_precision(mode)
            assert block.precision is None                           # a refused mode is not set
        for kw in ({"decoder_grad": True}, {"decoder_grad": True, "encoder_grad": True}, {"decoder_grad": True, "decoder_batch_stats": True},
                   {"decoder_grad": True, "encoder_grad": True, "decoder_batch_stats": True, "encoder_batch_stats": True}):
            with pytest.raises(NotImplementedError, match="decoder_grad=True"):
                _model(A, precision=mode, **kw)
            model = _model(A, **kw)
            with pytest.raises(NotImplementedError, match="inference"):
                model.set_precision(mode)
            assert model.precision is None and model.fp1.precision is None
    for mode in NOT_BUILT:                                           # the package's other modes: named, not built here
        for make in (lambda: _sa(M, precision=mode), lambda: _fp(M, precision=mode), lambda: _model(A, precision=mode),
                     lambda: _sa(M).set_precision(mode), lambda: _fp(M).set_precision(mode), lambda: _model(A).set_precision(mode)):
            with pytest.raises(NotImplementedError, match="'fp32'.*'bf16'"):
                make()
    L = sub("_lib")
    assert set(NOT_BUILT) | set(FP32_NAMES[1:]) | set(BF16_NAMES) == set(L.PRECISIONS)
    for make in (lambda: _sa(M, precision="fp16"), lambda: _fp(M).set_precision("fp16"), lambda: _model(A, precision="fp16")):
        with pytest.raises(ValueError, match="unknown matrix precision 'fp16'"):             # what checked_precision raises
            make()
    # a flag set after construction does not turn a bf16 block into an fp32 one silently
    block = _fp(M, precision="bf16")
    block.grad = True
    with pytest.raises(NotImplementedError, match="grad=True"):
        block._check_bf16()


def test_library_exports_the_entry_points_within_abi_17():
    L = sub("_lib")
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s + "(" in header, s
    for name in ("sa_forward_bf16", "fp_forward_bf16", "sa_forward_bf16_workspace_bytes", "fp_forward_bf16_workspace_bytes"):
        assert callable(getattr(L, name)), name
    assert list(inspect.signature(L.sa_forward_bf16).parameters) == list(inspect.signature(L.sa_forward_f32).parameters)
    assert list(inspect.signature(L.fp_forward_bf16).parameters) == list(inspect.signature(L.fp_forward_f32).parameters)
    assert "THE ROUNDING MODEL" in header and "v_mfma_f32_32x32x16_bf16" in header
    assert lib.ampnet_abi_version() == L.ABI_VERSION == 18      # the entry points above arrived within ABI 17; the baseline probe made it 18


def test_workspace_sizes_answer_on_the_host():
    """fold + per layer cout * (cin padded to 16) bf16; outside the limits 0 and an error that names the limit."""
    L = sub("_lib")
    pad = lambda c: (c + 15) // 16 * 16
    size = lambda cin, couts: L.SA_WORKSPACE_BYTES + 2 * sum(c * pad(k) for c, k in zip(couts, [cin] + list(couts)))
    assert L.SA_WORKSPACE_BYTES == L.FP_WORKSPACE_BYTES
    for D, couts in ((0, [32]), (9, [32, 32, 64]), (30, [64, 96, 160]), (317, [256, 256, 256])):
        got = L.sa_forward_bf16_workspace_bytes(D, 2, 12, 40, couts)
        assert got == size(3 + D, couts) > L.SA_WORKSPACE_BYTES and got % 16 == 0, (D, couts)
    assert L.sa_forward_bf16_workspace_bytes(9, 2, 12, 8, [32, 32, 64]) == L.SA_WORKSPACE_BYTES + 2 * (32 * 16 + 32 * 32 + 64 * 32)
    for D1, D2, couts in ((0, 40, [32]), (7, 121, [128, 96]), (7, 505, [256, 256, 256]), (0, 128, [128, 128, 128])):
        assert L.fp_forward_bf16_workspace_bytes(D1, D2, 2, 70, couts) == size(D1 + D2, couts), (D1, D2, couts)
    lib = L.lib()
    for args, match in (((318, 2, 12, 8, [32]), "321 exceeds 320"), ((9, 2, 12, 65, [32]), "nsample=65"), ((9, 2, 12, 0, [32]), "nsample=0"),
                        ((9, 2, 12, 8, [32, 48]), "cout=48"), ((9, 2, 12, 8, [288]), "cout=288"), ((9, 2, 12, 8, [32] * 4), "L=4"),
                        ((9, 2, 12, 8, []), "L=0"), ((9, 0, 12, 8, [32]), "n_clouds=0"), ((9, 1 << 16, 1 << 16, 8, [32]), "2\\^31")):
        with pytest.raises(L.AmpnetError, match=match):
            L.sa_forward_bf16_workspace_bytes(*args)
    for args, match in (((7, 506, 2, 70, [32]), "7 \\+ 506"), ((0, 0, 2, 70, [32]), "D2 >= 1"), ((0, 40, 2, 70, [32, 40]), "cout=40"),
                        ((0, 40, 2, 70, [32] * 4), "L=4"), ((0, 40, 0, 70, [32]), "n_clouds=0"), ((0, 40, 2, 0, [32]), "n=0")):
        with pytest.raises(L.AmpnetError, match=match):
            L.fp_forward_bf16_workspace_bytes(*args)
    import ctypes
    fn = lib.ampnet_fp_forward_bf16_workspace_bytes
    fn.restype = ctypes.c_size_t
    assert fn(0, 40, 2, 70, (ctypes.c_int * 1)(48), 1) == 0 and b"cout=48" in lib.ampnet_last_error()


def test_bad_arguments_are_errors_before_any_launch():
    """Every check runs on the host before any launch: host memory stands in for the device pointers, nothing is dereferenced."""
    import ctypes
    L = sub("_lib")
    lib = L.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    table = lambda n: (ctypes.c_void_p * (6 * n))(*[p.value] * (6 * n))
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    eps = lambda n: (ctypes.c_float * n)(*[1e-5] * n)
    need = L.sa_forward_bf16_workspace_bytes(9, 1, 4, 8, [32, 64])

    def sa(couts=(32, 64), nsample=8, D=9, ws_bytes=need, ws=p):
        return lib.ampnet_sa_forward_bf16(p, 1, 64, 3, p, 4, p, nsample, p, D, table(len(couts)), ints(couts), eps(len(couts)), len(couts), p, ws,
                                          ctypes.c_size_t(ws_bytes), None)

    for kw, match in (({"ws_bytes": need - 1}, "workspace"), ({"ws_bytes": L.SA_WORKSPACE_BYTES}, "workspace"), ({"couts": (32, 48)}, "cout=48"),
                      ({"nsample": 65}, "nsample=65"), ({"D": 318}, "321 exceeds 320"),
                      ({"ws": ctypes.c_void_p(p.value + 4)}, "16-byte aligned")):
        with pytest.raises(L.AmpnetError, match=match):
            L.check(sa(**kw), "ampnet_sa_forward_bf16")
    need = L.fp_forward_bf16_workspace_bytes(7, 33, 1, 64, [32, 64])

    def fp(couts=(32, 64), D1=7, D2=33, k=3, ws_bytes=need, ws=p):
        return lib.ampnet_fp_forward_bf16(p, D1, p, D2, 1, 64, 4, p, p, k, table(len(couts)), ints(couts), eps(len(couts)), len(couts), p, ws,
                                          ctypes.c_size_t(ws_bytes), None)

    for kw, match in (({"ws_bytes": need - 1}, "workspace"), ({"ws_bytes": L.FP_WORKSPACE_BYTES}, "workspace"), ({"couts": (32, 48)}, "cout=48"),
                      ({"k": 4}, "k=4"), ({"D2": 506}, "7 \\+ 506"), ({"ws": ctypes.c_void_p(p.value + 8)}, "16-byte aligned")):
        with pytest.raises(L.AmpnetError, match=match):
            L.check(fp(**kw), "ampnet_fp_forward_bf16")


def test_bf16_rounding_is_round_to_nearest_even():
    import numpy as np
    import torch
    x = np.concatenate([np.random.default_rng(3).standard_normal(4096).astype(np.float32),
                        np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39, 0.0, 65280.0, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32)])
    assert np.array_equal(R.bf16(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert R.bf16(np.float32(1.00390625)) == 1.0 and R.bf16(np.float32(1.01171875)) == np.float32(1.015625)       # ties go to even


@pytest.mark.parametrize("case", R.SA_CASES, ids=R.sa_id)
def test_sa_bf16_error_stands_above_the_implementation_noise(synth, case):
    exact, emu, E, F, F_m = R.sa_three(synth, case, model=True)
    print(f"sa {R.sa_id(case)}: E = {E:.3e}, F = {F:.3e}, the MFMA's order {F_m:.3e}, E / F = {E / max(F, 1e-300):.0f}")
    assert exact.shape == emu.shape == (R.B, R.SA_NPOINT, case[2][-1]) and (exact > 0).mean() > 0.2
    assert E >= 16.0 * F, (E, F)                                  # (F = 0 where a sum of three exact products has one value)
    assert R.seed_holds(emu, E, F, F_m), (E, F, F_m)


@pytest.mark.parametrize("case", R.FP_CASES, ids=R.fp_id)
def test_fp_bf16_error_stands_above_the_implementation_noise(synth, case):
    exact, emu, E, F, F_m = R.fp_three(synth, case, model=True)
    print(f"fp {R.fp_id(case)}: E = {E:.3e}, F = {F:.3e}, the MFMA's order {F_m:.3e}, E / F = {E / max(F, 1e-300):.0f}")
    assert exact.shape == emu.shape == (R.B, R.FP_N, case[3][-1]) and (exact > 0).mean() > 0.2
    assert E >= 16.0 * F, (E, F)                                  # (F = 0 where a sum of three exact products has one value)
    assert R.seed_holds(emu, E, F, F_m), (E, F, F_m)
