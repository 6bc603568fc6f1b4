"""The four backwards on clouds of UNEQUAL size packed back to back (include/ampnet_hip.h: ampnet_fp_backward_ragged_f32,
ampnet_fp_train_backward_ragged_f32, ampnet_sa_backward_ragged_f32, ampnet_sa_train_backward_ragged_f32), layer by layer, on the clouds of
tests/ragged_bwd_cases.py (128, 129, 200, 200 and 511 points):
  * frozen statistics: the gathered gradient (dpoints2, dfeats) of cloud b is, bit for bit, what the uniform entry point writes for that
    cloud alone with local indices;
  * every output against the float64 restatements (fp_bwd_ref, sa_bwd_ref, fp_train_ref, sa_train_ref) on the packed array as ONE cloud
    with global indices, at the bars those restatements derive -- the bars of the existing layer tests, which take them from the same
    functions;
  * every output equals, bit for bit, the uniform entry point on the packed array as one cloud (the indices keep to their cloud, so the
    two gathers visit the same entries in the same order) -- at three layers too, which the references cannot settle at these row counts;
  * a coarse point nobody picked and a point in no group get exact zeros; two runs give equal bits; every output is written and nothing
    past its end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import fp_bwd_ref                                  # noqa: E402
import fp_train_ref                                # noqa: E402
import ragged_bwd_cases as C                       # noqa: E402
import sa_bwd_ref                                  # noqa: E402
import sa_train_ref                                # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234.5
DEV = "cuda"
MOMENTUM = fp_train_ref.MOMENTUM


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Outs:
    """Output tensors in front of 64 guard words each, which the kernels must leave alone."""

    def __init__(self, prefill):
        self.prefill, self.bufs = prefill, {}

    def new(self, name, shape, dtype=torch.float32):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), self.prefill if dtype == torch.float32 else -77, dtype=dtype, device=DEV)
        buf[numel:] = GUARD if dtype == torch.float32 else int(GUARD)
        self.bufs[name] = buf
        return buf[:numel].view(*shape)

    def grads(self, layers, res):
        out = []
        for l, layer in enumerate(layers):
            out.append(tuple(self.new(f"{k}{l}", layer[j].shape) for k, j in (("dW", 0), ("dbias", 1), ("dgamma", 1), ("dbeta", 1))))
            res.update({f"{k}{l}": g for k, g in zip(("dW", "dbias", "dgamma", "dbeta"), out[-1])})
        return out

    def check(self):
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            assert (buf[-64:] == (GUARD if buf.dtype == torch.float32 else int(GUARD))).all(), f"{name}: written past its end"


def _ws(need):
    return torch.full((need,), 0xAB, dtype=torch.uint8, device=DEV)


def _off():
    return _t(C.OFF)


def _dev_layers(layers):
    return [tuple(_t(a) for a in layer) for layer in layers]


def _couts(layers):
    return [int(layer[0].shape[0]) for layer in layers]


# ---- feature propagation ----------------------------------------------------------------------------------------------------------------
def _fp_backward(L, p1, p2, idx, d2, layers, dout, cloud_off, prefill=float("nan")):
    """ampnet_fp_backward_f32 (cloud_off None) or its ragged namesake on device tensors -> {name: device tensor}."""
    o = _Outs(prefill)
    res = {"dpoints1": o.new("dpoints1", p1.shape), "dpoints2": o.new("dpoints2", p2.shape)}
    grads = o.grads(layers, res)
    need = L.fp_backward_workspace_bytes(p1.shape[2], p2.shape[2], p1.shape[0], p1.shape[1], _couts(layers))
    L.fp_backward_f32(p1, p2, idx, d2, layers, [C.BN_EPS] * len(layers), dout, res["dpoints1"], res["dpoints2"], grads, _ws(need),
                      cloud_off=cloud_off)
    o.check()
    return res


def _fp_train(L, i, cloud_off, prefill=float("nan")):
    """The train forward (no ragged form: the packed array is one cloud) and the train backward, uniform or ragged, of the inputs `i`
    -> {fp_train_ref name: device tensor}."""
    p1, p2, idx, d2, dout = (_t(i[k]) for k in ("points1", "points2", "idx", "dist2", "dout"))
    layers = _dev_layers(i["layers"])                                # fresh running statistics for every run
    couts = _couts(layers)
    o = _Outs(prefill)
    out, sm, si = o.new("out", (1, C.TOTAL, couts[-1])), o.new("save_mean", (sum(couts),)), o.new("save_invstd", (sum(couts),))
    L.fp_train_forward_f32(p1, p2, idx, d2, layers, i["eps"], MOMENTUM, out, sm, si,
                           _ws(L.fp_train_forward_workspace_bytes(p1.shape[2], p2.shape[2], 1, C.TOTAL, couts)))
    res = {"out": out, "dpoints1": o.new("dpoints1", p1.shape), "dpoints2": o.new("dpoints2", p2.shape)}
    c0 = 0
    for l, layer in enumerate(layers):
        res.update({f"save_mean{l}": sm[c0:c0 + couts[l]], f"save_invstd{l}": si[c0:c0 + couts[l]], f"running_mean{l}": layer[4],
                    f"running_var{l}": layer[5]})
        c0 += couts[l]
    grads = o.grads(layers, res)
    L.fp_train_backward_f32(p1, p2, idx, d2, layers, i["eps"], sm, si, dout, res["dpoints1"], res["dpoints2"], grads,
                            _ws(L.fp_train_backward_workspace_bytes(p1.shape[2], p2.shape[2], 1, C.TOTAL, couts)), cloud_off=cloud_off)
    o.check()
    return res


def _within_bars(what, got, want, names):
    ratios = {}
    for k in names:
        v, bar = want[k]
        g = got[k].cpu().numpy().astype(np.float64)
        assert g.shape == v.shape, (what, k, g.shape, v.shape)
        assert np.isfinite(g).all(), (what, k)
        err = np.abs(g - v)
        ratios[k] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())     # (0 / 0: an exact value met exactly)
    print(f"{what}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (what, k, r)


def _same_bits(what, a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@functools.lru_cache(maxsize=None)
def _fp_case(train):
    return C.fp_inputs(sub("synthetic"), train)


def test_fp_backward_ragged_cloud_by_cloud_bits_and_the_float64_reference():
    L = sub("_lib")
    i = _fp_case(False)
    p1, p2, idx, d2, dout = (_t(i[k]) for k in ("points1", "points2", "idx", "dist2", "dout"))
    layers = _dev_layers(i["layers"])
    got = _fp_backward(L, p1, p2, idx, d2, layers, dout, _off())     # every output starts as NaN: every element must be written
    _same_bits("second run", got, _fp_backward(L, p1, p2, idx, d2, layers, dout, _off(), prefill=-7.0))
    # cloud by cloud: the uniform entry point on the cloud alone, indices local
    local, S = _t(i["local_idx"]), C.FP_S
    for b, n in enumerate(C.SIZES):
        r0 = int(C.OFF[b])
        rows = lambda t: t[:, r0:r0 + n].contiguous()
        alone = _fp_backward(L, rows(p1), p2[:, b * S:(b + 1) * S].contiguous(), local[None, r0:r0 + n].contiguous(), rows(d2), layers, rows(dout),
                             None)
        assert torch.equal(got["dpoints2"][:, b * S:(b + 1) * S], alone["dpoints2"]), b
        assert torch.equal(got["dpoints1"][:, r0:r0 + n], alone["dpoints1"]), b
        assert (alone["dpoints2"] != 0).any()
    # the packed array as one cloud through the uniform entry point: the same entries in the same order
    _same_bits("one cloud", got, _fp_backward(L, p1, p2, idx, d2, layers, dout, None))
    assert (got["dpoints2"][0, _t(i["unpicked"])] == 0).all()          # nobody's neighbour: exact zeros, and written
    want, _ = fp_bwd_ref.fp_backward(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
    _within_bars("fp_backward_ragged", got, want, fp_bwd_ref.output_names(len(layers), True))


def test_fp_train_backward_ragged_against_the_float64_reference_and_the_uniform_bits():
    L = sub("_lib")
    i = _fp_case(True)
    got = _fp_train(L, i, _off())
    _same_bits("second run", got, _fp_train(L, i, _off(), prefill=-7.0))
    _same_bits("one cloud", got, _fp_train(L, i, None))
    assert (got["dpoints2"][0, _t(i["unpicked"])] == 0).all() and (got["dpoints2"] != 0).any()
    assert (got["dbias0"] == 0).all()                                # the bias has no effect on a batch-normalised output
    want, _ = fp_train_ref.fp_train(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
    _within_bars("fp_train_backward_ragged", got, want, fp_train_ref.output_names(len(i["layers"]), True))
    deep = C.fp_inputs(sub("synthetic"), True, C.DEEP_WIDTHS)        # three layers: every phase of the backward, by bits
    got = _fp_train(L, deep, _off())
    _same_bits("deep, one cloud", got, _fp_train(L, deep, None))
    assert all(torch.isfinite(v).all() and (k.startswith("dbias") or (v != 0).any()) for k, v in got.items())


# ---- set abstraction --------------------------------------------------------------------------------------------------------------------
def _sa_backward(L, xyz, centres, group_idx, feats, layers, dout, cloud_off, prefill=float("nan"), want_dfeats=True):
    """ampnet_sa_backward_f32 (cloud_off None) or its ragged namesake on device tensors -> {name: device tensor}, "arg" among them."""
    o = _Outs(prefill)
    res = {"arg": o.new("arg", tuple(centres.shape) + (_couts(layers)[-1],), torch.int32)}
    if want_dfeats:
        res["dfeats"] = o.new("dfeats", feats.shape)
    grads = o.grads(layers, res)
    need = L.sa_backward_workspace_bytes(feats.shape[2], centres.shape[0], centres.shape[1], group_idx.shape[2], _couts(layers))
    L.sa_backward_f32(xyz, centres, group_idx, feats, layers, [C.BN_EPS] * len(layers), dout, res.get("dfeats"), grads, _ws(need),
                      arg_out=res["arg"], cloud_off=cloud_off)
    o.check()
    return res


def _sa_train(L, i, cloud_off, prefill=float("nan")):
    """The train forward and the train backward, uniform or ragged, of the inputs `i` -> {sa_train_ref name: device tensor} and "arg"."""
    xyz, centres, group_idx, feats, dout = (_t(i[k]) for k in ("xyz", "centres", "group_idx", "feats", "dout"))
    layers = _dev_layers(i["layers"])
    couts = _couts(layers)
    GS = centres.shape[1]
    o = _Outs(prefill)
    out, sm, si = o.new("out", (1, GS, couts[-1])), o.new("save_mean", (sum(couts),)), o.new("save_invstd", (sum(couts),))
    L.sa_train_forward_f32(xyz, centres, group_idx, feats, layers, i["eps"], MOMENTUM, out, sm, si,
                           _ws(L.sa_train_forward_workspace_bytes(feats.shape[2], 1, GS, group_idx.shape[2], couts)))
    res = {"out": out, "dfeats": o.new("dfeats", feats.shape), "arg": o.new("arg", (1, GS, couts[-1]), torch.int32)}
    c0 = 0
    for l, layer in enumerate(layers):
        res.update({f"save_mean{l}": sm[c0:c0 + couts[l]], f"save_invstd{l}": si[c0:c0 + couts[l]], f"running_mean{l}": layer[4],
                    f"running_var{l}": layer[5]})
        c0 += couts[l]
    grads = o.grads(layers, res)
    L.sa_train_backward_f32(xyz, centres, group_idx, feats, layers, i["eps"], sm, si, dout, res["dfeats"], grads,
                            _ws(L.sa_train_backward_workspace_bytes(feats.shape[2], 1, GS, group_idx.shape[2], couts)), arg_out=res["arg"],
                            cloud_off=cloud_off)
    o.check()
    return res


@functools.lru_cache(maxsize=None)
def _sa_case(train):
    return C.sa_inputs(sub("synthetic"), train)


def test_sa_backward_ragged_cloud_by_cloud_bits_and_the_float64_reference():
    L = sub("_lib")
    i = _sa_case(False)
    xyz, centres, group_idx, feats, dout = (_t(i[k]) for k in ("xyz", "centres", "group_idx", "feats", "dout"))
    layers = _dev_layers(i["layers"])
    got = _sa_backward(L, xyz, centres, group_idx, feats, layers, dout, _off())
    _same_bits("second run", got, _sa_backward(L, xyz, centres, group_idx, feats, layers, dout, _off(), prefill=-7.0))
    no_df = _sa_backward(L, xyz, centres, group_idx, feats, layers, dout, _off(), want_dfeats=False)      # dfeats = NULL: the gather is skipped
    assert all(torch.equal(got[k], v) for k, v in no_df.items())
    lc, lg, S = _t(i["local_centres"]), _t(i["local_group_idx"]), C.SA_S
    for b, n in enumerate(C.SIZES):
        r0 = int(C.OFF[b])
        alone = _sa_backward(L, xyz[:, r0:r0 + n].contiguous(), lc[b:b + 1].contiguous(), lg[b:b + 1].contiguous(),
                             feats[:, r0:r0 + n].contiguous(), layers, dout[:, b * S:(b + 1) * S].contiguous(), None)
        assert torch.equal(got["dfeats"][:, r0:r0 + n], alone["dfeats"]), b
        assert torch.equal(got["arg"][:, b * S:(b + 1) * S], alone["arg"]), b
        assert (alone["dfeats"] != 0).any()
    _same_bits("one cloud", got, _sa_backward(L, xyz, centres, group_idx, feats, layers, dout, None))
    assert (got["dfeats"][0, _t(i["unpicked"])] == 0).all()            # in no group: exact zeros, and written
    tape, _ = sa_bwd_ref.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    arg = got["arg"].cpu().numpy()
    sa_bwd_ref.check_argmax(arg, tape, i["group_idx"])                 # the kernel's choice of the max's row is admissible
    want = sa_bwd_ref.sa_backward(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
    _within_bars("sa_backward_ragged", got, want, sa_bwd_ref.output_names(len(layers), True))


def test_sa_train_backward_ragged_against_the_float64_reference_and_the_uniform_bits():
    L = sub("_lib")
    i = _sa_case(True)
    got = _sa_train(L, i, _off())
    _same_bits("second run", got, _sa_train(L, i, _off(), prefill=-7.0))
    _same_bits("one cloud", got, _sa_train(L, i, None))
    assert (got["dfeats"][0, _t(i["unpicked"])] == 0).all() and (got["dfeats"] != 0).any()
    assert (got["dbias0"] == 0).all()
    tape, _ = sa_train_ref.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    arg = got["arg"].cpu().numpy()
    sa_train_ref.check_argmax(arg, tape[-1], i["group_idx"])
    want = sa_train_ref.sa_train(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
    _within_bars("sa_train_backward_ragged", got, want, sa_train_ref.output_names(len(i["layers"]), True))
    deep = C.sa_inputs(sub("synthetic"), True, C.DEEP_WIDTHS)
    got = _sa_train(L, deep, _off())
    _same_bits("deep, one cloud", got, _sa_train(L, deep, None))
    assert all(torch.isfinite(v.float()).all() and (k.startswith("dbias") or (v != 0).any()) for k, v in got.items())


def test_refusals_and_the_precondition():
    """What the wrappers and the entry points refuse, each with a sentence; and an index outside its cloud is clamped into the cloud by
    the gather: nothing is read or written out of bounds."""
    L = sub("_lib")
    i = _fp_case(False)
    p1, p2, idx, d2, dout = (_t(i[k]) for k in ("points1", "points2", "idx", "dist2", "dout"))
    layers = _dev_layers(i["layers"])
    seven = _t(np.arange(8, dtype=np.int32))
    with pytest.raises(L.AmpnetError, match="cloud_off"):
        _fp_backward(L, p1, p2, idx, d2, layers, dout, _off().long())
    with pytest.raises(L.AmpnetError, match="equal shares"):
        _fp_backward(L, p1, p2, idx, d2, layers, dout, seven)                             # 80 coarse points for 7 clouds
    two = lambda t: torch.cat([t, t]).contiguous()
    with pytest.raises(L.AmpnetError, match="leading dimension 1"):
        _fp_backward(L, two(p1), two(p2), two(idx), two(d2), layers, two(dout), _off())
    j = _sa_case(False)
    xyz, centres, group_idx, feats, sdout = (_t(j[k]) for k in ("xyz", "centres", "group_idx", "feats", "dout"))
    with pytest.raises(L.AmpnetError, match="equal shares"):
        _sa_backward(L, xyz, centres, group_idx, feats, _dev_layers(j["layers"]), sdout, seven)                # 60 centres
    wild = idx.clone()
    wild[0, 0, 0], wild[0, -1, 2] = C.Q * C.FP_S - 1, 0                                   # cloud 0 names the last coarse point, the last cloud the first
    got = _fp_backward(L, p1, p2, wild, d2, layers, dout, _off())
    assert all(torch.isfinite(v).all() for v in got.values())
