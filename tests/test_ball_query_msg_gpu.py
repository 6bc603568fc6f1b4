"""The multi-radius ball query (include/ampnet_hip.h: ampnet_ball_query_msg_f32): scale by scale bit for bit the single-radius kernel
(utils.ball_query, torch.equal) and the CPU restatement tests/sa_ref.py: ball_query (array_equal), index lists and counts.  Every case
also runs with count_host NULL and with a single count pointer NULL."""
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
import sa_ref                                      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234


class _Outs:
    """int32 output tensors in front of 64 guard words each, which the kernel must leave alone."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), -77, dtype=torch.int32, device="cuda")
        buf[numel:] = GUARD
        self.bufs.append(buf)
        return buf[:numel].view(*shape)

    def check_guards(self):
        torch.cuda.synchronize()
        for i, buf in enumerate(self.bufs):
            assert (buf[-64:] == GUARD).all(), f"output {i}: written past its end"

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((buf[:-64] == -77).all()) for buf in self.bufs)


def _check(pc, cent, radii, nsamples):
    """pc [B, n, ld] numpy, cent [B, s] numpy int32: the K lists and counts of one call == K ball_query calls == the restatement;
    returns the restatement's counts, K arrays [B, s]."""
    U, L = sub("utils.utils"), sub("_lib")
    x, c = torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda()
    K = len(radii)
    outs, cnts = U.ball_query_msg(x, c, radii, nsamples, return_counts=True)
    assert len(outs) == K and len(cnts) == K
    want_cnts = []
    for k in range(K):
        assert outs[k].dtype == torch.int32 and cnts[k].dtype == torch.int32 and tuple(outs[k].shape) == cent.shape + (nsamples[k],)
        single, single_cnt = U.ball_query(x, c, radii[k], nsamples[k], return_counts=True)
        assert torch.equal(outs[k], single) and torch.equal(cnts[k], single_cnt), (k, radii[k], nsamples[k])
        want, want_cnt = zip(*(sa_ref.ball_query(pc[b], cent[b], radii[k], nsamples[k]) for b in range(pc.shape[0])))
        assert np.array_equal(cnts[k].cpu().numpy(), np.stack(want_cnt)), (k, radii[k], nsamples[k])
        assert np.array_equal(outs[k].cpu().numpy(), np.stack(want)), (k, radii[k], nsamples[k])
        want_cnts.append(np.stack(want_cnt))
    only = U.ball_query_msg(x, c, radii, nsamples)                                     # count_host = NULL
    assert all(torch.equal(a, b) for a, b in zip(only, outs))
    # one count pointer NULL (the last scale's), behind guard words
    o = _Outs()
    xc = x.float().contiguous()
    outs2 = [o.new(*cent.shape, ns) for ns in nsamples]
    cnts2 = [o.new(*cent.shape) for _ in range(K - 1)] + [None]
    L.ball_query_msg_f32(xc, c, radii, nsamples, outs2, cnts2)
    o.check_guards()
    assert all(torch.equal(a, b) for a, b in zip(outs2, outs)) and all(torch.equal(a, b) for a, b in zip(cnts2[:-1], cnts))
    return want_cnts


def _kth_distances(pc, cent, nsample):
    """Per centre the float32 squared distances to its nsample-th and (nsample+1)-th nearest point (the centre counts), [B, s, 2]."""
    return np.array([[np.sort(sa_ref.sq_dists(pc[c], i))[[nsample - 1, nsample]] for i in cent[c]] for c in range(pc.shape[0])], dtype=np.float64)


def test_one_scale(synth):
    U = sub("utils.utils")
    pc = synth.clouds(5, 2, 100)
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), 10).cpu().numpy()
    for radius, nsample in ((0.2, 8), (0.05, 1), (5.0, 64)):
        _check(pc, cent, [radius], [nsample])


def test_three_scales_padded_and_truncated_in_one_call(synth):
    """n = 777, s = 33, nsamples (4, 64, 16), the radii chosen from the seeded cloud by the k-th-nearest distances as in
    test_ball_query_gpu.py and NOT in ascending order: scale 0 (nsample 4) above every centre's d_5 -- every ball truncated; scale 1
    (nsample 64) below most centres' d_64 -- most balls padded; scale 2 (nsample 16) the median d_16 -- a mix."""
    U = sub("utils.utils")
    pc = synth.clouds(5, 2, 777)
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), 33).cpu().numpy()
    nsamples = [4, 64, 16]
    radii = [float(np.sqrt(_kth_distances(pc, cent, 4)[..., 1].max()) * 1.001),
             float(np.sqrt(np.quantile(_kth_distances(pc, cent, 64)[..., 0], 0.1)) * 0.999),
             float(np.sqrt(np.median(_kth_distances(pc, cent, 16)[..., 0])))]
    assert not (radii[0] <= radii[1] <= radii[2]) and not (radii[0] >= radii[1] >= radii[2]), radii
    want = [np.stack([sa_ref.ball_query(pc[c], cent[c], r, ns)[1] for c in range(2)]) for r, ns in zip(radii, nsamples)]
    members0 = np.stack([sa_ref.ball_query(pc[c], cent[c], radii[0], 777)[1] for c in range(2)])
    assert (want[0] == 4).all() and (members0 > 4).all(), want[0]                      # every ball truncated
    assert (want[1] < 64).mean() > 0.5, want[1]                                        # most balls padded
    assert 0.2 < (want[2] < 16).mean() < 0.8, want[2]
    got = _check(pc, cent, radii, nsamples)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_four_scales_two_equal_radii(synth):
    U = sub("utils.utils")
    pc = synth.clouds(7, 2, 2048)
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), 256).cpu().numpy()
    cnt = _check(pc, cent, [0.2, 0.1, 0.2, 0.05], [32, 16, 8, 64])
    assert np.array_equal(np.minimum(cnt[0], 8), cnt[2])                               # scales 0 and 2: one radius, two nsample


def test_the_walk_goes_on_until_every_list_is_full():
    """The line-plus-cluster cloud of test_ball_query_gpu.py::test_members_past_the_first_step_are_found.  Centre 2 with radius 0.5 has the
    members 2, 130 and 299; with nsample 1 that list is full after the first 64 candidates, while the nsample-3 list of the same centre
    takes the members 130 and 299: a walk that ended when the FIRST list filled would lose them.  Asserted on the restatement first."""
    line = np.stack([10.0 * np.arange(300), np.zeros(300), np.zeros(300)], 1)
    line[130] = line[2]
    line[299] = line[2]
    cluster = np.array([5000.0, 7.0, -3.0]) + 0.01 * np.arange(11)[:, None]
    pc = np.concatenate([line, cluster]).astype(np.float32)[None]
    cent = np.array([[305, 2, 300, 310, 64]], dtype=np.int32)
    radii, nsamples = [0.5, 0.5, 15.0], [1, 3, 2]
    full_early, cnt_early = sa_ref.ball_query(pc[0], cent[0], radii[0], nsamples[0])
    late, cnt_late = sa_ref.ball_query(pc[0], cent[0], radii[1], nsamples[1])
    assert cnt_early[1] == 1 and full_early[1, 0] < 64                                 # full within the first step
    assert cnt_late[1] == 3 and late[1].tolist() == [2, 130, 299] and (late[1, 1:] >= 64).all()
    cnt = _check(pc, cent, radii, nsamples)
    assert cnt[1][0].tolist() == [3, 3, 3, 3, 1] and cnt[2][0].tolist() == [2, 2, 2, 2, 2]
    _check(pc, cent, [0.5, 0.5], [3, 1])                                               # the same with the short list last


def test_radius_zero_and_exact_boundaries_in_one_call():
    """The integer grid with duplicates of test_ball_query_gpu.py: radius 0 takes the duplicates only, and at radii 1.0 and 2.0 d == r2
    exactly for the axis neighbours, which are members."""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pc = np.concatenate([g, g[:64], np.zeros((128, 3), np.float32)], 0)[None]
    cent = np.array([[0, 5, 100, 341, 1023, 1024, 1024 + 5, pc.shape[1] - 1]], dtype=np.int32)
    cnt = _check(pc, cent, [0.0, 1.0, 2.0], [8, 40, 64])
    assert cnt[0][0, 1] == 2 and cnt[0][0, 2] == 1 and cnt[0][0, 0] == 8               # the copy, no copy, the origin's 130 copies truncated
    assert cnt[1][0, 3] == 7 and cnt[2][0, 3] == 32                                    # point 341 = (5, 5, 1): the counts of the existing grid test
    _check(pc, cent, [2.0, 0.0, 1.0, 1.0], [7, 64, 4, 64])


def test_rows_wider_than_three_columns(synth):
    U = sub("utils.utils")
    pc = synth.clouds(6, 2, 500, dims=9)                                               # ld = 9: columns 3 .. 8 must not matter
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), 20).cpu().numpy()
    cnt = _check(pc, cent, [0.15, 0.3], [4, 16])
    assert (cnt[0] < 4).any() and (cnt[0] == 4).any()
    x, c = torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda()
    narrow = U.ball_query_msg(x[..., :3].contiguous(), c, [0.15, 0.3], [4, 16])
    wide = U.ball_query_msg(x, c, [0.15, 0.3], [4, 16])
    assert all(torch.equal(a, b) for a, b in zip(narrow, wide))


def test_refusals_write_nothing(synth):
    U, L = sub("utils.utils"), sub("_lib")
    x = torch.from_numpy(synth.clouds(4, 1, 64)).cuda()
    c = torch.zeros((1, 4), dtype=torch.int32).cuda()

    def c_abi(xx, radii, nsamples, match):
        """the C entry point itself, on outputs in front of guard words: refused, the scale named, nothing written"""
        o, K, n = _Outs(), len(nsamples), max(len(nsamples), 1)
        outs = [o.new(1, 4, min(max(ns, 1), 64)) for ns in nsamples]
        cnts = [o.new(1, 4) for _ in nsamples]
        rc = L.lib().ampnet_ball_query_msg_f32(L.ptr(xx), 1, xx.shape[1], 3, L.ptr(c), 4, (ctypes.c_float * n)(*radii),
                                               (ctypes.c_int * n)(*nsamples), K, (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                               (ctypes.c_void_p * n)(*[t.data_ptr() for t in cnts]), L.stream_ptr(xx.device))
        with pytest.raises(L.AmpnetError, match=match):
            L.check(rc, "ampnet_ball_query_msg_f32")
        o.check_guards()
        assert o.untouched()

    c_abi(x, [], [], "K=0")
    c_abi(x, [0.1] * 5, [4] * 5, "K=5")
    c_abi(x, [0.1, 0.1], [4, 0], "scale 1.*nsample=0")
    c_abi(x, [0.1, 0.1, 0.2], [4, 4, 65], "scale 2")
    c_abi(x, [0.1, -1.0], [4, 4], "scale 1.*radius")
    c_abi(torch.zeros((1, 12289, 3), device="cuda"), [0.1, 0.2], [4, 4], "12289")
    with pytest.raises(L.AmpnetError):
        U.ball_query_msg(x, c, [], [])
    with pytest.raises(L.AmpnetError):
        U.ball_query_msg(x, c, [0.1] * 5, [4] * 5)
    with pytest.raises(L.AmpnetError):
        U.ball_query_msg(x, c, [0.1, 0.2], [4])
    with pytest.raises(IndexError):
        U.ball_query_msg(x, c, [0.1, 0.2], [4, 0])
    with pytest.raises(IndexError):
        U.ball_query_msg(x, c, [0.1, 0.2], [65, 4])
    with pytest.raises(L.AmpnetError, match="scale 1"):
        U.ball_query_msg(x, c, [0.1, -1.0], [4, 4])
    with pytest.raises(Exception, match="12289"):
        U.ball_query_msg(torch.zeros((1, 12289, 3), device="cuda"), c, [0.1, 0.2], [4, 4])      # coordinates must fit LDS
    with pytest.raises(IndexError):
        U.ball_query_msg(x, c + 64, [0.1, 0.2], [4, 4])
    with pytest.raises(IndexError):
        U.ball_query_msg(x, c - 1, [0.1, 0.2], [4, 4])
    with pytest.raises(Exception):
        U.ball_query_msg(x, c.long(), [0.1, 0.2], [4, 4])                      # centres must be int32
    with pytest.raises(Exception):
        U.ball_query_msg(x.cpu(), c, [0.1, 0.2], [4, 4])                       # no CPU fallback
    with pytest.raises(L.AmpnetError):
        L.ball_query_msg_f32(x.cpu(), c, [0.1], [4], [torch.empty((1, 4, 4), dtype=torch.int32, device="cuda")])
    assert [tuple(t.shape) for t in U.ball_query_msg(torch.zeros((1, 12288, 3), device="cuda"), c, [0.0, 1.0], [2, 3])] == [(1, 4, 2), (1, 4, 3)]
