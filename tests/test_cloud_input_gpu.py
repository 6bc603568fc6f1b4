"""The ragged input pipeline on the GPU (include/ampnet_hip.h: ampnet_cloud_input_f32; pn2_step.cloud_input) against (a) the chain of torch
operations it replaces -- amp_test._upload_clusters, the utils.pad_cloud_sizes gather and the torch.where of the targets -- bit for bit
with the augmentation off, and (b) the numpy restatement tests/cloud_input_ref.py with the shuffle and the rotation on: rows bit-equal
(the gathered features, then utils.rotate_point_cloud_z with the step's angle on x, y, z), targets and source rows equal.  Clouds of
1, 5, 90, 128 and 300 points padded to npoint = 128 (more than one workgroup, a workgroup that spans four clouds, a last workgroup that is
not full), and 128 + 129 points with nothing to pad; column 9 holds every class code that matters.  Every test takes well under a second."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import cloud_input_ref as R                        # noqa: E402

pytestmark = pytest.mark.gpu

CODES = np.array([3, 4, 5, 14, 15, 0, 2, 255, 300.0, -1.0], dtype=np.float32)
CASES = {"padded": ([1, 5, 90, 128, 300], 128), "exact": ([128, 129], 128), "one": ([77], 128), "wide": ([700, 3, 513], 256)}


def _clusters(synth, sizes, seed=60):
    """list of [n, 10] float32 CPU tensors: x, y, z like a cluster's, six more features, every code of CODES in turn."""
    out = []
    for i, n in enumerate(sizes):
        x = np.concatenate([synth.clouds(seed + i, 1, n)[0], synth.uniform(seed + 100 + i, (n, 6), -1.0, 1.0)], -1)
        codes = CODES[(np.arange(n) + 3 * i) % len(CODES)]
        out.append(torch.from_numpy(np.concatenate([x, codes[:, None]], -1).astype(np.float32)))
    return out


def _raw(clusters):
    return torch.cat(clusters, 0).cuda()


@pytest.mark.parametrize("case", list(CASES))
def test_without_augmentation_the_kernel_writes_the_bits_of_the_torch_chain(synth, case):
    S, A, U = sub("pointNet.pn2_step"), sub("pointNet.amp_test"), sub("utils.utils")
    sizes, npoint = CASES[case]
    clusters = _clusters(synth, sizes)
    rows0, tg0, _ = A._upload_clusters(clusters, torch.device("cuda"))
    padded, _, gather, keep = U.pad_cloud_sizes(sizes, npoint)
    own = np.zeros(len(gather), dtype=bool)
    own[keep] = True
    g = torch.from_numpy(gather).cuda()
    want_rows, want_tg = rows0[g], torch.where(torch.from_numpy(own).cuda(), tg0[g], -1)
    rows, tg, p, src = S.cloud_input(_raw(clusters), sizes, npoint, train=False, seed=99, step=5, want_src=True)
    assert p == padded and rows.dtype == torch.float32 and tg.dtype == torch.int64 and src.dtype == torch.int32
    assert tuple(rows.shape) == (sum(padded), 9) and tuple(tg.shape) == tuple(src.shape) == (sum(padded),)
    assert torch.equal(rows.view(torch.int32), want_rows.view(torch.int32)) and torch.equal(tg, want_tg)
    assert torch.equal(src.long(), g)
    assert set(tg.unique().tolist()) >= ({0, 1, 2, 3, 4} if max(sizes) >= 10 else {0})
    three = S.cloud_input(_raw(clusters), sizes, npoint, train=False, seed=1, step=2)
    assert len(three) == 3 and torch.equal(three[0], rows) and torch.equal(three[1], tg)      # eval ignores the keys; src is optional


@pytest.mark.parametrize("case", list(CASES))
def test_with_augmentation_the_kernel_equals_the_numpy_restatement(synth, case):
    S, U = sub("pointNet.pn2_step"), sub("utils.utils")
    sizes, npoint = CASES[case]
    clusters = _clusters(synth, sizes)
    raw = torch.cat(clusters, 0).numpy()
    seed, step = 0x6A09E667, 3
    rows, tg, p, src = S.cloud_input(_raw(clusters), sizes, npoint, train=True, seed=seed, step=step, want_src=True)
    _, want_tg, want_src, want_p = R.cloud_input(raw, sizes, npoint, seed, step, permute=True, rotate=True)
    assert p == want_p and np.array_equal(src.cpu().numpy(), want_src) and np.array_equal(tg.cpu().numpy(), want_tg)
    want_rows = raw[want_src, :9].copy()
    angle = S.step_angle(seed, step)
    assert angle == R.step_angle(seed, step) and angle != 0.0
    want_rows[:, :3] = U.rotate_point_cloud_z(want_rows[None, :, :3], angle)[0]
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want_rows.view(np.int32))
    # src over a cloud's first n rows is a permutation of the cloud's rows; the padding repeats it cyclically
    src, r0, o0 = src.cpu().numpy().astype(np.int64), 0, 0
    for n, pb in zip(sizes, p):
        mine = src[o0:o0 + pb]
        assert np.array_equal(np.sort(mine[:n]), r0 + np.arange(n)) and np.array_equal(mine, mine[np.arange(pb) % n])
        if n >= 64:
            assert not np.array_equal(mine[:n], r0 + np.arange(n))
        r0, o0 = r0 + n, o0 + pb
    assert (tg.cpu().numpy() == -1).sum() == sum(p) - sum(sizes)


def test_a_step_is_a_function_of_seed_and_step(synth):
    S = sub("pointNet.pn2_step")
    sizes, npoint = CASES["padded"]
    raw = _raw(_clusters(synth, sizes))
    a = S.cloud_input(raw, sizes, npoint, train=True, seed=7, step=0, want_src=True)
    b = S.cloud_input(raw, sizes, npoint, train=True, seed=7, step=0, want_src=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for seed, step in ((7, 1), (8, 0)):
        c = S.cloud_input(raw, sizes, npoint, train=True, seed=seed, step=step, want_src=True)
        assert not torch.equal(a[3], c[3]) and not torch.equal(a[0], c[0])
    # the shuffle alone and the rotation alone, through the typed wrapper
    L = sub("_lib")
    off = torch.tensor([[0, 1, 6, 96, 224, 524], [0, 128, 256, 384, 512, 812]], dtype=torch.int32, device="cuda")
    rows, tg, src = torch.empty(812, 9, device="cuda"), torch.empty(812, dtype=torch.int64, device="cuda"), torch.empty(812, dtype=torch.int32, device="cuda")
    L.cloud_input_f32(raw, off[0], off[1], 7, 0, True, False, 1.0, 0.0, rows, tg, src)
    assert torch.equal(src, a[3]) and torch.equal(rows, raw[src.long(), :9])
    L.cloud_input_f32(raw, off[0], off[1], 7, 0, False, True, 0.0, 1.0, rows, tg, None)            # a quarter turn: (x, y) -> (-y, x)
    plain = S.cloud_input(raw, sizes, npoint, train=False, seed=0, step=0)[0]
    assert torch.equal(rows[:, 0], -plain[:, 1]) and torch.equal(rows[:, 1], plain[:, 0]) and torch.equal(rows[:, 2:], plain[:, 2:])


def test_bad_arguments_are_ampnet_errors(synth):
    S, L = sub("pointNet.pn2_step"), sub("_lib")
    sizes, npoint = CASES["exact"]
    raw = _raw(_clusters(synth, sizes))
    kw = dict(train=True, seed=1, step=0)
    with pytest.raises(L.AmpnetError, match="GPU"):
        S.cloud_input(raw.cpu(), sizes, npoint, **kw)
    with pytest.raises(L.AmpnetError, match="tile"):
        S.cloud_input(raw, [128, 128], npoint, **kw)
    with pytest.raises(L.AmpnetError, match="tile"):
        S.cloud_input(raw, [], npoint, **kw)
    with pytest.raises(L.AmpnetError, match="tile"):
        S.cloud_input(raw, [257, 0], npoint, **kw)
    with pytest.raises(L.AmpnetError, match=r"\[total, 10\]"):
        S.cloud_input(raw[:, :9].contiguous(), sizes, npoint, **kw)
    with pytest.raises(L.AmpnetError, match=r"\[total, 10\]"):
        S.cloud_input(raw.double(), sizes, npoint, **kw)
    off = torch.tensor([0, 128, 257], dtype=torch.int32, device="cuda")
    rows, tg = torch.empty(257, 9, device="cuda"), torch.empty(257, dtype=torch.int64, device="cuda")
    good = dict(raw=raw, in_off=off, out_off=off, seed=1, step=0, permute=True, rotate=False, cos_a=1.0, sin_a=0.0, rows=rows, targets=tg)
    L.cloud_input_f32(**good)
    for name in ("raw", "in_off", "out_off", "rows", "targets"):
        with pytest.raises(L.AmpnetError, match=name + " is None"):
            L.cloud_input_f32(**{**good, name: None})
    for name, bad in (("rows", torch.empty(257, 10, device="cuda")), ("targets", tg[:256]), ("out_off", off[:2]), ("in_off", off[:1]),
                      ("targets", tg.int()), ("in_off", off.long()), ("src", torch.empty(256, dtype=torch.int32, device="cuda"))):
        with pytest.raises(L.AmpnetError):
            L.cloud_input_f32(**{**good, name: bad})
    with pytest.raises(L.AmpnetError, match="bad totals"):                      # fewer output rows than input rows: refused by the C ABI
        L.cloud_input_f32(**{**good, "rows": rows[:200], "targets": tg[:200]})
