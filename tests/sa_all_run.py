"""What the GPU tests of the group_all set abstraction share (tests/test_sa_all_gpu.py, tests/test_sa_all_backward_gpu.py): the seeded
cases with their float64 tape, computed once, and the guarded call of the forward kernel.  Test infrastructure."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import sa_all_ref as R                             # noqa: E402

GUARD = -1234.5


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, forward tape) of a case, computed once and shared (nobody writes to them)."""
    i = R.case_inputs(sub("synthetic"), name)
    tape, _ = R.forward_tape(i["xyz"], i["feats"], i["layers"], i["eps"])
    return i, tape


def to_gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_forward(L, i, xyz=None, feats="auto", layers=None, want_arg=True, prefill=float("nan"), ws_short=0, out_shape=None, arg_shape=None):
    """-> (out, arg or None) as numpy.  out, arg and the workspace start as NaN / -1 / NaN bit patterns; out and arg live in front of 64
    guard elements, which the kernels must leave alone."""
    xyz = i["xyz"] if xyz is None else xyz
    f = i["feats"] if isinstance(feats, str) else feats
    layers = i["layers"] if layers is None else layers
    B, n = xyz.shape[:2]
    C = layers[-1][0].shape[0]

    def guarded(shape, dtype, fill, guard):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), fill, dtype=dtype, device="cuda")
        buf[numel:] = guard
        return buf, buf[:numel].view(*shape)

    obuf, out = guarded(out_shape or (B, C), torch.float32, prefill, GUARD)
    abuf, arg = guarded(arg_shape or (B, C), torch.int32, -1, -77) if want_arg else (None, None)
    try:
        need = L.sa_all_forward_workspace_bytes(0 if f is None else f.shape[2], B, n, [layer[0].shape[0] for layer in layers])
    except L.AmpnetError:
        need = 1 << 20                                             # a refused shape: sa_all_forward_f32 has to say so itself
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device="cuda").view(torch.uint8)[:need - ws_short]
    L.sa_all_forward_f32(to_gpu(xyz), to_gpu(f), [tuple(to_gpu(a) for a in layer) for layer in layers], [R.BN_EPS] * len(layers), out, ws, arg_out=arg)
    torch.cuda.synchronize()
    assert (obuf[-64:] == GUARD).all() and (abuf is None or (abuf[-64:] == -77).all()), "written past the end"
    return out.cpu().numpy(), None if arg is None else arg.cpu().numpy()
