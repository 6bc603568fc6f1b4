"""ctypes binding of libampnet_hip.so (include/ampnet_hip.h).

There is no CPU fallback: if the library is missing, fails to load, or reports an error, the caller
gets an exception.  torch is imported first so that the HIP runtime torch already mapped
(its bundled libamdhip64, SONAME libamdhip64.so.7) is the one this library binds to -- two HIP runtimes in
one process would not share device pointers.
"""
import contextlib
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMPNET_LIB_PATH") or os.path.join(_HERE, "libampnet_hip.so")   # the override is for A/B runs of two builds
ABI_VERSION = 17

_lib = None


class AmpnetError(RuntimeError):
    pass


def _hip_runtimes_mapped():
    seen = set()
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64" in line:
                    seen.add(line.split()[-1])
    except OSError:
        pass
    return seen


def lib():
    """The loaded library (loads on first use; raises AmpnetError when it cannot)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmpnetError(f"{LIB_PATH} is missing: run `python __graft_entry__.py build` (hipcc, gfx950). "
                          "There is no CPU fallback for the HIP path.")
    try:
        l = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise AmpnetError(f"cannot load {LIB_PATH}: {e}") from e
    rts = _hip_runtimes_mapped()
    if len(rts) > 1:
        raise AmpnetError(f"two HIP runtimes mapped in one process: {sorted(rts)}")
    l.ampnet_abi_version.restype = ctypes.c_int
    l.ampnet_last_error.restype = ctypes.c_char_p
    v = l.ampnet_abi_version()
    if v != ABI_VERSION and not (os.environ.get("AMPNET_LIB_PATH") and v < ABI_VERSION):
        # (an OLDER build named explicitly through AMPNET_LIB_PATH is accepted: same-box A/B runs against a previous round's library,
        # tools/ab_lib.sh -- entry points added since then are simply absent from it)
        raise AmpnetError(f"libampnet_hip.so ABI {v} != expected {ABI_VERSION}: rebuild")
    _lib = l
    return l


PRECISIONS = {"fp32": 0, "f32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "bf16_train": 2, "bf16_store": 3,
              "f32x3": 4, "fp32_split": 4}


def set_matrix_precision(mode):
    """'fp32' (default, exact fp32 products: the mode the parity figures hold in), 'bf16' (the forward per-point layers
    round their MFMA operands to bf16, fp32 accumulation) 'bf16_train' (forward and the fused backward of those layers) or 'bf16_store' (bf16_train + the
    activations kept for the backward stored as bf16) or 'f32x3' (fp32 results from the bf16 matrix pipe: three-term bf16 split of
    both operands of the MFMA-bound layers, six exact partial products, fp32 accumulation; include/ampnet_hip.h: ampnet_set_matrix_precision)."""
    if mode not in PRECISIONS:
        raise AmpnetError(f"unknown matrix precision {mode!r}: one of {sorted(PRECISIONS)}")
    check(lib().ampnet_set_matrix_precision(PRECISIONS[mode]), "ampnet_set_matrix_precision")


_MODE_NAMES = {0: "fp32", 1: "bf16", 2: "bf16_train", 3: "bf16_store", 4: "f32x3"}
PRECISION_NAMES = ("fp32", "f32x3", "bf16", "bf16_train", "bf16_store")   # the canonical names: what --precision offers


def get_matrix_precision():
    """The process-wide default (set_matrix_precision); a precision_scope does not show here."""
    return _MODE_NAMES[lib().ampnet_get_matrix_precision()]


def effective_matrix_precision():
    """What an entry point called on THIS thread would dispatch on: the innermost precision_scope, else the process-wide default."""
    return _MODE_NAMES[lib().ampnet_effective_matrix_precision()]


def checked_precision(mode):
    if mode not in PRECISIONS:
        raise ValueError(f"unknown matrix precision {mode!r}: one of {list(PRECISION_NAMES)}")
    return mode


@contextlib.contextmanager
def precision_scope(mode):
    """Runs the body with `mode` as the matrix precision of every C-ABI call made on this thread (include/ampnet_hip.h:
    ampnet_precision_scope_begin / _end), whatever the process-wide default is; other threads and the default are untouched.
    mode=None: no scope, the calls follow the default.  The scope is closed when the body raises, too."""
    if mode is None:
        yield
        return
    L = lib()
    check(L.ampnet_precision_scope_begin(PRECISIONS[checked_precision(mode)]), "ampnet_precision_scope_begin")
    try:
        yield
    finally:
        check(L.ampnet_precision_scope_end(), "ampnet_precision_scope_end")


def resolve_precision(explicit=None):
    """The precision a driver runs in: the explicit value (a keyword argument, a --precision flag), else AMPNET_PRECISION from the
    environment, else None = follow the library's process-wide default (fp32 unless set_matrix_precision changed it)."""
    mode = explicit if explicit is not None else (os.environ.get("AMPNET_PRECISION") or None)
    return None if mode is None else checked_precision(mode)


def describe_precision(mode):
    """For the line a driver logs at start: the mode's name, or what None falls back to."""
    return mode if mode is not None else f"library default ({get_matrix_precision()})"


def tape_conflict(a, b):
    """True when two precisions cannot share a train step: 'bf16_store' keeps the saved activations as bf16, every other mode as fp32."""
    return a is not None and b is not None and (PRECISIONS[a] == 3) != (PRECISIONS[b] == 3)


def check(rc, what):
    if rc != 0:
        msg = lib().ampnet_last_error()
        raise AmpnetError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device (or host) pointer of a contiguous torch tensor as c_void_p; None -> NULL."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_contiguous():
        raise AmpnetError("tensor handed to the C ABI must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """Current torch HIP stream as a void* for the C ABI."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t, name):
    if not t.is_cuda:
        raise AmpnetError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")


# ---- PointNet++ grouping (include/ampnet_hip.h: ampnet_ball_query_f32, ampnet_sa_forward_f32) ---------------------------------------
SA_MAX_NSAMPLE, SA_MAX_LAYERS, SA_MAX_CIN, SA_MAX_COUT = 64, 3, 320, 256
SA_WORKSPACE_BYTES = SA_MAX_LAYERS * 2 * SA_MAX_COUT * 4


def ball_query_f32(xyz, centres, radius, nsample, out, count=None):
    """xyz [B, N, ld] float32, centres [B, S] int32, out [B, S, nsample] int32, count [B, S] int32 or None: contiguous GPU tensors."""
    B, N, ld = xyz.shape
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_ball_query_f32(ptr(xyz), B, N, ld, ptr(centres), centres.shape[1], ctypes.c_float(radius), int(nsample), ptr(out),
                                         ptr(count), stream_ptr(xyz.device))
    check(rc, "ampnet_ball_query_f32")


def _mlp_tables(prefix, layers, cin, eps, workspace, workspace_bytes):
    """What the fused forwards (sa_forward_f32, fp_forward_f32) share: every layer is six contiguous float32 GPU tensors of shapes
    [(cout, cin)] + [(cout,)] * 5 chained from cin (the kernels trust these shapes: a short tensor would be read past its end), eps has one
    entry per layer, the workspace holds workspace_bytes GPU bytes -> the (pointer table, couts, epss) ctypes arrays of the C ABI."""
    L = len(layers)
    for i, layer in enumerate(layers):
        cout = int(layer[0].shape[0])
        want = [(cout, cin)] + [(cout,)] * 5
        if len(layer) != 6 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                                  for t, w in zip(layer, want)):
            raise AmpnetError(f"{prefix}: layer {i} needs six contiguous float32 GPU tensors of shapes {want}, "
                              f"got {[tuple(t.shape) for t in layer]}")
        cin = cout
    if len(eps) != L:
        raise AmpnetError(f"{prefix}: eps has {len(eps)} entries for {L} layers")
    if workspace.numel() * workspace.element_size() < workspace_bytes or not workspace.is_cuda:
        raise AmpnetError(f"{prefix}: the workspace must hold {workspace_bytes} GPU bytes")
    tensors = [t for layer in layers for t in layer]
    return ((ctypes.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors]),
            (ctypes.c_int * max(L, 1))(*[int(layer[0].shape[0]) for layer in layers]),
            (ctypes.c_float * max(L, 1))(*[float(e) for e in eps]))


def sa_forward_f32(xyz, centres, group_idx, feats, layers, eps, out, workspace):
    """One fused set-abstraction layer.  layers: per layer the six contiguous float32 GPU tensors (weight [cout, cin], conv bias, BatchNorm
    weight, bias, running_mean, running_var); eps: per layer the BatchNorm eps; feats [B, N, D] or None; out [B, S, cout_last]."""
    B, N, ld = xyz.shape
    L = len(layers)
    for name, t, dt in (("xyz", xyz, torch.float32), ("centres", centres, torch.int32), ("group_idx", group_idx, torch.int32),
                        ("feats", feats, torch.float32), ("out", out, torch.float32)):
        if t is not None and (not t.is_cuda or t.dtype != dt):
            raise AmpnetError(f"sa_forward: {name} must be a {dt} GPU tensor")
    S = centres.shape[1]
    if tuple(centres.shape) != (B, S) or group_idx.dim() != 3 or tuple(group_idx.shape[:2]) != (B, S) \
            or (feats is not None and tuple(feats.shape[:2]) != (B, N)) or (L and tuple(out.shape) != (B, S, int(layers[-1][0].shape[0]))):
        raise AmpnetError("sa_forward: centres [B, S], group_idx [B, S, nsample], feats [B, N, D], out [B, S, cout] do not agree with xyz [B, N, ld]")
    table, couts, epss = _mlp_tables("sa_forward", layers, 3 + (0 if feats is None else feats.shape[2]), eps, workspace, SA_WORKSPACE_BYTES)
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_forward_f32(ptr(xyz), B, N, ld, ptr(centres), centres.shape[1], ptr(group_idx), group_idx.shape[2], ptr(feats),
                                         0 if feats is None else feats.shape[2], table, couts, epss, L, ptr(out), ptr(workspace),
                                         ctypes.c_size_t(workspace.numel() * workspace.element_size()), stream_ptr(xyz.device))
    check(rc, "ampnet_sa_forward_f32")


# ---- PointNet++ feature propagation (include/ampnet_hip.h: ampnet_three_nn_f32, ampnet_fp_forward_f32) ------------------------------
THREE_NN_MAX_S = 12288
FP_MAX_LAYERS, FP_MAX_CIN, FP_MAX_COUT = 3, 512, 256
FP_WORKSPACE_BYTES = FP_MAX_LAYERS * 2 * FP_MAX_COUT * 4


def three_nn_f32(fine, coarse, idx, dist2):
    """fine [B, N, ld1] float32, coarse [B, S, ld2] float32, idx [B, N, k] int32, dist2 [B, N, k] float32, k = min(3, S): contiguous GPU
    tensors."""
    B, N, ld1 = fine.shape
    S, ld2 = coarse.shape[1], coarse.shape[2]
    k = min(3, S)
    for name, t, dt in (("fine", fine, torch.float32), ("coarse", coarse, torch.float32), ("idx", idx, torch.int32), ("dist2", dist2, torch.float32)):
        if not t.is_cuda or t.dtype != dt:
            raise AmpnetError(f"three_nn: {name} must be a {dt} GPU tensor")
    if coarse.shape[0] != B or tuple(idx.shape) != (B, N, k) or tuple(dist2.shape) != (B, N, k):
        raise AmpnetError(f"three_nn: coarse [B, S, ld2], idx and dist2 [B, N, min(3, S)] do not agree with fine {tuple(fine.shape)}")
    with torch.cuda.device(fine.device):
        rc = lib().ampnet_three_nn_f32(ptr(fine), B, N, ld1, ptr(coarse), S, ld2, ptr(idx), ptr(dist2), stream_ptr(fine.device))
    check(rc, "ampnet_three_nn_f32")


def fp_forward_f32(points1, points2, idx, dist2, layers, eps, out, workspace):
    """One fused feature-propagation layer.  points1 [B, N, D1] or None, points2 [B, S, D2], idx int32 / dist2 float32 [B, N, k] (the output
    of three_nn_f32), layers and eps as in sa_forward_f32 with cin_0 = D1 + D2, out [B, N, cout_last]."""
    L = len(layers)
    for name, t, dt in (("points1", points1, torch.float32), ("points2", points2, torch.float32), ("idx", idx, torch.int32),
                        ("dist2", dist2, torch.float32), ("out", out, torch.float32)):
        if t is not None and (not t.is_cuda or t.dtype != dt or t.dim() != 3):
            raise AmpnetError(f"fp_forward: {name} must be a 3-d {dt} GPU tensor")
    B, N, k = idx.shape
    S, D2 = points2.shape[1], points2.shape[2]
    D1 = 0 if points1 is None else points1.shape[2]
    if points2.shape[0] != B or tuple(dist2.shape) != (B, N, k) or (points1 is not None and tuple(points1.shape[:2]) != (B, N)) \
            or (L and tuple(out.shape) != (B, N, int(layers[-1][0].shape[0]))):
        raise AmpnetError("fp_forward: points1 [B, N, D1], points2 [B, S, D2], dist2 [B, N, k], out [B, N, cout] do not agree with "
                          f"idx {tuple(idx.shape)}")
    table, couts, epss = _mlp_tables("fp_forward", layers, D1 + D2, eps, workspace, FP_WORKSPACE_BYTES)
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_forward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss, L, ptr(out),
                                         ptr(workspace), ctypes.c_size_t(workspace.numel() * workspace.element_size()),
                                         stream_ptr(points2.device))
    check(rc, "ampnet_fp_forward_f32")


def fp_backward_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_backward_f32 needs for points1 [B, N, D1], points2 [B, S, D2] and layers of widths `couts` (include/ampnet_hip.h:
    ampnet_fp_backward_workspace_bytes); a shape outside the kernel's limits is an AmpnetError that names the limit."""
    couts = [int(c) for c in couts]
    fn = lib().ampnet_fp_backward_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = fn(int(D1), int(D2), int(B), int(N), (ctypes.c_int * max(len(couts), 1))(*couts), len(couts))
    if not need:
        check(-1, "ampnet_fp_backward_workspace_bytes")
    return int(need)


def fp_backward_f32(points1, points2, idx, dist2, layers, eps, dout, dpoints1, dpoints2, grads, workspace):
    """The backward of fp_forward_f32 with the running statistics frozen.  points1 .. eps: the forward's arguments; dout [B, N, cout_last];
    dpoints1 [B, N, D1] (None exactly when points1 is None) and dpoints2 [B, S, D2]: written; grads: per layer the four contiguous float32
    GPU tensors (dW [cout, cin], dbias [cout], dgamma [cout], dbeta [cout]), written; workspace: fp_backward_workspace_bytes(...) GPU
    bytes."""
    L = len(layers)
    for name, t, dt in (("points1", points1, torch.float32), ("points2", points2, torch.float32), ("idx", idx, torch.int32),
                        ("dist2", dist2, torch.float32), ("dout", dout, torch.float32), ("dpoints1", dpoints1, torch.float32),
                        ("dpoints2", dpoints2, torch.float32)):
        if t is not None and (not t.is_cuda or t.dtype != dt or t.dim() != 3):
            raise AmpnetError(f"fp_backward: {name} must be a 3-d {dt} GPU tensor")
    B, N, k = idx.shape
    S, D2 = points2.shape[1], points2.shape[2]
    D1 = 0 if points1 is None else points1.shape[2]
    if points2.shape[0] != B or tuple(dist2.shape) != (B, N, k) or (points1 is not None and tuple(points1.shape[:2]) != (B, N)):
        raise AmpnetError(f"fp_backward: points1 [B, N, D1], points2 [B, S, D2], dist2 [B, N, k] do not agree with idx {tuple(idx.shape)}")
    if (dpoints1 is None) != (points1 is None):
        raise AmpnetError(f"fp_backward: dpoints1 must be None exactly when points1 is (D1 = {D1}), got "
                          f"{None if dpoints1 is None else tuple(dpoints1.shape)}")
    if dpoints1 is not None and tuple(dpoints1.shape) != tuple(points1.shape):
        raise AmpnetError(f"fp_backward: dpoints1 {tuple(dpoints1.shape)} must have the shape of points1 {tuple(points1.shape)}")
    if tuple(dpoints2.shape) != tuple(points2.shape):
        raise AmpnetError(f"fp_backward: dpoints2 {tuple(dpoints2.shape)} must have the shape of points2 {tuple(points2.shape)}")
    table, couts, epss = _mlp_tables("fp_backward", layers, D1 + D2, eps, workspace, 0)
    if L and tuple(dout.shape) != (B, N, int(layers[-1][0].shape[0])):
        raise AmpnetError(f"fp_backward: dout {tuple(dout.shape)} must be [B, N, cout_last] = {[B, N, int(layers[-1][0].shape[0])]}")
    if len(grads) != L:
        raise AmpnetError(f"fp_backward: grads has {len(grads)} entries for {L} layers")
    for i, (layer, g) in enumerate(zip(layers, grads)):
        want = [tuple(layer[0].shape)] + [tuple(layer[1].shape)] * 3
        if len(g) != 4 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t, w in zip(g, want)):
            raise AmpnetError(f"fp_backward: the gradients of layer {i} must be four contiguous float32 GPU tensors of shapes {want}, "
                              f"got {[tuple(t.shape) for t in g]}")
    need = fp_backward_workspace_bytes(D1, D2, B, N, [int(layer[0].shape[0]) for layer in layers])
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise AmpnetError(f"fp_backward: the workspace holds {have} bytes, the shape needs {need} GPU bytes")
    gtensors = [t for g in grads for t in g]
    gtable = (ctypes.c_void_p * max(len(gtensors), 1))(*[t.data_ptr() for t in gtensors])
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_backward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss, L,
                                          ptr(dout), ptr(dpoints1), ptr(dpoints2), gtable, ptr(workspace), ctypes.c_size_t(have),
                                          stream_ptr(points2.device))
    check(rc, "ampnet_fp_backward_f32")


# ---- train-mode feature propagation (include/ampnet_hip.h: ampnet_fp_train_forward_f32, ampnet_fp_train_backward_f32) ----------------
def _fp_train_workspace_bytes(which, D1, D2, B, N, couts):
    couts = [int(c) for c in couts]
    name = f"ampnet_fp_train_{which}_workspace_bytes"
    fn = getattr(lib(), name)
    fn.restype = ctypes.c_size_t
    need = fn(int(D1), int(D2), int(B), int(N), (ctypes.c_int * max(len(couts), 1))(*couts), len(couts))
    if not need:
        check(-1, name)
    return int(need)


def fp_train_forward_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_train_forward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _fp_train_workspace_bytes("forward", D1, D2, B, N, couts)


def fp_train_backward_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_train_backward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _fp_train_workspace_bytes("backward", D1, D2, B, N, couts)


def _fp_train_shapes(prefix, points1, points2, idx, dist2, extra):
    for name, t, dt in (("points1", points1, torch.float32), ("points2", points2, torch.float32), ("idx", idx, torch.int32),
                        ("dist2", dist2, torch.float32)) + tuple(extra):
        if t is not None and (not t.is_cuda or t.dtype != dt or t.dim() != 3):
            raise AmpnetError(f"{prefix}: {name} must be a 3-d {dt} GPU tensor")
    B, N, k = idx.shape
    S, D2 = points2.shape[1], points2.shape[2]
    D1 = 0 if points1 is None else points1.shape[2]
    if points2.shape[0] != B or tuple(dist2.shape) != (B, N, k) or (points1 is not None and tuple(points1.shape[:2]) != (B, N)):
        raise AmpnetError(f"{prefix}: points1 [B, N, D1], points2 [B, S, D2], dist2 [B, N, k] do not agree with idx {tuple(idx.shape)}")
    return B, N, k, S, D1, D2


def _fp_saved(prefix, name, t, sum_c, null_ok=False):
    if t is None and null_ok:                                   # (NULL: the C ABI refuses it by name)
        return
    if t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (sum_c,):
        raise AmpnetError(f"{prefix}: {name} must be a contiguous float32 GPU tensor of sum(cout) = {sum_c} elements, got "
                          f"{None if t is None else tuple(t.shape)}")


def fp_train_forward_f32(points1, points2, idx, dist2, layers, eps, momentum, out, save_mean, save_invstd, workspace):
    """One fused feature-propagation layer with batch-statistics BatchNorm.  The arguments of fp_forward_f32; running_mean and running_var
    (entries 4 and 5 of every layer) are UPDATED IN PLACE with `momentum` (a float in [0, 1]); save_mean / save_invstd [sum of couts]:
    written, layer l at the offset of the layers before it; workspace: fp_train_forward_workspace_bytes(...) GPU bytes."""
    L = len(layers)
    B, N, k, S, D1, D2 = _fp_train_shapes("fp_train_forward", points1, points2, idx, dist2, (("out", out, torch.float32),))
    if L and tuple(out.shape) != (B, N, int(layers[-1][0].shape[0])):
        raise AmpnetError(f"fp_train_forward: out {tuple(out.shape)} must be [B, N, cout_last] = {[B, N, int(layers[-1][0].shape[0])]}")
    if momentum is None:
        raise AmpnetError("fp_train_forward: momentum=None (the cumulative average) is not built; give a float in [0, 1]")
    table, couts, epss = _mlp_tables("fp_train_forward", layers, D1 + D2, eps, workspace, 0)
    sum_c = sum(int(layer[0].shape[0]) for layer in layers)
    _fp_saved("fp_train_forward", "save_mean", save_mean, sum_c, null_ok=True)
    _fp_saved("fp_train_forward", "save_invstd", save_invstd, sum_c, null_ok=True)
    have = workspace.numel() * workspace.element_size()
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_train_forward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss, L,
                                               ctypes.c_float(float(momentum)), ptr(out), ptr(save_mean), ptr(save_invstd), ptr(workspace),
                                               ctypes.c_size_t(have), stream_ptr(points2.device))
    check(rc, "ampnet_fp_train_forward_f32")


def fp_train_backward_f32(points1, points2, idx, dist2, layers, eps, save_mean, save_invstd, dout, dpoints1, dpoints2, grads, workspace):
    """The backward of fp_train_forward_f32 through the batch statistics.  layers: per layer (weight, conv bias, BatchNorm weight, bias) --
    further entries are ignored; save_mean / save_invstd: what the forward wrote (never recomputed); dout, dpoints1, dpoints2, grads as in
    fp_backward_f32 (dbias is written as zeros); workspace: fp_train_backward_workspace_bytes(...) GPU bytes."""
    L = len(layers)
    B, N, k, S, D1, D2 = _fp_train_shapes("fp_train_backward", points1, points2, idx, dist2,
                                          (("dout", dout, torch.float32), ("dpoints1", dpoints1, torch.float32),
                                           ("dpoints2", dpoints2, torch.float32)))
    if (dpoints1 is None) != (points1 is None):
        raise AmpnetError(f"fp_train_backward: dpoints1 must be None exactly when points1 is (D1 = {D1}), got "
                          f"{None if dpoints1 is None else tuple(dpoints1.shape)}")
    if dpoints1 is not None and tuple(dpoints1.shape) != tuple(points1.shape):
        raise AmpnetError(f"fp_train_backward: dpoints1 {tuple(dpoints1.shape)} must have the shape of points1 {tuple(points1.shape)}")
    if tuple(dpoints2.shape) != tuple(points2.shape):
        raise AmpnetError(f"fp_train_backward: dpoints2 {tuple(dpoints2.shape)} must have the shape of points2 {tuple(points2.shape)}")
    sum_c = sum(int(layer[0].shape[0]) for layer in layers)
    _fp_saved("fp_train_backward", "save_mean", save_mean, sum_c)
    _fp_saved("fp_train_backward", "save_invstd", save_invstd, sum_c)
    slotted, off = [], 0
    for layer in layers:                                        # slots 4 and 5 of the C ABI: the layer's saved statistics
        c = int(layer[0].shape[0])
        slotted.append(tuple(layer[:4]) + (save_mean[off:off + c], save_invstd[off:off + c]))
        off += c
    table, couts, epss = _mlp_tables("fp_train_backward", slotted, D1 + D2, eps, workspace, 0)
    if L and tuple(dout.shape) != (B, N, int(layers[-1][0].shape[0])):
        raise AmpnetError(f"fp_train_backward: dout {tuple(dout.shape)} must be [B, N, cout_last] = {[B, N, int(layers[-1][0].shape[0])]}")
    if len(grads) != L:
        raise AmpnetError(f"fp_train_backward: grads has {len(grads)} entries for {L} layers")
    for i, (layer, g) in enumerate(zip(layers, grads)):
        want = [tuple(layer[0].shape)] + [tuple(layer[1].shape)] * 3
        if len(g) != 4 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t, w in zip(g, want)):
            raise AmpnetError(f"fp_train_backward: the gradients of layer {i} must be four contiguous float32 GPU tensors of shapes {want}, "
                              f"got {[tuple(t.shape) for t in g]}")
    gtensors = [t for g in grads for t in g]
    gtable = (ctypes.c_void_p * max(len(gtensors), 1))(*[t.data_ptr() for t in gtensors])
    have = workspace.numel() * workspace.element_size()
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_train_backward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss, L,
                                                ptr(dout), ptr(dpoints1), ptr(dpoints2), gtable, ptr(workspace), ctypes.c_size_t(have),
                                                stream_ptr(points2.device))
    check(rc, "ampnet_fp_train_backward_f32")


# ---- the set-abstraction backward (include/ampnet_hip.h: ampnet_sa_backward_f32) -------------------------------------------------------
def sa_backward_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_backward_f32 needs for feats [B, N, D], S centres per cloud, groups of nsample and layers of widths `couts`
    (include/ampnet_hip.h: ampnet_sa_backward_workspace_bytes); a shape outside the kernel's limits is an AmpnetError that names the limit."""
    couts = [int(c) for c in couts]
    fn = lib().ampnet_sa_backward_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = fn(int(D), int(B), int(S), int(nsample), (ctypes.c_int * max(len(couts), 1))(*couts), len(couts))
    if not need:
        check(-1, "ampnet_sa_backward_workspace_bytes")
    return int(need)


def sa_backward_f32(xyz, centres, group_idx, feats, layers, eps, dout, dfeats, grads, workspace, arg_out=None):
    """The backward of sa_forward_f32 with the running statistics frozen.  xyz .. eps: the forward's arguments; dout [B, S, cout_last];
    dfeats [B, N, D] written, or None when it is not wanted (always None when feats is None); grads: per layer the four contiguous float32
    GPU tensors (dW [cout, cin], dbias [cout], dgamma [cout], dbeta [cout]), written; workspace: sa_backward_workspace_bytes(...) GPU
    bytes; arg_out: int32 [B, S, cout_last] or None, the row of each group that the max selected."""
    L = len(layers)
    for name, t, dt in (("xyz", xyz, torch.float32), ("centres", centres, torch.int32), ("group_idx", group_idx, torch.int32),
                        ("feats", feats, torch.float32), ("dout", dout, torch.float32), ("dfeats", dfeats, torch.float32),
                        ("arg_out", arg_out, torch.int32)):
        if t is None and name in ("xyz", "centres", "group_idx", "dout"):
            raise AmpnetError(f"sa_backward: {name} is None, it must be a {dt} GPU tensor")
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt):
            raise AmpnetError(f"sa_backward: {name} must be a {dt} GPU tensor")
    if xyz.dim() != 3 or xyz.shape[2] < 3:
        raise AmpnetError(f"sa_backward: xyz must be [B, N, ld >= 3], got {tuple(xyz.shape)}")
    B, N, ld = xyz.shape
    if centres.dim() != 2 or centres.shape[0] != B or group_idx.dim() != 3 or tuple(group_idx.shape[:2]) != tuple(centres.shape) \
            or (feats is not None and (feats.dim() != 3 or tuple(feats.shape[:2]) != (B, N))):
        raise AmpnetError(f"sa_backward: centres [B, S], group_idx [B, S, nsample], feats [B, N, D] do not agree with xyz {tuple(xyz.shape)}")
    S, nsample = centres.shape[1], group_idx.shape[2]
    D = 0 if feats is None else feats.shape[2]
    if feats is None and dfeats is not None:
        raise AmpnetError(f"sa_backward: dfeats must be None when feats is (D = 0), got {tuple(dfeats.shape)}")
    if dfeats is not None and tuple(dfeats.shape) != tuple(feats.shape):
        raise AmpnetError(f"sa_backward: dfeats {tuple(dfeats.shape)} must have the shape of feats {tuple(feats.shape)}")
    table, couts, epss = _mlp_tables("sa_backward", layers, 3 + D, eps, workspace, 0)
    want = (B, S, int(layers[-1][0].shape[0])) if L else None
    if L and tuple(dout.shape) != want:
        raise AmpnetError(f"sa_backward: dout {tuple(dout.shape)} must be [B, S, cout_last] = {list(want)}")
    if L and arg_out is not None and tuple(arg_out.shape) != want:
        raise AmpnetError(f"sa_backward: arg_out {tuple(arg_out.shape)} must be [B, S, cout_last] = {list(want)}")
    if len(grads) != L:
        raise AmpnetError(f"sa_backward: grads has {len(grads)} entries for {L} layers")
    for i, (layer, g) in enumerate(zip(layers, grads)):
        wantg = [tuple(layer[0].shape)] + [tuple(layer[1].shape)] * 3
        if len(g) != 4 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t, w in zip(g, wantg)):
            raise AmpnetError(f"sa_backward: the gradients of layer {i} must be four contiguous float32 GPU tensors of shapes {wantg}, "
                              f"got {[tuple(t.shape) for t in g]}")
    need = sa_backward_workspace_bytes(D, B, S, nsample, [int(layer[0].shape[0]) for layer in layers])
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise AmpnetError(f"sa_backward: the workspace holds {have} bytes, the shape needs {need} GPU bytes")
    gtensors = [t for g in grads for t in g]
    gtable = (ctypes.c_void_p * max(len(gtensors), 1))(*[t.data_ptr() for t in gtensors])
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_backward_f32(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss, L,
                                          ptr(dout), ptr(dfeats), gtable, ptr(arg_out), ptr(workspace), ctypes.c_size_t(have),
                                          stream_ptr(xyz.device))
    check(rc, "ampnet_sa_backward_f32")


# ---- set abstraction over one group of all points (include/ampnet_hip.h: ampnet_sa_all_forward_f32, ampnet_sa_all_backward_f32) -------
def _sa_all_workspace_bytes(which, D, B, N, couts):
    couts = [int(c) for c in couts]
    name = f"ampnet_sa_all_{which}_workspace_bytes"
    fn = getattr(lib(), name)
    fn.restype = ctypes.c_size_t
    need = fn(int(D), int(B), int(N), (ctypes.c_int * max(len(couts), 1))(*couts), len(couts))
    if not need:
        check(-1, name)
    return int(need)


def sa_all_forward_workspace_bytes(D, B, N, couts):
    """Device bytes sa_all_forward_f32 needs for B clouds of N points with D features and layers of widths `couts`; a shape outside the
    kernel's limits is an AmpnetError that names the limit."""
    return _sa_all_workspace_bytes("forward", D, B, N, couts)


def sa_all_backward_workspace_bytes(D, B, N, couts):
    """Device bytes sa_all_backward_f32 needs (as sa_all_forward_workspace_bytes)."""
    return _sa_all_workspace_bytes("backward", D, B, N, couts)


def _sa_all_shapes(prefix, xyz, feats, extra):
    """The checks sa_all_forward_f32 and sa_all_backward_f32 share -> (B, N, ld, D).  extra: (name, tensor, dtype, required) of the rest."""
    for name, t, dt, required in (("xyz", xyz, torch.float32, True), ("feats", feats, torch.float32, False)) + tuple(extra):
        if t is None and required:
            raise AmpnetError(f"{prefix}: {name} is None, it must be a {dt} GPU tensor")
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt):
            raise AmpnetError(f"{prefix}: {name} must be a {dt} GPU tensor")
    if xyz.dim() != 3 or xyz.shape[2] < 3:
        raise AmpnetError(f"{prefix}: xyz must be [B, N, ld >= 3], got {tuple(xyz.shape)}")
    B, N, ld = xyz.shape
    if feats is not None and (feats.dim() != 3 or tuple(feats.shape[:2]) != (B, N)):
        raise AmpnetError(f"{prefix}: feats {tuple(feats.shape)} must be [B, N, D] with xyz {tuple(xyz.shape)}")
    return B, N, ld, 0 if feats is None else feats.shape[2]


def sa_all_forward_f32(xyz, feats, layers, eps, out, workspace, arg_out=None):
    """One fused set-abstraction layer over ONE group of all N points per cloud (group_all=True).  xyz [B, N, ld], feats [B, N, D] or None,
    layers / eps as in sa_forward_f32 with cin_0 = 3 + D; out [B, cout_last]; arg_out: int32 [B, cout_last] or None, the lowest row that
    attains each maximum; workspace: sa_all_forward_workspace_bytes(...) GPU bytes."""
    L = len(layers)
    B, N, ld, D = _sa_all_shapes("sa_all_forward", xyz, feats, (("out", out, torch.float32, True), ("arg_out", arg_out, torch.int32, False)))
    table, couts, epss = _mlp_tables("sa_all_forward", layers, 3 + D, eps, workspace, 0)
    want = (B, int(layers[-1][0].shape[0])) if L else None
    if L and tuple(out.shape) != want:
        raise AmpnetError(f"sa_all_forward: out {tuple(out.shape)} must be [B, cout_last] = {list(want)}")
    if L and arg_out is not None and tuple(arg_out.shape) != want:
        raise AmpnetError(f"sa_all_forward: arg_out {tuple(arg_out.shape)} must be [B, cout_last] = {list(want)}")
    need = sa_all_forward_workspace_bytes(D, B, N, [int(layer[0].shape[0]) for layer in layers])
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise AmpnetError(f"sa_all_forward: the workspace holds {have} bytes, the shape needs {need} GPU bytes")
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_all_forward_f32(ptr(xyz), B, N, ld, ptr(feats), D, table, couts, epss, L, ptr(out), ptr(arg_out), ptr(workspace),
                                             ctypes.c_size_t(have), stream_ptr(xyz.device))
    check(rc, "ampnet_sa_all_forward_f32")


def sa_all_backward_f32(xyz, feats, layers, eps, arg, dout, dfeats, grads, workspace):
    """The backward of sa_all_forward_f32 with the running statistics frozen.  xyz .. eps: the forward's arguments; arg: int32
    [B, cout_last], the forward's arg_out (an input); dout [B, cout_last]; dfeats [B, N, D] written (zeros outside the rows in arg), or None
    when it is not wanted (always None when feats is None); grads as in sa_backward_f32; workspace: sa_all_backward_workspace_bytes(...)
    GPU bytes."""
    L = len(layers)
    B, N, ld, D = _sa_all_shapes("sa_all_backward", xyz, feats, (("arg", arg, torch.int32, True), ("dout", dout, torch.float32, True),
                                                                 ("dfeats", dfeats, torch.float32, False)))
    if feats is None and dfeats is not None:
        raise AmpnetError(f"sa_all_backward: dfeats must be None when feats is (D = 0), got {tuple(dfeats.shape)}")
    if dfeats is not None and tuple(dfeats.shape) != tuple(feats.shape):
        raise AmpnetError(f"sa_all_backward: dfeats {tuple(dfeats.shape)} must have the shape of feats {tuple(feats.shape)}")
    table, couts, epss = _mlp_tables("sa_all_backward", layers, 3 + D, eps, workspace, 0)
    want = (B, int(layers[-1][0].shape[0])) if L else None
    if L and tuple(dout.shape) != want:
        raise AmpnetError(f"sa_all_backward: dout {tuple(dout.shape)} must be [B, cout_last] = {list(want)}")
    if L and tuple(arg.shape) != want:
        raise AmpnetError(f"sa_all_backward: arg {tuple(arg.shape)} must be [B, cout_last] = {list(want)}")
    if len(grads) != L:
        raise AmpnetError(f"sa_all_backward: grads has {len(grads)} entries for {L} layers")
    for i, (layer, g) in enumerate(zip(layers, grads)):
        wantg = [tuple(layer[0].shape)] + [tuple(layer[1].shape)] * 3
        if len(g) != 4 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t, w in zip(g, wantg)):
            raise AmpnetError(f"sa_all_backward: the gradients of layer {i} must be four contiguous float32 GPU tensors of shapes {wantg}, "
                              f"got {[tuple(t.shape) for t in g]}")
    need = sa_all_backward_workspace_bytes(D, B, N, [int(layer[0].shape[0]) for layer in layers])
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise AmpnetError(f"sa_all_backward: the workspace holds {have} bytes, the shape needs {need} GPU bytes")
    gtensors = [t for g in grads for t in g]
    gtable = (ctypes.c_void_p * max(len(gtensors), 1))(*[t.data_ptr() for t in gtensors])
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_all_backward_f32(ptr(xyz), B, N, ld, ptr(feats), D, table, couts, epss, L, ptr(arg), ptr(dout), ptr(dfeats), gtable,
                                              ptr(workspace), ctypes.c_size_t(have), stream_ptr(xyz.device))
    check(rc, "ampnet_sa_all_backward_f32")


# ---- train-mode set abstraction (include/ampnet_hip.h: ampnet_sa_train_forward_f32, ampnet_sa_train_backward_f32) --------------------
SA_TRAIN_MAX_ROWS = 1 << 24


def _sa_train_workspace_bytes(which, D, B, S, nsample, couts):
    couts = [int(c) for c in couts]
    name = f"ampnet_sa_train_{which}_workspace_bytes"
    fn = getattr(lib(), name)
    fn.restype = ctypes.c_size_t
    need = fn(int(D), int(B), int(S), int(nsample), (ctypes.c_int * max(len(couts), 1))(*couts), len(couts))
    if not need:
        check(-1, name)
    return int(need)


def sa_train_forward_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_train_forward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _sa_train_workspace_bytes("forward", D, B, S, nsample, couts)


def sa_train_backward_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_train_backward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _sa_train_workspace_bytes("backward", D, B, S, nsample, couts)


def sa_train_backward_tape(D, B, S, nsample, couts, l):
    """Test hook (ampnet_sa_train_backward_tape): where layer l's input rows x_l and its dz_l lie in the workspace that
    sa_train_backward_f32 has run on -> (x byte offset, x row stride in floats, dz byte offset, dz row stride in floats)."""
    couts = [int(c) for c in couts]
    xo, dzo = ctypes.c_size_t(0), ctypes.c_size_t(0)
    xs, dzs = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().ampnet_sa_train_backward_tape(int(D), int(B), int(S), int(nsample), (ctypes.c_int * max(len(couts), 1))(*couts), len(couts), int(l),
                                             ctypes.byref(xo), ctypes.byref(xs), ctypes.byref(dzo), ctypes.byref(dzs))
    check(rc, "ampnet_sa_train_backward_tape")
    return int(xo.value), int(xs.value), int(dzo.value), int(dzs.value)


def _sa_train_shapes(prefix, xyz, centres, group_idx, feats, extra):
    for name, t, dt in (("xyz", xyz, torch.float32), ("centres", centres, torch.int32), ("group_idx", group_idx, torch.int32),
                        ("feats", feats, torch.float32)) + tuple(extra):
        if t is None and name in ("xyz", "centres", "group_idx", "out", "dout"):
            raise AmpnetError(f"{prefix}: {name} is None, it must be a {dt} GPU tensor")
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
            raise AmpnetError(f"{prefix}: {name} must be a contiguous {dt} GPU tensor")
    if xyz.dim() != 3 or xyz.shape[2] < 3:
        raise AmpnetError(f"{prefix}: xyz must be [B, N, ld >= 3], got {tuple(xyz.shape)}")
    B, N, ld = xyz.shape
    if centres.dim() != 2 or centres.shape[0] != B or group_idx.dim() != 3 or tuple(group_idx.shape[:2]) != tuple(centres.shape) \
            or (feats is not None and (feats.dim() != 3 or tuple(feats.shape[:2]) != (B, N))):
        raise AmpnetError(f"{prefix}: centres [B, S], group_idx [B, S, nsample], feats [B, N, D] do not agree with xyz {tuple(xyz.shape)}")
    return B, N, ld, centres.shape[1], group_idx.shape[2], 0 if feats is None else feats.shape[2]


def sa_train_forward_f32(xyz, centres, group_idx, feats, layers, eps, momentum, out, save_mean, save_invstd, workspace):
    """One fused set-abstraction layer with batch-statistics BatchNorm over all B * S * nsample rows.  The arguments of sa_forward_f32;
    running_mean and running_var (entries 4 and 5 of every layer) are UPDATED IN PLACE with `momentum` (a float in [0, 1]); save_mean /
    save_invstd [sum of couts]: written, layer l at the offset of the layers before it; workspace: sa_train_forward_workspace_bytes(...)
    GPU bytes."""
    L = len(layers)
    B, N, ld, S, nsample, D = _sa_train_shapes("sa_train_forward", xyz, centres, group_idx, feats, (("out", out, torch.float32),))
    if L and tuple(out.shape) != (B, S, int(layers[-1][0].shape[0])):
        raise AmpnetError(f"sa_train_forward: out {tuple(out.shape)} must be [B, S, cout_last] = {[B, S, int(layers[-1][0].shape[0])]}")
    if momentum is None:
        raise AmpnetError("sa_train_forward: momentum=None (the cumulative average) is not built; give a float in [0, 1]")
    table, couts, epss = _mlp_tables("sa_train_forward", layers, 3 + D, eps, workspace, 0)
    sum_c = sum(int(layer[0].shape[0]) for layer in layers)
    _fp_saved("sa_train_forward", "save_mean", save_mean, sum_c, null_ok=True)
    _fp_saved("sa_train_forward", "save_invstd", save_invstd, sum_c, null_ok=True)
    have = workspace.numel() * workspace.element_size()
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_train_forward_f32(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss, L,
                                               ctypes.c_float(float(momentum)), ptr(out), ptr(save_mean), ptr(save_invstd), ptr(workspace),
                                               ctypes.c_size_t(have), stream_ptr(xyz.device))
    check(rc, "ampnet_sa_train_forward_f32")


def sa_train_backward_f32(xyz, centres, group_idx, feats, layers, eps, save_mean, save_invstd, dout, dfeats, grads, workspace, arg_out=None):
    """The backward of sa_train_forward_f32 through the batch statistics.  layers: per layer (weight, conv bias, BatchNorm weight, bias) --
    further entries are ignored; save_mean / save_invstd: what the forward wrote (never recomputed); dout, dfeats, grads, arg_out as in
    sa_backward_f32 (dbias is written as zeros); workspace: sa_train_backward_workspace_bytes(...) GPU bytes."""
    L = len(layers)
    B, N, ld, S, nsample, D = _sa_train_shapes("sa_train_backward", xyz, centres, group_idx, feats,
                                               (("dout", dout, torch.float32), ("dfeats", dfeats, torch.float32),
                                                ("arg_out", arg_out, torch.int32)))
    if feats is None and dfeats is not None:
        raise AmpnetError(f"sa_train_backward: dfeats must be None when feats is (D = 0), got {tuple(dfeats.shape)}")
    if dfeats is not None and tuple(dfeats.shape) != tuple(feats.shape):
        raise AmpnetError(f"sa_train_backward: dfeats {tuple(dfeats.shape)} must have the shape of feats {tuple(feats.shape)}")
    sum_c = sum(int(layer[0].shape[0]) for layer in layers)
    _fp_saved("sa_train_backward", "save_mean", save_mean, sum_c)
    _fp_saved("sa_train_backward", "save_invstd", save_invstd, sum_c)
    slotted, off = [], 0
    for layer in layers:                                        # slots 4 and 5 of the C ABI: the layer's saved statistics
        c = int(layer[0].shape[0])
        slotted.append(tuple(layer[:4]) + (save_mean[off:off + c], save_invstd[off:off + c]))
        off += c
    table, couts, epss = _mlp_tables("sa_train_backward", slotted, 3 + D, eps, workspace, 0)
    want = (B, S, int(layers[-1][0].shape[0])) if L else None
    if L and tuple(dout.shape) != want:
        raise AmpnetError(f"sa_train_backward: dout {tuple(dout.shape)} must be [B, S, cout_last] = {list(want)}")
    if L and arg_out is not None and tuple(arg_out.shape) != want:
        raise AmpnetError(f"sa_train_backward: arg_out {tuple(arg_out.shape)} must be [B, S, cout_last] = {list(want)}")
    if len(grads) != L:
        raise AmpnetError(f"sa_train_backward: grads has {len(grads)} entries for {L} layers")
    for i, (layer, g) in enumerate(zip(layers, grads)):
        wantg = [tuple(layer[0].shape)] + [tuple(layer[1].shape)] * 3
        if len(g) != 4 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t, w in zip(g, wantg)):
            raise AmpnetError(f"sa_train_backward: the gradients of layer {i} must be four contiguous float32 GPU tensors of shapes {wantg}, "
                              f"got {[tuple(t.shape) for t in g]}")
    gtensors = [t for g in grads for t in g]
    gtable = (ctypes.c_void_p * max(len(gtensors), 1))(*[t.data_ptr() for t in gtensors])
    have = workspace.numel() * workspace.element_size()
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_train_backward_f32(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss,
                                                L, ptr(dout), ptr(dfeats), gtable, ptr(arg_out), ptr(workspace), ctypes.c_size_t(have),
                                                stream_ptr(xyz.device))
    check(rc, "ampnet_sa_train_backward_f32")
