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
ABI_VERSION = 18

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


# ---- PointNet++ (include/ampnet_hip.h: ampnet_ball_query_f32, ampnet_three_nn_f32 and the ampnet_sa_*, ampnet_fp_* entry points) -----
SA_MAX_NSAMPLE, SA_MAX_LAYERS, SA_MAX_CIN, SA_MAX_COUT = 64, 3, 320, 256
SA_WORKSPACE_BYTES = SA_MAX_LAYERS * 2 * SA_MAX_COUT * 4
SA_MSG_MAX_SCALES = 4
SA_TRAIN_MAX_ROWS = 1 << 24
THREE_NN_MAX_S = 12288
FP_MAX_LAYERS, FP_MAX_CIN, FP_MAX_COUT = 3, 512, 256
FP_WORKSPACE_BYTES = FP_MAX_LAYERS * 2 * FP_MAX_COUT * 4
_F32, _I32 = torch.float32, torch.int32


def ball_query_f32(xyz, centres, radius, nsample, out, count=None):
    """xyz [B, N, ld] float32, centres [B, S] int32, out [B, S, nsample] int32, count [B, S] int32 or None: contiguous GPU tensors."""
    B, N, ld = xyz.shape
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_ball_query_f32(ptr(xyz), B, N, ld, ptr(centres), centres.shape[1], ctypes.c_float(radius), int(nsample), ptr(out),
                                         ptr(count), stream_ptr(xyz.device))
    check(rc, "ampnet_ball_query_f32")


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


BALL_QUERY_MAX_N = 12288


def ball_query_ragged_f32(rows, cloud_off, max_n, centres, radius, nsample, global_index, out, count=None):
    """rows [total, ld] float32, cloud_off [Q + 1] int32 (device), centres [Q, S] int32 relative to their cloud, out [Q, S, nsample] int32,
    count [Q, S] int32 or None: contiguous GPU tensors; max_n the largest cloud (host int)."""
    total, ld = rows.shape
    Q, S = centres.shape
    with torch.cuda.device(rows.device):
        rc = lib().ampnet_ball_query_ragged_f32(ptr(rows), ld, ptr(cloud_off), Q, total, int(max_n), ptr(centres), S, ctypes.c_float(radius),
                                                int(nsample), int(bool(global_index)), ptr(out), ptr(count), stream_ptr(rows.device))
    check(rc, "ampnet_ball_query_ragged_f32")


def three_nn_ragged_f32(fine, cloud_off, max_n, coarse, global_index, idx, dist2):
    """fine [total, ld1] float32, cloud_off [Q + 1] int32 (device), coarse [Q, S, ld2] float32, idx int32 / dist2 float32 [total, k],
    k = min(3, S): contiguous GPU tensors; max_n the largest fine cloud (host int)."""
    total, ld1 = fine.shape
    Q, S, ld2 = coarse.shape
    k = min(3, S)
    for name, t, dt in (("fine", fine, _F32), ("cloud_off", cloud_off, _I32), ("coarse", coarse, _F32), ("idx", idx, _I32), ("dist2", dist2, _F32)):
        if not t.is_cuda or t.dtype != dt:
            raise AmpnetError(f"three_nn_ragged: {name} must be a {dt} GPU tensor")
    if cloud_off.numel() != Q + 1 or tuple(idx.shape) != (total, k) or tuple(dist2.shape) != (total, k):
        raise AmpnetError(f"three_nn_ragged: cloud_off [Q + 1], idx and dist2 [total, min(3, S)] do not agree with fine {tuple(fine.shape)} "
                          f"and coarse {tuple(coarse.shape)}")
    with torch.cuda.device(fine.device):
        rc = lib().ampnet_three_nn_ragged_f32(ptr(fine), ld1, ptr(cloud_off), Q, total, int(max_n), ptr(coarse), S, ld2,
                                              int(bool(global_index)), ptr(idx), ptr(dist2), stream_ptr(fine.device))
    check(rc, "ampnet_three_nn_ragged_f32")


# The rules the fused set-abstraction (sa_*) and feature-propagation (fp_*) wrappers share, each written once.  The kernels take bare
# pointers and no strides: what a wrapper lets through is read wrongly without any error.  `prefix` is the wrapper's name, the start of
# every message.
def _workspace_bytes(symbol, ints, couts):
    """Device bytes the entry point sized by the C symbol `symbol` needs for the shape `ints` and layers of widths `couts`; a shape
    outside the kernel's limits is an AmpnetError that names the limit."""
    couts = [int(c) for c in couts]
    fn = getattr(lib(), symbol)
    fn.restype = ctypes.c_size_t
    need = fn(*[int(v) for v in ints], (ctypes.c_int * max(len(couts), 1))(*couts), len(couts))
    if not need:
        check(-1, symbol)
    return int(need)


def _check_tensors(prefix, rows):
    """rows: (name, tensor, dtype, ndim, required).  A missing required tensor is named first; every tensor that is given must be a
    contiguous GPU tensor of that dtype and rank."""
    for name, t, dt, nd, required in rows:
        if t is None and required:
            raise AmpnetError(f"{prefix}: {name} is None, it must be a contiguous {nd}-d {dt} GPU tensor")
    for name, t, dt, nd, _ in rows:
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or t.dim() != nd or not t.is_contiguous()):
            got = f"{tuple(t.shape)} {t.dtype} on {t.device}, strides {t.stride()}" if torch.is_tensor(t) else type(t).__name__
            raise AmpnetError(f"{prefix}: {name} must be a contiguous {nd}-d {dt} GPU tensor, got {got}")


def _sa_geometry(prefix, xyz, centres, group_idx, feats, extra):
    """xyz [B, N, ld >= 3], centres [B, S], group_idx [B, S, nsample], feats [B, N, D] or None -> (B, N, ld, S, nsample, D).  extra: the
    _check_tensors rows of the wrapper's other tensors."""
    _check_tensors(prefix, [("xyz", xyz, _F32, 3, True), ("centres", centres, _I32, 2, True), ("group_idx", group_idx, _I32, 3, True),
                            ("feats", feats, _F32, 3, False)] + extra)
    B, N, ld = xyz.shape
    if ld < 3:
        raise AmpnetError(f"{prefix}: xyz must be [B, N, ld >= 3], got {tuple(xyz.shape)}")
    if centres.shape[0] != B or tuple(group_idx.shape[:2]) != tuple(centres.shape) or (feats is not None and tuple(feats.shape[:2]) != (B, N)):
        raise AmpnetError(f"{prefix}: centres [B, S], group_idx [B, S, nsample], feats [B, N, D] do not agree with xyz {tuple(xyz.shape)}")
    return B, N, ld, centres.shape[1], group_idx.shape[2], 0 if feats is None else feats.shape[2]


def _sa_all_geometry(prefix, xyz, feats, extra):
    """xyz [B, N, ld >= 3], feats [B, N, D] or None -> (B, N, ld, D).  extra as in _sa_geometry."""
    _check_tensors(prefix, [("xyz", xyz, _F32, 3, True), ("feats", feats, _F32, 3, False)] + extra)
    B, N, ld = xyz.shape
    if ld < 3:
        raise AmpnetError(f"{prefix}: xyz must be [B, N, ld >= 3], got {tuple(xyz.shape)}")
    if feats is not None and tuple(feats.shape[:2]) != (B, N):
        raise AmpnetError(f"{prefix}: feats {tuple(feats.shape)} must be [B, N, D] with xyz {tuple(xyz.shape)}")
    return B, N, ld, 0 if feats is None else feats.shape[2]


def _fp_geometry(prefix, points1, points2, idx, dist2, extra):
    """points1 [B, N, D1] or None, points2 [B, S, D2], idx and dist2 [B, N, k] -> (B, N, k, S, D1, D2).  extra as in _sa_geometry."""
    _check_tensors(prefix, [("points1", points1, _F32, 3, False), ("points2", points2, _F32, 3, True), ("idx", idx, _I32, 3, True),
                            ("dist2", dist2, _F32, 3, True)] + extra)
    B, N, k = idx.shape
    if points2.shape[0] != B or tuple(dist2.shape) != (B, N, k) or (points1 is not None and tuple(points1.shape[:2]) != (B, N)):
        raise AmpnetError(f"{prefix}: points1 [B, N, D1], points2 [B, S, D2], dist2 [B, N, k] do not agree with idx {tuple(idx.shape)}")
    return B, N, k, points2.shape[1], 0 if points1 is None else points1.shape[2], points2.shape[2]


def _mlp_tables(prefix, layers, cin, eps):
    """Every layer is six contiguous float32 GPU tensors of shapes [(cout, cin)] + [(cout,)] * 5 chained from cin (the kernels trust these
    shapes: a short tensor would be read past its end) and eps has one entry per layer -> the (pointer table, couts, epss) ctypes arrays
    of the C ABI."""
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
    tensors = [t for layer in layers for t in layer]
    return ((ctypes.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors]),
            (ctypes.c_int * max(L, 1))(*[int(layer[0].shape[0]) for layer in layers]),
            (ctypes.c_float * max(L, 1))(*[float(e) for e in eps]))


def _check_cout_last(prefix, layers, lead, label, **tensors):
    """Each tensor that is given must be `lead` + (cout_last,); `label` is how the message writes `lead`."""
    if layers:
        want = tuple(lead) + (int(layers[-1][0].shape[0]),)
        for name, t in tensors.items():
            if t is not None and tuple(t.shape) != want:
                raise AmpnetError(f"{prefix}: {name} {tuple(t.shape)} must be [{label}, cout_last] = {list(want)}")


def _check_grad_of(prefix, dname, d, name, t, optional=False):
    """d, the gradient written for the input t: None exactly when t is (optional: also wherever it is not wanted), else of t's shape."""
    if d is None and (t is None or optional):
        return
    if d is None or t is None:
        raise AmpnetError(f"{prefix}: {dname} must be None {'when' if optional else 'exactly when'} {name} is, got "
                          f"{None if d is None else tuple(d.shape)}")
    if tuple(d.shape) != tuple(t.shape):
        raise AmpnetError(f"{prefix}: {dname} {tuple(d.shape)} must have the shape of {name} {tuple(t.shape)}")


def _grad_table(prefix, layers, grads):
    """grads: per layer (dW, dbias, dgamma, dbeta) of the shapes of the layer's weight and bias -> the pointer table of the C ABI."""
    if len(grads) != len(layers):
        raise AmpnetError(f"{prefix}: grads has {len(grads)} entries for {len(layers)} layers")
    for i, (layer, g) in enumerate(zip(layers, grads)):
        want = [tuple(layer[0].shape)] + [tuple(layer[1].shape)] * 3
        if len(g) != 4 or any(tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t, w in zip(g, want)):
            raise AmpnetError(f"{prefix}: the gradients of layer {i} must be four contiguous float32 GPU tensors of shapes {want}, "
                              f"got {[tuple(t.shape) for t in g]}")
    tensors = [t for g in grads for t in g]
    return (ctypes.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


def _saved_rows(save_mean, save_invstd):
    return [("save_mean", save_mean, _F32, 1, True), ("save_invstd", save_invstd, _F32, 1, True)]


def _check_saved(prefix, layers, save_mean, save_invstd):
    """The batch statistics of a train entry point: sum(cout) elements each, layer l at the offset of the layers before it."""
    sum_c = sum(int(layer[0].shape[0]) for layer in layers)
    for name, t in (("save_mean", save_mean), ("save_invstd", save_invstd)):
        if t.numel() != sum_c:
            raise AmpnetError(f"{prefix}: {name} must hold sum(cout) = {sum_c} elements, got {tuple(t.shape)}")


def _saved_slots(prefix, layers, save_mean, save_invstd):
    """The layers a train backward hands to _mlp_tables: (weight, conv bias, BatchNorm weight, bias) of each layer -- further entries are
    ignored -- and, in slots 4 and 5 of the C ABI, the layer's saved statistics."""
    _check_saved(prefix, layers, save_mean, save_invstd)
    slotted, off = [], 0
    for layer in layers:
        c = int(layer[0].shape[0])
        slotted.append(tuple(layer[:4]) + (save_mean[off:off + c], save_invstd[off:off + c]))
        off += c
    return slotted


def _momentum(prefix, momentum):
    if momentum is None:
        raise AmpnetError(f"{prefix}: momentum=None (the cumulative average) is not built; give a float in [0, 1]")
    return ctypes.c_float(float(momentum))


def _workspace_args(prefix, workspace):
    """(pointer, size in bytes) of the workspace.  Its size is checked against the shape by every ampnet_*_f32 entry point itself -- the
    copy of that rule that cannot go stale -- so only what the C ABI cannot see is checked here."""
    if not torch.is_tensor(workspace) or not workspace.is_cuda or not workspace.is_contiguous():
        raise AmpnetError(f"{prefix}: the workspace must be a contiguous GPU tensor")
    return ptr(workspace), ctypes.c_size_t(workspace.numel() * workspace.element_size())


def _ragged_clouds(prefix, cloud_off, B, S, label):
    """The ragged form of a backward (cloud_off given): the tensors hold the packed array as ONE cloud (B = 1) and cloud_off, int32
    [Q + 1] on the device, says where its Q clouds lie; the S `label` of the call are Q equal shares -> (Q, S // Q)."""
    _check_tensors(prefix, [("cloud_off", cloud_off, _I32, 1, True)])
    Q = cloud_off.numel() - 1
    if B != 1 or Q < 1 or S % Q:
        raise AmpnetError(f"{prefix}: with cloud_off the tensors hold the packed clouds as one (leading dimension 1, got {B}) and the "
                          f"{S} {label} are the equal shares of the {Q} clouds of cloud_off {tuple(cloud_off.shape)}")
    return Q, S // Q


def fp_backward_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_backward_f32 needs for points1 [B, N, D1], points2 [B, S, D2] and layers of widths `couts` (include/ampnet_hip.h:
    ampnet_fp_backward_workspace_bytes); a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_fp_backward_workspace_bytes", (D1, D2, B, N), couts)


def fp_train_forward_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_train_forward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_fp_train_forward_workspace_bytes", (D1, D2, B, N), couts)


def fp_train_backward_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_train_backward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_fp_train_backward_workspace_bytes", (D1, D2, B, N), couts)


def sa_backward_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_backward_f32 needs for feats [B, N, D], S centres per cloud, groups of nsample and layers of widths `couts`
    (include/ampnet_hip.h: ampnet_sa_backward_workspace_bytes); a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_sa_backward_workspace_bytes", (D, B, S, nsample), couts)


def sa_train_forward_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_train_forward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_sa_train_forward_workspace_bytes", (D, B, S, nsample), couts)


def sa_train_backward_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_train_backward_f32 needs; a shape outside the kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_sa_train_backward_workspace_bytes", (D, B, S, nsample), couts)


def sa_all_forward_workspace_bytes(D, B, N, couts):
    """Device bytes sa_all_forward_f32 needs for B clouds of N points with D features and layers of widths `couts`; a shape outside the
    kernel's limits is an AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_sa_all_forward_workspace_bytes", (D, B, N), couts)


def sa_all_backward_workspace_bytes(D, B, N, couts):
    """Device bytes sa_all_backward_f32 needs (as sa_all_forward_workspace_bytes)."""
    return _workspace_bytes("ampnet_sa_all_backward_workspace_bytes", (D, B, N), couts)


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


# ---- set abstraction: eval forward and frozen-statistics backward ------------------------------------------------------------------------
def _sa_forward(prefix, symbol, xyz, centres, group_idx, feats, layers, eps, out, workspace):
    """The eval forward under its two arithmetics: one argument list, one set of checks (`prefix` opens their messages)."""
    B, N, ld, S, nsample, D = _sa_geometry(prefix, xyz, centres, group_idx, feats, [("out", out, _F32, 3, True)])
    table, couts, epss = _mlp_tables(prefix, layers, 3 + D, eps)
    _check_cout_last(prefix, layers, (B, S), "B, S", out=out)
    ws, ws_bytes = _workspace_args(prefix, workspace)
    with torch.cuda.device(xyz.device):
        rc = getattr(lib(), symbol)(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss,
                                    len(layers), ptr(out), ws, ws_bytes, stream_ptr(xyz.device))
    check(rc, symbol)


def sa_forward_f32(xyz, centres, group_idx, feats, layers, eps, out, workspace):
    """One fused set-abstraction layer.  layers: per layer the six contiguous float32 GPU tensors (weight [cout, cin], conv bias, BatchNorm
    weight, bias, running_mean, running_var); eps: per layer the BatchNorm eps; feats [B, N, D] or None; out [B, S, cout_last]; workspace:
    SA_WORKSPACE_BYTES GPU bytes."""
    _sa_forward("sa_forward", "ampnet_sa_forward_f32", xyz, centres, group_idx, feats, layers, eps, out, workspace)


def sa_forward_bf16_workspace_bytes(D, B, S, nsample, couts):
    """Device bytes sa_forward_bf16 needs (the BatchNorm fold and every layer's weights as bf16); a shape outside the kernel's limits is an
    AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_sa_forward_bf16_workspace_bytes", (D, B, S, nsample), couts)


def sa_forward_bf16(xyz, centres, group_idx, feats, layers, eps, out, workspace):
    """sa_forward_f32 with the matrix products in bf16 (include/ampnet_hip.h, "the rounding model"): the same float32 arguments and
    output; workspace: sa_forward_bf16_workspace_bytes(D, B, S, nsample, couts) GPU bytes, 16-byte aligned."""
    _sa_forward("sa_forward_bf16", "ampnet_sa_forward_bf16", xyz, centres, group_idx, feats, layers, eps, out, workspace)


# ---- multi-scale grouping: K radii, K branches around the same centres ------------------------------------------------------------------
def ball_query_msg_f32(xyz, centres, radii, nsamples, outs, counts=None):
    """ball_query_f32 at K radii in one launch.  xyz [B, N, ld] float32, centres [B, S] int32; radii, nsamples: K host numbers each;
    outs: K int32 tensors, outs[k] [B, S, nsamples[k]]; counts: None, or K entries each an int32 [B, S] tensor or None."""
    K = len(outs)
    if len(radii) != K or len(nsamples) != K or (counts is not None and len(counts) != K):
        raise AmpnetError(f"ball_query_msg: radii, nsamples, outs and counts must have one entry per scale, got {len(radii)}, "
                          f"{len(nsamples)}, {K}, {None if counts is None else len(counts)}")
    rows = [("xyz", xyz, _F32, 3, True), ("centres", centres, _I32, 2, True)]
    rows += [(f"outs[{k}]", t, _I32, 3, True) for k, t in enumerate(outs)]
    rows += [(f"counts[{k}]", t, _I32, 2, False) for k, t in enumerate(counts or ())]
    _check_tensors("ball_query_msg", rows)
    B, N, ld = xyz.shape
    S = centres.shape[1]
    if centres.shape[0] != B or any(tuple(t.shape) != (B, S, int(ns)) for t, ns in zip(outs, nsamples)) \
            or any(t is not None and tuple(t.shape) != (B, S) for t in counts or ()):
        raise AmpnetError(f"ball_query_msg: centres [B, S], outs[k] [B, S, nsamples[k]], counts[k] [B, S] do not agree with xyz "
                          f"{tuple(xyz.shape)}, nsamples {list(nsamples)}")
    n = max(K, 1)
    out_table = (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs])
    count_table = None if counts is None else (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in counts])
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_ball_query_msg_f32(ptr(xyz), B, N, ld, ptr(centres), S, (ctypes.c_float * n)(*[float(r) for r in radii]),
                                             (ctypes.c_int * n)(*[int(ns) for ns in nsamples]), K, out_table, count_table,
                                             stream_ptr(xyz.device))
    check(rc, "ampnet_ball_query_msg_f32")


def sa_msg_forward_workspace_bytes(K):
    """Device bytes sa_msg_forward_f32 needs for K branches: K * SA_WORKSPACE_BYTES, answered on the host; K outside
    [1, SA_MSG_MAX_SCALES] is an AmpnetError."""
    fn = lib().ampnet_sa_msg_forward_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = fn(int(K))
    if not need:
        check(-1, "ampnet_sa_msg_forward_workspace_bytes")
    return int(need)


def sa_msg_forward_f32(xyz, centres, group_idxs, feats, branches, eps, out, workspace):
    """K fused set-abstraction branches around the same centres in one launch.  group_idxs: K int32 tensors [B, S, nsample_k]; branches:
    per branch the `layers` of sa_forward_f32 (cin_0 = 3 + D in every branch); eps: per branch the per-layer BatchNorm eps; out
    [B, S, sum of the branches' cout_last], branch k in its column slice; workspace: sa_msg_forward_workspace_bytes(K) GPU bytes."""
    K = len(branches)
    if len(group_idxs) != K or len(eps) != K:
        raise AmpnetError(f"sa_msg_forward: group_idxs, branches and eps must have one entry per branch, got {len(group_idxs)}, {K}, {len(eps)}")
    _check_tensors("sa_msg_forward", [("xyz", xyz, _F32, 3, True), ("centres", centres, _I32, 2, True), ("out", out, _F32, 3, True)])
    (B, N, ld), S, D = xyz.shape, centres.shape[1], 0 if feats is None else feats.shape[-1]
    params, couts, epss, C = [], [], [], 0
    for k, layers in enumerate(branches):
        prefix = f"sa_msg_forward: branch {k}"
        _, _, _, _, _, D = _sa_geometry(prefix, xyz, centres, group_idxs[k], feats, [])
        table, cout, e = _mlp_tables(prefix, layers, 3 + D, eps[k])
        params += table[:6 * len(layers)]
        couts += cout[:len(layers)]
        epss += e[:len(layers)]
        C += couts[-1] if layers else 0
    if K and tuple(out.shape) != (B, S, C):
        raise AmpnetError(f"sa_msg_forward: out {tuple(out.shape)} must be [B, S, sum of the branches' cout_last] = {[B, S, C]}")
    ws, ws_bytes = _workspace_args("sa_msg_forward", workspace)
    n = max(K, 1)
    cat = lambda ctype, values: (ctype * max(len(values), 1))(*values)
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_msg_forward_f32(ptr(xyz), B, N, ld, ptr(centres), S, (ctypes.c_void_p * n)(*[g.data_ptr() for g in group_idxs]),
                                             (ctypes.c_int * n)(*[int(g.shape[2]) for g in group_idxs]), ptr(feats), D,
                                             cat(ctypes.c_void_p, params), cat(ctypes.c_int, couts), cat(ctypes.c_float, epss),
                                             (ctypes.c_int * n)(*[len(b) for b in branches]), K, ptr(out), ws, ws_bytes, stream_ptr(xyz.device))
    check(rc, "ampnet_sa_msg_forward_f32")


def sa_backward_f32(xyz, centres, group_idx, feats, layers, eps, dout, dfeats, grads, workspace, arg_out=None, cloud_off=None):
    """The backward of sa_forward_f32 with the running statistics frozen.  xyz .. eps: the forward's arguments; dout [B, S, cout_last];
    dfeats [B, N, D] written, or None when it is not wanted (always None when feats is None); grads: per layer (dW [cout, cin],
    dbias [cout], dgamma [cout], dbeta [cout]), written (_grad_table); workspace: sa_backward_workspace_bytes(...) GPU bytes; arg_out: int32 [B, S, cout_last] or None, the row of each group that the max selected.
    cloud_off: int32 [Q + 1] on the device, or None.  Given, the tensors are Q clouds of unequal size packed as one (B = 1, N = total,
    S = Q centres-per-cloud, global indices) and the call is ampnet_sa_backward_ragged_f32: the same phases, the dfeats gather cloud by cloud."""
    B, N, ld, S, nsample, D = _sa_geometry("sa_backward", xyz, centres, group_idx, feats,
                                           [("dout", dout, _F32, 3, True), ("dfeats", dfeats, _F32, 3, False), ("arg_out", arg_out, _I32, 3, False)])
    _check_grad_of("sa_backward", "dfeats", dfeats, "feats", feats, optional=True)
    table, couts, epss = _mlp_tables("sa_backward", layers, 3 + D, eps)
    _check_cout_last("sa_backward", layers, (B, S), "B, S", dout=dout, arg_out=arg_out)
    gtable = _grad_table("sa_backward", layers, grads)
    ws, ws_bytes = _workspace_args("sa_backward", workspace)
    if cloud_off is not None:
        Q, S1 = _ragged_clouds("sa_backward", cloud_off, B, S, "centres")
        with torch.cuda.device(xyz.device):
            rc = lib().ampnet_sa_backward_ragged_f32(ptr(xyz), ptr(cloud_off), Q, N, ld, ptr(centres), S1, ptr(group_idx), nsample, ptr(feats), D,
                                                     table, couts, epss, len(layers), ptr(dout), ptr(dfeats), gtable, ptr(arg_out), ws, ws_bytes,
                                                     stream_ptr(xyz.device))
        return check(rc, "ampnet_sa_backward_ragged_f32")
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_backward_f32(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss,
                                          len(layers), ptr(dout), ptr(dfeats), gtable, ptr(arg_out), ws, ws_bytes, stream_ptr(xyz.device))
    check(rc, "ampnet_sa_backward_f32")


# ---- set abstraction over one group of all points ---------------------------------------------------------------------------------------
def sa_all_forward_f32(xyz, feats, layers, eps, out, workspace, arg_out=None):
    """One fused set-abstraction layer over ONE group of all N points per cloud (group_all=True).  xyz [B, N, ld], feats [B, N, D] or None,
    layers / eps as in sa_forward_f32 with cin_0 = 3 + D; out [B, cout_last]; arg_out: int32 [B, cout_last] or None, the lowest row that
    attains each maximum; workspace: sa_all_forward_workspace_bytes(...) GPU bytes."""
    B, N, ld, D = _sa_all_geometry("sa_all_forward", xyz, feats, [("out", out, _F32, 2, True), ("arg_out", arg_out, _I32, 2, False)])
    table, couts, epss = _mlp_tables("sa_all_forward", layers, 3 + D, eps)
    _check_cout_last("sa_all_forward", layers, (B,), "B", out=out, arg_out=arg_out)
    ws, ws_bytes = _workspace_args("sa_all_forward", workspace)
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_all_forward_f32(ptr(xyz), B, N, ld, ptr(feats), D, table, couts, epss, len(layers), ptr(out), ptr(arg_out), ws,
                                             ws_bytes, stream_ptr(xyz.device))
    check(rc, "ampnet_sa_all_forward_f32")


def sa_all_backward_f32(xyz, feats, layers, eps, arg, dout, dfeats, grads, workspace):
    """The backward of sa_all_forward_f32 with the running statistics frozen.  xyz .. eps: the forward's arguments; arg: int32
    [B, cout_last], the forward's arg_out (an input); dout [B, cout_last]; dfeats [B, N, D] written (zeros outside the rows in arg), or None
    when it is not wanted (always None when feats is None); grads as in sa_backward_f32; workspace: sa_all_backward_workspace_bytes(...)
    GPU bytes."""
    B, N, ld, D = _sa_all_geometry("sa_all_backward", xyz, feats,
                                   [("arg", arg, _I32, 2, True), ("dout", dout, _F32, 2, True), ("dfeats", dfeats, _F32, 3, False)])
    _check_grad_of("sa_all_backward", "dfeats", dfeats, "feats", feats, optional=True)
    table, couts, epss = _mlp_tables("sa_all_backward", layers, 3 + D, eps)
    _check_cout_last("sa_all_backward", layers, (B,), "B", dout=dout, arg=arg)
    gtable = _grad_table("sa_all_backward", layers, grads)
    ws, ws_bytes = _workspace_args("sa_all_backward", workspace)
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_all_backward_f32(ptr(xyz), B, N, ld, ptr(feats), D, table, couts, epss, len(layers), ptr(arg), ptr(dout),
                                              ptr(dfeats), gtable, ws, ws_bytes, stream_ptr(xyz.device))
    check(rc, "ampnet_sa_all_backward_f32")


# ---- train-mode set abstraction ----------------------------------------------------------------------------------------------------------
def sa_train_forward_f32(xyz, centres, group_idx, feats, layers, eps, momentum, out, save_mean, save_invstd, workspace):
    """One fused set-abstraction layer with batch-statistics BatchNorm over all B * S * nsample rows.  The arguments of sa_forward_f32;
    running_mean and running_var (entries 4 and 5 of every layer) are UPDATED IN PLACE with `momentum` (a float in [0, 1]); save_mean /
    save_invstd [sum of couts]: written, layer l at the offset of the layers before it; workspace: sa_train_forward_workspace_bytes(...)
    GPU bytes."""
    B, N, ld, S, nsample, D = _sa_geometry("sa_train_forward", xyz, centres, group_idx, feats,
                                           [("out", out, _F32, 3, True)] + _saved_rows(save_mean, save_invstd))
    mom = _momentum("sa_train_forward", momentum)
    table, couts, epss = _mlp_tables("sa_train_forward", layers, 3 + D, eps)
    _check_cout_last("sa_train_forward", layers, (B, S), "B, S", out=out)
    _check_saved("sa_train_forward", layers, save_mean, save_invstd)
    ws, ws_bytes = _workspace_args("sa_train_forward", workspace)
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_train_forward_f32(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss,
                                               len(layers), mom, ptr(out), ptr(save_mean), ptr(save_invstd), ws, ws_bytes,
                                               stream_ptr(xyz.device))
    check(rc, "ampnet_sa_train_forward_f32")


def sa_train_backward_f32(xyz, centres, group_idx, feats, layers, eps, save_mean, save_invstd, dout, dfeats, grads, workspace, arg_out=None,
                          cloud_off=None):
    """The backward of sa_train_forward_f32 through the batch statistics.  layers: per layer (weight, conv bias, BatchNorm weight, bias) --
    further entries are ignored; save_mean / save_invstd: what the forward wrote (never recomputed); dout, dfeats, grads, arg_out as in
    sa_backward_f32 (dbias is written as zeros); workspace: sa_train_backward_workspace_bytes(...) GPU bytes; cloud_off as in
    sa_backward_f32 (ampnet_sa_train_backward_ragged_f32)."""
    B, N, ld, S, nsample, D = _sa_geometry("sa_train_backward", xyz, centres, group_idx, feats,
                                           _saved_rows(save_mean, save_invstd) + [("dout", dout, _F32, 3, True), ("dfeats", dfeats, _F32, 3, False),
                                                                                  ("arg_out", arg_out, _I32, 3, False)])
    _check_grad_of("sa_train_backward", "dfeats", dfeats, "feats", feats, optional=True)
    table, couts, epss = _mlp_tables("sa_train_backward", _saved_slots("sa_train_backward", layers, save_mean, save_invstd), 3 + D, eps)
    _check_cout_last("sa_train_backward", layers, (B, S), "B, S", dout=dout, arg_out=arg_out)
    gtable = _grad_table("sa_train_backward", layers, grads)
    ws, ws_bytes = _workspace_args("sa_train_backward", workspace)
    if cloud_off is not None:
        Q, S1 = _ragged_clouds("sa_train_backward", cloud_off, B, S, "centres")
        with torch.cuda.device(xyz.device):
            rc = lib().ampnet_sa_train_backward_ragged_f32(ptr(xyz), ptr(cloud_off), Q, N, ld, ptr(centres), S1, ptr(group_idx), nsample, ptr(feats),
                                                           D, table, couts, epss, len(layers), ptr(dout), ptr(dfeats), gtable, ptr(arg_out), ws,
                                                           ws_bytes, stream_ptr(xyz.device))
        return check(rc, "ampnet_sa_train_backward_ragged_f32")
    with torch.cuda.device(xyz.device):
        rc = lib().ampnet_sa_train_backward_f32(ptr(xyz), B, N, ld, ptr(centres), S, ptr(group_idx), nsample, ptr(feats), D, table, couts, epss,
                                                len(layers), ptr(dout), ptr(dfeats), gtable, ptr(arg_out), ws, ws_bytes, stream_ptr(xyz.device))
    check(rc, "ampnet_sa_train_backward_f32")


# ---- feature propagation: eval forward and frozen-statistics backward --------------------------------------------------------------------
def _fp_forward(prefix, symbol, points1, points2, idx, dist2, layers, eps, out, workspace):
    """The eval forward under its two arithmetics: one argument list, one set of checks (`prefix` opens their messages)."""
    B, N, k, S, D1, D2 = _fp_geometry(prefix, points1, points2, idx, dist2, [("out", out, _F32, 3, True)])
    table, couts, epss = _mlp_tables(prefix, layers, D1 + D2, eps)
    _check_cout_last(prefix, layers, (B, N), "B, N", out=out)
    ws, ws_bytes = _workspace_args(prefix, workspace)
    with torch.cuda.device(points2.device):
        rc = getattr(lib(), symbol)(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss, len(layers),
                                    ptr(out), ws, ws_bytes, stream_ptr(points2.device))
    check(rc, symbol)


def fp_forward_f32(points1, points2, idx, dist2, layers, eps, out, workspace):
    """One fused feature-propagation layer.  points1 [B, N, D1] or None, points2 [B, S, D2], idx int32 / dist2 float32 [B, N, k] (the output
    of three_nn_f32), layers and eps as in sa_forward_f32 with cin_0 = D1 + D2, out [B, N, cout_last]; workspace: FP_WORKSPACE_BYTES GPU
    bytes."""
    _fp_forward("fp_forward", "ampnet_fp_forward_f32", points1, points2, idx, dist2, layers, eps, out, workspace)


def fp_forward_bf16_workspace_bytes(D1, D2, B, N, couts):
    """Device bytes fp_forward_bf16 needs (the BatchNorm fold and every layer's weights as bf16); a shape outside the kernel's limits is an
    AmpnetError that names the limit."""
    return _workspace_bytes("ampnet_fp_forward_bf16_workspace_bytes", (D1, D2, B, N), couts)


def fp_forward_bf16(points1, points2, idx, dist2, layers, eps, out, workspace):
    """fp_forward_f32 with the matrix products in bf16 (include/ampnet_hip.h, "the rounding model"): the same float32 arguments and
    output; workspace: fp_forward_bf16_workspace_bytes(D1, D2, B, N, couts) GPU bytes, 16-byte aligned."""
    _fp_forward("fp_forward_bf16", "ampnet_fp_forward_bf16", points1, points2, idx, dist2, layers, eps, out, workspace)


def _fp_backward_rows(dout, dpoints1, dpoints2):
    return [("dout", dout, _F32, 3, True), ("dpoints1", dpoints1, _F32, 3, False), ("dpoints2", dpoints2, _F32, 3, True)]


def fp_backward_f32(points1, points2, idx, dist2, layers, eps, dout, dpoints1, dpoints2, grads, workspace, cloud_off=None):
    """The backward of fp_forward_f32 with the running statistics frozen.  points1 .. eps: the forward's arguments; dout [B, N, cout_last];
    dpoints1 [B, N, D1] (None exactly when points1 is None) and dpoints2 [B, S, D2]: written; grads as in sa_backward_f32; workspace:
    fp_backward_workspace_bytes(...) GPU bytes.
    cloud_off: int32 [Q + 1] on the device, or None.  Given, the tensors are Q fine clouds of unequal size packed as one (B = 1, N = total,
    S = Q coarse-points-per-cloud, global indices) and the call is ampnet_fp_backward_ragged_f32: the same phases, the dpoints2 gather
    cloud by cloud."""
    B, N, k, S, D1, D2 = _fp_geometry("fp_backward", points1, points2, idx, dist2, _fp_backward_rows(dout, dpoints1, dpoints2))
    _check_grad_of("fp_backward", "dpoints1", dpoints1, "points1", points1)
    _check_grad_of("fp_backward", "dpoints2", dpoints2, "points2", points2)
    table, couts, epss = _mlp_tables("fp_backward", layers, D1 + D2, eps)
    _check_cout_last("fp_backward", layers, (B, N), "B, N", dout=dout)
    gtable = _grad_table("fp_backward", layers, grads)
    ws, ws_bytes = _workspace_args("fp_backward", workspace)
    if cloud_off is not None:
        Q, S1 = _ragged_clouds("fp_backward", cloud_off, B, S, "coarse points")
        with torch.cuda.device(points2.device):
            rc = lib().ampnet_fp_backward_ragged_f32(ptr(points1), D1, ptr(points2), D2, ptr(cloud_off), Q, N, S1, ptr(idx), ptr(dist2), k, table,
                                                     couts, epss, len(layers), ptr(dout), ptr(dpoints1), ptr(dpoints2), gtable, ws, ws_bytes,
                                                     stream_ptr(points2.device))
        return check(rc, "ampnet_fp_backward_ragged_f32")
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_backward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss, len(layers),
                                          ptr(dout), ptr(dpoints1), ptr(dpoints2), gtable, ws, ws_bytes, stream_ptr(points2.device))
    check(rc, "ampnet_fp_backward_f32")


# ---- train-mode feature propagation ------------------------------------------------------------------------------------------------------
def fp_train_forward_f32(points1, points2, idx, dist2, layers, eps, momentum, out, save_mean, save_invstd, workspace):
    """One fused feature-propagation layer with batch-statistics BatchNorm.  The arguments of fp_forward_f32; running_mean and running_var
    (entries 4 and 5 of every layer) are UPDATED IN PLACE with `momentum` (a float in [0, 1]); save_mean / save_invstd [sum of couts]:
    written, layer l at the offset of the layers before it; workspace: fp_train_forward_workspace_bytes(...) GPU bytes."""
    B, N, k, S, D1, D2 = _fp_geometry("fp_train_forward", points1, points2, idx, dist2,
                                      [("out", out, _F32, 3, True)] + _saved_rows(save_mean, save_invstd))
    mom = _momentum("fp_train_forward", momentum)
    table, couts, epss = _mlp_tables("fp_train_forward", layers, D1 + D2, eps)
    _check_cout_last("fp_train_forward", layers, (B, N), "B, N", out=out)
    _check_saved("fp_train_forward", layers, save_mean, save_invstd)
    ws, ws_bytes = _workspace_args("fp_train_forward", workspace)
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_train_forward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss,
                                               len(layers), mom, ptr(out), ptr(save_mean), ptr(save_invstd), ws, ws_bytes,
                                               stream_ptr(points2.device))
    check(rc, "ampnet_fp_train_forward_f32")


def fp_train_backward_f32(points1, points2, idx, dist2, layers, eps, save_mean, save_invstd, dout, dpoints1, dpoints2, grads, workspace,
                          cloud_off=None):
    """The backward of fp_train_forward_f32 through the batch statistics.  layers: per layer (weight, conv bias, BatchNorm weight, bias) --
    further entries are ignored; save_mean / save_invstd: what the forward wrote (never recomputed); dout, dpoints1, dpoints2, grads as in
    fp_backward_f32 (dbias is written as zeros); workspace: fp_train_backward_workspace_bytes(...) GPU bytes; cloud_off as in
    fp_backward_f32 (ampnet_fp_train_backward_ragged_f32)."""
    B, N, k, S, D1, D2 = _fp_geometry("fp_train_backward", points1, points2, idx, dist2,
                                      _saved_rows(save_mean, save_invstd) + _fp_backward_rows(dout, dpoints1, dpoints2))
    _check_grad_of("fp_train_backward", "dpoints1", dpoints1, "points1", points1)
    _check_grad_of("fp_train_backward", "dpoints2", dpoints2, "points2", points2)
    table, couts, epss = _mlp_tables("fp_train_backward", _saved_slots("fp_train_backward", layers, save_mean, save_invstd), D1 + D2, eps)
    _check_cout_last("fp_train_backward", layers, (B, N), "B, N", dout=dout)
    gtable = _grad_table("fp_train_backward", layers, grads)
    ws, ws_bytes = _workspace_args("fp_train_backward", workspace)
    if cloud_off is not None:
        Q, S1 = _ragged_clouds("fp_train_backward", cloud_off, B, S, "coarse points")
        with torch.cuda.device(points2.device):
            rc = lib().ampnet_fp_train_backward_ragged_f32(ptr(points1), D1, ptr(points2), D2, ptr(cloud_off), Q, N, S1, ptr(idx), ptr(dist2), k,
                                                           table, couts, epss, len(layers), ptr(dout), ptr(dpoints1), ptr(dpoints2), gtable, ws,
                                                           ws_bytes, stream_ptr(points2.device))
        return check(rc, "ampnet_fp_train_backward_ragged_f32")
    with torch.cuda.device(points2.device):
        rc = lib().ampnet_fp_train_backward_f32(ptr(points1), D1, ptr(points2), D2, B, N, S, ptr(idx), ptr(dist2), k, table, couts, epss,
                                                len(layers), ptr(dout), ptr(dpoints1), ptr(dpoints2), gtable, ws, ws_bytes,
                                                stream_ptr(points2.device))
    check(rc, "ampnet_fp_train_backward_f32")


# ---- the segmentation head: per-point classifier, eval forward and frozen-statistics backward ------------------------------------------
SEG_HEAD_MAX_CIN, SEG_HEAD_MAX_HIDDEN, SEG_HEAD_MAX_CLASSES = 256, 256, 32


def _seg_head_bytes(symbol, cin, hidden, n_classes, M):
    fn = getattr(lib(), symbol)
    fn.restype = ctypes.c_size_t
    need = fn(int(cin), int(hidden), int(n_classes), ctypes.c_longlong(int(M)))
    if not need:
        check(-1, symbol)
    return int(need)


def seg_head_forward_workspace_bytes(cin, hidden, n_classes, M):
    """Device bytes seg_head_forward_f32 needs (the BatchNorm fold); a shape outside the kernel's limits is an AmpnetError that names the
    limit."""
    return _seg_head_bytes("ampnet_seg_head_forward_workspace_bytes", cin, hidden, n_classes, M)


def seg_head_backward_workspace_bytes(cin, hidden, n_classes, M):
    """Device bytes seg_head_backward_f32 needs for M rows (include/ampnet_hip.h: ampnet_seg_head_backward_workspace_bytes)."""
    return _seg_head_bytes("ampnet_seg_head_backward_workspace_bytes", cin, hidden, n_classes, M)


def _seg_head_args(prefix, x, params, eps, extra):
    """x [M, ld] and the 8 parameters W1 [hidden, cin], b1, gamma, beta, running_mean, running_var, W2 [n_classes, hidden], b2 ->
    (M, ld, cin, hidden, n_classes, the pointer table of the C ABI).  conv1 is a layer of _mlp_tables; extra as in _sa_geometry."""
    _check_tensors(prefix, [("x", x, _F32, 2, True)] + extra)
    if len(params) != 8 or not torch.is_tensor(params[0]) or params[0].dim() != 2:
        raise AmpnetError(f"{prefix}: params must be the 8 tensors W1 [hidden, cin], b1, gamma, beta, running_mean, running_var, "
                          f"W2 [n_classes, hidden], b2")
    hidden, cin = (int(v) for v in params[0].shape)
    _mlp_tables(prefix, [tuple(params[:6])], cin, [eps])
    w2, b2 = params[6], params[7]
    n_classes = int(w2.shape[0]) if torch.is_tensor(w2) and w2.dim() == 2 else -1
    want = [(n_classes, hidden), (n_classes,)]
    if any(not torch.is_tensor(t) or tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
           for t, w in zip((w2, b2), want)):
        raise AmpnetError(f"{prefix}: W2 and b2 must be contiguous float32 GPU tensors of shapes [n_classes, {hidden}] and [n_classes], got "
                          f"{[tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in (w2, b2)]}")
    M, ld = x.shape
    if ld < cin:
        raise AmpnetError(f"{prefix}: x {tuple(x.shape)} must be [M, ld >= cin] with cin = {cin}")
    return M, ld, cin, hidden, n_classes, (ctypes.c_void_p * 8)(*[t.data_ptr() for t in params])


def _seg_head_grads(prefix, params, grads):
    """The six gradient tensors (dW1, db1, dgamma, dbeta, dW2, db2) checked against the parameters -> the pointer table of the C ABI."""
    want = [tuple(params[q].shape) for q in (0, 1, 1, 1, 6, 7)]
    if len(grads) != 6 or any(not torch.is_tensor(t) or tuple(t.shape) != w or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                              for t, w in zip(grads, want)):
        raise AmpnetError(f"{prefix}: grads must be six contiguous float32 GPU tensors (dW1, db1, dgamma, dbeta, dW2, db2) of "
                          f"shapes {want}, got {[tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in grads]}")
    return (ctypes.c_void_p * 6)(*[t.data_ptr() for t in grads])


def seg_head_forward_f32(x, params, eps, logp, preds, workspace):
    """The fused per-point classifier in eval mode (include/ampnet_hip.h: ampnet_seg_head_forward_f32).  x [M, ld >= cin] float32 rows,
    params the 8 tensors W1 [hidden, cin], b1, gamma, beta, running_mean, running_var, W2 [n_classes, hidden], b2, eps BatchNorm's;
    logp [M, n_classes] float32 and preds [M] int64 (or None): written; workspace: seg_head_forward_workspace_bytes(...) GPU bytes."""
    M, ld, cin, hidden, C, table = _seg_head_args("seg_head_forward", x, params, eps, [("logp", logp, _F32, 2, True),
                                                                                         ("preds", preds, torch.int64, 1, False)])
    if tuple(logp.shape) != (M, C) or (preds is not None and tuple(preds.shape) != (M,)):
        raise AmpnetError(f"seg_head_forward: logp {tuple(logp.shape)} must be [M, n_classes] = {[M, C]} and preds "
                          f"{None if preds is None else tuple(preds.shape)} [M] or None")
    ws, ws_bytes = _workspace_args("seg_head_forward", workspace)
    with torch.cuda.device(x.device):
        rc = lib().ampnet_seg_head_forward_f32(ptr(x), ld, ctypes.c_longlong(M), cin, hidden, C, table, ctypes.c_float(float(eps)), ptr(logp),
                                               ptr(preds), ws, ws_bytes, stream_ptr(x.device))
    check(rc, "ampnet_seg_head_forward_f32")


def seg_head_backward_f32(x, params, eps, dlogp, dx, grads, workspace):
    """The backward of seg_head_forward_f32 with the running statistics frozen.  x, params, eps: the forward's; dlogp [M, n_classes] any
    upstream gradient; dx [M, cin] or None (not wanted) and grads = (dW1, db1, dgamma, dbeta, dW2, db2): written; workspace:
    seg_head_backward_workspace_bytes(...) GPU bytes."""
    M, ld, cin, hidden, C, table = _seg_head_args("seg_head_backward", x, params, eps, [("dlogp", dlogp, _F32, 2, True),
                                                                                          ("dx", dx, _F32, 2, False)])
    if tuple(dlogp.shape) != (M, C):
        raise AmpnetError(f"seg_head_backward: dlogp {tuple(dlogp.shape)} must be [M, n_classes] = {[M, C]}")
    if dx is not None and tuple(dx.shape) != (M, cin):
        raise AmpnetError(f"seg_head_backward: dx {tuple(dx.shape)} must be [M, cin] = {[M, cin]} or None")
    gtable = _seg_head_grads("seg_head_backward", params, grads)
    ws, ws_bytes = _workspace_args("seg_head_backward", workspace)
    with torch.cuda.device(x.device):
        rc = lib().ampnet_seg_head_backward_f32(ptr(x), ld, ctypes.c_longlong(M), cin, hidden, C, table, ctypes.c_float(float(eps)), ptr(dlogp),
                                                ptr(dx), gtable, ws, ws_bytes, stream_ptr(x.device))
    check(rc, "ampnet_seg_head_backward_f32")


# ---- the segmentation head in train mode: batch-statistics bn1 and dropout ------------------------------------------------------------
def seg_head_train_forward_workspace_bytes(cin, hidden, n_classes, M):
    """Device bytes seg_head_train_forward_f32 needs (the fold and the statistics' partial rows); fewer than 2 or more than 2^24 rows are
    AmpnetErrors, as is a shape outside the eval head's limits."""
    return _seg_head_bytes("ampnet_seg_head_train_forward_workspace_bytes", cin, hidden, n_classes, M)


def seg_head_train_backward_workspace_bytes(cin, hidden, n_classes, M):
    """Device bytes seg_head_train_backward_f32 needs for M rows (include/ampnet_hip.h)."""
    return _seg_head_bytes("ampnet_seg_head_train_backward_workspace_bytes", cin, hidden, n_classes, M)


def _seg_head_saved(prefix, hidden, save_mean, save_invstd):
    if any(tuple(t.shape) != (hidden,) for t in (save_mean, save_invstd)):
        raise AmpnetError(f"{prefix}: save_mean {tuple(save_mean.shape)} and save_invstd {tuple(save_invstd.shape)} must be [hidden] = "
                          f"{[hidden]}")


def seg_head_train_forward_f32(x, params, eps, momentum, drop_p, seed, logp, save_mean, save_invstd, workspace):
    """The fused per-point classifier in train mode (include/ampnet_hip.h: ampnet_seg_head_train_forward_f32): bn1 on the statistics of
    the M rows, dropout with probability drop_p in [0, 1) and the mask `seed` selects.  x, params, eps as in seg_head_forward_f32;
    running_mean and running_var (params[4], params[5]) are UPDATED IN PLACE with `momentum` (a float in [0, 1]); logp [M, n_classes],
    save_mean / save_invstd [hidden]: written; workspace: seg_head_train_forward_workspace_bytes(...) GPU bytes."""
    M, ld, cin, hidden, C, table = _seg_head_args("seg_head_train_forward", x, params, eps,
                                                  [("logp", logp, _F32, 2, True)] + _saved_rows(save_mean, save_invstd))
    mom = _momentum("seg_head_train_forward", momentum)
    if tuple(logp.shape) != (M, C):
        raise AmpnetError(f"seg_head_train_forward: logp {tuple(logp.shape)} must be [M, n_classes] = {[M, C]}")
    _seg_head_saved("seg_head_train_forward", hidden, save_mean, save_invstd)
    ws, ws_bytes = _workspace_args("seg_head_train_forward", workspace)
    with torch.cuda.device(x.device):
        rc = lib().ampnet_seg_head_train_forward_f32(ptr(x), ld, ctypes.c_longlong(M), cin, hidden, C, table, ctypes.c_float(float(eps)), mom,
                                                     ctypes.c_float(float(drop_p)), ctypes.c_uint32(int(seed) & 0xFFFFFFFF), ptr(logp),
                                                     ptr(save_mean), ptr(save_invstd), ws, ws_bytes, stream_ptr(x.device))
    check(rc, "ampnet_seg_head_train_forward_f32")


def seg_head_train_backward_f32(x, params, eps, drop_p, seed, save_mean, save_invstd, dlogp, dx, grads, workspace):
    """The backward of seg_head_train_forward_f32 through the batch statistics and the dropout mask.  x, params, eps, drop_p, seed: the
    forward's (running_mean, running_var and b1 are not read); save_mean / save_invstd: what the forward wrote; dlogp, dx, grads as in
    seg_head_backward_f32 (db1 is written as zeros); workspace: seg_head_train_backward_workspace_bytes(...) GPU bytes."""
    M, ld, cin, hidden, C, table = _seg_head_args("seg_head_train_backward", x, params, eps,
                                                  _saved_rows(save_mean, save_invstd) + [("dlogp", dlogp, _F32, 2, True),
                                                                                         ("dx", dx, _F32, 2, False)])
    if tuple(dlogp.shape) != (M, C):
        raise AmpnetError(f"seg_head_train_backward: dlogp {tuple(dlogp.shape)} must be [M, n_classes] = {[M, C]}")
    if dx is not None and tuple(dx.shape) != (M, cin):
        raise AmpnetError(f"seg_head_train_backward: dx {tuple(dx.shape)} must be [M, cin] = {[M, cin]} or None")
    _seg_head_saved("seg_head_train_backward", hidden, save_mean, save_invstd)
    gtable = _seg_head_grads("seg_head_train_backward", params, grads)
    ws, ws_bytes = _workspace_args("seg_head_train_backward", workspace)
    with torch.cuda.device(x.device):
        rc = lib().ampnet_seg_head_train_backward_f32(ptr(x), ld, ctypes.c_longlong(M), cin, hidden, C, table, ctypes.c_float(float(eps)),
                                                      ctypes.c_float(float(drop_p)), ctypes.c_uint32(int(seed) & 0xFFFFFFFF), ptr(save_mean),
                                                      ptr(save_invstd), ptr(dlogp), ptr(dx), gtable, ws, ws_bytes, stream_ptr(x.device))
    check(rc, "ampnet_seg_head_train_backward_f32")


# ---- the loss behind the segmentation head: masked, weighted NLL with predictions and confusion counts (csrc/seg_loss.hip) ---------------
_F64, _I64 = torch.float64, torch.int64


def seg_nll_forward_workspace_bytes(M):
    """Device bytes seg_nll_forward_f32 needs for M rows (the workgroups' float64 partial rows); M outside [1, AMPNET_SEG_HEAD_MAX_ROWS] is
    an AmpnetError."""
    fn = lib().ampnet_seg_nll_forward_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = fn(ctypes.c_longlong(int(M)))
    if not need:
        check(-1, "ampnet_seg_nll_forward_workspace_bytes")
    return int(need)


def _seg_nll_args(prefix, target, class_w, C, extra):
    """target [M] int64, class_w [C] float32 or None and the wrapper's other tensors (`extra`: _check_tensors rows) -> M."""
    _check_tensors(prefix, [("target", target, _I64, 1, True), ("class_w", class_w, _F32, 1, False)] + extra)
    if class_w is not None and tuple(class_w.shape) != (C,):
        raise AmpnetError(f"{prefix}: class_w {tuple(class_w.shape)} must be [C] = {[C]} or None")
    return int(target.shape[0])


def seg_nll_forward_f32(logp, target, class_w, sums, loss, preds, counts, workspace):
    """The masked, weighted NLL of logp [M, C] float32 against target [M] int64 (a target outside [0, C) -- the drivers' -1 -- is ignored) with
    class_w [C] float32 or None (include/ampnet_hip.h: ampnet_seg_nll_forward_f32).  Written: sums [2] float64, loss [1] float32, preds [M]
    int64 or None (the lowest arg-max), counts [C * C + 1] int64 or None (confusion_device's layout); workspace:
    seg_nll_forward_workspace_bytes(M) GPU bytes."""
    _check_tensors("seg_nll_forward", [("logp", logp, _F32, 2, True)])
    M, C = (int(v) for v in logp.shape)
    m = _seg_nll_args("seg_nll_forward", target, class_w, C, [("sums", sums, _F64, 1, True), ("loss", loss, _F32, 1, True),
                                                              ("preds", preds, _I64, 1, False), ("counts", counts, _I64, 1, False)])
    if m != M or tuple(sums.shape) != (2,) or tuple(loss.shape) != (1,) or (preds is not None and tuple(preds.shape) != (M,)) \
            or (counts is not None and tuple(counts.shape) != (C * C + 1,)):
        raise AmpnetError(f"seg_nll_forward: logp {tuple(logp.shape)} needs target [M] = {[M]}, sums [2], loss [1], preds {[M]} or None and "
                          f"counts {[C * C + 1]} or None, got {tuple(target.shape)} {tuple(sums.shape)} {tuple(loss.shape)} "
                          f"{None if preds is None else tuple(preds.shape)} {None if counts is None else tuple(counts.shape)}")
    ws, ws_bytes = _workspace_args("seg_nll_forward", workspace)
    with torch.cuda.device(logp.device):
        rc = lib().ampnet_seg_nll_forward_f32(ptr(logp), ctypes.c_longlong(M), C, ptr(target), ptr(class_w), ptr(sums), ptr(loss), ptr(preds),
                                              ptr(counts), ws, ws_bytes, stream_ptr(logp.device))
    check(rc, "ampnet_seg_nll_forward_f32")


def seg_nll_backward_f32(target, class_w, sums, grad_loss, dlogp):
    """The backward of seg_nll_forward_f32: target, class_w, sums as the forward had / wrote them, grad_loss [1] float32 on the GPU (read
    there: no synchronisation); dlogp [M, C] float32: every element written, it may be uninitialised."""
    _check_tensors("seg_nll_backward", [("dlogp", dlogp, _F32, 2, True)])
    M, C = (int(v) for v in dlogp.shape)
    m = _seg_nll_args("seg_nll_backward", target, class_w, C, [("sums", sums, _F64, 1, True), ("grad_loss", grad_loss, _F32, 1, True)])
    if m != M or tuple(sums.shape) != (2,) or tuple(grad_loss.shape) != (1,):
        raise AmpnetError(f"seg_nll_backward: dlogp {tuple(dlogp.shape)} needs target [M] = {[M]}, sums [2] and grad_loss [1], got "
                          f"{tuple(target.shape)} {tuple(sums.shape)} {tuple(grad_loss.shape)}")
    with torch.cuda.device(dlogp.device):
        rc = lib().ampnet_seg_nll_backward_f32(ptr(target), ptr(class_w), ptr(sums), ptr(grad_loss), ctypes.c_longlong(M), C, ptr(dlogp),
                                               stream_ptr(dlogp.device))
    check(rc, "ampnet_seg_nll_backward_f32")


# ---- the input pipeline of clouds of unequal size (csrc/augment_clouds.hip) ---------------------------------------------------------------
def cloud_input_f32(raw, in_off, out_off, seed, step, permute, rotate, cos_a, sin_a, rows, targets, src=None):
    """One launch from the uploaded clusters to what forward_ragged and the loss consume (include/ampnet_hip.h: ampnet_cloud_input_f32).
    raw [total_in, 10] float32, in_off / out_off int32 [Q + 1] (the clouds in raw and in the padded output; TRUSTED: they are built on the
    host by the caller and not read back), seed / step: the keys of the point shuffle (u32), permute / rotate: flags, cos_a / sin_a: the
    step's angle.  Written, every element: rows [total_out, 9] float32, targets [total_out] int64 (-1 on padding rows), src [total_out]
    int32 or None (the row of raw behind every output row).  Contiguous GPU tensors."""
    _check_tensors("cloud_input", [("raw", raw, _F32, 2, True), ("in_off", in_off, _I32, 1, True), ("out_off", out_off, _I32, 1, True),
                                   ("rows", rows, _F32, 2, True), ("targets", targets, _I64, 1, True), ("src", src, _I32, 1, False)])
    Q = int(in_off.numel()) - 1
    total_in, total_out = int(raw.shape[0]), int(rows.shape[0])
    if raw.shape[1] != 10 or rows.shape[1] != 9 or Q < 1 or out_off.numel() != Q + 1 or targets.numel() != total_out \
            or (src is not None and src.numel() != total_out):
        raise AmpnetError(f"cloud_input: expected raw [total_in, 10], in_off and out_off [Q + 1 >= 2], rows [total_out, 9], targets and src "
                          f"[total_out], got {tuple(raw.shape)} {tuple(in_off.shape)} {tuple(out_off.shape)} {tuple(rows.shape)} "
                          f"{tuple(targets.shape)} {None if src is None else tuple(src.shape)}")
    with torch.cuda.device(raw.device):
        rc = lib().ampnet_cloud_input_f32(ptr(raw), ptr(in_off), ptr(out_off), Q, ctypes.c_longlong(total_in), ctypes.c_longlong(total_out),
                                          ctypes.c_uint32(int(seed) & 0xFFFFFFFF), ctypes.c_uint32(int(step) & 0xFFFFFFFF),
                                          int(bool(permute)), int(bool(rotate)), ctypes.c_double(float(cos_a)), ctypes.c_double(float(sin_a)),
                                          ptr(rows), ptr(targets), ptr(src), stream_ptr(raw.device))
    check(rc, "ampnet_cloud_input_f32")


# ---- the window token: one linear layer and a segmented max, fused (csrc/token_pool.hip) ------------------------------------------------
def _token_pool_workspace_bytes(symbol, cin, cout, Q, total):
    fn = getattr(lib(), symbol)
    fn.restype = ctypes.c_size_t
    need = fn(int(cin), int(cout), int(Q), ctypes.c_longlong(int(total)))
    if not need:
        check(-1, symbol)
    return int(need)


def token_pool_forward_workspace_bytes(cin, cout, Q, total):
    """Device bytes token_pool_forward_f32 needs for Q clouds of `total` rows in all, cin -> cout; a shape outside the kernel's limits is
    an AmpnetError that names the limit."""
    return _token_pool_workspace_bytes("ampnet_token_pool_forward_workspace_bytes", cin, cout, Q, total)


def token_pool_backward_workspace_bytes(cin, cout, Q, total):
    """Device bytes token_pool_backward_f32 needs (as token_pool_forward_workspace_bytes)."""
    return _token_pool_workspace_bytes("ampnet_token_pool_backward_workspace_bytes", cin, cout, Q, total)


def _token_pool_geometry(prefix, rows, cloud_off, weight, extra, per_cloud):
    """rows [total, cin], cloud_off int32 [Q + 1] (the device table of a utils.RaggedLayout: TRUSTED, it is not read back), weight
    [cout, cin] -> (Q, total, cin, cout).  extra: the _check_tensors rows of the wrapper's other tensors; per_cloud: the names among them
    that must be [Q, cout]."""
    _check_tensors(prefix, [("rows", rows, _F32, 2, True), ("cloud_off", cloud_off, _I32, 1, True), ("weight", weight, _F32, 2, True)] + extra)
    total, cin = rows.shape
    Q, cout = cloud_off.numel() - 1, weight.shape[0]
    if Q < 1 or weight.shape[1] != cin:
        raise AmpnetError(f"{prefix}: rows [total, cin], cloud_off [Q + 1 >= 2] and weight [cout, cin] do not agree: {tuple(rows.shape)} "
                          f"{tuple(cloud_off.shape)} {tuple(weight.shape)}")
    for name, t, _, _, _ in extra:
        if name in per_cloud and t is not None and tuple(t.shape) != (Q, cout):
            raise AmpnetError(f"{prefix}: {name} must be [Q, cout] = [{Q}, {cout}], got {tuple(t.shape)}")
    return Q, total, cin, cout


def token_pool_forward_f32(rows, cloud_off, weight, bias, out, workspace, arg_out=None):
    """ampnet_token_pool_forward_f32 (include/ampnet_hip.h): rows [total, cin] float32 = the clouds back to back, cloud_off int32 [Q + 1]
    on the device, weight [cout, cin], bias [cout]; written: out [Q, cout] float32 and arg_out [Q, cout] int32 or None (the lowest row of
    the cloud that attains each maximum); workspace: token_pool_forward_workspace_bytes(...) GPU bytes.  Contiguous GPU tensors."""
    Q, total, cin, cout = _token_pool_geometry("token_pool_forward", rows, cloud_off, weight,
                                               [("bias", bias, _F32, 1, True), ("out", out, _F32, 2, True), ("arg_out", arg_out, _I32, 2, False)],
                                               ("out", "arg_out"))
    if bias.numel() != cout:
        raise AmpnetError(f"token_pool_forward: bias must be [cout] = [{cout}], got {tuple(bias.shape)}")
    ws, ws_bytes = _workspace_args("token_pool_forward", workspace)
    with torch.cuda.device(rows.device):
        rc = lib().ampnet_token_pool_forward_f32(ptr(rows), ptr(cloud_off), Q, ctypes.c_longlong(total), ptr(weight), ptr(bias), cin, cout,
                                                 ptr(out), ptr(arg_out), ws, ws_bytes, stream_ptr(rows.device))
    check(rc, "ampnet_token_pool_forward_f32")


def token_pool_backward_f32(rows, cloud_off, weight, arg, dout, dx, dW, db, workspace):
    """ampnet_token_pool_backward_f32: rows, cloud_off, weight as in the forward, arg int32 [Q, cout] (the forward's arg_out), dout
    [Q, cout]; written, each or None when it is not wanted: dx [total, cin] (every element), dW [cout, cin], db [cout]; workspace:
    token_pool_backward_workspace_bytes(...) GPU bytes."""
    Q, total, cin, cout = _token_pool_geometry("token_pool_backward", rows, cloud_off, weight,
                                               [("arg", arg, _I32, 2, True), ("dout", dout, _F32, 2, True), ("dx", dx, _F32, 2, False),
                                                ("dW", dW, _F32, 2, False), ("db", db, _F32, 1, False)], ("arg", "dout"))
    for name, t, want in (("dx", dx, (total, cin)), ("dW", dW, (cout, cin)), ("db", db, (cout,))):
        if t is not None and tuple(t.shape) != want:
            raise AmpnetError(f"token_pool_backward: {name} must be {list(want)}, got {tuple(t.shape)}")
    ws, ws_bytes = _workspace_args("token_pool_backward", workspace)
    with torch.cuda.device(rows.device):
        rc = lib().ampnet_token_pool_backward_f32(ptr(rows), ptr(cloud_off), Q, ctypes.c_longlong(total), ptr(weight), cin, cout, ptr(arg),
                                                  ptr(dout), ptr(dx), ptr(dW), ptr(db), ws, ws_bytes, stream_ptr(rows.device))
    check(rc, "ampnet_token_pool_backward_f32")
