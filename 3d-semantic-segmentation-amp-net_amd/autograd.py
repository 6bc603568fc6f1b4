"""torch.autograd bridges for the drop-in modules.

When a caller drives the modules the reference's way -- pointnet(x) per window, att_net(...), a torch loss on the
logits, loss.backward(), optimizer.step() (train_pointnet-attention.py:396-470) -- autograd needs a backward for
the HIP forward.  These Functions call the C-ABI backward entry points; every forward in grad mode keeps a private
workspace alive until its backward has run (the reference makes W encoder calls before one backward).
The package's own train_loop does not go through autograd (trainer.fused_train_step).

Matrix precision: each forward opens _lib.precision_scope(module.precision) and records the mode it actually ran in on ctx; the
backward opens a scope with THAT mode.  It reads neither the module's attribute (which may have changed since) nor the process-wide
default, and the scope stack is per thread: autograd runs the backward on a thread of its own.
"""
import torch

from . import _lib, ops
from . import params as P


def _ordered_params(module, table):
    named = dict(module.named_parameters())
    return [named[n] for n in table.keys()]


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, x, *params):
        module, pt, bt, off, Q, total, mx, n_slots = meta
        ws = ops.Workspace()
        with _lib.precision_scope(module.precision):
            ctx.precision = _lib.effective_matrix_precision()
            local, glob, feat_T, _ = ops.encoder_forward(pt, bt, x, off, Q, total, mx, n_slots, True, ws)
        # tensors go through save_for_backward: keeping an OUTPUT on ctx directly makes an output -> grad_fn -> ctx -> output cycle
        # the garbage collector cannot break, i.e. the whole activation workspace leaks when the backward never runs
        ctx.save_for_backward(x, local, feat_T)
        ctx.meta = (module, pt, off, Q, total, mx, n_slots, ws)
        return local, glob, feat_T

    @staticmethod
    def backward(ctx, d_local, d_glob, d_ft):
        module, pt, off, Q, total, mx, n_slots, ws = ctx.meta
        x, local, feat_T = ctx.saved_tensors
        named = dict(module.named_parameters())
        grads = {n: torch.empty_like(named[n]) for n in P.ENC_PARAMS}
        gt = ops.PointerTable(P.ENC_PARAMS, grads, "encoder gradients")
        with _lib.precision_scope(ctx.precision):
            ops.encoder_backward(pt, gt, x, off, Q, total, mx, n_slots, local, feat_T,
                                 d_local.contiguous().float(), d_glob.contiguous().float(), d_ft.contiguous().float(),
                                 ws, ops.Workspace())
        ctx.meta = None
        return (None, None) + tuple(grads[n] for n in P.ENC_PARAMS)


def encoder_apply(module, pt, bt, rows, off, Q, total, mx, n_slots):
    params = _ordered_params(module, P.ENC_PARAMS)
    out = _EncoderFn.apply((module, pt, bt, off, Q, total, mx, n_slots), rows.contiguous(), *params)
    module._bump_batches(n_slots)
    return out


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, gl, lo, *params):
        module, pt, bt, cent, off, mask, B, W, total, mx, n_classes, p_drop, seed = meta
        ws = ops.Workspace()
        with _lib.precision_scope(module.precision):
            ctx.precision = _lib.effective_matrix_precision()
            logits, _, _ = ops.head_forward(pt, bt, gl, lo, cent, off, mask, B, W, total, mx, n_classes, True, p_drop, seed, ws)
        ctx.save_for_backward(lo)
        ctx.meta = (module, pt, cent, off, B, W, total, mx, n_classes, p_drop, seed, ws)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        module, pt, cent, off, B, W, total, mx, n_classes, p_drop, seed, ws = ctx.meta
        lo, = ctx.saved_tensors
        table = module._param_table()
        named = dict(module.named_parameters())
        grads = {n: torch.empty_like(named[n]) for n in table}
        gt = ops.PointerTable(table, grads, "head gradients")
        with _lib.precision_scope(ctx.precision):
            d_lo, d_gl = ops.head_backward(pt, gt, lo, cent, off, B, W, total, mx, n_classes, p_drop, seed,
                                           dlogits.contiguous().float(), ws, ops.Workspace())
        ctx.meta = None
        return (None, d_gl, d_lo) + tuple(grads[n] for n in table)


def head_apply(module, pt, bt, gl_rows, lo_rows, centroids, off, mask, B, W, total, mx, n_classes, p_drop, seed,
               targets=None, class_w=None, want_preds=False):
    """Grad-mode head forward: returns (logits, preds or None, None) -- the loss is the caller's (a torch loss on the
    logits back-propagates through _HeadFn)."""
    params = _ordered_params(module, module._param_table())
    cent = centroids.to(gl_rows.device).float().contiguous()
    logits = _HeadFn.apply((module, pt, bt, cent, off, mask, B, W, total, mx, n_classes, p_drop, seed),
                           gl_rows.contiguous().float(), lo_rows.contiguous().float(), *params)
    torch._foreach_add_([module.bn_2.num_batches_tracked, module.bn_3.num_batches_tracked], 1)
    preds = logits.detach().argmax(dim=1) if want_preds else None
    return logits, preds, None


class _GruHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, gl, lo, *params):
        module, pt, bt, off, B, W, total, mx, n_classes, p_drop, seed = meta
        ws = ops.Workspace()
        with _lib.precision_scope(module.precision):
            ctx.precision = _lib.effective_matrix_precision()
            logits, _, _ = ops.gru_head_forward(pt, bt, gl, lo, off, B, W, total, mx, n_classes, True, p_drop, seed, ws)
        ctx.save_for_backward(gl, lo)
        ctx.meta = (module, pt, off, B, W, total, mx, n_classes, p_drop, seed, ws)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        module, pt, off, B, W, total, mx, n_classes, p_drop, seed, ws = ctx.meta
        gl, lo = ctx.saved_tensors
        table = module._param_table()
        named = dict(module.named_parameters())
        grads = {n: torch.empty_like(named[n]) for n in table}
        gt = ops.PointerTable(table, grads, "GRU head gradients")
        with _lib.precision_scope(ctx.precision):
            d_lo, d_gl = ops.gru_head_backward(pt, gt, gl, lo, off, B, W, total, mx, n_classes, p_drop, seed,
                                               dlogits.contiguous().float(), ws, ops.Workspace())
        ctx.meta = None
        return (None, d_gl, d_lo) + tuple(grads[n] for n in table)


def gru_head_apply(module, pt, bt, gl_rows, lo_rows, off, B, W, total, mx, n_classes, p_drop, seed, want_preds=False):
    """Grad-mode forward of SegmentationWithGRU: (logits, preds or None, None); a torch loss on the logits back-propagates
    through _GruHeadFn (the reference's loop, pointNet/rnn/train_pointnetGRU.py:403-433)."""
    params = _ordered_params(module, module._param_table())
    logits = _GruHeadFn.apply((module, pt, bt, off, B, W, total, mx, n_classes, p_drop, seed),
                              gl_rows.contiguous().float(), lo_rows.contiguous().float(), *params)
    torch._foreach_add_([module.bn_2.num_batches_tracked, module.bn_3.num_batches_tracked], 1)
    preds = logits.detach().argmax(dim=1) if want_preds else None
    return logits, preds, None


class _ClsHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, gl, *params):
        module, pt, bt, mask, B, W, n_classes, p_drop, seed = meta
        ws = ops.Workspace()
        with _lib.precision_scope(module.precision):
            ctx.precision = _lib.effective_matrix_precision()
            out, aw = ops.cls_head_forward(pt, bt, gl, mask, B, W, n_classes, True, p_drop, seed, ws)
        ctx.save_for_backward(gl)
        ctx.meta = (module, pt, B, W, n_classes, p_drop, seed, ws)
        ctx.mark_non_differentiable(aw)
        return out, aw

    @staticmethod
    def backward(ctx, d_out, _d_aw):
        module, pt, B, W, n_classes, p_drop, seed, ws = ctx.meta
        gl, = ctx.saved_tensors
        table = module._param_table()
        named = dict(module.named_parameters())
        grads = {n: torch.empty_like(named[n]) for n in table}
        gt = ops.PointerTable(table, grads, "classification head gradients")
        with _lib.precision_scope(ctx.precision):
            d_gl = ops.cls_head_backward(pt, gt, gl, B, W, n_classes, p_drop, seed, d_out.contiguous().float(), ws, ops.Workspace())
        ctx.meta = None
        return (None, d_gl) + tuple(grads[n] for n in table)


def cls_head_apply(module, pt, bt, gl_rows, mask, B, W, n_classes, p_drop, seed):
    params = _ordered_params(module, module._param_table())
    out, aw = _ClsHeadFn.apply((module, pt, bt, mask, B, W, n_classes, p_drop, seed), gl_rows.contiguous().float(), *params)
    module.bn_2.num_batches_tracked += 1
    return out, aw


# ---- what the five PointNet++ Functions below share ------------------------------------------------------------------------------------
def _block_tensors(module, stats=True, w0=None):
    """The conv and BatchNorm tensors of a PointNetSetAbstraction / PointNetFeaturePropagation block, the module's own, layer after layer:
    conv weight, conv bias, BatchNorm weight, bias and, with `stats`, running_mean, running_var.  w0: what stands in for layer 0's conv
    weight (a branch of PointNetSetAbstractionMsg hands it with its columns rotated, by a differentiable op when a graph is wanted)."""
    return [t for l, (conv, bn) in enumerate(zip(module.mlp_convs, module.mlp_bns))
            for t in (w0 if l == 0 and w0 is not None else conv.weight, conv.bias, bn.weight, bn.bias)
            + ((bn.running_mean, bn.running_var) if stats else ())]


def _mlp_layers(tensors, per):
    """The `per` contiguous float32 tensors per layer that the C ABI takes, from the module's own (weight [out, in, 1(, 1)] -> [out, in])."""
    return [tuple(t.detach().reshape(t.shape[0], -1).float().contiguous() if q == 0 else t.detach().float().contiguous()
                  for q, t in enumerate(tensors[i:i + per])) for i in range(0, len(tensors), per)]


def _couts(layers):
    return [int(layer[0].shape[0]) for layer in layers]


def _width(t):
    return 0 if t is None else t.shape[2]


def _ws(nbytes, device):
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _alloc_grads(layers):
    return [tuple(torch.empty_like(t) for t in layer[:4]) for layer in layers]


def _param_grads(tensors, grads, per, need_grad, first):
    """The parameter tail of a backward's return tuple.  tensors: the forward's *tensors, `per` of them per layer, tensors[0] being the
    forward's argument number `first`; grads: per layer (dW, dbias, dgamma, dbeta).  dW takes the conv weight's own shape (its trailing
    singleton dimensions), the running statistics (per = 6) get None, and so does every tensor that did not ask for a gradient."""
    ret = []
    for l, g in enumerate(grads):
        for q in range(per):
            wanted = q < 4 and need_grad[first + per * l + q]
            ret.append(None if not wanted else g[q] if q else g[0].reshape(tensors[per * l].shape))
    return tuple(ret)


_ragged_note = """cloud_off of fp_apply, fp_train_apply, sa_apply and sa_train_apply (pointnet2_utils' _forward_ragged).  None: B clouds of one size.
An int32 [Q + 1] device table (utils.RaggedLayout.off): the tensors hold Q clouds of UNEQUAL size packed back to back as ONE cloud
(leading dimension 1, N = total) with the Q * S centres or coarse points behind one another and GLOBAL indices, as the ragged searches
write them.  The forwards need nothing else -- no row of theirs mixes with another, and batch statistics over all rows of the call are
the right statistics -- and run unchanged; the backward goes through the ampnet_*_backward_ragged_f32 entry points, whose last gather
scans a point's own cloud and not the whole array (include/ampnet_hip.h)."""


class _FpFn(torch.autograd.Function):
    """One fused feature-propagation layer with BatchNorm's running statistics frozen (pointnet2_utils.PointNetFeaturePropagation with
    grad=True).  tensors: per layer conv weight [out, in, 1], conv bias, BatchNorm weight, bias, running_mean, running_var.  The forward
    is the eval forward, unchanged, and keeps no activation: the backward kernel recomputes them (csrc/feature_propagation_bwd.hip).
    Exact fp32 whatever the matrix precision is, so there is no precision scope to carry over.
    cloud_off: None, or the int32 [Q + 1] device table of Q fine clouds of unequal size that p1 .. dist2 hold packed as ONE cloud with global
    indices (_ragged_note): the forward is unchanged and the backward gathers dp2 cloud by cloud."""

    @staticmethod
    def forward(ctx, eps, cloud_off, fold_ws, p1, p2, idx, dist2, *tensors):
        layers = _mlp_layers(tensors, 6)
        out = torch.empty((p2.shape[0], idx.shape[1], layers[-1][0].shape[0]), dtype=torch.float32, device=p2.device)
        _lib.fp_forward_f32(p1, p2, idx, dist2, layers, eps, out, fold_ws)
        ctx.save_for_backward(p1, p2, idx, dist2, *tensors)        # (inputs only: see the note in _EncoderFn.forward)
        ctx.eps, ctx.cloud_off = eps, cloud_off
        return out

    @staticmethod
    def backward(ctx, dout):
        p1, p2, idx, dist2, *tensors = ctx.saved_tensors
        layers = _mlp_layers(tensors, 6)
        dp1 = None if p1 is None else torch.empty_like(p1)
        dp2 = torch.empty_like(p2)
        grads = _alloc_grads(layers)
        need = _lib.fp_backward_workspace_bytes(_width(p1), p2.shape[2], p2.shape[0], idx.shape[1], _couts(layers))
        _lib.fp_backward_f32(p1, p2, idx, dist2, layers, ctx.eps, dout.contiguous().float(), dp1, dp2, grads, _ws(need, p2.device),
                             cloud_off=ctx.cloud_off)
        need_grad = ctx.needs_input_grad
        return (None, None, None, dp1 if need_grad[3] else None, dp2 if need_grad[4] else None, None, None) \
            + _param_grads(tensors, grads, 6, need_grad, 7)


def fp_apply(module, p1, p2, idx, dist2, fold_ws, cloud_off=None):
    """Grad-mode forward of a PointNetFeaturePropagation block on point-major rows: p1 [B, N, D1] or None, p2 [B, S, D2], idx / dist2
    [B, N, k] from utils.three_nn -> [B, N, mlp[-1]] with a graph to p1, p2 and the block's conv and BatchNorm affine parameters.
    cloud_off: _ragged_note."""
    return _FpFn.apply([bn.eps for bn in module.mlp_bns], cloud_off, fold_ws, p1, p2, idx, dist2, *_block_tensors(module))


class _FpTrainFn(torch.autograd.Function):
    """One fused feature-propagation layer with TRAIN-mode BatchNorm (pointnet2_utils.PointNetFeaturePropagation with grad=True and
    batch_stats=True, in train mode).  tensors: per layer conv weight [out, in, 1], conv bias, BatchNorm weight, bias; stats: per layer the
    module's (running_mean, running_var) buffers, updated in place by the forward and NOT saved -- the backward takes the batch statistics
    the forward wrote (save_mean, save_invstd), so a later forward cannot change an earlier one's gradient.  Exact fp32 whatever the matrix
    precision is (csrc/feature_propagation_train.hip)."""

    @staticmethod
    def forward(ctx, eps, cloud_off, momentum, stats, p1, p2, idx, dist2, *tensors):
        layers = [layer + tuple(st) for layer, st in zip(_mlp_layers(tensors, 4), stats)]
        out, save_mean, save_invstd = fp_train_forward(p1, p2, idx, dist2, layers, eps, momentum)
        ctx.save_for_backward(p1, p2, idx, dist2, save_mean, save_invstd, *tensors)
        ctx.eps, ctx.cloud_off = eps, cloud_off
        return out

    @staticmethod
    def backward(ctx, dout):
        p1, p2, idx, dist2, save_mean, save_invstd, *tensors = ctx.saved_tensors
        layers = _mlp_layers(tensors, 4)
        dp1 = None if p1 is None else torch.empty_like(p1)
        dp2 = torch.empty_like(p2)
        grads = _alloc_grads(layers)
        need = _lib.fp_train_backward_workspace_bytes(_width(p1), p2.shape[2], p2.shape[0], idx.shape[1], _couts(layers))
        _lib.fp_train_backward_f32(p1, p2, idx, dist2, layers, ctx.eps, save_mean, save_invstd, dout.contiguous().float(), dp1, dp2, grads,
                                   _ws(need, p2.device), cloud_off=ctx.cloud_off)
        need_grad = ctx.needs_input_grad
        return (None, None, None, None, dp1 if need_grad[4] else None, dp2 if need_grad[5] else None, None, None) \
            + _param_grads(tensors, grads, 4, need_grad, 8)                         # (dbias is zeros)


def fp_train_forward(p1, p2, idx, dist2, layers, eps, momentum):
    """ampnet_fp_train_forward_f32 on layers of six tensors (the running statistics are updated in place) -> (out, save_mean, save_invstd)."""
    couts = _couts(layers)
    out = torch.empty((p2.shape[0], idx.shape[1], couts[-1]), dtype=torch.float32, device=p2.device)
    save_mean, save_invstd = (torch.empty(sum(couts), dtype=torch.float32, device=p2.device) for _ in range(2))
    need = _lib.fp_train_forward_workspace_bytes(_width(p1), p2.shape[2], p2.shape[0], idx.shape[1], couts)
    _lib.fp_train_forward_f32(p1, p2, idx, dist2, layers, eps, momentum, out, save_mean, save_invstd, _ws(need, p2.device))
    return out, save_mean, save_invstd


def fp_train_apply(module, p1, p2, idx, dist2, momentum, cloud_off=None):
    """Grad-mode, train-mode forward of a PointNetFeaturePropagation block on point-major rows (as fp_apply): batch statistics, the
    module's running statistics updated in place, a graph to p1, p2 and the block's conv and BatchNorm affine parameters (the conv bias
    gets zeros: it has no effect on a batch-normalised output).  cloud_off: _ragged_note."""
    stats = [(bn.running_mean, bn.running_var) for bn in module.mlp_bns]
    return _FpTrainFn.apply([bn.eps for bn in module.mlp_bns], cloud_off, momentum, stats, p1, p2, idx, dist2,
                            *_block_tensors(module, stats=False))


class _SaFn(torch.autograd.Function):
    """One fused set-abstraction layer with BatchNorm's running statistics frozen (pointnet2_utils.PointNetSetAbstraction with grad=True).
    tensors: per layer conv weight [out, in, 1, 1], conv bias, BatchNorm weight, bias, running_mean, running_var.  The forward is the eval
    forward, unchanged, and keeps its inputs only: the backward kernel recomputes the activations and the max's choice
    (csrc/set_abstraction_bwd.hip).  Exact fp32 whatever the matrix precision is, so there is no precision scope to carry over."""

    @staticmethod
    def forward(ctx, eps, cloud_off, fold_ws, x, centres, group_idx, feats, *tensors):
        layers = _mlp_layers(tensors, 6)
        out = torch.empty((x.shape[0], centres.shape[1], layers[-1][0].shape[0]), dtype=torch.float32, device=x.device)
        _lib.sa_forward_f32(x, centres, group_idx, feats, layers, eps, out, fold_ws)
        ctx.save_for_backward(x, centres, group_idx, feats, *tensors)        # (inputs only: see the note in _EncoderFn.forward)
        ctx.eps, ctx.cloud_off = eps, cloud_off
        return out

    @staticmethod
    def backward(ctx, dout):
        x, centres, group_idx, feats, *tensors = ctx.saved_tensors
        layers = _mlp_layers(tensors, 6)
        need_grad = ctx.needs_input_grad
        dfeats = torch.empty_like(feats) if feats is not None and need_grad[6] else None
        grads = _alloc_grads(layers)
        need = _lib.sa_backward_workspace_bytes(_width(feats), x.shape[0], centres.shape[1], group_idx.shape[2], _couts(layers))
        _lib.sa_backward_f32(x, centres, group_idx, feats, layers, ctx.eps, dout.contiguous().float(), dfeats, grads, _ws(need, x.device),
                             arg_out=None, cloud_off=ctx.cloud_off)
        return (None, None, None, None, None, None, dfeats) + _param_grads(tensors, grads, 6, need_grad, 7)


def sa_apply(module, x, centres, group_idx, feats, fold_ws, w0=None, cloud_off=None):
    """Grad-mode forward of a PointNetSetAbstraction block on point-major rows: x [B, N, 3], centres [B, S] and group_idx [B, S, nsample]
    int32, feats [B, N, D] or None -> [B, S, mlp[-1]] with a graph to feats and the block's conv and BatchNorm affine parameters.
    w0: as in _block_tensors.  cloud_off: _ragged_note."""
    return _SaFn.apply([bn.eps for bn in module.mlp_bns], cloud_off, fold_ws, x, centres, group_idx, feats, *_block_tensors(module, w0=w0))


class _SaAllFn(torch.autograd.Function):
    """One fused set-abstraction layer over ONE group of all points per cloud (pointnet2_utils.PointNetSetAbstraction with group_all=True
    and grad=True), BatchNorm's running statistics frozen.  tensors as in _SaFn.  The forward is the eval forward and also asks for the row
    each maximum came from: [B, cout_last] int32, tiny, and it spares the backward a second pass over all N rows -- the backward runs on
    those rows alone (csrc/set_abstraction_all.hip).  Exact fp32 whatever the matrix precision is."""

    @staticmethod
    def forward(ctx, eps, x, feats, *tensors):
        out, arg = sa_all_forward(x, feats, _mlp_layers(tensors, 6), eps, want_arg=True)
        ctx.save_for_backward(x, feats, arg, *tensors)               # (inputs and arg only: see the note in _EncoderFn.forward)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dout):
        x, feats, arg, *tensors = ctx.saved_tensors
        layers = _mlp_layers(tensors, 6)
        need_grad = ctx.needs_input_grad
        dfeats = torch.empty_like(feats) if feats is not None and need_grad[2] else None
        grads = _alloc_grads(layers)
        need = _lib.sa_all_backward_workspace_bytes(_width(feats), x.shape[0], x.shape[1], _couts(layers))
        _lib.sa_all_backward_f32(x, feats, layers, ctx.eps, arg, dout.contiguous().float(), dfeats, grads, _ws(need, x.device))
        return (None, None, dfeats) + _param_grads(tensors, grads, 6, need_grad, 3)


def sa_all_forward(x, feats, layers, eps, want_arg=False):
    """ampnet_sa_all_forward_f32 on layers of six tensors -> (out [B, cout_last], arg int32 [B, cout_last] or None)."""
    couts = _couts(layers)
    out = torch.empty((x.shape[0], couts[-1]), dtype=torch.float32, device=x.device)
    arg = torch.empty((x.shape[0], couts[-1]), dtype=torch.int32, device=x.device) if want_arg else None
    need = _lib.sa_all_forward_workspace_bytes(_width(feats), x.shape[0], x.shape[1], couts)
    _lib.sa_all_forward_f32(x, feats, layers, eps, out, _ws(need, x.device), arg_out=arg)
    return out, arg


def sa_all_apply(module, x, feats):
    """Grad-mode forward of a group_all PointNetSetAbstraction block on point-major rows: x [B, N, 3], feats [B, N, D] or None ->
    [B, mlp[-1]] with a graph to feats and the block's conv and BatchNorm affine parameters."""
    return _SaAllFn.apply([bn.eps for bn in module.mlp_bns], x, feats, *_block_tensors(module))


class _SaTrainFn(torch.autograd.Function):
    """One fused set-abstraction layer with TRAIN-mode BatchNorm (pointnet2_utils.PointNetSetAbstraction with grad=True and
    batch_stats=True, in train mode).  tensors: per layer conv weight [out, in, 1, 1], conv bias, BatchNorm weight, bias; stats: per layer
    the module's (running_mean, running_var) buffers, updated in place by the forward and NOT saved -- the backward takes the batch
    statistics the forward wrote (save_mean, save_invstd), so a later forward cannot change an earlier one's gradient.  Exact fp32 whatever
    the matrix precision is (csrc/set_abstraction_train.hip)."""

    @staticmethod
    def forward(ctx, eps, cloud_off, momentum, stats, x, centres, group_idx, feats, *tensors):
        layers = [layer + tuple(st) for layer, st in zip(_mlp_layers(tensors, 4), stats)]
        out, save_mean, save_invstd = sa_train_forward(x, centres, group_idx, feats, layers, eps, momentum)
        ctx.save_for_backward(x, centres, group_idx, feats, save_mean, save_invstd, *tensors)
        ctx.eps, ctx.cloud_off = eps, cloud_off
        return out

    @staticmethod
    def backward(ctx, dout):
        x, centres, group_idx, feats, save_mean, save_invstd, *tensors = ctx.saved_tensors
        layers = _mlp_layers(tensors, 4)
        need_grad = ctx.needs_input_grad
        dfeats = torch.empty_like(feats) if feats is not None and need_grad[7] else None
        grads = _alloc_grads(layers)
        need = _lib.sa_train_backward_workspace_bytes(_width(feats), x.shape[0], centres.shape[1], group_idx.shape[2], _couts(layers))
        _lib.sa_train_backward_f32(x, centres, group_idx, feats, layers, ctx.eps, save_mean, save_invstd, dout.contiguous().float(), dfeats,
                                   grads, _ws(need, x.device), arg_out=None, cloud_off=ctx.cloud_off)
        return (None, None, None, None, None, None, None, dfeats) + _param_grads(tensors, grads, 4, need_grad, 8)      # (dbias is zeros)


def sa_train_forward(x, centres, group_idx, feats, layers, eps, momentum):
    """ampnet_sa_train_forward_f32 on layers of six tensors (the running statistics are updated in place) -> (out, save_mean, save_invstd)."""
    couts = _couts(layers)
    out = torch.empty((x.shape[0], centres.shape[1], couts[-1]), dtype=torch.float32, device=x.device)
    save_mean, save_invstd = (torch.empty(sum(couts), dtype=torch.float32, device=x.device) for _ in range(2))
    need = _lib.sa_train_forward_workspace_bytes(_width(feats), x.shape[0], centres.shape[1], group_idx.shape[2], couts)
    _lib.sa_train_forward_f32(x, centres, group_idx, feats, layers, eps, momentum, out, save_mean, save_invstd, _ws(need, x.device))
    return out, save_mean, save_invstd


def sa_train_apply(module, x, centres, group_idx, feats, momentum, w0=None, cloud_off=None):
    """Grad-mode, train-mode forward of a PointNetSetAbstraction block on point-major rows (as sa_apply): batch statistics over all
    B * npoint * nsample rows, the module's running statistics updated in place, a graph to feats and the block's conv and BatchNorm affine
    parameters (the conv bias gets zeros: it has no effect on a batch-normalised output).  w0: as in _block_tensors.  cloud_off:
    _ragged_note."""
    stats = [(bn.running_mean, bn.running_var) for bn in module.mlp_bns]
    return _SaTrainFn.apply([bn.eps for bn in module.mlp_bns], cloud_off, momentum, stats, x, centres, group_idx, feats,
                            *_block_tensors(module, stats=False, w0=w0))


def seg_head_tensors(module):
    """The eight tensors of a PointNetSegHead, the module's own: conv1 weight [hidden, in, 1] and bias, bn1 weight, bias, running_mean,
    running_var, conv2 weight [classes, hidden, 1] and bias."""
    return [module.conv1.weight, module.conv1.bias, module.bn1.weight, module.bn1.bias, module.bn1.running_mean, module.bn1.running_var,
            module.conv2.weight, module.conv2.bias]


def seg_head_params(tensors):
    """The eight contiguous float32 tensors the C ABI takes, from seg_head_tensors' (the conv weights as [out, in])."""
    return [t.detach().reshape(t.shape[0], -1).float().contiguous() if q in (0, 6) else t.detach().float().contiguous()
            for q, t in enumerate(tensors)]


_SEG_GRAD_SLOTS = (0, 1, 2, 3, 6, 7)                                # of seg_head_tensors: the tensors that have a gradient, in the C ABI's order


class _SegHeadFn(torch.autograd.Function):
    """The fused per-point classifier with bn1's running statistics frozen (pointnet2_utils.PointNetSegHead with grad=True).  rows [M, cin];
    tensors: seg_head_tensors.  The forward is the eval forward, unchanged, and keeps no activation: the backward kernel recomputes them
    (csrc/seg_head_bwd.hip).  Exact fp32 whatever the matrix precision is, so there is no precision scope to carry over."""

    @staticmethod
    def forward(ctx, eps, fold_ws, rows, *tensors):
        params = seg_head_params(tensors)
        logp = torch.empty((rows.shape[0], params[6].shape[0]), dtype=torch.float32, device=rows.device)
        _lib.seg_head_forward_f32(rows, params, eps, logp, None, fold_ws)
        ctx.save_for_backward(rows, *tensors)                      # (inputs only: see the note in _EncoderFn.forward)
        ctx.eps = eps
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        rows, *tensors = ctx.saved_tensors
        params = seg_head_params(tensors)
        need_grad = ctx.needs_input_grad
        dx = torch.empty((rows.shape[0], params[0].shape[1]), dtype=torch.float32, device=rows.device) if need_grad[2] else None
        grads = [torch.empty_like(params[q]) for q in _SEG_GRAD_SLOTS]
        need = _lib.seg_head_backward_workspace_bytes(params[0].shape[1], params[0].shape[0], params[6].shape[0], rows.shape[0])
        _lib.seg_head_backward_f32(rows, params, ctx.eps, dlogp.contiguous().float(), dx, grads, _ws(need, rows.device))
        ret = [None] * 8
        for g, q in zip(grads, _SEG_GRAD_SLOTS):
            if need_grad[3 + q]:
                ret[q] = g.reshape(tensors[q].shape)
        return (None, None, dx) + tuple(ret)


def seg_head_train_forward(rows, params, eps, momentum, p, seed):
    """ampnet_seg_head_train_forward_f32 on the eight tensors of seg_head_params, running_mean and running_var (entries 4 and 5) being the
    buffers themselves: updated in place -> (logp [M, classes], save_mean, save_invstd)."""
    hidden, cin = params[0].shape
    logp = torch.empty((rows.shape[0], params[6].shape[0]), dtype=torch.float32, device=rows.device)
    save_mean, save_invstd = (torch.empty(hidden, dtype=torch.float32, device=rows.device) for _ in range(2))
    need = _lib.seg_head_train_forward_workspace_bytes(cin, hidden, params[6].shape[0], rows.shape[0])
    _lib.seg_head_train_forward_f32(rows, params, eps, momentum, p, seed, logp, save_mean, save_invstd, _ws(need, rows.device))
    return logp, save_mean, save_invstd


class _SegHeadTrainFn(torch.autograd.Function):
    """The fused per-point classifier in TRAIN mode (pointnet2_utils.PointNetSegHead with grad=True and batch_stats=True, in train mode):
    bn1 on the batch's statistics, dropout with probability p and the mask `seed` selects.  stats: the module's (running_mean, running_var)
    buffers, updated in place by the forward and NOT saved; tensors: conv1 weight and bias, bn1 weight and bias, conv2 weight and bias.
    Saved for the backward: the rows, save_mean, save_invstd and the six tensors, with p and the seed -- no activation and no mask: the
    backward kernels recompute both (csrc/seg_head_train_bwd.hip).  Exact fp32 whatever the matrix precision is."""

    @staticmethod
    def forward(ctx, eps, momentum, p, seed, stats, rows, *tensors):
        params = seg_head_params(list(tensors[:4]) + list(stats) + list(tensors[4:]))
        params[4], params[5] = stats                               # (the buffers themselves: float32 and contiguous by construction)
        logp, save_mean, save_invstd = seg_head_train_forward(rows, params, eps, momentum, p, seed)
        ctx.save_for_backward(rows, save_mean, save_invstd, *tensors)
        ctx.eps, ctx.p, ctx.seed = eps, p, seed
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        rows, save_mean, save_invstd, *tensors = ctx.saved_tensors
        params = seg_head_params(list(tensors[:4]) + [save_mean, save_invstd] + list(tensors[4:]))      # (slots 4 and 5 are not read)
        need_grad = ctx.needs_input_grad
        dx = torch.empty((rows.shape[0], params[0].shape[1]), dtype=torch.float32, device=rows.device) if need_grad[5] else None
        grads = [torch.empty_like(params[q]) for q in _SEG_GRAD_SLOTS]
        need = _lib.seg_head_train_backward_workspace_bytes(params[0].shape[1], params[0].shape[0], params[6].shape[0], rows.shape[0])
        _lib.seg_head_train_backward_f32(rows, params, ctx.eps, ctx.p, ctx.seed, save_mean, save_invstd, dlogp.contiguous().float(), dx, grads,
                                         _ws(need, rows.device))
        ret = [g.reshape(t.shape) if need_grad[6 + q] else None for q, (g, t) in enumerate(zip(grads, tensors))]      # (db1 is zeros)
        return (None, None, None, None, None, dx) + tuple(ret)


def seg_head_train_apply(module, rows, momentum, p, seed):
    """Grad-mode, train-mode forward of a PointNetSegHead on rows [M, in_channel] -> log-probabilities [M, num_classes]: batch statistics,
    bn1's running statistics updated in place, dropout, a graph to the rows and to conv1, bn1 (weight and bias) and conv2 (conv1's bias
    gets zeros: it has no effect on a batch-normalised output)."""
    t = seg_head_tensors(module)
    return _SegHeadTrainFn.apply(module.bn1.eps, momentum, p, seed, (t[4], t[5]), rows, *(t[q] for q in _SEG_GRAD_SLOTS))


def seg_head_apply(module, rows, fold_ws):
    """Grad-mode forward of a PointNetSegHead on rows [M, in_channel] -> log-probabilities [M, num_classes] with a graph to the rows and to
    the head's conv1, bn1 (weight and bias) and conv2."""
    return _SegHeadFn.apply(module.bn1.eps, fold_ws, rows, *seg_head_tensors(module))


def seg_nll_forward(logp, target, class_w, want_preds, want_counts):
    """ampnet_seg_nll_forward_f32 on logp [M, C], target [M] -> (loss 0-d, sums [2] float64, preds [M] or None, counts [C * C + 1] or None)."""
    M, C = logp.shape
    dev = logp.device
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    preds = torch.empty(M, dtype=torch.int64, device=dev) if want_preds else None
    counts = torch.empty(C * C + 1, dtype=torch.int64, device=dev) if want_counts else None
    _lib.seg_nll_forward_f32(logp, target, class_w, sums, loss, preds, counts, _ws(_lib.seg_nll_forward_workspace_bytes(M), dev))
    return loss.reshape(()), sums, preds, counts


class _SegNllFn(torch.autograd.Function):
    """The masked, weighted NLL behind the segmentation head (pointnet2_utils.seg_nll_loss): logp [M, C] -> (loss 0-d, preds, counts), the
    last two None when not wanted.  Saved for the backward: target, class_w and the forward's float64 sums -- not logp, the gradient does
    not depend on it.  preds and counts are integers: marked non-differentiable."""

    @staticmethod
    def forward(ctx, logp, target, class_w, want_preds, want_counts):
        loss, sums, preds, counts = seg_nll_forward(logp, target, class_w, want_preds, want_counts)
        ctx.save_for_backward(target, sums, *(() if class_w is None else (class_w,)))
        ctx.shape = tuple(logp.shape)
        ctx.mark_non_differentiable(*(t for t in (preds, counts) if t is not None))
        return loss, preds, counts

    @staticmethod
    def backward(ctx, gloss, _gpreds, _gcounts):
        target, sums, *w = ctx.saved_tensors
        dlogp = torch.empty(ctx.shape, dtype=torch.float32, device=target.device)
        _lib.seg_nll_backward_f32(target, w[0] if w else None, sums, gloss.detach().float().reshape(1).contiguous(), dlogp)
        return dlogp, None, None, None, None


# ---- the window token of pointnet_2: conv1 and the max over a cloud's points, fused (csrc/token_pool.hip) ---------------------------------
def token_pool_forward(rows, cloud_off, weight, bias, want_arg=False):
    """ampnet_token_pool_forward_f32 on rows [total, cin], the device table cloud_off int32 [Q + 1], weight [cout, cin], bias [cout]
    -> (tokens [Q, cout], arg int32 [Q, cout] or None)."""
    Q, cout = cloud_off.numel() - 1, weight.shape[0]
    out = torch.empty((Q, cout), dtype=torch.float32, device=rows.device)
    arg = torch.empty((Q, cout), dtype=torch.int32, device=rows.device) if want_arg else None
    need = _lib.token_pool_forward_workspace_bytes(rows.shape[1], cout, Q, rows.shape[0])
    _lib.token_pool_forward_f32(rows, cloud_off, weight, bias, out, _ws(need, rows.device), arg_out=arg)
    return out, arg


class _TokenPoolFn(torch.autograd.Function):
    """tokens[q, c] = max over the rows of cloud q of (weight[c, :] . row + bias[c]) (pointnet2_utils.token_pool): rows [total, cin]
    float32 contiguous, cloud_off the int32 [Q + 1] device table, weight [cout, cin] or nn.Conv1d's [cout, cin, 1], bias [cout]
    -> (tokens [Q, cout], arg int32 [Q, cout]).  Saved for the backward: the inputs and arg only -- the [total, cout] products are never
    stored, the backward runs on the winning rows alone.  The lowest row takes the whole gradient of a tie.  Exact fp32 whatever the
    matrix precision is, so there is no precision scope to carry over.  arg is an integer: marked non-differentiable."""

    @staticmethod
    def forward(ctx, cloud_off, rows, weight, bias):
        w = weight.detach().reshape(weight.shape[0], -1).float().contiguous()
        out, arg = token_pool_forward(rows, cloud_off, w, bias.detach().float().contiguous(), want_arg=True)
        ctx.save_for_backward(rows, cloud_off, arg, weight)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        rows, cloud_off, arg, weight = ctx.saved_tensors
        w = weight.detach().reshape(weight.shape[0], -1).float().contiguous()
        need_grad = ctx.needs_input_grad
        dx = torch.empty_like(rows) if need_grad[1] else None
        dW = torch.empty_like(w) if need_grad[2] else None
        db = torch.empty(w.shape[0], dtype=torch.float32, device=w.device) if need_grad[3] else None
        need = _lib.token_pool_backward_workspace_bytes(w.shape[1], w.shape[0], cloud_off.numel() - 1, rows.shape[0])
        _lib.token_pool_backward_f32(rows, cloud_off, w, arg, dout.contiguous().float(), dx, dW, db, _ws(need, rows.device))
        return None, dx, None if dW is None else dW.reshape(weight.shape), db
