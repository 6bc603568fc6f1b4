"""PointNet++ building blocks on the HIP path: the two layer types the reference's `pointnet_2` class needs.

The reference imports `PointNetSetAbstraction` and `PointNetFeaturePropagation` from a package it does not ship (pointnetAtt.py:4,
used at :285-292).  This module provides both with the constructors and the state_dict keys of the usual PointNet++ implementation --
`mlp_convs.{i}.{weight, bias}` (weight [out, in, 1, 1] in the set abstraction, [out, in, 1] in the feature propagation),
`mlp_bns.{i}.{weight, bias, running_mean, running_var, num_batches_tracked}` -- so its checkpoints load.  Eval mode only:
  * PointNetSetAbstraction: farthest-point sampling (ampnet_fps_f32), ball query (ampnet_ball_query_f32) and ONE fused kernel for
    gather + shared MLP + max (ampnet_sa_forward_f32);
  * PointNetFeaturePropagation: the 3 nearest coarse points of every fine point (ampnet_three_nn_f32) and ONE fused kernel for
    inverse-distance interpolation + concatenation + shared MLP (ampnet_fp_forward_f32).
Both fused kernels are exact fp32 whatever the matrix precision is: the process-wide mode, a precision scope and AMPNET_PRECISION do
not reach these blocks.  The blocks' exact-bits contracts -- the multi-scale block equals its branches, a train-mode forward equals the
eval kernel on the batch's statistics, a backward finds the forward's ReLU masks and max again -- rest on that, so here precision=None
MEANS fp32 (for the other models it follows the library's default: a deliberate difference).

bf16 is opt-in and an inference mode: PointNetSetAbstraction(..., precision='bf16') and PointNetFeaturePropagation(..., precision='bf16')
(keyword-only; also set_precision(mode)) run the eval forward without a graph through ampnet_sa_forward_bf16 / ampnet_fp_forward_bf16:
the input rows, the weights and the hidden activations rounded to bf16, fp32 accumulation, BatchNorm and max (include/ampnet_hip.h, "the
rounding model").  Sampling, ball query, 3-NN and the interpolation weights are untouched, so the groups and neighbours are those of the
fp32 block.  A block built with grad=True, batch_stats=True or group_all=True refuses the mode (NotImplementedError) at construction and
in set_precision: a forward value never depends on whether a graph is wanted.  The other precision names of the package ('f32x3',
'bf16_train', 'bf16_store') are not built here and raise NotImplementedError.

Gradients are opt-in.  PointNetFeaturePropagation(..., grad=True) in EVAL mode is differentiable (ampnet_fp_backward_f32 through
autograd._FpFn) with respect to points1, points2, its conv weights and biases and its BatchNorm weight and bias;
PointNetSetAbstraction(..., grad=True) in EVAL mode is differentiable (ampnet_sa_backward_f32 through autograd._SaFn) with respect to
`points`, its conv weights and biases and its BatchNorm weight and bias, the max over the group sending each gradient to the lowest row
that attains it.  running_mean and running_var are constants of both backwards and are never updated, the coordinates get no gradient,
and farthest-point sampling, ball query and the gather of the centres run under no_grad.  That is what fitting a pretrained backbone to
new clouds needs (pointnetAtt.pointnet_2(decoder_grad=True, encoder_grad=True)).

Train-mode BatchNorm is opt-in too: PointNetFeaturePropagation(..., batch_stats=True) in TRAIN mode normalises with the statistics of
the batch (all B * N rows of the call), updates running_mean / running_var in place with each BatchNorm's `momentum` and counts
num_batches_tracked (ampnet_fp_train_forward_f32); with grad=True its backward goes through the statistics
(ampnet_fp_train_backward_f32 through autograd._FpTrainFn), as torch's does.  PointNetSetAbstraction(..., batch_stats=True) does the same
over all B * npoint * nsample rows of its groups -- the slots that ball query filled by repeating a group's first member are rows like any
other, as they are for BatchNorm2d over [B, C, nsample, npoint] (ampnet_sa_train_forward_f32, ampnet_sa_train_backward_f32 through
autograd._SaTrainFn).  In eval mode the flag changes nothing, and without it .train() still raises.

Clouds of UNEQUAL size packed back to back go through the blocks' _forward_ragged (pointnetAtt.pointnet_2_seg.forward_ragged): the ragged
searches write GLOBAL indices and the fused kernels above take the packed array as ONE cloud.  grad=True and batch_stats=True work there
as in _forward_rows -- the statistics over all rows of the call -- and the backward gathers the gradient of the features (set abstraction)
or of the coarse points (feature propagation) cloud by cloud (autograd._ragged_note; ampnet_*_backward_ragged_f32).

PointNetSetAbstraction(..., group_all=True) forms ONE group of all N points of a cloud, runs the shared MLP on [xyz, features] (the
coordinates as they are) and takes the max over the points: the global descriptor of a cloud (ampnet_sa_all_forward_f32).  Eval mode,
with grad=True the frozen-statistics backward (ampnet_sa_all_backward_f32 through autograd._SaAllFn), which runs on the rows that won a
channel and on nothing else.

PointNetSetAbstractionMsg is the multi-scale-grouping layer of the usual implementation (conv_blocks / bn_blocks): several (radius, nsample,
mlp) branches around the same centres, concatenated.  Farthest-point sampling runs once, one ball query fills all index lists
(ampnet_ball_query_msg_f32) and in eval mode one launch runs all branches (ampnet_sa_msg_forward_f32); grad=True and batch_stats=True go
branch by branch through the kernels above.  It serves models defined inside the set-abstraction limits (its docstring).

PointNetSegHead is the per-point classifier behind the backbone (conv1, bn1, ReLU, drop1, conv2, log_softmax): one fused kernel in eval
mode (ampnet_seg_head_forward_f32), with grad=True differentiable through ampnet_seg_head_backward_f32 (its docstring;
pointnetAtt.pointnet_2_seg puts it behind pointnet_2's six blocks); batch_stats=True adds train mode -- bn1 on batch statistics and a real
dropout (ampnet_seg_head_train_forward_f32, ampnet_seg_head_train_backward_f32).  Its bf16 and a loss fused into its kernel are not built;
seg_nll_loss is the loss BEHIND it: masked, weighted NLL, predictions and confusion counts in one pass over the log-probabilities
(ampnet_seg_nll_forward_f32, ampnet_seg_nll_backward_f32 through autograd._SegNllFn).
Not built: momentum=None, gradients to coordinates, train-mode BatchNorm (batch_stats=True) in a `group_all=True` block, a `precision`
keyword for PointNetSetAbstractionMsg (its one-launch forward is fp32 only), bf16 in a backward, a train-mode or a group_all forward.

Differences from the usual implementation: its farthest-point sampling starts from a RANDOM point of each cloud; here the centres come
from the project's `fps_indices`, whose seed is point 0 (the rule of the reference's utils.fps).  Pass `centres=` to use other ones.
Its feature propagation finds the 3 neighbours by sorting a `-2 x.y + |x|^2 + |y|^2` matrix, so its choice among NEARLY equal neighbours
depends on the library; here the distance is float32 ((dx*dx + dy*dy) + dz*dz) and equal distances go to the lower index
(utils.three_nn).
"""
import torch
import torch.nn as nn

from ... import _lib
from ...utils import utils as U
from ._precision import _EvalForwardPrecision, is_bf16


class _Conv(nn.Module):
    """Holder with the parameter names, shapes and initialisation bounds of nn.Conv2d(cin, cout, 1) (tail = (1, 1)) or nn.Conv1d(cin, cout, 1)
    (tail = (1,))."""

    def __init__(self, cin, cout, tail, device):
        super().__init__()
        k = 1.0 / cin ** 0.5
        self.weight = nn.Parameter(torch.empty(cout, cin, *tail, device=device).uniform_(-k, k))
        self.bias = nn.Parameter(torch.empty(cout, device=device).uniform_(-k, k))


class _BN2d(nn.Module):
    """Holder with nn.BatchNorm2d's parameter and buffer names."""

    def __init__(self, c, device, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.momentum = 0.1                       # (an attribute, not a state_dict key; used by the batch_stats=True blocks in train mode)
        self.weight = nn.Parameter(torch.ones(c, device=device))
        self.bias = nn.Parameter(torch.zeros(c, device=device))
        self.register_buffer("running_mean", torch.zeros(c, device=device))
        self.register_buffer("running_var", torch.ones(c, device=device))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long, device=device))


assert (_lib.SA_MAX_LAYERS, _lib.SA_MAX_COUT) == (_lib.FP_MAX_LAYERS, _lib.FP_MAX_COUT)     # _build_mlp checks one pair for both layers


def _build_mlp(mod, in_channel, mlp, tail, ok, limits, device):
    """Sets mod.in_channel, mod.mlp_convs and mod.mlp_bns (BatchNorm1d has BatchNorm2d's names and shapes) for the widths `mlp`; `ok` is the layer's own limit check and `limits` the sentence that names every limit."""
    mlp = [int(c) for c in mlp]
    if not (1 <= len(mlp) <= _lib.SA_MAX_LAYERS) or any(c % 32 or not 32 <= c <= _lib.SA_MAX_COUT for c in mlp) or not ok:
        raise NotImplementedError(limits)
    mod.in_channel = int(in_channel)
    mod.mlp_convs, mod.mlp_bns = nn.ModuleList(), nn.ModuleList()
    last = mod.in_channel
    for c in mlp:
        mod.mlp_convs.append(_Conv(last, c, tail, device))
        mod.mlp_bns.append(_BN2d(c, device))
        last = c
    mod._ws = None


def _workspace(mod, nbytes, device):
    """The module's workspace (the BatchNorm fold; in bf16 mode also the converted weights), allocated on first use and again when the
    input moves to another device or a call needs more than the buffer holds."""
    if mod._ws is None or mod._ws.device != device or mod._ws.numel() < nbytes:
        mod._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return mod._ws


def _mlp_tensors(mod, live_stats=False, w0=None):
    """Per layer the six contiguous float32 tensors the fused kernels take: weight [cout, cin], conv bias, BatchNorm weight, bias,
    running_mean, running_var -- the statistics as float32 copies (eval: they are read) or, with live_stats, the module's buffers
    themselves (train: the forward updates them in place).  w0: what stands in for layer 0's conv weight (autograd._block_tensors)."""
    from ... import autograd as A
    if not live_stats:
        return A._mlp_layers(A._block_tensors(mod, w0=w0), 6)
    return [layer + (bn.running_mean, bn.running_var)
            for layer, bn in zip(A._mlp_layers(A._block_tensors(mod, stats=False, w0=w0), 4), mod.mlp_bns)]


def _momentum(mod, what):
    """The one float momentum of the block's BatchNorms (train mode)."""
    momenta = {bn.momentum for bn in mod.mlp_bns}
    if None in momenta or len(momenta) != 1:
        raise NotImplementedError(f"train-mode {what} takes one float momentum for the block's BatchNorms, got "
                                  f"{[bn.momentum for bn in mod.mlp_bns]} (momentum=None, the cumulative average, is not built)")
    return float(momenta.pop())


def _count_batch(mod):
    with torch.no_grad():
        torch._foreach_add_([bn.num_batches_tracked for bn in mod.mlp_bns], 1)


_SA_EVAL_ONLY = "the HIP set abstraction is built for eval mode (BatchNorm running statistics, no backward): call .eval() first"


class _SetAbstraction(nn.Module):
    """What PointNetSetAbstraction and PointNetSetAbstractionMsg share: the channel-major interface around _forward_rows and the centres
    of a block.  The class name opens the messages; D, the width of `points`, is the caller's (in_channel counts the coordinates in one
    class and not in the other)."""

    def _forward_channel_major(self, xyz, points, centres, D):
        """forward() of both classes: the shape checks, the transposes to point-major rows and back, with or without a graph."""
        if self.training and not self.batch_stats:
            raise NotImplementedError(_SA_EVAL_ONLY)
        name = type(self).__name__
        _lib.require_gpu(xyz, "xyz")
        if xyz.dim() != 3 or xyz.shape[1] != 3:
            raise _lib.AmpnetError(f"{name}: expected xyz [B, 3, N], got {tuple(xyz.shape)}")
        B, _, N = xyz.shape
        if (points is None) != (D == 0) or (points is not None and (points.dim() != 3 or tuple(points.shape) != (B, D, N))):
            raise _lib.AmpnetError(f"{name}: in_channel={self.in_channel} needs points "
                                   f"{'None' if D == 0 else [B, D, N]}, got {None if points is None else tuple(points.shape)}")
        if points is not None:
            _lib.require_gpu(points, "points")
        rows = lambda t: None if t is None else t.float().transpose(1, 2).contiguous()       # [B, N, 3], [B, N, D]
        if self._wants_grad(points):                                 # a differentiable transpose; the coordinates get no gradient
            new_xyz, out = self._forward_rows(rows(xyz.detach()), rows(points), centres)
        else:
            with torch.no_grad():
                new_xyz, out = self._forward_rows(rows(xyz), rows(points), centres)
        return new_xyz.transpose(1, 2).contiguous(), out.transpose(1, 2).contiguous()

    def _wants_grad(self, feats):
        return self.grad and torch.is_grad_enabled() and ((feats is not None and feats.requires_grad)
                                                          or any(p.requires_grad for p in self.parameters()))

    def _sample_and_group(self, x, centres, query):
        """The centres of x [B, N, 3] (`centres`, or farthest-point sampling from point 0) and what query(x, centres), the class's ball
        query, finds around them -> (x detached, centres, the query's result, new_xyz [B, npoint, 3]).  The query validates the centres,
        so it runs before the gather."""
        with torch.no_grad():
            x = x.detach()
            if centres is None:
                centres = U.fps_indices(x, self.npoint)
            elif centres.dim() != 2 or tuple(centres.shape) != (x.shape[0], self.npoint):
                raise _lib.AmpnetError(f"{type(self).__name__}: centres must be [B, npoint] = {[x.shape[0], self.npoint]}, "
                                       f"got {tuple(centres.shape)}")
            groups = query(x, centres)
            centres = centres.contiguous()
            return x, centres, groups, U.gather_rows(x, centres)


class PointNetSetAbstraction(_EvalForwardPrecision, _SetAbstraction):
    """One set-abstraction layer: `npoint` centres by farthest-point sampling, per centre the first `nsample` points within `radius`
    (utils.ball_query), the shared MLP `mlp` (Conv2d 1x1 + BatchNorm2d + ReLU per entry) on [relative xyz, point features], max over the
    group.  `in_channel` counts the 3 coordinates, as in the usual implementation.
    grad=True: in eval mode, with grad mode on and `points` or a parameter that requires grad, new_points carries a graph to `points` and
    the conv / BatchNorm affine parameters (the running statistics stay frozen; new_xyz never carries one).  grad=False (default): no
    graph, ever.
    batch_stats=False (default): eval mode only, the running statistics frozen; train mode raises.  batch_stats=True: train mode is
    accepted and runs BatchNorm on the statistics of all B * npoint * nsample rows, updating running_mean / running_var (momentum: the
    `momentum` attribute of the block's mlp_bns, one value for the block) and num_batches_tracked once per forward, graph or not; with
    grad=True the backward goes through the statistics; eval mode is unchanged.
    group_all=True: ONE group of all N points per cloud, the coordinates as they are (the usual sample_and_group_all): npoint, radius and
    nsample are ignored and may be None, new_xyz is zeros [B, 3, 1] and new_points [B, mlp[-1], 1] (ampnet_sa_all_forward_f32); grad=True
    works as above (ampnet_sa_all_backward_f32 through autograd._SaAllFn: only the rows that won a channel carry a gradient);
    `centres=` raises and batch_stats=True is refused at construction.
    precision (keyword-only; set_precision(mode)): None or 'fp32' -- the exact-fp32 kernel, whatever the library's mode is; 'bf16' -- the
    eval forward without a graph through ampnet_sa_forward_bf16 (the module docstring), refused together with grad=True, batch_stats=True
    or group_all=True."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all, device='cuda', grad=False, batch_stats=False, *, precision=None):
        super().__init__()
        self.grad = bool(grad)
        self.batch_stats = bool(batch_stats)
        self.group_all = bool(group_all)
        self.set_precision(precision)
        if group_all:
            if self.batch_stats:
                raise NotImplementedError("group_all=True is built for eval mode (with grad=True: the running statistics frozen); train mode "
                                          "-- batch_stats=True, BatchNorm over the B * N rows of the whole-cloud group -- is not")
            _build_mlp(self, in_channel, mlp, (1, 1), 3 <= in_channel <= _lib.SA_MAX_CIN,
                       f"the HIP set abstraction with group_all=True is built for 1..{_lib.SA_MAX_LAYERS} MLP layers of widths that are "
                       f"multiples of 32 up to {_lib.SA_MAX_COUT} and 3 <= in_channel <= {_lib.SA_MAX_CIN}", device)
            self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, True      # (ignored; they may be None)
            return
        _build_mlp(self, in_channel, mlp, (1, 1), 3 <= in_channel <= _lib.SA_MAX_CIN and 1 <= nsample <= _lib.SA_MAX_NSAMPLE,
                   f"the HIP set abstraction is built for 1..{_lib.SA_MAX_LAYERS} MLP layers of widths that are multiples "
                   f"of 32 up to {_lib.SA_MAX_COUT}, 3 <= in_channel <= {_lib.SA_MAX_CIN}, nsample <= {_lib.SA_MAX_NSAMPLE}", device)
        self.npoint, self.radius, self.nsample, self.group_all = int(npoint), float(radius), int(nsample), False

    def _bf16_refusal(self):
        flags = [f for f in ("grad", "batch_stats", "group_all") if getattr(self, f)]
        return f"this block was built with {', '.join(f + '=True' for f in flags)}" if flags else None

    def forward(self, xyz, points, centres=None):
        """xyz [B, 3, N], points [B, D, N] or None (D = in_channel - 3) -> (new_xyz [B, 3, npoint], new_points [B, mlp[-1], npoint]);
        npoint counts as 1 in a group_all block.  centres: int32 [B, npoint] point indices to use instead of farthest-point sampling
        from point 0."""
        return self._forward_channel_major(xyz, points, centres, self.in_channel - 3)

    def _forward_rows(self, x, feats, centres=None):
        """The layer on point-major tensors (what the kernels take): x [B, N, 3], feats [B, N, D] or None, float32 contiguous GPU
        -> (new_xyz [B, npoint, 3], new_points [B, npoint, mlp[-1]]).  pointnet_2 chains its blocks through this, without the transpose
        pair per block that forward() owes to the channel-major interface."""
        self._check_bf16()
        if self.group_all:
            return self._all_rows(x, feats, centres)
        B = x.shape[0]
        x, centres, group_idx, new_xyz = self._sample_and_group(x, centres, lambda x, c: U.ball_query(x, c, self.radius, self.nsample))
        if self.training:
            return new_xyz, self._train_rows(x, centres, group_idx, feats)
        if self._wants_grad(feats):
            from ... import autograd
            return new_xyz, autograd.sa_apply(self, x, centres, group_idx, feats, _workspace(self, _lib.SA_WORKSPACE_BYTES, x.device))
        feats = None if feats is None else feats.detach()
        layers = _mlp_tensors(self)
        out = torch.empty((B, self.npoint, layers[-1][0].shape[0]), dtype=torch.float32, device=x.device)
        if is_bf16(self.precision):
            need = _lib.sa_forward_bf16_workspace_bytes(self.in_channel - 3, B, self.npoint, self.nsample, [w.shape[0] for w, *_ in layers])
            _lib.sa_forward_bf16(x, centres, group_idx, feats, layers, [bn.eps for bn in self.mlp_bns], out, _workspace(self, need, x.device))
        else:
            _lib.sa_forward_f32(x, centres, group_idx, feats, layers, [bn.eps for bn in self.mlp_bns], out,
                                _workspace(self, _lib.SA_WORKSPACE_BYTES, x.device))
        return new_xyz, out

    def _forward_ragged(self, x, feats, layout):
        """The layer on clouds of UNEQUAL size packed back to back: x [total, 3], feats [total, D] or None, float32 contiguous GPU,
        layout = utils.RaggedLayout of the clouds, every one of >= npoint points -> (new_xyz [Q, npoint, 3], new_points [Q, npoint, mlp[-1]]),
        in eval mode cloud by cloud the bits of _forward_rows on that cloud alone.  Ragged FPS, then the ragged ball query with GLOBAL
        indices, then the fused kernel of _forward_rows on the packed array as ONE cloud of `total` points and Q * npoint centres: a
        centre's row of the output depends on its own group and the weights alone (csrc/set_abstraction.hip: a wave owns a centre, a fixed
        contraction order, no atomics), so which launch it shares is immaterial.  No host read-back (the centres are FPS's own).
        A default block: eval mode, no graph.  grad=True: a graph when _wants_grad says so, to `feats` and the parameters; its backward
        gathers dfeats cloud by cloud (autograd._ragged_note).  batch_stats=True in train mode: the train-mode layer of _train_rows on the
        packed array -- the statistics over all Q * npoint * nsample rows, what _forward_rows takes over B = Q equal clouds -- the buffers
        updated and num_batches_tracked counted once.  group_all and bf16 are refused."""
        self._check_bf16()
        if self.group_all or (self.training and not self.batch_stats) or is_bf16(self.precision):
            raise NotImplementedError("PointNetSetAbstraction._forward_ragged is built for the exact-fp32 eval forward of a grouping block "
                                      "(group_all=False, .eval(), precision fp32); train mode needs a block built with batch_stats=True")
        Q, S = len(layout.sizes), self.npoint
        if min(layout.sizes) < S:
            raise _lib.AmpnetError(f"PointNetSetAbstraction: every cloud needs at least npoint={S} points for farthest-point sampling, "
                                   f"got sizes {layout.sizes}")
        with torch.no_grad():
            x = x.detach()
            centres = torch.stack(U.fps_indices_ragged(x, layout.sizes, S))                       # [Q, npoint], relative to their cloud
            group_idx = U.ball_query_ragged(x, layout, centres, self.radius, self.nsample, global_index=True, _trusted_centres=True)
            centres = (centres + layout.off[:-1].unsqueeze(1)).reshape(1, Q * S)                  # rows of the packed array
            group_idx = group_idx.reshape(1, Q * S, self.nsample)
            packed = x.unsqueeze(0)
            new_xyz = U.gather_rows(packed, centres).reshape(Q, S, 3)
        packed_feats = None if feats is None else feats.unsqueeze(0)                              # (a view: the graph goes through it)
        if self.training:
            out = self._train_rows(packed, centres, group_idx, packed_feats, cloud_off=layout.off)
        elif self._wants_grad(feats):
            from ... import autograd
            out = autograd.sa_apply(self, packed, centres, group_idx, packed_feats, _workspace(self, _lib.SA_WORKSPACE_BYTES, x.device),
                                    cloud_off=layout.off)
        else:
            with torch.no_grad():
                layers = _mlp_tensors(self)
                out = torch.empty((1, Q * S, layers[-1][0].shape[0]), dtype=torch.float32, device=x.device)
                _lib.sa_forward_f32(packed, centres, group_idx, None if feats is None else packed_feats.detach(), layers,
                                    [bn.eps for bn in self.mlp_bns], out, _workspace(self, _lib.SA_WORKSPACE_BYTES, x.device))
        return new_xyz, out.reshape(Q, S, -1)

    def _all_rows(self, x, feats, centres):
        """_forward_rows of a group_all block: ONE group of all N points per cloud, the coordinates as they are (no centre)
        -> (zeros [B, 1, 3], [B, 1, mlp[-1]])."""
        if centres is not None:
            raise _lib.AmpnetError("PointNetSetAbstraction: group_all=True has no centres (one group of all points, new_xyz is the origin)")
        if self.training:
            raise NotImplementedError(_SA_EVAL_ONLY)
        from ... import autograd
        x = x.detach()
        new_xyz = torch.zeros((x.shape[0], 1, 3), dtype=torch.float32, device=x.device)
        if self._wants_grad(feats):
            return new_xyz, autograd.sa_all_apply(self, x, feats).unsqueeze(1)
        with torch.no_grad():
            out, _ = autograd.sa_all_forward(x, None if feats is None else feats.detach(), _mlp_tensors(self), [bn.eps for bn in self.mlp_bns])
        return new_xyz, out.unsqueeze(1)

    def _train_rows(self, x, centres, group_idx, feats, cloud_off=None):
        """The fused layer of _forward_rows in train mode (batch_stats=True): batch statistics, the buffers updated in place, a graph when
        one is wanted.  cloud_off: autograd._ragged_note (_forward_ragged)."""
        if not self.batch_stats:
            raise NotImplementedError(_SA_EVAL_ONLY)
        momentum = _momentum(self, "set abstraction")
        from ... import autograd
        if self._wants_grad(feats):
            out = autograd.sa_train_apply(self, x, centres, group_idx, feats, momentum, cloud_off=cloud_off)
        else:
            with torch.no_grad():
                out, _, _ = autograd.sa_train_forward(x, centres, group_idx, None if feats is None else feats.detach(),
                                                      _mlp_tensors(self, live_stats=True), [bn.eps for bn in self.mlp_bns], momentum)
        _count_batch(self)
        return out


class _Branch:
    """One branch of a PointNetSetAbstractionMsg as _build_mlp lays a block out (mlp_convs, mlp_bns): what the helpers of the single-scale
    blocks take.  Not a Module and never kept: the owner registers the two lists under the usual implementation's names (conv_blocks[i],
    bn_blocks[i]) and makes a view of them per call."""

    def __init__(self, mlp_convs=None, mlp_bns=None):
        self.mlp_convs, self.mlp_bns = mlp_convs, mlp_bns


class _Bns:
    """All BatchNorms of a PointNetSetAbstractionMsg as one block's mlp_bns, for the rules that cover the module (_momentum, _count_batch)."""

    def __init__(self, branches):
        self.mlp_bns = [bn for b in branches for bn in b.mlp_bns]


class PointNetSetAbstractionMsg(_SetAbstraction):
    """One multi-scale-grouping set-abstraction layer: `npoint` centres by farthest-point sampling, and for every (radius, nsample, mlp) of
    radius_list, nsample_list and mlp_list a branch that groups the first `nsample` points within `radius` of each centre
    (utils.ball_query_msg: all radii in one pass), runs its shared MLP (Conv2d 1x1 + BatchNorm2d + ReLU per entry) on the group and takes
    the max; new_points is the branches' outputs concatenated in list order.  Constructor, attribute names and state_dict keys are the usual
    implementation's -- conv_blocks.{i}.{j}.{weight [out, in, 1, 1], bias}, bn_blocks.{i}.{j}.{weight, bias, running_mean, running_var,
    num_batches_tracked} -- so checkpoints are exchanged with a torch model.
    `in_channel` does NOT count the 3 coordinates here (layer 0 of every branch has in = in_channel + 3); PointNetSetAbstraction's does.
    That difference is the usual implementation's own.
    Row order: the usual MSG row is [point features (D), relative xyz (3)], features FIRST ([relative xyz] alone when points is None);
    the kernels take [relative xyz, features].  The module hands them layer 0's weight with its columns rotated
    (cat(W[:, D:], W[:, :D])): the checkpoint keeps the usual order, and with grad=True the rotation is a differentiable op, so layer 0's
    weight gradient arrives in the checkpoint's column order.
    Eval mode without a graph: ONE launch for all branches (ampnet_sa_msg_forward_f32), each branch writing its column slice.
    grad=True (eval mode): branch by branch through autograd._SaFn on the shared centres, concatenated; the value equals the fused
    forward's bit for bit, and the gradient to `points` is the sum over the branches.  batch_stats=True (train mode): branch by branch
    through ampnet_sa_train_forward_f32 / autograd._SaTrainFn, each branch with its own statistics over its B * npoint * nsample_k rows
    and its running statistics updated in place; num_batches_tracked goes up once per forward; one float momentum covers the module.
    Without the flag .train() raises.  grad and batch_stats otherwise as in PointNetSetAbstraction.
    Limits: 1..SA_MSG_MAX_SCALES branches, each within the set-abstraction limits (1..3 layers, widths multiples of 32 up to 256,
    in_channel + 3 <= 320, nsample <= 64).  This block serves models DEFINED inside those limits: the stock MSG segmentation model's
    widths 16, 196, 384 and 512 are outside them and are refused, not approximated.  Not built: group_all or k-NN grouping inside this
    block, a fused multi-branch backward or train path."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list, device='cuda', grad=False, batch_stats=False):
        super().__init__()
        self.grad = bool(grad)
        self.batch_stats = bool(batch_stats)
        radius_list, nsample_list, mlp_list = list(radius_list), list(nsample_list), list(mlp_list)
        K = len(radius_list)
        limits = (f"the HIP multi-scale set abstraction is built for radius_list, nsample_list and mlp_list of one length in "
                  f"1..{_lib.SA_MSG_MAX_SCALES}, every branch with 1..{_lib.SA_MAX_LAYERS} MLP layers of widths that are multiples of 32 up to "
                  f"{_lib.SA_MAX_COUT}, 0 <= in_channel and in_channel + 3 <= {_lib.SA_MAX_CIN}, nsample <= {_lib.SA_MAX_NSAMPLE}")
        if len(nsample_list) != K or len(mlp_list) != K or not 1 <= K <= _lib.SA_MSG_MAX_SCALES:
            raise NotImplementedError(limits)
        self.npoint, self.in_channel = int(npoint), int(in_channel)
        self.radius_list, self.nsample_list = [float(r) for r in radius_list], [int(ns) for ns in nsample_list]
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for nsample, mlp in zip(self.nsample_list, mlp_list):
            b = _Branch()
            _build_mlp(b, self.in_channel + 3, mlp, (1, 1), 3 <= self.in_channel + 3 <= _lib.SA_MAX_CIN and 1 <= nsample <= _lib.SA_MAX_NSAMPLE,
                       limits, device)
            self.conv_blocks.append(b.mlp_convs)
            self.bn_blocks.append(b.mlp_bns)
        self._ws = None

    @property
    def _branches(self):
        return [_Branch(convs, bns) for convs, bns in zip(self.conv_blocks, self.bn_blocks)]

    def forward(self, xyz, points, centres=None):
        """xyz [B, 3, N], points [B, D, N] or None (D = in_channel) -> (new_xyz [B, 3, npoint], new_points [B, sum of the branches' last
        widths, npoint]).  centres: int32 [B, npoint] point indices to use instead of farthest-point sampling from point 0."""
        return self._forward_channel_major(xyz, points, centres, self.in_channel)

    def _w0(self, b):
        """Layer 0's weight of branch b as the kernels take it: the checkpoint's columns [features (D), xyz (3)] rotated to [xyz, features]."""
        D, w = self.in_channel, b.mlp_convs[0].weight
        return None if D == 0 else torch.cat((w[:, D:], w[:, :D]), dim=1)

    def _forward_rows(self, x, feats, centres=None):
        """The layer on point-major tensors (what the kernels take): x [B, N, 3], feats [B, N, D] or None, float32 contiguous GPU
        -> (new_xyz [B, npoint, 3], new_points [B, npoint, sum of the branches' last widths]).  Farthest-point sampling and the ball
        query at all radii run once."""
        B, K = x.shape[0], len(self._branches)
        x, centres, group_idxs, new_xyz = self._sample_and_group(
            x, centres, lambda x, c: U.ball_query_msg(x, c, self.radius_list, self.nsample_list))
        wants_grad = self._wants_grad(feats)
        if self.training:
            return new_xyz, self._train_rows(x, centres, group_idxs, feats, wants_grad)
        ws = _workspace(self, _lib.sa_msg_forward_workspace_bytes(K), x.device)
        if wants_grad:                                               # K launches of the single-branch kernel, each with its own fold region
            from ... import autograd
            step = _lib.SA_WORKSPACE_BYTES
            return new_xyz, torch.cat([autograd.sa_apply(b, x, centres, g, feats, ws[k * step:(k + 1) * step], w0=self._w0(b))
                                       for k, (b, g) in enumerate(zip(self._branches, group_idxs))], dim=2)
        feats = None if feats is None else feats.detach()
        branches = [_mlp_tensors(b, w0=self._w0(b)) for b in self._branches]
        out = torch.empty((B, self.npoint, sum(layers[-1][0].shape[0] for layers in branches)), dtype=torch.float32, device=x.device)
        _lib.sa_msg_forward_f32(x, centres, group_idxs, feats, branches, [[bn.eps for bn in b.mlp_bns] for b in self._branches], out, ws)
        return new_xyz, out

    def _train_rows(self, x, centres, group_idxs, feats, wants_grad):
        """_forward_rows in train mode (batch_stats=True): every branch on its own batch statistics, its buffers updated in place, a graph
        when one is wanted; the launches are those of K PointNetSetAbstraction blocks in train mode."""
        if not self.batch_stats:
            raise NotImplementedError(_SA_EVAL_ONLY)
        every = _Bns(self._branches)
        momentum = _momentum(every, "multi-scale set abstraction")
        from ... import autograd
        outs = []
        for b, g in zip(self._branches, group_idxs):
            if wants_grad:
                outs.append(autograd.sa_train_apply(b, x, centres, g, feats, momentum, w0=self._w0(b)))
            else:
                with torch.no_grad():
                    outs.append(autograd.sa_train_forward(x, centres, g, None if feats is None else feats.detach(),
                                                          _mlp_tensors(b, live_stats=True, w0=self._w0(b)), [bn.eps for bn in b.mlp_bns],
                                                          momentum)[0])
        _count_batch(every)
        return torch.cat(outs, dim=2)


_FP_EVAL_ONLY = ("the HIP feature propagation is built for eval mode (BatchNorm running statistics, no backward): call .eval() first, "
                 "or build the block with batch_stats=True")


class PointNetFeaturePropagation(_EvalForwardPrecision, nn.Module):
    """One feature-propagation layer: every fine point takes the inverse-squared-distance weighted mean of the features of its 3 nearest
    coarse points (utils.three_nn; all of them when there are fewer than 3), concatenated behind its own features, through the shared MLP
    `mlp` (Conv1d 1x1 + BatchNorm1d + ReLU per entry).  `in_channel` = D1 + D2, as in the usual implementation.
    grad=True: with grad mode on and an input or a parameter that requires grad, the result carries a graph to points1, points2 and the
    conv / BatchNorm affine parameters.  grad=False (default): no graph, ever.
    batch_stats=False (default): eval mode only, the running statistics frozen; train mode raises.  batch_stats=True: train mode is
    accepted and runs BatchNorm on the batch's statistics, updating running_mean / running_var (momentum: the `momentum` attribute of the
    block's mlp_bns, one value for the block) and num_batches_tracked once per forward, graph or not; eval mode is unchanged.
    precision (keyword-only; set_precision(mode)): None or 'fp32' -- the exact-fp32 kernel, whatever the library's mode is; 'bf16' -- the
    eval forward without a graph through ampnet_fp_forward_bf16 (the module docstring), refused together with grad=True or
    batch_stats=True."""

    def __init__(self, in_channel, mlp, device='cuda', grad=False, batch_stats=False, *, precision=None):
        super().__init__()
        self.grad = bool(grad)
        self.batch_stats = bool(batch_stats)
        self.set_precision(precision)
        _build_mlp(self, in_channel, mlp, (1,), 1 <= in_channel <= _lib.FP_MAX_CIN,
                   f"the HIP feature propagation is built for 1..{_lib.FP_MAX_LAYERS} MLP layers of widths that are "
                   f"multiples of 32 up to {_lib.FP_MAX_COUT} and 1 <= in_channel <= {_lib.FP_MAX_CIN}", device)

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 [B, 3, N] the fine points, xyz2 [B, 3, S] the coarse ones, points1 [B, D1, N] or None, points2 [B, D2, S]
        (D1 + D2 = in_channel) -> new_points [B, mlp[-1], N]."""
        if self.training and not self.batch_stats:
            raise NotImplementedError(_FP_EVAL_ONLY)
        for name, t in (("xyz1", xyz1), ("xyz2", xyz2), ("points1", points1), ("points2", points2)):
            if t is not None:
                _lib.require_gpu(t, name)
        if xyz1.dim() != 3 or xyz1.shape[1] != 3 or xyz2.dim() != 3 or xyz2.shape[1] != 3 or xyz2.shape[0] != xyz1.shape[0]:
            raise _lib.AmpnetError(f"PointNetFeaturePropagation: expected xyz1 [B, 3, N] and xyz2 [B, 3, S], got {tuple(xyz1.shape)} "
                                   f"{tuple(xyz2.shape)}")
        B, _, N = xyz1.shape
        S = xyz2.shape[2]
        if points2 is None or points2.dim() != 3 or points2.shape[0] != B or points2.shape[2] != S:
            raise _lib.AmpnetError(f"PointNetFeaturePropagation: points2 must be [B, D2, S] = [{B}, D2, {S}], got "
                                   f"{None if points2 is None else tuple(points2.shape)}")
        D1 = self.in_channel - points2.shape[1]
        if D1 < 0 or (points1 is None) != (D1 == 0) or (points1 is not None and tuple(points1.shape) != (B, D1, N)):
            raise _lib.AmpnetError(f"PointNetFeaturePropagation: in_channel={self.in_channel} with points2 {tuple(points2.shape)} needs "
                                   f"points1 {'None' if D1 == 0 else [B, D1, N]}, got {None if points1 is None else tuple(points1.shape)}")
        if self._wants_grad(points1, points2):                       # differentiable transposes; the coordinates get no gradient
            rows = lambda t: None if t is None else t.float().transpose(1, 2).contiguous()
            out = self._forward_rows(rows(xyz1.detach()), rows(xyz2.detach()), rows(points1), rows(points2))
            return out.transpose(1, 2).contiguous()
        with torch.no_grad():
            rows = lambda t: None if t is None else t.detach().float().transpose(1, 2).contiguous()
            out = self._forward_rows(rows(xyz1), rows(xyz2), rows(points1), rows(points2))
        return out.transpose(1, 2).contiguous()

    def _bf16_refusal(self):
        flags = [f for f in ("grad", "batch_stats") if getattr(self, f)]
        return f"this block was built with {', '.join(f + '=True' for f in flags)}" if flags else None

    def _wants_grad(self, p1, p2):
        return self.grad and torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in (p1, p2))
                                                          or any(p.requires_grad for p in self.parameters()))

    def _forward_rows(self, x1, x2, p1, p2):
        """The layer on point-major tensors: x1 [B, N, 3], x2 [B, S, 3], p1 [B, N, D1] or None, p2 [B, S, D2], float32 contiguous GPU
        -> [B, N, mlp[-1]]."""
        self._check_bf16()
        idx, dist2 = U.three_nn(x1.detach(), x2.detach())
        if self.training:
            return self._train_rows(p1, p2, idx, dist2)
        if self._wants_grad(p1, p2):
            from ... import autograd
            return autograd.fp_apply(self, p1, p2, idx, dist2, _workspace(self, _lib.FP_WORKSPACE_BYTES, x1.device))
        layers = _mlp_tensors(self)
        out = torch.empty((x1.shape[0], x1.shape[1], layers[-1][0].shape[0]), dtype=torch.float32, device=x1.device)
        if is_bf16(self.precision):
            need = _lib.fp_forward_bf16_workspace_bytes(0 if p1 is None else p1.shape[2], p2.shape[2], x1.shape[0], x1.shape[1],
                                                        [w.shape[0] for w, *_ in layers])
            _lib.fp_forward_bf16(p1, p2, idx, dist2, layers, [bn.eps for bn in self.mlp_bns], out, _workspace(self, need, x1.device))
        else:
            _lib.fp_forward_f32(p1, p2, idx, dist2, layers, [bn.eps for bn in self.mlp_bns], out,
                                _workspace(self, _lib.FP_WORKSPACE_BYTES, x1.device))
        return out

    def _forward_ragged(self, x1, layout, x2, p1, p2):
        """The layer from fine clouds of UNEQUAL size packed back to back to S coarse points per cloud: x1 [total, 3], p1 [total, D1] or
        None, layout = utils.RaggedLayout of the fine clouds, x2 [Q, S, 3], p2 [Q, S, D2], float32 contiguous GPU -> [total, mlp[-1]], in
        eval mode cloud by cloud the bits of _forward_rows on that cloud alone.  The ragged 3-NN with GLOBAL indices, then the fused kernel
        of _forward_rows on the packed arrays as ONE cloud (total fine, Q * S coarse points): a fine point's output row depends on its own
        input row and the weights alone (csrc/feature_propagation.hip: the rows of a tile do not mix, a fixed contraction order, no
        atomics), so where the tile boundaries fall is immaterial.
        A default block: eval mode, no graph.  grad=True: a graph when _wants_grad says so, to p1, p2 and the parameters; its backward
        gathers dp2 cloud by cloud (autograd._ragged_note).  batch_stats=True in train mode: the train-mode layer of _train_rows on the
        packed arrays, the statistics over all `total` rows, the buffers updated and num_batches_tracked counted once.  bf16 is refused."""
        self._check_bf16()
        if (self.training and not self.batch_stats) or is_bf16(self.precision):
            raise NotImplementedError("PointNetFeaturePropagation._forward_ragged is built for the exact-fp32 eval forward (.eval(), "
                                      "precision fp32); train mode needs a block built with batch_stats=True")
        Q, S = x2.shape[0], x2.shape[1]
        with torch.no_grad():
            idx, dist2 = U.three_nn_ragged(x1.detach(), layout, x2.detach(), global_index=True)
            idx, dist2 = idx.unsqueeze(0), dist2.unsqueeze(0)
        packed1 = None if p1 is None else p1.unsqueeze(0)                                          # (views: the graph goes through them)
        packed2 = p2.reshape(1, Q * S, p2.shape[2])
        if self.training:
            return self._train_rows(packed1, packed2, idx, dist2, cloud_off=layout.off)[0]
        if self._wants_grad(p1, p2):
            from ... import autograd
            return autograd.fp_apply(self, packed1, packed2, idx, dist2, _workspace(self, _lib.FP_WORKSPACE_BYTES, x1.device),
                                     cloud_off=layout.off)[0]
        with torch.no_grad():
            layers = _mlp_tensors(self)
            out = torch.empty((1, layout.total, layers[-1][0].shape[0]), dtype=torch.float32, device=x1.device)
            _lib.fp_forward_f32(None if p1 is None else packed1.detach(), packed2.detach(), idx, dist2, layers, [bn.eps for bn in self.mlp_bns],
                                out, _workspace(self, _lib.FP_WORKSPACE_BYTES, x1.device))
        return out[0]

    def _train_rows(self, p1, p2, idx, dist2, cloud_off=None):
        """_forward_rows in train mode (batch_stats=True): batch statistics, the buffers updated in place, a graph when one is wanted.
        cloud_off: autograd._ragged_note (_forward_ragged)."""
        if not self.batch_stats:
            raise NotImplementedError(_FP_EVAL_ONLY)
        momentum = _momentum(self, "feature propagation")
        from ... import autograd
        if self._wants_grad(p1, p2):
            out = autograd.fp_train_apply(self, p1, p2, idx, dist2, momentum, cloud_off=cloud_off)
        else:
            with torch.no_grad():
                out, _, _ = autograd.fp_train_forward(None if p1 is None else p1.detach(), p2.detach(), idx, dist2,
                                                      _mlp_tensors(self, live_stats=True), [bn.eps for bn in self.mlp_bns], momentum)
        _count_batch(self)
        return out


_SEG_EVAL_ONLY = ("the HIP segmentation head is built for eval mode (bn1 on its running statistics, dropout the identity): call .eval() "
                  "first, or build the head with batch_stats=True")


class PointNetSegHead(nn.Module):
    """The per-point classifier of the usual PointNet++ semantic-segmentation model -- conv1 (Conv1d 1x1), bn1, ReLU, drop1, conv2 (Conv1d
    1x1), log_softmax over the classes, permute -- the lines the reference's pointnet_2 carries commented out (pointnetAtt.py:294-296,
    :318-321), as ONE fused kernel (ampnet_seg_head_forward_f32): the hidden activations and the logits never reach memory.
    `conv1`, `bn1` and `conv2` are holders with the names and shapes of nn.Conv1d(in_channel, hidden, 1), nn.BatchNorm1d(hidden) and
    nn.Conv1d(hidden, num_classes, 1), `drop1` has no state: a strict state_dict exchange with a torch head built that way works in both
    directions.  forward(points [B, in_channel, N]) -> log-probabilities [B, N, num_classes]; predict(points) -> the classes, int64 [B, N]
    (the lowest class among equal logits).
    batch_stats=False (default): eval mode only -- bn1 normalises with its running statistics and dropout is the identity; .train()
    followed by a call raises.  batch_stats=True: train mode is accepted and is the layer torch trains (ampnet_seg_head_train_forward_f32):
    bn1 normalises with the statistics of the call's B * N rows and updates running_mean / running_var (with bn1.momentum, a float) and
    num_batches_tracked once per forward, graph or not; drop1 drops with p = drop1.p (p >= 1 raises) and the package's counter hash.  The
    mask of a call comes from `seed` and `_step` (next_seed(): seed + 0x632BE5AB * _step, _step advancing by one per train-mode call): two
    heads with equal seed and _step draw equal masks, consecutive calls different ones, and setting `seed` reproduces a run.  predict() is
    an eval operation and raises in train mode; eval mode is the same whatever batch_stats is.
    grad=True: with grad mode on and an input or a parameter that requires grad, the result carries a graph to the points and to conv1,
    bn1's weight and bias and conv2 (ampnet_seg_head_backward_f32 through autograd._SegHeadFn; running_mean and running_var are constants;
    in train mode ampnet_seg_head_train_backward_f32 through autograd._SegHeadTrainFn, back through the batch statistics and the mask).
    grad=False (default): no graph, ever.
    Limits: 1 <= in_channel <= 256, hidden a multiple of 32 in [32, 256], 2 <= num_classes <= 32.  The head is exact fp32 and has no
    `precision` keyword.  Not built: bf16, a fused loss (F.nll_loss on the [B * N, num_classes] log-probabilities is a small operation;
    seg_nll_loss below is that operation with the predictions and the confusion counts in one pass, behind the head, not inside its kernel),
    momentum=None (the cumulative average), dropout in eval mode."""

    def __init__(self, in_channel, hidden, num_classes, dropout=0.5, device='cuda', grad=False, batch_stats=False):
        super().__init__()
        in_channel, hidden, num_classes = int(in_channel), int(hidden), int(num_classes)
        if not (1 <= in_channel <= _lib.SEG_HEAD_MAX_CIN and 32 <= hidden <= _lib.SEG_HEAD_MAX_HIDDEN and hidden % 32 == 0
                and 2 <= num_classes <= _lib.SEG_HEAD_MAX_CLASSES):
            raise NotImplementedError(f"the HIP segmentation head is built for 1 <= in_channel <= {_lib.SEG_HEAD_MAX_CIN}, hidden a multiple "
                                      f"of 32 in [32, {_lib.SEG_HEAD_MAX_HIDDEN}] and 2 <= num_classes <= {_lib.SEG_HEAD_MAX_CLASSES}, got "
                                      f"in_channel={in_channel} hidden={hidden} num_classes={num_classes}")
        self.grad = bool(grad)
        self.batch_stats = bool(batch_stats)
        self.in_channel, self.hidden, self.num_classes = in_channel, hidden, num_classes
        self.conv1 = _Conv(in_channel, hidden, (1,), device)
        self.bn1 = _BN2d(hidden, device)
        self.drop1 = nn.Dropout(dropout)                            # (a holder as well: its p is read in train mode, nothing else)
        self.conv2 = _Conv(hidden, num_classes, (1,), device)
        self._ws = None
        self._step = 0
        self.seed = 0x6A09E667

    def next_seed(self):
        """The dropout seed of this call; train mode advances the step (the convention of pointnetAtt.SegmentationWithGRU)."""
        seed = (self.seed + 0x632BE5AB * self._step) & 0xFFFFFFFF
        if self.training:
            self._step += 1
        return seed

    def _wants_grad(self, points):
        return self.grad and torch.is_grad_enabled() and (points.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _check_input(self, points):
        if self.training and not self.batch_stats:
            raise NotImplementedError(_SEG_EVAL_ONLY)
        _lib.require_gpu(points, "points")
        if points.dim() != 3 or points.shape[1] != self.in_channel:
            raise _lib.AmpnetError(f"PointNetSegHead: expected points [B, {self.in_channel}, N], got {tuple(points.shape)}")

    def forward(self, points):
        """points [B, in_channel, N] -> log-probabilities [B, N, num_classes]."""
        self._check_input(points)
        if self._wants_grad(points):                                 # a differentiable transpose
            return self._forward_rows(points.float().transpose(1, 2).contiguous())
        with torch.no_grad():
            return self._forward_rows(points.detach().float().transpose(1, 2).contiguous())

    def predict(self, points):
        """points [B, in_channel, N] -> the class of every point, int64 [B, N]: the kernel's own arg-max of the logits, the lowest class
        among equal ones (what utils.get_metrics.confusion_device takes).  Never a graph."""
        if self.training and self.batch_stats:                       # (without batch_stats: _check_input's refusal, as before)
            raise NotImplementedError("PointNetSegHead.predict is an eval operation: call .eval() first")
        self._check_input(points)
        with torch.no_grad():
            return self._forward_rows(points.detach().float().transpose(1, 2).contiguous(), want_preds=True)[1]

    def _forward_rows(self, rows, want_preds=False):
        """The head on point-major rows [B, N, in_channel], float32 contiguous GPU -> [B, N, num_classes]; want_preds: (that, int64
        [B, N]) without a graph."""
        from ... import autograd
        B, N, _ = rows.shape
        flat = rows.reshape(B * N, self.in_channel)
        if self.training:
            if want_preds:
                raise NotImplementedError("PointNetSegHead.predict is an eval operation: call .eval() first")
            return self._train_rows(flat).reshape(B, N, self.num_classes)
        ws = _workspace(self, _lib.seg_head_forward_workspace_bytes(self.in_channel, self.hidden, self.num_classes, B * N), rows.device)
        if not want_preds and self._wants_grad(rows):
            return autograd.seg_head_apply(self, flat, ws).reshape(B, N, self.num_classes)
        logp = torch.empty((B * N, self.num_classes), dtype=torch.float32, device=rows.device)
        preds = torch.empty((B * N,), dtype=torch.int64, device=rows.device) if want_preds else None
        _lib.seg_head_forward_f32(flat.detach(), autograd.seg_head_params(autograd.seg_head_tensors(self)), self.bn1.eps, logp, preds, ws)
        logp = logp.reshape(B, N, self.num_classes)
        return (logp, preds.reshape(B, N)) if want_preds else logp

    def _train_rows(self, flat):
        """_forward_rows in train mode (batch_stats=True) on the flat rows [B * N, in_channel]: batch statistics, bn1's buffers updated in
        place, dropout from next_seed(), a graph when one is wanted."""
        if not self.batch_stats:
            raise NotImplementedError(_SEG_EVAL_ONLY)
        p = float(self.drop1.p)
        if not 0.0 <= p < 1.0:
            raise NotImplementedError(f"the HIP segmentation head drops with 0 <= p < 1, got drop1.p={self.drop1.p}")
        if self.bn1.momentum is None:
            raise NotImplementedError("train-mode segmentation head takes one float momentum for bn1, got None (momentum=None, the cumulative "
                                      "average, is not built)")
        momentum = float(self.bn1.momentum)
        from ... import autograd
        seed = self.next_seed()
        if self._wants_grad(flat):
            logp = autograd.seg_head_train_apply(self, flat, momentum, p, seed)
        else:
            with torch.no_grad():
                t = autograd.seg_head_tensors(self)
                params = autograd.seg_head_params(t)
                params[4], params[5] = t[4], t[5]                   # the buffers themselves: the forward updates them in place
                logp, _, _ = autograd.seg_head_train_forward(flat.detach(), params, self.bn1.eps, momentum, p, seed)
        with torch.no_grad():
            self.bn1.num_batches_tracked += 1
        return logp


def seg_nll_loss(log_probs, target, weight=None, want_preds=False, want_counts=False):
    """The loss behind PointNetSegHead / pointnet_2_seg in one pass over the log-probabilities (ampnet_seg_nll_forward_f32):
    log_probs [..., C] float32, target [...] int64 (a target outside [0, C) is ignored; -1 is the padding label), weight [C] float32 or None
    -> (loss 0-d, preds int64 [...] or None, counts int64 [C * C + 1] or None).
    loss is F.nll_loss(log_probs.reshape(-1, C), target.reshape(-1), weight, ignore_index=-1) with the two sums taken in float64 (NaN when
    every row is ignored, as torch); preds the lowest class among the equal largest entries of a row (the head's own rule), ignored rows
    included; counts what utils.get_metrics.confusion_device(preds, target, C) returns, so metrics_from_confusion applies unchanged.
    GPU tensors only, nothing synchronises.  With grad mode on and log_probs requiring grad, loss carries a graph to log_probs
    (ampnet_seg_nll_backward_f32 through autograd._SegNllFn, the upstream gradient read on the device); preds and counts never do.
    Limits: 2 <= C <= 32 (the head's)."""
    from ... import autograd
    _lib.require_gpu(log_probs, "log_probs")
    _lib.require_gpu(target, "target")
    if log_probs.dim() < 1 or tuple(target.shape) != tuple(log_probs.shape[:-1]) or target.dtype != torch.int64:
        raise _lib.AmpnetError(f"seg_nll_loss: expected log_probs [..., C] and an int64 target of shape [...], got {tuple(log_probs.shape)} "
                               f"{log_probs.dtype} / {tuple(target.shape)} {target.dtype}")
    C = log_probs.shape[-1]
    flat = log_probs.float().reshape(-1, C).contiguous()            # (views of the head's output: no copy)
    t = target.reshape(-1).contiguous()
    if weight is not None:
        _lib.require_gpu(weight, "weight")
        weight = weight.detach().float().contiguous()
    if torch.is_grad_enabled() and log_probs.requires_grad:
        loss, preds, counts = autograd._SegNllFn.apply(flat, t, weight, bool(want_preds), bool(want_counts))
    else:
        with torch.no_grad():
            loss, _, preds, counts = autograd.seg_nll_forward(flat.detach(), t, weight, bool(want_preds), bool(want_counts))
    return loss, (None if preds is None else preds.reshape(target.shape)), counts


def token_pool(rows, weight, bias, sizes=None, want_arg=False):
    """One token per cloud in ONE fused kernel (ampnet_token_pool_forward_f32): tokens[q, c] = max over the rows r of cloud q of
    (weight[c, :] . rows[r, :] + bias[c]) -- nn.Conv1d(cin, cout, 1) and the max over the points, what pointnet_2 ends in, on point-major
    rows: no transpose, no [Q, cout, n] tensor.  No BatchNorm, no ReLU: a maximum below zero stays below zero.
    rows: [Q, n, cin] with sizes=None, or the clouds packed back to back [total, cin] with `sizes`, their row counts (each >= 1; or a
    utils.RaggedLayout); float32 GPU.  weight: [cout, cin] or nn.Conv1d's [cout, cin, 1]; bias [cout].  cin and cout multiples of 32 in
    [32, 256].  -> tokens [Q, cout] float32, or (tokens, arg) with want_arg: arg int32 [Q, cout], the index inside its cloud of the LOWEST
    row that attains the maximum.
    Exact fp32 whatever the matrix precision is (no precision scope is consulted), and a row's value is a function of the row and the
    weights alone: cloud by cloud the packed call gives the bits of the call on that cloud alone, and two calls give the same bits.
    Graph: torch's own rule -- with grad mode on and rows, weight or bias requiring grad the tokens carry a graph to those of them
    (autograd._TokenPoolFn: ampnet_token_pool_backward_f32 on the winning rows alone; the gradient of rows is dense, zero outside the
    winners).  Tie rule: the lowest row takes the whole gradient, where torch.amax's backward splits it evenly among equal maxima.  Equal
    maxima arise from exact duplicate rows (cyclic padding), and there both rules give the same gradients of weight and bias.
    A layout that does not tile the rows, a size below 1, a width outside the limits and a CPU tensor are AmpnetError."""
    from ... import autograd
    for name, t in (("rows", rows), ("weight", weight), ("bias", bias)):
        if not torch.is_tensor(t):
            raise _lib.AmpnetError(f"token_pool: {name} must be a GPU tensor, got {type(t).__name__}")
        _lib.require_gpu(t, name)
    if weight.dim() == 3 and weight.shape[2] == 1:
        w2 = weight.reshape(weight.shape[0], weight.shape[1])
    else:
        w2 = weight
    if w2.dim() != 2 or bias.dim() != 1 or bias.shape[0] != w2.shape[0]:
        raise _lib.AmpnetError(f"token_pool: expected weight [cout, cin] or [cout, cin, 1] and bias [cout], got {tuple(weight.shape)} "
                               f"{tuple(bias.shape)}")
    cout, cin = w2.shape
    if sizes is None:
        if rows.dim() != 3 or rows.shape[2] != cin or rows.shape[0] < 1 or rows.shape[1] < 1:
            raise _lib.AmpnetError(f"token_pool: without sizes, expected rows [Q >= 1, n >= 1, cin = {cin}], got {tuple(rows.shape)}")
        Q, n = rows.shape[0], rows.shape[1]
        if Q * n > 0x7fffffff:
            raise _lib.AmpnetError(f"token_pool: {Q * n} rows exceed 2^31 - 1")
        off = torch.arange(0, (Q + 1) * n, n, dtype=torch.int32 if (Q + 1) * n <= 0x7fffffff else torch.int64, device=rows.device).int()
    else:
        if rows.dim() != 2 or rows.shape[1] != cin:
            raise _lib.AmpnetError(f"token_pool: with sizes, expected packed rows [total, cin = {cin}], got {tuple(rows.shape)}")
        off = U.ragged_layout("token_pool", rows, sizes).off
        Q = off.numel() - 1
    for name, v in (("cin", cin), ("cout", cout)):
        if v % 32 or not (32 <= v <= 256):
            raise _lib.AmpnetError(f"token_pool: {name}={v}, must be a multiple of 32 in [32, 256]")
    flat = rows.reshape(-1, cin)
    flat = (flat if flat.dtype == torch.float32 else flat.float()).contiguous()
    if torch.is_grad_enabled() and (rows.requires_grad or weight.requires_grad or bias.requires_grad):
        tokens, arg = autograd._TokenPoolFn.apply(off, flat, weight, bias)
    else:
        with torch.no_grad():
            tokens, arg = autograd.token_pool_forward(flat.detach(), off, w2.detach().float().contiguous(), bias.detach().float().contiguous(),
                                                      want_arg=bool(want_arg))
    return (tokens, arg) if want_arg else tokens
