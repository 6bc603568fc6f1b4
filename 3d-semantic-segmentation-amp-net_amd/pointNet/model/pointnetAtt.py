"""Drop-in AMP-Net modules on the MI355X HIP path.

Same class names, constructor arguments, forward signatures, return values and `state_dict` keys as the
reference's pointNet/model/pointnetAtt.py (TransformationNet :7-47, BasePointNet :50-112,
SegmentationWithAttention :154-209, SegmentationWithGRU :212-258, pointnet_2 :282-322 -- eval mode only), so reference checkpoints load and the reference's train/test scripts
run unchanged on top of them.  The modules own ordinary nn.Parameters / buffers (as holders: their own
`forward` is never used); every forward goes through the C ABI (ops.encoder_forward / ops.head_forward).
There is no CPU or torch fallback: on a CPU tensor the call raises.

Beyond the reference signatures, BasePointNet.forward_windows() and SegmentationWithAttention.forward_rows()
take ALL windows of a step at once (what the reference does with W serial encoder calls and a Python
repeat/cat loop); the package's train_loop uses those.

Also beyond the reference: the keyword-only constructor argument `precision` (and set_precision()) of the modules that launch
kernels -- the matrix precision their C-ABI calls run in ('fp32', 'f32x3', 'bf16', 'bf16_train', 'bf16_store'; None = the library's
process-wide default).  It is a plain attribute: not a parameter, not a buffer, not in the state_dict.

Only the AMP-Net configuration is implemented in HIP: point_dimension=3, global_feat_dim=256, local_dim=64,
embed_dim=256, num_heads=8, num_classes<=8 (train_pointnet-attention.py:110-118); other values raise.
"""
import contextlib

import torch
import torch.nn as nn

from ... import _lib, ops
from ... import params as P
from ...utils import utils as U
from ._precision import _EvalForwardPrecision, _HasPrecision, is_bf16     # noqa: F401  (_HasPrecision: _baseline.py takes it from here)
from .pointnet2_utils import PointNetFeaturePropagation, PointNetSegHead, PointNetSetAbstraction, token_pool


class _Conv(nn.Module):
    """Holder with nn.Conv1d(k=1)'s parameter names and shapes."""

    def __init__(self, cin, cout, bias, device):
        super().__init__()
        k = 1.0 / cin ** 0.5
        self.weight = nn.Parameter(torch.empty(cout, cin, 1, device=device).uniform_(-k, k))
        if bias:
            self.bias = nn.Parameter(torch.empty(cout, device=device).uniform_(-k, k))


class _Linear(nn.Module):
    def __init__(self, cin, cout, bias, device):
        super().__init__()
        k = 1.0 / cin ** 0.5
        self.weight = nn.Parameter(torch.empty(cout, cin, device=device).uniform_(-k, k))
        if bias:
            self.bias = nn.Parameter(torch.empty(cout, device=device).uniform_(-k, k))


class _BN(nn.Module):
    def __init__(self, c, device):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c, device=device))
        self.bias = nn.Parameter(torch.zeros(c, device=device))
        self.register_buffer("running_mean", torch.zeros(c, device=device))
        self.register_buffer("running_var", torch.ones(c, device=device))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long, device=device))


class _MHA(nn.Module):
    """Holder with nn.MultiheadAttention's parameter names (packed in-projection)."""

    def __init__(self, e, device):
        super().__init__()
        k = (6.0 / (4 * e)) ** 0.5                       # xavier_uniform_ on [3e, e]
        self.in_proj_weight = nn.Parameter(torch.empty(3 * e, e, device=device).uniform_(-k, k))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * e, device=device))
        self.out_proj = _Linear(e, e, True, device)
        with torch.no_grad():
            self.out_proj.bias.zero_()


def _named_tensors(module):
    d = {k: v for k, v in module.named_parameters()}
    d.update({k: v for k, v in module.named_buffers() if not k.endswith("num_batches_tracked")})
    return d


class _TableCache:
    """PointerTables rebuilt only when a tensor moved (load_state_dict copies in place, .to() may not) or the module's precision changed."""

    def __init__(self):
        self.key = None
        self.tables = None

    def get(self, module, ptable, btable, what):
        t = _named_tensors(module)
        precision = getattr(module, "precision", None)
        key = tuple(v.data_ptr() for v in t.values()) + (precision,)
        if key != self.key:
            self.tables = (ops.PointerTable(ptable, t, what + " parameters", precision), ops.PointerTable(btable, t, what + " buffers", precision))
            self.key = key
        return self.tables


class TransformationNet(nn.Module):
    """Parameter holder of one T-Net (pointnetAtt.py:9-26).  Its computation is part of BasePointNet's
    launch sequence (csrc/encoder.hip: run_tnet); calling it on its own is not supported."""

    def __init__(self, input_dim, output_dim, device):
        super().__init__()
        self.device = device
        self.output_dim = output_dim
        self.conv_1 = _Conv(input_dim, 64, False, device)
        self.conv_2 = _Conv(64, 128, False, device)
        self.conv_3 = _Conv(128, 256, False, device)
        self.bn_1, self.bn_2, self.bn_3 = _BN(64, device), _BN(128, device), _BN(256, device)
        self.bn_4, self.bn_5 = _BN(256, device), _BN(128, device)
        self.fc_1 = _Linear(256, 256, False, device)
        self.fc_2 = _Linear(256, 128, False, device)
        self.fc_3 = _Linear(128, output_dim * output_dim, True, device)

    def forward(self, x):
        raise _lib.AmpnetError("TransformationNet runs inside BasePointNet's HIP launch sequence; call BasePointNet")


class BasePointNet(_HasPrecision, nn.Module):

    def __init__(self, point_dimension=2, return_local_features=False, global_feat_dim=256, device='cuda', *, precision=None):
        super().__init__()
        self.set_precision(precision)
        if point_dimension != P.POINT_DIM or global_feat_dim != P.GLOBAL_DIM:
            raise NotImplementedError("the HIP encoder is built for point_dimension=3, global_feat_dim=256 "
                                      "(train_pointnet-attention.py:110-113)")
        self.global_feat_dim = global_feat_dim
        self.point_dimension = point_dimension
        self.return_local_features = return_local_features
        self.input_transform = TransformationNet(point_dimension, point_dimension, device)
        self.feature_transform = TransformationNet(64, 64, device)
        self.conv_1 = _Conv(9 + point_dimension, 64, False, device)
        self.conv_2 = _Conv(64, 64, False, device)
        self.conv_3 = _Conv(64, 64, False, device)
        self.conv_4 = _Conv(64, 128, False, device)
        self.conv_5 = _Conv(128, 128, False, device)
        self.conv_6 = _Conv(128, global_feat_dim, False, device)
        self.bn_1, self.bn_2, self.bn_3 = _BN(64, device), _BN(64, device), _BN(64, device)
        self.bn_4, self.bn_5, self.bn_6 = _BN(128, device), _BN(128, device), _BN(global_feat_dim, device)
        self._cache = _TableCache()
        self._ws = ops.Workspace()

    def _tables(self):
        return self._cache.get(self, P.ENC_PARAMS, P.ENC_BUFFERS, "BasePointNet")

    def _bn_counters(self):
        return [m.num_batches_tracked for m in self.modules() if isinstance(m, _BN)]

    def _bump_batches(self, n):
        # one multi-tensor launch for the 16 counters (16 single-element kernels per step otherwise)
        torch._foreach_add_(self._bn_counters(), n)

    def forward_windows(self, x, np_cluster=None, n_slots=1):
        """All windows of a step in one launch sequence.

        x: [Q, N, 9] (uniform windows) or [rows, 9] with np_cluster = list of Q window sizes.
        n_slots: train mode only -- windows q with equal q % n_slots share BatchNorm batch statistics
        (Q = B * n_slots, q = b * n_slots + w), i.e. n_slots = W reproduces the reference's W encoder calls.
        Returns (local [rows, 64], global [Q, 256], feature_transform [Q, 64, 64]); in train mode the
        feature transforms are slot-major (the last Q / n_slots rows belong to the last slot)."""
        if x.dim() == 3:
            sizes = [x.shape[1]] * x.shape[0]
            rows = x.reshape(-1, x.shape[2])
        else:
            if np_cluster is None:
                raise _lib.AmpnetError("forward_windows: [rows, 9] input needs np_cluster")
            sizes, rows = [int(n) for n in np_cluster], x
        _lib.require_gpu(rows, "x")
        off, total, mx = ops.window_offsets(sizes, rows.device)
        pt, bt = self._tables()
        train = self.training
        if train and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from ...autograd import encoder_apply
            return encoder_apply(self, pt, bt, rows.float(), off, len(sizes), total, mx, n_slots)
        with _lib.precision_scope(self.precision):
            local, glob, feat_T, _ = ops.encoder_forward(pt, bt, rows.float(), off, len(sizes), total, mx,
                                                         n_slots if train else 1, train, self._ws)
        if train:
            self._bump_batches(n_slots)
        return local, glob, feat_T

    def forward(self, x):
        """Reference signature (pointnetAtt.py:80-112): x [B, N, 9] ->
        (cat([global.repeat(N), local], 2) [B, N, 320], feature_transform [B, 64, 64]) when
        return_local_features else (global [B, 256], feature_transform)."""
        B, N = x.shape[0], x.shape[1]
        local, glob, feat_T = self.forward_windows(x, n_slots=1)
        if self.return_local_features:
            out = torch.cat([glob.unsqueeze(1).expand(B, N, self.global_feat_dim), local.view(B, N, 64)], dim=2)
            return out, feat_T
        return glob, feat_T


class SegmentationWithAttention(_HasPrecision, nn.Module):

    def __init__(self, embed_dim, num_heads, num_classes=2, local_dim=128, dropout=0.3, device='cuda', *, precision=None):
        super().__init__()
        self.set_precision(precision)
        if embed_dim != P.GLOBAL_DIM or num_heads != P.HEADS or local_dim != P.LOCAL_DIM or not (1 <= num_classes <= 8):
            raise NotImplementedError("the HIP head is built for embed_dim=256, num_heads=8, local_dim=64, "
                                      "num_classes<=8 (train_pointnet-attention.py:118)")
        self.embed_dim = embed_dim
        self.device = device
        self.num_classes = num_classes
        self.p_drop = float(dropout)
        self.fc1 = _Linear(2, 16, True, device)
        self.fc2 = _Linear(16, embed_dim, True, device)
        self.attention = _MHA(embed_dim, device)
        self.conv_2 = _Conv(local_dim + embed_dim, embed_dim // 2, True, device)
        self.conv_3 = _Conv(embed_dim // 2, 64, True, device)
        self.conv_4 = _Conv(64, num_classes, True, device)
        self.bn_2 = _BN(embed_dim // 2, device)
        self.bn_3 = _BN(64, device)
        self._cache = _TableCache()
        self._ws = ops.Workspace()
        self._step = 0
        self.seed = 0x5EED

    def _param_table(self):
        from collections import OrderedDict
        table = OrderedDict(P.HEAD_PARAMS)
        table["conv_4.weight"] = (self.num_classes, 64, 1)
        table["conv_4.bias"] = (self.num_classes,)
        return table

    def _tables(self):
        return self._cache.get(self, self._param_table(), P.HEAD_BUFFERS, "SegmentationWithAttention")

    def forward_rows(self, gl_rows, lo_rows, centroids, np_cluster, attn_mask=None, targets=None, class_w=None,
                     want_preds=False):
        """gl_rows [B*W, 256] (row b*W+w), lo_rows [B*P, 64] -> (logits [B, C, P], preds or None, loss or None)."""
        B, W = centroids.shape[0], centroids.shape[1]
        sizes = [int(n) for n in np_cluster] * B
        off, total, mx = ops.window_offsets(sizes, lo_rows.device)
        pt, bt = self._tables()
        train = self.training
        seed = (self.seed + 0x632BE5AB * self._step) & 0xFFFFFFFF
        if train:
            self._step += 1
        if train and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from ...autograd import head_apply
            return head_apply(self, pt, bt, gl_rows, lo_rows, centroids, off, attn_mask, B, W, total, mx,
                              self.num_classes, self.p_drop, seed, targets, class_w, want_preds)
        with _lib.precision_scope(self.precision):
            out = ops.head_forward(pt, bt, gl_rows, lo_rows, centroids, off, attn_mask, B, W, total, mx, self.num_classes,
                                   train, self.p_drop, seed, self._ws, targets=targets, class_w=class_w, want_preds=want_preds)
        if train:
            torch._foreach_add_([self.bn_2.num_batches_tracked, self.bn_3.num_batches_tracked], 1)
        return out

    def forward(self, gl_feats, lo_feats, centroids, np_cluster, attn_mask=None):
        """Reference signature (pointnetAtt.py:176-209): gl_feats [W, B, 256], lo_feats [B, P, 64],
        centroids [B, W, 2], np_cluster list of W sizes, attn_mask [B, W] bool -> (logits [B, C, P], 0)."""
        W, B = gl_feats.shape[0], gl_feats.shape[1]
        gl_rows = gl_feats.transpose(0, 1).reshape(B * W, self.embed_dim)
        lo_rows = lo_feats.reshape(-1, lo_feats.shape[2])
        logits, _, _ = self.forward_rows(gl_rows, lo_rows, centroids, np_cluster, attn_mask)
        return logits, 0


class _GRU(nn.Module):
    """Holder with nn.GRU(input, hidden, num_layers=1)'s parameter names, shapes and U(-1/sqrt(H), 1/sqrt(H)) initialisation."""

    def __init__(self, cin, hidden, device):
        super().__init__()
        k = 1.0 / hidden ** 0.5
        self.weight_ih_l0 = nn.Parameter(torch.empty(3 * hidden, cin, device=device).uniform_(-k, k))
        self.weight_hh_l0 = nn.Parameter(torch.empty(3 * hidden, hidden, device=device).uniform_(-k, k))
        self.bias_ih_l0 = nn.Parameter(torch.empty(3 * hidden, device=device).uniform_(-k, k))
        self.bias_hh_l0 = nn.Parameter(torch.empty(3 * hidden, device=device).uniform_(-k, k))


class SegmentationWithGRU(_HasPrecision, nn.Module):
    """The GRU variant of the sequence model (pointnetAtt.py:212-258): nn.GRU(256 -> 64, batch_first, h0 = 0) over the
    window tokens, hidden state of step w broadcast over the points of window w, then conv_2 / bn_2 / conv_3 / bn_3 / conv_4 with
    Dropout(0.3) twice.  Runs through ampnet_gru_head_fwd_f32 / _bwd_f32 (csrc/gru_head.hip)."""
    head_kind = "gru"

    def __init__(self, num_classes, global_feat_size, hidden_size, device, *, precision=None):
        super().__init__()
        self.set_precision(precision)
        if global_feat_size != P.GLOBAL_DIM or hidden_size != P.GRU_HIDDEN or not (1 <= num_classes <= 8):
            raise NotImplementedError("the HIP GRU head is built for global_feat_size=256, hidden_size=64, num_classes<=8 "
                                      "(pointNet/rnn/train_pointnetGRU.py:27-28,128)")
        self.hidden_size = hidden_size
        self.device = device
        self.num_classes = num_classes
        self.p_drop = 0.3                                   # nn.Dropout(0.3), pointnetAtt.py:225
        self.gru_global = _GRU(global_feat_size, hidden_size, device)
        self.conv_2 = _Conv(64 + 64, 128, True, device)
        self.conv_3 = _Conv(128, 64, True, device)
        self.conv_4 = _Conv(64, num_classes, True, device)
        self.bn_2 = _BN(128, device)
        self.bn_3 = _BN(64, device)
        self._cache = _TableCache()
        self._ws = ops.Workspace()
        self._step = 0
        self.seed = 0x6A09E667

    def _param_table(self):
        from collections import OrderedDict
        table = OrderedDict(P.GRU_HEAD_PARAMS)
        table["conv_4.weight"] = (self.num_classes, 64, 1)
        table["conv_4.bias"] = (self.num_classes,)
        return table

    def _tables(self):
        return self._cache.get(self, self._param_table(), P.HEAD_BUFFERS, "SegmentationWithGRU")

    def next_seed(self):
        seed = (self.seed + 0x632BE5AB * self._step) & 0xFFFFFFFF
        if self.training:
            self._step += 1
        return seed

    def forward_rows(self, gl_rows, lo_rows, np_cluster, B, targets=None, class_w=None, want_preds=False):
        """gl_rows [B*W, 256] (row b*W+w), lo_rows [B*P, 64], np_cluster: the W window sizes of a sample
        -> (logits [B, C, P], preds or None, loss or None)."""
        W = len(np_cluster)
        sizes = [int(n) for n in np_cluster] * B
        off, total, mx = ops.window_offsets(sizes, lo_rows.device)
        pt, bt = self._tables()
        train = self.training
        seed = self.next_seed()
        if train and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from ...autograd import gru_head_apply
            return gru_head_apply(self, pt, bt, gl_rows, lo_rows, off, B, W, total, mx, self.num_classes, self.p_drop, seed, want_preds)
        with _lib.precision_scope(self.precision):
            out = ops.gru_head_forward(pt, bt, gl_rows.contiguous().float(), lo_rows.contiguous().float(), off, B, W, total, mx, self.num_classes,
                                       train, self.p_drop, seed, self._ws, targets=targets, class_w=class_w, want_preds=want_preds)
        if train:
            torch._foreach_add_([self.bn_2.num_batches_tracked, self.bn_3.num_batches_tracked], 1)
        return out

    def forward(self, global_seq, local_feats, np_cluster):
        """Reference signature (pointnetAtt.py:232-250): global_seq [B, W, 256], local_feats [B, P, 64], np_cluster list of W sizes
        -> logits [B, C, P]."""
        B, W = global_seq.shape[0], global_seq.shape[1]
        logits, _, _ = self.forward_rows(global_seq.reshape(B * W, -1), local_feats.reshape(-1, local_feats.shape[2]), np_cluster, B)
        return logits

    def initHidden(self, x):
        return torch.zeros(1, x.shape[0], self.hidden_size, device=x.device)


class ClassificationFromGRU(nn.Module):
    """Parameter-compatible holder of pointnetAtt.py:261-279.  The reference's forward reads self.embed_dim, which its __init__ never
    sets, and no reference script reaches it (train_pointnetGRU.py:405-407 leaves the classification branch without logits): calling it
    raises AttributeError there; here it raises with the reason."""

    def __init__(self, num_classes=2, dropout=0.3, num_w=5, embed_dim=256, device='cuda'):
        super().__init__()
        self.conv_1 = _Conv(num_w, 1, True, device)
        self.fc_2 = _Linear(embed_dim, 128, True, device)
        self.fc_3 = _Linear(128, num_classes, True, device)
        self.bn_2 = _BN(128, device)

    def forward(self, x):
        raise AttributeError("'ClassificationFromGRU' object has no attribute 'embed_dim' (the reference's forward fails the same way, "
                             "pointnetAtt.py:274; the classification task is not runnable in the reference)")


class ClassificationWithAttention(_HasPrecision, nn.Module):
    """pointnetAtt.py:115-151 on the HIP path (ampnet_cls_head_fwd_f32 / _bwd_f32, csrc/cls_head.hip): MultiheadAttention over the window
    tokens, conv_1 = Conv1d(num_w -> 1, 1) over the attention output re-viewed as [B, W, E] (a view of the sequence-first tensor, as the
    reference writes it), fc_2 -> bn_2 -> ReLU -> fc_3.  forward(gl_feats [W, B, E], centroids, attn_mask) -> (out [B, C], weights
    [B, W, W]); centroids are unused by the reference (the positional encoding is commented out there)."""

    def __init__(self, embed_dim, num_heads, num_classes=2, dropout=0.3, num_w=9, device='cuda', *, precision=None):
        super().__init__()
        self.set_precision(precision)
        if embed_dim != P.GLOBAL_DIM or num_heads != P.HEADS or not (1 <= num_classes <= 16) or not (1 <= num_w <= 32):
            raise NotImplementedError("the HIP classification head is built for embed_dim=256, num_heads=8, num_classes<=16, num_w<=32")
        self.embed_dim = embed_dim
        self.num_classes, self.num_w = num_classes, num_w
        self.p_drop = float(dropout)
        self.attention = _MHA(embed_dim, device)
        self.conv_1 = _Conv(num_w, 1, True, device)
        self.fc_2 = _Linear(embed_dim, 128, True, device)
        self.fc_3 = _Linear(128, num_classes, True, device)
        self.bn_2 = _BN(128, device)
        self._cache = _TableCache()
        self._ws = ops.Workspace()
        self._step = 0
        self.seed = 0x3C6EF372

    def _param_table(self):
        return P.cls_head_params(self.num_classes, self.num_w)

    def _tables(self):
        return self._cache.get(self, self._param_table(), P.CLS_HEAD_BUFFERS, "ClassificationWithAttention")

    def forward(self, gl_feats, centroids=None, attn_mask=None):
        W, B = gl_feats.shape[0], gl_feats.shape[1]
        if W != self.num_w:
            raise _lib.AmpnetError(f"ClassificationWithAttention: {W} tokens per sample, conv_1 was built for num_w={self.num_w}")
        gl_rows = gl_feats.transpose(0, 1).reshape(B * W, self.embed_dim)
        pt, bt = self._tables()
        train = self.training
        seed = (self.seed + 0x632BE5AB * self._step) & 0xFFFFFFFF
        if train:
            self._step += 1
        if train and torch.is_grad_enabled() and (gl_feats.requires_grad or any(p.requires_grad for p in self.parameters())):
            from ...autograd import cls_head_apply
            return cls_head_apply(self, pt, bt, gl_rows, attn_mask, B, W, self.num_classes, self.p_drop, seed)
        with _lib.precision_scope(self.precision):
            out = ops.cls_head_forward(pt, bt, gl_rows.contiguous().float(), attn_mask, B, W, self.num_classes, train, self.p_drop, seed, self._ws)
        if train:
            self.bn_2.num_batches_tracked += 1
        return out


class pointnet_2(_EvalForwardPrecision, nn.Module):
    """The PointNet++ backbone of pointnetAtt.py:282-322 in eval mode: three set-abstraction layers (`sa1`..`sa3`), three
    feature-propagation layers (`fp3`..`fp1`) and `conv1`, with the reference's constructor argument, attribute names, layer sizes and
    state_dict keys.  forward(xyz [B, 9, N]) -> (global_feature [B, 128], l0_points [B, 128, N]); the nine input channels are the point
    features of `sa1`, the first three of them the coordinates.  Every block runs its fused HIP kernel (pointnet2_utils.py) and hands the
    next one its point-major [B, N, C] result as it is; `conv1` and the max over the points are torch operations.  `num_classes` is
    unused, as in the reference (its classifier layers are commented out there).

    decoder_grad=True makes the decoder trainable in eval mode (fine-tuning a pretrained backbone with a torch loss and a torch
    optimiser): `fp3`, `fp2`, `fp1` run with grad=True and `conv1` is a torch layer, so both outputs carry a graph to the conv weights
    and biases and the BatchNorm weights and biases of fp1..fp3 and to conv1.  Without encoder_grad, `sa1`..`sa3` are frozen (the encoder
    runs under no_grad on detached inputs, its parameters get no gradient).  encoder_grad=True (needs decoder_grad=True, else ValueError)
    runs `sa1`..`sa3` with grad=True as well: the gradient reaches them through l1_points, l2_points and l3_points -- the skip and coarse
    inputs of fp1..fp3 and the features of sa2 and sa3 -- so the whole backbone can be fine-tuned.  The input and every running_mean /
    running_var stay frozen either way, and without decoder_batch_stats train mode is not built: .train() raises.

    decoder_batch_stats=True (needs decoder_grad=True, else ValueError) lets the decoder TRAIN as torch trains it: `fp3`, `fp2`, `fp1` are
    built with batch_stats=True, and .train(mode) puts the model, fp1..fp3 and conv1 in `mode` while `sa1`..`sa3` stay in eval mode
    whatever encoder_grad is -- without encoder_batch_stats the encoder remains a frozen-statistics feature extractor.  In
    train mode fp1..fp3 normalise with batch statistics, update their running statistics and back-propagate through them.

    encoder_batch_stats=True (needs encoder_grad=True and decoder_batch_stats=True, else ValueError) trains the model from scratch as
    torch trains it: `sa1`..`sa3` are built with batch_stats=True and .train(mode) puts the WHOLE model in `mode`.  In train mode every
    block normalises with the statistics of its batch (the set abstraction over all B * npoint * nsample rows), updates its running
    statistics and num_batches_tracked, and back-propagates through the statistics.

    precision (keyword-only; also set_precision(mode)) is handed to the six blocks (pointnet2_utils.py): None and 'fp32' are the exact-fp32
    kernels whatever the library's mode is, 'bf16' runs every block's matrix products in bf16 -- an inference mode, refused
    (NotImplementedError) together with any of the four flags above.  `conv1` and the max stay fp32.

    forward_tokens(points [Q, N, 9]) -> (tokens [Q, 128], l0_rows [Q, N, 128]) and forward_tokens_ragged(rows [total, 9], sizes) ->
    (tokens [Q, 128], l0_rows [total, 128]) are the model as a WINDOW ENCODER on point-major rows, for windows of one size and for clouds
    of native size: `conv1` and the max run as one fused exact-fp32 kernel with a backward (pointnet2_utils.token_pool), nothing is
    transposed and no [Q, 128, N] tensor is written.  forward() itself stays the torch `conv1` + amax, bit for bit."""

    def __init__(self, num_classes, device='cuda', decoder_grad=False, encoder_grad=False, decoder_batch_stats=False,
                 encoder_batch_stats=False, *, precision=None):
        super().__init__()
        self.decoder_grad = bool(decoder_grad)
        self.encoder_grad = bool(encoder_grad)
        self.decoder_batch_stats = bool(decoder_batch_stats)
        self.encoder_batch_stats = bool(encoder_batch_stats)
        if self.encoder_batch_stats and not (self.encoder_grad and self.decoder_batch_stats):
            raise ValueError("pointnet_2: encoder_batch_stats=True needs encoder_grad=True and decoder_batch_stats=True (train mode is for "
                             "training the whole backbone)")
        if self.decoder_batch_stats and not self.decoder_grad:
            raise ValueError("pointnet_2: decoder_batch_stats=True needs decoder_grad=True (train mode is for training the decoder)")
        if self.encoder_grad and not self.decoder_grad:
            raise ValueError("pointnet_2: encoder_grad=True needs decoder_grad=True (the gradient reaches sa1..sa3 through fp1..fp3)")
        self.sa1 = PointNetSetAbstraction(1024, 0.1, 32, 9 + 3, [32, 32, 64], False, device=device, grad=self.encoder_grad,
                                          batch_stats=self.encoder_batch_stats)
        self.sa2 = PointNetSetAbstraction(256, 0.2, 32, 64 + 3, [64, 64, 128], False, device=device, grad=self.encoder_grad,
                                          batch_stats=self.encoder_batch_stats)
        self.sa3 = PointNetSetAbstraction(64, 0.4, 32, 128 + 3, [128, 128, 256], False, device=device, grad=self.encoder_grad,
                                          batch_stats=self.encoder_batch_stats)
        self.fp3 = PointNetFeaturePropagation(384, [256, 256], device=device, grad=self.decoder_grad, batch_stats=self.decoder_batch_stats)
        self.fp2 = PointNetFeaturePropagation(320, [256, 128], device=device, grad=self.decoder_grad, batch_stats=self.decoder_batch_stats)
        self.fp1 = PointNetFeaturePropagation(128, [128, 128, 128], device=device, grad=self.decoder_grad, batch_stats=self.decoder_batch_stats)
        self.conv1 = nn.Conv1d(128, 128, 1, device=device)
        self.set_precision(precision)

    def _bf16_refusal(self):
        flags = [f for f in ("decoder_grad", "encoder_grad", "decoder_batch_stats", "encoder_batch_stats") if getattr(self, f)]
        return f"this model was built with {', '.join(f + '=True' for f in flags)}" if flags else None

    def set_precision(self, mode):
        super().set_precision(mode)                                  # (the model's own refusals first: nothing is half set)
        for m in (self.sa1, self.sa2, self.sa3, self.fp3, self.fp2, self.fp1):
            m.set_precision(self.precision)
        return self

    def train(self, mode=True):
        super().train(mode)
        if self.decoder_batch_stats and not self.encoder_batch_stats:                 # the encoder keeps its frozen statistics
            for m in (self.sa1, self.sa2, self.sa3):
                m.train(False)
        return self

    def forward(self, xyz):
        _, l0_points = self._backbone(xyz)
        global_feature = self.conv1(l0_points).amax(2)                                # MaxPool1d(N) + view(-1, 128)
        return global_feature, l0_points

    def _check_block_modes(self):
        """The blocks follow the model's mode (train()): sa1..sa3 train only with encoder_batch_stats, fp1..fp3 with the model."""
        for m in (self.sa1, self.sa2, self.sa3):
            if m.training != (self.training and self.encoder_batch_stats):
                raise NotImplementedError("pointnet_2: a block of the model is in train mode; call .eval() on the model" if m.training else
                                          "pointnet_2: sa1..sa3 follow the model's mode; call .train() on the model, not on its blocks")
        for m in (self.fp3, self.fp2, self.fp1):
            if m.training != self.training:
                raise NotImplementedError("pointnet_2: a block of the model is in train mode; call .eval() on the model" if m.training else
                                          "pointnet_2: fp1..fp3 follow the model's mode; call .train() on the model, not on its blocks")

    def _backbone(self, xyz, rows=False):
        """The six blocks -> (fp1's point-major result [B, N, 128] as it left the kernel, l0_points [B, 128, N]): what pointnet_2 puts
        conv1 and the max behind, and pointnet_2_seg its head.  rows=True: `xyz` is the point-major [B, N, 9] float32 contiguous tensor the
        blocks consume, taken as it is, and l0_points is None -- neither the transpose in nor the [B, 128, N] copy out."""
        if self.training and not self.decoder_batch_stats:
            raise NotImplementedError("pointnet_2 on the HIP path is built for eval mode (BatchNorm running statistics, no backward): "
                                      "call .eval() first")
        self._check_bf16()
        _lib.require_gpu(xyz, "xyz")
        if rows:
            if xyz.dim() != 3 or xyz.shape[2] != 9 or xyz.dtype != torch.float32 or not xyz.is_contiguous():
                raise _lib.AmpnetError(f"pointnet_2: expected point-major rows [Q, N, 9], float32 and contiguous, got {tuple(xyz.shape)} "
                                       f"{xyz.dtype}, strides {xyz.stride()}")
        elif xyz.dim() != 3 or xyz.shape[1] != 9:
            raise _lib.AmpnetError(f"pointnet_2: expected xyz [B, 9, N], got {tuple(xyz.shape)}")
        self._check_block_modes()
        with torch.no_grad():
            l0_points = xyz.detach() if rows else xyz.detach().float().transpose(1, 2).contiguous()      # [B, N, 9]
            l0_xyz = l0_points[:, :, :3].contiguous()                                 # [B, N, 3]
        with contextlib.nullcontext() if self.encoder_grad else torch.no_grad():    # (the caller's grad mode, or none)
            l1_xyz, l1_points = self.sa1._forward_rows(l0_xyz, l0_points)             # [B, 1024, 3], [B, 1024, 64]
            l2_xyz, l2_points = self.sa2._forward_rows(l1_xyz, l1_points)             # [B, 256, 3], [B, 256, 128]
            l3_xyz, l3_points = self.sa3._forward_rows(l2_xyz, l2_points)             # [B, 64, 3], [B, 64, 256]
        with torch.enable_grad() if self.decoder_grad and torch.is_grad_enabled() else torch.no_grad():
            l2_points = self.fp3._forward_rows(l2_xyz, l3_xyz, l2_points, l3_points)  # [B, 256, 256]
            l1_points = self.fp2._forward_rows(l1_xyz, l2_xyz, l1_points, l2_points)  # [B, 1024, 128]
            l0_rows = self.fp1._forward_rows(l0_xyz, l1_xyz, None, l1_points)         # [B, N, 128]
            l0_points = None if rows else l0_rows.transpose(1, 2).contiguous()        # [B, 128, N], the reference's layout
        return l0_rows, l0_points

    def _backbone_ragged(self, rows, sizes):
        """The six blocks on `rows` [total, 9] = clouds of `sizes` points back to back -> (fp1's rows [total, 128], the utils.RaggedLayout).
        Only level 0 is ragged: sa1 emits npoint centres for every cloud, so sa2, sa3, fp3 and fp2 see uniform [Q, npoint, .] tensors and
        run as they are; sa1 samples and groups ragged clouds and fp1 searches from ragged fine points.  The graph rules are _backbone's;
        the mode check is the caller's.  What pointnet_2.forward_tokens_ragged puts the token behind and pointnet_2_seg its head."""
        who = type(self).__name__
        self._check_block_modes()
        _lib.require_gpu(rows, "rows")
        if rows.dim() != 2 or rows.shape[1] != 9 or rows.dtype != torch.float32 or not rows.is_contiguous():
            raise _lib.AmpnetError(f"{who}: expected packed rows [total, 9], float32 and contiguous, got {tuple(rows.shape)} "
                                   f"{rows.dtype}, strides {rows.stride()}")
        layout = U.ragged_layout(who, rows, sizes)
        if min(layout.sizes) < self.sa1.npoint:
            raise _lib.AmpnetError(f"{who}: every cloud needs at least sa1.npoint={self.sa1.npoint} points, cloud "
                                   f"{layout.sizes.index(min(layout.sizes))} has {min(layout.sizes)} (predict_clouds pads such clouds)")
        with torch.no_grad():
            l0_points = rows.detach()
            l0_xyz = l0_points[:, :3].contiguous()                                             # [total, 3]
        with contextlib.nullcontext() if self.encoder_grad else torch.no_grad():             # (the caller's grad mode, or none)
            l1_xyz, l1_points = self.sa1._forward_ragged(l0_xyz, l0_points, layout)            # [Q, 1024, 3], [Q, 1024, 64]
            l2_xyz, l2_points = self.sa2._forward_rows(l1_xyz, l1_points)
            l3_xyz, l3_points = self.sa3._forward_rows(l2_xyz, l2_points)
        with torch.enable_grad() if self.decoder_grad and torch.is_grad_enabled() else torch.no_grad():
            l2_points = self.fp3._forward_rows(l2_xyz, l3_xyz, l2_points, l3_points)
            l1_points = self.fp2._forward_rows(l1_xyz, l2_xyz, l1_points, l2_points)
            l0_rows = self.fp1._forward_ragged(l0_xyz, layout, l1_xyz, None, l1_points)        # [total, 128]
        return l0_rows, layout

    # ---- the fused token path: conv1 and the max as ONE kernel on fp1's rows (pointnet2_utils.token_pool) ---------------------------------
    def forward_tokens(self, points):
        """The model as a window encoder on point-major rows: points [Q, N, 9] float32 contiguous GPU -> (tokens [Q, 128], l0_rows
        [Q, N, 128]): one token per window for a sequence model, per-point local features for a head.  The six blocks as
        _backbone(points, rows=True) runs them, then pointnet2_utils.token_pool(l0_rows, conv1.weight, conv1.bias): neither the
        transpose in nor the [Q, 128, N] copy out, and conv1's [Q, 128, N] output is never written.  tokens is forward()'s global_feature
        up to float32 rounding (another summation order), l0_rows its l0_points transposed, bit for bit.
        Mode checks, flags and graph rules are _backbone's; conv1 has no BatchNorm, so the call works in every mode the backbone accepts.
        conv1 is a torch parameter: with grad mode on, tokens carries a graph to conv1 in every model, and with decoder_grad=True both
        results carry one to the decoder (with encoder_grad=True the whole backbone); a consumer may use either or both, autograd adds the
        two gradients of l0_rows.  The token kernel is exact fp32, behind precision='bf16' blocks too.  Tie rule: the LOWEST row of a
        window takes the whole gradient of a channel, where torch.amax (forward()) splits it evenly among equal maxima; equal maxima arise
        from exact duplicate rows (cyclic padding), and there both rules give the same parameter gradients."""
        l0_rows, _ = self._backbone(points, rows=True)
        return token_pool(l0_rows, self.conv1.weight, self.conv1.bias), l0_rows

    def forward_tokens_ragged(self, rows, sizes):
        """forward_tokens on clouds of UNEQUAL size in one launch sequence: rows [total, 9] float32 contiguous GPU = clouds of `sizes`
        points back to back, sa1.npoint <= n_i <= 12288 -> (tokens [Q, 128], l0_rows [total, 128]).  The ragged backbone that
        pointnet_2_seg.forward_ragged runs, followed by the segmented max; in eval mode, cloud by cloud, the token and the rows are the
        bits of forward_tokens on that cloud alone.  Mode checks, flags and graph rules are forward_tokens'; in train mode (the
        batch-statistics flags) every BatchNorm runs over all rows of the call."""
        if self.training and not self.decoder_batch_stats:
            raise NotImplementedError("pointnet_2 on the HIP path is built for eval mode (BatchNorm running statistics, no backward): "
                                      "call .eval() first")
        self._check_bf16()
        l0_rows, layout = self._backbone_ragged(rows, sizes)
        return token_pool(l0_rows, self.conv1.weight, self.conv1.bias, sizes=layout), l0_rows


class pointnet_2_seg(pointnet_2):
    """pointnet_2 with the classifier the reference carries commented out (pointnetAtt.py:294-296, :318-321) restored: the six blocks,
    then conv1, bn1, ReLU, drop1, conv2 and log_softmax per point as ONE fused kernel (pointnet2_utils.PointNetSegHead).
    forward(xyz [B, 9, N]) -> (log_probs [B, N, num_classes], l0_points [B, 128, N]); predict(xyz) -> the classes, int64 [B, N].
    The state_dict keys are sa1..fp1, conv1.*, bn1.*, conv2.* -- what the reference's class would have with those lines restored -- so a
    pointnet_2 checkpoint loads with strict=False, only bn1.* and conv2.* missing.  `conv1` is the head's first layer here; the global
    feature of pointnet_2 (conv1 and a max over the points) is not computed.

    The four flags are pointnet_2's, with the same rules; the head runs with grad = decoder_grad, so with decoder_grad=True
    F.nll_loss(log_probs.reshape(-1, num_classes), target.reshape(-1)).backward() reaches conv2, bn1's weight and bias, conv1 and the
    decoder (with encoder_grad=True: the whole backbone).  .train(mode) with the batch-statistics flags moves the backbone as in
    pointnet_2 and, without head_batch_stats, KEEPS THE HEAD IN EVAL MODE: bn1 then always normalises with its running statistics, which are
    never updated, and drop1 is always the identity.

    head_batch_stats=True (needs decoder_batch_stats=True, else ValueError) trains the head as torch trains it: the head is built with
    batch_stats=True and .train(mode) moves it with the decoder, so in train mode bn1 normalises with the statistics of the batch, updates
    its running statistics and drop1 drops (PointNetSegHead; the mask follows the head's `seed`).  With all five flags the model trains
    from scratch; .eval() afterwards is the eval forward on the trained state, bit for bit what a default pointnet_2_seg loaded with that
    state_dict gives.  forward_rows / predict_rows are forward / predict on point-major [Q, N, 9] rows, without the transposes
    (pointNet/pn2_step.py trains through them, with pointnet2_utils.seg_nll_loss as the loss).  forward_ragged / predict_ragged /
    predict_clouds label clouds of UNEQUAL size in one launch sequence, cloud by cloud the bits of forward_rows / predict_rows on that cloud
    alone (pointNet/pn2_infer.py drives them); forward_ragged also carries a graph and trains under forward_rows' rules, so the model learns
    from clouds of native size (pn2_step.train_loop_clouds), the two predict calls stay eval operations without a graph.  Not built: bf16 (the model has no
    `precision` keyword and refuses set_precision('bf16')), a loss fused into the head's kernel, momentum=None, dropout in eval mode, train
    mode for group_all set abstraction."""

    def __init__(self, num_classes, device='cuda', decoder_grad=False, encoder_grad=False, decoder_batch_stats=False,
                 encoder_batch_stats=False, head_batch_stats=False):
        super().__init__(num_classes, device, decoder_grad, encoder_grad, decoder_batch_stats, encoder_batch_stats)
        self.head_batch_stats = bool(head_batch_stats)
        if self.head_batch_stats and not self.decoder_batch_stats:
            raise ValueError("pointnet_2_seg: head_batch_stats=True needs decoder_batch_stats=True (the head trains with the decoder)")
        head = PointNetSegHead(128, 128, num_classes, device=device, grad=self.decoder_grad, batch_stats=self.head_batch_stats)
        # the reference's flat names; the head itself is not a registered child (its keys would carry a prefix)
        self.conv1, self.bn1, self.drop1, self.conv2 = head.conv1, head.bn1, head.drop1, head.conv2
        self.__dict__["_head"] = head.eval()

    def _bf16_refusal(self):
        return "the segmentation head is exact fp32"

    def train(self, mode=True):
        super().train(mode)
        self._head.train(bool(mode) and self.head_batch_stats)       # (bn1 and drop1 with it: they are the head's own children)
        return self

    def forward(self, xyz):
        l0_rows, l0_points = self._backbone(xyz)
        with torch.enable_grad() if self.decoder_grad and torch.is_grad_enabled() else torch.no_grad():
            log_probs = self._head._forward_rows(l0_rows)
        return log_probs, l0_points

    def forward_tokens(self, points):
        raise NotImplementedError("pointnet_2_seg: conv1 is the first layer of the segmentation head here, not the token's; forward_tokens "
                                  "and forward_tokens_ragged belong to pointnet_2")

    def forward_tokens_ragged(self, rows, sizes):
        raise NotImplementedError("pointnet_2_seg: conv1 is the first layer of the segmentation head here, not the token's; forward_tokens "
                                  "and forward_tokens_ragged belong to pointnet_2")

    def predict(self, xyz):
        """xyz [B, 9, N] -> the class of every point, int64 [B, N] (the lowest class among equal logits).  Never a graph."""
        with torch.no_grad():
            l0_rows, _ = self._backbone(xyz)
            return self._head._forward_rows(l0_rows, want_preds=True)[1]

    def forward_rows(self, points):
        """forward() on point-major rows: points [Q, N, 9] float32 contiguous GPU (what the device input pipeline writes per window,
        amp_step.augment_ragged_device) -> log_probs [Q, N, num_classes], the bits of forward(points.transpose(1, 2))[0].  The six blocks
        and the head consume and produce rows, so nothing is transposed on the way in and the [Q, 128, N] copy of l0_points -- 604 MB at
        576 windows of 2048 points, with a backward mirror, read by nobody in a train step -- is not made.  Mode checks, graph rules and
        flags are forward()'s."""
        l0_rows, _ = self._backbone(points, rows=True)
        with torch.enable_grad() if self.decoder_grad and torch.is_grad_enabled() else torch.no_grad():
            return self._head._forward_rows(l0_rows)

    def predict_rows(self, points):
        """predict() on point-major rows [Q, N, 9] -> int64 [Q, N].  An eval operation, never a graph."""
        with torch.no_grad():
            l0_rows, _ = self._backbone(points, rows=True)
            return self._head._forward_rows(l0_rows, want_preds=True)[1]

    # ---- clouds of UNEQUAL size in one launch sequence -----------------------------------------------------------------------------------
    # Only level 0 is ragged: sa1 emits npoint centres for every cloud, so sa2, sa3, fp3 and fp2 see uniform [Q, npoint, .] tensors and
    # run as they are; sa1 samples and groups ragged clouds, fp1 searches from ragged fine points, and the head takes any number of rows.
    # forward_ragged follows forward_rows' mode and graph rules (the backwards of sa1 and fp1 gather cloud by cloud: autograd._ragged_note);
    # the two predict calls are eval operations.

    def _ragged(self, rows, sizes, want_preds):
        """The six blocks and the head on `rows` [total, 9] = clouds of `sizes` points back to back -> the head's result on [1, total, 128].
        want_preds: an eval operation, the caller holds no_grad; else the mode checks and the graph rules of _backbone."""
        if want_preds:
            every = (self, self._head, self.sa1, self.sa2, self.sa3, self.fp3, self.fp2, self.fp1)
        else:
            every = (self,) if not self.decoder_batch_stats else ()
        if any(m.training for m in every):
            raise NotImplementedError("pointnet_2_seg: forward_ragged / predict_ragged / predict_clouds are eval operations: call .eval() "
                                      "first (forward_ragged trains in a model built with the batch-statistics flags)")
        l0_rows = self._backbone_ragged(rows, sizes)[0]
        with torch.enable_grad() if self.decoder_grad and torch.is_grad_enabled() else torch.no_grad():
            return self._head._forward_rows(l0_rows.unsqueeze(0), want_preds=want_preds)

    def forward_ragged(self, rows, sizes):
        """rows [total, 9] float32 contiguous GPU = clouds of `sizes` points back to back, every one of >= sa1.npoint points
        -> log_probs [total, num_classes].  One launch sequence for all clouds, no host read-back.  Mode checks, graph rules and flags are
        forward_rows': in eval mode the rows of cloud b are the bits of forward_rows on that cloud alone, with decoder_grad=True and grad
        mode on they carry a graph, and in train mode (the batch-statistics flags) the model trains on the clouds as ONE batch -- every
        BatchNorm over all rows of the call, the dropout mask over `total` rows -- which is forward_rows' train mode when the clouds are of
        one size.  A model built without the flags never builds a graph, and its train mode raises NotImplementedError."""
        return self._ragged(rows, sizes, False)[0]

    def predict_ragged(self, rows, sizes):
        """forward_ragged's classes, int64 [total]: cloud by cloud the bits of predict_rows.  An eval operation, never a graph."""
        with torch.no_grad():
            return self._ragged(rows, sizes, True)[1].reshape(-1)

    def _predict_padded(self, rows, sizes):
        """predict_ragged for clouds of ANY size >= 1: a cloud below sa1.npoint points is padded on the device by repeating its rows
        cyclically (utils.pad_cloud_sizes) and the padding's predictions are dropped -> int64 [total]."""
        sizes = [int(n) for n in sizes]
        if not sizes or min(sizes) >= self.sa1.npoint:
            return self.predict_ragged(rows, sizes)
        if sum(sizes) != rows.shape[0]:
            raise _lib.AmpnetError(f"pointnet_2_seg: sizes (sum {sum(sizes)}) do not tile the {rows.shape[0]} rows")
        padded, _, gather, keep = U.pad_cloud_sizes(sizes, self.sa1.npoint)
        preds = self.predict_ragged(rows[torch.from_numpy(gather).to(rows.device, non_blocking=True)], padded)
        return preds[torch.from_numpy(keep).to(rows.device, non_blocking=True)]

    def predict_clouds(self, clouds):
        """clouds: a list of [n_i, >= 9] tensors (the first nine columns are the features; CPU or GPU) -> a list of int64 [n_i] GPU tensors,
        each the bits of predict_rows on that cloud alone.  A cloud with fewer than sa1.npoint points is padded by repeating its rows
        cyclically and the padding's predictions are dropped."""
        if not clouds:
            return []
        dev = self.conv1.weight.device
        sizes = [int(c.shape[0]) for c in clouds]
        rows = torch.cat([torch.as_tensor(c)[:, :9].float().to(dev, non_blocking=True) for c in clouds], dim=0).contiguous()
        return list(self._predict_padded(rows, sizes).split(sizes))
