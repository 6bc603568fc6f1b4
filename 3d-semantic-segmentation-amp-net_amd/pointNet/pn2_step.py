"""The per-batch step of pointnet_2_seg training / validation on the HIP path: what amp_step.train_loop is for AMP-Net and
gru_step.train_loop for the GRU variant, for the PointNet++ segmentation model (pointNet/model/pointnetAtt.py: pointnet_2_seg).  The
reference has no such step (its pointnet_2 carries the classifier commented out), so the argument list is this project's.

The batch is the k-means window dataset's: up to 9 windows of 2048 points per sample.  PointNet++ has no sequence model over the windows,
so every REAL window is one cloud of the batch:
  * the device input pipeline that already exists augments the batch (amp_step.augment_ragged_device / augment_batch_device: same draws
    from numpy's RNG, same order) and writes the point-major [B, W, N, 9] rows the blocks consume;
  * the padding windows (a sample with w_b < W windows is padded by replicating its last one, targets -1) are dropped: window (b, w) of
    the augmented batch is real iff cperm[w] < w_b, cperm being the cluster permutation the augmentation drew.  Kept, a replica would
    enter every BatchNorm statistic twice.  The selection is ONE index_select whose index tensor is built on the host from cperm and the
    window counts, so nothing synchronises;
  * pointnet_2_seg.forward_rows runs the six blocks and the head on the rows (no transpose in, no [Q, 128, N] copy out);
  * pointnet2_utils.seg_nll_loss gives the weighted loss, the predictions and the confusion counts in one pass;
  * backward() and optimizer.step() (trainer.FusedAdam).
train_loop_clouds is the same step on clouds of UNEQUAL size taken as they are (the clusters of a `<name>_clusters_list.pkl`), through
pointnet_2_seg.forward_ragged: no windows, no resampling; its input side is ONE kernel (cloud_input), which in train_loop_clouds_aug with
a CloudAugment also shuffles the points of every cloud and rotates the step's clouds about z.
The model is exact fp32: there is no `precision` argument.  With device_outputs=True (the default) nothing in the step waits for the GPU:
no .item(), no download, no data-dependent shape.

Data parallelism.  Under torch.distributed (trainer._collectives_on(): more than one rank, or one rank with AMPNET_FORCE_COLLECTIVES=1) a
train-mode step of both loops keeps its gradients in ONE flat float32 buffer (p.grad are views of it), all-reduces that buffer once after
backward() (trainer.reduce_gradients: SUM, 1 / world folded into FusedAdam.grad_scale) and then steps the optimiser, so every rank applies
the same update.  By default every rank's BatchNorm statistics and loss are its own batch's.  After trainer.enable_sync_batchnorm() the 17
train-mode BatchNorms take the statistics of the GLOBAL batch (one exchange per layer and direction inside the C library, csrc/bn_train.hip)
and the loss is the global batch's weighted mean (global_loss), which metrics['loss'] then reports on every rank: the step of N ranks is
the single-process step on the concatenated batch, except that every rank draws the dropout mask of its own rows from its own head.seed.
Without a process group nothing changes, bits included."""
import math

import numpy as np
import torch

from .. import _lib, trainer
from .amp_step import augment_batch_device, augment_ragged_device
from .collate_fns import CloudBatch, RaggedBatch
from .model.pointnet2_utils import seg_nll_loss

NUM_CLASSES = 5


def window_counts(pc_clusters, targets):
    """w_b, the number of real windows of every sample, as a Python list: from RaggedBatch.meta[:, 1], or from the padded targets [B, N, W]
    (a padding window holds -1 only).  Reads the values on the host: on device tensors this synchronises, so the drivers call it on the
    host copy, before the prefetcher, and hand the list to train_loop."""
    if isinstance(pc_clusters, RaggedBatch):
        return [int(w) for w in pc_clusters.meta[:, 1].tolist()]
    return [int(w) for w in (torch.as_tensor(targets) != -1).any(dim=1).sum(dim=1).tolist()]


def real_window_index(cperm, n_windows):
    """The flat indices b * W + w of the real windows of an augmented batch [B, W, ...], ascending: int64 host tensor [sum(w_b)]."""
    W = len(cperm)
    keep = np.asarray(cperm)[None, :] < np.asarray(n_windows, dtype=np.int64)[:, None]          # [B, W]
    return torch.from_numpy(np.arange(keep.size, dtype=np.int64)[keep.reshape(-1)])


class FlatGrads:
    """The data-parallel step's gradients: ONE flat float32 buffer with a 256-byte aligned view per trainable parameter, in the manner of
    trainer.GradStore, for a module whose backward runs through autograd (which adds into a p.grad that exists, in place)."""

    def __init__(self, module):
        self.params = [p for p in module.parameters() if p.requires_grad]
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.params[0].device)
        self.views = [self.flat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, self.params)]

    def matches(self, module):
        ps = [p for p in module.parameters() if p.requires_grad]
        return len(ps) == len(self.params) and all(a is b for a, b in zip(ps, self.params)) and ps[0].device == self.flat.device

    def zero_attach(self):
        """What optimizer.zero_grad() is for the plain step: zeroes the buffer and makes every p.grad its view again (set-to-None would
        drop the views)."""
        self.flat.zero_()
        for p, v in zip(self.params, self.views):
            p.grad = v


def _flat_grads(model):
    st = model.__dict__.get("_dp_grads")
    if st is None or not st.matches(model):
        st = FlatGrads(model)
        model.__dict__["_dp_grads"] = st
    return st


def loss_weight_sum(target, class_w, num_classes):
    """W of seg_nll_loss's weighted mean S / W: the sum of the class weights (1 without class_w) over the rows whose target is in
    [0, num_classes), float64 0-d on target's device.  Nothing synchronises."""
    live = (target >= 0) & (target < num_classes)
    if class_w is None:
        return live.sum().double()
    return (class_w.double()[target.clamp(0, num_classes - 1)] * live).sum()


def global_loss(loss, weight_sum):
    """The weighted-mean loss of the GLOBAL batch from every rank's own weighted mean `loss` = S_r / W_r and `weight_sum` = W_r (0-d
    tensors on one device, CPU tensors under gloo included) -> (sum_r S_r / sum_r W_r, world * W_r / sum_r W_r), both in loss's dtype.
    The second is the seed of this rank's backward(): d(global loss) / d(loss_r) is W_r / sum W, and the gradient all-reduce is followed
    by 1 / world.  One all-reduce of two float64 values; a rank without a live row (its loss is NaN, its W_r 0) contributes nothing.
    With one rank the pair is (loss, 1), bit for bit."""
    dist, world = trainer._dist_world()
    w = weight_sum.detach().double()
    pack = torch.stack([torch.where(w > 0, loss.detach().double() * w, torch.zeros_like(w)), w])
    dist.all_reduce(pack, op=dist.ReduceOp.SUM)
    return (pack[0] / pack[1]).to(loss.dtype), (world * w / pack[1]).to(loss.dtype)


def _train_pass(model, optimizer, class_w, forward, tg):
    """forward() -> log_probs, the loss against tg, backward(), optimizer.step() -> (the loss to report, preds, counts).  Plain without a
    process group; data parallel as the module's docstring says."""
    _, _, on = trainer._collectives_on()
    if not on:
        optimizer.zero_grad()
        loss, preds, counts = seg_nll_loss(forward(), tg, class_w, want_preds=True, want_counts=True)
        loss.backward()
        optimizer.step()
        return loss.detach(), preds, counts
    grads = _flat_grads(model)
    grads.zero_attach()
    sync = trainer._SYNC["on"]
    try:
        log_probs = forward()
        loss, preds, counts = seg_nll_loss(log_probs, tg, class_w, want_preds=True, want_counts=True)
        if sync:
            reported, seed = global_loss(loss, loss_weight_sum(tg, class_w, log_probs.shape[-1]))
            loss.backward(seed)
        else:
            reported = loss.detach()
            loss.backward()
    except Exception as e:
        # a collective that failed inside the C library's callback: the exception it kept says why, the library's status only that
        err = trainer._SYNC["state"]["error"] if sync else None
        if err is not None and err is not e:
            trainer._SYNC["state"]["error"] = None
            raise err from e
        raise
    trainer.reduce_gradients([grads.flat], (optimizer,))
    optimizer.step()
    return reported, preds, counts


def train_loop(data, optimizer, class_w, model, train=True, device_outputs=True):
    """One step on one batch -> (metrics {'loss'}, targets [Q, N], preds [Q, N], counts [C * C + 1]), Q = sum(w_b) the real windows.
    data: what collate_seq_ragged / collate_seq_padd return (pc_clusters, targets, filenames, centroids), optionally followed by the Python
    list n_windows (w_b per sample); without it the step counts on the host (window_counts).  class_w: float32 [C] GPU tensor or None.
    train=True: model.train(), forward, loss, backward(), optimizer.step(); else model.eval() under no_grad.  counts is
    utils.get_metrics.confusion_device's layout.  device_outputs=True: everything stays on the GPU and nothing synchronises;
    False: targets, preds and counts are downloaded.  Under torch.distributed a train-mode step is data parallel (the module's docstring)."""
    pc_clusters, targets = data[0], data[1]
    n_windows = data[4] if len(data) > 4 else window_counts(pc_clusters, targets)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.AmpnetError("the pointnet_2_seg HIP path needs the model on the GPU")
    model.train(train)
    if isinstance(pc_clusters, RaggedBatch):
        x, t, cperm = augment_ragged_device(pc_clusters, train, dev, return_perm=True)
    else:
        x, t, cperm = augment_batch_device(pc_clusters, targets, train, dev, return_perm=True)
    B, W, N, _ = x.shape
    if len(n_windows) != B or not all(1 <= w <= W for w in n_windows):
        raise _lib.AmpnetError(f"train_loop: n_windows must hold one count in [1, {W}] per sample of the batch ({B}), got {list(n_windows)}")
    idx = real_window_index(cperm, n_windows).to(dev, non_blocking=True)
    rows = x.view(B * W, N, 9).index_select(0, idx)                  # [Q, N, 9]
    tg = t.view(B * W, N).index_select(0, idx)                       # [Q, N]
    if train:
        loss, preds, counts = _train_pass(model, optimizer, class_w, lambda: model.forward_rows(rows), tg)
    else:
        with torch.no_grad():
            loss, preds, counts = seg_nll_loss(model.forward_rows(rows), tg, class_w, want_preds=True, want_counts=True)
    metrics = {'loss': loss.detach()}
    if device_outputs:
        return metrics, tg, preds, counts
    return metrics, tg.to('cpu'), preds.to('cpu'), counts.to('cpu')           # (the one place that waits for the GPU, on request)


def _mix32(x):
    """kernels.h: mix32 (the dropout hash) on a Python int."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def step_angle(seed, step):
    """The z-rotation angle of step `step` under `seed`: 2 pi * mix32(base ^ 0x3C6EF372) / 2^32, base = mix32(seed + step * 0x9E3779B9)
    (include/ampnet_hip.h: ampnet_cloud_input_f32).  A function of the two ints alone: nothing is drawn from numpy's or torch's RNG."""
    base = _mix32((int(seed) + int(step) * 0x9E3779B9) & 0xFFFFFFFF)
    return 2.0 * math.pi * _mix32(base ^ 0x3C6EF372) / 4294967296.0


class CloudAugment:
    """The augmentation state of train_loop_clouds_aug: two ints.  `seed` is fixed, `_step` advances by one per train-mode step (the convention
    of PointNetSegHead.seed / _step); step k shuffles the points of every cloud with the keyed bijection of ampnet_cloud_input_f32 and
    rotates all clouds about z by step_angle(seed, k) -- the reference's shuffle_data and rotate_point_cloud_z (one angle per step).  A run
    is reproducible from state_dict().  The shuffle is an augmentation shuffle, not a uniform sampler of permutations."""

    def __init__(self, seed=0x6A09E667):
        self.seed, self._step = int(seed) & 0xFFFFFFFF, 0

    def state_dict(self):
        return {'seed': self.seed, 'step': self._step}

    def load_state_dict(self, state):
        self.seed, self._step = int(state['seed']) & 0xFFFFFFFF, int(state['step'])


def _cloud_input(raw, sizes, npoint, train, seed, step, want_src):
    """cloud_input -> (rows, targets, the padded clouds as a utils.RaggedLayout -- its device table is the one the kernel read, so
    forward_ragged uploads none of its own --, src or None)."""
    from ..utils.utils import RaggedLayout
    _lib.require_gpu(raw, "raw")
    npoint = int(npoint)
    if raw.dim() != 2 or raw.shape[1] != 10 or raw.dtype != torch.float32 or not raw.is_contiguous():
        raise _lib.AmpnetError(f"cloud_input: expected raw contiguous [total, 10] float32, got {tuple(raw.shape)} {raw.dtype}")
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)                # (numpy from here on: the call is bound by its host side)
    if n.size == 0 or n.min() < 1 or n.sum() != raw.shape[0] or npoint < 1:
        raise _lib.AmpnetError(f"cloud_input: sizes (sum {int(n.sum())}, each >= 1) must tile the {raw.shape[0]} rows of raw, npoint={npoint} >= 1")
    p = np.maximum(n, npoint)
    total_out = int(p.sum())
    if total_out > 0x7fffffff:
        raise _lib.AmpnetError(f"cloud_input: {total_out} padded rows exceed 2^31 - 1")
    padded = p.tolist()
    off = np.zeros((2, n.size + 1), dtype=np.int32)
    np.cumsum(n, dtype=np.int32, out=off[0, 1:])
    np.cumsum(p, dtype=np.int32, out=off[1, 1:])
    off = torch.from_numpy(off).to(raw.device, non_blocking=True)
    rows = torch.empty((total_out, 9), dtype=torch.float32, device=raw.device)
    targets = torch.empty((total_out,), dtype=torch.int64, device=raw.device)
    src = torch.empty((total_out,), dtype=torch.int32, device=raw.device) if want_src else None
    angle = step_angle(seed, step) if train else 0.0
    _lib.cloud_input_f32(raw, off[0], off[1], seed, step, train, train, math.cos(angle), math.sin(angle), rows, targets, src)
    return rows, targets, RaggedLayout(padded, off[1]), src


def cloud_input(raw, sizes, npoint, *, train, seed, step, want_src=False):
    """The input side of train_loop_clouds in ONE launch (include/ampnet_hip.h: ampnet_cloud_input_f32)
    -> (rows [sum p_i, 9] f32, targets [sum p_i] int64, padded sizes [p_i][, src int32 [sum p_i]]).
    raw: [sum n_i, 10] float32 ON THE DEVICE, the clouds back to back (columns 0 .. 8 the features, column 9 the ASPRS class code); sizes:
    the n_i (host ints); npoint: every cloud below it is padded to p_i = max(n_i, npoint) by repeating its rows cyclically, targets -1 on
    the padding rows (utils.pad_cloud_sizes' rule).  The labels are amp_test._label_lut's.  train=True: the points of every cloud are
    shuffled by the bijection keyed with (seed, step, cloud) and x, y, z are rotated about z by step_angle(seed, step), bit for bit
    utils.rotate_point_cloud_z; train=False: neither, and rows / targets are what _upload_clusters + the pad_cloud_sizes gather give.
    want_src: also the row of `raw` behind every output row.  Both offset tables are built on the host and go up in one non-blocking
    copy: the call never waits for the GPU."""
    rows, targets, layout, src = _cloud_input(raw, sizes, npoint, train, seed, step, want_src)
    return (rows, targets, layout.sizes, src) if want_src else (rows, targets, layout.sizes)


def _upload_raw(clouds, device):
    """list of [n_i, >= 10] float tensors -> raw [sum n_i, 10] f32 on the device: one concatenation into amp_test's page-locked staging
    buffer, one asynchronous upload (the host half of amp_test._upload_clusters)."""
    from .amp_test import _STAGE, _Staging
    st = _STAGE.setdefault(str(device), _Staging())
    k, buf = st.take(sum(int(c.shape[0]) for c in clouds), 10)
    torch.cat([torch.as_tensor(c)[:, :10].float() for c in clouds], dim=0, out=buf)
    raw = buf.to(device, non_blocking=True)
    st.uploaded(k, device)
    return raw


def train_loop_clouds(clouds, optimizer, class_w, model, train=True, device_outputs=True):
    """One step on clouds of UNEQUAL size, as the cluster files (`<name>_clusters_list.pkl`) hold them
    -> (metrics {'loss'}, targets [sum n_i], preds [sum n_i], counts [C * C + 1]).
    clouds: a list of [n_i, >= 10] tensors, columns 0 .. 8 the features and column 9 the ASPRS class code -- one concatenation into
    page-locked memory, one upload -- or a collate_fns.CloudBatch; one that is on the device already (the DevicePrefetcher moved it) is
    taken as it is and the step uploads nothing but the clouds' offsets (one [2, Q + 1] table, which forward_ragged reads too) and, with a
    short cloud, the indices of the clouds' own rows.  ONE kernel (cloud_input) then writes the rows, the labels from the class-code
    column and the padding.  The clouds go through pointnet_2_seg.forward_ragged as ONE batch at their native sizes: no resampling to
    windows, one launch sequence, every BatchNorm over all rows of the call.  A cloud below sa1.npoint points is padded by repeating its
    rows cyclically (utils.pad_cloud_sizes' rule) with target -1 for the padding rows: the padding rows ENTER the BatchNorm statistics
    (they are rows of the call like any other, and farthest-point sampling needs them) but NOT the loss, the predictions returned or the
    counts' confusion cells (counts[-1], the ignored rows, counts them).  targets and preds come back without the padding, in the clouds'
    order.  No augmentation: the results are bit for bit those of the step before the kernel existed; train_loop_clouds_aug is this step
    with the keyword `augment`.
    The loss is pointnet2_utils.seg_nll_loss with class_w (float32 [C] GPU tensor or None).  train=True: model.train(), forward, loss,
    backward(), optimizer.step() -- the model needs the flags forward_rows' train mode needs; else model.eval() under no_grad.
    device_outputs=True: everything stays on the GPU and nothing in the step waits for it; False: targets, preds and counts are
    downloaded.  Under torch.distributed a train-mode step is data parallel (the module's docstring): one gradient all-reduce per step, and
    after trainer.enable_sync_batchnorm() the BatchNorm statistics and the loss of the global batch; with the nccl backend the step still
    never waits for the GPU."""
    return train_loop_clouds_aug(clouds, optimizer, class_w, model, train, device_outputs, augment=None)


def train_loop_clouds_aug(clouds, optimizer, class_w, model, train=True, device_outputs=True, *, augment=None):
    """train_loop_clouds with the device augmentation: the same arguments, results and rules, plus the keyword-only `augment` (the
    keyword lives here, not on train_loop_clouds, whose argument list is pinned).
    augment: None or a CloudAugment.  None: train_loop_clouds.  A CloudAugment with train=True: the points of every cloud are shuffled
    and all clouds rotated about z by the step's angle (cloud_input), then augment._step advances by one; with train=False nothing is
    augmented and _step stays.  targets and preds come back without the padding, cloud after cloud, and are consistent with each other;
    WITH augmentation they are in the AUGMENTED order of every cloud (row j of cloud b is the cloud's point perm_b(j);
    cloud_input(want_src=True) names it), not the file's."""
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.AmpnetError("the pointnet_2_seg HIP path needs the model on the GPU")
    if isinstance(clouds, CloudBatch):
        raw, sizes = clouds.raw.to(dev, non_blocking=True), clouds.sizes
    else:
        if not clouds or any(c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 10 for c in clouds):
            raise _lib.AmpnetError(f"train_loop_clouds: expected a list of [n_i >= 1, >= 10] tensors, got {[tuple(c.shape) for c in clouds]}")
        raw = _upload_raw(clouds, dev)
        sizes = [int(c.shape[0]) for c in clouds]
    if augment is not None and not isinstance(augment, CloudAugment):
        raise _lib.AmpnetError(f"train_loop_clouds_aug: augment must be None or a CloudAugment, got {type(augment).__name__}")
    model.train(train)
    aug = train and augment is not None
    rows, tg, layout, _ = _cloud_input(raw, sizes, model.sa1.npoint, aug, augment.seed if aug else 0, augment._step if aug else 0, False)
    if aug:
        augment._step += 1
    keep = None
    if layout.sizes != sizes:
        off = np.concatenate([[0], np.cumsum(layout.sizes)[:-1]]).astype(np.int64)
        keep = torch.from_numpy(np.concatenate([o + np.arange(n, dtype=np.int64) for o, n in zip(off, sizes)])).to(dev, non_blocking=True)
    sizes = layout                                                   # forward_ragged reads the table the kernel read: no second upload
    if train:
        loss, preds, counts = _train_pass(model, optimizer, class_w, lambda: model.forward_ragged(rows, sizes), tg)
    else:
        with torch.no_grad():
            loss, preds, counts = seg_nll_loss(model.forward_ragged(rows, sizes), tg, class_w, want_preds=True, want_counts=True)
    if keep is not None:
        tg, preds = tg[keep], preds[keep]
    metrics = {'loss': loss.detach()}
    if device_outputs:
        return metrics, tg, preds, counts
    return metrics, tg.to('cpu'), preds.to('cpu'), counts.to('cpu')           # (the one place that waits for the GPU, on request)
