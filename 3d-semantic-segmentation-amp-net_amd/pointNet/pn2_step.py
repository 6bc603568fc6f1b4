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
pointnet_2_seg.forward_ragged: no windows, no resampling, no augmentation.
The model is exact fp32: there is no `precision` argument.  With device_outputs=True (the default) nothing in the step waits for the GPU:
no .item(), no download, no data-dependent shape."""
import numpy as np
import torch

from .. import _lib
from .amp_step import augment_batch_device, augment_ragged_device
from .collate_fns import RaggedBatch
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


def train_loop(data, optimizer, class_w, model, train=True, device_outputs=True):
    """One step on one batch -> (metrics {'loss'}, targets [Q, N], preds [Q, N], counts [C * C + 1]), Q = sum(w_b) the real windows.
    data: what collate_seq_ragged / collate_seq_padd return (pc_clusters, targets, filenames, centroids), optionally followed by the Python
    list n_windows (w_b per sample); without it the step counts on the host (window_counts).  class_w: float32 [C] GPU tensor or None.
    train=True: model.train(), forward, loss, backward(), optimizer.step(); else model.eval() under no_grad.  counts is
    utils.get_metrics.confusion_device's layout.  device_outputs=True: everything stays on the GPU and nothing synchronises;
    False: targets, preds and counts are downloaded."""
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
        optimizer.zero_grad()
        log_probs = model.forward_rows(rows)
        loss, preds, counts = seg_nll_loss(log_probs, tg, class_w, want_preds=True, want_counts=True)
        loss.backward()
        optimizer.step()
    else:
        with torch.no_grad():
            loss, preds, counts = seg_nll_loss(model.forward_rows(rows), tg, class_w, want_preds=True, want_counts=True)
    metrics = {'loss': loss.detach()}
    if device_outputs:
        return metrics, tg, preds, counts
    return metrics, tg.to('cpu'), preds.to('cpu'), counts.to('cpu')           # (the one place that waits for the GPU, on request)


def train_loop_clouds(clouds, optimizer, class_w, model, train=True, device_outputs=True):
    """One step on clouds of UNEQUAL size, as the cluster files (`<name>_clusters_list.pkl`) hold them
    -> (metrics {'loss'}, targets [sum n_i], preds [sum n_i], counts [C * C + 1]).
    clouds: a list of [n_i, >= 10] tensors, columns 0 .. 8 the features and column 9 the ASPRS class code; one concatenation into
    page-locked memory, one upload, and the labels from the class-code column by one table look-up on the device
    (amp_test._upload_clusters).  The clouds go through pointnet_2_seg.forward_ragged as ONE batch at their native sizes: no resampling to
    windows, one launch sequence, every BatchNorm over all rows of the call.  A cloud below sa1.npoint points is padded by repeating its
    rows cyclically (utils.pad_cloud_sizes) with target -1 for the padding rows: the padding rows ENTER the BatchNorm statistics (they are
    rows of the call like any other, and farthest-point sampling needs them) but NOT the loss, the predictions returned or the counts'
    confusion cells (counts[-1], the ignored rows, counts them).  targets and preds come back without the padding, in the clouds' order.
    The loss is pointnet2_utils.seg_nll_loss with class_w (float32 [C] GPU tensor or None).  train=True: model.train(), forward, loss,
    backward(), optimizer.step() -- the model needs the flags forward_rows' train mode needs; else model.eval() under no_grad.
    device_outputs=True: everything stays on the GPU and nothing in the step waits for it; False: targets, preds and counts are
    downloaded.  Not built: augmentation of ragged clouds (the device pipeline is window-shaped), an epoch driver, data parallelism."""
    from .amp_test import _upload_clusters
    from ..utils import utils as U
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.AmpnetError("the pointnet_2_seg HIP path needs the model on the GPU")
    if not clouds or any(c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 10 for c in clouds):
        raise _lib.AmpnetError(f"train_loop_clouds: expected a list of [n_i >= 1, >= 10] tensors, got {[tuple(c.shape) for c in clouds]}")
    model.train(train)
    rows, tg, _ = _upload_clusters(clouds, dev)
    sizes = [int(c.shape[0]) for c in clouds]
    keep = None
    if min(sizes) < model.sa1.npoint:
        sizes, _, gather, keep = U.pad_cloud_sizes(sizes, model.sa1.npoint)
        own = np.zeros(len(gather), dtype=bool)
        own[keep] = True
        gather = torch.from_numpy(gather).to(dev, non_blocking=True)
        keep = torch.from_numpy(keep).to(dev, non_blocking=True)
        rows = rows[gather]
        tg = torch.where(torch.from_numpy(own).to(dev, non_blocking=True), tg[gather], -1)
    if train:
        optimizer.zero_grad()
        log_probs = model.forward_ragged(rows, sizes)
        loss, preds, counts = seg_nll_loss(log_probs, tg, class_w, want_preds=True, want_counts=True)
        loss.backward()
        optimizer.step()
    else:
        with torch.no_grad():
            loss, preds, counts = seg_nll_loss(model.forward_ragged(rows, sizes), tg, class_w, want_preds=True, want_counts=True)
    if keep is not None:
        tg, preds = tg[keep], preds[keep]
    metrics = {'loss': loss.detach()}
    if device_outputs:
        return metrics, tg, preds, counts
    return metrics, tg.to('cpu'), preds.to('cpu'), counts.to('cpu')           # (the one place that waits for the GPU, on request)
