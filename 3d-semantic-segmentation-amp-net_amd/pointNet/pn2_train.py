"""Training / inference drivers of the PointNet++ segmentation model (pointNet/model/pointnetAtt.py: pointnet_2_seg) on the HIP path: what
amp_train / amp_test are for AMP-Net and gru_train for the GRU variant.  The reference carries the model's classifier commented out and
has no driver for it; files read and written are those of the other two families.

  train_pn2  reads <path_list_files>/train_seg_files.txt, val_seg_files.txt and <dataset_folder>/kmeans_<name>.pt, trains
             pointnet_2_seg(5) with all five flags (from scratch: every BatchNorm on batch statistics, dropout in the head) on the REAL
             windows of every batch (pn2_step.train_loop), weighted NLL with class weights [1, 2, 2, 1, 1], ONE FusedAdam(lr), MultiStepLR
             milestones [150, 250, 350] gamma 0.5 stepped per epoch; writes pointNet/checkpoints/checkpoint_<name>.pth
             (utils.save_checkpoint: keys 'model', 'optimizer', ...) whenever the mean validation loss improves
  train_pn2_clouds  train_pn2's twin on the clusters of `<cluster_dir>/<name>_clusters_list.pkl` at their NATIVE sizes -- the clouds
             pn2_infer.test evaluates on: `files_per_step` files are one ragged batch (pn2_step.train_loop_clouds_aug), shuffled and rotated
             on the device (pn2_step.CloudAugment), validation without augmentation
  test       one file per step, clustered in situ with kmeans_clustering(pc, n_points, True, MAX_CLUSTERS = 18) as gru_train.test does;
             every cluster is one cloud of its own size (segment_file).

The model is exact fp32 (pointnet2_utils.py), so neither driver takes a `precision` argument.

Data parallelism: both training drivers read the launch from the environment, as amp_train.train_att does --
    python -m torch.distributed.run --nproc-per-node <GPUs> pointNet/<the CLI file> ...
starts one process per GPU (device cuda:LOCAL_RANK whatever `device` says, nccl).  The train and validation files are sharded by rank
(trainer.shard_indices: equal step counts), every step all-reduces the gradients once (pn2_step), rank 0 alone prints and writes
checkpoints, and every rank takes the same checkpoint decision because reduce_epoch_metrics gives all of them the same validation loss.
Default: every rank's BatchNorm statistics and loss are its own batch's; AMPNET_SYNC_BN=1 (trainer.enable_sync_batchnorm) makes both the
global batch's.  Each rank draws its own dropout masks (head seed + rank) and its own augmentation (CloudAugment(seed + rank))."""
import datetime
import os
import time

import numpy as np
import torch

from ..trainer import FusedAdam, enable_sync_batchnorm, shard_indices
from ..utils.get_metrics import get_accuracy, get_iou_obj, metrics_from_confusion
from ..utils.utils import get_labels, kmeans_clustering, limit_host_threads, save_checkpoint
from .amp_train import IOU_NAMES, _dist_setup, reduce_epoch_metrics, start_workers
from .collate_fns import collate_clouds, collate_seq_ragged
from .datasets import LidarClusterDataset, LidarDataset4Test, LidarKmeansDataset
from .model.pointnetAtt import pointnet_2_seg
from .pn2_step import NUM_CLASSES, CloudAugment, train_loop, train_loop_clouds_aug, window_counts
from .prefetch import DevicePrefetcher

MAX_CLUSTERS = 18
CLASS_KEYS = ['bckg', 'tower', 'cables', 'low_veg', 'high_veg']
TRAIN_FLAGS = dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True, head_batch_stats=True)


class _WithWindowCounts:
    """A loader whose batches carry, as a trailing Python list, the number of real windows of every sample -- read off the HOST copy, in
    front of the prefetcher (which passes lists through untouched), so the step never asks the device for it."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield tuple(batch) + (window_counts(batch[0], batch[1]),)


def _run_steps(batches, step, dev):
    """One pass: `step(batch)` -> (metrics, targets, preds, counts) for every prefetched batch; the loss and the confusion counts of every
    step stay queued on the device, ONE download per epoch."""
    sums = dict(loss=[], acc=[])
    ious = {k: [] for k in IOU_NAMES}
    counts, losses = [], []
    for data in DevicePrefetcher(batches, dev):
        metrics, _, _, c = step(data)
        counts.append(c)
        losses.append(metrics['loss'].reshape(()))
    if counts:
        counts_h, losses_h = torch.stack(counts).cpu().numpy(), torch.stack(losses).cpu().numpy()
        for c, l in zip(counts_h, losses_h):
            acc, per = metrics_from_confusion(c, NUM_CLASSES)
            sums['acc'].append(acc)
            for name, v in zip(IOU_NAMES, per):
                ious[name].append(v)
            sums['loss'].append(float(l))
    return reduce_epoch_metrics(sums, ious, device=dev)


def _epoch(loader, train, model, optimizer, class_w):
    """One pass over the window loader (pn2_step.train_loop on every batch)."""
    return _run_steps(_WithWindowCounts(loader), lambda data: train_loop(data, optimizer, class_w, model, train=train, device_outputs=True),
                      next(model.parameters()).device)


class _AsTuple:
    """A loader of CloudBatch objects as the 1-tuples the prefetcher moves entry by entry."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield (batch,)


def _epoch_clouds(loader, train, model, optimizer, class_w, augment):
    """One pass over the cluster loader (pn2_step.train_loop_clouds_aug on every batch; the CloudBatch arrives on the device)."""
    return _run_steps(_AsTuple(loader), lambda data: train_loop_clouds_aug(data[0], optimizer, class_w, model, train=train,
                                                                           device_outputs=True, augment=augment), next(model.parameters()).device)


def _launch(device):
    """The launch from the environment -> (rank, world, device): one process, `device` as given; under torch.distributed.run the process
    group (amp_train._dist_setup), cuda:LOCAL_RANK and, with AMPNET_SYNC_BN=1, global-batch BatchNorm."""
    rank, world, local = _dist_setup()
    if world > 1:
        device = torch.device('cuda', local)
        if os.environ.get("AMPNET_SYNC_BN") == "1":
            enable_sync_batchnorm()
    return rank, world, torch.device(device)


def _shard(files, rank, world):
    return [files[i] for i in shard_indices(len(files), rank, world)] if world > 1 else files


def _same_start(model, rank, world):
    """Every rank its own dropout masks (head seed + rank) and, from rank 0, the same parameters and buffers."""
    model._head.seed = (model._head.seed + rank) & 0xFFFFFFFF
    if world > 1:
        import torch.distributed as dist
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t.data, src=0)


def train_pn2(dataset_folder, path_list_files, output_folder, n_points, batch_size, epochs, learning_rate, number_of_workers=4,
              model_checkpoint=None, device='cuda'):
    """Trains pointnet_2_seg(5) from scratch (or from `model_checkpoint`, a file this function wrote) on the k-means window dataset and
    returns the per-epoch history [(train metrics, validation metrics)].  Exact fp32: no `precision` argument.  Data parallel under
    `python -m torch.distributed.run` (the module's docstring): files sharded by rank, `batch_size` per rank."""
    start = time.time()
    rank, world, device = _launch(device)
    limit_host_threads(reserve=number_of_workers)
    with open(os.path.join(path_list_files, 'train_seg_files.txt')) as f:
        train_files = _shard(f.read().splitlines(), rank, world)
    with open(os.path.join(path_list_files, 'val_seg_files.txt')) as f:
        val_files = _shard(f.read().splitlines(), rank, world)
    name = 'PN2seg' + str(n_points)
    train_ds = LidarKmeansDataset(dataset_folder, task='segmentation', number_of_points=n_points, files=train_files, lazy=True)
    val_ds = LidarKmeansDataset(dataset_folder, task='segmentation', number_of_points=n_points, files=val_files, lazy=True)
    # persistent workers, forked before the first pinned batch exists (amp_train.start_workers: a later fork stalls the GPU queues)
    mk = lambda ds: torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=True, num_workers=number_of_workers,   # noqa: E731
                                                drop_last=True, collate_fn=collate_seq_ragged, pin_memory=True,
                                                persistent_workers=number_of_workers > 0)
    train_loader, val_loader = mk(train_ds), mk(val_ds)
    start_workers(val_loader, train_loader)
    if rank == 0:
        print(f'Dataset folder: {dataset_folder}\nSamples for training: {len(train_ds)}\nSamples for validation: {len(val_ds)}'
              + (f' (per rank, {world} ranks)' if world > 1 else ''))
    model = pointnet_2_seg(NUM_CLASSES, device=device, **TRAIN_FLAGS)
    class_w = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=device)
    optimizer = FusedAdam(model.parameters(), lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[150, 250, 350], gamma=0.5)
    if rank == 0:
        print(f"Total Trainable Params: {sum(p.numel() for p in model.parameters())}")
    best_vloss, epoch_ini, since = 1_000_000., 0, 0
    if model_checkpoint:
        ck = torch.load(model_checkpoint, map_location=device, weights_only=True)
        model.load_state_dict(ck['model'])
        optimizer.load_state_dict(ck['optimizer'])
        epoch_ini = ck['epoch']
    _same_start(model, rank, world)
    history = []
    for epoch in range(epoch_ini, epochs):
        t0 = time.time()
        tr = _epoch(train_loader, True, model, optimizer, class_w)
        va = _epoch(val_loader, False, model, optimizer, class_w)
        scheduler.step()
        history.append((tr, va))
        if rank == 0:
            print(f"epoch {epoch}: train loss {tr['loss']:.4f} acc {tr['acc']:.3f} | val loss {va['loss']:.4f} acc {va['acc']:.3f} "
                  f"iou tower {va['iou_tower']:.3f} | {time.time() - t0:.1f} s", flush=True)
        if va['loss'] < best_vloss:
            best_vloss, since = va['loss'], 0
            if rank == 0:
                stamp = datetime.datetime.now().strftime("%m-%d-%H:%M")
                save_checkpoint(stamp + name, epoch, since, model, optimizer, va['acc'], batch_size, learning_rate, n_points)
        else:
            since += 1
    if rank == 0:
        print("--- TOTAL TIME: %s h ---" % (round((time.time() - start) / 3600, 3)))
    return history


def train_pn2_clouds(cluster_dir, path_list_files, output_folder, files_per_step, epochs, learning_rate, number_of_workers=4,
                     model_checkpoint=None, device='cuda', allow_pickle=None, seed=0x6A09E667):
    """train_pn2 on clusters of NATIVE size: reads <path_list_files>/train_seg_files.txt, val_seg_files.txt and
    `<cluster_dir>/<name>_clusters_list.pkl` (datasets.LidarClusterDataset), trains pointnet_2_seg(5) with all five flags; the clusters
    of `files_per_step` files are ONE ragged batch (pn2_step.train_loop_clouds_aug, every BatchNorm over all its rows).  The same class
    weights, FusedAdam, MultiStepLR and checkpoint keys as train_pn2 (utils.save_checkpoint; 'batch_size' holds files_per_step,
    'number_of_points' None -- the clouds keep their sizes -- and 'weighing_method', the free slot, {'cloud_augment': the two ints of
    the augmentation}, so a run continued from `model_checkpoint` draws the steps the uninterrupted run would have drawn).  Train steps
    shuffle the points of every cloud and rotate the batch about z on the device (pn2_step.CloudAugment(seed): a function of
    (seed, step), nothing is drawn from numpy's or torch's RNG); validation is not augmented.  Returns the per-epoch history
    [(train metrics, validation metrics)].  The checkpoint loads into a default pointnet_2_seg(5) and into pn2_infer.test.  Exact fp32:
    no `precision` argument.  Data parallel under `python -m torch.distributed.run` (the module's docstring): files sharded by rank,
    `files_per_step` files per rank and step, rank r augmenting with CloudAugment(seed + r)."""
    start = time.time()
    rank, world, device = _launch(device)
    limit_host_threads(reserve=number_of_workers)
    with open(os.path.join(path_list_files, 'train_seg_files.txt')) as f:
        train_files = _shard(f.read().splitlines(), rank, world)
    with open(os.path.join(path_list_files, 'val_seg_files.txt')) as f:
        val_files = _shard(f.read().splitlines(), rank, world)
    train_ds = LidarClusterDataset(cluster_dir, train_files, allow_pickle=allow_pickle)
    val_ds = LidarClusterDataset(cluster_dir, val_files, allow_pickle=allow_pickle)
    # persistent workers, forked before the first pinned batch exists (amp_train.start_workers: a later fork stalls the GPU queues)
    mk = lambda ds, train: torch.utils.data.DataLoader(ds, batch_size=files_per_step, shuffle=train, num_workers=number_of_workers,  # noqa: E731
                                                       drop_last=train, collate_fn=collate_clouds, pin_memory=True,
                                                       persistent_workers=number_of_workers > 0)
    train_loader, val_loader = mk(train_ds, True), mk(val_ds, False)
    start_workers(val_loader, train_loader)
    if rank == 0:
        print(f'Cluster folder: {cluster_dir}\nFiles for training: {len(train_ds)}\nFiles for validation: {len(val_ds)}'
              + (f' (per rank, {world} ranks)' if world > 1 else ''))
    model = pointnet_2_seg(NUM_CLASSES, device=device, **TRAIN_FLAGS)
    class_w = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=device)
    optimizer = FusedAdam(model.parameters(), lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[150, 250, 350], gamma=0.5)
    augment = CloudAugment(seed)
    if rank == 0:
        print(f"Total Trainable Params: {sum(p.numel() for p in model.parameters())}")
    best_vloss, epoch_ini, since = 1_000_000., 0, 0
    if model_checkpoint:
        ck = torch.load(model_checkpoint, map_location=device, weights_only=True)
        model.load_state_dict(ck['model'])
        optimizer.load_state_dict(ck['optimizer'])
        epoch_ini = ck['epoch']
        if isinstance(ck.get('weighing_method'), dict) and 'cloud_augment' in ck['weighing_method']:
            augment.load_state_dict(ck['weighing_method']['cloud_augment'])
    augment.seed = (augment.seed + rank) & 0xFFFFFFFF             # data parallel: every rank its own shuffles and angles
    _same_start(model, rank, world)
    history = []
    for epoch in range(epoch_ini, epochs):
        t0 = time.time()
        tr = _epoch_clouds(train_loader, True, model, optimizer, class_w, augment)
        va = _epoch_clouds(val_loader, False, model, optimizer, class_w, None)
        scheduler.step()
        history.append((tr, va))
        if rank == 0:
            print(f"epoch {epoch}: train loss {tr['loss']:.4f} acc {tr['acc']:.3f} | val loss {va['loss']:.4f} acc {va['acc']:.3f} "
                  f"iou tower {va['iou_tower']:.3f} | {time.time() - t0:.1f} s", flush=True)
        if va['loss'] < best_vloss:
            best_vloss, since = va['loss'], 0
            if rank == 0:
                stamp = datetime.datetime.now().strftime("%m-%d-%H:%M")
                save_checkpoint(stamp + 'PN2segClouds', epoch, since, model, optimizer, va['acc'], files_per_step, learning_rate, None,
                                weighing_method={'cloud_augment': augment.state_dict()})   # (rank 0's: the seed as given)
        else:
            since += 1
    if rank == 0:
        print("--- TOTAL TIME: %s h ---" % (round((time.time() - start) / 3600, 3)))
    return history


def segment_file(model, clusters_list, device):
    """clusters_list: list of [n_i, >= 10] tensors (cols 0..8 features, col 9 class code) -> (preds [sum n_i] cpu, targets [sum n_i] cpu),
    in the list's order.  Every cluster is one cloud of its own size; clusters of equal size share one predict_rows call.  A cluster with
    fewer points than sa1.npoint (the centres farthest-point sampling has to find) is padded by repeating its rows cyclically, and the
    padding's predictions are dropped."""
    targets = torch.cat(get_labels([c.clone() for c in clusters_list]), dim=0)
    by_size = {}
    for i, c in enumerate(clusters_list):
        by_size.setdefault(int(c.shape[0]), []).append(i)
    preds = [None] * len(clusters_list)
    for n, members in by_size.items():
        rows = torch.stack([torch.as_tensor(clusters_list[i])[:, :9].float() for i in members], dim=0).to(device)      # [k, n, 9]
        if n < model.sa1.npoint:
            rows = rows[:, torch.arange(model.sa1.npoint, device=rows.device) % n]
        out = model.predict_rows(rows.contiguous())[:, :n].cpu()
        for i, p in zip(members, out):
            preds[i] = p
    return torch.cat(preds, dim=0).reshape(-1), targets.reshape(-1)


def test(dataset_folder, output_folder, n_points, number_of_workers, model_checkpoint, path_list_files, device='cuda', allow_pickle=None):
    """Per-file accuracy and per-class IoU of a train_pn2 checkpoint over <path_list_files>/test_seg_files.txt; appends the CSV row of
    gru_train.test and returns its dict.  Exact fp32: no `precision` argument."""
    start = time.time()
    device = torch.device(device)
    checkpoint = torch.load(model_checkpoint, map_location=device, weights_only=True)
    with open(os.path.join(path_list_files, 'test_seg_files.txt')) as f:
        test_files = f.read().splitlines()
    ds = LidarDataset4Test(dataset_folder, task='segmentation', number_of_points=n_points, files=test_files, fixed_num_points=False,
                           allow_pickle=allow_pickle)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=number_of_workers, drop_last=False)
    model = pointnet_2_seg(NUM_CLASSES, device=device)
    model.load_state_dict(checkpoint['model'])
    model.eval()
    total_params = sum(p.numel() for p in model.parameters())
    print(f"Total Trainable Params: {total_params}")
    iou = {k: [] for k in CLASS_KEYS}
    accuracy = []
    for pc, file_name in loader:
        clusters_list, _ = kmeans_clustering(pc, n_points=n_points, get_centroids=True, max_clusters=MAX_CLUSTERS)
        preds, targets = segment_file(model, clusters_list, device)
        accuracy.append(get_accuracy(preds.numpy(), targets.numpy(), {}, 'segmentation')['accuracy'])
        present = set(targets.numpy().reshape(-1).tolist())
        for c, k in enumerate(CLASS_KEYS):
            if c in present:
                iou[k].append(get_iou_obj(preds, targets, c))
    iou_arr = [np.mean(iou['tower']), np.mean(iou['low_veg']), np.mean(iou['high_veg']), np.mean(iou['bckg']), np.mean(iou['cables'])]
    mean_iou = float(np.mean(iou_arr))
    print('mean_iou: ', mean_iou, ' accuracy: ', float(np.mean(accuracy)))
    minutes = round((time.time() - start) / 60, 3)
    print("--- TOTAL TIME: %s min ---" % minutes)
    model_name = model_checkpoint.split('/')[-1].split('.')[0]
    os.makedirs(output_folder, exist_ok=True)
    with open(os.path.join(os.path.dirname(output_folder.rstrip('/')) or '.', 'IoU-results-v2.csv'), 'a') as fid:
        fid.write('%s,%s,%s,%s,%s,%s,%s,%s,%s,%s,%s\n' % (
            model_name, n_points, round(float(np.mean(iou['tower'])), 3), round(float(np.mean(iou['low_veg'])), 3),
            round(float(np.mean(iou['high_veg'])), 3), round(float(np.mean(iou['cables'])), 3), round(float(np.mean(iou['bckg'])), 3),
            round(mean_iou, 4), round(float(np.mean(accuracy)), 3), total_params, minutes))
    return dict(mean_iou=mean_iou, accuracy=float(np.mean(accuracy)), iou={k: float(np.mean(v)) if v else float('nan') for k, v in iou.items()})
