"""Inference driver of the PointNet++ segmentation model (pointNet/model/pointnetAtt.py: pointnet_2_seg) for clouds of UNEQUAL size: what
amp_test is for AMP-Net.  pn2_train.segment_file runs the whole network once per distinct cluster size -- up to 18 passes per file, each
with a host read-back in its ball query -- and pn2_train.test clusters every file in situ and forms the metrics on the host, file by file.
Here

  segment_file   all clusters of a file are ONE ragged launch sequence (pointnet_2_seg.predict_ragged: ragged FPS, ragged ball query, the
                 fused blocks on the packed rows, ragged 3-NN, the head), without a host read-back;
  segment_files  all clusters of SEVERAL files are one such sequence;
  test           reads the precomputed clusters `<cluster_dir>/<name>_clusters_list.pkl` (as amp_test.test does; synthetic.write_dataset and
                 utils.kmeans_clustering write them), keeps predictions and labels on the device, queues one confusion count per file
                 and downloads the counts ONCE; the CSV row and the returned dict are pn2_train.test's.

Predictions are bit for bit those of pn2_train.segment_file on the same clusters (tests/test_pn2_ragged_gpu.py).  Staging, upload, the
label table and the download are amp_test's.  The model is exact fp32: no `precision` argument."""
import os
import time

import numpy as np
import torch

from .amp_test import CLASS_KEYS, _download, _load_list, _upload_clusters
from .model.pointnetAtt import pointnet_2_seg

NUM_CLASSES = 5


def _segment(model, cluster_tensors, device, device_outputs):
    """All clusters as one ragged call -> (preds, targets) int64 [sum n_i], on the device or downloaded."""
    device = torch.device(device)
    sizes = [int(c.shape[0]) for c in cluster_tensors]
    rows, targets, slot = _upload_clusters(cluster_tensors, device)
    preds = model._predict_padded(rows, sizes)
    if device_outputs:
        return preds, targets
    return _download(preds, targets, slot, device)


def segment_file(model, clusters_list, device, device_outputs=False):
    """clusters_list: list of [n_i, >= 10] tensors (cols 0..8 features, col 9 class code) -> (preds [sum n_i] int64, targets [sum n_i]
    int64) in the list's order, on the CPU, or left on the device without any synchronisation (device_outputs=True).  ONE ragged call for
    the whole file, whatever the clusters' sizes; a cluster with fewer points than sa1.npoint is padded by repeating its rows cyclically
    and the padding's predictions are dropped, as pn2_train.segment_file does: the predictions are the same bits."""
    return _segment(model, clusters_list, device, device_outputs)


def segment_files(model, files, device, device_outputs=False):
    """files: a list of clusters_lists as segment_file takes them -> a list of (preds, targets) per file, identical to segment_file's file
    by file (an eval forward: nothing a cloud computes depends on its neighbours).  All clusters of all files are ONE ragged call, one
    upload and one download."""
    if not files:
        return []
    preds, targets = _segment(model, [c for cl in files for c in cl], device, device_outputs)
    out, r0 = [], 0
    for cl in files:
        n = sum(int(c.shape[0]) for c in cl)
        out.append((preds[r0:r0 + n], targets[r0:r0 + n]))
        r0 += n
    return out


def test(dataset_path, out_path, n_points, number_of_workers, model_checkpoint, path_list_files, cluster_dir='k_means_25', device='cuda',
         allow_pickle=None, files_per_launch=1):
    """Per-file accuracy and per-class IoU of a train_pn2 checkpoint over <path_list_files>/test_seg_files.txt, from the precomputed
    clusters in `cluster_dir`; appends the CSV row of pn2_train.test and returns its dict.  files_per_launch: how many files share one
    launch sequence (segment_files); the per-file metrics, their order and the CSV row are the same for any value.  Only the cluster files
    are read -- the point clouds under `dataset_path` are not, so there is no loader and `number_of_workers` has nothing to start; both
    parameters keep the signature of the other test drivers."""
    from ..utils.get_metrics import confusion_device, metrics_from_confusion
    start = time.time()
    device = torch.device(device)
    checkpoint = torch.load(model_checkpoint, map_location=device, weights_only=True)
    with open(os.path.join(path_list_files, 'test_seg_files.txt')) as f:
        test_files = f.read().splitlines()
    model = pointnet_2_seg(NUM_CLASSES, device=device)
    model.load_state_dict(checkpoint['model'])
    model.eval()
    total_params = sum(p.numel() for p in model.parameters())
    print(f"Total Trainable Params: {total_params}")

    def results():
        group = []
        for file_name in test_files:
            name = file_name.split('/')[-1].split('.')[0]
            clusters = _load_list(os.path.join(cluster_dir, name + '_clusters_list.pkl'), allow_pickle)
            if files_per_launch <= 1:
                yield segment_file(model, clusters, device, device_outputs=True)
                continue
            group.append(clusters)
            if len(group) == files_per_launch:
                yield from segment_files(model, group, device, device_outputs=True)
                group = []
        if group:
            yield from segment_files(model, group, device, device_outputs=True)

    # one confusion-count kernel per file queued behind its forward, ONE download per run; accuracy and IoU are the float32 quotients of
    # those integers (utils/get_metrics.py: metrics_from_confusion, bit-identical to get_accuracy / get_iou_obj); a class enters a file's
    # IoU only if the file's TARGETS hold it, as in pn2_train.test
    counts = [confusion_device(preds, targets, NUM_CLASSES) for preds, targets in results()]
    counts_h = torch.stack(counts).cpu().numpy() if counts else np.zeros((0, NUM_CLASSES * NUM_CLASSES + 1), dtype=np.int64)
    iou = {k: [] for k in CLASS_KEYS}
    accuracy = []
    for c in counts_h:
        acc, per = metrics_from_confusion(c, NUM_CLASSES)
        accuracy.append(acc)
        in_targets = c[:NUM_CLASSES * NUM_CLASSES].reshape(NUM_CLASSES, NUM_CLASSES).sum(axis=1) > 0
        for k, key in enumerate(CLASS_KEYS):
            if in_targets[k]:
                iou[key].append(per[k])
    iou_arr = [np.mean(iou['tower']), np.mean(iou['low_veg']), np.mean(iou['high_veg']), np.mean(iou['bckg']), np.mean(iou['cables'])]
    mean_iou = float(np.mean(iou_arr))
    print('mean_iou: ', mean_iou, ' accuracy: ', float(np.mean(accuracy)))
    minutes = round((time.time() - start) / 60, 3)
    print("--- TOTAL TIME: %s min ---" % minutes)
    model_name = model_checkpoint.split('/')[-1].split('.')[0]
    os.makedirs(out_path, exist_ok=True)
    with open(os.path.join(os.path.dirname(out_path.rstrip('/')) or '.', 'IoU-results-v2.csv'), 'a') as fid:
        fid.write('%s,%s,%s,%s,%s,%s,%s,%s,%s,%s,%s\n' % (
            model_name, n_points, round(float(np.mean(iou['tower'])), 3), round(float(np.mean(iou['low_veg'])), 3),
            round(float(np.mean(iou['high_veg'])), 3), round(float(np.mean(iou['cables'])), 3), round(float(np.mean(iou['bckg'])), 3),
            round(mean_iou, 4), round(float(np.mean(accuracy)), 3), total_params, minutes))
    return dict(mean_iou=mean_iou, accuracy=float(np.mean(accuracy)), iou={k: float(np.mean(v)) if v else float('nan') for k, v in iou.items()})
