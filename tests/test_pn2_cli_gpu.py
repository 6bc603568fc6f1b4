"""The pointnet_2_seg drivers end to end on the GPU, on a synthetic dataset in the reference's on-disk formats: one pn2_step.train_loop call
against the same step composed by hand, train_pn2 (the loss goes down, the checkpoint has utils.save_checkpoint's keys and loads into a
default model), then test() on that checkpoint against numpy metrics recomputed from predict() on the same clusters, one per call."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu

EPOCHS = 4
KEYS = ("bckg", "tower", "cables", "low_veg", "high_veg")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("pn2")
    return root, sub("synthetic").write_dataset(str(root), n_train=8, n_val=4, n_test=2, n_points=2048, seed=902)


@pytest.fixture(scope="module")
def trained(dataset):
    """train_pn2 once for the module: (history, checkpoint path, test()'s result), run from the dataset's folder (checkpoints are written
    relative to the working directory, as the other drivers write theirs)."""
    root, paths = dataset
    T = sub("pointNet.pn2_train")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        hist = T.train_pn2(paths["data"], paths["lists"], str(root / "out"), 2048, 4, EPOCHS, 1e-3, number_of_workers=0)
        cks = sorted(os.listdir("pointNet/checkpoints"))
        assert cks
        ck_path = os.path.abspath(os.path.join("pointNet/checkpoints", cks[-1]))
        res = T.test(paths["data"], str(root / "res" / "preds"), 2048, 0, ck_path, paths["lists"])
    finally:
        os.chdir(cwd)
    return hist, ck_path, res


def _batch(paths, collate, lazy):
    """The first four training samples, collated; the resampling to 2048 points draws from torch's RNG, seeded here so that both collates
    draw alike."""
    D = sub("pointNet.datasets")
    torch.manual_seed(21)
    files = open(os.path.join(paths["lists"], "train_seg_files.txt")).read().split()[:4]
    ds = D.LidarKmeansDataset(paths["data"], task="segmentation", number_of_points=2048, files=files, lazy=lazy)
    return collate([ds[i] for i in range(4)])


def test_one_step_equals_the_step_composed_by_hand(dataset):
    _, paths = dataset
    A, S, U = sub("pointNet.model.pointnetAtt"), sub("pointNet.pn2_step"), sub("pointNet.model.pointnet2_utils")
    C, T, P = sub("pointNet.collate_fns"), sub("trainer"), sub("pointNet.pn2_train")
    batch = _batch(paths, C.collate_seq_ragged, lazy=True)
    w_b = S.window_counts(batch[0], batch[1])
    B, W, N = 4, C.MAX_WINDOWS, 2048
    assert len(w_b) == B and all(1 <= w <= 5 for w in w_b) and sum(w_b) < B * W          # max_w = 5 < 9: the batch holds padded windows
    torch.manual_seed(5)
    one = A.pointnet_2_seg(5, **P.TRAIN_FLAGS)
    two = A.pointnet_2_seg(5, **P.TRAIN_FLAGS)
    two.load_state_dict(one.state_dict())
    cw = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device="cuda")
    opt1, opt2 = T.FusedAdam(one.parameters(), lr=1e-3), T.FusedAdam(two.parameters(), lr=1e-3)
    # the step
    np.random.seed(11)
    metrics, targets, preds, counts = S.train_loop(batch + (w_b,), opt1, cw, one, train=True)
    assert set(metrics) == {"loss"} and metrics["loss"].is_cuda and targets.is_cuda and preds.is_cuda and counts.is_cuda
    # the same step by hand
    np.random.seed(11)
    x, t, cperm = sub("pointNet.amp_step").augment_ragged_device(batch[0], True, "cuda", return_perm=True)
    idx = torch.tensor([b * W + w for b in range(B) for w in range(W) if cperm[w] < w_b[b]], device="cuda")
    rows, tg = x.view(B * W, N, 9)[idx].contiguous(), t.view(B * W, N)[idx].contiguous()
    assert (tg != -1).any(dim=1).all()                               # every kept window is real ...
    dropped = torch.ones(B * W, dtype=torch.bool, device="cuda")
    dropped[idx] = False
    assert (t.view(B * W, N)[dropped] == -1).all()                   # ... and every dropped one is padding
    two.train()
    opt2.zero_grad()
    loss, p2, c2 = U.seg_nll_loss(two.forward_rows(rows), tg, cw, want_preds=True, want_counts=True)
    loss.backward()
    opt2.step()
    assert torch.equal(metrics["loss"], loss.detach()) and torch.equal(preds, p2) and torch.equal(counts, c2) and torch.equal(targets, tg)
    params = dict(two.named_parameters())
    for k, p in one.named_parameters():
        assert torch.equal(p, params[k]), k
    buffers = dict(two.named_buffers())
    for k, v in one.named_buffers():
        assert torch.equal(v, buffers[k]), k
    # the model saw exactly sum(w_b) windows, once
    assert targets.shape == (sum(w_b), N) and int(counts.sum()) == sum(w_b) * N and int(counts[25]) == 0
    assert int(one.bn1.num_batches_tracked) == int(two.bn1.num_batches_tracked) == 1 and int(one.sa1.mlp_bns[0].num_batches_tracked) == 1
    # without the list the step counts the windows itself; eval mode; the padded collate gives the same batch
    np.random.seed(12)
    m_e, t_e, p_e, c_e = S.train_loop(batch, opt1, cw, one, train=False)
    assert not one.training and int(one.bn1.num_batches_tracked) == 1 and not m_e["loss"].requires_grad
    np.random.seed(12)
    m_p, t_p, p_p, c_p = S.train_loop(_batch(paths, C.collate_seq_padd, lazy=False), opt1, cw, one, train=False, device_outputs=False)
    assert torch.equal(m_e["loss"], m_p["loss"]) and not t_p.is_cuda and torch.equal(t_e.cpu(), t_p) and torch.equal(p_e.cpu(), p_p)
    assert torch.equal(c_e.cpu(), c_p)
    acc, ious = sub("utils.get_metrics").metrics_from_confusion(c_p.numpy(), 5)
    assert abs(acc - float((p_p == t_p).float().mean())) < 1e-6 and len(ious) == 5


def test_training_lowers_the_loss_and_writes_a_loadable_checkpoint(trained):
    """Four epochs of two steps each (batch 4, lr 1e-3, seeds 0).  Observed on an MI355X, mean train loss per epoch: 1.7214, 1.4740, 1.3131,
    1.2075 (validation 1.6679, 1.6490, 1.6271, 1.6071): the last epoch is 0.51 below the first, so four epochs leave room to spare.  (The
    validation ACCURACY is poor after eight steps -- the running statistics of 17 BatchNorms have barely moved from their initial values --
    which is why the test asks for the train loss and for nothing about quality.)"""
    hist, ck_path, _ = trained
    losses = [tr["loss"] for tr, _ in hist]
    print("train_pn2 mean train loss per epoch:", ", ".join(f"{l:.4f}" for l in losses),
          "| validation:", ", ".join(f"{va['loss']:.4f}" for _, va in hist))
    assert len(hist) == EPOCHS and all(np.isfinite(losses)) and losses[-1] < losses[0]
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert set(ck) == {"model", "optimizer", "batch_size", "lr", "number_of_points", "epoch", "epochs_since_improvement", "accuracy",
                       "weighing_method"}
    assert (ck["batch_size"], ck["lr"], ck["number_of_points"]) == (4, 1e-3, 2048)
    plain = sub("pointNet.model.pointnetAtt").pointnet_2_seg(5)
    plain.load_state_dict(ck["model"], strict=True)
    assert int(plain.bn1.num_batches_tracked) > 0


def test_test_driver_reports_the_metrics_of_predict_on_the_same_clusters(dataset, trained):
    root, paths = dataset
    _, ck_path, res = trained
    assert os.path.exists(root / "res" / "IoU-results-v2.csv")
    row = open(root / "res" / "IoU-results-v2.csv").read().strip().split("\n")[-1].split(",")
    assert len(row) == 11 and row[0] == os.path.basename(ck_path).split(".")[0] and row[1] == "2048"
    T, U = sub("pointNet.pn2_train"), sub("utils.utils")
    model = sub("pointNet.model.pointnetAtt").pointnet_2_seg(5).eval()
    model.load_state_dict(torch.load(ck_path, map_location="cuda", weights_only=True)["model"])
    ds = sub("pointNet.datasets").LidarDataset4Test(paths["data"], task="segmentation", number_of_points=2048,
                                                    files=open(os.path.join(paths["lists"], "test_seg_files.txt")).read().split(),
                                                    fixed_num_points=False)
    accs, ious = [], {k: [] for k in KEYS}
    for i in range(len(ds)):
        pc, _ = ds[i]
        clusters, _ = U.kmeans_clustering(torch.as_tensor(pc)[None], n_points=2048, get_centroids=True, max_clusters=T.MAX_CLUSTERS)
        preds = np.concatenate([model.predict(c[None, :, :9].float().cuda().transpose(1, 2).contiguous()).cpu().numpy().reshape(-1)
                                for c in clusters])
        tg = torch.cat(U.get_labels([c.clone() for c in clusters])).numpy()
        accs.append(float(np.float32((preds == tg).sum()) / np.float32(len(tg))))
        for c, k in enumerate(KEYS):
            if (tg == c).any():
                tp = np.logical_and(preds == c, tg == c).sum()
                ious[k].append(float(np.float32(tp) / np.float32((tg == c).sum() + (preds == c).sum() - tp)))
    assert abs(res["accuracy"] - float(np.mean(accs))) < 2e-4
    for k, v in ious.items():
        want = float(np.mean(v)) if v else float("nan")
        assert (np.isnan(want) and np.isnan(res["iou"][k])) or abs(res["iou"][k] - want) < 1e-3, (k, res["iou"][k], want)
    want_miou = float(np.mean([np.mean(ious[k]) for k in ("tower", "low_veg", "high_veg", "bckg", "cables")]))
    assert (np.isnan(want_miou) and np.isnan(res["mean_iou"])) or abs(res["mean_iou"] - want_miou) < 1e-3, (res["mean_iou"], want_miou)


def test_segment_file_pads_a_small_cluster_and_drops_the_padding(synth):
    """A cluster with fewer points than sa1.npoint is repeated cyclically up to it; what comes back covers the cluster's own rows only, and
    clusters of equal size share a call without changing a prediction."""
    T = sub("pointNet.pn2_train")
    model = sub("pointNet.model.pointnetAtt").pointnet_2_seg(5).eval()
    clusters, _ = synth.test_file_clusters(41, 3, n_points=600, spread=1)            # three clusters of 600 points: one call
    small = clusters[0][:300]
    preds, targets = T.segment_file(model, [small] + clusters, "cuda")
    assert preds.shape == targets.shape == (300 + 3 * 600,) and preds.dtype == torch.int64 and not preds.is_cuda
    rows = small[:, :9].float().cuda()
    padded = rows[torch.arange(model.sa1.npoint, device="cuda") % 300][None].contiguous()
    assert torch.equal(preds[:300], model.predict_rows(padded)[0, :300].cpu())
    for i, c in enumerate(clusters):
        alone = model.predict_rows(c[None, torch.arange(model.sa1.npoint) % 600, :9].float().cuda().contiguous())[0, :600].cpu()
        assert torch.equal(preds[300 + 600 * i:300 + 600 * (i + 1)], alone), i
