"""Training pointnet_2_seg on clusters of NATIVE size with the device augmentation, end to end on the GPU, on
synthetic.write_cluster_dataset(n_train=4, n_val=2, n_test=1): three clusters of 1024 .. 1323 points per file, one cut to 513 so the
padding path runs.  One pn2_step.train_loop_clouds_aug(..., augment=CloudAugment(7)) step against the same step composed by hand from
cloud_input + forward_ragged + seg_nll_loss + backward + FusedAdam, bit for bit; train=False ignores the augmentation; then
pn2_train.train_pn2_clouds (the loss goes down, the checkpoint has utils.save_checkpoint's keys, remembers the augmentation's two ints and
loads strictly into a default model) and pn2_infer.test on that checkpoint against the test split."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu

EPOCHS = 3
SEED = 7


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("pn2clouds")
    return root, sub("synthetic").write_cluster_dataset(str(root), n_train=4, n_val=2, n_test=1, seed=930)


@pytest.fixture(scope="module")
def trained(dataset):
    """train_pn2_clouds once for the module: (history, checkpoint path, pn2_infer.test()'s result), run from the dataset's folder
    (checkpoints are written relative to the working directory, as the other drivers write theirs)."""
    root, paths = dataset
    T, I = sub("pointNet.pn2_train"), sub("pointNet.pn2_infer")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        hist = T.train_pn2_clouds(paths["clusters"], paths["lists"], str(root / "out"), 2, EPOCHS, 1e-3, number_of_workers=0, seed=SEED)
        cks = sorted(os.listdir("pointNet/checkpoints"))
        assert cks
        ck_path = os.path.abspath(os.path.join("pointNet/checkpoints", cks[-1]))
        res = I.test(str(root), str(root / "res" / "preds"), 1024, 0, ck_path, paths["lists"], cluster_dir=paths["clusters"])
    finally:
        os.chdir(cwd)
    return hist, ck_path, res


def _files(paths, split, k):
    D = sub("pointNet.datasets")
    ds = D.LidarClusterDataset(paths["clusters"], open(os.path.join(paths["lists"], f"{split}_seg_files.txt")).read().split())
    return [ds[i] for i in range(k)]


def _pair():
    A, T, P = sub("pointNet.model.pointnetAtt"), sub("trainer"), sub("pointNet.pn2_train")
    torch.manual_seed(5)
    one = A.pointnet_2_seg(5, **P.TRAIN_FLAGS)
    two = A.pointnet_2_seg(5, **P.TRAIN_FLAGS)
    two.load_state_dict(one.state_dict())
    return one, two, T.FusedAdam(one.parameters(), lr=1e-3), T.FusedAdam(two.parameters(), lr=1e-3)


def test_one_augmented_step_equals_the_step_composed_by_hand(dataset):
    _, paths = dataset
    S, U, C = sub("pointNet.pn2_step"), sub("pointNet.model.pointnet2_utils"), sub("pointNet.collate_fns")
    files = _files(paths, "train", 2)
    clusters = files[0] + files[1]
    sizes = [int(c.shape[0]) for c in clusters]
    assert len(sizes) == 6 and sizes[1] == 513 and all(1024 <= n < 1324 for n in sizes[:1] + sizes[2:]) and len(set(sizes)) > 3
    one, two, opt1, opt2 = _pair()
    cw = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device="cuda")
    aug = S.CloudAugment(SEED)
    # the step, fed by a CloudBatch that is on the device already
    batch = C.collate_clouds(files).to("cuda")
    metrics, targets, preds, counts = S.train_loop_clouds_aug(batch, opt1, cw, one, train=True, augment=aug)
    assert aug._step == 1 and aug.state_dict() == {"seed": SEED, "step": 1}
    assert set(metrics) == {"loss"} and metrics["loss"].is_cuda and targets.is_cuda and preds.is_cuda and counts.is_cuda
    # the same step by hand
    raw = torch.cat(clusters, 0).cuda()
    rows, tg, padded, src = S.cloud_input(raw, sizes, two.sa1.npoint, train=True, seed=SEED, step=0, want_src=True)
    assert padded == [max(n, 1024) for n in sizes]
    two.train()
    opt2.zero_grad()
    loss, p2, c2 = U.seg_nll_loss(two.forward_ragged(rows, padded), tg, cw, want_preds=True, want_counts=True)
    loss.backward()
    opt2.step()
    own = tg != -1                                                   # the clouds' own rows: a label is never -1
    assert int(own.sum()) == sum(sizes) and int(counts[-1]) == sum(padded) - sum(sizes) == 511
    assert torch.equal(metrics["loss"], loss.detach()) and torch.equal(counts, c2)
    assert torch.equal(targets, tg[own]) and torch.equal(preds, p2[own])
    params = dict(two.named_parameters())
    for k, p in one.named_parameters():
        assert torch.equal(p, params[k]), k
    buffers = dict(two.named_buffers())
    for k, v in one.named_buffers():
        assert torch.equal(v, buffers[k]), k
    # the targets returned are in the AUGMENTED order: the labels of the source rows, not the file's order
    lut = sub("pointNet.amp_test")._label_lut(torch.device("cuda"))
    assert torch.equal(targets, lut[raw[src[own].long(), 9].long()]) and not torch.equal(targets, lut[raw[:, 9].long()])
    # a list of clusters gives the step the CloudBatch gave (one upload instead of none)
    again = S.train_loop_clouds_aug(clusters, opt2, cw, two, train=False, augment=S.CloudAugment(SEED))
    batch_eval = S.train_loop_clouds_aug(batch, opt1, cw, one, train=False, augment=aug)
    assert torch.equal(again[0]["loss"], batch_eval[0]["loss"]) and all(torch.equal(a, b) for a, b in zip(again[1:], batch_eval[1:]))


def test_eval_ignores_the_augmentation_and_keeps_its_step(dataset):
    _, paths = dataset
    S = sub("pointNet.pn2_step")
    files = _files(paths, "train", 2)
    clusters = files[0] + files[1]
    one, _, opt1, _ = _pair()
    cw = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device="cuda")
    aug = S.CloudAugment(SEED)
    aug._step = 4
    with_aug = S.train_loop_clouds_aug(clusters, opt1, cw, one, train=False, augment=aug)
    assert aug._step == 4 and not one.training and not with_aug[0]["loss"].requires_grad
    without = S.train_loop_clouds(clusters, opt1, cw, one, train=False)
    assert torch.equal(with_aug[0]["loss"], without[0]["loss"]) and all(torch.equal(a, b) for a, b in zip(with_aug[1:], without[1:]))
    want = sub("pointNet.amp_test")._upload_clusters(clusters, torch.device("cuda"))[1]
    assert torch.equal(without[1], want)                             # unaugmented: the file's order
    with pytest.raises(sub("_lib").AmpnetError, match="CloudAugment"):
        S.train_loop_clouds_aug(clusters, opt1, cw, one, train=False, augment=7)


def test_training_lowers_the_loss_and_writes_a_loadable_checkpoint(trained):
    """Three epochs of two steps each (two files = six clouds per step, lr 1e-3, seeds 0 / 7).  Observed on an MI355X, mean train loss per
    epoch: 1.7200, 1.5131, 1.3717 (validation 1.6632, 1.6435, 1.6231): the last epoch is 0.35 below the first, so three epochs leave room
    to spare.  (As in test_pn2_cli_gpu.py the validation accuracy is poor after six steps -- the running statistics have barely moved --
    which is why the test asks for the train loss and for nothing about quality.)"""
    hist, ck_path, _ = trained
    losses = [tr["loss"] for tr, _ in hist]
    print("train_pn2_clouds mean train loss per epoch:", ", ".join(f"{l:.4f}" for l in losses),
          "| validation:", ", ".join(f"{va['loss']:.4f}" for _, va in hist))
    assert len(hist) == EPOCHS and all(np.isfinite(losses)) and all(np.isfinite([va["loss"] for _, va in hist]))
    assert losses[-1] < losses[0]
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert set(ck) == {"model", "optimizer", "batch_size", "lr", "number_of_points", "epoch", "epochs_since_improvement", "accuracy",
                       "weighing_method"}                            # train_pn2's key set
    assert (ck["batch_size"], ck["lr"], ck["number_of_points"]) == (2, 1e-3, None)
    state = ck["weighing_method"]["cloud_augment"]
    assert state["seed"] == SEED and state["step"] == 2 * (ck["epoch"] + 1)          # two train steps per epoch, none in validation
    plain = sub("pointNet.model.pointnetAtt").pointnet_2_seg(5)
    plain.load_state_dict(ck["model"], strict=True)
    assert int(plain.bn1.num_batches_tracked) == 2 * (ck["epoch"] + 1)


def test_the_inference_driver_runs_on_the_checkpoint(dataset, trained):
    root, _ = dataset
    _, ck_path, res = trained
    assert set(res) == {"mean_iou", "accuracy", "iou"} and 0.0 <= res["accuracy"] <= 1.0
    row = open(root / "res" / "IoU-results-v2.csv").read().strip().split("\n")[-1].split(",")
    assert len(row) == 11 and row[0] == os.path.basename(ck_path).split(".")[0]
