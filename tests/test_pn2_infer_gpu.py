"""pn2_infer.test end to end on a synthetic dataset in the reference's on-disk formats: the metrics of a seeded default pointnet_2_seg(5)
checkpoint from the precomputed clusters, with one and with several files per launch, against accuracy and IoU recomputed here from
predict_rows on every cluster alone."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("bckg", "tower", "cables", "low_veg", "high_veg")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(paths, checkpoint path, result with files_per_launch=1, result with 3, root): four test files of three clusters each, no training."""
    root = tmp_path_factory.mktemp("pn2_infer")
    paths = sub("synthetic").write_dataset(str(root), n_train=0, n_val=0, n_test=4, n_points=2048, seed=940)
    torch.manual_seed(17)
    model = sub("pointNet.model.pointnetAtt").pointnet_2_seg(5)
    ck = str(root / "checkpoint_seeded.pth")
    torch.save({"model": model.state_dict()}, ck)
    I = sub("pointNet.pn2_infer")
    one = I.test(paths["data"], str(root / "res" / "preds"), 2048, 0, ck, paths["lists"], cluster_dir=paths["clusters"])
    three = I.test(paths["data"], str(root / "res" / "preds"), 2048, 0, ck, paths["lists"], cluster_dir=paths["clusters"], files_per_launch=3)
    return paths, ck, one, three, root


def test_files_per_launch_does_not_change_the_result(run):
    _, _, one, three, _ = run
    assert set(one) == {"mean_iou", "accuracy", "iou"} and set(one["iou"]) == set(KEYS)
    assert repr(one) == repr(three)                 # (repr: a class no file holds gives nan, which is not equal to itself)


def test_the_csv_row_is_the_family_s(run):
    _, ck, one, _, root = run
    lines = open(root / "res" / "IoU-results-v2.csv").read().strip().split("\n")
    assert len(lines) == 2                          # one row per run
    for line in lines:
        row = line.split(",")
        assert len(row) == 11 and row[0] == "checkpoint_seeded" and row[1] == "2048"
        assert float(row[7]) == round(one["mean_iou"], 4) or np.isnan(one["mean_iou"])
        assert float(row[8]) == round(one["accuracy"], 3)
    assert lines[0].rsplit(",", 1)[0] == lines[1].rsplit(",", 1)[0]                   # all but the minutes


def test_the_metrics_are_those_of_predict_rows_on_every_cluster_alone(run):
    paths, ck, one, three, _ = run
    U = sub("utils.utils")
    model = sub("pointNet.model.pointnetAtt").pointnet_2_seg(5).eval()
    model.load_state_dict(torch.load(ck, map_location="cuda", weights_only=True)["model"])
    names = [f.split(".")[0] for f in open(os.path.join(paths["lists"], "test_seg_files.txt")).read().split()]
    assert len(names) == 4
    accs, ious = [], {k: [] for k in KEYS}
    for name in names:
        clusters = torch.load(os.path.join(paths["clusters"], name + "_clusters_list.pkl"), weights_only=True)
        assert len({c.shape[0] for c in clusters}) == len(clusters) == 3              # unequal sizes: the ragged path is what runs
        preds = np.concatenate([model.predict_rows(c[None, :, :9].float().cuda().contiguous()).cpu().numpy().reshape(-1) for c in clusters])
        tg = torch.cat(U.get_labels([c.clone() for c in clusters])).numpy()
        accs.append(float(np.float32((preds == tg).sum()) / np.float32(len(tg))))
        for c, k in enumerate(KEYS):
            if (tg == c).any():
                tp = np.logical_and(preds == c, tg == c).sum()
                ious[k].append(float(np.float32(tp) / np.float32((tg == c).sum() + (preds == c).sum() - tp)))
    for res in (one, three):
        assert abs(res["accuracy"] - float(np.mean(accs))) < 2e-4
        for k, v in ious.items():
            want = float(np.mean(v)) if v else float("nan")
            assert (np.isnan(want) and np.isnan(res["iou"][k])) or abs(res["iou"][k] - want) < 1e-3, (k, res["iou"][k], want)
        want_miou = float(np.mean([np.mean(ious[k]) for k in ("tower", "low_veg", "high_veg", "bckg", "cables")]))
        assert (np.isnan(want_miou) and np.isnan(res["mean_iou"])) or abs(res["mean_iou"] - want_miou) < 1e-3, (res["mean_iou"], want_miou)
