"""pointnet_2_seg inference on clusters of unequal size: pn2_infer (ONE ragged launch sequence) against pn2_train.segment_file (one pass of
the whole network per distinct cluster size, each with a host read-back in its ball query -- the only way before the ragged path existed).
python3 tools/prof_pn2_ragged.py [steps] [warmup]  -- HIP events around `steps` calls after `warmup` calls, the two sides in ALTERNATING
rounds in this one process, the median round reported and every round listed; prints one JSON line.  (a) times 4 * steps calls per round
(tens of milliseconds a call: time enough of them), (b) `steps`.

(a) one file of 18 clusters of pairwise different sizes between 1100 and 4000 points: pn2_infer.segment_file against
    pn2_train.segment_file;
(b) 16 such files: pn2_infer.segment_files (one call) against pn2_train.segment_file file by file.
Both sides take the clusters from host memory and hand predictions and labels back on the host, as the drivers' callers get them; the
predictions of the two sides are compared (they are the same bits).  The model is the default pointnet_2_seg(5), seeded, in eval mode.
Under rocprofv3 (a kernel trace in a run of its own) the kernels to look for are ball_query_ragged_kernel and three_nn_ragged_kernel."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
PKG = "3d-semantic-segmentation-amp-net_amd"
sub = lambda name: importlib.import_module(PKG + "." + name)
synth, A, I, T = sub("synthetic"), sub("pointNet.model.pointnetAtt"), sub("pointNet.pn2_infer"), sub("pointNet.pn2_train")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 1
ROUNDS, CLUSTERS, FILES, LO, HI = 5, 18, 16, 1100, 4000
assert torch.cuda.is_available(), "tools/prof_pn2_ragged.py measures on the GPU"
dev = torch.device("cuda")


def timed(fn, n=steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


med = lambda rounds, q: sorted(r[q] for r in rounds)[len(rounds) // 2]


def make_file(seed):
    """18 clusters [n_i, 10] (9 features with x, y in [-1, 1] + ASPRS class code, the rows of synthetic.test_file_clusters) of pairwise
    different sizes in [LO, HI]."""
    sizes = list(dict.fromkeys(int(v) for v in synth.randint(seed * 64 + 63, (4 * CLUSTERS,), LO, HI + 1)))[:CLUSTERS]     # in drawing order
    out = []
    for i, s in enumerate(sizes):
        p = synth.kmeans_file_tensor(seed * 64 + i, s, 1, noise_frac=0.0)[:, :, 0]
        c = np.concatenate([p[:, :3], p[:, 4:10], p[:, 3:4]], axis=1).astype(np.float32)
        c[:, 0] = c[:, 0] * 2 - 1
        c[:, 1] = c[:, 1] * 2 - 1
        out.append(torch.from_numpy(c))
    assert len({c.shape[0] for c in out}) == CLUSTERS
    return out


def leg(files, n):
    torch.manual_seed(0)
    model = A.pointnet_2_seg(5, device=dev).eval()
    last = {}

    def ragged():
        last["new"] = I.segment_files(model, files, dev) if len(files) > 1 else [I.segment_file(model, files[0], dev)]

    def per_size():
        last["old"] = [T.segment_file(model, cl, dev) for cl in files]

    rounds = [(timed(ragged, n), timed(per_size, n)) for _ in range(ROUNDS)]
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(last["new"], last["old"]))
    sizes = [c.shape[0] for cl in files for c in cl]
    return {"files": len(files), "clusters": len(sizes), "points": sum(sizes), "min_size": min(sizes), "max_size": max(sizes),
            "calls_per_timing": n, "pn2_infer_ms": round(med(rounds, 0), 3), "pn2_train_segment_file_ms": round(med(rounds, 1), 3),
            "parent_over_ragged": round(med(rounds, 1) / med(rounds, 0), 3), "rounds_ms_ragged_parent": [[round(v, 3) for v in r] for r in rounds],
            "predictions_and_labels_equal": bool(same)}


files = [make_file(700 + f) for f in range(FILES)]
print(json.dumps({"steps": steps, "warmup": warmup, "one_file": leg(files[:1], steps * 4), "sixteen_files": leg(files, steps)}))
