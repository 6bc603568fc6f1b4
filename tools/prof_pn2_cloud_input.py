"""The input side of pn2_step.train_loop_clouds: ONE kernel (pn2_step.cloud_input -> ampnet_cloud_input_f32) against the chain of torch
operations it replaced, and a whole train step with and without the device augmentation.
python3 tools/prof_pn2_cloud_input.py [steps] [warmup] [input|step|all]  -- HIP events around `steps` calls after `warmup` calls, the two sides in
ALTERNATING rounds in this one process, the median of 5 rounds reported and every round listed; prints one JSON line.

Workloads: 16 files x 18 clusters of pairwise different sizes in [1100, 4000] (tools/prof_pn2_ragged.py's files), the same with two
clusters per file cut to 600 points (below sa1.npoint = 1024: the padding path), and one file.  The upload is excluded on both sides: both
start from the [total, 10] float32 array on the device.
(a) input: cloud_input (train=False, then train=True: shuffle + rotation) against the chain -- raw[:, :9].contiguous(), the
    long().clamp_().index label look-up and, with a short cloud, the pad_cloud_sizes gather of rows and targets, torch.where and the three
    small uploads.  The unaugmented outputs of the two sides are compared (equal bits).  host_ms is the host's time to ENQUEUE one call
    (perf_counter, no synchronise inside the window).
    torch_chain_with_layout adds the offsets' upload forward_ragged then did itself (the kernel's call hands its table on).
(b) step: train_loop_clouds_aug on a CloudBatch that is on the device, augment=CloudAugment() against augment=None, and against the step
    composed as it was before the kernel existed (the chain, then forward_ragged, seg_nll_loss, backward, FusedAdam).  The plain and the
    chain side run the same steps from the same state: their last losses must agree.
Under rocprofv3 (a kernel trace in a run of its own, `input` leg) the kernel to look for is cloud_input_kernel; the chain's are torch's copy,
index and where kernels."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
PKG = "3d-semantic-segmentation-amp-net_amd"
sub = lambda name: importlib.import_module(PKG + "." + name)
synth, A, S, U, X, C, T, P, U2 = (sub(n) for n in ("synthetic", "pointNet.model.pointnetAtt", "pointNet.pn2_step", "utils.utils",
                                                   "pointNet.amp_test", "pointNet.collate_fns", "trainer", "pointNet.pn2_train",
                                                   "pointNet.model.pointnet2_utils"))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 1
legs = sys.argv[3] if len(sys.argv) > 3 else "all"
ROUNDS, CLUSTERS, FILES, LO, HI, NPOINT, SHORT = 5, 18, 16, 1100, 4000, 1024, 600
assert torch.cuda.is_available(), "tools/prof_pn2_cloud_input.py measures on the GPU"
dev = torch.device("cuda")


def timed(fn, n):
    """(device ms per call, host ms per call spent enqueueing)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3 / n
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, host


med = lambda rounds, q: sorted(r[q] for r in rounds)[len(rounds) // 2]


def make_file(seed, short):
    """18 clusters [n_i, 10] (9 features with x, y in [-1, 1] + ASPRS class code) of pairwise different sizes in [LO, HI]; the first `short`
    are cut to SHORT points."""
    sizes = list(dict.fromkeys(int(v) for v in synth.randint(seed * 64 + 63, (4 * CLUSTERS,), LO, HI + 1)))[:CLUSTERS]
    out = []
    for i, s in enumerate(sizes):
        p = synth.kmeans_file_tensor(seed * 64 + i, s, 1, noise_frac=0.0)[:, :, 0]
        c = np.concatenate([p[:, :3], p[:, 4:10], p[:, 3:4]], axis=1).astype(np.float32)
        c[:, 0] = c[:, 0] * 2 - 1
        c[:, 1] = c[:, 1] * 2 - 1
        out.append(torch.from_numpy(c[:SHORT] if i < short else c))
    return out


def chain(raw, sizes):
    """The input side of train_loop_clouds before the kernel existed, from the uploaded array on."""
    rows = raw[:, :9].contiguous()
    tg = X._label_lut(dev)[raw[:, 9].long().clamp_(0, 255)]
    if min(sizes) < NPOINT:
        sizes, _, gather, keep = U.pad_cloud_sizes(sizes, NPOINT)
        own = np.zeros(len(gather), dtype=bool)
        own[keep] = True
        gather = torch.from_numpy(gather).to(dev, non_blocking=True)
        keep = torch.from_numpy(keep).to(dev, non_blocking=True)
        rows = rows[gather]
        tg = torch.where(torch.from_numpy(own).to(dev, non_blocking=True), tg[gather], -1)
    return rows, tg, sizes


def input_leg(files):
    batch = C.collate_clouds(files).to(dev)
    raw, sizes = batch.raw, batch.sizes
    n = max(steps * 10, 20)                                           # sub-millisecond calls: a longer window
    kernel = lambda: S.cloud_input(raw, sizes, NPOINT, train=False, seed=0, step=0)
    augmented = lambda: S.cloud_input(raw, sizes, NPOINT, train=True, seed=7, step=3)
    old = lambda: chain(raw, sizes)

    def old_with_layout():                                            # + the offsets forward_ragged then uploaded itself; the kernel's
        rows, _, padded_sizes = chain(raw, sizes)                     # call hands its own table on (pn2_step._cloud_input)
        U.ragged_layout("prof", rows, padded_sizes)

    rounds = [timed(kernel, n) + timed(augmented, n) + timed(old, n) + timed(old_with_layout, n) for _ in range(ROUNDS)]
    (r1, t1, _), (r0, t0, _) = kernel(), old()
    padded = sum(max(s, NPOINT) for s in sizes)
    return {"clouds": len(sizes), "rows_in": sum(sizes), "rows_out": padded, "cloud_input_ms": round(med(rounds, 0), 4),
            "cloud_input_augmented_ms": round(med(rounds, 2), 4), "torch_chain_ms": round(med(rounds, 4), 4),
            "torch_chain_with_layout_ms": round(med(rounds, 6), 4), "chain_over_kernel": round(med(rounds, 4) / med(rounds, 0), 2),
            "chain_with_layout_over_kernel": round(med(rounds, 6) / med(rounds, 0), 2),
            "host_ms_kernel_augmented_chain": [round(med(rounds, q), 4) for q in (1, 3, 5)],
            "augmented_GBps": round((sum(sizes) * 40 + padded * 44) / med(rounds, 2) / 1e6, 1),
            "rounds_ms_kernel_augmented_chain": [[round(r[q], 4) for q in (0, 2, 4)] for r in rounds],
            "outputs_equal": bool(torch.equal(r1.view(torch.int32), r0.view(torch.int32)) and torch.equal(t1, t0))}


def step_leg(files):
    batch = C.collate_clouds(files).to(dev)
    class_w = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=dev)

    def side(augment):
        torch.manual_seed(0)
        net = A.pointnet_2_seg(5, device=dev, **P.TRAIN_FLAGS)
        opt = T.FusedAdam(net.parameters(), lr=1e-3)
        last = {}

        def step():
            last["loss"] = S.train_loop_clouds_aug(batch, opt, class_w, net, train=True, augment=augment)[0]["loss"]

        return step, last

    def parent_side():
        """The step as it was composed before the kernel existed: the chain, forward_ragged on the list of sizes."""
        torch.manual_seed(0)
        net = A.pointnet_2_seg(5, device=dev, **P.TRAIN_FLAGS).train()
        opt = T.FusedAdam(net.parameters(), lr=1e-3)
        last = {}

        def step():
            rows, tg, padded_sizes = chain(batch.raw, batch.sizes)
            opt.zero_grad()
            loss, _, _ = U2.seg_nll_loss(net.forward_ragged(rows, padded_sizes), tg, class_w, want_preds=True, want_counts=True)
            loss.backward()
            opt.step()
            last["loss"] = loss.detach()

        return step, last

    aug, la = side(S.CloudAugment())
    plain, lp = side(None)
    parent, lq = parent_side()
    rounds = [timed(aug, steps) + timed(plain, steps) + timed(parent, steps) for _ in range(ROUNDS)]
    return {"clouds": len(batch.sizes), "rows": sum(batch.sizes), "step_augmented_ms": round(med(rounds, 0), 3),
            "step_plain_ms": round(med(rounds, 2), 3), "step_torch_chain_ms": round(med(rounds, 4), 3),
            "augmented_over_plain": round(med(rounds, 0) / med(rounds, 2), 3), "plain_over_chain": round(med(rounds, 2) / med(rounds, 4), 3),
            "host_ms_augmented_plain_chain": [round(med(rounds, q), 3) for q in (1, 3, 5)],
            "rounds_ms_augmented_plain_chain": [[round(r[q], 3) for q in (0, 2, 4)] for r in rounds],
            "last_loss_augmented": float(la["loss"]), "last_loss_plain": float(lp["loss"]), "last_loss_chain": float(lq["loss"])}


many = [make_file(s, 0) for s in range(FILES)]
short = [make_file(s, 2) for s in range(FILES)]
workloads = {"16_files": many, "16_files_2_short_each": short, "1_file": many[:1]}
out = {"steps": steps, "warmup": warmup}
if legs in ("input", "all"):
    out["input"] = {k: input_leg(v) for k, v in workloads.items()}
if legs in ("step", "all"):
    out["step"] = {k: step_leg(v) for k, v in workloads.items()}
print(json.dumps(out))
