"""Rank program and shared helpers of tests/test_pn2_dp_gpu.py: data-parallel pointnet_2_seg with global-batch BatchNorm.
Test infrastructure; the rank programs are started by torch.distributed.run (two gloo ranks, both on cuda:0) or, for `onerank`, as one
process with the nccl backend under AMPNET_FORCE_COLLECTIVES=1.  A rank that fails leaves with a non-zero status.

Usage: pn2_dp_worker.py MODE OUT_DIR [ARG]
  layers   every entry of LAYERS through the train entry points of the C ABI with a registered collective, this rank's share of the case
           -> OUT_DIR/layers<rank>.pt
  step     with global-batch BatchNorm, then without (one launch for both): two mode-T steps of train_loop_clouds_aug on this rank's share of
           the five clouds (3 | 2) without moving the parameters (lr 0), then one with lr 1e-3 -> OUT_DIR/step<1 / 0>_<rank>.pt
  driver   train_pn2_clouds for one epoch on the dataset under OUT_DIR, run from OUT_DIR/rank<rank> -> OUT_DIR/driver<rank>.pt
  onerank  ARG = 1 / 0 (global-batch BatchNorm or the gradient all-reduce alone): one_step() -> OUT_DIR/onerank<ARG>.pt"""
import datetime
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "3d-semantic-segmentation-amp-net_amd"
DEV = "cuda"

# (kind, case of the kind's table, what rank 0 holds: clouds for fp / sa, rows for the head).  Every fp / sa case of the tables has two
# clouds or many; the head's rows are split off the 32-row tile and unevenly.
LAYERS = [("fp", "tail_tile", 1), ("fp", "negative_gamma", 1), ("fp", "fp1_l0", 1), ("fp", "many_tiles", 401),
          ("sa", "tail_group", 1), ("sa", "no_feats", 1), ("sa", "two_tiles", 1), ("sa", "many_groups", 1),
          ("head", "no_drop", 27), ("head", "rows257", 100)]
HEAD_ROWS257 = dict(M=257, cin=32, hidden=64, C=5, base=7913)       # p = 0: 100 | 157 rows, three and five tiles with a tail each
SPLIT = 3                                                          # the whole step: clouds 0 .. 2 on rank 0 (457 rows), 3 .. 4 on rank 1 (711)
SLICED = {"fp": ("points1", "points2", "idx", "dist2", "dout"), "sa": ("xyz", "centres", "group_idx", "feats", "dout"),
          "head": ("x", "dlogp")}
PER_RANK = {"fp": ("out", "dpoints1", "dpoints2"), "sa": ("out", "arg", "dfeats"), "head": ("logp", "dx")}       # concatenated over the ranks
SAME = ("save_mean", "save_invstd", "running_mean", "running_var")                                           # equal on every rank


def sub(name):
    return importlib.import_module(PKG + ("." + name if name else ""))


def layer_inputs(kind, name):
    """The numpy inputs of a LAYERS entry from the kind's restatement module."""
    synth = sub("synthetic")
    if kind == "fp":
        import fp_train_ref
        return fp_train_ref.case_inputs(synth, name)
    if kind == "sa":
        import sa_train_ref
        return sa_train_ref.case_inputs(synth, name)
    import seg_head_train_ref as H
    if name != "rows257":
        return H.case_inputs(synth, name)
    c = HEAD_ROWS257                                               # a case of case_inputs' making at 257 rows, p = 0
    x = synth.uniform(c["base"] * 16 + 1, (c["M"], c["cin"]), -1.0, 1.0)
    layer = H.make_layers(c["base"] + 1, c["cin"], [c["hidden"]])[0]
    H.settle_beta(x, layer, H.BN_EPS)
    k = 1.0 / np.sqrt(c["hidden"])
    W2 = synth.uniform(c["base"] * 16 + 2, (c["C"], c["hidden"]), -4.0 * k, 4.0 * k)
    b2 = synth.uniform(c["base"] * 16 + 3, (c["C"],), -1.0, 1.0)
    dlogp = synth.uniform(c["base"] * 16 + 4, (c["M"], c["C"]), -1.0, 1.0)
    return dict(x=x, params=tuple(layer) + (W2, b2), dlogp=dlogp, eps=H.BN_EPS, p=0.0, drop_seed=H.DROP_SEED)


def share(kind, i, first, rank):
    """Rank `rank`'s part of the inputs: the leading `first` clouds (rows) or the rest."""
    sl = slice(0, first) if rank == 0 else slice(first, None)
    return dict(i, **{k: None if i[k] is None else np.ascontiguousarray(i[k][sl]) for k in SLICED[kind]})


def run_layer(kind, i):
    """Forward and backward of a case through the existing layer tests' own drivers -> {name: numpy array}."""
    L = sub("_lib")
    mod = importlib.import_module({"fp": "test_fp_train_gpu", "sa": "test_sa_train_gpu", "head": "test_seg_head_train_gpu"}[kind])
    return mod._run(L, i)


def step_clouds():
    """The five clouds of pn2_ragged_ref.case_inputs as cluster files hold them ([n_i, 10], column 9 the ASPRS class code) and the labels
    [total] the step reads off the codes.  No class code means "ignore" (only padding rows are -1, and no cloud here is padded), so the
    case's -1 targets become class 0; class 4 stays absent."""
    import pn2_ragged_ref as G
    inputs = G.case_inputs(sub("synthetic"))
    target = np.where(inputs["target"] < 0, 0, inputs["target"])
    code = np.array([1, 15, 14, 3, 5], dtype=np.float32)[target]
    raw = torch.from_numpy(np.concatenate([inputs["x"], code[:, None]], -1).astype(np.float32))
    return list(raw.split(list(G.SIZES))), target.astype(np.int64)


def snapshot(net, world, loss):
    """What pn2_model_ref.errors compares, from the model after a step: averaged gradients, running statistics, counters."""
    return dict(loss=loss.detach().cpu(), grads={k: (p.grad / world).detach().cpu() for k, p in net.named_parameters()},
                buffers={k: v.detach().cpu().clone() for k, v in net.named_buffers() if not k.endswith("num_batches_tracked")},
                counts={k: int(v) for k, v in net.named_buffers() if k.endswith("num_batches_tracked")})


def one_step():
    """On the reduced model of tests/test_pn2_ragged_train_gpu.py and its five clouds: a train-mode forward_ragged (log_probs), then, on a
    second model of the same seed, one train_loop_clouds step with FusedAdam -> dict of CPU tensors."""
    import test_pn2_ragged_train_gpu as RT
    S, T = sub("pointNet.pn2_step"), sub("trainer")
    clouds, _ = step_clouds()
    rows = torch.cat(clouds)[:, :9].contiguous().to(DEV)
    res = {"log_probs": RT._model("T").forward_ragged(rows, list(RT.SIZES)).detach().cpu()}
    net = RT._model("T")
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    metrics, _, _, counts = S.train_loop_clouds(clouds, opt, torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=DEV), net, train=True)
    torch.cuda.synchronize()
    res["loss"], res["counts"] = metrics["loss"].cpu(), counts.cpu()
    for k, p in net.named_parameters():
        res["grad/" + k], res["param/" + k] = p.grad.detach().cpu().clone(), p.detach().cpu().clone()
    for k, v in net.named_buffers():
        res["buf/" + k] = v.detach().cpu().clone()
    return res


def _layers(out_dir, rank):
    res = {}
    for kind, name, first in LAYERS:
        got = run_layer(kind, share(kind, layer_inputs(kind, name), first, rank))
        res.update({f"{kind}/{name}/{k}": torch.from_numpy(v) for k, v in got.items()})
    # the row-count rule under a collective: M * world_size must stay an exact float (a host-side refusal, nothing is launched)
    L = sub("_lib")
    assert L.fp_train_forward_workspace_bytes(16, 32, 1, 1 << 23, [32]) > 0
    try:
        L.fp_train_forward_workspace_bytes(16, 32, 1, (1 << 23) + 1, [32])
        res["refusal"] = ""
    except L.AmpnetError as e:
        res["refusal"] = str(e)
    torch.save(res, os.path.join(out_dir, f"layers{rank}.pt"))


def _step(out_dir, rank, world, sync):
    import pn2_model_ref as R
    import test_pn2_ragged_train_gpu as RT
    S, T = sub("pointNet.pn2_step"), sub("trainer")
    clouds, _ = step_clouds()
    mine = clouds[:SPLIT] if rank == 0 else clouds[SPLIT:]
    net = RT._model("T")
    net._head.seed = (net._head.seed + rank) & 0xFFFFFFFF            # as the drivers set it
    opt = T.FusedAdam(net.parameters(), lr=0.0)                      # (the restatement has no optimiser between its two steps)
    class_w = torch.tensor(R.CLASS_W, device=DEV)
    res = {}
    for step in range(2):
        metrics, _, _, _ = S.train_loop_clouds_aug(mine, opt, class_w, net, train=True, augment=None)
        torch.cuda.synchronize()
        res[f"step{step}"] = snapshot(net, world, metrics["loss"])
    opt.param_groups[0]["lr"] = 1e-3
    S.train_loop_clouds_aug(mine, opt, class_w, net, train=True, augment=None)
    torch.cuda.synchronize()
    res["state"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    torch.save(res, os.path.join(out_dir, f"step{int(sync)}_{rank}.pt"))


def _driver(out_dir, rank):
    P = sub("pointNet.pn2_train")
    seen = []
    dataset = P.LidarClusterDataset

    def recording(cluster_dir, files, **kw):
        seen.append(list(files))
        return dataset(cluster_dir, files, **kw)

    P.LidarClusterDataset = recording
    cwd = os.path.join(out_dir, f"rank{rank}")
    os.makedirs(cwd, exist_ok=True)
    os.chdir(cwd)                                                    # checkpoints are written relative to the working directory
    hist = P.train_pn2_clouds(os.path.join(out_dir, "k_means_25"), os.path.join(out_dir, "lists"), os.path.join(cwd, "out"), 2, 1, 1e-3,
                              number_of_workers=0, seed=7)
    torch.save(dict(train_files=seen[0], val_files=seen[1], val_loss=hist[0][1]["loss"], train_loss=hist[0][0]["loss"]),
               os.path.join(out_dir, f"driver{rank}.pt"))


if __name__ == "__main__":
    import torch.distributed as dist
    mode, out_dir = sys.argv[1], sys.argv[2]
    arg = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    torch.cuda.set_device(0)
    T = sub("trainer")
    if mode == "onerank":
        assert os.environ.get("AMPNET_FORCE_COLLECTIVES") == "1"
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0), timeout=datetime.timedelta(seconds=60))
        assert dist.get_world_size() == 1 and dist.get_backend() == "nccl"
    else:
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
    rank, world = dist.get_rank(), dist.get_world_size()
    if mode == "driver":
        os.environ["LOCAL_RANK"] = "0"                               # one GPU: both ranks on cuda:0
        _driver(out_dir, rank)
    else:
        if mode == "step":
            for sync in (1, 0):
                assert T.enable_sync_batchnorm() if sync else not T._SYNC["on"]
                _step(out_dir, rank, world, sync)
                T.disable_sync_batchnorm()
        else:
            if mode == "layers" or arg:
                assert T.enable_sync_batchnorm()
            if mode == "layers":
                _layers(out_dir, rank)
            else:
                torch.save(one_step(), os.path.join(out_dir, f"onerank{arg}.pt"))
    dist.barrier()
    T.disable_sync_batchnorm()
    dist.destroy_process_group()
