"""The host cost of data-parallel pointnet_2_seg on ONE GPU: a pn2_step.train_loop_clouds_aug step (full model, all five flags, FusedAdam,
CloudAugment) in three forms, in ALTERNATING rounds in this one process --
  plain     no exchange (AMPNET_FORCE_COLLECTIVES unset: a one-rank group issues none);
  dp        AMPNET_FORCE_COLLECTIVES=1: the flat gradient buffer and its one all-reduce per step;
  dp_sync   dp plus trainer.enable_sync_batchnorm(): the 17 + 17 global-batch BatchNorm exchanges of csrc/bn_train.hip and the loss
            all-reduce.
One rank initialises the `nccl` backend (RCCL) on the GPU, as tests/test_rccl_gpu.py does; with one rank every collective is the identity,
so dp_sync - plain is the HOST cost of issuing the exchanges, not a scaling figure (a one-rank ring moves no bytes).  Two shapes: 16 clouds
of 2048 points and 2 clouds of 1024 (a per-call cost does not depend on the batch; a small step shows it undiluted).
python3 tools/prof_pn2_dp.py [steps] [warmup]  -- wall time around `steps` steps after `warmup`, a synchronize on either side; the median
of 5 rounds is reported and every round listed; prints one JSON line."""
import importlib, json, os, socket, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist
PKG = "3d-semantic-segmentation-amp-net_amd"
sub = lambda name: importlib.import_module(PKG + "." + name)
synth, A, S, T, P = (sub(n) for n in ("synthetic", "pointNet.model.pointnetAtt", "pointNet.pn2_step", "trainer", "pointNet.pn2_train"))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ROUNDS = 5
assert torch.cuda.is_available(), "tools/prof_pn2_dp.py measures on the GPU"
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
if not dist.is_initialized():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    s.close()
    dist.init_process_group("nccl", device_id=dev)
assert dist.get_world_size() == 1 and dist.get_backend() == "nccl"
class_w = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=dev)
med = lambda rounds, q: sorted(r[q] for r in rounds)[len(rounds) // 2]


def clouds_of(seed, count, n):
    x = np.concatenate([synth.clouds(seed, count, n), synth.uniform(seed + 1, (count, n, 6), -1.0, 1.0)], -1)
    code = np.array([1, 15, 14, 3, 5], dtype=np.float32)[synth.randint(seed + 2, (count, n), 0, 5)]
    return list(torch.from_numpy(np.concatenate([x, code[..., None]], -1).astype(np.float32)))


def side(clouds, force, sync):
    """A model, its optimiser and augmentation of their own -> step(): one train step in the side's form."""
    torch.manual_seed(0)
    net = A.pointnet_2_seg(5, device=dev, **P.TRAIN_FLAGS)
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    aug = S.CloudAugment(7)
    last = {}

    def step_n(n):
        if force:
            os.environ["AMPNET_FORCE_COLLECTIVES"] = "1"
        else:
            os.environ.pop("AMPNET_FORCE_COLLECTIVES", None)
        if sync:
            assert T.enable_sync_batchnorm()
        try:
            for _ in range(warmup):
                S.train_loop_clouds_aug(clouds, opt, class_w, net, train=True, augment=aug)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                last["loss"] = S.train_loop_clouds_aug(clouds, opt, class_w, net, train=True, augment=aug)[0]["loss"]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3
        finally:
            if sync:
                T.disable_sync_batchnorm()
            os.environ.pop("AMPNET_FORCE_COLLECTIVES", None)

    return step_n, last


def shape_leg(count, n):
    clouds = clouds_of(940, count, n)
    sides = [side(clouds, False, False), side(clouds, True, False), side(clouds, True, True)]
    rounds = [tuple(s[0](steps) for s in sides) for _ in range(ROUNDS)]
    plain, dp, dp_sync = (med(rounds, q) for q in range(3))
    # (the three sides ran the same steps from the same state; with one rank their losses are the same bits)
    losses = [float(s[1]["loss"]) for s in sides]
    return {"clouds": count, "points_per_cloud": n, "plain_step_ms": round(plain, 3), "dp_step_ms": round(dp, 3),
            "dp_sync_step_ms": round(dp_sync, 3), "gradient_allreduce_cost_ms": round(dp - plain, 3),
            "sync_bn_exchanges_cost_ms": round(dp_sync - dp, 3), "dp_sync_minus_plain_ms": round(dp_sync - plain, 3),
            "rounds_ms_plain_dp_sync": [[round(v, 3) for v in r] for r in rounds], "last_losses_equal": len(set(losses)) == 1}


out = {"steps": steps, "warmup": warmup, "large": shape_leg(16, 2048), "small": shape_leg(2, 1024)}
dist.barrier()
dist.destroy_process_group()
print(json.dumps(out))
