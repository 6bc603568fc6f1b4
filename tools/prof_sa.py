"""Ball query + fused set-abstraction forward at the reference's sa1 shape (B = 16, N = 8192, npoint = 1024, nsample = 32, D = 9,
MLP [32, 32, 64]) against what torch-ROCm offers for the same layer: gather + conv2d + BatchNorm2d (eval) + relu + max.
python3 tools/prof_sa.py [steps] [warmup]  -- HIP events, warm-up first, both sides in this process; prints one JSON line.
Under rocprofv3 (counters in a run of their own) the kernels to look for are ball_query_kernel and sa_forward_kernel."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
PKG = "3d-semantic-segmentation-amp-net_amd"
synth = importlib.import_module(PKG + ".synthetic")
U = importlib.import_module(PKG + ".utils.utils")
L = importlib.import_module(PKG + "._lib")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B, N, S, K, D, MLP, RADIUS = 16, 8192, 1024, 32, 9, [32, 32, 64], 0.1
dev = "cuda"
xyz = torch.from_numpy(synth.clouds(200, B, N)).to(dev)
feats = torch.from_numpy(synth.uniform(201, (B, N, D), -1.0, 1.0)).to(dev)
cent = U.fps_indices(xyz, S)
g = torch.Generator().manual_seed(0)
layers, cin = [], 3 + D
for cout in MLP:
    layers.append(tuple(t.to(dev) for t in ((torch.rand(cout, cin, generator=g) - 0.5) * 2 / cin ** 0.5, (torch.rand(cout, generator=g) - 0.5) * 0.2,
                                            0.5 + torch.rand(cout, generator=g), torch.rand(cout, generator=g) - 0.5,
                                            (torch.rand(cout, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=g))))
    cin = cout
ws = torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
out = torch.empty((B, S, MLP[-1]), device=dev)
grp, cnt = U.ball_query(xyz, cent, RADIUS, K, return_counts=True)


def timed(fn):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def torch_layer():
    """The same layer in torch: the grouped tensor [B, 3 + D, S, K] goes through memory, as a user of the usual implementation has it."""
    gi = grp.long()
    bi = torch.arange(B, device=dev)[:, None, None]
    g_xyz = xyz[bi, gi] - xyz[torch.arange(B, device=dev)[:, None], cent.long()][:, :, None, :]
    x = torch.cat([g_xyz, feats[bi, gi]], -1).permute(0, 3, 1, 2)
    for w, b, gamma, beta, mean, var in layers:
        x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w[:, :, None, None], b), mean, var, gamma, beta, False, 0.0, 1e-5))
    return x.max(-1)[0].transpose(1, 2)


with torch.no_grad():
    bq_ms = timed(lambda: U.ball_query(xyz, cent, RADIUS, K))
    sa_ms = timed(lambda: L.sa_forward_f32(xyz, cent, grp, feats, layers, [1e-5] * len(MLP), out, ws))
    ref = torch_layer()
    torch_ms = timed(torch_layer)
err = float((out - ref).abs().max())
w_bytes = sum(sum(t.numel() for t in layer) for layer in layers) * 4
# the algorithmic bytes of the fused forward: the cloud once (coordinates + features), the centres and group indices, the weights, the output
algo = B * N * (3 + D) * 4 + B * S * 4 + B * S * K * 4 + w_bytes + B * S * MLP[-1] * 4
flops = 2.0 * B * S * K * sum(a * b for a, b in zip([3 + D] + MLP[:-1], MLP))
print(json.dumps({"shape": {"B": B, "N": N, "npoint": S, "nsample": K, "D": D, "mlp": MLP, "radius": RADIUS},
                  "mean_members": round(float(cnt.float().mean()), 2), "ball_query_ms": round(bq_ms, 4), "sa_forward_ms": round(sa_ms, 4),
                  "torch_gather_conv2d_max_ms": round(torch_ms, 4), "torch_over_fused": round(torch_ms / sa_ms, 2),
                  "sa_algorithmic_bytes": algo, "sa_GBps_at_algorithmic_bytes": round(algo / (sa_ms * 1e-3) / 1e9, 1),
                  "sa_useful_TFLOPs": round(flops / (sa_ms * 1e-3) / 1e12, 2), "max_abs_diff_vs_torch": err}))
