"""The fused segmentation head (ampnet_seg_head_forward_f32, ampnet_seg_head_backward_f32) at the shape it has behind pointnet_2 -- 16 x 2048
rows, 128 -> 128 -> 5 -- against torch's eval composition on the SAME tensors: conv1d + BatchNorm1d (eval) + relu + conv1d + log_softmax, and
torch.autograd's backward of it (graph built once and retained, only the backward is timed).
python3 tools/prof_seg_head.py [steps] [warmup] [train]  -- HIP events, warm-up first, `steps` calls per timing, fused and torch in ALTERNATING
rounds in this one process, the median round reported and every round listed; prints one JSON line.  Under rocprofv3 (a kernel trace in a run
of its own) the kernels to look for are sa_fold_kernel, seg_head_forward_kernel, seg_head_backward_kernel, fp_wgrad_kernel,
fp_wgrad_reduce_kernel, seg_db2_kernel and fp_bwd_finalize_kernel.
`train`: the train-mode entry points (ampnet_seg_head_train_forward_f32, ampnet_seg_head_train_backward_f32; dropout 0.5) against torch's
train-mode composition: conv1d + batch_norm (training, momentum 0.1) + relu + F.dropout(0.5) + conv1d + log_softmax -- torch draws its own
mask when timed; the differences are taken on an untimed pass that multiplies by the fused path's mask instead.  Kernels: segt_stats_kernel,
fpt_stats_finalize_kernel, seg_head_forward_kernel<true>, fpt_fold_kernel, segt_bwd_phase1_kernel, fpt_bwd_finalize_kernel,
segt_bwd_phase2_kernel and the weight-gradient tail above."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
PKG = "3d-semantic-segmentation-amp-net_amd"
synth = importlib.import_module(PKG + ".synthetic")
L = importlib.import_module(PKG + "._lib")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 10
TRAIN = len(sys.argv) > 3 and sys.argv[3] == "train"
DROP_P, SEED, MOMENTUM = 0.5, 0x6A09E667, 0.1
ROUNDS = 5
B, N, CIN, HIDDEN, C = 16, 2048, 128, 128, 5
M, EPS = B * N, 1e-5
dev = "cuda"
x = torch.from_numpy(synth.uniform(310, (M, CIN), -1.0, 1.0)).to(dev)
dlogp = torch.from_numpy(synth.uniform(311, (M, C), -1.0, 1.0)).to(dev)
g = torch.Generator().manual_seed(0)
params = [t.to(dev) for t in ((torch.rand(HIDDEN, CIN, generator=g) - 0.5) * 2 / CIN ** 0.5, (torch.rand(HIDDEN, generator=g) - 0.5) * 0.2,
                              0.5 + torch.rand(HIDDEN, generator=g), torch.rand(HIDDEN, generator=g) - 0.5,
                              (torch.rand(HIDDEN, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(HIDDEN, generator=g),
                              (torch.rand(C, HIDDEN, generator=g) - 0.5) * 8 / HIDDEN ** 0.5, torch.rand(C, generator=g) - 0.5)]
logp = torch.empty((M, C), device=dev)
preds = torch.empty((M,), dtype=torch.int64, device=dev)
ws = torch.empty(L.seg_head_forward_workspace_bytes(CIN, HIDDEN, C, M), dtype=torch.uint8, device=dev)
bws = torch.empty(L.seg_head_backward_workspace_bytes(CIN, HIDDEN, C, M), dtype=torch.uint8, device=dev)
dx = torch.empty((M, CIN), device=dev)
grads = [torch.empty_like(params[q]) for q in (0, 1, 1, 1, 6, 7)]


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


xt = x.reshape(B, N, CIN).transpose(1, 2).contiguous()                  # [B, cin, N], the layout torch's head is handed
W1, b1, gamma, beta, mean, var, W2, b2 = params


def torch_head(inp, mask=None):
    """mask: None -- eval mode, or train mode with torch's own dropout; a tensor [B, hidden, N] -- train mode with that keep * scale."""
    a = F.conv1d(inp, W1[:, :, None], b1)
    if not TRAIN:
        h = torch.relu(F.batch_norm(a, mean, var, gamma, beta, False, 0.0, EPS))
    else:
        h = torch.relu(F.batch_norm(a, t_mean, t_var, gamma, beta, True, MOMENTUM, EPS))
        h = F.dropout(h, DROP_P, True) if mask is None else h * mask
    return torch.log_softmax(F.conv1d(h, W2[:, :, None], b2), dim=1).permute(0, 2, 1)        # [B, N, C]


def torch_fwd():
    with torch.no_grad():
        return torch_head(xt)


if TRAIN:
    t_mean, t_var = mean.clone(), var.clone()                           # torch's running statistics; the fused path updates `params`' own
    save_mean, save_invstd = torch.empty(HIDDEN, device=dev), torch.empty(HIDDEN, device=dev)
    ws = torch.empty(L.seg_head_train_forward_workspace_bytes(CIN, HIDDEN, C, M), dtype=torch.uint8, device=dev)
    bws = torch.empty(L.seg_head_train_backward_workspace_bytes(CIN, HIDDEN, C, M), dtype=torch.uint8, device=dev)
    fused_fwd = lambda: L.seg_head_train_forward_f32(x, params, EPS, MOMENTUM, DROP_P, SEED, logp, save_mean, save_invstd, ws)
    fused_bwd = lambda: L.seg_head_train_backward_f32(x, params, EPS, DROP_P, SEED, save_mean, save_invstd, dlogp, dx, grads, bws)
    fused_fwd()                                                         # (save_mean and save_invstd for the timed backward)
else:
    fused_fwd = lambda: L.seg_head_forward_f32(x, params, EPS, logp, preds, ws)
    fused_bwd = lambda: L.seg_head_backward_f32(x, params, EPS, dlogp, dx, grads, bws)
leaves = [xt.requires_grad_(True)] + [params[q].requires_grad_(True) for q in (0, 1, 2, 3, 6, 7)]
t_out = torch_head(xt)
d3 = dlogp.reshape(B, N, C)
torch_bwd = lambda: torch.autograd.grad(t_out, leaves, d3, retain_graph=True)
rounds = [(timed(fused_fwd), timed(torch_fwd), timed(fused_bwd), timed(torch_bwd)) for _ in range(ROUNDS)]
fused_fwd()
fused_bwd()
if TRAIN:                                                               # the same mask on both sides, untimed
    oracle = importlib.import_module("oracle.ampnet_oracle")
    keep = torch.from_numpy(oracle.keep_mask(SEED, 0, M * HIDDEN, DROP_P)).to(dev).reshape(B, N, HIDDEN).transpose(1, 2)
    t_out = torch_head(xt, keep.float() * (1.0 / (1.0 - DROP_P)))
t_grads = torch_bwd()
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
diff = {"logp_max_abs": float((logp.reshape(B, N, C) - t_out.detach()).abs().max()),
        "dx": rel(dx.reshape(B, N, CIN), t_grads[0].transpose(1, 2))}
if not TRAIN:
    diff["preds_differ"] = int((preds.reshape(B, N) != t_out.detach().argmax(-1)).sum())
for name, got, want in zip(("dW1", "db1", "dgamma", "dbeta", "dW2", "db2"), grads, t_grads[1:]):
    if TRAIN and name == "db1":                                         # exact zeros here, a cancelling sum in torch
        diff[name + "_max_abs"] = float((got - want.reshape(got.shape)).abs().max())
    else:
        diff[name] = rel(got, want.reshape(got.shape))
med = lambda q: sorted(r[q] for r in rounds)[ROUNDS // 2]
w_bytes = sum(p.numel() for p in params) * 4
fwd_bytes = M * CIN * 4 + w_bytes + M * C * 4 + M * 8                   # the rows once, the weights, logp, preds
if TRAIN:
    fwd_bytes += M * CIN * 4 - M * 8                                    # the statistics pass reads the rows a second time; no preds
fwd_flops = 2.0 * M * (CIN * HIDDEN + HIDDEN * C)
bwd_flops = 2.0 * M * (3 * CIN * HIDDEN + 3 * HIDDEN * C)               # the recomputed forward, dx = dz W and dW = dz^T x of both layers
print(json.dumps({"mode": "train" if TRAIN else "eval", "shape": {"rows": M, "cin": CIN, "hidden": HIDDEN, "classes": C}, "steps": steps, "warmup": warmup,
                  "seg_head_forward_ms": round(med(0), 4), "torch_forward_ms": round(med(1), 4), "torch_forward_over_fused": round(med(1) / med(0), 2),
                  "seg_head_backward_ms": round(med(2), 4), "torch_backward_ms": round(med(3), 4),
                  "torch_backward_over_fused": round(med(3) / med(2), 2),
                  "rounds_ms_fused_fwd_torch_fwd_fused_bwd_torch_bwd": [[round(v, 4) for v in r] for r in rounds],
                  "forward_algorithmic_bytes": fwd_bytes, "forward_GBps_at_algorithmic_bytes": round(fwd_bytes / (med(0) * 1e-3) / 1e9, 1),
                  "forward_useful_TFLOPs": round(fwd_flops / (med(0) * 1e-3) / 1e12, 2),
                  "backward_useful_TFLOPs": round(bwd_flops / (med(2) * 1e-3) / 1e12, 2), "backward_workspace_MB": round(bws.numel() / 1e6, 1),
                  "max_diff_vs_torch": diff}))
