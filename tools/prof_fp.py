"""3-NN search + fused feature-propagation forward at the reference's fp1 shape (the one that follows from tools/prof_sa.py's sa1 shape:
B = 16, N = 8192 fine points, S = 1024 coarse points, D1 = 0, D2 = 128, MLP [128, 128, 128]) against what torch-ROCm offers for the same
layer: cdist + topk, gather, weighted sum, conv1d + BatchNorm1d (eval) + relu.
python3 tools/prof_fp.py [steps] [warmup]  -- HIP events, warm-up first, each of the three in a timed loop of its own, all in this process;
prints one JSON line.  Under rocprofv3 (counters in a run of their own) the kernels to look for are three_nn_kernel and fp_forward_kernel.
The backward leg, same shape, same inputs, same process: the fused backward (ampnet_fp_backward_f32: sa_fold_kernel, fp_backward_kernel,
fp_wgrad_kernel + fp_wgrad_reduce_kernel per layer, fp_scatter_kernel, fp_bwd_finalize_kernel) against torch.autograd's backward of the
torch composition below on the SAME neighbours (graph built once and retained, only the backward is timed); the two are timed in
alternating rounds and every round is reported.
The train-mode leg, same shape, same process ("train" in the JSON line): the fused batch-statistics forward (ampnet_fp_train_forward_f32:
per layer fpt_stats_kernel + fpt_stats_finalize_kernel, then fp_forward_kernel) and backward (ampnet_fp_train_backward_f32:
fpt_fold_kernel, L + 1 fpt_bwd_phase_kernel with fpt_bwd_finalize_kernel between them, fp_wgrad_kernel + fp_wgrad_reduce_kernel per layer,
fp_scatter_kernel) against torch's train-mode composition -- conv1d + batch_norm(training=True) + relu per layer -- on the SAME interpolated
rows, which torch is handed ready-made (the fused side interpolates in its forward and gathers dpoints2 in its backward).  Same protocol:
HIP events, `steps` calls after `warmup`, three alternating rounds, the median round reported.  Per-kernel times: a kernel-trace run of
this tool, on its own, never together with counters.
The bf16 leg ("bf16" in the JSON line): ampnet_fp_forward_bf16 (sa_fold_kernel, mlp_bf16_weights_kernel, fp_forward_bf16_kernel) on the same
inputs in the same process, timed against ampnet_fp_forward_f32 in three alternating rounds, every round reported.  A third argument
`forward` ends the run after the forward legs."""
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
B, N, S, D1, D2, MLP = 16, 8192, 1024, 0, 128, [128, 128, 128]
dev = "cuda"
fine = torch.from_numpy(synth.clouds(210, B, N)).to(dev)
coarse = U.gather_rows(fine, U.fps_indices(fine, S))                  # the coarse points are FPS centres of the fine ones, as after sa1
feats = torch.from_numpy(synth.uniform(211, (B, S, D2), -1.0, 1.0)).to(dev)
g = torch.Generator().manual_seed(0)
layers, cin = [], D1 + D2
for cout in MLP:
    layers.append(tuple(t.to(dev) for t in ((torch.rand(cout, cin, generator=g) - 0.5) * 2 / cin ** 0.5, (torch.rand(cout, generator=g) - 0.5) * 0.2,
                                            0.5 + torch.rand(cout, generator=g), torch.rand(cout, generator=g) - 0.5,
                                            (torch.rand(cout, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=g))))
    cin = cout
ws = torch.empty(L.FP_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
out = torch.empty((B, N, MLP[-1]), device=dev)
idx, dist2 = U.three_nn(fine, coarse)


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


def torch_layer(neighbours=None):
    """The same layer in torch, as a user of the usual implementation has it: the [B, N, S] distance matrix, the three smallest per row,
    the gathered [B, N, 3, D2] features and every activation go through memory.  neighbours = (idx, dist2): skip the search and use these
    (the comparison of the two outputs: cdist's matrix-product distances pick other neighbours at near-ties and turn a distance of 0
    into ~1e-7, and an inverse-distance mean over another third neighbour is another number)."""
    d, i = torch.cdist(fine, coarse).square().topk(3, dim=-1, largest=False) if neighbours is None else (neighbours[1], neighbours[0].long())
    r = 1.0 / (d + 1e-8)
    w = r / r.sum(-1, keepdim=True)
    x = (feats[torch.arange(B, device=dev)[:, None, None], i] * w[..., None]).sum(2).transpose(1, 2)      # [B, D2, N]
    for wt, b, gamma, beta, mean, var in layers:
        x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv1d(x, wt[:, :, None], b), mean, var, gamma, beta, False, 0.0, 1e-5))
    return x.transpose(1, 2)


with torch.no_grad():
    nn_ms = timed(lambda: U.three_nn(fine, coarse))
    fp_ms = timed(lambda: L.fp_forward_f32(None, feats, idx, dist2, layers, [1e-5] * len(MLP), out, ws))
    torch_ms = timed(torch_layer)
    err_same = float((out - torch_layer((idx, dist2))).abs().max())
    err_own = float((out - torch_layer()).abs().max())
    t_idx = torch.cdist(fine, coarse).topk(3, dim=-1, largest=False)[1]
    other = float((t_idx.sort(-1)[0] != idx.long().sort(-1)[0]).any(-1).float().mean())
    # ---- the bf16 leg: the two arithmetics in alternating rounds ----
    ws16 = torch.empty(L.fp_forward_bf16_workspace_bytes(D1, D2, B, N, MLP), dtype=torch.uint8, device=dev)
    out16 = torch.empty_like(out)
    fwd32 = lambda: L.fp_forward_f32(None, feats, idx, dist2, layers, [1e-5] * len(MLP), out, ws)
    fwd16 = lambda: L.fp_forward_bf16(None, feats, idx, dist2, layers, [1e-5] * len(MLP), out16, ws16)
    f_rounds = [(timed(fwd32), timed(fwd16)) for _ in range(3)]
    bf16 = {"fp_forward_f32_ms": round(sorted(r[0] for r in f_rounds)[1], 4), "fp_forward_bf16_ms": round(sorted(r[1] for r in f_rounds)[1], 4),
            "rounds_ms_f32_bf16": [[round(a, 4), round(b, 4)] for a, b in f_rounds],
            "f32_over_bf16": round(sorted(r[0] for r in f_rounds)[1] / sorted(r[1] for r in f_rounds)[1], 2),
            "max_abs_diff_bf16_vs_f32": float((out16 - out).abs().max()), "max_abs_out": float(out.abs().max())}
if len(sys.argv) > 3 and sys.argv[3] == "forward":
    print(json.dumps({"shape": {"B": B, "N": N, "S": S, "D1": D1, "D2": D2, "mlp": MLP}, "three_nn_ms": round(nn_ms, 4),
                      "fp_forward_ms": round(fp_ms, 4), "bf16": bf16}))
    sys.exit(0)

# ---- the backward leg -----------------------------------------------------------------------------------------------------------------
dout = torch.from_numpy(synth.uniform(212, (B, N, MLP[-1]), -1.0, 1.0)).to(dev)
bws = torch.empty(L.fp_backward_workspace_bytes(D1, D2, B, N, MLP), dtype=torch.uint8, device=dev)
dfeats = torch.empty_like(feats)
grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in layers]
fused_bwd = lambda: L.fp_backward_f32(None, feats, idx, dist2, layers, [1e-5] * len(MLP), dout, None, dfeats, grads, bws)
leaves = [feats.requires_grad_(True)] + [t.requires_grad_(True) for layer in layers for t in layer[:4]]
t_out = torch_layer((idx, dist2))
torch_bwd = lambda: torch.autograd.grad(t_out, leaves, dout, retain_graph=True)
rounds = [(timed(fused_bwd), timed(torch_bwd)) for _ in range(3)]
t_grads = torch_bwd()
fused_bwd()
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
bwd_diff = {"dpoints2": rel(dfeats, t_grads[0])}
for l in range(len(MLP)):
    for q, name in enumerate(("dW", "dbias", "dgamma", "dbeta")):
        bwd_diff[f"{name}{l}"] = rel(grads[l][q], t_grads[1 + 4 * l + q])
for t in leaves:
    t.requires_grad_(False)
fb_ms, tb_ms = sorted(r[0] for r in rounds)[1], sorted(r[1] for r in rounds)[1]
# useful flops of the backward: the recomputed forward (all layers), dx = dz W and dW = dz^T x per layer, the interpolation and its scatter
bwd_flops = 2.0 * B * N * (3 * sum(a * b for a, b in zip([D1 + D2] + MLP[:-1], MLP)) + 2 * 3 * D2)

# ---- the train-mode leg ---------------------------------------------------------------------------------------------------------------
A = importlib.import_module(PKG + ".autograd")
t_layers = [tuple(t.detach().clone() for t in layer) for layer in layers]                # the fused side's own running statistics
sum_c = sum(MLP)
save_mean, save_invstd = torch.empty(sum_c, device=dev), torch.empty(sum_c, device=dev)
fws = torch.empty(L.fp_train_forward_workspace_bytes(D1, D2, B, N, MLP), dtype=torch.uint8, device=dev)
tbws = torch.empty(L.fp_train_backward_workspace_bytes(D1, D2, B, N, MLP), dtype=torch.uint8, device=dev)
t_out_f = torch.empty((B, N, MLP[-1]), device=dev)
feats_d = feats.detach()
fused_tf = lambda: L.fp_train_forward_f32(None, feats_d, idx, dist2, t_layers, [1e-5] * len(MLP), 0.1, t_out_f, save_mean, save_invstd, fws)
fused_tb = lambda: L.fp_train_backward_f32(None, feats_d, idx, dist2, t_layers, [1e-5] * len(MLP), save_mean, save_invstd, dout, None, dfeats,
                                           grads, tbws)
with torch.no_grad():
    r = 1.0 / (dist2 + 1e-8)
    w = r / r.sum(-1, keepdim=True)
    x0 = (feats_d[torch.arange(B, device=dev)[:, None, None], idx.long()] * w[..., None]).sum(2).transpose(1, 2).contiguous()   # [B, D2, N]
x0.requires_grad_(True)
p_layers = [tuple(t.detach().clone() for t in layer) for layer in layers]                # torch's own running statistics
t_leaves = [x0] + [t.requires_grad_(True) for layer in p_layers for t in layer[:4]]


def torch_train():
    x = x0
    for wt, b, gamma, beta, mean, var in p_layers:
        x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv1d(x, wt[:, :, None], b), mean, var, gamma, beta, True, 0.1, 1e-5))
    return x.transpose(1, 2)


def torch_train_fwd():
    with torch.no_grad():
        torch_train()


tt_out = torch_train()
torch_tb = lambda: torch.autograd.grad(tt_out, t_leaves, dout, retain_graph=True)
t_rounds = [(timed(fused_tf), timed(torch_train_fwd), timed(fused_tb), timed(torch_tb)) for _ in range(3)]
fused_tf()
fused_tb()
tt_grads = torch_tb()
train_diff = {"out": rel(t_out_f, tt_out.detach())}
for l in range(len(MLP)):
    for q, name in enumerate(("dW", "dbias", "dgamma", "dbeta")):
        if name != "dbias":                                                              # (zeros on one side, roundings of zero on the other)
            train_diff[f"{name}{l}"] = rel(grads[l][q], tt_grads[1 + 4 * l + q])
# torch's statistics differ from the fused ones in the last bits, so a few of the 16.8 M ReLU inputs per layer change sign between the two and each
# moves a gradient by a whole term; the fused dbeta of the last layer against a float64 sum over the fused output's OWN mask tells the two apart
mask = t_out_f > 0
train_diff["last_layer_relu_sign_mismatches_vs_torch"] = int((mask != (tt_out.detach() > 0)).sum())
own = (dout.double() * mask).sum((0, 1))
train_diff["dbeta_last_vs_float64_sum_over_own_mask"] = float((grads[-1][3].double() - own).abs().max() / own.abs().max())
med = lambda q: sorted(r[q] for r in t_rounds)[1]
train = {"fp_train_forward_ms": round(med(0), 4), "torch_train_forward_ms": round(med(1), 4), "fp_train_backward_ms": round(med(2), 4),
         "torch_train_backward_ms": round(med(3), 4), "torch_forward_over_fused": round(med(1) / med(0), 2),
         "torch_backward_over_fused": round(med(3) / med(2), 2), "train_forward_over_eval_forward": round(med(0) / fp_ms, 2),
         "train_backward_over_eval_backward": round(med(2) / fb_ms, 2),
         "rounds_ms_fused_fwd_torch_fwd_fused_bwd_torch_bwd": [[round(v, 4) for v in r] for r in t_rounds],
         "train_forward_workspace_MB": round(fws.numel() / 1e6, 2), "train_backward_workspace_MB": round(tbws.numel() / 1e6, 1),
         "max_rel_diff_vs_torch": train_diff}

w_bytes = sum(sum(t.numel() for t in layer) for layer in layers) * 4
# the algorithmic bytes of the fused forward: the coarse features once, the neighbours and distances, the weights, the output
algo = B * S * D2 * 4 + B * N * 3 * 8 + w_bytes + B * N * MLP[-1] * 4
flops = 2.0 * B * N * (3 * D2 + sum(a * b for a, b in zip([D1 + D2] + MLP[:-1], MLP)))
print(json.dumps({"shape": {"B": B, "N": N, "S": S, "D1": D1, "D2": D2, "mlp": MLP}, "three_nn_ms": round(nn_ms, 4),
                  "fp_forward_ms": round(fp_ms, 4), "torch_cdist_topk_gather_conv1d_ms": round(torch_ms, 4),
                  "torch_over_three_nn_plus_fused": round(torch_ms / (nn_ms + fp_ms), 2),
                  "fp_algorithmic_bytes": algo, "fp_GBps_at_algorithmic_bytes": round(algo / (fp_ms * 1e-3) / 1e9, 1),
                  "fp_useful_TFLOPs": round(flops / (fp_ms * 1e-3) / 1e12, 2), "max_abs_diff_vs_torch_on_the_same_neighbours": err_same,
                  "max_abs_diff_vs_torch_on_its_own_neighbours": err_own, "rows_where_torch_picks_other_neighbours": other,
                  "fp_backward_ms": round(fb_ms, 4), "torch_backward_ms": round(tb_ms, 4), "torch_backward_over_fused": round(tb_ms / fb_ms, 2),
                  "backward_rounds_ms_fused_torch": [[round(a, 4), round(b, 4)] for a, b in rounds],
                  "fp_backward_useful_TFLOPs": round(bwd_flops / (fb_ms * 1e-3) / 1e12, 2), "fp_backward_workspace_MB": round(bws.numel() / 1e6, 1),
                  "backward_max_rel_diff_vs_torch": bwd_diff, "backward_hbm_counters": "not measured", "train": train, "bf16": bf16}))
