"""Ball query + fused set-abstraction forward at the reference's sa1 shape (B = 16, N = 8192, npoint = 1024, nsample = 32, D = 9,
MLP [32, 32, 64]) against what torch-ROCm offers for the same layer: gather + conv2d + BatchNorm2d (eval) + relu + max.
python3 tools/prof_sa.py [steps] [warmup]  -- HIP events, warm-up first, both sides in this process; prints one JSON line.
Under rocprofv3 (counters in a run of their own) the kernels to look for are ball_query_kernel and sa_forward_kernel.
The backward leg, at the sa1, sa2 and sa3 shapes of pointnet_2 at B = 16 (sa2's cloud is sa1's centres, sa3's is sa2's): the fused backward
(ampnet_sa_backward_f32: sa_fold_kernel, sa_backward_kernel, fp_wgrad_kernel + fp_wgrad_reduce_kernel per layer, sa_dfeats_kernel,
fp_bwd_finalize_kernel) against torch.autograd's backward of the torch composition below on the SAME groups (graph built once and retained,
only the backward is timed); the two are timed in alternating rounds and every round is reported.  sa1's features are the input data, so
its dfeats is not requested, as in the model; sa2 and sa3 are also timed without dfeats, which prices layer 0's dx plus the gather.
python3 tools/prof_sa.py [steps] [warmup] trace  -- runs nothing but the fused backward, `steps` times per shape, for a
`rocprofv3 --kernel-trace --stats` run that splits it by kernel (sa2 and sa3 with dfeats: sa_dfeats_kernel's own time is in that split).
The train-mode leg, at the same three shapes: the fused train forward and backward (ampnet_sa_train_forward_f32: sat_stats_kernel +
fpt_stats_finalize_kernel per layer, sa_forward_kernel; ampnet_sa_train_backward_f32: fpt_fold_kernel, sat_bwd_last_kernel,
sat_bwd_phase_kernel per remaining phase, fpt_bwd_finalize_kernel per layer, fp_wgrad_kernel + fp_wgrad_reduce_kernel per layer,
sa_dfeats_kernel) against torch's train-mode composition (batch_norm(training=True), forward under no_grad and the backward of a retained
graph) and against this project's eval forward and eval backward, in alternating rounds, every round reported.
python3 tools/prof_sa.py [steps] [warmup] train        -- the train-mode leg alone; prints one JSON line.
python3 tools/prof_sa.py [steps] [warmup] train-trace  -- nothing but the fused train forward and backward, for a kernel trace.
The group_all leg: one group of all N points per cloud at B = 16, D = 256, MLP [256, 256, 256], N = 64 and N = 1024 side by side -- the fused
forward (ampnet_sa_all_forward_f32: sa_fold_kernel, sa_all_forward_kernel, sa_all_reduce_kernel) and backward (ampnet_sa_all_backward_f32:
sa_all_compact_kernel, the kernels of ampnet_sa_backward_f32 on the compacted winners, a memset of dfeats, sa_all_scatter_kernel) against
torch's composition conv2d 1x1 + eval batch_norm + relu on [B, C, N, 1], then max (forward under no_grad, the backward of a retained graph),
in alternating rounds, every round reported.  The backward works on the winners alone: its time should not grow with N.
python3 tools/prof_sa.py [steps] [warmup] group_all        -- the group_all leg alone; prints one JSON line.
python3 tools/prof_sa.py [steps] [warmup] group_all-trace  -- nothing but the fused group_all forward and backward, for a kernel trace.
The msg leg: multi-scale grouping with two scales at B = 16, an sa1-like shape (this file's N = 8192 cloud, 1024 centres, radii (0.1, 0.2),
nsample (16, 32), D = 9, [32, 32, 64] twice) and an sa3-like one (a 256-point cloud, 64 centres, radii (0.4, 0.8), nsample (16, 32), D = 128,
[128, 128, 256] twice): (a) one utils.ball_query_msg (ball_query_kernel<2>) against two utils.ball_query calls (ball_query_kernel<1>), and the same pair again as
bare kernels on preallocated outputs, without the helpers' validation of the centres; (b) one sa_msg_forward_f32 (two sa_fold_kernel launches,
sa_msg_forward_kernel) against two sa_forward_f32 calls plus torch.cat.  Five alternating rounds, every round reported, medians quoted.
python3 tools/prof_sa.py [steps] [warmup] msg        -- the msg leg alone; prints one JSON line.
python3 tools/prof_sa.py [steps] [warmup] msg-trace  -- nothing but ball_query_msg and sa_msg_forward_f32, for a kernel trace.
The bf16 leg, at the sa1 shape above: ampnet_sa_forward_bf16 (sa_fold_kernel, mlp_bf16_weights_kernel, sa_forward_bf16_kernel) against
ampnet_sa_forward_f32 on the same groups in the same process, three alternating rounds, every round reported ("bf16" in the JSON line).
python3 tools/prof_sa.py [steps] [warmup] bf16       -- the bf16 leg alone; prints one JSON line."""
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
mode = sys.argv[3] if len(sys.argv) > 3 else ""
trace_only = mode == "trace"
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


def make_layers(cin, mlp, seed):
    gen, res = torch.Generator().manual_seed(seed), []
    for cout in mlp:
        res.append(tuple(t.to(dev) for t in ((torch.rand(cout, cin, generator=gen) - 0.5) * 2 / cin ** 0.5, (torch.rand(cout, generator=gen) - 0.5) * 0.2,
                                             0.5 + torch.rand(cout, generator=gen), torch.rand(cout, generator=gen) - 0.5,
                                             (torch.rand(cout, generator=gen) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=gen))))
        cin = cout
    return res


def torch_sa(pts, f, c, gi, lay):
    """torch_layer() on any cloud: gather, 1x1 conv, eval BatchNorm, ReLU, max."""
    b = pts.shape[0]
    bi = torch.arange(b, device=dev)[:, None, None]
    g_xyz = pts[bi, gi.long()] - pts[torch.arange(b, device=dev)[:, None], c.long()][:, :, None, :]
    x = torch.cat([g_xyz, f[bi, gi.long()]], -1).permute(0, 3, 1, 2)
    for w, bias, gamma, beta, mean, var in lay:
        x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w[:, :, None, None], bias), mean, var, gamma, beta, False, 0.0, 1e-5))
    return x.max(-1)[0].transpose(1, 2)


def backward_leg():
    """-> {block: figures} for sa1, sa2, sa3 of pointnet_2 at B = 16."""
    res, pts = {}, xyz
    for block, (s_, k_, d_, mlp, radius, want_df) in {"sa1": (1024, 32, 9, [32, 32, 64], 0.1, False), "sa2": (256, 32, 64, [64, 64, 128], 0.2, True),
                                                      "sa3": (64, 32, 128, [128, 128, 256], 0.4, True)}.items():
        n_ = pts.shape[1]
        f = torch.from_numpy(synth.uniform(220 + d_, (B, n_, d_), -1.0, 1.0)).to(dev)
        c = U.fps_indices(pts, s_)
        gi = U.ball_query(pts, c, radius, k_)
        lay = make_layers(3 + d_, mlp, d_)
        dout = torch.from_numpy(synth.uniform(230 + d_, (B, s_, mlp[-1]), -1.0, 1.0)).to(dev)
        bws = torch.empty(L.sa_backward_workspace_bytes(d_, B, s_, k_, mlp), dtype=torch.uint8, device=dev)
        df = torch.empty_like(f)
        grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in lay]
        eps = [1e-5] * len(mlp)
        fused = lambda with_df: L.sa_backward_f32(pts, c, gi, f, lay, eps, dout, df if with_df else None, grads, bws)
        if trace_only:
            for _ in range(steps):
                fused(want_df)
            torch.cuda.synchronize()
            pts = U.gather_rows(pts, c)
            continue
        leaves = ([f.requires_grad_(True)] if want_df else []) + [t.requires_grad_(True) for layer in lay for t in layer[:4]]
        t_out = torch_sa(pts, f, c, gi, lay)
        torch_bwd = lambda: torch.autograd.grad(t_out, leaves, dout, retain_graph=True)
        rounds = [(timed(lambda: fused(want_df)), timed(torch_bwd)) for _ in range(3)]
        no_df_ms = timed(lambda: fused(False)) if want_df else None
        t_grads = torch_bwd()
        fused(want_df)
        rel = lambda a, b_: float((a - b_).abs().max() / b_.abs().max())
        diff = {"dfeats": rel(df, t_grads[0])} if want_df else {}
        for l in range(len(mlp)):
            for q, name in enumerate(("dW", "dbias", "dgamma", "dbeta")):
                diff[f"{name}{l}"] = rel(grads[l][q], t_grads[int(want_df) + 4 * l + q])
        for t in leaves:
            t.requires_grad_(False)
        fb, tb = sorted(r[0] for r in rounds)[1], sorted(r[1] for r in rounds)[1]
        M = B * s_ * k_
        cins = [3 + d_] + mlp[:-1]
        # the workspace traffic by construction: x_l and dz_l of every row written once by sa_backward_kernel and read by fp_wgrad_kernel
        # once per 32-row block of dW (x_l) / per 128-column block of dW (dz_l); dx_0 written once and read by the gather
        ldxs = [(ci + 31) // 32 * 32 for ci in cins]
        written = 4 * M * (sum(ldxs) + sum(mlp) + (d_ if want_df else 0))
        wgrad_reads = 4 * M * sum(lx * (co // 32) + co * ((lx + 127) // 128) for lx, co in zip(ldxs, mlp))
        flops = 2.0 * M * (3 * sum(a * b_ for a, b_ in zip(cins, mlp)) - (0 if want_df else cins[0] * mlp[0]))
        res[block] = {"shape": {"B": B, "N": n_, "npoint": s_, "nsample": k_, "D": d_, "mlp": mlp, "radius": radius, "dfeats": want_df},
                      "sa_backward_ms": round(fb, 4), "torch_backward_ms": round(tb, 4), "torch_backward_over_fused": round(tb / fb, 2),
                      "rounds_ms_fused_torch": [[round(a, 4), round(b_, 4)] for a, b_ in rounds],
                      "sa_backward_without_dfeats_ms": None if no_df_ms is None else round(no_df_ms, 4),
                      "layer0_dx_plus_gather_ms": None if no_df_ms is None else round(fb - no_df_ms, 4),
                      "useful_TFLOPs": round(flops / (fb * 1e-3) / 1e12, 2), "workspace_MB": round(bws.numel() / 1e6, 1),
                      "workspace_bytes_written_by_construction_MB": round(written / 1e6, 1),
                      "workspace_bytes_read_by_wgrad_by_construction_MB": round(wgrad_reads / 1e6, 1),
                      "max_rel_diff_vs_torch": diff, "hbm_counters": "not measured"}
        pts = U.gather_rows(pts, c)
    return res


def train_leg(trace):
    """-> {block: figures} for sa1, sa2, sa3 of pointnet_2 at B = 16 in train mode (batch statistics over all B npoint nsample rows)."""
    res, pts = {}, xyz
    for block, (s_, k_, d_, mlp, radius, want_df) in {"sa1": (1024, 32, 9, [32, 32, 64], 0.1, False), "sa2": (256, 32, 64, [64, 64, 128], 0.2, True),
                                                      "sa3": (64, 32, 128, [128, 128, 256], 0.4, True)}.items():
        n_ = pts.shape[1]
        f = torch.from_numpy(synth.uniform(220 + d_, (B, n_, d_), -1.0, 1.0)).to(dev)
        c = U.fps_indices(pts, s_)
        gi = U.ball_query(pts, c, radius, k_)
        lay = make_layers(3 + d_, mlp, d_)                                    # the fused side's own running statistics
        dout = torch.from_numpy(synth.uniform(230 + d_, (B, s_, mlp[-1]), -1.0, 1.0)).to(dev)
        eps, sum_c = [1e-5] * len(mlp), sum(mlp)
        fws = torch.empty(L.sa_train_forward_workspace_bytes(d_, B, s_, k_, mlp), dtype=torch.uint8, device=dev)
        bws = torch.empty(L.sa_train_backward_workspace_bytes(d_, B, s_, k_, mlp), dtype=torch.uint8, device=dev)
        ews = torch.empty(L.sa_backward_workspace_bytes(d_, B, s_, k_, mlp), dtype=torch.uint8, device=dev)
        sm, si = torch.empty(sum_c, device=dev), torch.empty(sum_c, device=dev)
        o, df = torch.empty((B, s_, mlp[-1]), device=dev), torch.empty_like(f)
        grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in lay]
        fused_f = lambda: L.sa_train_forward_f32(pts, c, gi, f, lay, eps, 0.1, o, sm, si, fws)
        fused_b = lambda: L.sa_train_backward_f32(pts, c, gi, f, lay, eps, sm, si, dout, df if want_df else None, grads, bws)
        if trace:
            for _ in range(steps):
                fused_f()
                fused_b()
            torch.cuda.synchronize()
            pts = U.gather_rows(pts, c)
            continue
        e_lay = make_layers(3 + d_, mlp, d_)
        eval_f = lambda: L.sa_forward_f32(pts, c, gi, f, e_lay, eps, o, ws)
        eval_b = lambda: L.sa_backward_f32(pts, c, gi, f, e_lay, eps, dout, df if want_df else None, grads, ews)
        p_lay = make_layers(3 + d_, mlp, d_)                                  # torch's own running statistics
        bi = torch.arange(B, device=dev)[:, None, None]
        fg = f.detach().clone().requires_grad_(want_df)
        leaves = ([fg] if want_df else []) + [t.requires_grad_(True) for layer in p_lay for t in layer[:4]]

        def torch_train():
            g_xyz = pts[bi, gi.long()] - pts[torch.arange(B, device=dev)[:, None], c.long()][:, :, None, :]
            x = torch.cat([g_xyz, fg[bi, gi.long()]], -1).permute(0, 3, 1, 2)
            for w, bias, gamma, beta, mean, var in p_lay:
                x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w[:, :, None, None], bias), mean, var, gamma, beta, True,
                                                              0.1, 1e-5))
            return x.max(-1)[0].transpose(1, 2)

        def torch_f():
            with torch.no_grad():
                torch_train()

        t_out = torch_train()
        torch_b = lambda: torch.autograd.grad(t_out, leaves, dout, retain_graph=True)
        rounds = [(timed(fused_f), timed(torch_f), timed(fused_b), timed(torch_b), timed(eval_f), timed(eval_b)) for _ in range(3)]
        fused_f()
        fused_b()
        t_grads = torch_b()
        rel = lambda a, b_: float((a - b_).abs().max() / b_.abs().max())
        diff = {"out": rel(o, t_out.detach())}
        if want_df:
            diff["dfeats"] = rel(df, t_grads[0])
        for l in range(len(mlp)):
            for q, name in enumerate(("dW", "dbias", "dgamma", "dbeta")):
                if name != "dbias":                                          # (zeros on one side, roundings of zero on the other)
                    diff[f"{name}{l}"] = rel(grads[l][q], t_grads[int(want_df) + 4 * l + q])
        for t in leaves:
            t.requires_grad_(False)
        med = lambda q: sorted(r[q] for r in rounds)[1]
        res[block] = {"shape": {"B": B, "N": n_, "npoint": s_, "nsample": k_, "D": d_, "mlp": mlp, "radius": radius, "dfeats": want_df},
                      "sa_train_forward_ms": round(med(0), 4), "torch_train_forward_ms": round(med(1), 4),
                      "sa_train_backward_ms": round(med(2), 4), "torch_train_backward_ms": round(med(3), 4),
                      "sa_eval_forward_ms": round(med(4), 4), "sa_eval_backward_ms": round(med(5), 4),
                      "torch_forward_over_fused": round(med(1) / med(0), 2), "torch_backward_over_fused": round(med(3) / med(2), 2),
                      "train_forward_over_eval_forward": round(med(0) / med(4), 2), "train_backward_over_eval_backward": round(med(2) / med(5), 2),
                      "rounds_ms_fused_fwd_torch_fwd_fused_bwd_torch_bwd_eval_fwd_eval_bwd": [[round(v, 4) for v in r] for r in rounds],
                      "train_forward_workspace_MB": round(fws.numel() / 1e6, 2), "train_backward_workspace_MB": round(bws.numel() / 1e6, 1),
                      "max_rel_diff_vs_torch": diff}
        pts = U.gather_rows(pts, c)
    return res


def group_all_leg(trace):
    """-> {"n64": figures, "n1024": figures}: one group of all points, B = 16, D = 256, [256, 256, 256]."""
    res, d_, mlp = {}, 256, [256, 256, 256]
    for n_ in (64, 1024):
        pts = torch.from_numpy(synth.clouds(240, B, n_)).to(dev)
        f = torch.from_numpy(synth.uniform(241, (B, n_, d_), -1.0, 1.0)).to(dev)
        lay = make_layers(3 + d_, mlp, 7)
        dout = torch.from_numpy(synth.uniform(242, (B, mlp[-1]), -1.0, 1.0)).to(dev)
        eps = [1e-5] * len(mlp)
        fws = torch.empty(L.sa_all_forward_workspace_bytes(d_, B, n_, mlp), dtype=torch.uint8, device=dev)
        bws = torch.empty(L.sa_all_backward_workspace_bytes(d_, B, n_, mlp), dtype=torch.uint8, device=dev)
        o, arg = torch.empty((B, mlp[-1]), device=dev), torch.empty((B, mlp[-1]), dtype=torch.int32, device=dev)
        df = torch.empty_like(f)
        grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in lay]
        fused_f = lambda: L.sa_all_forward_f32(pts, f, lay, eps, o, fws, arg_out=arg)
        fused_b = lambda: L.sa_all_backward_f32(pts, f, lay, eps, arg, dout, df, grads, bws)
        fused_f()                                                             # (the backward takes the forward's arg)
        if trace:
            for _ in range(steps):
                fused_f()
                fused_b()
            torch.cuda.synchronize()
            continue
        fg = f.detach().clone().requires_grad_(True)
        leaves = [fg] + [t.requires_grad_(True) for layer in lay for t in layer[:4]]

        def torch_all():
            x = torch.cat([pts, fg], -1).permute(0, 2, 1)[..., None]          # [B, C, N, 1]
            for w, bias, gamma, beta, mean, var in lay:
                x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w[:, :, None, None], bias), mean, var, gamma, beta, False,
                                                              0.0, 1e-5))
            return x.max(2)[0].squeeze(-1)

        def torch_f():
            with torch.no_grad():
                torch_all()

        t_out = torch_all()
        torch_b = lambda: torch.autograd.grad(t_out, leaves, dout, retain_graph=True)
        rounds = [(timed(fused_f), timed(torch_f), timed(fused_b), timed(torch_b)) for _ in range(3)]
        fused_f()
        fused_b()
        t_grads = torch_b()
        rel = lambda a, b_: float((a - b_).abs().max() / b_.abs().max())
        diff = {"out": rel(o, t_out.detach()), "dfeats": rel(df, t_grads[0])}
        for l in range(len(mlp)):
            for q, name in enumerate(("dW", "dbias", "dgamma", "dbeta")):
                diff[f"{name}{l}"] = rel(grads[l][q], t_grads[1 + 4 * l + q])
        for t in leaves:
            t.requires_grad_(False)
        med = lambda q: sorted(r[q] for r in rounds)[1]
        flops = 2.0 * B * n_ * sum(a * b_ for a, b_ in zip([3 + d_] + mlp[:-1], mlp))
        res[f"n{n_}"] = {"shape": {"B": B, "N": n_, "D": d_, "mlp": mlp},
                         "sa_all_forward_ms": round(med(0), 4), "torch_forward_ms": round(med(1), 4),
                         "sa_all_backward_ms": round(med(2), 4), "torch_backward_ms": round(med(3), 4),
                         "torch_forward_over_fused": round(med(1) / med(0), 2), "torch_backward_over_fused": round(med(3) / med(2), 2),
                         "rounds_ms_fused_fwd_torch_fwd_fused_bwd_torch_bwd": [[round(v, 4) for v in r] for r in rounds],
                         "forward_useful_TFLOPs": round(flops / (med(0) * 1e-3) / 1e12, 2),
                         "distinct_winners_per_cloud_mean": round(float(sum(len(torch.unique(a)) for a in arg) / B), 1),
                         "forward_workspace_MB": round(fws.numel() / 1e6, 2), "backward_workspace_MB": round(bws.numel() / 1e6, 2),
                         "max_rel_diff_vs_torch": diff}
    return res


def msg_leg(trace):
    """-> {"sa1_like": figures, "sa3_like": figures}: two scales around the same centres at B = 16, (a) one ball_query_msg against two
    ball_query calls, (b) one sa_msg_forward_f32 against two sa_forward_f32 calls plus torch.cat -- the baselines are the single-scale
    building blocks, never the new code."""
    res = {}
    pts3 = U.gather_rows(xyz, cent)                                           # sa2's cloud: sa1's 1024 centres
    pts3 = U.gather_rows(pts3, U.fps_indices(pts3, 256))                      # sa3's cloud: sa2's 256 centres
    for name, (pts, s_, radii, ks, d_, mlps) in {"sa1_like": (xyz, 1024, (0.1, 0.2), (16, 32), 9, [[32, 32, 64], [32, 32, 64]]),
                                                 "sa3_like": (pts3, 64, (0.4, 0.8), (16, 32), 128, [[128, 128, 256], [128, 128, 256]])}.items():
        n_, nb = pts.shape[1], len(radii)
        f = torch.from_numpy(synth.uniform(250 + d_, (B, n_, d_), -1.0, 1.0)).to(dev)
        c = cent if pts is xyz else U.fps_indices(pts, s_)
        lays = [make_layers(3 + d_, mlp, 260 + i) for i, mlp in enumerate(mlps)]
        eps = [[1e-5] * len(mlp) for mlp in mlps]
        gis, cnts = U.ball_query_msg(pts, c, radii, ks, return_counts=True)
        mws = torch.empty(L.sa_msg_forward_workspace_bytes(nb), dtype=torch.uint8, device=dev)
        wss = [torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device=dev) for _ in range(nb)]
        o = torch.empty((B, s_, sum(mlp[-1] for mlp in mlps)), device=dev)
        parts = [torch.empty((B, s_, mlp[-1]), device=dev) for mlp in mlps]
        bq_msg = lambda: U.ball_query_msg(pts, c, radii, ks)
        bq_each = lambda: [U.ball_query(pts, c, r, k_) for r, k_ in zip(radii, ks)]
        sa_msg = lambda: L.sa_msg_forward_f32(pts, c, gis, f, lays, eps, o, mws)
        # the two queries again without the helpers' validation (its read-back): the kernels alone, on preallocated outputs
        raw_msg = lambda: L.ball_query_msg_f32(pts, c, radii, ks, gis)
        raw_each = lambda: [L.ball_query_f32(pts, c, r, k_, gi) for r, k_, gi in zip(radii, ks, gis)]

        def sa_each():
            for gi, lay, e, part, w in zip(gis, lays, eps, parts, wss):
                L.sa_forward_f32(pts, c, gi, f, lay, e, part, w)
            return torch.cat(parts, dim=2)

        if trace:
            for _ in range(steps):
                bq_msg()
                sa_msg()
            torch.cuda.synchronize()
            continue
        with torch.no_grad():
            rounds = [(timed(bq_msg), timed(bq_each), timed(sa_msg), timed(sa_each), timed(raw_msg), timed(raw_each)) for _ in range(5)]
            sa_msg()
            same = bool(torch.equal(o, sa_each())) and all(bool(torch.equal(a, b_)) for a, b_ in zip(bq_msg(), bq_each()))
        med = lambda q: sorted(r[q] for r in rounds)[len(rounds) // 2]
        res[name] = {"shape": {"B": B, "N": n_, "npoint": s_, "radii": radii, "nsample": ks, "D": d_, "mlps": mlps},
                     "mean_members": [round(float(t.float().mean()), 2) for t in cnts],
                     "ball_query_msg_ms": round(med(0), 4), "ball_query_each_ms": round(med(1), 4),
                     "sa_msg_forward_ms": round(med(2), 4), "sa_forward_each_plus_cat_ms": round(med(3), 4),
                     "ball_query_msg_kernel_ms": round(med(4), 4), "ball_query_each_kernels_ms": round(med(5), 4),
                     "each_over_msg_ball_query": round(med(1) / med(0), 2), "each_over_msg_forward": round(med(3) / med(2), 2),
                     "each_over_msg_ball_query_kernels": round(med(5) / med(4), 2),
                     "rounds_ms_bq_msg_bq_each_sa_msg_sa_each_kernel_msg_kernel_each": [[round(v, 4) for v in r] for r in rounds],
                     "bitwise_equal_to_the_single_scale_calls": same}
    return res


def bf16_leg():
    """The eval forward under its two arithmetics at the sa1 shape, in alternating rounds."""
    with torch.no_grad():
        ws16 = torch.empty(L.sa_forward_bf16_workspace_bytes(D, B, S, K, MLP), dtype=torch.uint8, device=dev)
        out16 = torch.empty_like(out)
        fwd32 = lambda: L.sa_forward_f32(xyz, cent, grp, feats, layers, [1e-5] * len(MLP), out, ws)
        fwd16 = lambda: L.sa_forward_bf16(xyz, cent, grp, feats, layers, [1e-5] * len(MLP), out16, ws16)
        rounds = [(timed(fwd32), timed(fwd16)) for _ in range(3)]
        m32, m16 = sorted(r[0] for r in rounds)[1], sorted(r[1] for r in rounds)[1]
        return {"sa_forward_f32_ms": round(m32, 4), "sa_forward_bf16_ms": round(m16, 4), "f32_over_bf16": round(m32 / m16, 2),
                "rounds_ms_f32_bf16": [[round(a, 4), round(b, 4)] for a, b in rounds],
                "max_abs_diff_bf16_vs_f32": float((out16 - out).abs().max()), "max_abs_out": float(out.abs().max())}


if mode == "bf16":
    print(json.dumps({"shape": {"B": B, "N": N, "npoint": S, "nsample": K, "D": D, "mlp": MLP, "radius": RADIUS}, "bf16": bf16_leg()}))
    sys.exit(0)

if mode in ("msg", "msg-trace"):
    r = msg_leg(mode == "msg-trace")
    print(json.dumps({"trace_only": True, "msg_calls_per_shape": steps} if mode == "msg-trace" else {"msg": r}))
    sys.exit(0)

if mode in ("group_all", "group_all-trace"):
    r = group_all_leg(mode == "group_all-trace")
    print(json.dumps({"trace_only": True, "fused_group_all_calls_per_shape": steps} if mode == "group_all-trace" else {"group_all": r}))
    sys.exit(0)

if mode in ("train", "train-trace"):
    r = train_leg(mode == "train-trace")
    print(json.dumps({"trace_only": True, "fused_train_calls_per_shape": steps} if mode == "train-trace" else {"train": r}))
    sys.exit(0)

if trace_only:
    backward_leg()
    print(json.dumps({"trace_only": True, "fused_backward_calls_per_shape": steps}))
    sys.exit(0)

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
                  "sa_useful_TFLOPs": round(flops / (sa_ms * 1e-3) / 1e12, 2), "max_abs_diff_vs_torch": err, "backward": backward_leg(), "train": train_leg(False),
                  "bf16": bf16_leg()}))
