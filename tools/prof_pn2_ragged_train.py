"""pointnet_2_seg TRAINING on clouds packed back to back (forward_ragged with a graph, train mode) against the uniform path, and the one
kernel that makes it affordable.  python3 tools/prof_pn2_ragged_train.py [steps] [warmup]  -- HIP events around `steps` calls after
`warmup` calls, the two sides in ALTERNATING rounds in this one process, the median of 5 rounds reported and every round listed; prints
one JSON line.

(a) a train step (zero_grad, forward, seg_nll_loss, backward, FusedAdam.step) of pointnet_2_seg with all five flags in train mode on 16
    clouds of 2048 points: through forward_ragged on the packed [32768, 9] rows against forward_rows on the same rows as [16, 2048, 9].
    Equal work -- the same searches, rows, statistics and gradients -- so the two are expected to be close; the ragged side pays the
    ragged searches and ONE launch of each of sa1's and fp1's kernels over all clouds.  The losses of the two sides are compared.
(b) fp1's backward (D1 = 0, D2 = 128, three layers of 128, 1024 coarse points per cloud) on the packed array of those 16 clouds through
    ampnet_fp_backward_ragged_f32 against ampnet_fp_backward_f32 on the same array as one cloud: the same phases, the dpoints2 gather
    scanning a coarse point's own cloud (2048 x 3 entries) or the whole array (32768 x 3).  The outputs are the same bits (compared).
Under rocprofv3 (a kernel trace in a run of its own) the kernels to look for are fp_scatter_ragged_kernel and fp_scatter_kernel."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
PKG = "3d-semantic-segmentation-amp-net_amd"
sub = lambda name: importlib.import_module(PKG + "." + name)
synth, A, P, U, L, T = (sub(n) for n in ("synthetic", "pointNet.model.pointnetAtt", "pointNet.model.pointnet2_utils", "utils.utils", "_lib",
                                         "trainer"))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ROUNDS, CLOUDS, N, S1 = 5, 16, 2048, 1024
assert torch.cuda.is_available(), "tools/prof_pn2_ragged_train.py measures on the GPU"
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
x = np.concatenate([synth.clouds(900, CLOUDS, N), synth.uniform(901, (CLOUDS, N, 6), -1.0, 1.0)], -1).astype(np.float32)
rows = torch.from_numpy(x).to(dev)                                   # [16, 2048, 9]
packed, sizes = rows.reshape(CLOUDS * N, 9), [N] * CLOUDS
target = torch.from_numpy(synth.randint(902, (CLOUDS, N), 0, 5)).to(dev)
class_w = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=dev)


def train_step_leg():
    def side(forward, tg):
        torch.manual_seed(0)
        net = A.pointnet_2_seg(5, device=dev, decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True,
                               head_batch_stats=True).train()
        opt = T.FusedAdam(net.parameters(), lr=1e-3)
        last = {}

        def step():
            opt.zero_grad()
            loss, _, _ = P.seg_nll_loss(forward(net), tg, class_w)
            loss.backward()
            opt.step()
            last["loss"] = loss.detach()

        return step, last

    ragged, lr = side(lambda net: net.forward_ragged(packed, sizes), target.reshape(-1))
    uniform, lu = side(lambda net: net.forward_rows(rows), target)
    rounds = [(timed(ragged), timed(uniform)) for _ in range(ROUNDS)]
    # (both sides ran the same number of steps from the same state: equal statistics, equal masks, the losses agree to float32 sums)
    return {"clouds": CLOUDS, "points_per_cloud": N, "forward_ragged_step_ms": round(med(rounds, 0), 3),
            "forward_rows_step_ms": round(med(rounds, 1), 3), "ragged_over_rows": round(med(rounds, 0) / med(rounds, 1), 3),
            "rounds_ms_ragged_rows": [[round(v, 3) for v in r] for r in rounds], "last_loss_ragged": float(lr["loss"]),
            "last_loss_rows": float(lu["loss"])}


def fp1_backward_leg():
    g = torch.Generator().manual_seed(3)
    xyz = packed[:, :3].contiguous()
    layout = U.ragged_layout("prof", xyz, sizes)
    centres = torch.stack(U.fps_indices_ragged(xyz, sizes, S1))
    coarse = xyz[(centres + layout.off[:-1].unsqueeze(1)).long()].contiguous()        # [16, 1024, 3]
    idx, dist2 = (t.unsqueeze(0) for t in U.three_nn_ragged(xyz, layout, coarse, global_index=True))
    p2 = (torch.rand((1, CLOUDS * S1, 128), generator=g) - 0.5).to(dev)
    dout = (torch.rand((1, CLOUDS * N, 128), generator=g) - 0.5).to(dev)
    layers, cin = [], 128
    for cout in (128, 128, 128):
        w = (torch.rand((cout, cin), generator=g) - 0.5) * (2.0 / cin ** 0.5)
        vec = [(torch.rand(cout, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=g), (torch.rand(cout, generator=g) - 0.5) * 0.6,
               (torch.rand(cout, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=g)]
        layers.append(tuple(t.to(dev) for t in [w] + vec))
        cin = cout
    ws = torch.empty(L.fp_backward_workspace_bytes(0, 128, 1, CLOUDS * N, [128, 128, 128]), dtype=torch.uint8, device=dev)
    outs = {}

    def run(name, cloud_off):
        dp2 = torch.empty_like(p2)
        grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in layers]
        outs[name] = (dp2, grads)
        L.fp_backward_f32(None, p2, idx, dist2, layers, [1e-5] * 3, dout, None, dp2, grads, ws, cloud_off=cloud_off)

    rounds = [(timed(lambda: run("ragged", layout.off)), timed(lambda: run("one_cloud", None))) for _ in range(ROUNDS)]
    same = torch.equal(outs["ragged"][0], outs["one_cloud"][0]) and all(torch.equal(a, b) for ga, gb in zip(outs["ragged"][1], outs["one_cloud"][1])
                                                                         for a, b in zip(ga, gb))
    return {"clouds": CLOUDS, "fine_rows": CLOUDS * N, "coarse_per_cloud": S1, "fp_backward_ragged_ms": round(med(rounds, 0), 3),
            "fp_backward_one_cloud_ms": round(med(rounds, 1), 3), "one_cloud_over_ragged": round(med(rounds, 1) / med(rounds, 0), 3),
            "rounds_ms_ragged_one_cloud": [[round(v, 3) for v in r] for r in rounds], "outputs_equal": bool(same)}


print(json.dumps({"steps": steps, "warmup": warmup, "train_step": train_step_leg(), "fp1_backward": fp1_backward_leg()}))
