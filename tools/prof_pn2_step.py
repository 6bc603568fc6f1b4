"""The pointnet_2_seg train step and its loss kernel against the way both had to be written before they existed.
python3 tools/prof_pn2_step.py [steps] [warmup]  -- HIP events around `steps` calls after `warmup` calls, the two sides of every comparison in
ALTERNATING rounds in this one process, the median round reported and every round listed; prints one JSON line.

(a) pointnet2_utils.seg_nll_loss (forward with predictions and counts, then backward to a leaf log_probs; ampnet_seg_nll_forward_f32 and
    ampnet_seg_nll_backward_f32) against the torch composition on the SAME tensors: F.nll_loss(weight, ignore_index=-1) + argmax +
    utils.get_metrics.confusion_device, and torch.autograd's backward of the loss.  M = 16 * 2048 and 576 * 2048 rows, C = 5, 20 % of the
    targets -1.  Under rocprofv3 (a kernel trace in a run of its own) the kernels to look for are seg_nll_forward_kernel,
    seg_nll_finalize_kernel and seg_nll_backward_kernel.
(b) pn2_step.train_loop on a resident batch of 4 samples holding 16 real windows of 2048 points (36 with the padding) against the same step
    written with what the package offered before: the same device augmentation, the real windows picked by a boolean mask of the targets
    (which waits for the GPU), model(xyz) on [Q, 9, N] (a transpose in, the [Q, 128, N] copy out and its backward mirror), F.nll_loss,
    argmax, confusion_device, the same FusedAdam.  Both sides start from the same state and draw the same augmentation."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
PKG = "3d-semantic-segmentation-amp-net_amd"
sub = lambda name: importlib.import_module(PKG + "." + name)
synth, U, A, S, T = sub("synthetic"), sub("pointNet.model.pointnet2_utils"), sub("pointNet.model.pointnetAtt"), sub("pointNet.pn2_step"), sub("trainer")
AS, P = sub("pointNet.amp_step"), sub("pointNet.pn2_train")
confusion_device = sub("utils.get_metrics").confusion_device
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ROUNDS, C, N = 5, 5, 2048
assert torch.cuda.is_available(), "tools/prof_pn2_step.py measures on the GPU"
dev = torch.device("cuda")
cw = torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device=dev)


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


def loss_leg(M):
    logp = torch.log_softmax(torch.from_numpy(synth.uniform(410, (M, C), -4.0, 4.0)).to(dev), dim=1).requires_grad_(True)
    target = torch.from_numpy(synth.randint(411, (M,), 0, C)).to(dev)
    target[torch.from_numpy(synth.uniform01(412, (M,)) < 0.2).to(dev)] = -1
    out = {}

    def fused():
        logp.grad = None
        loss, preds, counts = U.seg_nll_loss(logp, target, cw, want_preds=True, want_counts=True)
        loss.backward()
        out["fused"] = (loss.detach(), preds, counts, logp.grad)

    def composed():
        logp.grad = None
        loss = F.nll_loss(logp, target, cw, ignore_index=-1)
        preds = logp.detach().argmax(-1)
        counts = confusion_device(preds, target, C)
        loss.backward()
        out["torch"] = (loss.detach(), preds, counts, logp.grad)

    n = steps * 20                                                    # (tens of microseconds a call: time enough of them)
    rounds = [(timed(fused, n), timed(composed, n)) for _ in range(ROUNDS)]
    fused()
    composed()
    f, t = out["fused"], out["torch"]
    return {"rows": M, "calls_per_timing": n, "seg_nll_loss_fwd_bwd_ms": round(med(rounds, 0), 4), "torch_composition_fwd_bwd_ms": round(med(rounds, 1), 4),
            "torch_over_fused": round(med(rounds, 1) / med(rounds, 0), 2), "rounds_ms_fused_torch": [[round(v, 4) for v in r] for r in rounds],
            "algorithmic_bytes": M * C * 4 * 2 + M * 8 * 3, "loss_abs_diff": float((f[0] - t[0]).abs()), "preds_differ": int((f[1] != t[1]).sum()),
            "counts_equal": bool(torch.equal(f[2], t[2])), "grad_max_rel_diff": float((f[3] - t[3]).abs().max() / t[3].abs().max())}


def step_leg():
    w_real = [5, 3, 6, 2]                                             # 16 real windows of 4 * 9
    pc, tg, _, _ = synth.sample_batch(420, 4, N, max_w=9, w_real=w_real)
    pc, tg = torch.from_numpy(pc).to(dev), torch.from_numpy(tg).to(dev)
    torch.manual_seed(0)
    new, old = A.pointnet_2_seg(C, **P.TRAIN_FLAGS), A.pointnet_2_seg(C, **P.TRAIN_FLAGS)
    old.load_state_dict(new.state_dict())
    opt_new, opt_old = T.FusedAdam(new.parameters(), lr=1e-3), T.FusedAdam(old.parameters(), lr=1e-3)
    data = (pc, tg, None, None, w_real)
    last = {}

    def step_new():
        m, _, _, counts = S.train_loop(data, opt_new, cw, new, train=True)
        last["new"] = (m["loss"], counts)

    def step_old():
        old.train()
        x, t = AS.augment_batch_device(pc, tg, True, dev)
        keep = (t.view(-1, N) != -1).any(dim=1)
        rows, tgt = x.view(-1, N, 9)[keep], t.view(-1, N)[keep]       # (a data-dependent shape: the host waits for the GPU here)
        opt_old.zero_grad()
        log_probs, _ = old(rows.transpose(1, 2).contiguous())
        loss = F.nll_loss(log_probs.reshape(-1, C), tgt.reshape(-1), cw, ignore_index=-1)
        preds = log_probs.detach().argmax(-1)
        counts = confusion_device(preds, tgt, C)
        loss.backward()
        opt_old.step()
        last["old"] = (loss.detach(), counts)

    np.random.seed(1)
    step_new()
    np.random.seed(1)
    step_old()
    first = {"loss_new": float(last["new"][0]), "loss_old": float(last["old"][0]), "counts_equal": bool(torch.equal(last["new"][1], last["old"][1]))}
    peak = {}
    for name, fn in (("new", step_new), ("old", step_old)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = round(torch.cuda.max_memory_allocated() / 1e6, 1)
    rounds = [(timed(step_new), timed(step_old)) for _ in range(ROUNDS)]
    return {"windows": sum(w_real), "points": N, "steps_per_timing": steps, "train_loop_ms": round(med(rounds, 0), 3), "parent_way_step_ms": round(med(rounds, 1), 3),
            "parent_over_train_loop": round(med(rounds, 1) / med(rounds, 0), 3), "rounds_ms_new_old": [[round(v, 3) for v in r] for r in rounds],
            "peak_allocated_MB_train_loop": peak["new"], "peak_allocated_MB_parent_way": peak["old"], "first_step": first}


print(json.dumps({"steps": steps, "warmup": warmup, "loss": [loss_leg(16 * N), loss_leg(576 * N)], "step": step_leg()}))
