"""Per-model matrix precision on the GPU: `precision=` on the modules, Trainer and the drivers, --precision / AMPNET_PRECISION on the
CLI files, over the library's per-thread scope (include/ampnet_hip.h: ampnet_precision_scope_begin / _end).

Everything here is an equality of bits: selecting a mode through a scope must run exactly the kernels that selecting it through the
process-wide switch runs, so outputs, losses, gradients, parameters and optimiser state are compared with torch.equal -- there is no
tolerance to choose.  Shapes are the suite's small ones: B = 2 samples x W = 3 windows x N = 256 points (the head on lo [2, 768, 64]),
the baseline PointNet at [4, 512, 9].  The scope stack itself (nesting, depth, errors, threads) is tested without a device in
tests/test_precision_api_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import PKG, sub                      # noqa: E402
from helpers import baseline_state                 # noqa: E402

pytestmark = pytest.mark.gpu

B, W, N = 2, 3, 256
MODES = ["f32x3", "bf16", "bf16_store"]


def _load(module, synth, seed, ptable, btable):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(seed, ptable).items()}
    sd.update({k: torch.from_numpy(v) for k, v in synth.make_buffers(seed, btable).items()})
    r = module.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and all(k.endswith("num_batches_tracked") for k in r.missing_keys)
    return module.train()


def _pair(synth, params, kind, precision):
    """(encoder, head) with the suite's seeded weights, freshly built: dropout step counters at 0, so equal runs draw equal masks."""
    M = sub("pointNet.model.pointnetAtt")
    enc = _load(M.BasePointNet(point_dimension=3, return_local_features=True, global_feat_dim=256, device="cuda", precision=precision),
                synth, 3, params.ENC_PARAMS, params.ENC_BUFFERS)
    if kind == "att":
        head = _load(M.SegmentationWithAttention(256, 8, num_classes=5, local_dim=64, dropout=0.3, device="cuda", precision=precision),
                     synth, 4, params.HEAD_PARAMS, params.HEAD_BUFFERS)
    else:
        head = _load(M.SegmentationWithGRU(num_classes=5, global_feat_size=256, hidden_size=64, device="cuda", precision=precision),
                     synth, 8, params.GRU_HEAD_PARAMS, params.HEAD_BUFFERS)
    return enc, head


@pytest.fixture(scope="module")
def batch(synth):
    """The B = 2 synthetic batch every test here shares (read-only): x [B, W, N, 9], targets [B, W*N] (-1 on padded windows),
    centroids [B, W, 2], the key-padding mask of the reference."""
    pc, tg, cent, _ = synth.sample_batch(812, B, N, max_w=W)
    x = torch.from_numpy(np.ascontiguousarray(pc.transpose(0, 3, 1, 2))).cuda()
    t = torch.from_numpy(np.ascontiguousarray(tg.transpose(0, 2, 1))).cuda()
    tpc = t.reshape(B, W * N)
    return dict(x=x, t=t, tpc=tpc, cent=torch.from_numpy(cent).cuda(), mask=sub("ops").pad_mask(tpc, W),
                cw=torch.tensor([1.0, 2.0, 2.0, 1.0, 1.0], device="cuda"))


def _forward(enc, head, kind, b):
    """The reference-style step through autograd: encoder, head, a torch loss on the logits plus a term on the feature transforms."""
    local, glob, feat_T = enc.forward_windows(b["x"].reshape(B * W, N, 9), n_slots=W)
    if kind == "att":
        logits, _, _ = head.forward_rows(glob, local, b["cent"], [N] * W, b["mask"])
    else:
        logits, _, _ = head.forward_rows(glob, local, [N] * W, B)
    loss = F.cross_entropy(logits, b["tpc"], weight=b["cw"], ignore_index=-1) + 1e-3 * feat_T.square().sum()
    return logits, loss


def _grads(*modules):
    return {f"{i}.{k}": p.grad.clone() for i, m in enumerate(modules) for k, p in m.named_parameters()}


def _step(enc, head, kind, b):
    logits, loss = _forward(enc, head, kind, b)
    loss.backward()
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), loss=loss.detach().clone(), **_grads(enc, head))


def _baseline_step(synth, precision):
    M = sub("pointNet.model.pointnet")
    net = M.SegmentationPointNet(num_classes=5, point_dimension=3, device="cuda", precision=precision)
    table = {k: tuple(v.shape) for k, v in net.state_dict().items() if "num_batches" not in k}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in baseline_state(synth, table, 9000).items()}, strict=False)
    net.train()
    x = torch.from_numpy(synth.windows(31, 4, 512)).cuda()
    tg = torch.from_numpy(synth.randint(32, (4, 512), 0, 5)).cuda().long()
    logits, feat_T = net(x)
    loss = F.cross_entropy(logits, tg) + 1e-3 * feat_T.square().sum()
    loss.backward()
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), loss=loss.detach().clone(), **_grads(net))


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: not bit-equal in {bad[:6]} ({len(bad)} of {len(a)} tensors)"
    assert all(torch.isfinite(v).all() for v in a.values()), what


def _run(synth, params, kind, precision, b):
    if kind == "baseline":
        return _baseline_step(synth, precision)
    return _step(*_pair(synth, params, kind, precision), kind, b)


# ---- 1. a mode chosen per model equals the same mode chosen through the process-wide switch ------------------------------------------
@pytest.mark.parametrize("kind", ["att", "gru", "baseline"])
@pytest.mark.parametrize("mode", MODES)
def test_scoped_equals_global(synth, params, batch, mode, kind):
    L = sub("_lib")
    try:
        L.set_matrix_precision("fp32")
        scoped = _run(synth, params, kind, mode, batch)                 # run A: default fp32, the models carry the mode
        assert L.get_matrix_precision() == "fp32" and L.effective_matrix_precision() == "fp32"
        plain = _run(synth, params, kind, None, batch) if mode != "f32x3" and kind != "baseline" else None
        L.set_matrix_precision(mode)
        switched = _run(synth, params, kind, None, batch)               # run B: the switch carries the mode, the models follow it
    finally:
        L.set_matrix_precision("fp32")
    _assert_same(scoped, switched, f"{kind} in {mode}: precision={mode!r} against set_matrix_precision({mode!r})")
    if plain is not None:                                               # and the scope did select something: bf16 operands are not fp32's
        assert not torch.equal(scoped["logits"], plain["logits"]), f"{kind}: precision={mode!r} gave the fp32 logits"


def test_scope_is_closed_when_a_call_raises(synth, params, batch):
    L = sub("_lib")
    try:
        enc, head = _pair(synth, params, "att", "bf16_store")
        with pytest.raises(L.AmpnetError, match="encoder_forward"):
            enc.forward_windows(torch.zeros(B * W * N, 5, device="cuda"), np_cluster=[N] * (B * W))       # 5 columns, not 9
        assert L.effective_matrix_precision() == L.get_matrix_precision() == "fp32"
        with torch.no_grad(), pytest.raises(L.AmpnetError, match="head_forward"):
            head.forward_rows(torch.zeros(B * W, 256, device="cuda"), torch.zeros(7, 64, device="cuda"), batch["cent"], [N] * W)
        assert L.effective_matrix_precision() == L.get_matrix_precision() == "fp32"
        _step(enc, head, "att", batch)                                  # and the models still run in their own mode afterwards
        assert L.effective_matrix_precision() == "fp32"
    finally:
        L.set_matrix_precision("fp32")


# ---- 2. two models of one process in different modes, their steps interleaved -------------------------------------------------------
@pytest.mark.parametrize("mode_p,mode_q", [("fp32", "bf16_store"), ("fp32", "f32x3")])
def test_interleaved_models_equal_each_alone(synth, params, batch, mode_p, mode_q):
    """forward P, forward Q, backward P, backward Q -- Q's tape is bf16 while P's is fp32 in the first pair, so a backward that ran in the
    other model's mode would be refused by the workspace tags (or silently use other kernels in the second pair)."""
    L = sub("_lib")
    try:
        L.set_matrix_precision("fp32")
        alone_p = _step(*_pair(synth, params, "att", mode_p), "att", batch)
        alone_q = _step(*_pair(synth, params, "att", mode_q), "att", batch)
        p, q = _pair(synth, params, "att", mode_p), _pair(synth, params, "att", mode_q)
        logits_p, loss_p = _forward(*p, "att", batch)
        logits_q, loss_q = _forward(*q, "att", batch)
        loss_p.backward()
        loss_q.backward()
        torch.cuda.synchronize()
        assert L.get_matrix_precision() == "fp32" and L.effective_matrix_precision() == "fp32"
    finally:
        L.set_matrix_precision("fp32")
    _assert_same(dict(logits=logits_p.detach(), loss=loss_p.detach(), **_grads(*p)), alone_p, f"P ({mode_p}) interleaved with Q ({mode_q})")
    _assert_same(dict(logits=logits_q.detach(), loss=loss_q.detach(), **_grads(*q)), alone_q, f"Q ({mode_q}) interleaved with P ({mode_p})")


# ---- 3. the mode a forward ran in is the mode of its backward ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32x3", "bf16_store"])
def test_backward_runs_in_the_recorded_mode(synth, params, batch, mode):
    """set_precision('fp32') between forward and backward: the gradients are those of the undisturbed step.  ('bf16_store' besides the
    'f32x3' case: there a backward in the attribute's new value would not only differ, it would be refused.)"""
    L = sub("_lib")
    try:
        L.set_matrix_precision("fp32")
        want = _step(*_pair(synth, params, "att", mode), "att", batch)
        enc, head = _pair(synth, params, "att", mode)
        logits, loss = _forward(enc, head, "att", batch)
        enc.set_precision("fp32")
        head.set_precision("fp32")
        loss.backward()
        torch.cuda.synchronize()
    finally:
        L.set_matrix_precision("fp32")
    _assert_same(dict(logits=logits.detach(), loss=loss.detach(), **_grads(enc, head)), want, f"{mode} forward, set_precision('fp32'), backward")


# ---- 4. Trainer(precision=...) ------------------------------------------------------------------------------------------------------
def _trainer_state(tr):
    out = {}
    for tag, m, opt in (("enc", tr.pointnet, tr.opt_p), ("att", tr.att_net, tr.opt_a)):
        for k, v in m.state_dict().items():
            out[f"{tag}.{k}"] = v.detach().clone()
        for k, p in m.named_parameters():
            st = opt.state[p]
            out[f"{tag}.{k}.exp_avg"], out[f"{tag}.{k}.exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
            out[f"{tag}.{k}.step"] = st["step"].clone().cuda()
    return out


def test_trainer_precision_equals_the_global_switch(synth, params, batch):
    T, L = sub("trainer"), sub("_lib")
    res = {}
    try:
        for how in ("scoped", "switched"):
            L.set_matrix_precision("fp32" if how == "scoped" else "f32x3")
            enc, att = _pair(synth, params, "att", None)
            tr = T.Trainer(enc, att, lr=1e-3, class_w=batch["cw"], precision="f32x3" if how == "scoped" else None)
            assert tr.precision == ("f32x3" if how == "scoped" else None)
            assert (enc.precision, att.precision) == (None, None)          # the trainer's precision is its own, not the modules'
            for _ in range(2):
                out = tr.step(batch["x"], batch["t"], batch["cent"])
            torch.cuda.synchronize()
            assert L.effective_matrix_precision() == L.get_matrix_precision()
            res[how] = dict(_trainer_state(tr), ce=out["ce"].clone(), reg=out["reg"].clone(), logits=out["logits"].clone())
    finally:
        L.set_matrix_precision("fp32")
    _assert_same(res["scoped"], res["switched"], "two steps of Trainer(precision='f32x3') against set_matrix_precision('f32x3')")


def test_trainer_refuses_bf16_store_on_one_side_only(synth, params, batch):
    T, L = sub("trainer"), sub("_lib")
    M = sub("pointNet.model.pointnetAtt")
    enc, _ = _pair(synth, params, "att", "bf16_store")
    att = _load(M.SegmentationWithAttention(256, 8, num_classes=5, local_dim=64, dropout=0.3, device="cuda", precision="fp32"),
                synth, 4, params.HEAD_PARAMS, params.HEAD_BUFFERS)
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    with pytest.raises(ValueError, match="bf16_store"):
        T.Trainer(enc, att)
    with pytest.raises(ValueError, match="bf16_store"):
        T.forward_backward(enc, att, batch["x"], batch["t"], batch["cent"], batch["cw"])
    with pytest.raises(ValueError, match="bf16_store"):
        T.fused_train_step(enc, att, T.FusedAdam(enc.parameters()), T.FusedAdam(att.parameters()), batch["x"], batch["t"], batch["cent"], batch["cw"])
    torch.cuda.synchronize()
    # before any launch: not even the BatchNorm counters or running statistics of the encoder moved
    assert all(torch.equal(v, before[k]) for k, v in enc.state_dict().items())
    assert L.effective_matrix_precision() == "fp32"
    T.Trainer(enc, att, precision="bf16_store").step(batch["x"], batch["t"], batch["cent"])       # one mode for both: runs
    torch.cuda.synchronize()
    assert (enc.precision, att.precision) == ("bf16_store", "fp32")     # and leaves the modules' own attributes alone


# ---- 5 / 6. the CLI files ----------------------------------------------------------------------------------------------------------
# A CLI run in a fresh process starts from unseeded generators (weight initialisation, shuffling, augmentation) and has no flag for a
# seed, so the child seeds python's, numpy's and torch's generators and then executes the CLI file as __main__ with its arguments.
_SEEDED_MAIN = ("import random, runpy, sys, numpy, torch; random.seed(0); numpy.random.seed(0); torch.manual_seed(0); "
                "sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')")


def _cli(rel, args, cwd, precision_env):
    env = {k: v for k, v in os.environ.items() if k != "AMPNET_PRECISION"}
    if precision_env is not None:
        env["AMPNET_PRECISION"] = precision_env
    os.makedirs(cwd, exist_ok=True)
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-c", _SEEDED_MAIN, os.path.join(ROOT, PKG, "pointNet", rel)] + args
    r = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"{rel} {' '.join(args)} -> exit {r.returncode}\n{r.stdout[-3000:]}"
    return r.stdout


@pytest.fixture(scope="module")
def cli_runs(synth, tmp_path_factory):
    """One epoch of the attention CLI on a tiny dataset (2 training files, 1 validation file, N = 256), twice: --precision f32x3, and
    AMPNET_PRECISION=f32x3 without the flag.  Each run has a working directory of its own (checkpoints are named by the minute)."""
    root = tmp_path_factory.mktemp("precision_cli")
    paths = synth.write_dataset(str(root), n_train=2, n_val=1, n_test=1, n_points=256, seed=930, max_w=3)
    args = [paths["data"], "--path_list_files", paths["lists"], "--out_path", str(root / "out"), "--number_of_points", "256",
            "--batch_size", "1", "--epochs", "1", "--number_of_workers", "0"]
    runs = {}
    for tag, extra, env in (("flag", ["--precision", "f32x3"], None), ("env", [], "f32x3")):
        cwd = str(root / tag)
        out = _cli("self-attention/train_pointnet-attention.py", args + extra, cwd, env)
        cks = sorted(os.listdir(os.path.join(cwd, "pointNet", "checkpoints")))
        assert len(cks) == 1, (tag, cks, out[-2000:])
        runs[tag] = dict(out=out, ck=os.path.join(cwd, "pointNet", "checkpoints", cks[0]))
    return dict(paths=paths, root=root, **runs)


def _flat(prefix, obj, out):
    if torch.is_tensor(obj):
        out[prefix] = obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _flat(f"{prefix}.{k}", v, out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _flat(f"{prefix}[{i}]", v, out)
    return out


def test_cli_training_flag_equals_environment(cli_runs):
    for tag in ("flag", "env"):
        assert "matrix precision: f32x3" in cli_runs[tag]["out"], cli_runs[tag]["out"][-2000:]
        assert cli_runs[tag]["out"].count("matrix precision:") == 1             # logged once
    a = _flat("ck", torch.load(cli_runs["flag"]["ck"], map_location="cpu", weights_only=True), {})
    b = _flat("ck", torch.load(cli_runs["env"]["ck"], map_location="cpu", weights_only=True), {})
    assert len(a) > 100 and a.keys() == b.keys()
    assert not any(k.endswith("precision") for k in a)                          # the checkpoint dict is the reference's, nothing added
    _assert_same(a, b, "checkpoint of --precision f32x3 against AMPNET_PRECISION=f32x3")


def test_cli_inference_equals_the_in_process_call(cli_runs, capsys):
    """The inference CLI with --precision f32x3 (a fresh child under its own timeout) prints the per-file and mean IoU that the in-process
    call test(..., precision='f32x3') prints, under a global fp32.  pointNet/amp_test.py and its CLI file keep the reference's signature
    and flags; the precision-taking driver and CLI are pointNet/amp_infer.py and self-attention/infer_pointnet_att_segmen.py."""
    paths, root, ck = cli_runs["paths"], cli_runs["root"], cli_runs["flag"]["ck"]
    L = sub("_lib")
    args = ["--dataset_path", paths["data"], "--number_of_points", "256", "--number_of_workers", "0", "--model_checkpoint", ck,
            "--path_list_files", paths["lists"], "--cluster_dir", paths["clusters"]]
    out = _cli("self-attention/infer_pointnet_att_segmen.py", args + ["--out_path", str(root / "res_cli"), "--precision", "f32x3"],
               str(root / "infer"), None)
    capsys.readouterr()
    try:
        res = sub("pointNet.amp_infer").test(paths["data"], str(root / "res_call"), 256, 0, ck, paths["lists"], cluster_dir=paths["clusters"],
                                             precision="f32x3")
        assert L.get_matrix_precision() == L.effective_matrix_precision() == "fp32"
    finally:
        L.set_matrix_precision("fp32")
    mine = capsys.readouterr().out
    iou_lines = lambda text: [l for l in text.splitlines() if l.startswith("[") or l.startswith("mean_iou:")]       # noqa: E731
    for text in (out, mine):
        assert text.count("matrix precision: f32x3") == 1 and text.count("matrix precision:") == 1
    assert len(iou_lines(mine)) == 2 and iou_lines(out) == iou_lines(mine), (iou_lines(out), iou_lines(mine))
    assert np.isfinite(res["accuracy"])


def test_inference_follows_the_environment_and_the_enclosing_scope(cli_runs, capsys, monkeypatch):
    """amp_infer.test without an argument reads AMPNET_PRECISION; amp_test.test itself, which takes none, follows the scope it is called
    in.  Both print what the run under set_matrix_precision('f32x3') prints."""
    paths, root, ck = cli_runs["paths"], cli_runs["root"], cli_runs["flag"]["ck"]
    L, A, I = sub("_lib"), sub("pointNet.amp_test"), sub("pointNet.amp_infer")
    iou_lines = lambda text: [l for l in text.splitlines() if l.startswith("[") or l.startswith("mean_iou:")]       # noqa: E731
    run = lambda fn, tag: fn(paths["data"], str(root / tag), 256, 0, ck, paths["lists"], cluster_dir=paths["clusters"])   # noqa: E731
    capsys.readouterr()
    try:
        monkeypatch.setenv("AMPNET_PRECISION", "f32x3")
        run(I.test, "res_env")
        out_env = capsys.readouterr().out
        monkeypatch.delenv("AMPNET_PRECISION")
        with L.precision_scope("f32x3"):
            run(A.test, "res_scoped")
        assert L.get_matrix_precision() == L.effective_matrix_precision() == "fp32"
        out_scoped = capsys.readouterr().out
        L.set_matrix_precision("f32x3")
        run(A.test, "res_switched")
        out_switched = capsys.readouterr().out
    finally:
        L.set_matrix_precision("fp32")
    assert "matrix precision: f32x3" in out_env
    assert len(iou_lines(out_switched)) == 2 and iou_lines(out_env) == iou_lines(out_scoped) == iou_lines(out_switched)


def test_head_forward_files_runs_in_the_heads_precision(synth, params):
    """The several-files eval head (amp_test.segment_files calls it with the head's tables, not the head): logits of a head built with
    precision='bf16' under a global fp32 are those of a plain head under set_matrix_precision('bf16'), and not the fp32 ones."""
    ops, L = sub("ops"), sub("_lib")
    n_files, Wf, n = 2, 3, 200
    sizes = [n, n + 37, n - 11, n + 5, 0, 0]                            # the second file holds one cluster: two zero-row slots, masked
    off, total, mx = ops.window_offsets(sizes, torch.device("cuda", torch.cuda.current_device()))
    gl = torch.from_numpy(synth.uniform(41, (n_files * Wf, 256), -1.0, 1.0)).cuda()
    lo = torch.from_numpy(synth.uniform(42, (total, 64), 0.0, 1.0)).cuda()
    cent = torch.from_numpy(synth.uniform(43, (n_files, Wf, 2), -1.0, 1.0)).cuda()
    mask = torch.tensor([[0, 0, 0], [0, 1, 1]], dtype=torch.uint8, device="cuda")

    def run(precision):
        _, head = _pair(synth, params, "att", precision)
        head.eval()
        pt, bt = head._tables()
        logits, preds = ops.head_forward_files(pt, bt, gl, lo, cent, off, mask, n_files, Wf, total, mx, 5, head._ws)
        torch.cuda.synchronize()
        return dict(logits=logits.clone(), preds=preds.clone())
    try:
        L.set_matrix_precision("fp32")
        scoped, plain = run("bf16"), run(None)
        assert L.effective_matrix_precision() == "fp32"
        L.set_matrix_precision("bf16")
        switched = run(None)
    finally:
        L.set_matrix_precision("fp32")
    _assert_same(scoped, switched, "head_forward_files: precision='bf16' against set_matrix_precision('bf16')")
    assert not torch.equal(scoped["logits"], plain["logits"])
