"""Data-parallel pointnet_2_seg with global-batch BatchNorm (csrc/bn_train.hip's two finalize launchers under a registered collective,
pn2_step's data-parallel train pass, pn2_train's launch from the environment).  The rank programs are tests/pn2_dp_worker.py.

  layers    two gloo ranks, each on its share of a case of the existing layer tables, through the existing train entry points: outputs and
            input gradients (concatenated over the ranks), parameter gradients (SUMMED over the ranks in float32, as the gradient
            all-reduce does) and statistics against the float64 layer restatements under THEIR bars; the saved and running statistics
            bit-equal between the ranks.
  one rank  nccl, world 1, AMPNET_FORCE_COLLECTIVES=1: every exchange is the identity and the step with global-batch BatchNorm equals
            the plain step bit for bit.
  step      457 | 711 rows: two steps against pn2_ragged_ref.run on the WHOLE batch under its bars; with per-rank statistics the same
            comparison fails by more than 10 x.
  driver    train_pn2_clouds under two ranks.
After a rank program's non-zero status nothing further is started."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_dp_worker as Wk                         # noqa: E402

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "pn2_dp_worker.py")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(mode, out_dir, arg=0, **env):
    """Two gloo ranks on cuda:0; a rank that fails fails the launcher, and the assert ends the test before anything else starts."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), WORKER, mode, str(out_dir), str(int(arg))]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def _run_one_rank(out_dir, arg):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AMPNET_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, WORKER, "onerank", str(out_dir), str(int(arg))], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---- layers ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layer_ranks(tmp_path_factory):
    """Both ranks' outputs of every LAYERS entry: ONE launch for the module."""
    out = tmp_path_factory.mktemp("pn2dp_layers")
    _run_ranks("layers", out)
    return [torch.load(out / f"layers{r}.pt", weights_only=True) for r in range(2)]


def _merged(kind, name, ranks):
    """{output name: numpy array} of the two-rank call as the single process would hold it; asserts the ranks' statistics bit-equal."""
    pre = f"{kind}/{name}/"
    r0, r1 = ({k[len(pre):]: v for k, v in r.items() if k.startswith(pre)} for r in ranks)           # ("refusal" has no such prefix)
    assert r0 and sorted(r0) == sorted(r1)
    got = {}
    for k in r0:
        if k in Wk.PER_RANK[kind]:
            got[k] = torch.cat([r0[k], r1[k]]).numpy()
        elif k.rstrip("0123456789") in Wk.SAME:
            assert torch.equal(r0[k], r1[k]), (kind, name, k)         # every rank wrote the same statistics, bit for bit
            got[k] = r0[k].numpy()
        else:
            got[k] = (r0[k] + r1[k]).numpy()                          # a parameter gradient: the all-reduce's float32 sum
    return got


def _within_bars(kind, name, got, want, names):
    ratios = {}
    for k in names:
        v, bar = want[k]
        assert got[k].shape == v.shape, (kind, name, k)
        err = np.abs(got[k].astype(np.float64) - v)
        ratios[k] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())     # (0 / 0: an exact value met exactly)
    print(f"two ranks, {kind}_train {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (kind, name, k, r)


@pytest.mark.parametrize("name", [n for k, n, _ in Wk.LAYERS if k == "fp"])
def test_fp_train_two_ranks_meet_the_layer_bars(layer_ranks, name):
    import fp_train_ref as R
    i = Wk.layer_inputs("fp", name)
    got = _merged("fp", name, layer_ranks)
    want, _ = R.fp_train(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
    assert sorted(got) == sorted(want)
    _within_bars("fp", name, got, want, R.output_names(len(i["layers"]), i["points1"] is not None))
    for l in range(len(i["layers"])):
        assert (got[f"dbias{l}"] == 0).all()


@pytest.mark.parametrize("name", [n for k, n, _ in Wk.LAYERS if k == "sa"])
def test_sa_train_two_ranks_meet_the_layer_bars(layer_ranks, name):
    import sa_train_ref as R
    i = Wk.layer_inputs("sa", name)
    got = _merged("sa", name, layer_ranks)
    tape, _ = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    R.check_argmax(got["arg"], tape[-1], i["group_idx"])
    want = R.sa_train(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], got["arg"], tape)
    assert sorted(got) == sorted(list(want) + ["arg"])
    _within_bars("sa", name, got, want, R.output_names(len(i["layers"]), i["feats"] is not None))


@pytest.mark.parametrize("name", [n for k, n, _ in Wk.LAYERS if k == "head"])
def test_seg_head_train_two_ranks_uneven_rows_meet_the_layer_bars(layer_ranks, name):
    import seg_head_train_ref as R
    i = Wk.layer_inputs("head", name)
    first = next(f for k, n, f in Wk.LAYERS if k == "head" and n == name)
    assert i["p"] == 0.0 and first % 32 and (i["x"].shape[0] - first) % 32 and 2 * first != i["x"].shape[0]
    got = _merged("head", name, layer_ranks)
    want, _ = R.seg_train(i["x"], i["params"], i["eps"], i["p"], i["drop_seed"], i["dlogp"])
    _within_bars("head", name, got, want, R.FORWARD + R.BACKWARD)
    assert (got["db1"] == 0).all()


def test_rows_times_world_size_beyond_the_float_limit_are_refused(layer_ranks):
    """2^23 + 1 rows are within the limit for one process and beyond it for two ranks (the conservative M * world_size rule)."""
    assert sub("_lib").fp_train_forward_workspace_bytes(16, 32, 1, (1 << 23) + 1, [32]) > 0
    for r in layer_ranks:
        assert "8388609 rows x 2 ranks exceed 16777216" in r["refusal"] and "conservative" in r["refusal"], r["refusal"]


# ---- one rank --------------------------------------------------------------------------------------------------------------------------
def test_one_rank_with_global_batch_batchnorm_equals_the_plain_step_bit_for_bit(tmp_path):
    plain = Wk.one_step()                                            # no process group in this process: the plain path
    _run_one_rank(tmp_path, 1)
    got = torch.load(tmp_path / "onerank1.pt", weights_only=True)
    assert sorted(got) == sorted(plain)
    for k, v in plain.items():
        assert torch.equal(got[k], v), f"{k}: the one-rank step with global-batch BatchNorm differs from the plain step"
    moved = [k for k in plain if k.startswith("param/")]
    assert moved and any(k.startswith("grad/") and bool((v != 0).any()) for k, v in plain.items())


# ---- the whole step ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _whole_batch_reference():
    """pn2_ragged_ref.run in float64 on the WHOLE batch with the keep mask the two ranks drew: rank r's dropout_mask over its own rows from
    its own head seed (HEAD_SEED + r), concatenated."""
    import pn2_model_ref as R
    import pn2_ragged_ref as G
    import test_pn2_ragged_train_gpu as RT
    inputs, _, idx = RT._case()
    _, target = Wk.step_clouds()
    rows = (sum(G.SIZES[:Wk.SPLIT]), sum(G.SIZES[Wk.SPLIT:]))
    assert rows == (457, 711)
    plain_mask = R.dropout_mask

    def ranks_mask(seed, step, total, dtype):
        assert total == sum(rows)
        return torch.cat([plain_mask((seed + r) & 0xFFFFFFFF, step, n, dtype) for r, n in enumerate(rows)])

    R.dropout_mask = ranks_mask
    try:
        return G.run(R.random_state(RT.SEED), dict(inputs, target=target), idx, "T", torch.float64)
    finally:
        R.dropout_mask = plain_mask


def _step_ratios(got, ref):
    """{kind: error / bar} of one step of rank 0 (loss, averaged gradients, running statistics) against the restatement's."""
    import pn2_model_ref as R
    import pn2_ragged_ref as G
    assert got["counts"] == ref["counts"]
    ref = dict(ref, out=dict(loss=ref["out"]["loss"]))              # (the step does not return log_probs)
    err = R.errors(dict(out=dict(loss=got["loss"]), grads=got["grads"], taps={}, buffers=got["buffers"]), ref, "T")
    rat = G.ratios(err, "T")
    for k, bar in G.BARS["T"].items():
        assert R.GPU_FACTOR * bar <= R.CAP, k
    return rat


def test_two_rank_step_equals_the_whole_batch_restatement(tmp_path):
    import pn2_model_ref as R
    ref = _whole_batch_reference()
    worst = {}
    _run_ranks("step", tmp_path)                                     # both variants in ONE launch
    for sync in (1, 0):
        r0, r1 = (torch.load(tmp_path / f"step{sync}_{r}.pt", weights_only=True) for r in range(2))
        rat = {}
        for step in range(2):
            for k, v in _step_ratios(r0[f"step{step}"], ref[step]).items():
                rat[k] = max(rat.get(k, 0.0), v)
        print(f"two ranks (457 | 711 rows), sync={sync}: " + R.summary(rat))
        worst[sync] = max(rat.values())
        for k in r0["state"]:
            assert torch.equal(r0["state"][k], r1["state"][k]) == bool(sync or "running" not in k), (sync, k)
        if sync:
            assert worst[1] <= 1.0, max(rat, key=rat.get)
            assert torch.equal(r0["step1"]["loss"], r1["step1"]["loss"])       # the global loss, on every rank
    print(f"worst error / bar: {worst[1]:.3g} with global-batch BatchNorm, {worst[0]:.3g} with per-rank statistics")
    assert worst[0] > 1.0 and worst[0] > 10.0 * worst[1]


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
def test_train_pn2_clouds_under_two_ranks(tmp_path):
    A = sub("pointNet.model.pointnetAtt")
    sub("synthetic").write_cluster_dataset(str(tmp_path), n_train=4, n_val=2, n_test=1, seed=930)
    _run_ranks("driver", tmp_path, AMPNET_SYNC_BN="1")
    r0, r1 = (torch.load(tmp_path / f"driver{r}.pt", weights_only=True) for r in range(2))         # both ranks finished
    for split in ("train_files", "val_files"):
        assert r0[split] and len(r0[split]) == len(r1[split]) and not set(r0[split]) & set(r1[split]), split
    assert len(r0["train_files"]) == 2 and len(r0["val_files"]) == 1
    assert r0["val_loss"] == r1["val_loss"] and np.isfinite(r0["val_loss"]) and np.isfinite(r0["train_loss"])
    cks = sorted(os.listdir(tmp_path / "rank0" / "pointNet" / "checkpoints"))
    assert len(cks) == 1 and not (tmp_path / "rank1" / "pointNet").exists()                          # one checkpoint, rank 0's
    ck = torch.load(tmp_path / "rank0" / "pointNet" / "checkpoints" / cks[0], map_location="cuda", weights_only=True)
    A.pointnet_2_seg(5).load_state_dict(ck["model"])
