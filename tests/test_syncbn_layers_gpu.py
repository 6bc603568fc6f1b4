"""Layer-local float64 parity of the AMP-Net global-batch BatchNorm (ampnet_set_collective): csrc/sync_bn.hip (sync_pack_kernel,
sync_constants_kernel, sync_fc_apply_kernel) and the sync_bn_on() branches of bn_finalize (bn_finalize_kernel<true> rank merge -> all-gather ->
bn_finalize_gathered), bn_bwd_finalize, pool_bwd and fc_bn_bwd.  The rank programs and the cases are tests/syncbn_layers_worker.py.

ONE launch of two gloo ranks (both on cuda:0) serves the module.  Each rank runs every case twice through the layer probes on its own, uneven
share: with no collective, then under trainer.enable_sync_batchnorm() -- the production callback.  The test process rebuilds both ranks'
inputs and holds the outputs to the float64 restatement of the WHOLE batch (tests/bn_probe.py: finalize_global_ref,
bn_bwd_finalize_global_ref, fc_bn_bwd_global_ref; tests/test_pooled_bwd_gpu.py: pool_bwd_global_ref; themselves held to torch in
tests/test_bn_refs_cpu.py).  Bars: pw_probe.bar, derived -- one fp32 rounding per rank and packed quantity (K = 1), the all-reduce of two
fp32 terms (K = 2, mag = the sum of the ranks' magnitudes), carried through to the outputs; row counts are exact.  Per test:
  * the global outputs (statistics, P1 .. P3) are within their bars and bit-equal between the ranks;
  * the outputs that stay per-rank (slot_ab, dpm; g uses the global means but the rank's rows) are the rank's own, under the single-process bars;
  * for one case of each op, or more, the answers WITHOUT a collective miss the same comparison by more than 10 x: each comparison can fail;
  * shapes past the scratch segment, and a probe op without a global form, are refused on both ranks before any exchange.
The worst error / bar of every output family is printed at teardown.  After the rank programs' non-zero status nothing further is started.

A slot with no row on any rank: sync_constants_kernel divided the all-reduced sums by the all-reduced row count 0 (0 / 0: NaN in P2 and P3,
where the plain launch wrote 0); the `empty` case of bn_bwd_finalize found it and the kernel now has bn_bwd_constants<true>'s n > 0 guard.

Observed worst error / bar on the MI355X: bn_finalize scale 0.157, shift 0.086, mean / stat_mean 0.093, invstd 0.082, stat_uvar 0.083 (without a
collective the same comparisons miss by 2e5 or more); bn_bwd_finalize<64> P1 0.097, P2 0.057, P3 0.059, slot_ab 0.098, <16> P1 0.090, P2 / P3 0.004,
slot_ab 0.012 (without a collective P2 / P3 miss by 5.7e4 or more).
"""
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
import bn_probe as B                               # noqa: E402
import pw_probe as PP                              # noqa: E402
import syncbn_layers_worker as Wk                  # noqa: E402

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "syncbn_layers_worker.py")
WORST, PLAIN = {}, {}


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """Both ranks' outputs of every case: ONE launch for the module; a rank that fails fails the launcher and with it every test here."""
    out = tmp_path_factory.mktemp("syncbn_layers")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), WORKER, str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [torch.load(out / f"layers{k}.pt", weights_only=True) for k in range(2)]


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    for k in sorted(WORST):
        print(f"[syncbn layers] worst error/bar {k}: {WORST[k]:.4f}" + (f"   (without a collective: {PLAIN[k]:.3g})" if k in PLAIN else ""))


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    assert r <= 1.0, f"{family}: error at {r:.3f} of the bar"


def outputs(ranks, kind, name, tag):
    """[rank 0's, rank 1's] {output: float array} of a case's plain / sync run."""
    pre = f"{kind}/{name}/{tag}/"
    res = [{k[len(pre):]: v.numpy() for k, v in r.items() if k.startswith(pre)} for r in ranks]
    assert res[0] and sorted(res[0]) == sorted(res[1]), (kind, name, tag)
    return res


def same_bits(a, b, what):
    assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32)), f"{what}: the ranks' values differ"


def misses(family, got, want_bar):
    """the answer without a collective against the global restatement: error / bar, recorded (NaN where nothing finite was written: a miss)"""
    want, b = want_bar
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(want.shape) - want)
    r = float(np.max(np.where(np.isfinite(err), err, np.inf) / np.maximum(b, 1e-300)))
    PLAIN[family] = min(PLAIN.get(family, np.inf), r)
    return r


def names_of(kind):
    return [n for k, n in Wk.CASES if k == kind]


# ---- bn_finalize: rank merge -> all-gather -> gathered finalize ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", names_of("fin"))
def test_bn_finalize_two_ranks(ranks, name):
    ks = Wk.case_inputs("fin", name)
    S, C = ks[0]["S"], ks[0]["C"]
    part = [(np.nan_to_num(k["mean"]), np.nan_to_num(k["m2"]), k["rows"], k["slots"]) for k in ks]
    ref = B.finalize_global_ref(part, S, ks[0]["gamma"], ks[0]["beta"])
    got, plain = outputs(ranks, "fin", name, "sync"), outputs(ranks, "fin", name, "plain")
    for n in Wk.FIN_OUT:
        same_bits(got[0][n], got[1][n], n)
        note(f"bn_finalize {n}", B.worst(got[0][n].reshape(S, C), ref[n]))
    N = [B.finalize_ref(*p, S, ks[0]["gamma"], ks[0]["beta"])["N"][:, 0] for p in part]
    if name.startswith("rank0_only"):
        assert N[0][2] > 0 and N[1][2] == 0 and ref["N"][2, 0] == N[0][2]
    if name.startswith("empty"):                      # no row anywhere: finalize_ref's mean 0, variance 0
        assert N[0][1] == 0 and N[1][1] == 0
        assert np.all(got[0]["mean"].reshape(S, C)[1] == 0) and np.all(got[0]["stat_uvar"].reshape(S, C)[1] == 0)
        assert np.array_equal(got[0]["invstd"].reshape(S, C)[1], np.full(C, np.float32(1.0 / np.sqrt(B.BN_EPS))))
    for r in range(2):                                # without a collective: the rank's own statistics, far from the global ones
        own = B.finalize_ref(*part[r], S, ks[0]["gamma"], ks[0]["beta"])
        for n in Wk.FIN_OUT:
            note(f"bn_finalize {n} (no collective, own rows)", B.worst(plain[r][n].reshape(S, C), own[n]))
            assert misses(f"bn_finalize {n}", plain[r][n], ref[n]) > 10.0, (n, r)


# ---- bn_bwd_finalize -> sync_pack_kernel -> all-reduce -> sync_constants_kernel ---------------------------------------------------------------
def bwd_cpb(k):
    import test_bn_glue_gpu as G
    return G.bwd_cpb(k["S"], k["C"], k["Q"], k["part_Q"], k["chunks"])


@pytest.mark.parametrize("name", names_of("bwd"))
def test_bn_bwd_finalize_two_ranks(ranks, name):
    ks = Wk.case_inputs("bwd", name)
    S, C = ks[0]["S"], ks[0]["C"]
    assert all(bwd_cpb(k) == (16 if name.startswith("cpb16") else 64) for k in ks)
    ref = B.bn_bwd_finalize_global_ref([(k["part_a"], k["part_b"], k["slots"], k["slot_rows"]) for k in ks], ks[0]["gamma"], ks[0]["mean"],
                                       ks[0]["invstd"], S)
    got, plain = outputs(ranks, "bwd", name, "sync"), outputs(ranks, "bwd", name, "plain")
    if S > 1:                                         # sync_pack_kernel's per-slot window count differs between the slots on rank 1
        assert len({(ks[1]["Q"] - s + S - 1) // S for s in range(S)}) > 1
    fam = "bn_bwd_finalize" + ("<16>" if name.startswith("cpb16") else "")
    for n in ("P1", "P2", "P3"):
        same_bits(got[0][n], got[1][n], n)
        note(f"{fam} {n}", B.worst(got[0][n].reshape(S, C), ref[n]))
    for r in range(2):
        note(f"{fam} slot_ab", B.worst(got[r]["slot_ab"].reshape(S, C, 2), ref["slot_ab"][r]))          # the rank's own
        assert np.array_equal(got[r]["slot_ab"], plain[r]["slot_ab"])
        for n in ("P2", "P3"):
            assert misses(f"{fam} {n}", plain[r][n], ref[n]) > 10.0, (n, r)
    if name.startswith("rank0_only"):                 # the plain launch wrote 0 on the rank without rows; the global values replace it
        assert ks[1]["slot_rows"][2] == 0 and ks[0]["slot_rows"][2] > 0
        assert np.all(plain[1]["P2"].reshape(S, C)[2] == 0) and np.all(plain[1]["P3"].reshape(S, C)[2] == 0)
        assert np.all(got[1]["P2"].reshape(S, C)[2] != 0) and np.all(got[1]["P3"].reshape(S, C)[2] != 0)
    if name.startswith("empty"):                      # no row anywhere: P2 = P3 = 0, P1 finite
        assert ks[0]["slot_rows"][1] == 0 and ks[1]["slot_rows"][1] == 0
        for r in range(2):
            assert np.all(got[r]["P2"].reshape(S, C)[1] == 0) and np.all(got[r]["P3"].reshape(S, C)[1] == 0)
            assert np.all(np.isfinite(got[r]["P1"]))


# ---- fc_bn_bwd -> sync_fc_apply_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names_of("fc"))
def test_fc_bn_bwd_two_ranks(ranks, name):
    ks = Wk.case_inputs("fc", name)
    S, C, pers = ks[0]["n_slots"], ks[0]["C"], [k["per"] for k in ks]
    assert pers[0] != pers[1]
    ref = B.fc_bn_bwd_global_ref([k["da"] for k in ks], [k["z"] for k in ks], ks[0]["scale"], ks[0]["shift"], ks[0]["mean"], ks[0]["invstd"], S, pers)
    assert all(s.all() for s in ref["sure"])
    got, plain = outputs(ranks, "fc", name, "sync"), outputs(ranks, "fc", name, "plain")
    for r in range(2):
        note("fc_bn_bwd g", B.worst(got[r]["g"].reshape(S * pers[r], C), ref["g"][r]))
        note("fc_bn_bwd slot_ab", B.worst(got[r]["slot_ab"].reshape(S, C, 2), ref["slot_ab"][r]))       # the rank's own
        assert np.array_equal(got[r]["slot_ab"], plain[r]["slot_ab"])
        assert np.all(got[r]["slot_ab"].reshape(S, C, 2)[:, 0, :] == 0), "a column the ReLU kills everywhere: da is ignored"
        assert misses("fc_bn_bwd g", plain[r]["g"], ref["g"][r]) > 10.0, r


# ---- pool_bwd -> sync_pack_kernel -> all-reduce -> sync_constants_kernel -------------------------------------------------------------------
@pytest.mark.parametrize("name", names_of("pool"))
def test_pool_bwd_two_ranks(ranks, name):
    import test_pooled_bwd_gpu as PB
    hs = Wk.case_inputs("pool", name)
    S = hs[0]["S"]
    assert hs[0]["Q"] != hs[1]["Q"] and hs[0]["sm"] == int(name[2:])
    ref = PB.pool_bwd_global_ref(hs)
    got, plain = outputs(ranks, "pool", name, "sync"), outputs(ranks, "pool", name, "plain")
    for n in ("P1", "P2", "P3"):
        same_bits(got[0][n], got[1][n], n)
        note(f"pool_bwd {n}", B.worst(got[0][n], ref[n]))
    assert np.array_equal(got[0]["P1"], hs[0]["scale"]), "P1 is the forward's scale itself"
    for r, (h, pr) in enumerate(zip(hs, ref["ranks"])):
        K = h["Q"] // S                               # the rank's own outputs under the bars of tests/test_pooled_bwd_gpu.py (check_pool_bwd)
        assert np.array_equal(got[r]["dpm"].astype(np.float64), pr["dpm"]), "dpm differs from the masked pooled gradient"
        note("pool_bwd slot_ab", max(PP.ratio(got[r]["slot_ab"][..., 0], pr["A"], pr["Am"], K), PP.ratio(got[r]["slot_ab"][..., 1], pr["Bs"], pr["Bm"], K)))
        assert np.array_equal(got[r]["slot_ab"], plain[r]["slot_ab"]) and np.array_equal(got[r]["dpm"], plain[r]["dpm"])
        for n in ("P2", "P3"):
            assert misses(f"pool_bwd {n}", plain[r][n], ref[n]) > 10.0, (n, r)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_under_a_collective_return_on_both_ranks(ranks):
    for r in ranks:
        rc, msg = r["refusal/bwd"]
        assert rc == B.AMPNET_E_ARG and "33 slots x 256 channels exceed the scratch segment" in msg, (rc, msg)
        rc, msg = r["refusal/fin"]
        assert rc == B.AMPNET_E_ARG and "sync BatchNorm: segment of" in msg, (rc, msg)
        rc, msg = r["refusal/pw_input"]
        assert rc == B.AMPNET_E_ARG and "a collective is installed" in msg, (rc, msg)
    assert ranks[0]["refusal/bwd"] == ranks[1]["refusal/bwd"] and ranks[0]["refusal/fin"] == ranks[1]["refusal/fin"]
