"""The host side of multi-scale grouping, without a GPU: the library exports the new entry points within ABI 17 and the header names
them, the workspace size answers on the host, and PointNetSetAbstractionMsg constructs on the CPU with the usual implementation's
state_dict keys and refuses what is outside its limits."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402

SYMBOLS = ("ampnet_ball_query_msg_f32", "ampnet_sa_msg_forward_workspace_bytes", "ampnet_sa_msg_forward_f32")


def test_library_exports_the_entry_points_within_abi_17():
    L = sub("_lib")
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s + "(" in header, s
    assert "#define AMPNET_SA_MSG_MAX_SCALES 4" in header and L.SA_MSG_MAX_SCALES == 4
    assert "added within ABI 17" in header
    assert lib.ampnet_abi_version() == L.ABI_VERSION == 18      # the entry points above arrived within ABI 17; the baseline probe made it 18


def test_workspace_size_answers_on_the_host():
    L = sub("_lib")
    for K in range(1, L.SA_MSG_MAX_SCALES + 1):
        assert L.sa_msg_forward_workspace_bytes(K) == K * L.SA_WORKSPACE_BYTES
    for K in (0, L.SA_MSG_MAX_SCALES + 1, -1):
        with pytest.raises(L.AmpnetError, match=f"K={K}"):
            L.sa_msg_forward_workspace_bytes(K)


def test_bad_arguments_are_errors_before_any_launch():
    """Every check runs on the host before any launch: host memory stands in for the device pointers, nothing is dereferenced."""
    L = sub("_lib")
    lib = L.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    outs = (ctypes.c_void_p * 5)(*[p.value] * 5)

    def query(K, radii, nsamples, n=64):
        return lib.ampnet_ball_query_msg_f32(p, 1, n, 3, p, 4, (ctypes.c_float * 5)(*radii), (ctypes.c_int * 5)(*nsamples), K, outs, None, None)

    for K, radii, nsamples, n, match in ((0, [0.1] * 5, [4] * 5, 64, "K=0"), (5, [0.1] * 5, [4] * 5, 64, "K=5"),
                                        (2, [0.1] * 5, [4, 0, 4, 4, 4], 64, "scale 1: nsample=0"),
                                        (3, [0.1] * 5, [4, 4, 65, 4, 4], 64, "scale 2: nsample=65"),
                                        (2, [0.1, -1.0, 0, 0, 0], [4] * 5, 64, "scale 1: radius"),
                                        (2, [0.1] * 5, [4] * 5, 12289, "n=12289")):
        with pytest.raises(L.AmpnetError, match=match):
            L.check(query(K, radii, nsamples, n), "ampnet_ball_query_msg_f32")
    assert lib.ampnet_ball_query_msg_f32(None, 1, 64, 3, p, 4, (ctypes.c_float * 5)(), (ctypes.c_int * 5)(), 1, outs, None, None) != 0

    def forward(K, nsamples, couts, Ls, D=9, ws_bytes=4 * L.SA_WORKSPACE_BYTES):
        n_layers = max(sum(Ls), 1)
        return lib.ampnet_sa_msg_forward_f32(p, 1, 64, 3, p, 4, outs, (ctypes.c_int * 5)(*nsamples), p, D,
                                             (ctypes.c_void_p * (6 * n_layers))(*[p.value] * (6 * n_layers)), (ctypes.c_int * n_layers)(*couts),
                                             (ctypes.c_float * n_layers)(*[1e-5] * n_layers), (ctypes.c_int * 5)(*Ls), K, p, p,
                                             ctypes.c_size_t(ws_bytes), None)

    for K, nsamples, couts, Ls, kw, match in ((0, [8] * 5, [32], [1] * 5, {}, "K=0"), (5, [8] * 5, [32] * 5, [1] * 5, {}, "K=5"),
                                             (2, [8] * 5, [32, 32], [1, 1, 0, 0, 0], {"ws_bytes": 2 * L.SA_WORKSPACE_BYTES - 1}, "workspace"),
                                             (2, [8] * 5, [32, 32, 48], [1, 2, 0, 0, 0], {}, "branch 1: layer 1 has cout=48"),
                                             (2, [8] * 5, [32] * 5, [1, 4, 0, 0, 0], {}, "branch 1: L=4 layers"),
                                             (2, [8, 65, 8, 8, 8], [32, 32], [1, 1, 0, 0, 0], {}, "branch 1: nsample=65"),
                                             (2, [8] * 5, [32, 32], [1, 1, 0, 0, 0], {"D": 318}, "321 exceeds 320")):
        with pytest.raises(L.AmpnetError, match=match):
            L.check(forward(K, nsamples, couts, Ls, **kw), "ampnet_sa_msg_forward_f32")


def test_the_block_constructs_on_the_cpu():
    M, L = sub("pointNet.model.pointnet2_utils"), sub("_lib")
    msg = M.PointNetSetAbstractionMsg(16, [0.1, 0.2], [16, 32], 6, [[32, 64], [32]], device="cpu")
    tail = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    assert list(msg.state_dict()) == ["conv_blocks.0.0.weight", "conv_blocks.0.0.bias", "conv_blocks.0.1.weight", "conv_blocks.0.1.bias",
                                      "conv_blocks.1.0.weight", "conv_blocks.1.0.bias"] \
        + [f"bn_blocks.0.0.{t}" for t in tail] + [f"bn_blocks.0.1.{t}" for t in tail] + [f"bn_blocks.1.0.{t}" for t in tail]
    assert tuple(msg.conv_blocks[0][0].weight.shape) == (32, 9, 1, 1) and tuple(msg.conv_blocks[1][0].weight.shape) == (32, 9, 1, 1)
    assert tuple(msg.conv_blocks[0][1].weight.shape) == (64, 32, 1, 1) and tuple(msg.bn_blocks[0][1].running_var.shape) == (64,)
    assert (msg.npoint, msg.radius_list, msg.nsample_list, msg.in_channel) == (16, [0.1, 0.2], [16, 32], 6)
    assert tuple(M.PointNetSetAbstractionMsg(16, [0.1], [16], 0, [[32]], device="cpu").conv_blocks[0][0].weight.shape) == (32, 3, 1, 1)
    for args in ((16, [0.1, 0.2], [16], 6, [[32], [32]]),                            # lists of different lengths
                 (16, [0.1, 0.2], [16, 32], 6, [[32]]),
                 (16, [], [], 6, []),                                                # K = 0
                 (16, [0.1] * 5, [16] * 5, 6, [[32]] * 5),                           # K = 5
                 (16, [0.1, 0.2], [16, 32], 6, [[32], [48]]),                        # a width that is no multiple of 32
                 (16, [0.1, 0.2], [16, 32], 6, [[32], [288]]),
                 (16, [0.1, 0.2], [16, 32], 6, [[32], [32, 32, 32, 32]]),            # four layers
                 (16, [0.1, 0.2], [16, 32], 6, [[32], []]),
                 (16, [0.1, 0.2], [16, 65], 6, [[32], [32]]),                        # nsample
                 (16, [0.1, 0.2], [16, 0], 6, [[32], [32]]),
                 (16, [0.1, 0.2], [16, 32], 318, [[32], [32]])):                     # in_channel + 3 = 321
        with pytest.raises(NotImplementedError, match=f"1..{L.SA_MSG_MAX_SCALES}.*multiples of 32.*{L.SA_MAX_CIN}.*nsample <= {L.SA_MAX_NSAMPLE}"):
            M.PointNetSetAbstractionMsg(*args, device="cpu")
