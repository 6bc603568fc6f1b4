"""What the fine-tuning tests of pointnet_2 share (tests/test_pointnet2_encoder_finetune_gpu.py): the reduced model, seeded state and input
of tests/test_pointnet2_finetune_gpu.py.  Test infrastructure."""
import numpy as np
import torch

from conftest import sub

B, N = 2, 512


def randomise(mod, seed):
    """Seeded values for every parameter and BatchNorm buffer (as tests/test_pointnet2_model_gpu.py does)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in mod.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var") or ("mlp_bns" in k and k.endswith("weight")):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * (0.6 if v.dim() == 1 else 2.0 / v.shape[1] ** 0.5)
    mod.load_state_dict(sd)


def model(state=None, **kwargs):
    """pointnet_2(5, **kwargs) in eval mode at reduced sizes (128 / 32 / 8 centres); seeded state, or `state`."""
    M = sub("pointNet.model.pointnetAtt")
    net = M.pointnet_2(5, **kwargs).eval()
    for sa, npoint, radius in ((net.sa1, 128, 0.2), (net.sa2, 32, 0.4), (net.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    if state is None:
        randomise(net, 8)
    else:
        net.load_state_dict(state)
    return net


def model_input(synth):
    x = np.concatenate([synth.clouds(55, B, N), synth.uniform(56, (B, N, 6), -1.0, 1.0)], -1)        # [B, N, 9]
    return torch.from_numpy(x).cuda().transpose(1, 2).contiguous()                                  # [B, 9, N]
