"""What the binding tests of the PointNet++ wrappers share (tests/test_pn2_bindings_cpu.py, tests/test_pn2_bindings_gpu.py): one valid
keyword call per `*_f32` wrapper of _lib at a tiny shape, and which of its arguments are tensors.  Test infrastructure."""
import torch

B, N, S, NSAMPLE, D, LD = 2, 40, 4, 8, 3, 3
D1, D2, S_COARSE, K = 3, 5, 4, 3
COUTS = [32, 64]
EPS = [1e-5, 1e-5]

# per wrapper: its tensor arguments, in the order of its signature (the first one is the first a check can name)
TENSOR_ARGS = {
    "sa_forward": ("xyz", "centres", "group_idx", "feats", "out"),
    "sa_backward": ("xyz", "centres", "group_idx", "feats", "dout", "dfeats", "arg_out"),
    "sa_all_forward": ("xyz", "feats", "out", "arg_out"),
    "sa_all_backward": ("xyz", "feats", "arg", "dout", "dfeats"),
    "sa_train_forward": ("xyz", "centres", "group_idx", "feats", "out", "save_mean", "save_invstd"),
    "sa_train_backward": ("xyz", "centres", "group_idx", "feats", "save_mean", "save_invstd", "dout", "dfeats", "arg_out"),
    "fp_forward": ("points1", "points2", "idx", "dist2", "out"),
    "fp_backward": ("points1", "points2", "idx", "dist2", "dout", "dpoints1", "dpoints2"),
    "fp_train_forward": ("points1", "points2", "idx", "dist2", "out", "save_mean", "save_invstd"),
    "fp_train_backward": ("points1", "points2", "idx", "dist2", "save_mean", "save_invstd", "dout", "dpoints1", "dpoints2"),
}
WRAPPERS = tuple(TENSOR_ARGS)
OPTIONAL = ("feats", "dfeats", "arg_out", "points1", "dpoints1")          # None is a legal value of these


def required(name):
    return [a for a in TENSOR_ARGS[name] if a not in OPTIONAL]


def _layers(cin, device, n):
    """Per layer weight [cout, cin], conv bias, BatchNorm weight, bias, running_mean, running_var (the first n of them), seeded."""
    g = torch.Generator().manual_seed(11)
    out = []
    for cout in COUTS:
        w = (torch.rand((cout, cin), generator=g) - 0.5) * (2.0 / cin ** 0.5)
        vec = [(torch.rand(cout, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=g), (torch.rand(cout, generator=g) - 0.5) * 0.6,
               (torch.rand(cout, generator=g) - 0.5) * 0.6, 0.5 + torch.rand(cout, generator=g)]
        out.append(tuple(t.to(device) for t in [w] + vec)[:n])
        cin = cout
    return out


def valid_args(L, name, device):
    """Keyword arguments of one valid call of L.<name>_f32 on `device`: every tensor contiguous, of the right dtype, rank and shape, the
    indices in range, the workspace of the size the library asks for."""
    g = torch.Generator().manual_seed(5)
    f32 = lambda *shape: torch.rand(shape, generator=g).to(device)
    i32 = lambda hi, *shape: torch.randint(0, hi, shape, generator=g, dtype=torch.int32).to(device)
    ws = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=device)
    grads = lambda layers: [tuple(torch.zeros_like(t) for t in layer[:4]) for layer in layers]
    train, backward = "_train_" in name, name.endswith("backward")
    sum_c, last = sum(COUTS), COUTS[-1]
    a = {}
    if name.startswith("fp"):
        layers = _layers(D1 + D2, device, 4 if train and backward else 6)
        a.update(points1=f32(B, N, D1), points2=f32(B, S_COARSE, D2), idx=i32(S_COARSE, B, N, K), dist2=f32(B, N, K), layers=layers, eps=EPS)
        dims, rows = (D1, D2, B, N), (B, N, last)
    elif name.startswith("sa_all"):
        layers = _layers(3 + D, device, 6)
        a.update(xyz=f32(B, N, LD), feats=f32(B, N, D), layers=layers, eps=EPS)
        dims, rows = (D, B, N), (B, last)
    else:
        layers = _layers(3 + D, device, 4 if train and backward else 6)
        a.update(xyz=f32(B, N, LD), centres=i32(N, B, S), group_idx=i32(N, B, S, NSAMPLE), feats=f32(B, N, D), layers=layers, eps=EPS)
        dims, rows = (D, B, S, NSAMPLE), (B, S, last)
    if train:
        a.update(save_mean=torch.zeros(sum_c, device=device), save_invstd=torch.ones(sum_c, device=device))
    if name == "sa_all_backward":
        a["arg"] = i32(N, *rows)
    if backward:
        a.update(dout=f32(*rows), grads=grads(layers))
        if name.startswith("fp"):
            a.update(dpoints1=torch.zeros_like(a["points1"]), dpoints2=torch.zeros_like(a["points2"]))
        else:
            a["dfeats"] = torch.zeros_like(a["feats"])
    else:
        a["out"] = torch.zeros(rows, device=device)
        if train:
            a["momentum"] = 0.1
    if name in ("sa_backward", "sa_train_backward", "sa_all_forward"):
        a["arg_out"] = torch.zeros(rows, dtype=torch.int32, device=device)
    if name == "sa_forward":
        a["workspace"] = ws(L.SA_WORKSPACE_BYTES)
    elif name == "fp_forward":
        a["workspace"] = ws(L.FP_WORKSPACE_BYTES)
    else:
        a["workspace"] = ws(getattr(L, name + "_workspace_bytes")(*dims, COUTS))
    return a


def call(L, name, args):
    return getattr(L, name + "_f32")(**args)
