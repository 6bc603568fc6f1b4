"""CPU restatements of the PointNet++ grouping kernels, written from the spec in include/ampnet_hip.h (ampnet_ball_query_f32,
ampnet_sa_forward_f32): float32 for the query, float64 for the MLP.  Test infrastructure: no GPU, no library."""
import numpy as np

EPS32 = 2.0 ** -24


def sq_dists(xyz, c):
    """float32 ((dx*dx + dy*dy) + dz*dz) from point c to every point, one rounding per operation."""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=np.float32)
    d = p[c] - p
    sq = d * d
    return (sq[:, 0] + sq[:, 1]) + sq[:, 2]


def ball_query(xyz, centres, radius, nsample):
    """xyz [n, >=3] float32, centres [s] point indices -> (idx int32 [s, nsample], count int32 [s]).
    d(j) = float32 ((dx*dx + dy*dy) + dz*dz), one rounding per operation; member when d(j) <= float32(radius * radius); the first
    nsample members in ascending index order, the remaining slots repeat the first member; count = min(members, nsample)."""
    r = np.float32(radius)
    r2 = np.float32(r * r)
    idx = np.empty((len(centres), nsample), np.int32)
    cnt = np.empty(len(centres), np.int32)
    for i, c in enumerate(np.asarray(centres)):
        dist = sq_dists(xyz, c)
        assert dist.dtype == np.float32
        members = np.nonzero(dist <= r2)[0][:nsample]
        cnt[i] = len(members)
        idx[i, :len(members)] = members
        idx[i, len(members):] = members[0]
    return idx, cnt


def make_layers(seed, cin, widths, negative_gamma=False):
    """Seeded parameters of a shared MLP: per layer (weight [cout, cin], bias, gamma, beta, running_mean, running_var), float32."""
    rng = np.random.default_rng(seed)
    layers = []
    for cout in widths:
        k = 1.0 / np.sqrt(cin)
        gamma = rng.uniform(0.5, 1.5, cout)
        if negative_gamma:
            gamma = gamma * np.where(rng.random(cout) < 0.5, -1.0, 1.0)
        layers.append(tuple(a.astype(np.float32) for a in (
            rng.uniform(-k, k, (cout, cin)), rng.uniform(-k, k, cout), gamma, rng.uniform(-0.5, 0.5, cout),
            rng.uniform(-0.3, 0.3, cout), rng.uniform(0.5, 1.5, cout))))
        cin = cout
    return layers


def mlp_chain(a, b_in, layers, eps):
    """The shared MLP of the fused forwards on rows a [..., cin_0] (float64) that carry the error bound b_in: per layer
    a <- relu(bn_eval(W a + b)), bn_eval(v) = (v - mean) / sqrt(var + eps) * gamma + beta, in float64 -> (a, b_in) of the last layer.

    The float32 error bound of tests/pw_probe.py::bar pushed through the chain, per element.  With e = 2^-24:
      * a layer with input a (bound b_in), product z = W a of length K:  |W| b_in  +  8 e sqrt(K) (|W| |a|)  +  2 e |z|   (pw_probe.bar);
      * the folded BatchNorm y = fma(z, scale, shift), scale = gamma / sqrt(var + eps), shift = (b - mean) scale + beta, multiplies that by
        |scale| and adds its own roundings: scale carries <= 2 e (sum, sqrt, quotient, each half an ulp), b - mean one, the product and
        sum of shift one each, the final fma one -- in all <= 3 e |z scale| + 6 e |(b - mean) scale| + 2 e |beta|, bounded here by
        6 e (|z scale| + |(b - mean) scale| + |beta|);
      * ReLU is 1-Lipschitz: the bound of relu(y) is that of y."""
    for (w, b, gamma, beta, mean, var), e in zip(layers, eps):
        w, b, gamma, beta, mean, var = (np.asarray(v, dtype=np.float64) for v in (w, b, gamma, beta, mean, var))
        K = w.shape[1]
        z = a @ w.T
        mag = np.abs(a) @ np.abs(w).T
        scale = gamma / np.sqrt(var + np.float64(np.float32(e)))
        y = (z + b - mean) * scale + beta
        bz = b_in @ np.abs(w).T + 8.0 * EPS32 * np.sqrt(K) * mag + 2.0 * EPS32 * np.abs(z)
        b_in = np.abs(scale) * bz + 6.0 * EPS32 * (np.abs(z * scale) + np.abs((b - mean) * scale) + np.abs(beta))
        a = np.maximum(y, 0.0)
    return a, b_in


def sa_forward(xyz, centres, group_idx, feats, layers, eps):
    """One cloud.  xyz [n, >=3] float32, centres [s], group_idx [s, nsample], feats [n, D] float32 or None, layers as make_layers, eps per
    layer -> (out float64 [s, cout_last], bar float64 [s, cout_last]).

    out: float64 evaluation of  max_t relu(bn_eval(W row_t + b))  over the layers, row_t = [xyz[idx_t] - xyz[centre], feats[idx_t]] formed
    exactly from the float32 inputs, bn_eval(v) = (v - mean) / sqrt(var + eps) * gamma + beta.

    bar: the float32 error bound per output element.  With e = 2^-24:
      * input: the kernel rounds the three coordinate differences once, |err| <= e |dx|; the features are exact;
      * the layers: mlp_chain;
      * max is 1-Lipschitz: the bound of the max is the largest row bound of the group."""
    p = np.asarray(xyz, dtype=np.float64)[:, :3]
    rows = p[group_idx] - p[np.asarray(centres)][:, None, :]                             # [s, nsample, 3], exact in float64
    b_in = EPS32 * np.abs(rows)
    if feats is not None:
        f = np.asarray(feats, dtype=np.float64)[group_idx]
        rows = np.concatenate([rows, f], -1)
        b_in = np.concatenate([b_in, np.zeros_like(f)], -1)
    a, b_in = mlp_chain(rows, b_in, layers, eps)
    return a.max(1), b_in.max(1)
