"""numpy restatement of the ragged input pipeline, written from the text of include/ampnet_hip.h (ampnet_cloud_input_f32): the keyed point
shuffle, the padding rule, the label table and the z-rotation.  No GPU, no library: the arbiter of tests/test_cloud_input_gpu.py."""
import numpy as np

_U32 = np.uint32


def mix32(x):
    """The dropout hash on a uint32 array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> _U32(16)
        x *= _U32(0x7feb352d)
        x ^= x >> _U32(15)
        x *= _U32(0x846ca68b)
        x ^= x >> _U32(16)
    return x


def _mix1(x):
    return int(mix32(np.array([x & 0xFFFFFFFF], dtype=np.uint32))[0])


def step_base(seed, step):
    return _mix1(seed + step * 0x9E3779B9)


def cloud_key(seed, step, cloud):
    return _mix1(step_base(seed, step) + cloud * 0x85EBCA6B)


def step_angle(seed, step):
    return 2.0 * np.pi * _mix1(step_base(seed, step) ^ 0x3C6EF372) / 4294967296.0


def feistel(ck, n, x):
    """One application of the four-round network on the domain of 2^(2 half) values; x uint32 array."""
    bits = max(int(n - 1).bit_length(), 1)
    half = (bits + 1) // 2
    mask = _U32((1 << half) - 1)
    L, R = x >> _U32(half), x & mask
    for r in range(4):
        L, R = R, L ^ (mix32(_U32(ck) ^ ((R << _U32(2)) | _U32(r))) & mask)
    return (L << _U32(half)) | R


def perm(seed, step, cloud, n, return_rounds=False):
    """perm_b as an int64 array [n]: position j holds the cloud's row perm_b(j)."""
    ck = cloud_key(seed, step, cloud)
    y = feistel(ck, n, np.arange(n, dtype=np.uint32))
    rounds = 1
    while True:
        out = y >= n
        if not out.any():
            break
        y[out] = feistel(ck, n, y[out])
        rounds += 1
        assert rounds <= 4 * n + 4, "the walk must end: the network is a bijection of at most 4 n values"
    y = y.astype(np.int64)
    return (y, rounds) if return_rounds else y


def labels(codes):
    """float class codes -> int64 labels: (long)code clamped to 0 .. 255, then 15 -> 1, 14 -> 2, 3 / 4 -> 3, 5 -> 4, else 0."""
    k = np.clip(np.trunc(np.asarray(codes, dtype=np.float64)), 0, 255).astype(np.int64)
    lut = np.zeros(256, dtype=np.int64)
    lut[15], lut[14], lut[3], lut[4], lut[5] = 1, 2, 3, 3, 4
    return lut[k]


def rotate_z(xyz, angle):
    """utils.rotate_point_cloud_z restated: the float64 product with [[c, s, 0], [-s, c, 0], [0, 0, 1]], rounded to float32."""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
    return np.dot(np.asarray(xyz, dtype=np.float32).reshape(-1, 3), rot).astype(np.float32)


def cloud_input(raw, sizes, npoint, seed, step, permute, rotate):
    """raw [sum n, 10] float32, sizes -> (rows [sum p, 9] f32, targets [sum p] i64, src [sum p] i32, padded sizes), p = max(n, npoint)."""
    raw = np.asarray(raw, dtype=np.float32)
    padded = [max(int(n), int(npoint)) for n in sizes]
    src, own, r0 = [], [], 0
    for b, (n, p) in enumerate(zip(sizes, padded)):
        j = np.arange(p, dtype=np.int64)
        pb = perm(seed, step, b, n) if permute else np.arange(n, dtype=np.int64)
        src.append(r0 + pb[j % n])
        own.append(j < n)
        r0 += n
    src, own = np.concatenate(src), np.concatenate(own)
    rows = raw[src, :9].copy()
    if rotate:
        rows[:, :3] = rotate_z(rows[:, :3], step_angle(seed, step))
    targets = np.where(own, labels(raw[src, 9]), -1).astype(np.int64)
    return rows, targets, src.astype(np.int32), padded
