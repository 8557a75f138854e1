"""rayca_hip_ambient_device restated (helper module; test_ambient_cpu.py, test_gpu_ambient.py): the header's comment on
RaycaAmbient in numpy f32, operation by operation -- every + - * / rounds on its own, comparisons and selects, no square root, no
trigonometry.  The frame, ambient_ray and the fold of a mask into hits / open / bent, and nothing else: whether a ray is occluded
is an input here (the oracle's records on the CPU, DeviceScene.query(kind="occluded") on the GPU)."""
import numpy as np

F0, F1 = np.float32(0), np.float32(1)


def f32(x):
    return np.asarray(x, np.float32)


def frame(n):
    """(T, B) of the normals n [..., 3]: the branch-free basis of Duff et al. 2017, its sign taken by a comparison"""
    n = f32(n)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    with np.errstate(all="ignore"):
        sg = np.where(nz >= F0, F1, -F1).astype(np.float32)
        a = -F1 / (sg + nz)
        b = (nx * ny) * a
        t = np.stack([F1 + ((sg * nx) * nx) * a, sg * b, (-sg) * nx], -1)
        bt = np.stack([b, sg + (ny * ny) * a, -ny], -1)
    return t.astype(np.float32), bt.astype(np.float32)


def active(p, n):
    """the inactive rule: a zero normal (+0 or -0), or any of the six inputs not finite"""
    p, n = f32(p), f32(n)
    zero = (n[..., 0] == F0) & (n[..., 1] == F0) & (n[..., 2] == F0)
    return ~zero & np.isfinite(p).all(-1) & np.isfinite(n).all(-1)


def ambient_ray(p, n, rot, dirs, j, bias):
    """(o, d) of sample j (dirs[j]: the table from dir_first on) at the points p [N, 3] with normals n [N, 3]; rot [N, 2] = (c, s) or
    None: then rx = lx, ry = ly and no operation is performed"""
    p, n, dirs, bias = f32(p), f32(n), f32(dirs), np.float32(bias)
    t, b = frame(n)
    lx, ly, lz = dirs[j, 0], dirs[j, 1], dirs[j, 2]
    with np.errstate(all="ignore"):
        if rot is None:
            rx, ry = np.full(p.shape[:-1], lx, np.float32), np.full(p.shape[:-1], ly, np.float32)
        else:
            c, s = f32(rot)[..., 0], f32(rot)[..., 1]
            rx = c * lx - s * ly
            ry = s * lx + c * ly
        d = ((t * rx[..., None]) + (b * ry[..., None])) + n * lz
        o = p + n * bias
    return o.astype(np.float32), d.astype(np.float32)


def rays(p, n, rot, dirs, samples, bias, dir_first=0):
    """(o, d), each [N, S, 3]: every sample of every point (inactive points included: their rows are never traced)"""
    od = [ambient_ray(p, n, rot, f32(dirs)[dir_first:], j, bias) for j in range(samples)]
    return np.stack([o for o, _ in od], 1), np.stack([d for _, d in od], 1)


def fold(occluded, act, d, samples):
    """(mask u64, hits u32, open f32, bent [N, 3] f32) from per-ray occlusion [N, S] (ignored for inactive points), the active flags
    [N] and the directions [N, S, 3].  bent: acc = 0; for j ascending: if not occluded, acc = acc + d_j."""
    occ = np.asarray(occluded, bool) & np.asarray(act, bool)[:, None]
    n = occ.shape[0]
    mask = np.zeros(n, np.uint64)
    for j in range(samples):
        mask |= occ[:, j].astype(np.uint64) << np.uint64(j)
    hits = np.array([bin(int(m)).count("1") for m in mask], np.uint32).reshape(n)
    opened = (np.uint32(samples) - hits).astype(np.float32) / np.float32(samples)
    acc = np.zeros((n, 3), np.float32)
    with np.errstate(all="ignore"):
        for j in range(samples):
            acc = np.where((~occ[:, j] & act)[:, None], acc + f32(d)[:, j], acc).astype(np.float32)
    return mask, hits, opened.astype(np.float32), acc
