"""rayca_hip_gather_device restated (helper module; test_gather_cpu.py, test_gpu_gather.py): the header's comment on RaycaGather in
numpy f32, operation by operation -- every + - * / rounds on its own.  The nine basis functions and the fold of per-ray radiance
into irradiance, coefficients and the kept count, and nothing else: the rays are tests/ambient_literal.py's (the two calls share
them), and the radiance along a ray is an input here (DeviceScene.radiance on the GPU, made-up values on the CPU)."""
import numpy as np

from ambient_literal import active, rays  # noqa: F401  (the rays of the specification: imported, not restated)

F0, F1, F3 = np.float32(0), np.float32(1), np.float32(3)
C0, C1, C2, C3, C4 = (np.float32(x) for x in (0.2820948, 0.4886025, 1.0925484, 0.3153916, 0.5462742))


def f32(x):
    return np.asarray(x, np.float32)


def basis(d):
    """Y_k(d), k = 0..8, of the directions d [..., 3]: [..., 9] f32"""
    d = f32(d)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        ys = [np.full(x.shape, C0, np.float32), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * ((F3 * (z * z)) - F1), C2 * (x * z),
              C4 * ((x * x) - (y * y))]
    return np.stack(ys, -1).astype(np.float32)


def counts(L):
    """a sample counts iff r, g and b are finite (x - x == 0 for each)"""
    L = f32(L)
    with np.errstate(all="ignore"):
        return ((L[..., :3] - L[..., :3]) == F0).all(-1)


def fold(L, act, d, samples, weights=None):
    """(irradiance [N, 4], sh [N, 9, 4], kept [N] u32, samples [N, S, 4]) from the per-ray radiance L [N, S, 4] (ignored for inactive
    points), the active flags [N], the traced directions d [N, S, 3] and the weights [S] of the samples (the table from dir_first
    on) or None.  j ascending; E = E + c, H[k] = H[k] + c * Y_k(d_j), then both divided by float(kept) where kept > 0."""
    L, d, act = f32(L), f32(d), np.asarray(act, bool)
    n = L.shape[0]
    E = np.zeros((n, 3), np.float32)
    H = np.zeros((n, 9, 3), np.float32)
    kept = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        for j in range(samples):
            take = counts(L[:, j]) & act
            c = L[:, j, :3]
            if weights is not None:
                c = f32(weights)[j] * c
            y = basis(d[:, j])
            E = np.where(take[:, None], E + c, E).astype(np.float32)
            H = np.where(take[:, None, None], H + c[:, None, :] * y[:, :, None], H).astype(np.float32)
            kept = kept + take.astype(np.uint32)
        some = kept > 0
        div = np.where(some, kept, 1).astype(np.float32)
        E = np.where(some[:, None], E / div[:, None], E).astype(np.float32)
        H = np.where(some[:, None, None], H / div[:, None, None], H).astype(np.float32)
        frac = kept.astype(np.float32) / np.float32(samples)
    irradiance = np.concatenate([E, frac[:, None]], 1).astype(np.float32)
    sh = np.concatenate([H, np.zeros((n, 9, 1), np.float32)], 2)
    out_samples = np.where(act[:, None, None], L, F0).astype(np.float32)
    return irradiance, sh, kept, out_samples
