"""The edge-avoiding a-trous filter of rayca_hip_denoise_device, restated literally in numpy float32 from its specification
(include/rayca_hip.h) -- not from the kernel.  Vectorised over pixels, a Python loop over the 25 taps in the stated
order (dy = -2..2 outer, dx = -2..2 inner); every operation is one float32 operation, in the association the specification
writes, so under the library's arithmetic contract (no contraction, no fast math) the kernels give the same bits.  The output
stage is restated for gamma == 1 only (powf belongs to the render kernels and is pinned against them on the GPU).

max() is maxNum, np.fmax: a NaN operand gives the other one."""
import numpy as np

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))


def quantize(c):
    """RGBA8::from(Color): c * 255, NaN -> 0, clamped to [0, 255], truncated"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(c, F) * F(255.0)
        v = np.where(v != v, F(0.0), v)
        v = np.where(v < F(0.0), F(0.0), v)
        v = np.where(v > F(255.0), F(255.0), v)
        return v.astype(np.uint8)


def _shifted(a, dy, dx, s):
    """(a[y + dy s, x + dx s] where that lies inside the image, else a zero; the mask of the pixels where it does)"""
    h, w = a.shape[:2]
    oy, ox = dy * s, dx * s
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def atrous_iteration(c, step, *, normal=None, point=None, id=None, sigma_color=4.0, sigma_plane=None, normal_power_log2=7):
    """One iteration on c (H, W, 4) float32; returns the new (H, W, 4), alpha as it was."""
    h, w = c.shape[:2]
    kc = F(1.0) / (F(sigma_color) * F(sigma_color)) if sigma_color > 0 else None
    kp = F(1.0) / (F(sigma_plane) * F(sigma_plane)) if point is not None else None
    total = np.zeros((h, w, 3), F)
    wsum = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(c, dy, dx, step)
                wt = np.full((h, w), K[abs(dx)] * K[abs(dy)], F)
                if kc is not None:
                    d = c[..., :3] - cq[..., :3]
                    dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wt = wt / (F(1.0) + dc * kc)
                if normal is not None:
                    nq, _ = _shifted(normal, dy, dx, step)
                    dn = np.fmax((normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2], F(0.0))
                    for _ in range(normal_power_log2):
                        dn = dn * dn
                    wt = wt * dn
                if point is not None:
                    xq, _ = _shifted(point, dy, dx, step)
                    e = xq - point
                    pd = (normal[..., 0] * e[..., 0] + normal[..., 1] * e[..., 1]) + normal[..., 2] * e[..., 2]
                    wt = wt / (F(1.0) + (pd * pd) * kp)
                take = inside & (wt > F(0.0))
                if id is not None:
                    idq, _ = _shifted(id, dy, dx, step)
                    take &= idq == id
                for ch in range(3):
                    total[..., ch] = np.where(take, total[..., ch] + wt * cq[..., ch], total[..., ch])
                wsum = np.where(take, wsum + wt, wsum)
        out = c.copy()
        ok = wsum > F(0.0)
        for ch in range(3):
            out[..., ch] = np.where(ok, total[..., ch] / wsum, c[..., ch])
    assert out.dtype == F
    return out


def denoise(color, *, albedo=None, normal=None, point=None, id=None, iterations=5, sigma_color=4.0, sigma_plane=None,
            normal_power_log2=7):
    """The whole call for gamma == 1: (rgba32f (H, W, 4) float32, rgba8 (H, W, 4) uint8)."""
    color = np.ascontiguousarray(color, F)
    assert color.ndim == 3 and color.shape[2] == 4 and 0 <= iterations <= 8 and 0 <= normal_power_log2 <= 10
    assert point is None or (normal is not None and sigma_plane is not None and sigma_plane > 0)
    c = color.copy()
    den = None
    with np.errstate(all="ignore"):
        if albedo is not None and iterations > 0:
            den = np.fmax(np.asarray(albedo, F)[..., :3], F(1e-3))
            c[..., :3] = c[..., :3] / den
        for i in range(iterations):
            c = atrous_iteration(c, 1 << i, normal=normal, point=point, id=id, sigma_color=sigma_color, sigma_plane=sigma_plane,
                                 normal_power_log2=normal_power_log2)
        if den is not None:
            c[..., :3] = c[..., :3] * den
    assert c.dtype == F
    return c, quantize(c)


def synthetic(width, height, seed, *, specials=False):
    """A fixed-seed frame with every guide: two planes that meet at a slanted line, with their own normals and ids, under the
    same light; a checker albedo of one-pixel cells; multiplicative noise.  Returns a dict: clean, color, albedo (H, W, 4),
    normal, point (H, W, 3) float32, id (H, W) uint32.  `specials` puts a NaN, a +inf, denormals and a zero normal at fixed
    pixels (where they fit).

    Why this frame: the filter has no variance estimate, so an iteration lowers the error only while the noise it removes
    outweighs the signal it smears.  Demodulated, each plane is flat, and with the guides nothing crosses the line between
    them: every iteration can only average noise away.  Without guides the filter at sigma_color 4 is nearly a plain B3 blur,
    which cannot keep a texture finer than its footprint; the one-pixel checker is the texture it loses completely in the
    first iteration (the B3 taps 1 4 6 4 1 put 8/16 on either parity), so that the smear is there from iteration 1 on and
    does not grow, and what the later iterations change is again the noise alone."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(F)
    side = (x + F(0.37) * y) > F(0.55) * F(width)
    normal = np.where(side[..., None], np.array([0.6, 0.0, 0.8], F), np.array([0.0, 0.0, 1.0], F)).astype(F)
    depth = np.where(side, F(0.75) * (x - F(0.55) * F(width)), F(0.0)).astype(F)
    point = np.stack([x * F(0.1), y * F(0.1), -depth * F(0.1)], -1).astype(F)
    ident = np.where(side, np.uint32(7), np.uint32(3)).astype(np.uint32)
    checker = ((x.astype(np.int64) + y.astype(np.int64)) % 2).astype(bool)
    albedo = np.ones((height, width, 4), F)
    albedo[..., :3] = np.where(checker[..., None], np.array([0.8, 0.7, 0.5], F), np.array([0.5, 0.6, 0.8], F))
    clean = albedo.copy()
    noise = rng.gamma(2.0, 0.5, size=(height, width, 3)).astype(F)   # mean 1, like a 1-spp estimate's spread
    color = clean.copy()
    color[..., :3] = clean[..., :3] * noise
    if specials:
        def at(py, px):
            return (py % height, px % width)
        color[at(2, 3)][0] = np.nan
        color[at(5, 17)][1] = np.inf
        color[at(7, 9)][:3] = np.array([1e-41, 3e-42, 0.0], F)
        color[at(11, 30)][:3] = F(1e-45)
        normal[at(4, 8)] = 0.0
        normal[at(9, 2)] = 0.0
    return dict(clean=clean, color=color, albedo=albedo, normal=normal, point=point, id=ident)
