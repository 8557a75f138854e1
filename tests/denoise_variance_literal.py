"""The variance-guided a-trous filter of rayca_hip_denoise_variance_device, restated literally in numpy float32 from its
specification (include/rayca_hip.h) -- not from the kernel.  Vectorised over pixels, Python loops over the taps in
the stated orders; every operation is one float32 operation, in the association the specification writes, so under the
library's arithmetic contract (no contraction, no fast math) the kernels give the same bits.  As in denoise_literal the output
stage is restated for gamma == 1 only.

max() is maxNum, np.fmax: a NaN operand gives the other one.  A comparison with a NaN is False."""
import numpy as np

from denoise_literal import F, K, _shifted, quantize

G3 = (F(0.5), F(0.25))   # the 3 x 3 prefilter is the outer product of (0.25, 0.5, 0.25): 0.25 centre, 0.125 edge, 0.0625 corner


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _guide_terms(wt, dy, dx, step, normal, point, kp, normal_power_log2):
    """the normal and the point term of the tap (dy, dx) at `step`, in that order, as rayca_hip_denoise_device writes them"""
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
    return wt


def initial_variance(c, variance, *, ld=None, length=None, min_history=0, normal=None, point=None, id=None, sigma_plane=None,
                     normal_power_log2=7):
    """v0 (H, W) float32 from the (demodulated) image c, the accumulation's variance and, where given, lum(den) and the length"""
    h, w = c.shape[:2]
    kp = F(1.0) / (F(sigma_plane) * F(sigma_plane)) if point is not None else None
    with np.errstate(all="ignore"):
        v = np.fmax(np.asarray(variance, F), F(0.0))
        if ld is not None:
            v = v / (ld * ld)
        if length is not None:
            length = np.asarray(length, F)
            v = v / np.fmax(length, F(1.0))
        if min_history > 0:
            s1, s2, ws = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    cq, inside = _shifted(c, dy, dx, 1)
                    wt = _guide_terms(np.full((h, w), F(1.0), F), dy, dx, 1, normal, point, kp, normal_power_log2)
                    lq = lum(cq)
                    take = inside & (wt > F(0.0)) & ((lq - lq) == F(0.0))
                    if id is not None:
                        idq, _ = _shifted(id, dy, dx, 1)
                        take &= idq == id
                    s1 = np.where(take, s1 + wt * lq, s1)
                    s2 = np.where(take, s2 + wt * (lq * lq), s2)
                    ws = np.where(take, ws + wt, ws)
            m1, m2 = s1 / ws, s2 / ws
            spatial = np.where(ws > F(0.0), np.fmax(m2 - m1 * m1, F(0.0)), F(0.0))
            v = np.where(length < F(min_history), spatial, v)
    assert v.dtype == F
    return v


def iteration(c, v, step, *, normal=None, point=None, id=None, sigma_luminance=4.0, sigma_plane=None, variance_floor=1e-10,
              normal_power_log2=7):
    """One iteration on c (H, W, 4) and v (H, W) float32; returns the new pair, alpha as it was."""
    h, w = c.shape[:2]
    kp = F(1.0) / (F(sigma_plane) * F(sigma_plane)) if point is not None else None
    sl2 = F(sigma_luminance) * F(sigma_luminance)
    with np.errstate(all="ignore"):
        gs, gw = np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vq, inside = _shifted(v, dy, dx, 1)
                g = G3[abs(dx)] * G3[abs(dy)]
                gs = np.where(inside, gs + g * vq, gs)
                gw = np.where(inside, gw + g, gw)
        dnm = sl2 * (gs / gw) + F(variance_floor)
        lp = lum(c)
        total = np.zeros((h, w, 3), F)
        vs, ws = np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(c, dy, dx, step)
                vq, _ = _shifted(v, dy, dx, step)
                wt = np.full((h, w), K[abs(dx)] * K[abs(dy)], F)
                d = lp - lum(cq)
                wt = wt / (F(1.0) + (d * d) / dnm)
                wt = _guide_terms(wt, dy, dx, step, normal, point, kp, normal_power_log2)
                take = inside & (wt > F(0.0))
                if id is not None:
                    idq, _ = _shifted(id, dy, dx, step)
                    take &= idq == id
                for ch in range(3):
                    total[..., ch] = np.where(take, total[..., ch] + wt * cq[..., ch], total[..., ch])
                vs = np.where(take, vs + (wt * wt) * vq, vs)
                ws = np.where(take, ws + wt, ws)
        out = c.copy()
        ok = ws > F(0.0)
        for ch in range(3):
            out[..., ch] = np.where(ok, total[..., ch] / ws, c[..., ch])
        vout = np.where(ok, vs / (ws * ws), v)
    assert out.dtype == F and vout.dtype == F
    return out, vout


def denoise_variance(color, variance, *, length=None, min_history=4, sigma_luminance=4.0, variance_floor=1e-10, albedo=None, normal=None,
                     point=None, id=None, iterations=5, sigma_plane=None, normal_power_log2=7):
    """The whole call for gamma == 1: (rgba32f (H, W, 4) float32, rgba8 (H, W, 4) uint8, variance_out (H, W) float32).
    As DeviceScene.denoise_variance, min_history applies only where a length is given."""
    color = np.ascontiguousarray(color, F)
    assert color.ndim == 3 and color.shape[2] == 4 and 1 <= iterations <= 8 and 0 <= normal_power_log2 <= 10
    assert point is None or (normal is not None and sigma_plane is not None and sigma_plane > 0)
    assert sigma_luminance > 0 and variance_floor > 0
    c = color.copy()
    den = ld = None
    guides = dict(normal=normal, point=point, id=id, sigma_plane=sigma_plane, normal_power_log2=normal_power_log2)
    with np.errstate(all="ignore"):
        if albedo is not None:
            den = np.fmax(np.asarray(albedo, F)[..., :3], F(1e-3))
            c[..., :3] = c[..., :3] / den
            ld = lum(den)
        v = initial_variance(c, variance, ld=ld, length=length, min_history=min_history if length is not None else 0, **guides)
        for i in range(iterations):
            c, v = iteration(c, v, 1 << i, sigma_luminance=sigma_luminance, variance_floor=variance_floor, **guides)
        if den is not None:
            c[..., :3] = c[..., :3] * den
    assert c.dtype == F and v.dtype == F
    return c, quantize(c), v


def film_like(width, height, seed, samples, *, cell=6):
    """A fixed-seed frame as a film holds one after `samples` frames, with every guide of denoise_literal.synthetic: the mean of
    `samples` gamma-noise samples of a clean frame whose lighting is a checker of `cell`-pixel cells that no guide shows; the
    top half noisy (gamma(2, 0.5): relative spread 0.71), the bottom half calm (a tenth of that spread).  Returns synthetic()'s
    dict plus variance and length (H, W) float32: the variance of the luminance over the samples, as the accumulation's
    moments give it (max(m2 - m1^2, 0)), and the sample count."""
    from denoise_literal import synthetic
    s = synthetic(width, height, seed)
    rng = np.random.default_rng(seed + 1)
    y, x = np.mgrid[0:height, 0:width]
    light = np.where(((x // cell) + (y // cell)) % 2 == 0, F(1.0), F(0.45)).astype(F)
    clean = s["albedo"].copy()
    clean[..., :3] = s["albedo"][..., :3] * light[..., None]
    noise = rng.gamma(2.0, 0.5, size=(samples, height, width, 3))
    calm = 1.0 + 0.1 * (noise - 1.0)
    noise = np.where((y < height // 2)[None, :, :, None], noise, calm)
    frames = clean[None, ..., :3].astype(np.float64) * noise
    l = 0.2126 * frames[..., 0] + 0.7152 * frames[..., 1] + 0.0722 * frames[..., 2]
    m1, m2 = l.mean(0), (l * l).mean(0)
    color = clean.copy()
    color[..., :3] = frames.mean(0).astype(F)
    s.update(clean=clean, color=color, variance=np.maximum(m2 - m1 * m1, 0.0).astype(F), length=np.full((height, width), F(samples), F))
    return s
