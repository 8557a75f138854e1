"""The guided upsampling of rayca_hip_upsample_device, restated literally in numpy float32 from its specification
(include/rayca_hip.h) -- not from the kernel.  Vectorised over pixels, a Python loop over the four taps in the stated
order (j = 0, 1 outer, i = 0, 1 inner), as tests/temporal_literal.py is; every operation is one float32 operation, in the
association the specification writes, so under the library's arithmetic contract (no contraction, no fast math) the kernel gives
the same bits.  The output stage is restated for gamma == 1 only (powf belongs to the render kernels; the GPU tests pin the
gamma of this pass against the denoiser's output stage).

max() is maxNum (np.fmax); every comparison is one a NaN fails.

Guides travel as two dicts, `low` and `high`, with the keys albedo (.., 4), normal, point (.., 3) float32 and id (..) uint32."""
import numpy as np

from denoise_literal import quantize

F = np.float32
GUIDES = ("albedo", "normal", "point", "id")


def footprint(scale, width, height):
    """(x0, tx, y0, ty) of every output pixel, as the specification writes them: int64 and float32 arrays (H, W)"""
    y, x = np.mgrid[0:height, 0:width]
    s = F(scale)
    fx = (x.astype(F) + F(0.5)) / s - F(0.5)
    fy = (y.astype(F) + F(0.5)) / s - F(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0f, fy - y0f
    assert tx.dtype == F and ty.dtype == F
    return x0f.astype(np.int64), tx, y0f.astype(np.int64), ty


def demodulated(color, albedo_low):
    c = np.array(color, F)
    if albedo_low is not None:
        c[..., :3] = c[..., :3] / np.fmax(np.asarray(albedo_low, F)[..., :3], F(1e-3))
    return c


def upsample(color, scale, *, low=None, high=None, sigma_plane=None, normal_power_log2=7):
    """The whole call for gamma == 1: (rgba32f (H, W, 4) float32, rgba8 (H, W, 4) uint8, weight (H, W) float32)."""
    color = np.ascontiguousarray(color, F)
    low, high = dict(low or {}), dict(high or {})
    assert color.ndim == 3 and color.shape[2] == 4 and 1 <= scale <= 8 and 0 <= normal_power_log2 <= 10
    assert set(low) == set(high) and set(low) <= set(GUIDES)
    assert "point" not in low or ("normal" in low and sigma_plane is not None and sigma_plane > 0)
    h, w = color.shape[:2]
    hgt, wid = h * scale, w * scale
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        d = color - color
        finite = (d[..., 0] == zero) & (d[..., 1] == zero) & (d[..., 2] == zero) & (d[..., 3] == zero)
        c = demodulated(color, low.get("albedo"))
        x0, tx, y0, ty = footprint(scale, wid, hgt)
        kp = one / (F(sigma_plane) * F(sigma_plane)) if "point" in low else None
        if "normal" in low:
            n_p = np.asarray(high["normal"], F)
            n0, n1, n2 = n_p[..., 0], n_p[..., 1], n_p[..., 2]
            miss = (n0 == zero) & (n1 == zero) & (n2 == zero)
        wsum, bsum = np.zeros((hgt, wid), F), np.zeros((hgt, wid), F)
        total, totalb = np.zeros((hgt, wid, 4), F), np.zeros((hgt, wid, 4), F)
        for j in (0, 1):
            for i in (0, 1):
                qy, qx = y0 + j, x0 + i
                exists = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                b = (tx if i else one - tx) * (ty if j else one - ty)
                exists &= b > zero
                exists &= finite[qy, qx]
                cq = c[qy, qx]
                # the fallback's pass: w = b alone
                bsum = np.where(exists, bsum + b, bsum)
                for k in range(4):
                    totalb[..., k] = np.where(exists, totalb[..., k] + b * cq[..., k], totalb[..., k])
                # the guided pass
                wt = b
                take = exists.copy()
                if "normal" in low:
                    nq = np.asarray(low["normal"], F)[qy, qx]
                    miss_q = (nq[..., 0] == zero) & (nq[..., 1] == zero) & (nq[..., 2] == zero)
                    dn = np.fmax((n0 * nq[..., 0] + n1 * nq[..., 1]) + n2 * nq[..., 2], zero)
                    for _ in range(normal_power_log2):
                        dn = dn * dn
                    guided = b * dn
                    if "point" in low:
                        e = np.asarray(low["point"], F)[qy, qx] - np.asarray(high["point"], F)
                        pd = (n0 * e[..., 0] + n1 * e[..., 1]) + n2 * e[..., 2]
                        guided = guided / (one + (pd * pd) * kp)
                    wt = np.where(miss, b, guided)
                    take &= np.where(miss, miss_q, True)
                if "id" in low:
                    take &= np.asarray(low["id"])[qy, qx] == np.asarray(high["id"])
                take &= wt > zero
                wsum = np.where(take, wsum + wt, wsum)
                for k in range(4):
                    total[..., k] = np.where(take, total[..., k] + wt * cq[..., k], total[..., k])
        yy, xx = np.mgrid[0:hgt, 0:wid]
        nearest = c[np.minimum(yy // scale, h - 1), np.minimum(xx // scale, w - 1)]
        guided_ok, plain_ok = wsum > zero, bsum > zero
        o = np.where(guided_ok[..., None], total / wsum[..., None], np.where(plain_ok[..., None], totalb / bsum[..., None], nearest))
        if "albedo" in high:
            o[..., :3] = o[..., :3] * np.fmax(np.asarray(high["albedo"], F)[..., :3], F(1e-3))
    assert o.dtype == F and wsum.dtype == F
    return o, quantize(o), wsum


def bilinear(color, scale):
    """An independent plain bilinear resampler of the same footprint, written another way: the low image padded by one pixel of
    zeros, separable weight vectors, and a weight of zero where the literal skips a tap (outside the image, not finite), so
    that every output is a four-term weighted sum over a dense gather.  Adding w * c with w == 0 and a finite c changes no bit
    of a sum that started at +0, and the terms enter in the literal's order, so the association is the literal's and the
    comparison is bit for bit.  Where no weight is left the nearest low pixel is returned."""
    color = np.ascontiguousarray(color, F)
    h, w = color.shape[:2]
    hgt, wid = h * scale, w * scale
    s = F(scale)
    with np.errstate(all="ignore"):
        ok = np.isfinite(color).all(-1)
        padded = np.zeros((h + 2, w + 2, 4), F)
        padded[1:-1, 1:-1] = np.where(ok[..., None], color, F(0.0))
        valid = np.zeros((h + 2, w + 2), F)
        valid[1:-1, 1:-1] = ok
        fx = (np.arange(wid, dtype=F) + F(0.5)) / s - F(0.5)
        fy = (np.arange(hgt, dtype=F) + F(0.5)) / s - F(0.5)
        ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        ax, ay = fx - np.floor(fx), fy - np.floor(fy)
        wx = np.stack([F(1.0) - ax, ax])          # (2, W)
        wy = np.stack([F(1.0) - ay, ay])          # (2, H)
        acc, norm = np.zeros((hgt, wid, 4), F), np.zeros((hgt, wid), F)
        for j in (0, 1):
            rows = iy + 1 + j
            for i in (0, 1):
                cols = ix + 1 + i
                wgt = (wx[i][None, :] * wy[j][:, None]) * valid[rows[:, None], cols[None, :]]
                acc = acc + wgt[..., None] * padded[rows[:, None], cols[None, :]]
                norm = norm + wgt
        near = color[(np.arange(hgt) // scale)[:, None], (np.arange(wid) // scale)[None, :]]
        out = np.where((norm > 0)[..., None], acc / norm[..., None], near)
    assert out.dtype == F
    return out


# ---- one analytic scene at a pair of resolutions -----------------------------------------------------------------------------------
# Everything is a function of the position in FULL-size pixel units (X, Y), evaluated at each resolution's own pixel centres:
# X = (x + 0.5) * (full width / this width).  Two planes meet at a slanted line (a normal and a depth edge); rows above SKY_ROWS
# are misses; a thin feature one full-size pixel wide, with its own normal and id, lies where no low pixel centre falls.
ID_LEFT, ID_RIGHT, ID_THIN = np.uint32(3), np.uint32(7), np.uint32(11)
N_LEFT, N_RIGHT, N_THIN = (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 1.0, 0.0)   # the thin feature's normal is orthogonal to both planes'
SKY = (0.1, 0.12, 0.2, 1.0)
NAN_PIXELS = ((4, 5), (9, 12), (10, 2))   # (y, x) of the low image, modulo its size: a NaN, a +inf, a NaN


def scene_constants(full_width, full_height, scale):
    """where the edge, the sky and the thin feature lie for a size: the feature's column is chosen so that no low pixel centre
    (k + 0.5) * scale falls into [column, column + 1)"""
    column = int(0.27 * full_width)
    while scale > 1 and any(column <= (k + 0.5) * scale < column + 1 for k in range(full_width // scale)):
        column += 1
    return dict(edge=0.56 * full_width, slant=0.13, sky=0.18 * full_height, column=column, rows=(0.45 * full_height, 0.8 * full_height))


def edge_x(k, Y):
    return k["edge"] + k["slant"] * Y


def view(width, height, full_width, full_height, scale):
    """The G-buffer, the irradiance and the clean frame of the scene at width x height: a dict albedo, clean (H, W, 4), normal,
    point (H, W, 3) float32, id (H, W) uint32, and thin (H, W) bool.  A miss has a zero normal, point and id and albedo 1."""
    k = scene_constants(full_width, full_height, scale)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    X, Y = (x + 0.5) * (full_width / width), (y + 0.5) * (full_height / height)
    hit = Y >= k["sky"]
    thin = hit & (X >= k["column"]) & (X < k["column"] + 1) & (Y >= k["rows"][0]) & (Y < k["rows"][1])
    right = hit & ~thin & (X > edge_x(k, Y))
    left = hit & ~thin & ~right
    ident = np.where(thin, ID_THIN, np.where(right, ID_RIGHT, np.where(left, ID_LEFT, np.uint32(0)))).astype(np.uint32)
    normal = np.zeros((height, width, 3))
    normal[left], normal[right], normal[thin] = N_LEFT, N_RIGHT, N_THIN
    # the right plane starts half a world unit behind the left one and recedes; the thin feature floats in front
    depth = np.where(right, 0.5 + 0.75 * 0.05 * (X - edge_x(k, Y)), np.where(thin, -0.3, 0.0))
    point = np.where(hit[..., None], np.stack([X * 0.05, Y * 0.05, -depth], -1), 0.0)
    u, v = X / full_width, Y / full_height
    tex = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * 23 * u) * np.cos(2 * np.pi * 17 * v), 0.5 + 0.4 * np.cos(2 * np.pi * 19 * u + 2 * np.pi * 13 * v),
                    0.55 + 0.35 * np.sin(2 * np.pi * 29 * v - 2 * np.pi * 7 * u)], -1)
    albedo = np.ones((height, width, 4))
    albedo[..., :3] = np.where(hit[..., None], tex, 1.0)
    e_left = np.stack([0.8 + 0.15 * np.sin(2.0 * u + v), 0.75 + 0.2 * np.cos(1.5 * v), 0.7 + 0.1 * np.sin(3.0 * u)], -1)
    e_right = np.stack([0.35 + 0.1 * np.cos(3.0 * v), 0.3 + 0.1 * np.sin(2.0 * u), 0.4 + 0.05 * np.cos(u + v)], -1)
    e_thin = np.broadcast_to(np.array([1.6, 1.4, 0.2]), e_left.shape)
    irradiance = np.where(thin[..., None], e_thin, np.where(right[..., None], e_right, e_left))
    clean = np.ones((height, width, 4))
    clean[..., :3] = np.where(hit[..., None], albedo[..., :3] * irradiance, np.array(SKY[:3]))
    return dict(albedo=albedo.astype(F), clean=clean.astype(F), normal=normal.astype(F), point=point.astype(F), id=ident, thin=thin)


def synthetic_pair(low_width, low_height, scale, *, specials=True):
    """(low, high, constants): the scene at low_width x low_height and at `scale` times that.  low["color"] is the low clean
    frame with, for `specials`, a NaN, a +inf and a NaN at NAN_PIXELS."""
    full_width, full_height = low_width * scale, low_height * scale
    low = view(low_width, low_height, full_width, full_height, scale)
    high = view(full_width, full_height, full_width, full_height, scale)
    color = low["clean"].copy()
    if specials:
        for n, (py, px) in enumerate(NAN_PIXELS):
            color[py % low_height, px % low_width, n % 3] = np.inf if n == 1 else np.nan
    low["color"] = color
    return low, high, scene_constants(full_width, full_height, scale)


def guides_of(view_, which=GUIDES):
    return {g: view_[g] for g in which}
