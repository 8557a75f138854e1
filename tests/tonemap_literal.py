"""rayca_hip_meter_device and rayca_hip_tonemap_device, restated literally from their specification (include/rayca_hip.h,
DESIGN 4.13) -- not from the kernels.  The per-pixel part is numpy float32, vectorised over pixels, every operation one float32
operation in the association the specification writes; the bins come from a uint32 view of the luminance; everything behind the
histogram is Python integers, and the few float32 values of the exposure record are formed one rounded operation at a time.  Under
the library's arithmetic contract (no contraction, no fast math) the kernels give the same words.  The output stage is restated
for gamma == 1 only (powf belongs to the render kernels; the GPU tests pin the gamma of the pass against the denoiser's output
stage).

Every comparison is one a NaN fails."""
import numpy as np

from denoise_literal import quantize

F = np.float32
WORDS, COUNTED, BLACK, NOT_FINITE = 260, 256, 257, 258
LINEAR, REINHARD, ACES = 0, 1, 2
OPS = {"linear": LINEAR, "reinhard": REINHARD, "aces": ACES}
BIAS = (127 - 16) << 3


def luminance(r, g, b):
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def histogram(color):
    """hist_out: 260 uint32 words -- the bins, counted, black, not finite, 0"""
    c = np.ascontiguousarray(color, F).reshape(-1, 4)
    zero = F(0.0)
    with np.errstate(all="ignore"):
        r, g, b = c[:, 0], c[:, 1], c[:, 2]
        y = luminance(r, g, b)
        assert y.dtype == F
        finite = (r - r == zero) & (g - g == zero) & (b - b == zero) & (y - y == zero)
        black = finite & (y <= zero)
        counted = finite & ~black
    bins = (y[counted].view(np.uint32) >> np.uint32(20)).astype(np.int64) - BIAS
    bins = np.clip(bins, 0, 255)
    hist = np.zeros(WORDS, np.uint32)
    hist[:256] = np.bincount(bins, minlength=256)
    hist[COUNTED], hist[BLACK], hist[NOT_FINITE] = counted.sum(), black.sum(), (~finite).sum()
    return hist


def trimmed(hist, low_permille, high_permille):
    """(K, T): the pixels the trimmed mean keeps and their sum of 2 i + 1, Python integers"""
    n = int(hist[COUNTED])
    a, b = n * low_permille // 1000, n * high_permille // 1000
    c0 = k_sum = t_sum = 0
    for i in range(256):
        c1 = c0 + int(hist[i])
        k = max(0, min(c1, b) - max(c0, a))
        k_sum += k
        t_sum += k * (2 * i + 1)
        c0 = c1
    return k_sum, t_sum


def usable(prev):
    if prev is None:
        return False
    with np.errstate(all="ignore"):
        p = F(np.asarray(prev, F).reshape(-1)[0])
        return bool(p > F(0.0)) and bool(p - p == F(0.0))


def exposure(hist, *, low_permille=10, high_permille=990, key=0.18, min_scale=2.0 ** -10, max_scale=2.0 ** 10, rate=1.0, prev=None):
    """exposure_out: float32 {scale, target, L, 0}"""
    assert 0 <= low_permille < high_permille <= 1000 and key > 0 and 0 < min_scale <= max_scale and 0 < rate <= 1
    k_sum, t_sum = trimmed(hist, low_permille, high_permille)
    ok = usable(prev)
    p = F(np.asarray(prev, F).reshape(-1)[0]) if ok else None
    if k_sum == 0:
        lum, target = F(0.0), (p if ok else F(1.0))
    else:
        assert (t_sum << 12) < 2 ** 53
        q = (t_sum << 12) // k_sum
        lum = (F(1.0) + F(q & 0xffff) / F(65536.0)) * F(2.0 ** ((q >> 16) - 16))
        with np.errstate(all="ignore"):
            target = np.minimum(np.maximum(F(key) / lum, F(min_scale)), F(max_scale))
    with np.errstate(all="ignore"):
        scale = p + (target - p) * F(rate) if ok else target
    out = np.array([scale, target, lum, 0.0], F)
    assert type(lum) is F and out.dtype == F
    return out


def meter(color, *, exposure_out=True, **kw):
    """the whole call: (hist_out, exposure_out or None)"""
    hist = histogram(color)
    return hist, (exposure(hist, **kw) if exposure_out else None)


def aces(x):
    return (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))


def tonemap(color, op, *, scale=1.0, white=0.0):
    """The whole call for gamma == 1: (rgba32f (H, W, 4) float32, rgba8 (H, W, 4) uint8).  `scale` is the host's scale, or word 0
    of the exposure record (the same float32 either way)."""
    op = OPS.get(op, op)
    c = np.ascontiguousarray(color, F)
    assert c.ndim == 3 and c.shape[2] == 4 and op in (LINEAR, REINHARD, ACES) and (white == 0 or op == REINHARD)
    s, one = F(scale), F(1.0)
    o = c.copy()
    with np.errstate(all="ignore"):
        x = c[..., :3] * s
        if op == LINEAR:
            o[..., :3] = x
        elif op == REINHARD:
            inv_white2 = one / (F(white) * F(white)) if white != 0 else F(0.0)
            y = luminance(x[..., 0], x[..., 1], x[..., 2])
            m = (one + y * inv_white2) / (one + y)
            o[..., :3] = np.where((y > F(0.0))[..., None], x * m[..., None], x)
        else:
            o[..., :3] = aces(x)
    assert o.dtype == F
    return o, quantize(o)
