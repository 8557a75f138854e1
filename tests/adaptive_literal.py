"""The sample plan of rayca_hip_sample_plan_device and the fold of rayca_hip_film_fold_device, restated literally from their
specification (include/rayca_hip.h) -- not from the kernels.  The weight is numpy float32, one operation a line's
term, in the association the specification writes; the sum, the prefix sums and the offsets are Python integers; the fold is a loop
over a pixel's samples around the blend rows of the accumulation (tests/temporal_literal.py states the same rows, vectorised over a
frame: test_adaptive_cpu.py holds the two against each other).

min() / max() are minNum / maxNum (np.fmin / np.fmax); every comparison is one a NaN fails."""
import numpy as np

from temporal_literal import luminance

F = np.float32


def weights(color, variance, length, *, target=0.05, lum_floor=1e-3, base_weight=0, fresh_weight=255, min_history=4):
    """(H, W) uint32, each 0..255"""
    c = np.ascontiguousarray(color, F)
    zero, one, top = F(0.0), F(1.0), F(255.0)
    with np.errstate(all="ignore"):
        t2 = F(target) * F(target)
        d = np.fmax(luminance(c), F(lum_floor))
        v = np.fmax(np.asarray(variance, F), zero)
        L = np.asarray(length, F)
        e = (v / np.fmax(L, one)) / (d * d)
        r = e / t2
        assert r.dtype == F
        q = np.where(r >= zero, np.floor(np.fmin(r, top)), zero)   # (a NaN fails r >= 0)
    w = np.minimum(np.uint32(base_weight) + q.astype(np.uint32), np.uint32(255))
    fresh = ~(L >= F(min_history))
    return np.where(fresh, np.maximum(w, np.uint32(fresh_weight)), w).astype(np.uint32)


def offsets(w, budget):
    """(H * W + 1,) uint32 from the weights in raster order, in Python integers"""
    flat = [int(x) for x in np.asarray(w).reshape(-1)]
    total = sum(flat)
    if total == 0:
        flat, total = [1] * len(flat), len(flat)
    out, before = [], 0
    for x in flat:
        out.append(before * budget // total)
        before += x
    out.append(budget)
    assert max(out) < 1 << 32
    return np.array(out, np.uint32)


def ray_pixels(offset):
    """pixel_out: (B,) uint32, the pixel p with offset[p] <= j < offset[p + 1] for every ray j"""
    counts = np.diff(np.asarray(offset).astype(np.int64))
    return np.repeat(np.arange(counts.size, dtype=np.uint32), counts)


def ray_strata(offset, jitter, first_stratum=0):
    """(B,) the stratum of every ray: (first_stratum + k) mod n^2 for the k-th ray of its pixel"""
    offset = np.asarray(offset).astype(np.int64)
    p = ray_pixels(offset).astype(np.int64)
    k = np.arange(p.size, dtype=np.int64) - offset[p]
    return ((first_stratum + k) % (jitter * jitter)).astype(np.uint32)


def plan(color, variance, length, budget, **kw):
    w = weights(color, variance, length, **kw)
    off = offsets(w, budget)
    return dict(weight=w, offset=off, pixel=ray_pixels(off))


def blend(present, h, L, m, c, max_history):
    """One sample into one pixel's state: the four rows of the accumulation's table.  h, c (4,), m (2,) float32; returns
    (color, length, moments)."""
    zero = F(0.0)
    with np.errstate(all="ignore"):
        d = c - c
        finite = bool(d[0] == zero and d[1] == zero and d[2] == zero and d[3] == zero)
        lum = luminance(c)
        if present and finite:
            n = L + F(1.0)
            if max_history > 0:
                n = np.fmin(n, F(max_history))
            a = F(1.0) / n
            return h + (c - h) * a, n, np.array([m[0] + (lum - m[0]) * a, m[1] + (lum * lum - m[1]) * a], F)
        if present:
            return h, L, m
        if finite:
            return c, F(1.0), np.array([lum, lum * lum], F)
        return c, zero, np.zeros(2, F)


def fold(samples, offset, history, *, max_history=0):
    """The whole call on a history dict color (H, W, 4), length (H, W), moments (H, W, 2): a dict color, length, moments and
    variance, float32.  A loop over the pixels, and over each pixel's samples in their order."""
    samples = np.ascontiguousarray(samples, F).reshape(-1, 4)
    offset = np.asarray(offset).astype(np.int64)
    color = np.array(history["color"], F)
    length = np.array(history["length"], F)
    moments = np.array(history["moments"], F)
    hgt, wid = length.shape
    assert offset.size == hgt * wid + 1
    zero = F(0.0)
    for p in range(hgt * wid):
        at = divmod(p, wid)
        o, L, m = color[at].copy(), length[at], moments[at].copy()
        for j in range(offset[p], offset[p + 1]):
            present = bool(L > zero)   # as identity mode takes a history; nothing of an absent one counts
            if not present:
                o, L, m = np.zeros(4, F), zero, np.zeros(2, F)
            o, L, m = blend(present, o, L, m, samples[j], max_history)
        color[at], length[at], moments[at] = o, L, m
    with np.errstate(all="ignore"):
        variance = np.fmax(moments[..., 1] - moments[..., 0] * moments[..., 0], zero)
    result = dict(color=color, length=length, moments=moments, variance=variance)
    for k, v in result.items():
        assert v.dtype == F, k
    return result


def synthetic_film(width, height, seed):
    """A film state to plan on: a calm left half and a noisy right half, and at fixed pixels (modulo the size; where they
    collide the later wins) NaN, negative and infinite variances, lengths 0, 1 and fractional, a NaN length, a black and a NaN
    colour.  A dict color (H, W, 4), variance, length (H, W) float32."""
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.05, 2.0, size=(height, width, 4)).astype(F)
    color[..., 3] = 1.0
    noisy = np.arange(width)[None, :] >= width // 2
    variance = np.where(noisy, rng.gamma(2.0, 0.05, size=(height, width)), rng.gamma(2.0, 1e-5, size=(height, width))).astype(F)
    length = rng.integers(4, 40, size=(height, width)).astype(F)

    def at(y, x):
        return y % height, x % width

    variance[at(0, 0)] = np.nan
    variance[at(1, 2)] = -1.0
    variance[at(2, 5)] = np.inf
    variance[at(2, 7)] = 0.0
    length[at(2, 7)] = 1.0           # one sample: variance 0, and not converged
    length[at(3, 1)] = 0.0
    length[at(3, 4)] = 2.5
    length[at(4, 3)] = np.nan
    color[at(5, 6)][:3] = 0.0        # black: the floor divides
    color[at(6, 2)][1] = np.nan
    color[at(7, 9)][0] = np.inf
    return dict(color=color, variance=variance, length=length)
