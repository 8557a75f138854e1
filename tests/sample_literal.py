"""The header's text on RaycaSurfaceCdf / RaycaSurfaceSample (include/rayca_hip.h) in numpy: areas and the samples' tails in
f32, one rounding per operation in the association the header writes; weights, sums and targets as Python integers; the hash
restated in uint32.  Nothing here knows about kernels, waves or a search: cdf() is a running sum, draw() a searchsorted on
exact integers."""
import numpy as np

NONE = 0xFFFFFFFF
F = np.float32
_U = np.uint32


# ---- the counter-based hash (rayca_math.hpp), on uint32 arrays: products and sums wrap ------------------------------------------
def rng_mix(h):
    h = np.asarray(h, _U).copy()
    h ^= h >> _U(16)
    h *= _U(0x85EBCA6B)
    h ^= h >> _U(13)
    h *= _U(0xC2B2AE35)
    h ^= h >> _U(16)
    return h


def rng_hash2(a, b):
    with np.errstate(over="ignore"):
        return rng_mix(np.asarray(a, _U) * _U(0x9E3779B1) + rng_mix(np.asarray(b, _U) + _U(0x7F4A7C15)))


def rng_root(seed, index, sample):
    return rng_hash2(rng_hash2(_U(seed), index), _U(sample))


def rng_word(key, dim):
    """W(key, d): the word rng_f32 takes its mantissa from"""
    return rng_hash2(np.asarray(key, _U) ^ _U(0xA511E9B3), _U(dim))


def rng_f32(key, dim):
    bits = _U(0x3F800000) | (rng_word(key, dim) >> _U(9))
    return bits.view(F) - F(1)


# ---- the table ----------------------------------------------------------------------------------------------------------------
def normals(tris):
    """ab, ac, n and a2 of (T, 3, 3) f32 triangles, every operation rounded to f32"""
    tris = np.asarray(tris, F)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        ab, ac = b - a, c - a
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1],
                      ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
        a2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    return ab, ac, n, a2


def areas(tris, include=None):
    """area_i as it counts: sqrt(a2) correctly rounded (numpy's f32 sqrt is), 0 where it is NaN or infinite or excluded"""
    with np.errstate(invalid="ignore"):
        area = np.sqrt(normals(tris)[3])
    assert area.dtype == F
    area = np.where(np.isfinite(area), area, F(0)).astype(F)
    if include is not None:
        area = np.where(np.asarray(include).astype(bool), area, F(0)).astype(F)
    return area


def weights(tris, include=None):
    """Python integers, one per slot"""
    area = areas(tris, include)
    amax = area[np.argmax(area.view(_U))] if area.size else F(0)   # the integer maximum over the bits
    if amax == 0:
        return [0] * area.size
    _, e = np.frexp(amax)   # amax = m * 2^e, 0.5 <= m < 1
    with np.errstate(under="ignore"):
        shifted = np.ldexp(area, np.int32(32 - int(e)))   # area * 2^(32 - e): exact unless it underflows
    assert shifted.dtype == F
    w = [int(x) for x in np.floor(shifted)]
    assert all(0 <= x < 1 << 32 for x in w)
    return w


def cdf(tris, include=None):
    """T + 1 Python integers: 0, then the running sums of the weights"""
    out = [0]
    for w in weights(tris, include):
        out.append(out[-1] + w)
    return out


def cdf_words(tris, include=None):
    return np.array(cdf(tris, include), np.uint64)


# ---- the draw -----------------------------------------------------------------------------------------------------------------
def keys(count, seed=0, sample=0, first_index=0):
    index = ((int(first_index) + np.arange(count, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(_U)
    return rng_root(seed, index, sample)


def barycentrics(key):
    s0, t0 = rng_f32(key, 2), rng_f32(key, 3)
    fold = s0 + t0 > F(1)
    s = np.where(fold, F(1) - s0, s0).astype(F)
    t = np.where(fold, F(1) - t0, t0).astype(F)
    return s, t


def slots_for(table, key):
    """prim per key: the i with table[i] <= target < table[i + 1], by exact integer arithmetic; NONE where the total is 0"""
    table = [int(x) for x in table]
    total = table[-1]
    if total == 0:
        return np.full(key.shape, NONE, _U)
    assert all(0 <= x < 1 << 64 for x in table)
    # target = floor(r * total / 2^64) < total with r = W(key, 0) * 2^32 + W(key, 1), on Python integers
    hi, lo = rng_word(key, 0), rng_word(key, 1)
    target = np.array([((int(h) << 32 | int(l)) * total) >> 64 for h, l in zip(hi, lo)], dtype=np.uint64)
    prim = np.searchsorted(np.array(table, np.uint64), target, side="right") - 1   # the last entry <= target
    assert (prim >= 0).all() and (prim < len(table) - 1).all()
    return prim.astype(_U)


def draw(tris, table, count, seed=0, sample=0, first_index=0):
    """(prim u32 (count,), uv f32 (count, 2), point f32 (count, 3), normal f32 (count, 3)) of samples 0 .. count - 1"""
    tris = np.asarray(tris, F)
    key = keys(count, seed, sample, first_index)
    prim = slots_for(table, key)
    uv, point, normal = np.zeros((count, 2), F), np.zeros((count, 3), F), np.zeros((count, 3), F)
    hit = prim != NONE
    if hit.any():
        s, t = barycentrics(key[hit])
        p = prim[hit]
        ab, ac, n, a2 = normals(tris[p])
        a = tris[p, 0]
        uv[hit] = np.stack([(F(1) - s) - t, s], axis=1)
        point[hit] = (a + ab * s[:, None]) + ac * t[:, None]
        normal[hit] = n / np.sqrt(a2)[:, None]
    return prim, uv, point, normal
