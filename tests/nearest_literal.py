"""rayca_hip_nearest_device restated (helper module; test_nearest_cpu.py, test_gpu_nearest.py): the header's comment on
RaycaNearest in numpy f32, operation by operation -- every + - * / rounds on its own, comparisons and selects, no square root.
Brute force over the slots in slot order; nothing here knows about a tree or a cull.

`tris` is (n, 3, 3) f32: the world-space vertices of slot 0, 1, ... (OracleScene.world_triangles permuted by
DeviceScene.primitive_order(): `slot_triangles`)."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
NONE = np.uint32(0xFFFFFFFF)
F0, F1 = np.float32(0), np.float32(1)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def on_triangle(a, b, c, p):
    """(s, t, q, dist2, region) of the nearest point of triangle (a, b, c) to p; arrays broadcast, [..., 3] f32.  region: 0 vertex
    a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 interior."""
    a, b, c, p = (np.asarray(x, np.float32) for x in (a, b, c, p))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)]
        region = np.full(d1.shape, 6, np.int32)
        for k in reversed(range(6)):   # the first test that holds decides
            region = np.where(tests[k], k, region)
        den = (va + vb) + vc
        si, ti = vb / den, vc / den
        si = np.where(si < 0, F0, si)
        si = np.where(si > 1, F1, si)
        room = F1 - si
        ti = np.where(ti < 0, F0, ti)
        ti = np.where(ti > room, room, ti)
        t_bc = d43 / (d43 + d56)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        s = np.select([region == 0, region == 1, region == 2, region == 3, region == 4, region == 5], [zero, one, d1 / (d1 - d3), zero, zero, F1 - t_bc], si)
        t = np.select([region == 0, region == 1, region == 2, region == 3, region == 4, region == 5], [zero, zero, zero, one, d2 / (d2 - d6), t_bc], ti)
        s, t = s.astype(np.float32), t.astype(np.float32)
        q = (a + ab * s[..., None]) + ac * t[..., None]
        shape = q.shape
        q = np.where((region == 0)[..., None], np.broadcast_to(a, shape), q)
        q = np.where((region == 1)[..., None], np.broadcast_to(b, shape), q)
        q = np.where((region == 3)[..., None], np.broadcast_to(c, shape), q).astype(np.float32)
        d = p - q
        dist2 = _dot(d, d)
    assert dist2.dtype == np.float32 and q.dtype == np.float32
    return s, t, q, dist2, region


def closest(tris, points, radius=None, chunk=256):
    """(dist2, prim, point, uv, within) per point: the smallest dist2 among the slots with dist2 < radius * radius, the lowest
    slot on equal dist2.  radius: None (unbounded), a scalar or an (N,) array."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = points.shape[0]
    radius = np.broadcast_to(np.asarray(np.inf if radius is None else radius, np.float32), (n,))
    with np.errstate(all="ignore"):
        r2 = radius * radius
    dist2_out = np.full(n, FLT_MAX, np.float32)
    prim_out = np.full(n, NONE, np.uint32)
    point_out = np.zeros((n, 3), np.float32)
    uv_out = np.zeros((n, 2), np.float32)
    for lo in range(0, n, chunk):
        p = points[lo:lo + chunk]
        s, t, q, dist2, _ = on_triangle(tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], p[:, None, :])   # [points, slots]
        with np.errstate(all="ignore"):
            counts = dist2 < r2[lo:lo + chunk, None]                   # (false for a NaN dist2 and for dist2 = +inf)
        alive = (radius[lo:lo + chunk] > 0) & np.isfinite(p).all(1)    # (false for a NaN radius)
        counts &= alive[:, None]
        key = np.where(counts, dist2, np.float32(np.inf))
        best = key.argmin(1)                                           # the first, i.e. lowest, slot of the smallest dist2
        rows = np.arange(p.shape[0])
        found = counts[rows, best]
        sel = lo + rows[found]
        b = best[found]
        dist2_out[sel] = dist2[rows[found], b]
        prim_out[sel] = b.astype(np.uint32)
        point_out[sel] = q[rows[found], b]
        sb, tb = s[rows[found], b], t[rows[found], b]
        uv_out[sel] = np.stack([(F1 - sb) - tb, sb], 1)
    return dist2_out, prim_out, point_out, uv_out, (prim_out != NONE).astype(np.uint8)


def slot_triangles(oracle_scene, order):
    """The device's slots as the literal reads them: the oracle's world-space triangles (flatten order) permuted by
    DeviceScene.primitive_order()."""
    t = oracle_scene.world_triangles(oracle_scene.primitive_count).astype(np.float32).reshape(-1, 3, 3)
    return t[np.asarray(order, np.int64)]
