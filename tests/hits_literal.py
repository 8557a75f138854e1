"""rayca_hip_hits_device restated (helper module; test_hits_cpu.py, test_gpu_hits.py): the header's comment on RaycaHits in
numpy f32, operation by operation -- every + - * / rounds on its own.  Brute force over the reference's leaves and their
primitives: the box test on the leaf's box, the triangle test, the swap rule of RAYCA_HITS_BOTH, then the sort by (t, rank).
Nothing here knows about a traversal order, a cull or a list.

Primitives are numbered by RANK, their position in the reference's primitive order (OracleScene.primitive_order()); a column
index is a rank, so a stable sort by t alone is the sort by (t, rank).  Sphere candidates take their t from the oracle
(oracle_scene_primitive_intersects)."""
import ctypes as C

import numpy as np

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
FLT_EPSILON = F(1.1920929e-07)
NONE = np.uint32(0xFFFFFFFF)
K_MAX = 16   # RAYCA_HITS_MAX


# ---- the arithmetic of rayca_math.hpp, xyz lanes (the w lane of every product below is +0) -------------------------------------
def _dot(a, b):
    p = a * b
    return (((F(-0.0) + p[..., 0]) + p[..., 1]) + p[..., 2]) + F(0.0)


def _cross(a, b):
    t0 = a[..., [1, 2, 0]]
    t1 = b[..., [2, 0, 1]]
    t2 = t0 * b
    t3 = t0 * t1
    return t3 - t2[..., [1, 2, 0]]


def reciprocal(d):
    """zero-safe: 0 where the component is 0"""
    with np.errstate(all="ignore"):
        zero = d == 0
        return (np.where(zero, F(0), F(1)) / np.where(zero, F(1), d)).astype(F)


def slab(lo, hi, o, d):
    """AABB::intersects (trace_core.inc slab): (accepts, tmin); arrays broadcast, [..., 3] f32"""
    lo, hi, o, d = (np.asarray(x, F) for x in (lo, hi, o, d))
    with np.errstate(all="ignore"):
        rd = reciprocal(d)
        t1, t2 = (lo - o) * rd, (hi - o) * rd      # (fma(x, rd, 0): one rounding)
        far, near = np.fmax(t1, t2), np.fmin(t1, t2)   # fmaxf / fminf drop a NaN operand, as np.fmax / np.fmin do
        tmax = np.fmin(np.fmin(far[..., 0], far[..., 1]), np.fmin(far[..., 2], FLT_MAX))
        tmin = np.fmax(np.fmax(near[..., 0], near[..., 1]), np.fmax(near[..., 2], -FLT_MAX))
        return (tmax >= tmin) & (tmax > 0), tmin


def tri_test(v0, v1, v2, o, d):
    """Triangle::intersects on world-space vertices (trace_core.inc tri_test): (accepts, t, u, v, back) with `back` = rejected
    by the back-face line; arrays broadcast, [..., 3] f32"""
    v0, v1, v2, o, d = (np.asarray(x, F) for x in (v0, v1, v2, o, d))
    with np.errstate(all="ignore"):
        n = _cross(v1 - v0, v2 - v0)
        back = _dot(d, n) > 0
        denom = _dot(n, n)
        ndd = _dot(n, d)
        ok = ~back & ~(np.abs(ndd) < FLT_EPSILON)
        dd = -_dot(n, v0)
        t = -(_dot(n, o) + dd) / ndd
        ok &= ~(t < 0)
        p = o + d * t[..., None]
        ok &= ~(_dot(n, _cross(v1 - v0, p - v0)) < 0)
        u = _dot(n, _cross(v2 - v1, p - v1))
        ok &= ~(u < 0)
        v = _dot(n, _cross(v0 - v2, p - v2))
        ok &= ~(v < 0)
        return ok, t.astype(F), (u / denom).astype(F), (v / denom).astype(F), back


def slot_test(v0, v1, v2, o, d, both):
    """The hit of a triangle slot under RAYCA_HITS_FRONT / _BOTH: (hit, t, u, v, face)"""
    ok, t, u, v, back = tri_test(v0, v1, v2, o, d)
    face = np.zeros(ok.shape, np.uint8)
    if both:
        ok2, t2, u2, v2_, _ = tri_test(v0, v2, v1, o, d)
        take = ~ok & back & ok2
        with np.errstate(all="ignore"):
            w1 = ((F(1) - u2) - v2_).astype(F)
        t, u, v = np.where(take, t2, t), np.where(take, u2, u), np.where(take, w1, v)
        face = np.where(take, np.uint8(1), face)
        ok = ok | take
    return ok, t.astype(F), u.astype(F), v.astype(F), face


# ---- the reference's leaves -----------------------------------------------------------------------------------------------------
class Reference:
    """A scene as the literal reads it, by rank: tris (P, 3, 3) f32 world-space vertices, flat (P,) the flatten-order index,
    sphere (P,) bool, leaf (P,) the leaf that holds the primitive, lo / hi (L, 3) the leaves' boxes."""

    def __init__(self, orc):
        self.orc = orc
        p = orc.primitive_count
        self.flat = orc.primitive_order().astype(np.int64)
        world = orc.world_triangles(p).astype(F).reshape(-1, 3, 3)
        self.tris = world[self.flat]
        self.sphere = np.zeros(p, bool)
        leaf, lo, hi = np.full(p, -1, np.int64), [], []
        base = 0
        for b in range(orc.blas_count):
            boxes, rng = orc.blas_nodes(b)
            todo = [0]
            while todo:
                node = todo.pop()
                off, cnt = int(rng[node, 0]), int(rng[node, 1])
                if cnt == 0:   # an inner node: its children sit at offset, offset + 1
                    todo += [off, off + 1]
                else:
                    leaf[base + off:base + off + cnt] = len(lo)
                    lo.append(boxes[node, 0:3])
                    hi.append(boxes[node, 4:7])
            base += orc.lib.oracle_blas_primitive_count(orc.handle, b)
        assert base == p and (leaf >= 0).all()
        self.leaf, self.lo, self.hi = leaf, np.array(lo, F).reshape(-1, 3), np.array(hi, F).reshape(-1, 3)
        # sphere slots: world_triangles gives zeros for them, and the oracle tests them on request.  (A triangle that really is
        # all zeros accepts no ray, from the oracle neither: asking it costs time, never a result.)
        self.sphere = ~self.tris.reshape(p, -1).any(1)

    def sphere_t(self, src, o, d):
        t, uv = C.c_float(), (C.c_float * 2)()
        got = self.orc.lib.oracle_scene_primitive_intersects(self.orc.handle, int(src), (C.c_float * 3)(*[float(x) for x in o]),
                                                             (C.c_float * 3)(*[float(x) for x in d]), C.byref(t), uv)
        return F(t.value) if got == 1 else None


def all_hits(ref, rays, tmax=None, faces="front", chunk=128):
    """Every counting hit of every ray, in order: (t, rank, uv, face) as (N, K_MAX) arrays padded with the miss record, and
    total (N,), the number of counting hits."""
    assert faces in ("front", "both")
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n, p = rays.shape[0], ref.tris.shape[0]
    tm = np.broadcast_to(np.asarray(np.inf if tmax is None else tmax, F), (n,))
    bound = np.where(tm < FLT_MAX, tm, F(np.inf)).astype(F)          # FLT_MAX and +inf: unbounded, t < +inf
    alive = (tm > 0) & np.isfinite(rays).all(1)                       # (false for a NaN tmax)
    t_out, r_out = np.full((n, K_MAX), FLT_MAX, F), np.full((n, K_MAX), NONE, np.uint32)
    uv_out, f_out, total = np.zeros((n, K_MAX, 2), F), np.zeros((n, K_MAX), np.uint8), np.zeros(n, np.uint32)
    spheres = np.flatnonzero(ref.sphere)
    for a in range(0, n, chunk):
        r = rays[a:a + chunk]
        o, d = r[:, None, :3], r[:, None, 3:]
        seen = slab(ref.lo[None], ref.hi[None], o, d)[0][:, ref.leaf]                  # [rays, ranks]
        hit, t, u, v, face = slot_test(ref.tris[None, :, 0], ref.tris[None, :, 1], ref.tris[None, :, 2], o, d, faces == "both")
        hit = hit & ~ref.sphere[None]
        for s in spheres:
            for i in range(r.shape[0]):
                ts = ref.sphere_t(ref.flat[s], r[i, :3], r[i, 3:]) if alive[a + i] else None
                if ts is not None:
                    hit[i, s], t[i, s], u[i, s], v[i, s], face[i, s] = True, ts, 0, 0, 0
        with np.errstate(all="ignore"):
            counts = hit & seen & (t < bound[a:a + chunk, None]) & alive[a:a + chunk, None]   # (false for a NaN t and for t = +inf)
        key = np.where(counts, t, F(np.inf))
        order = np.argsort(key, axis=1, kind="stable")[:, :K_MAX]                             # by (t, rank)
        rows = np.arange(r.shape[0])[:, None]
        got = counts[rows, order]
        m = order.shape[1]
        t_out[a:a + chunk, :m] = np.where(got, t[rows, order], FLT_MAX)
        r_out[a:a + chunk, :m] = np.where(got, order.astype(np.uint32), NONE)
        uv_out[a:a + chunk, :m, 0] = np.where(got, u[rows, order], F(0))
        uv_out[a:a + chunk, :m, 1] = np.where(got, v[rows, order], F(0))
        f_out[a:a + chunk, :m] = np.where(got, face[rows, order], np.uint8(0))
        total[a:a + chunk] = counts.sum(1)
    return t_out, r_out, uv_out, f_out, total


def first_k(full, k, count_all=False):
    """rayca_hip_hits_device's five outputs from all_hits(): the first k entries and n"""
    t, rank, uv, face, total = full
    n = total if count_all else np.minimum(total, np.uint32(k))
    return t[:, :k].copy(), rank[:, :k].copy(), uv[:, :k].copy(), face[:, :k].copy(), n.astype(np.uint32)


def hits(ref, rays, k, tmax=None, faces="front", count_all=False):
    return first_k(all_hits(ref, rays, tmax, faces), k, count_all)
