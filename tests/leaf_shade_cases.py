"""Cases shared by test_leaf_shade_cpu.py, test_gpu_leaf_shade.py and make_leaf_shade_golden.py (helper module).

Frames: the small scenes, every combination of max_depth 1-3, samples_per_pixel 1-2 and light_samples 1-2 at 64x64.
Hit records: scenes whose primitive slots a batch of aimed rays must land on (first slots, the last slot, a record that
starts at byte 96 of a 128-B line, a 64-primitive leaf, a root that is a leaf, coincident triangles, a sphere slot), and
the soup fixture's rays with grazing rays (through triangle corners) and far rays (origins 10^6 units away, where a
triangle passes the triangle test while the box of its reference leaf fails the slab test) added."""
import math
import os

import numpy as np

import oracle_lib as ol
from rayca_amd import Config, PbrMaterial, TriangleMesh, Trs, flatten, scenes
from rayca_amd import model as M, sdtf

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = np.uint32(0xFFFFFFFF)
F = np.float32
FRAME = (64, 64)
COUNTER_KEYS = ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded", "boxes_tested", "triangles_tested")
LIGHT_POINT, LIGHT_QUAD = 1, 2   # include/rayca_hip.h RAYCA_LIGHT_*


def spheres_scene():
    scene = M.Scene()
    sdtf.push_sdtf_from_path(scene, os.path.join(G, "spheres.sdtf"))
    return scene


def quad_room():
    import test_gpu_general
    return test_gpu_general.quad_light_room("ggx")


FRAME_SCENES = {"box": scenes.box_scene, "cornell": scenes.cornell_scene, "spheres": spheres_scene, "quad_room": quad_room}
CONFIGS = [(f"d{d}_s{s}_l{l}", Config(max_depth=d, samples_per_pixel=s, light_samples=l, seed=17 + d))
           for d in (1, 2, 3) for s in (1, 2) for l in (1, 2)]

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def frame_desc(name):
    return _cached(("fdesc", name), lambda: flatten(FRAME_SCENES[name]()))


def light_kinds(desc):
    return [int(desc.c.lights[i].kind) for i in range(desc.c.light_count)]


# ---- hit-record scenes ---------------------------------------------------------------------------------------------------
def _tri_scene(tri, camera=(0.0, 0.0, 3.5)):
    tri = np.ascontiguousarray(tri, F).reshape(-1, 3)
    col = np.ones((tri.shape[0], 4), F)
    tm = TriangleMesh(tri, np.arange(tri.shape[0], dtype=np.uint32), colors=col)
    return scenes._single_model_scene([(tm, PbrMaterial(color=(1, 1, 1, 1), roughness_factor=1.0))], Trs(translation=tuple(camera)), math.pi / 4)


def _unit(seed, shape):
    return scenes.hash_unit(seed, np.arange(int(np.prod(shape)), dtype=np.uint32)).reshape(shape)


def coincident_scene():
    """70 copies of one triangle (an inseparable set: a 64-primitive leaf and the rest of its chain, every depth an exact
    tie) among 40 small triangles."""
    one = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.1], [0.0, 0.5, 0.1]], F)
    c = (_unit(0x7E5, (40, 1, 3)) * F(2) - F(1)) * F(0.8)
    soup = (c + (_unit(0x7E6, (40, 3, 3)) * F(2) - F(1)) * F(0.1)).astype(F)
    return _tri_scene(np.concatenate([np.broadcast_to(one, (70, 3, 3)), soup]))


def one_triangle_scene():
    return _tri_scene(np.array([[[-0.5, -0.4, 0.0], [0.6, -0.3, 0.1], [0.0, 0.7, -0.1]]], F))


HIT_SCENES = {"soup1k": lambda: scenes.soup_scene(1000, extent=0.12), "coincident": coincident_scene, "one_triangle": one_triangle_scene}


def hit_desc(name):
    return _cached(("hdesc", name), lambda: flatten(HIT_SCENES[name]()))


def oracle(name):
    return _cached(("oracle", name), lambda: ol.OracleScene(hit_desc(name), Config()))


def triangles(name):
    """[n, 3, 3] f32 world-space triangles in flatten order"""
    return _cached(("tri", name), lambda: oracle(name).world_triangles(oracle(name).primitive_count).reshape(-1, 3, 3))


def aimed_rays(tri):
    """Four rays per triangle from its front side (the triangle test culls back faces), a hundredth of its size away: at the
    centroid and at three interior points.  [n, 4, 6] f32"""
    t = tri.astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    size = np.sqrt(np.linalg.norm(n, axis=1, keepdims=True))
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    out = []
    for w in ((1, 1, 1), (4, 1, 1), (1, 4, 1), (1, 1, 4)):
        w = np.array(w, np.float64) / sum(w)
        p = (t * w[None, :, None]).sum(1)
        out.append(np.concatenate([p + n * size * 0.01, -n], 1))
    return np.stack(out, 1).astype(F)


# ---- the triangle test in f32, operation by operation (trace_core.inc tri_test) ----------------------------------------------
def _dot(a, b):
    p = a * b
    return ((F(-0.0) + p[..., 0]) + p[..., 1]) + p[..., 2]   # (the w lane adds +0)


def _cross(a, b):
    t0 = a[..., [1, 2, 0]]
    t1 = b[..., [2, 0, 1]]
    t2 = t0 * b
    t3 = t0 * t1
    return t3 - t2[..., [1, 2, 0]]


def tri_test_f32(tri, rays):
    """(passes [r, n] bool, t [r, n] f32) of every ray against every triangle, in the kernel's operation order"""
    with np.errstate(all="ignore"):
        o, d = rays[:, None, :3].astype(F), rays[:, None, 3:].astype(F)
        v0, v1, v2 = tri[None, :, 0].astype(F), tri[None, :, 1].astype(F), tri[None, :, 2].astype(F)
        n = _cross(v1 - v0, v2 - v0)
        ndd = _dot(n, d)
        ok = ~(_dot(d, n) > 0) & ~(np.abs(ndd) < F(1.1920929e-07))
        dd = -_dot(n, v0)
        t = -(_dot(n, o) + dd) / ndd
        ok &= ~(t < 0)
        p = o + d * t[..., None]
        ok &= ~(_dot(n, _cross(v1 - v0, p - v0)) < 0)
        ok &= ~(_dot(n, _cross(v2 - v1, p - v1)) < 0)
        ok &= ~(_dot(n, _cross(v0 - v2, p - v2)) < 0)
        return ok & np.isfinite(t), t


def grazing_rays(name="soup1k", per_corner=6):
    """Rays through the corners of the scene's triangles (exactly the f32 corner seen from hashed origins): the hit lies on an
    edge of the triangle and, where the corner is an extreme of its leaf, on a face of the leaf's box."""
    tri = triangles(name)
    corners = tri.reshape(-1, 3)
    k = np.arange(corners.shape[0] * per_corner, dtype=np.uint32)
    o = np.stack([(scenes.hash_unit(0x6A2 + a, k) * F(2) - F(1)) * F(2.5) for a in range(3)], 1).astype(F)
    target = np.repeat(corners, per_corner, 0)
    return np.concatenate([o, (target - o).astype(F)], 1).astype(F)


FAR_DISTANCES = (1.0e6, 3.0e6)   # scene units; the soup spans about 2.2 per axis


def far_rays(name="soup1k", per_corner=2):
    """Rays from origins 10^6 scene units away, aimed into the scene's triangles near their corners.  Over such a distance the
    slab test of a small box, (plane - o) * rd per plane, and the triangle's plane equation round differently: some of these
    rays pass the triangle test on a triangle whose reference leaf's box fails the slab test, so that the reference -- and the
    reference-leaf filter of the kernels, reference_candidate -- refuses the triangle and records a farther hit, or none."""
    tri = triangles(name)
    corners = tri.reshape(-1, 3).astype(np.float64)
    target = np.repeat(np.repeat(tri.astype(np.float64).mean(1), 3, 0) * 0.3 + corners * 0.7, per_corner, 0)
    k = np.arange(target.shape[0], dtype=np.uint32)
    d = np.stack([scenes.hash_unit(0x9B1 + a, k) * F(2) - F(1) for a in range(3)], 1).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = []
    for dist in FAR_DISTANCES:
        o = (target + d * dist).astype(F)
        out.append(np.concatenate([o, (target - o).astype(F)], 1))
    return np.concatenate(out).astype(F)


def soup_rays():
    """(rays, number of near rays): the soup fixture's rays and the grazing rays, then the far rays"""
    g = np.load(os.path.join(G, "soup1k_rays.npz"))
    near = np.concatenate([g["rays"], grazing_rays()]).astype(F)
    return np.concatenate([near, far_rays()]).astype(F), near.shape[0]


def nearer_passes(name, rays, chunk=512):
    """(indices, oracle depth [r], restated nearest depth [r]).  The indices are the rays on which some triangle passes the
    triangle test (f32, the kernel's operation order) at a depth below the oracle's record, or where the oracle records a miss:
    triangles the reference never tested, because the box of their leaf failed the slab test."""
    orc, tri = oracle(name), triangles(name)
    ot, oprim, _, _ = orc.trace_rays(rays)
    depth = np.where(oprim != NONE, ot, F(np.inf))
    nearest = np.empty(rays.shape[0], F)
    for s in range(0, rays.shape[0], chunk):
        ok, t = tri_test_f32(tri, rays[s:s + chunk])
        nearest[s:s + chunk] = np.where(ok, t, F(np.inf)).min(1)
    return np.flatnonzero(nearest < depth), depth, nearest


def soup_set():
    """(rays, number of near rays, indices of the refused rays, oracle depth, restated nearest depth): soup_rays() and
    nearer_passes() on it, made once"""
    def make():
        rays, n_near = soup_rays()
        return (rays, n_near) + nearer_passes("soup1k", rays)
    return _cached(("soup_set",), make)
