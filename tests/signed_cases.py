"""Closed meshes and point sets of the signed-distance tests (helper module; test_signed_cpu.py, test_gpu_signed.py), with the
analytic inside and distance of each shape.  Everything is deterministic; scene descriptions, oracles and the literal's view of a
scene are made once per process and shared.

  torus(nu, nv)  around the z axis, major radius 0.6, minor radius 0.25, outward wound; 24 x 12 = 576 triangles for the literal,
                 64 x 32 = 4 096 so that the model goes through the device builder
  two_boxes      (-0.8, -0.5, -0.5)..(0.2, 0.5, 0.5) and (-0.2, -0.3, -0.3)..(0.8, 0.7, 0.3): they overlap
  shell          the box (-0.8)^3..(0.8)^3 with the inward-wound box (-0.4)^3..(0.4)^3 inside it: a cavity
  holed          the 24 x 12 torus with one triangle removed"""
import math

import numpy as np

import hits_literal as hl
import oracle_lib as ol
import ray_edges as R
from rayca_amd import Config, PbrMaterial, TriangleMesh, Trs, flatten, scenes

F = np.float32
TORUS_R, TORUS_r = 0.6, 0.25
BAND = 0.02                      # analytic comparisons leave out the points this close to the surface
BOX_A = ((-0.8, -0.5, -0.5), (0.2, 0.5, 0.5))
BOX_B = ((-0.2, -0.3, -0.3), (0.8, 0.7, 0.3))
SHELL_OUTER, SHELL_INNER = ((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8)), ((-0.4, -0.4, -0.4), (0.4, 0.4, 0.4))
HOLE = 100                       # the triangle `holed` leaves out
NAMES = ["torus", "torus4k", "two_boxes", "shell", "holed"]

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
def signed_volume(pos, idx):
    """the divergence theorem over the triangles, f64: positive for a closed mesh wound outward"""
    t = np.asarray(pos, np.float64)[np.asarray(idx, np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def torus_mesh(nu, nv, skip=None):
    """(positions, indices): nu x nv shared vertices on the torus -- the seams share them too, so the mesh is closed bit for bit --
    two triangles per quad, wound so that d/du x d/dv, the outward normal, is their front"""
    u = (np.arange(nu) * (2 * math.pi / nu))[:, None]
    v = (np.arange(nv) * (2 * math.pi / nv))[None, :]
    ring = TORUS_R + TORUS_r * np.cos(v)
    pos = np.stack([ring * np.cos(u), ring * np.sin(u), np.broadcast_to(TORUS_r * np.sin(v), (nu, nv))], -1).reshape(-1, 3).astype(F)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    at = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)
    i0, i1, i2, i3 = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
    idx = np.stack([i0, i1, i2, i0, i2, i3], 1).reshape(-1, 3)
    assert signed_volume(pos, idx) > 0, "the torus must be wound outward"
    if skip is not None:
        idx = np.delete(idx, skip, 0)
    return pos, idx.reshape(-1).astype(np.uint32)


def _scene(pos, idx):
    pos = np.asarray(pos, F)
    tm = TriangleMesh(pos, np.asarray(idx, np.uint32), colors=np.ones((pos.shape[0], 4), F))
    return scenes._single_model_scene([(tm, PbrMaterial(color=(0.8, 0.8, 0.8, 1), roughness_factor=1.0))], Trs(translation=(0.0, 0.0, 4.0)), math.pi / 4)


def _boxes(*boxes):
    """(positions, indices) of axis-aligned boxes; a box given as (lo, hi, True) is wound inward"""
    pos, idx, nv = [], [], 0
    for lo, hi, *inward in boxes:
        b = scenes._MeshBuilder()
        b.box(lo, hi)
        p, i = np.concatenate(b.pos), np.concatenate(b.idx).reshape(-1, 3)
        if inward and inward[0]:
            i = i[:, [0, 2, 1]]
        assert (signed_volume(p, i) > 0) != bool(inward and inward[0])
        pos.append(p)
        idx.append(i.reshape(-1) + np.uint32(nv))
        nv += p.shape[0]
    return np.concatenate(pos), np.concatenate(idx)


def build_scene(name):
    if name == "torus":
        return _scene(*torus_mesh(24, 12))
    if name == "torus4k":
        return _scene(*torus_mesh(64, 32))
    if name == "holed":
        return _scene(*torus_mesh(24, 12, skip=HOLE))
    if name == "two_boxes":
        return _scene(*_boxes(BOX_A, BOX_B))
    if name == "shell":
        return _scene(*_boxes(SHELL_OUTER, (*SHELL_INNER, True)))
    raise KeyError(name)


def scene_desc(name):
    if name in NAMES:
        return cached(("desc", name), lambda: flatten(build_scene(name)))
    return R.scene_desc(name)


def oracle(name):
    if name in NAMES:
        return cached(("oracle", name), lambda: ol.OracleScene(scene_desc(name), Config()))
    return R.oracle_scene(name)


def reference(name):
    """the scene as hits_literal reads it"""
    return cached(("reference", name), lambda: hl.Reference(oracle(name)))


def flat_triangles(name):
    """(P, 3, 3) f32 world-space triangles in flatten order (permute by DeviceScene.primitive_order() for the device's slots)"""
    def make():
        orc = oracle(name)
        return orc.world_triangles(orc.primitive_count).astype(F).reshape(-1, 3, 3)
    return cached(("flat", name), make)


# ---- the analytic shapes ----------------------------------------------------------------------------------------------------------
def torus_distance(p):
    """signed distance to the torus itself (negative inside), f64"""
    p = np.asarray(p, np.float64)
    return np.hypot(np.hypot(p[:, 0], p[:, 1]) - TORUS_R, p[:, 2]) - TORUS_r


def box_distance(p, box):
    """signed distance to an axis-aligned box (negative inside), f64"""
    p, lo, hi = np.asarray(p, np.float64), np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    q = np.maximum(lo - p, p - hi)
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)


def facet_error(name, nu, nv):
    """How far the nu x nv torus mesh and the torus lie apart, the Hausdorff distance h = max(h1, h2): for every p the distance
    to the mesh and the distance to the torus differ by at most h.
      h1  mesh -> torus: the analytic distance at 28 points of every triangle (vertices, edge points, interior);
      h2  torus -> mesh: nearest_literal.closest from points of the torus -- the mesh repeats every 2 pi / nu around the axis,
          so one column of cells stands for all: 5 x 5 points in each of its nv cells (at most 1 000 points).
    Both are sampled maxima of smooth functions whose extremes lie at the cell centres and edge midpoints, which are sampled."""
    import nearest_literal as nl

    def make():
        tris = flat_triangles(name).astype(np.float64)
        k = 6
        w = np.array([(a, b, k - a - b) for a in range(k + 1) for b in range(k + 1 - a)], np.float64) / k
        on_mesh = np.einsum("sw,twc->tsc", w, tris).reshape(-1, 3)
        h1 = float(np.abs(torus_distance(on_mesh)).max())
        f = (np.arange(5) + 0.5) / 5
        u = (f * (2 * math.pi / nu))[:, None, None]
        v = ((np.arange(nv)[:, None] + f[None, :]) * (2 * math.pi / nv)).reshape(1, -1, 1)
        ring = TORUS_R + TORUS_r * np.cos(v)
        on_torus = np.concatenate([ring * np.cos(u), ring * np.sin(u), TORUS_r * np.sin(v) + 0 * u], -1).reshape(-1, 3).astype(F)
        assert on_torus.shape[0] <= 1000
        h2 = float(np.sqrt(nl.closest(flat_triangles(name), on_torus)[0].astype(np.float64)).max())
        return max(h1, h2), h1, h2
    return cached(("facet", name), make)


def torus_points(n=3000, seed=31):
    """uniform in (-1, 1) x (-1, 1) x (-0.4, 0.4): about 6 % of them lie within BAND of the torus"""
    return ((R._unit(seed, n, 3) * 2 - 1) * np.array([1.0, 1.0, 0.4])).astype(F)


def box_points(n=3000, seed=37, half=1.0):
    """uniform in (-half, half)^3"""
    return ((R._unit(seed, n, 3) * 2 - 1) * half).astype(F)


def surface_share(dist):
    """(keep, share): the points farther than BAND from the surface, and the share of the others -- at most a tenth"""
    keep = np.abs(dist) > BAND
    share = 1.0 - keep.mean()
    assert share <= 0.10, f"{share:.3f} of the points lie within {BAND} of the surface"
    return keep, share
