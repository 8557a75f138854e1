"""Scenes and ray sets of the multi-hit tests (helper module; test_hits_cpu.py, test_gpu_hits.py).  Everything is deterministic;
scene descriptions, oracles, the literal's view of a scene (hits_literal.Reference) and its full hit lists are made once per
process and shared."""
import os

import numpy as np

import hits_literal as hl
import oracle_lib as ol
import ray_edges as R
from rayca_amd import Config, Mesh, Model, Node, PbrMaterial, Primitive, Scene, Trs, flatten, scenes

F = np.float32
SCENES = ["box", "cornell", "soup1k", "twoblas", "coplanar", "louvre", "spheres"]
LOUVRE_QUADS = 40

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def louvre_scene() -> Scene:
    """Forty parallel unit quads [-0.5, 0.5]^2 at z = 0 .. 39, the even ones facing -z and the odd ones +z.  A ray from z = -1
    along +z through the interior (louvre_rays) hits quad i at t = i + 1, exactly in f32: the even ones with their front (twenty
    hits with RAYCA_HITS_FRONT), all forty with RAYCA_HITS_BOTH, faces 0, 1, 0, 1, ..."""
    model = Model("louvre")
    mat = model.materials.push(PbrMaterial(color=(0.8, 0.8, 0.8, 1), roughness_factor=1.0))
    x, y = np.array([1, 0, 0], F), np.array([0, 1, 0], F)
    prims = []
    for i in range(LOUVRE_QUADS):
        b = scenes._MeshBuilder()
        if i % 2 == 0:
            b.grid((-0.5, -0.5, float(i)), y, x, 1, 1)   # y cross x = -z
        else:
            b.grid((-0.5, -0.5, float(i)), x, y, 1, 1)   # x cross y = +z
        prims.append(model.primitives.push(Primitive(geometry=model.geometries.push(b.mesh()), material=mat)))
    model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=prims)))))
    scene = Scene("louvre")
    scene.push_model(model)
    scene.push_model(scenes.create_default_model())
    return scene


def chain_scene() -> Scene:
    """The deep scene of test_gpu_nearest.py, restated: a soup, and twenty-nine soups a tenth of its size in and around it.  The
    small models stay together in one TLAS leaf whose BLASes hang behind each other in a chain -- a stack need of 28 entries and
    more, beyond the LDS part of the node stack."""
    scene = scenes.soup_scene(24, seed=0xC4A10, extent=0.2)
    for k in range(1, 30):
        other = scenes.soup_scene(24, seed=0xC4A10 + k, extent=0.2)
        n = scene.push_model(other.models[0])
        scene.nodes[n].trs = Trs(translation=(0.45 * (k % 6) - 0.9, 0.45 * ((k // 6) % 3) - 0.4, 0.45 * (k // 18)), scale=(0.1, 0.1, 0.1))
    return scene


def scene_desc(name):
    if name == "louvre":
        return cached(("desc", name), lambda: flatten(louvre_scene()))
    if name == "chain":
        return cached(("desc", name), lambda: flatten(chain_scene()))
    return R.scene_desc(name)


def oracle(name):
    if name in ("louvre", "chain"):
        return cached(("oracle", name), lambda: ol.OracleScene(scene_desc(name), Config()))
    return R.oracle_scene(name)


def reference(name):
    """the scene as the literal reads it"""
    return cached(("reference", name), lambda: hl.Reference(oracle(name)))


def bounds(name):
    """(lo, hi, centre, diagonal) in f64"""
    if name == "spheres":
        return R.bounds(name)
    t = reference(name).tris.astype(np.float64).reshape(-1, 3)
    lo, hi = t.min(0), t.max(0)
    return lo, hi, (lo + hi) / 2, float(np.linalg.norm(hi - lo))


# ---- rays ---------------------------------------------------------------------------------------------------------------------
LOUVRE_TILT = 2.0 ** -10


def louvre_rays(n=256):
    """From z = -1 along +z through the interior of the quads, off the diagonal that splits them (sixty-fourths: exact in f32).
    The direction is (2^-10, 2^-10, 1), not (0, 0, 1): a ray with a direction component of exactly zero misses every box in the
    reference (the zero-safe reciprocal puts both planes of that axis at distance 0, and the box test wants tmax > 0), so it has
    no hits at all.  With dz = 1 and normals along z the depth is still (z - oz) / dz = i + 1 exactly; x and y move by 40 / 1024
    over the whole louvre and stay inside."""
    k = np.arange(n)
    x = ((k % 13) - 6) / 16.0 + 1 / 64.0
    y = ((k // 13 % 13) - 6) / 16.0 - 1 / 32.0
    o = np.stack([x, y, np.full(n, -1.0)], 1)
    return np.concatenate([o, np.tile([LOUVRE_TILT, LOUVRE_TILT, 1.0], (n, 1))], 1).astype(F)


def through_rays(name, n, seed):
    """Lines THROUGH the scene, from a shell around it: the origin 1.5 diagonals from the centre, the target a point of a
    triangle or anywhere in the bounds -- every triangle near the line is a candidate, in front of and behind the target."""
    lo, hi, c, diag = bounds(name)
    u = R._unit(seed, n, 3) * 2 - 1
    u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-3)
    o = c + u * (1.5 * diag)
    tris = reference(name).tris.astype(np.float64)
    tris = tris[np.abs(tris).sum((1, 2)) > 0]
    w = R._unit(seed + 1, n, 3) + 0.05
    tgt = (tris[R._pick(seed + 2, n, tris.shape[0])] * (w / w.sum(1, keepdims=True))[:, :, None]).sum(1)
    anywhere = c + (R._unit(seed + 3, n, 3) - 0.5) * np.maximum(hi - lo, 0.25 * diag)
    tgt[2::3] = anywhere[2::3]
    return np.concatenate([o, tgt - o], 1).astype(F)


def rays_for(name):
    """About 1 500 rays per scene: the committed or benign shell rays, lines through the scene, the scene's own special set."""
    def make():
        if name == "louvre":
            lo, hi, c, diag = bounds(name)
            back = louvre_rays(128).copy()          # the same lines from behind: z = 40 along -z, the odd quads show their front
            back[:, 2], back[:, 5] = 40.0, -1.0
            return np.concatenate([louvre_rays(256), back, through_rays(name, 400, 7)]).astype(F)
        if name == "chain":
            return through_rays(name, 1500, 17)
        if name == "soup1k":
            return soup_rays()
        parts = [R.shell_rays(name, 600, 5), through_rays(name, 700, 9)]
        if name == "coplanar":
            parts.append(R.family(name, "seams")[:400])
        return np.concatenate(parts).astype(F)
    return cached(("rays", name), make)


# Pairs of soup triangles (flatten order) whose centroids span a line that crosses eight to ten triangles, front or back: found
# once by a search over 24 000 such pairs with the literal, kept as data.  test_hits_cpu.py holds the counts.
SOUP_LINES = [(67, 368), (136, 158), (481, 82), (233, 576), (523, 93), (617, 689), (930, 639), (889, 488), (457, 693), (318, 45), (196, 876), (362, 861),
              (973, 27), (943, 609), (798, 530), (478, 321)]


def crossing_midpoints(tris):
    """The midpoint of the segment in which two triangles of a soup pierce each other, for every pair that does (f64).  A ray
    through such a point meets both triangles at the same depth up to rounding -- and often at exactly the same f32."""
    lo, hi = tris.min(1), tris.max(1)
    out = []
    for a in range(tris.shape[0]):
        near = np.flatnonzero((lo[a] <= hi).all(1) & (lo <= hi[a]).all(1))
        for b in near[near > a]:
            pts = []
            for p, q in ((tris[a], tris[b]), (tris[b], tris[a])):   # where an edge of p passes through the inside of q
                nq = np.cross(q[1] - q[0], q[2] - q[0])
                for e in range(3):
                    p0, p1 = p[e], p[(e + 1) % 3]
                    den = nq @ (p1 - p0)
                    if abs(den) < 1e-12:
                        continue
                    s = nq @ (q[0] - p0) / den
                    if 0 < s < 1:
                        x = p0 + s * (p1 - p0)
                        w = np.linalg.solve(np.stack([q[1] - q[0], q[2] - q[0], nq], 1), x - q[0])
                        if w[0] > 0 and w[1] > 0 and w[0] + w[1] < 1:
                            pts.append(x)
            if len(pts) >= 2:
                out.append((pts[0] + pts[1]) / 2)
    return np.array(out)


def soup_rays():
    """The soup's ray set: the committed rays (tests/golden/soup1k_rays.npz), lines through the scene, the lines of SOUP_LINES
    (many hits along each) and rays through the points where two triangles pierce each other (exact depth ties)."""
    def make():
        g = np.load(os.path.join(R.G, "soup1k_rays.npz"))["rays"].astype(F)
        tris = R.world_triangles("soup1k")
        cen = tris.mean(1)
        i, j = np.array(SOUP_LINES).T
        d = cen[j] - cen[i]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        lines = np.concatenate([cen[i] - 4.0 * d, d], 1)
        mids = crossing_midpoints(tris)
        o = R.shell_origins("soup1k", mids.shape[0], 400)
        return np.concatenate([g[:800], through_rays("soup1k", 400, 23), lines, np.concatenate([o, mids - o], 1)]).astype(F)
    return cached("soup_rays", make)


def full_lists(name, rays_key, rays, tmax_key, tmax, faces):
    """hits_literal.all_hits, once per (scene, ray set, bound set, faces)"""
    return cached(("full", name, rays_key, tmax_key, faces), lambda: hl.all_hits(reference(name), rays, tmax, faces))


def tmax_sets(name, rays):
    """{"none": None, "all": one bound for every ray, "per_ray": a bound per ray}.  per_ray: for every third ray exactly the t of
    one of its hits (the bound is strict: that hit and everything behind it drop out), for the next the float above it, then 0,
    negative, NaN, +inf, FLT_MAX and ordinary values in turn."""
    def make():
        t, _, _, _, total = full_lists(name, "main", rays, "none", None, "both")
        n = rays.shape[0]
        i = np.arange(n)
        finite = np.where(t[:, 0] < hl.FLT_MAX, t[:, 0], np.nan)
        typical = F(np.nanmedian(finite)) if np.isfinite(finite).any() else F(1)
        per = (typical * (0.25 + 1.5 * R._unit(77, n)[:, 0])).astype(F)
        special = np.array([0.0, -1.0, np.nan, np.inf, float(hl.FLT_MAX)], F)
        per = np.where(i % 16 >= 11, special[(i % 16 + 5 - 11) % 5], per).astype(F)
        pick = np.minimum((i // 3) % 4, np.maximum(total.astype(np.int64), 1) - 1)     # which hit the boundary sits on
        on = t[i, np.minimum(pick, hl.K_MAX - 1)]
        has = total > 0
        per = np.where(has & (i % 3 == 0) & (i % 16 < 11), on, per)
        with np.errstate(over="ignore"):   # (the miss record's FLT_MAX has no float above it; those rays take no boundary)
            above = np.nextafter(on, F(np.inf))
        per = np.where(has & (i % 3 == 1) & (i % 16 < 11), above, per).astype(F)
        return {"none": None, "all": typical, "per_ray": per}
    return cached(("tmax", name), make)
