"""rayca_hip_nearest_device / DeviceScene.nearest: the nearest surface point to points in device memory, within a radius.

Every comparison is bit-exact -- dist2, point and uv by their bits, prim and the mask directly -- against tests/nearest_literal.py,
the header's text in numpy f32: brute force over the slots, nothing about a tree.  The triangles the literal reads are the
oracle's world-space triangles permuted by DeviceScene.primitive_order().  Each scene is queried three ways:
RAYCA_BUILDER_REFERENCE, RAYCA_BUILDER_SAH after finish() and RAYCA_BUILDER_SAH right after creation; the cull is judged only
through equality with the uncut search (RAYCA_TRAVERSAL_EXHAUSTIVE) and the literal, and by its counters where it must bite."""
import ctypes as C

import numpy as np
import pytest

import nearest_literal as nl
import oracle_lib as ol
import ray_edges as R
from rayca_amd import Config, DeviceScene, Scene, Trs, abi, flatten, lib, scenes
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
FLT_MAX, NONE = nl.FLT_MAX, nl.NONE
HOW = ["reference", "sah", "sah_unfinished"]
NAMES = ["box", "cornell", "soup1k", "twoblas", "coplanar"]
LDS_ENTRIES = 24   # the LDS part of k_nearest's node stack (select.inc kMaxLdsEntries): a tree that needs more entries spills


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_scene(desc, how):
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    if how == "sah":
        ds.finish()
    return ds


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def slot_triangles(key, desc, ds):
    """(n, 3, 3) f32 by slot of `ds`; one oracle per scene, one permutation per slot order"""
    flat = cached(("flat", key), lambda: _flat_triangles(desc))
    order = ds.primitive_order()
    assert np.array_equal(np.sort(order), np.arange(flat.shape[0]))
    return flat[order], order.tobytes()


def _flat_triangles(desc):
    orc = ol.OracleScene(desc, Config())
    t = orc.world_triangles(orc.primitive_count).astype(np.float32).reshape(-1, 3, 3)
    orc.close()
    return t


def literal(key, desc, ds, points, radius, what):
    """the literal's (dist2, prim, point, uv, within), computed once per (scene, slot order, point set, radius set)"""
    tris, order_key = slot_triangles(key, desc, ds)
    return cached(("literal", key, order_key, what), lambda: nl.closest(tris, points, radius))


def bounds_of(tris):
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, (lo + hi) / 2, float(np.linalg.norm(hi - lo))


def far_points(centre, diag, factor, n, seed):
    u = R._unit(seed, n, 3) * 2 - 1
    u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-3)
    return centre + u * (factor * diag)


def points_for(name):
    """About 2 000 points: uniform in 1.5 x the bounds; on vertices, edges and inside triangles (ties, dist2 ~ 0) and one ulp
    beside them; the centre of the bounds (the Box: a six-way tie); 10 and 10^6 diagonals away; coordinates that are not finite."""
    def make():
        tris = R.world_triangles(name)
        lo, hi, c, diag = bounds_of(tris)
        ext = np.maximum(hi - lo, 0.1 * diag)
        parts = [c + (R._unit(11, 900, 3) - 0.5) * 1.5 * ext]
        for k, kind in enumerate(("vertex", "edge", "inside")):
            on = R.targets(name, kind, 240, 20 + 10 * k).astype(np.float32)
            beside = on.copy()
            axis = np.arange(on.shape[0]) % 3
            beside[np.arange(on.shape[0]), axis] = np.nextafter(on[np.arange(on.shape[0]), axis], np.float32(np.inf) * np.where(np.arange(on.shape[0]) % 2, 1, -1).astype(np.float32))
            parts += [on, beside[:100]]
        parts += [c[None], np.zeros((1, 3)), far_points(c, diag, 10.0, 16, 61), far_points(c, diag, 1e6, 16, 62)]
        p = np.concatenate(parts).astype(np.float32)
        bad = np.repeat(p[5:14], 1, 0).copy()
        for k in range(9):
            bad[k, k % 3] = np.float32([np.nan, np.inf, -np.inf])[k // 3]
        return np.concatenate([p, bad]), diag
    return cached(("points", name), make)


def radii_for(name, n, diag):
    """per point: 0, a negative value, NaN, +inf, FLT_MAX and ordinary values from 1 % to 60 % of the diagonal, in turn"""
    i = np.arange(n)
    ordinary = (0.01 + 0.59 * R._unit(71, n)[:, 0]) * diag
    special = np.array([0.0, -0.25 * diag, np.nan, np.inf, float(FLT_MAX)])
    return np.where(i % 8 < 5, special[i % 8 % 5], ordinary).astype(np.float32)


def run_closest(ds, points_d, radius=None, **kw):
    import torch
    d2, prim, point, uv = ds.nearest(points_d, radius=radius, kind="closest", **kw)
    torch.cuda.synchronize()
    assert d2.dtype == torch.float32 and prim.dtype == torch.int32 and point.dtype == torch.float32 and uv.dtype == torch.float32
    assert point.shape == (points_d.shape[0], 3) and uv.shape == (points_d.shape[0], 2)
    return d2.cpu().numpy(), prim.cpu().numpy().view(np.uint32), point.cpu().numpy(), uv.cpu().numpy()


def run_within(ds, points_d, radius=None, **kw):
    import torch
    m = ds.nearest(points_d, radius=radius, kind="within", **kw)
    torch.cuda.synchronize()
    assert m.dtype == torch.uint8
    return m.cpu().numpy()


def assert_same(got, want, what=""):
    (d2, prim, point, uv), (ed2, eprim, epoint, euv) = got, want[:4]
    bad = np.flatnonzero((prim != eprim) | (bits(d2) != bits(ed2)) | (bits(point) != bits(epoint)).any(axis=1) | (bits(uv) != bits(euv)).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {d2.size} records differ, first at {bad[:5]}: got {d2[bad[:5]]} {prim[bad[:5]]} {point[bad[:3]]} {uv[bad[:3]]}, "
                           f"want {ed2[bad[:5]]} {eprim[bad[:5]]} {epoint[bad[:3]]} {euv[bad[:3]]}")


# ---- 1: the five scenes, three builds, three kinds of radius ----------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", NAMES)
def test_all_outputs_match_the_literal(gpu, name, how):
    desc = R.scene_desc(name)
    ds = make_scene(desc, how)
    points, diag = points_for(name)
    n = points.shape[0]
    points_d = dev(points)
    per_point = radii_for(name, n, diag)
    found = {}
    for what, radius_np, radius_arg in (("none", None, None), ("scalar", np.float32(0.2 * diag), float(np.float32(0.2 * diag))), ("tensor", per_point, dev(per_point))):
        want = literal(name, desc, ds, points, radius_np, what)
        assert_same(run_closest(ds, points_d, radius_arg), want, f"{name} {how} radius {what}")
        mask = run_within(ds, points_d, radius_arg)
        assert np.array_equal(mask, want[4]), f"{name} {how} radius {what} within: {(mask != want[4]).sum()} differ"
        if what != "scalar":   # the uncut search: the same bits
            assert_same(run_closest(ds, points_d, radius_arg, traversal=abi.TRAVERSAL_EXHAUSTIVE), want, f"{name} {how} radius {what} exhaustive")
        found[what] = want[4]
        hit = want[1] != NONE
        assert (want[0][~hit] == FLT_MAX).all() and not want[2][~hit].any() and not want[3][~hit].any()
    # what the point set is there for: hits and misses under every kind of radius, exact zeros, and the special radii decide
    assert found["none"][:-9].all() and not found["none"][-9:].any()                   # only the non-finite points miss unbounded
    assert 0 < found["scalar"].sum() < n and 0 < found["tensor"].sum() < n
    i = np.arange(n)
    assert not found["tensor"][i % 8 < 3].any() and found["tensor"][:-9][(i % 8 == 3)[:-9] | (i % 8 == 4)[:-9]].all()
    free = literal(name, desc, ds, points, None, "none")
    assert (free[0] == 0).sum() >= 100, "points on the surface"
    ds.close()


def test_box_centre_is_a_six_way_tie_for_the_lowest_slot(gpu):
    desc = R.scene_desc("box")
    for how in ("reference", "sah"):
        ds = make_scene(desc, how)
        tris, _ = slot_triangles("box", desc, ds)
        d2_all = nl.on_triangle(tris[:, 0], tris[:, 1], tris[:, 2], np.zeros(3, np.float32))[3]
        ties = np.flatnonzero(d2_all == d2_all.min())
        assert ties.size >= 6
        d2, prim, _, _ = run_closest(ds, dev(np.zeros((1, 3), np.float32)))
        assert prim[0] == ties[0] and d2[0] == d2_all.min()
        ds.close()


# ---- 2: counts around the wave and the block, the empty batch ----------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_counts(gpu, how):
    desc = R.scene_desc("soup1k")
    ds = make_scene(desc, how)
    points, diag = points_for("soup1k")
    want = literal("soup1k", desc, ds, points, np.float32(0.2 * diag), "scalar")
    for count in (1, 63, 64, 65, 255, 257):
        got = run_closest(ds, dev(points[:count]), float(np.float32(0.2 * diag)))
        assert_same(got, tuple(w[:count] for w in want), f"{count} points")
        assert np.array_equal(run_within(ds, dev(points[:count]), float(np.float32(0.2 * diag))), want[4][:count])
    empty = ds.nearest(dev(points[:0]))
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0, 3), (0, 2)]
    assert tuple(ds.nearest(dev(points[:0]), kind="within").shape) == (0,)
    *_, st = ds.nearest(dev(points[:0]), want_stats=True)
    assert st["kernel_launches"] == 0
    ds.close()


# ---- 3: outputs: subsets, guards, in place ---------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_output_subsets_and_guards(gpu, how):
    import torch
    desc = R.scene_desc("twoblas")
    ds = make_scene(desc, how)
    points, diag = points_for("twoblas")
    n = 1000 - 5   # (not a multiple of 64)
    points_d = dev(points[:n])
    radius = float(np.float32(0.2 * diag))
    want = tuple(w[:n] for w in literal("twoblas", desc, ds, points, np.float32(0.2 * diag), "scalar"))
    big = {"dist2": torch.full((n + 128,), -7.0, dtype=torch.float32, device="cuda"), "prim": torch.full((n + 128,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
           "point": torch.full((n + 128, 3), -7.0, dtype=torch.float32, device="cuda"), "uv": torch.full((n + 128, 2), -7.0, dtype=torch.float32, device="cuda"),
           "within": torch.full((n + 128,), 0xA5, dtype=torch.uint8, device="cuda")}
    sentinel = {"dist2": -7.0, "prim": 0x5A5A5A5A, "point": -7.0, "uv": -7.0, "within": 0xA5}
    names = ("dist2", "prim", "point", "uv")
    out = tuple(big[k][64:-64] for k in names)
    r = ds.nearest(points_d, radius=radius, out=out)
    m = ds.nearest(points_d, radius=radius, kind="within", out=big["within"][64:-64])
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(r, out)) and m.data_ptr() == big["within"][64:-64].data_ptr()
    assert_same((r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32), r[2].cpu().numpy(), r[3].cpu().numpy()), want, "guarded outputs")
    assert np.array_equal(m.cpu().numpy(), want[4])
    for k, b in big.items():
        assert bool((b[:64] == sentinel[k]).all()) and bool((b[-64:] == sentinel[k]).all()), k
    # every subset of the four outputs: what is asked for is written, the rest is not touched
    for subset in range(1, 15):
        for k in names:
            big[k].fill_(sentinel[k])
        q = abi.RaycaNearest()
        q.kind, q.count, q.points, q.radius_all = abi.NEAREST_CLOSEST, n, points_d.data_ptr(), radius
        for j, k in enumerate(names):
            if subset >> j & 1:
                setattr(q, k + "_out", big[k][64:-64].data_ptr())
        o = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
        lib.check(gpu.rayca_hip_nearest_device(ds.handle, C.byref(o), C.byref(q), None))   # (no stream: the call waits)
        for j, k in enumerate(names):
            if subset >> j & 1:
                got = big[k][64:-64].cpu().numpy()
                assert np.array_equal(bits(got), bits(want[j])), (subset, k)
                assert bool((big[k][:64] == sentinel[k]).all()) and bool((big[k][-64:] == sentinel[k]).all())
            else:
                assert bool((big[k] == sentinel[k]).all()), (subset, k)
    # the wrapper's form of a subset: False leaves an output out
    d2, prim, point, uv = ds.nearest(points_d, radius=radius, out=(None, False, False, None))
    torch.cuda.synchronize()
    assert prim is None and point is None and np.array_equal(bits(d2.cpu().numpy()), bits(want[0])) and np.array_equal(bits(uv.cpu().numpy()), bits(want[3]))
    # in place: the nearest points over the points themselves (each lane reads its point before it writes)
    snapped = points_d.clone()
    ds.nearest(snapped, radius=radius, out=(False, False, snapped, False))
    torch.cuda.synchronize()
    assert np.array_equal(bits(snapped.cpu().numpy()), bits(want[2]))
    ds.close()


# ---- 4: another stream and context -------------------------------------------------------------------------------------------
def test_other_stream_and_context(gpu):
    import torch
    desc = R.scene_desc("cornell")
    ds = make_scene(desc, "sah")
    points, diag = points_for("cornell")
    points_d = dev(points)
    want = literal("cornell", desc, ds, points, None, "none")
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    res = [ds.nearest(points_d, stream=s, context=k + 1) for k, s in enumerate(streams)]
    raw = ds.nearest(points_d, stream=streams[0].cuda_stream, context=7, kind="within")
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        assert_same((r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32), r[2].cpu().numpy(), r[3].cpu().numpy()), want, f"context {k + 1}")
    assert np.array_equal(raw.cpu().numpy(), want[4])
    with pytest.raises(RaycaError):
        ds.nearest(points_d, context=8)
    ds.close()


# ---- 5: refusals that need a scene -------------------------------------------------------------------------------------------
def test_spheres_are_refused(gpu):
    import torch
    ds = make_scene(R.scene_desc("spheres"), "reference")
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    d2 = torch.full((64,), -7.0, dtype=torch.float32, device="cuda")
    for kind in ("closest", "within"):
        with pytest.raises(RaycaError) as e:
            ds.nearest(p, kind=kind, out=(d2, None, None, None) if kind == "closest" else None)
        assert e.value.code == abi.ERR_UNSUPPORTED and "sphere" in str(e.value)
    torch.cuda.synchronize()
    assert bool((d2 == -7.0).all())
    # behind the struct's and the options' checks, as documented: a bad context on the same scene is reported first
    with pytest.raises(RaycaError) as e:
        ds.nearest(p, context=9)
    assert e.value.code == abi.ERR_BAD_ARG
    assert tuple(ds.nearest(p[:0], kind="within").shape) == (0,)   # an empty batch asks nothing of the scene
    ds.close()


def test_wrapper_checks(gpu):
    import torch
    ds = make_scene(R.scene_desc("box"), "sah")
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ds.nearest(p.cpu())
    with pytest.raises(TypeError):
        ds.nearest(p.double())
    with pytest.raises(ValueError):
        ds.nearest(p.reshape(-1, 6))
    with pytest.raises(ValueError):
        ds.nearest(p, radius=torch.ones(65, device="cuda"))
    with pytest.raises(TypeError):
        ds.nearest(p, radius=torch.ones(64, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ds.nearest(p, kind="occluded")
    with pytest.raises(TypeError):
        ds.nearest(p, kind="within", out=torch.zeros(64, device="cuda"))
    with pytest.raises(ValueError):
        ds.nearest(p, out=(False, False, False, False))
    with pytest.raises(TypeError):
        ds.nearest(np.zeros((64, 3), np.float32))
    with pytest.raises(RaycaError) as e:
        ds.nearest(p, kind="within", traversal=abi.TRAVERSAL_EXHAUSTIVE)
    assert e.value.code == abi.ERR_UNSUPPORTED
    # a strided input is made contiguous
    wide = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = torch.linspace(-1, 1, 64, device="cuda")[:, None]
    a, b = run_closest(ds, wide[:, :3]), run_closest(ds, wide[:, :3].contiguous())
    assert_same(a, b, "strided points")
    ds.close()


# ---- 6: prim / uv are hit records' --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_surface_takes_prim_and_uv(gpu, how):
    """uv = (weight of vertex 0, weight of vertex 1), prim = the slot: what rayca_hip_surface_device reads.  The surface call runs
    on them as they are, gives a miss exactly where prim is NONE, and the colour of a hit is the colour of a ray's hit on the same
    primitive with the same (u, v)."""
    import torch
    desc = R.scene_desc("cornell")
    ds = make_scene(desc, how)
    points, diag = points_for("cornell")
    points_d = dev(points)
    d2, prim, point, uv = ds.nearest(points_d, radius=0.2 * diag)
    s = ds.surface(None, d2, prim, uv, want=("color", "material", "flags"))
    torch.cuda.synchronize()
    prim_np, flags = prim.cpu().numpy().view(np.uint32), s["flags"].cpu().numpy().view(np.uint32)
    miss = prim_np == NONE
    assert 0 < miss.sum() < miss.size
    assert np.array_equal((flags & np.uint32(abi.SURFACE_HIT)) == 0, miss)
    assert not s["color"].cpu().numpy()[miss].any() and (s["material"].cpu().numpy().view(np.uint32)[miss] == NONE).all()
    assert (s["color"].cpu().numpy()[~miss, 3] > 0).all()
    # the same records as hit records of rays: aimed at the nearest point from a little off the surface, the ray hits the same
    # slot where the nearest point lies inside its triangle, and the surface's colour there is the one read above
    uv_np = uv.cpu().numpy()
    inside = ~miss & (uv_np[:, 0] > 0.05) & (uv_np[:, 1] > 0.05) & (uv_np.sum(1) < 0.95) & (d2.cpu().numpy() > (1e-3 * diag) ** 2)
    assert inside.sum() > 50
    rays = torch.cat([points_d, point - points_d], 1)[torch.from_numpy(inside).cuda()]
    t, rprim, ruv = ds.query(rays)
    rs = ds.surface(None, t, rprim, ruv, want=("color", "material"))
    torch.cuda.synchronize()
    same = (rprim.cpu().numpy().view(np.uint32) == prim_np[inside])
    assert same.sum() > 20, same.sum()   # (back faces and nearer surfaces along the ray take the others)
    assert np.array_equal(rs["material"].cpu().numpy()[same], s["material"].cpu().numpy()[inside][same])
    assert np.abs(ruv.cpu().numpy()[same] - uv_np[inside][same]).max() < 1e-3
    assert np.abs(rs["color"].cpu().numpy()[same] - s["color"].cpu().numpy()[inside][same]).max() < 1e-3
    ds.close()


# ---- 7: a tree whose stack need exceeds the LDS part ------------------------------------------------------------------------
def chain_scene() -> Scene:
    """A soup, and twenty-nine soups a tenth of its size side by side in and around it.  The TLAS splits a set of models by
    comparing their half extents with the middle of the set's box (tlas.rs:74-134): the small ones are all alike and stay
    together, one TLAS leaf whose BLASes hang behind each other in a chain -- a stack need of 28 entries and more.  An ordered
    search that starts far from the head of the chain holds that many: the entries beyond the LDS part are used."""
    scene = scenes.soup_scene(24, seed=0xC4A10, extent=0.2)
    for k in range(1, 30):
        other = scenes.soup_scene(24, seed=0xC4A10 + k, extent=0.2)
        n = scene.push_model(other.models[0])
        scene.nodes[n].trs = Trs(translation=(0.45 * (k % 6) - 0.9, 0.45 * ((k // 6) % 3) - 0.4, 0.45 * (k // 18)), scale=(0.1, 0.1, 0.1))
    return scene


@pytest.mark.parametrize("how", HOW)
def test_tree_that_needs_the_spill_area(gpu, how):
    desc = cached("chain_desc", lambda: flatten(chain_scene()))
    ds = make_scene(desc, how)
    depth = ds.info()["max_depth"]
    print(f"chain scene, {how}: stack need {depth}")
    assert depth + 1 > LDS_ENTRIES, "the scene must need more stack entries than k_nearest keeps in LDS"
    tris, _ = slot_triangles("chain", desc, ds)
    lo, hi, c, diag = bounds_of(tris)
    u = R._unit(91, 1200, 3)
    points = np.concatenate([c + (u - 0.5) * 1.5 * (hi - lo), tris[R._pick(92, 300, tris.shape[0]), R._pick(93, 300, 3)], far_points(c, diag, 10.0, 8, 94)]).astype(np.float32)
    points_d = dev(points)
    per_point = radii_for("chain", points.shape[0], diag)
    for what, radius_np, radius_arg in (("none", None, None), ("tensor", per_point, dev(per_point))):
        want = literal("chain", desc, ds, points, radius_np, what)
        ordered = run_closest(ds, points_d, radius_arg)
        exhaustive = run_closest(ds, points_d, radius_arg, traversal=abi.TRAVERSAL_EXHAUSTIVE)
        assert_same(ordered, exhaustive, f"chain {how} {what}: ordered against exhaustive")
        assert_same(ordered, want, f"chain {how} {what}: against the literal")
        assert np.array_equal(run_within(ds, points_d, radius_arg), want[4])
    ds.close()


# ---- 8: a large scene: the cut search against the uncut one --------------------------------------------------------------------
def test_atrium_ordered_equals_exhaustive(gpu):
    """A hall of 23 000 triangles (the atrium at detail 4: the oracle that hands out the world-space triangles builds its BVH
    first, two seconds at this size), too many for the brute force on every point: the cut search against the uncut one on the
    device, and a few dozen points of both against the literal."""
    desc = flatten(scenes.atrium_scene(4))
    ds = make_scene(desc, "sah_unfinished")
    print(f"atrium at detail 4: {ds.info()['triangle_count']} triangles, stack need {ds.info()['max_depth']}")
    tris, _ = slot_triangles("atrium", desc, ds)
    lo, hi, c, diag = bounds_of(tris)
    n = 4096
    inside = c + (R._unit(101, n, 3) - 0.5) * (hi - lo)
    v = tris.reshape(-1, 3)
    near = v[R._pick(102, n, v.shape[0])] + (R._unit(103, n, 3) - 0.5) * 0.01 * diag
    points = np.where((np.arange(n) % 2 == 0)[:, None], inside, near).astype(np.float32)
    points[-1] = v[7]                                                      # a vertex: dist2 == 0, a tie among its triangles
    points_d = dev(points)
    per_point = radii_for("atrium", n, diag)
    for radius_np, radius_arg in ((None, None), (per_point, dev(per_point))):
        ordered = run_closest(ds, points_d, radius_arg)
        exhaustive = run_closest(ds, points_d, radius_arg, traversal=abi.TRAVERSAL_EXHAUSTIVE)
        assert_same(ordered, exhaustive, "atrium: ordered against exhaustive")
        assert np.array_equal(run_within(ds, points_d, radius_arg), (ordered[1] != NONE).astype(np.uint8))
        sub = np.arange(0, n, 128)[:32].tolist() + [n - 1]                 # a few dozen points against the brute force
        want = nl.closest(tris, points[sub], None if radius_np is None else radius_np[sub], chunk=8)
        assert_same(tuple(x[sub] for x in ordered), want, "atrium: a subsample against the literal")
        if radius_np is None:
            assert ordered[0][-1] == 0 and ordered[1].max() < tris.shape[0]
    ds.finish()
    assert_same(run_closest(ds, points_d, dev(per_point)), ordered, "atrium: after finish()")
    ds.close()


# ---- 9: the cull is alive, statistics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
@pytest.mark.parametrize("name", ["box", "soup1k"])
def test_cull_is_alive(gpu, name, how):
    """Points more than ten diagonals away with a radius of one diagonal: the root box and at most the root's two child boxes
    are priced, and no triangle."""
    desc = R.scene_desc(name)
    ds = make_scene(desc, how)
    tris, _ = slot_triangles(name, desc, ds)
    lo, hi, c, diag = bounds_of(tris)
    count = 333
    points_d = dev(far_points(c, diag, 12.0, count, 111).astype(np.float32))
    *res, st = ds.nearest(points_d, radius=diag, collect_stats=True)
    assert (res[1].cpu().numpy().view(np.uint32) == NONE).all()
    assert st["triangles_tested"] == 0 and 0 < st["boxes_tested"] <= 3 * count, st
    m, st_w = ds.nearest(points_d, radius=diag, kind="within", collect_stats=True)
    assert not m.cpu().numpy().any() and st_w["triangles_tested"] == 0 and st_w["boxes_tested"] <= 3 * count
    # unbounded from the same places: the cull still leaves most of the scene alone, the uncut search tests everything
    n_tris = tris.shape[0]
    *_, st_u = ds.nearest(points_d, collect_stats=True)
    *_, st_e = ds.nearest(points_d, collect_stats=True, traversal=abi.TRAVERSAL_EXHAUSTIVE)
    assert st_e["triangles_tested"] == n_tris * count
    assert 0 < st_u["triangles_tested"] <= st_e["triangles_tested"]
    if name == "soup1k":
        assert st_u["triangles_tested"] < st_e["triangles_tested"] and st_u["boxes_tested"] < st_e["boxes_tested"], (st_u, st_e)
    ds.close()


def test_statistics(gpu):
    desc = R.scene_desc("soup1k")
    ds = make_scene(desc, "sah")
    points, diag = points_for("soup1k")
    points_d = dev(points)
    n = points.shape[0]
    *_, st_c = ds.nearest(points_d, radius=0.1 * diag, collect_stats=True)
    _, st_w = ds.nearest(points_d, radius=0.1 * diag, kind="within", collect_stats=True)
    *_, st_u = ds.nearest(points_d, collect_stats=True)
    *_, st_plain = ds.nearest(points_d, radius=0.1 * diag, want_stats=True)
    for st in (st_c, st_w, st_u, st_plain):
        assert st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        assert st["class_launches"][abi.KERNEL_OTHER] == 1 and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
        assert all(v == 0 for k, v in st.items() if k.startswith("rays_")), st
    assert st_plain["boxes_tested"] == 0 and st_plain["triangles_tested"] == 0 and st_c["boxes_tested"] > 0 and st_c["triangles_tested"] > 0
    print({k: (st_w[k], st_c[k], st_u[k]) for k in ("boxes_tested", "triangles_tested")})
    for k in ("boxes_tested", "triangles_tested"):   # a search under a radius is a subset of the unbounded one; WITHIN ends earlier still
        assert st_w[k] <= st_c[k] <= st_u[k], k
    assert st_w["triangles_tested"] < st_c["triangles_tested"]
    ds.close()
