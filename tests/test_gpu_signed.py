"""rayca_hip_signed_device / DeviceScene.signed, signed_distance, occupancy: the nearest surface point of points in device memory
and a vote of crossing-count rays on the side they lie on, in one launch.

Every comparison of the entry's outputs is bit-exact: against the composition of the shipped entries (DeviceScene.nearest for the
distance part, DeviceScene.hits with k = 0 and count_all on torch-built rays for the counts, the literal's vote on those counts),
and against tests/signed_literal.py, the header's text in numpy f32.  Each scene is queried three ways -- RAYCA_BUILDER_REFERENCE,
RAYCA_BUILDER_SAH after finish() and right after creation; the ordered searches are judged through equality with the uncut ones
(RAYCA_TRAVERSAL_EXHAUSTIVE)."""
import ctypes as C

import numpy as np
import pytest

import nearest_literal as nl
import oracle_lib as ol
import ray_edges as R
import signed_cases as sc
import signed_literal as sl
from rayca_amd import Config, DeviceScene, abi, flatten, lib
from rayca_amd.lib import RaycaError
from rayca_amd.signed import grid_points, sign_directions
from test_gpu_nearest import chain_scene, far_points

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX, NONE = nl.FLT_MAX, nl.NONE
HOW = ["reference", "sah", "sah_unfinished"]
COMPOSED = ["box", "cornell", "soup1k", "torus", "torus4k", "two_boxes"]
LITERAL = ["box", "torus", "two_boxes", "shell", "holed"]
DIST = ("dist2", "prim", "point", "uv")
SIGN = ("inside", "votes", "cross")
DIRS5 = sign_directions(5)
LDS_ENTRIES = 24   # the LDS part of the node stack (select.inc kMaxLdsEntries): a tree that needs more entries spills


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(r):
    """a result dict as numpy arrays (after a synchronize)"""
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def make_scene(desc, how):
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    if how == "sah":
        ds.finish()
    return ds


def same(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} rows differ, first at {bad[:5]}: got {got[bad[:3]]}, want {want[bad[:3]]}"


def points_for(name, n=1800):
    """Uniform in 1.5 x the bounds; on vertices and centroids of triangles (dist2 ~ 0: either side of the surface); the centre; 10
    and 10^6 diagonals away; nine points with a coordinate that is not finite at the end.  (points, diagonal)"""
    def make():
        tris = sc.flat_triangles(name).astype(np.float64)
        tris = tris[np.abs(tris).sum((1, 2)) > 0]
        v = tris.reshape(-1, 3)
        lo, hi = v.min(0), v.max(0)
        c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
        ext = np.maximum(hi - lo, 0.1 * diag)
        parts = [c + (R._unit(211, n, 3) - 0.5) * 1.5 * ext, v[R._pick(212, 100, v.shape[0])], tris.mean(1)[R._pick(213, 100, tris.shape[0])], c[None],
                 far_points(c, diag, 10.0, 12, 214), far_points(c, diag, 1e6, 12, 215)]
        p = np.concatenate(parts).astype(F)
        bad = p[5:14].copy()
        for k in range(9):
            bad[k, k % 3] = F([np.nan, np.inf, -np.inf])[k // 3]
        return np.concatenate([p, bad]), diag
    return sc.cached(("gpu_points", name, n), make)


def radii_for(n, diag):
    """per point: 0, a negative value, NaN, +inf, FLT_MAX and ordinary values from 1 % to 60 % of the diagonal, in turn"""
    i = np.arange(n)
    ordinary = (0.01 + 0.59 * R._unit(271, n)[:, 0]) * diag
    special = np.array([0.0, -0.25 * diag, np.nan, np.inf, float(FLT_MAX)])
    return np.where(i % 8 < 5, special[i % 8 % 5], ordinary).astype(F)


def composed_counts(ds, points_d, dirs, **kw):
    """(front, back), (N, n_dirs) uint32 each, from the shipped multi-hit entry on rays built with torch"""
    import torch
    front, back = [], []
    for d in dirs:
        rays = torch.cat([points_d, torch.from_numpy(np.ascontiguousarray(d, F)).cuda().expand(points_d.shape[0], 3)], 1).contiguous()
        f = ds.hits(rays, 0, faces="front", count_all=True, outputs=("n",), **kw)["n"]
        b = ds.hits(rays, 0, faces="both", count_all=True, outputs=("n",), **kw)["n"]
        front.append(f)
        back.append(b - f)
    torch.cuda.synchronize()
    return (np.stack([x.cpu().numpy().view(np.uint32) for x in front], 1), np.stack([x.cpu().numpy().view(np.uint32) for x in back], 1))


def assert_signed_distance(sd, r):
    """signed_distance() against the outputs it is made of: the sign bit is `inside`, the magnitude torch's square root of dist2
    (compared within two units in the last place: nothing here says how that square root rounds)"""
    assert sd.dtype == np.float32 and np.array_equal(np.signbit(sd), r["inside"] != 0)
    want = np.sqrt(r["dist2"].astype(np.float64))
    assert (np.abs(np.abs(sd.astype(np.float64)) - want) <= 2.0 ** -22 * want).all()


def check_sign(r, front, back, rule, what):
    n_dirs = front.shape[1]
    votes, inside = sl.vote(front, back, sl.RULES[rule])
    same(r["cross"].view(np.uint32), np.stack([front, back], 2), f"{what}: cross")
    assert r["cross"].shape == (front.shape[0], n_dirs, 2)
    same(r["votes"], votes, f"{what}: votes")
    same(r["inside"], inside, f"{what}: inside")


# ---- 1: bit for bit the composition of the shipped entries ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", COMPOSED)
def test_equals_the_composition_of_nearest_and_hits(gpu, name, how):
    import torch
    desc = sc.scene_desc(name)
    ds = make_scene(desc, how)
    points, diag = points_for(name)
    n = points.shape[0]
    assert n <= 4000
    points_d = dev(points)
    per_point = radii_for(n, diag)
    front, back = composed_counts(ds, points_d, DIRS5)
    assert front[-9:].sum() == 0 and back[-9:].sum() == 0 and (front + back)[:-9].sum() > 0
    k = 0
    for rule in ("parity", "winding"):
        for n_dirs in (1, 3, 5):
            radius = (None, dev(per_point), float(F(0.2 * diag)))[k % 3]
            k += 1
            r = host(ds.signed(points_d, radius=radius, dirs=n_dirs, rule=rule))
            assert r["inside"].dtype == np.uint8 and r["votes"].dtype == np.uint8 and r["cross"].dtype == np.int32
            want = ds.nearest(points_d, radius=radius)
            torch.cuda.synchronize()
            for key, w in zip(DIST, want):
                same(r[key], w.cpu().numpy(), f"{name} {how} {rule} {n_dirs}: {key}")
            check_sign(r, front[:, :n_dirs], back[:, :n_dirs], rule, f"{name} {how} {rule} {n_dirs}")
            assert not r["inside"][-9:].any() and not r["votes"][-9:].any() and (r["prim"][-9:].view(np.uint32) == NONE).all()
    ds.close()


# ---- 2: against the literal, with per-point radii and the special values ----------------------------------------------------------------
def literal_counts(name, points):
    return sc.cached(("lit_counts", name, points.tobytes()), lambda: sl.crossings(sc.reference(name), points, DIRS5))


@pytest.mark.parametrize("how", ["reference", "sah"])
@pytest.mark.parametrize("name", LITERAL)
def test_all_outputs_match_the_literal(gpu, name, how):
    desc = sc.scene_desc(name)
    ds = make_scene(desc, how)
    points, diag = points_for(name, n=700)   # at most 1 000 points for the literal
    n = points.shape[0]
    assert n <= 1000
    points_d = dev(points)
    per_point = radii_for(n, diag)
    slot_tris = sc.flat_triangles(name)[ds.primitive_order()]
    front, back = literal_counts(name, points)
    for rule, n_dirs, radius_np, radius_arg in (("parity", 3, per_point, dev(per_point)), ("winding", 5, None, None), ("parity", 1, F(0.15 * diag), float(F(0.15 * diag)))):
        r = host(ds.signed(points_d, radius=radius_arg, dirs=n_dirs, rule=rule))
        want = nl.closest(slot_tris, points, radius_np)
        for key, w in zip(DIST, want):
            same(r[key], w, f"{name} {how} {rule} {n_dirs}: {key}")
        check_sign(r, front[:, :n_dirs], back[:, :n_dirs], rule, f"{name} {how} {rule} {n_dirs}")
        hit = want[1] != NONE
        if radius_np is not None:
            assert 0 < hit.sum() < n
        else:
            assert hit[:-9].all() and not hit[-9:].any()
    ds.close()


# ---- 3: the grid source ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 3, 2), (67, 9, 3)])
def test_grid_equals_points(gpu, dims):
    """The kernel's grid points are the literal's: a GRID call equals the POINTS call fed them, bit for bit.  67 x 9 x 3 has more
    than one wave per row of the grid and a ragged last block (1 809 = 7 x 256 + 17)."""
    ds = make_scene(sc.scene_desc("torus"), "sah")
    origin = (-0.95, -0.9, -0.3) if dims != (1, 1, 1) else (0.6, 0.01, 0.02)
    step = tuple(1.9 / max(d - 1, 1) * s for d, s in zip(dims, (1.0, 0.95, 0.3)))
    pts = sl.grid_points(origin, step, dims)
    assert np.array_equal(bits(pts), bits(grid_points(origin, step, dims)))
    radius = dev(radii_for(pts.shape[0], 2.0))
    for rule, n_dirs, rad in (("parity", 3, None), ("winding", 5, radius)):
        g = host(ds.signed(grid=(origin, step, dims), radius=rad, dirs=n_dirs, rule=rule))
        p = host(ds.signed(dev(pts), radius=rad, dirs=n_dirs, rule=rule))
        for key in DIST + SIGN:
            assert g[key].shape[0] == pts.shape[0]
            same(g[key], p[key], f"grid {dims} {rule}: {key}")
        if dims == (67, 9, 3):
            assert 0 < g["inside"].sum() < pts.shape[0]
        elif dims == (1, 1, 1):
            assert g["inside"][0] == 1 and g["votes"][0] == (1 << n_dirs) - 1   # inside the tube
    occ = ds.occupancy(grid=(origin, step, dims))
    sd = ds.signed_distance(grid=(origin, step, dims))
    import torch
    torch.cuda.synchronize()
    g = host(ds.signed(grid=(origin, step, dims)))
    assert np.array_equal(occ.cpu().numpy(), g["inside"])
    assert_signed_distance(sd.cpu().numpy(), g)
    ds.close()


# ---- 4: ordered against exhaustive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
@pytest.mark.parametrize("name", ["soup1k", "torus4k"])
def test_ordered_equals_exhaustive(gpu, name, how):
    ds = make_scene(sc.scene_desc(name), how)
    points, diag = points_for(name)
    points_d = dev(points)
    radius = dev(radii_for(points.shape[0], diag))
    for rule, n_dirs, rad in (("parity", 3, radius), ("winding", 5, None)):
        a = host(ds.signed(points_d, radius=rad, dirs=n_dirs, rule=rule, collect_stats=True))
        b = host(ds.signed(points_d, radius=rad, dirs=n_dirs, rule=rule, traversal=abi.TRAVERSAL_EXHAUSTIVE, collect_stats=True))
        for key in DIST + SIGN:
            same(a[key], b[key], f"{name} {how} {rule}: {key}, ordered against exhaustive")
        # the uncut nearest search tests every triangle for every live point; the ordered one is a subset
        assert a["stats"]["triangles_tested"] < b["stats"]["triangles_tested"], (a["stats"], b["stats"])
    ds.close()


# ---- 5: output subsets behind guard words ----------------------------------------------------------------------------------------------
def test_output_subsets_and_guards(gpu):
    import torch
    ds = make_scene(sc.scene_desc("two_boxes"), "sah")
    points, diag = points_for("two_boxes")
    n, n_dirs = 1000 - 5, 3   # (not a multiple of 64)
    points_d = dev(points[:n])
    radius = float(F(0.2 * diag))
    full = host(ds.signed(points_d, radius=radius, dirs=n_dirs, rule="winding"))
    shapes = {"dist2": (torch.float32, ()), "prim": (torch.int32, ()), "point": (torch.float32, (3,)), "uv": (torch.float32, (2,)),
              "inside": (torch.uint8, ()), "votes": (torch.uint8, ()), "cross": (torch.int32, (n_dirs, 2))}
    sentinel = {"dist2": -7.0, "prim": 0x5A5A5A5A, "point": -7.0, "uv": -7.0, "inside": 0xA5, "votes": 0xA5, "cross": 0x5A5A5A5A}
    big = {k: torch.full((n + 128, *tail), sentinel[k], dtype=dt, device="cuda") for k, (dt, tail) in shapes.items()}

    def run(names, stats=None):
        for k in big:
            big[k].fill_(sentinel[k])
        q = abi.RaycaSigned()
        q.count, q.source, q.points, q.radius_all, q.rule, q.n_dirs = n, abi.SIGNED_POINTS, points_d.data_ptr(), radius, abi.SIGNED_WINDING, n_dirs
        for j in range(n_dirs):
            for a in range(3):
                q.dirs[j][a] = float(DIRS5[j, a])
        for k in names:
            setattr(q, k + "_out", big[k][64:-64].data_ptr())
        o = ds._opts(abi.TRAVERSAL_ORDERED, stats is not None, None, None)
        rc = gpu.rayca_hip_signed_device(ds.handle, C.byref(o), C.byref(q), C.byref(stats) if stats is not None else None)   # (no stream: the call waits)
        torch.cuda.synchronize()
        return rc

    def check(names):
        for k in big:
            if k in names:
                same(big[k][64:-64].cpu().numpy(), full[k], f"outputs {names}: {k}")
                assert bool((big[k][:64] == sentinel[k]).all()) and bool((big[k][-64:] == sentinel[k]).all()), (names, k)
            else:
                assert bool((big[k] == sentinel[k]).all()), (names, k, "written without being asked for")

    lib.check(run(DIST + SIGN))
    check(DIST + SIGN)
    # the sign outputs alone: the nearest phase is compiled out -- no triangle is priced for it -- and no distance buffer is touched
    st_sign, st_all = abi.RaycaStats(), abi.RaycaStats()
    lib.check(run(SIGN, st_sign))
    check(SIGN)
    lib.check(run(DIST + SIGN, st_all))
    assert 0 < st_sign.triangles_tested < st_all.triangles_tested and 0 < st_sign.boxes_tested < st_all.boxes_tested
    for k in SIGN:                      # each sign output alone
        lib.check(run((k,)))
        check((k,))
    for k in DIST:                      # each distance output alone is a nearest-point query: refused, nothing written
        assert run((k,)) == abi.ERR_BAD_ARG
        check(())
        lib.check(run((k, "inside")))   # ... and beside one sign output
        check((k, "inside"))
    # the wrapper's form of a subset, into the caller's tensors
    out = {"votes": big["votes"][64:-64], "dist2": big["dist2"][64:-64]}
    r = ds.signed(points_d, radius=radius, dirs=n_dirs, rule="winding", outputs=("dist2", "votes"), out=out)
    torch.cuda.synchronize()
    assert set(r) == {"dist2", "votes"} and all(r[k].data_ptr() == out[k].data_ptr() for k in r)
    same(r["votes"].cpu().numpy(), full["votes"], "wrapper subset: votes")
    same(r["dist2"].cpu().numpy(), full["dist2"], "wrapper subset: dist2")
    ds.close()


# ---- 6: another stream and context -------------------------------------------------------------------------------------------------
def test_other_stream_and_context(gpu):
    import torch
    ds = make_scene(sc.scene_desc("cornell"), "sah")
    points, diag = points_for("cornell")
    points_d = dev(points)
    want = host(ds.signed(points_d, dirs=3, rule="winding"))
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    res = [ds.signed(points_d, dirs=3, rule="winding", stream=s, context=k + 1) for k, s in enumerate(streams)]
    raw = ds.occupancy(points_d, dirs=3, rule="winding", stream=streams[0].cuda_stream, context=7)
    sd = ds.signed_distance(points_d, dirs=3, rule="winding", stream=streams[1], context=2)
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        for key in DIST + SIGN:
            same(r[key].cpu().numpy(), want[key], f"context {k + 1}: {key}")
    assert np.array_equal(raw.cpu().numpy(), want["inside"])
    assert_signed_distance(sd.cpu().numpy(), want)
    with pytest.raises(RaycaError):
        ds.signed(points_d, context=8)
    ds.close()


# ---- 7: a tree whose stack need exceeds the LDS part -------------------------------------------------------------------------------
def chain_bounds(desc):
    orc = ol.OracleScene(desc, Config())
    v = orc.world_triangles(orc.primitive_count).astype(np.float64).reshape(-1, 3)
    orc.close()
    return v.min(0), v.max(0)


@pytest.mark.parametrize("how", HOW)
def test_tree_that_needs_the_spill_area(gpu, how):
    import torch
    desc = sc.cached("chain_desc", lambda: flatten(chain_scene()))
    ds = make_scene(desc, how)
    depth = ds.info()["max_depth"]
    assert depth + 1 > LDS_ENTRIES, "the scene must need more stack entries than the kernel keeps in LDS"
    lo, hi = sc.cached("chain_bounds", lambda: chain_bounds(desc))
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    points = np.concatenate([c + (R._unit(291, 1200, 3) - 0.5) * 1.5 * (hi - lo), far_points(c, diag, 10.0, 8, 294)]).astype(F)
    points_d = dev(points)
    radius = dev(radii_for(points.shape[0], diag))
    front, back = composed_counts(ds, points_d, DIRS5)
    assert (front + back).max() >= 2
    for rule, n_dirs, rad in (("parity", 5, None), ("winding", 3, radius)):
        a = host(ds.signed(points_d, radius=rad, dirs=n_dirs, rule=rule))
        b = host(ds.signed(points_d, radius=rad, dirs=n_dirs, rule=rule, traversal=abi.TRAVERSAL_EXHAUSTIVE))
        want = ds.nearest(points_d, radius=rad)
        torch.cuda.synchronize()
        for key, w in zip(DIST, want):
            same(a[key], w.cpu().numpy(), f"chain {how} {rule}: {key} against nearest()")
        for key in DIST + SIGN:
            same(a[key], b[key], f"chain {how} {rule}: {key}, ordered against exhaustive")
        check_sign(a, front[:, :n_dirs], back[:, :n_dirs], rule, f"chain {how} {rule}")
    ds.close()


# ---- 8: refusals that need a scene ---------------------------------------------------------------------------------------------------
def test_spheres_are_refused_then_a_scene_that_works(gpu):
    import torch
    ds = make_scene(R.scene_desc("spheres"), "reference")
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    inside = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    for outputs in (("inside",), ("inside", "dist2")):
        with pytest.raises(RaycaError) as e:
            ds.signed(p, outputs=outputs, out={"inside": inside})
        assert e.value.code == abi.ERR_UNSUPPORTED and "sphere" in str(e.value)
    torch.cuda.synchronize()
    assert bool((inside == 0xA5).all())
    with pytest.raises(RaycaError) as e:   # behind the struct's and the options' checks, as documented
        ds.signed(p, context=9)
    assert e.value.code == abi.ERR_BAD_ARG
    assert tuple(ds.occupancy(p[:0]).shape) == (0,)   # an empty batch asks nothing of the scene
    ds.close()
    ds = make_scene(sc.scene_desc("shell"), "reference")
    p = dev(F([[0, 0, 0], [0.6, 0, 0], [0.9, 0, 0]]))   # the cavity, the solid, outside
    assert ds.occupancy(p, out=inside[:3]).cpu().numpy().tolist() == [0, 1, 0]
    assert ds.occupancy(p, rule="winding").cpu().numpy().tolist() == [0, 1, 0]
    sd = ds.signed_distance(p).cpu().numpy()
    assert np.allclose(sd, [0.4, -0.2, 0.1], atol=1e-6)
    ds.close()


# ---- 9: the wrapper's checks -----------------------------------------------------------------------------------------------------------
def test_wrapper_checks(gpu):
    import torch
    ds = make_scene(sc.scene_desc("torus"), "sah")
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    grid = ((0, 0, 0), (0.1, 0.1, 0.1), (4, 4, 4))
    for bad in (dict(points=p.cpu()), dict(points=p.reshape(-1, 6)), dict(points=p, grid=grid), dict(), dict(points=p, rule="odd"), dict(points=p, dirs=2),
                dict(points=p, dirs=[[1, 0, 1]]), dict(points=p, dirs=np.ones((4, 3))), dict(points=p, outputs=()), dict(points=p, outputs=("dist2",)),
                dict(points=p, outputs=("inside", "inside")), dict(points=p, outputs=("inside", "within")), dict(points=p, radius=torch.ones(65, device="cuda")),
                dict(points=p, outputs=("inside",), out={"votes": torch.zeros(64, dtype=torch.uint8, device="cuda")}), dict(grid=((0, 0, 0), (1, 1, 1), (4, 0, 4))),
                dict(grid=((0, 0), (1, 1, 1), (4, 4, 4))), dict(grid=grid, radius=torch.ones(63, device="cuda")),
                dict(points=p, out={"inside": torch.zeros(63, dtype=torch.uint8, device="cuda")})):
        with pytest.raises(ValueError):
            ds.signed(bad.pop("points", None), **bad)
    for bad in (dict(points=p.double()), dict(points=np.zeros((64, 3), F)), dict(points=p, radius=torch.ones(64, device="cuda", dtype=torch.float64)),
                dict(points=p, out={"inside": torch.zeros(64, dtype=torch.int32, device="cuda")})):
        with pytest.raises(TypeError):
            ds.signed(bad.pop("points", None), **bad)
    # an (n, 3) array of directions, a strided input, an empty batch with statistics
    mine = F([[0.3, -0.5, 0.81], [-0.7, 0.2, 0.68], [0.11, 0.93, -0.35]])
    wide = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = torch.linspace(-1, 1, 64, device="cuda")[:, None] * torch.tensor([1.0, 0.31, 0.17], device="cuda")
    a, b = host(ds.signed(wide[:, :3], dirs=mine)), host(ds.signed(wide[:, :3].contiguous(), dirs=mine))
    front, back = composed_counts(ds, wide[:, :3].contiguous(), mine)
    for key in DIST + SIGN:
        same(a[key], b[key], f"strided points: {key}")
    check_sign(a, front, back, "parity", "caller's directions")
    assert 0 < a["inside"].sum() < 64
    empty = ds.signed(p[:0], dirs=5, want_stats=True)
    assert [tuple(empty[k].shape) for k in DIST + SIGN] == [(0,), (0,), (0, 3), (0, 2), (0,), (0,), (0, 5, 2)] and empty["stats"]["kernel_launches"] == 0
    ds.close()


# ---- 10: statistics --------------------------------------------------------------------------------------------------------------------
def test_statistics(gpu):
    ds = make_scene(sc.scene_desc("soup1k"), "sah")
    points, diag = points_for("soup1k")
    points_d = dev(points)
    n = points.shape[0]
    *_, st_near = ds.nearest(points_d, radius=0.1 * diag, collect_stats=True)
    for n_dirs in (1, 3, 5):
        st = ds.signed(points_d, radius=0.1 * diag, dirs=n_dirs, collect_stats=True)["stats"]
        plain = ds.signed(points_d, radius=0.1 * diag, dirs=n_dirs, want_stats=True)["stats"]
        sign_only = ds.signed(points_d, dirs=n_dirs, outputs=("inside",), collect_stats=True)["stats"]
        for s in (st, plain, sign_only):
            assert s["kernel_launches"] == 1 and s["kernel_ms"] > 0 and s["rays_primary"] == n * n_dirs
            assert s["class_launches"][abi.KERNEL_OTHER] == 1 and s["class_ms"][abi.KERNEL_OTHER] == s["kernel_ms"]
            assert s["rays_shadow"] == 0 and s["rays_bounce"] == 0
        assert plain["boxes_tested"] == 0 and plain["triangles_tested"] == 0
        assert st["boxes_tested"] > 0 and st["triangles_tested"] > 0 and sign_only["boxes_tested"] > 0 and sign_only["triangles_tested"] > 0
        # both phases are summed: the nearest call's work and the rays' on top
        assert st["boxes_tested"] == st_near["boxes_tested"] + sign_only["boxes_tested"], (st, st_near, sign_only)
        assert st["triangles_tested"] == st_near["triangles_tested"] + sign_only["triangles_tested"]
        if n_dirs == 1:
            assert st["boxes_tested"] >= st_near["boxes_tested"] and st["triangles_tested"] >= st_near["triangles_tested"]
    ds.close()


# ---- 11: signed_distance against the analytic torus ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["parity", "winding"])
def test_signed_distance_on_the_torus(gpu, rule):
    """The 4 096-triangle torus: the sign is exact away from the band, the magnitude lies within the distance between the mesh and
    the torus, which signed_cases.facet_error measures from the literal on the same mesh (and not from the kernel)."""
    import torch
    ds = make_scene(sc.scene_desc("torus4k"), "sah")
    points = sc.torus_points(4000, 61)
    dist = sc.torus_distance(points)
    keep, share = sc.surface_share(dist)
    sd = ds.signed_distance(dev(points), rule=rule)
    occ = ds.occupancy(dev(points), rule=rule)
    votes = ds.signed(dev(points), rule=rule, outputs=("votes",))["votes"]
    torch.cuda.synchronize()
    sd, occ, votes = sd.cpu().numpy(), occ.cpu().numpy(), votes.cpu().numpy()
    facet, h1, h2 = sc.facet_error("torus4k", 64, 32)
    err = np.abs(np.abs(sd.astype(np.float64)) - np.abs(dist))
    print(f"torus 64 x 32, {rule}: {share:.3f} within {sc.BAND}; mesh and torus up to {facet:.5f} apart ({h1:.5f}, {h2:.5f}); |distance| off by up to {err.max():.5f}")
    assert sd.dtype == np.float32 and np.array_equal(occ != 0, np.signbit(sd))
    assert np.isin(votes[keep], (0, 7)).all()
    assert np.array_equal(occ[keep], (dist[keep] < 0).astype(np.uint8))
    assert np.array_equal(sd[keep] < 0, dist[keep] < 0)
    assert err.max() <= 1.05 * facet + 1e-6   # (5 % for the sampling of the two maxima; 1e-6 for f32 at distances below 2)
    ds.close()
