"""rayca_hip_hits_device / DeviceScene.hits: the first k hits along rays in device memory, in order.

Every comparison is bit-exact and leaves no ray out -- t and uv by their bits, prim, face and n directly -- against
tests/hits_literal.py, the header's text in numpy f32: brute force over the reference's leaves, nothing about a traversal, a
cull or a list.  The literal numbers primitives by rank (the reference's primitive order); a device slot's rank comes from
DeviceScene.primitive_order().  Each scene is queried three ways: RAYCA_BUILDER_REFERENCE, RAYCA_BUILDER_SAH after finish() and
RAYCA_BUILDER_SAH right after creation.  tests/test_hits_cpu.py pins the literal to the oracle and holds the conditions on the
ray sets (long lists, exact ties, boundaries on a hit's t) without which these tests could pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import hits_cases as hc
import hits_literal as hl
import ray_edges as R
from rayca_amd import Config, DeviceScene, abi, lib
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
FLT_MAX, NONE = hl.FLT_MAX, hl.NONE
HOW = ["reference", "sah", "sah_unfinished"]
NAMES = ("t", "prim", "uv", "face", "n")
LDS_ENTRIES = 24   # the LDS part of k_hits' node stack (select.inc kMaxLdsEntries): a tree that needs more entries spills


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_scene(name, how):
    ds = DeviceScene(hc.scene_desc(name), Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    if how == "sah":
        ds.finish()
    return ds


def slot_of_rank(name, ds):
    """the device slot of the primitive with rank r"""
    order = np.asarray(ds.primitive_order(), np.int64)            # slot -> flatten index
    slot_of_flat = np.empty(order.size, np.int64)
    slot_of_flat[order] = np.arange(order.size)
    return slot_of_flat[hc.reference(name).flat]


def want_of(name, ds, rays_key, rays, tmax_key, tmax, faces, k, count_all=False):
    """the literal's five outputs for this device's slots"""
    t, rank, uv, face, n = hl.first_k(hc.full_lists(name, rays_key, rays, tmax_key, tmax, faces), k, count_all)
    sor = slot_of_rank(name, ds)
    prim = np.where(rank != NONE, sor[np.minimum(rank, sor.size - 1)], np.int64(NONE)).astype(np.uint32)
    return t, prim, uv, face, n


def run(ds, rays_d, k, **kw):
    import torch
    r = ds.hits(rays_d, k, **kw)
    torch.cuda.synchronize()
    n = rays_d.shape[0]
    if "t" in r:
        assert r["t"].dtype == torch.float32 and tuple(r["t"].shape) == (n, k)
    if "uv" in r:
        assert tuple(r["uv"].shape) == (n, k, 2)
    out = {name: x.cpu().numpy() for name, x in r.items() if name != "stats"}
    for name in ("prim", "n"):
        if name in out:
            out[name] = out[name].view(np.uint32)
    return out


def assert_same(got, want, what=""):
    wt, wprim, wuv, wface, wn = want
    n = wn.shape[0]
    bad = np.zeros(n, bool)
    if "t" in got:
        bad |= (bits(got["t"]) != bits(wt)).reshape(n, -1).any(1)
    if "prim" in got:
        bad |= (got["prim"] != wprim).reshape(n, -1).any(1)
    if "uv" in got:
        bad |= (bits(got["uv"]) != bits(wuv)).reshape(n, -1).any(1)
    if "face" in got:
        bad |= (got["face"] != wface).reshape(n, -1).any(1)
    if "n" in got:
        bad |= got["n"] != wn
    b = np.flatnonzero(bad)
    assert b.size == 0, (f"{what}: {b.size} of {n} rays differ, first at {b[:5]}: got n {got.get('n', wn)[b[:3]]} t {got.get('t', wt)[b[:2]]} prim "
                         f"{got.get('prim', wprim)[b[:2]]}, want n {wn[b[:3]]} t {wt[b[:2]]} prim {wprim[b[:2]]}")


# ---- 1: seven scenes, three builds, four k, both faces, three kinds of bound -----------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", hc.SCENES)
def test_all_outputs_match_the_literal(gpu, name, how):
    ds = make_scene(name, how)
    rays = hc.rays_for(name)
    rays_d = dev(rays)
    sets = hc.tmax_sets(name, rays)
    for tmax_key, tmax in sets.items():
        tmax_arg = dev(tmax) if isinstance(tmax, np.ndarray) and tmax.ndim else (None if tmax is None else float(tmax))
        for faces in ("front", "both"):
            for k in (1, 3, 8, 16):
                got = run(ds, rays_d, k, tmax=tmax_arg, faces=faces)
                assert_same(got, want_of(name, ds, "main", rays, tmax_key, tmax, faces, k), f"{name} {how} {tmax_key} {faces} k={k}")
    ds.close()


# ---- 2: count_all, ORDERED against EXHAUSTIVE ----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", ["soup1k", "louvre", "coplanar", "spheres"])
def test_count_all_and_exhaustive(gpu, name, how):
    ds = make_scene(name, how)
    rays = hc.rays_for(name)
    rays_d = dev(rays)
    sets = hc.tmax_sets(name, rays)
    for tmax_key in ("none", "per_ray"):
        tmax = sets[tmax_key]
        tmax_arg = None if tmax is None else dev(tmax)
        for faces in ("front", "both"):
            full = hc.full_lists(name, "main", rays, tmax_key, tmax, faces)
            crossings = run(ds, rays_d, 0, tmax=tmax_arg, faces=faces, count_all=True, outputs=("n",))
            assert set(crossings) == {"n"} and np.array_equal(crossings["n"], full[4]), f"{name} {how} {tmax_key} {faces}: crossing count"
            got = run(ds, rays_d, 3, tmax=tmax_arg, faces=faces, count_all=True)
            assert_same(got, want_of(name, ds, "main", rays, tmax_key, tmax, faces, 3, count_all=True), f"{name} {how} {tmax_key} {faces}: count_all, k = 3")
            if name == "louvre" and tmax is None:
                assert got["n"][:256].tolist() == [20 if faces == "front" else 40] * 256
            for k, count_all in ((3, False), (16, False), (3, True)):
                ordered = run(ds, rays_d, k, tmax=tmax_arg, faces=faces, count_all=count_all)
                exhaustive = run(ds, rays_d, k, tmax=tmax_arg, faces=faces, count_all=count_all, traversal=abi.TRAVERSAL_EXHAUSTIVE)
                for o in NAMES:
                    assert np.array_equal(bits(ordered[o]) if ordered[o].dtype == np.float32 else ordered[o],
                                          bits(exhaustive[o]) if exhaustive[o].dtype == np.float32 else exhaustive[o]), (name, how, tmax_key, faces, k, o)
                assert_same(exhaustive, want_of(name, ds, "main", rays, tmax_key, tmax, faces, k, count_all), f"{name} {how}: exhaustive")
    ds.close()


# ---- 3: the consequences: entry 0 is CLOSEST's record, n > 0 is OCCLUDED ---------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", ["cornell", "soup1k", "coplanar", "spheres"])
def test_entry_zero_is_the_closest_hit_and_n_is_occlusion(gpu, name, how):
    import torch
    ds = make_scene(name, how)
    rays = hc.rays_for(name)
    rays_d = dev(rays)
    sets = hc.tmax_sets(name, rays)
    for tmax_key, tmax in sets.items():
        tmax_arg = dev(tmax) if isinstance(tmax, np.ndarray) and tmax.ndim else (None if tmax is None else float(tmax))
        t, prim, uv = ds.query(rays_d, tmax=tmax_arg, kind="closest")
        occ = ds.query(rays_d, tmax=tmax_arg, kind="occluded")
        torch.cuda.synchronize()
        for k in (1, 8):
            got = run(ds, rays_d, k, tmax=tmax_arg)
            assert np.array_equal(bits(got["t"][:, 0]), bits(t.cpu().numpy())), (name, how, tmax_key, k)
            assert np.array_equal(got["prim"][:, 0], prim.cpu().numpy().view(np.uint32))
            assert np.array_equal(bits(got["uv"][:, 0]), bits(uv.cpu().numpy()))
            assert np.array_equal(got["n"] > 0, occ.cpu().numpy() == 1) and not got["face"].any()
    ds.close()


# ---- 4: the adversarial ray families ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["far", "axis", "scale", "seams", "surface"])
@pytest.mark.parametrize("name", ["soup1k", "coplanar"])
def test_adversarial_families(gpu, name, fam):
    """Origins hundreds to hundreds of thousands of diagonals away, zero / tiny / denormal direction components, scaled
    directions, rays through shared vertices and edges, origins on a surface: the conservative steering with its slack loses no
    hit of the literal, on the SAH scene before and after finish() and on the reference's own tree."""
    rays = R.family(name, fam)
    rays_d = dev(rays)
    for how in HOW:
        ds = make_scene(name, how)
        for faces, k in (("front", 3), ("both", 16)):
            got = run(ds, rays_d, k, faces=faces)
            assert_same(got, want_of(name, ds, fam, rays, "none", None, faces, k), f"{name} {fam} {how} {faces}")
        ds.close()
    assert (hc.full_lists(name, fam, rays, "none", None, "both")[4] > 0).any()


def test_rays_that_are_not_finite_have_no_hits(gpu):
    rays = R.family("cornell", "nonfinite")
    rays_d = dev(rays)
    ds = make_scene("cornell", "sah")
    for faces in ("front", "both"):
        got = run(ds, rays_d, 4, faces=faces, count_all=True)
        assert_same(got, want_of("cornell", ds, "nonfinite", rays, "none", None, faces, 4, True), f"nonfinite {faces}")
        bad = ~np.isfinite(rays).all(1)
        assert bad.sum() >= 32 and not got["n"][bad].any() and (got["prim"][bad] == NONE).all() and (got["n"][~bad] > 0).any()
    ds.close()


# ---- 5: counts around the wave and the workgroup ----------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_counts(gpu, how):
    ds = make_scene("coplanar", how)
    rays = hc.rays_for("coplanar")
    want = want_of("coplanar", ds, "main", rays, "none", None, "both", 8)
    for n in (1, 63, 64, 65, 255, 256, 257):
        got = run(ds, dev(rays[:n]), 8, faces="both")
        assert_same(got, tuple(w[:n] for w in want), f"count {n}")
    import torch
    empty = ds.hits(torch.zeros((0, 6), dtype=torch.float32, device="cuda"), 4, want_stats=True)
    assert tuple(empty["t"].shape) == (0, 4) and tuple(empty["n"].shape) == (0,) and empty["stats"]["kernel_launches"] == 0
    ds.close()


# ---- 6: every output subset, with guard words ----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_output_subsets_and_guards(gpu, how):
    import torch
    name, k = "twoblas", 5
    ds = make_scene(name, how)
    rays = hc.rays_for(name)
    n = 1000 - 5   # (not a multiple of 64)
    rays_d = dev(rays[:n])
    want = tuple(w[:n] for w in want_of(name, ds, "main", rays, "none", None, "both", k))
    shapes = {"t": (n * k,), "prim": (n * k,), "uv": (n * k * 2,), "face": (n * k,), "n": (n,)}
    dtypes = {"t": torch.float32, "prim": torch.int32, "uv": torch.float32, "face": torch.uint8, "n": torch.int32}
    sentinel = {"t": -7.0, "prim": 0x5A5A5A5A, "uv": -7.0, "face": 0xA5, "n": 0x5A5A5A5A}
    big = {o: torch.full((shapes[o][0] + 128,), sentinel[o], dtype=dtypes[o], device="cuda") for o in NAMES}
    view = {"t": (n, k), "prim": (n, k), "uv": (n, k, 2), "face": (n, k), "n": (n,)}
    inner = {o: big[o][64:-64].view(view[o]) for o in NAMES}

    def check_written(o, what):
        got = inner[o].cpu().numpy()
        w = want[NAMES.index(o)]
        assert np.array_equal(bits(got), bits(w)) if w.dtype == np.float32 else np.array_equal(got.view(w.dtype), w), (what, o)
        assert bool((big[o][:64] == sentinel[o]).all()) and bool((big[o][-64:] == sentinel[o]).all()), (what, o, "guards")

    r = ds.hits(rays_d, k, faces="both", out=inner)
    torch.cuda.synchronize()
    assert all(r[o].data_ptr() == inner[o].data_ptr() for o in NAMES)
    for o in NAMES:
        check_written(o, "all")
    for subset in range(1, 32):   # every subset of the five outputs: what is asked for is written, the rest is not touched
        for o in NAMES:
            big[o].fill_(sentinel[o])
        q = abi.RaycaHits()
        q.count, q.k, q.rays, q.tmax_all, q.faces = n, k, rays_d.data_ptr(), float("inf"), abi.HITS_BOTH
        for j, o in enumerate(NAMES):
            if subset >> j & 1:
                setattr(q, o + "_out", inner[o].data_ptr())
        opts = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
        lib.check(gpu.rayca_hip_hits_device(ds.handle, C.byref(opts), C.byref(q), None))   # (no stream: the call waits)
        for j, o in enumerate(NAMES):
            if subset >> j & 1:
                check_written(o, subset)
            else:
                assert bool((big[o] == sentinel[o]).all()), (subset, o)
    # the wrapper's form of a subset
    some = run(ds, rays_d, k, faces="both", outputs=("prim", "n"))
    assert set(some) == {"prim", "n"} and np.array_equal(some["prim"], want[1]) and np.array_equal(some["n"], want[4])
    ds.close()


# ---- 7: another stream and context; the wrapper's checks -----------------------------------------------------------------------
def test_other_stream_and_context(gpu):
    import torch
    name = "cornell"
    ds = make_scene(name, "sah")
    rays = hc.rays_for(name)
    rays_d = dev(rays)
    want = want_of(name, ds, "main", rays, "none", None, "both", 4)
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    res = [ds.hits(rays_d, 4, faces="both", stream=s, context=c + 1) for c, s in enumerate(streams)]
    raw = ds.hits(rays_d, 4, faces="both", stream=streams[0].cuda_stream, context=7)
    torch.cuda.synchronize()
    for c, r in enumerate(res + [raw]):
        got = {o: r[o].cpu().numpy() for o in NAMES}
        got["prim"], got["n"] = got["prim"].view(np.uint32), got["n"].view(np.uint32)
        assert_same(got, want, f"context {c + 1}")
    with pytest.raises(RaycaError):
        ds.hits(rays_d, 4, context=8)
    ds.close()


def test_wrapper_checks(gpu):
    import torch
    ds = make_scene("box", "sah")
    r = torch.zeros((64, 6), dtype=torch.float32, device="cuda")
    for bad in (dict(k=17), dict(k=-1), dict(k=2.0), dict(k=True), dict(k=0), dict(k=0, count_all=True), dict(k=0, count_all=True, outputs=("n", "t")),
                dict(faces="back"), dict(outputs=()), dict(outputs=("t", "t")), dict(outputs=("depth",)), dict(out={"uv": None}, outputs=("t",)),
                dict(tmax=torch.ones(65, device="cuda"))):
        kw = dict(k=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            ds.hits(r, kw.pop("k"), **kw)
    with pytest.raises(ValueError):
        ds.hits(r.cpu(), 4)
    with pytest.raises(ValueError):
        ds.hits(r.reshape(-1, 3), 4)
    for bad in (dict(tmax=torch.ones(64, device="cuda", dtype=torch.float64)), dict(out={"face": torch.zeros((64, 4), device="cuda")})):
        with pytest.raises(TypeError):
            ds.hits(r, 4, **bad)
    with pytest.raises(TypeError):
        ds.hits(np.zeros((64, 6), np.float32), 4)
    with pytest.raises(TypeError):
        ds.hits(r.double(), 4)
    # a strided input is made contiguous
    rays = hc.rays_for("box")[:256]
    wide = torch.zeros((256, 8), dtype=torch.float32, device="cuda")
    wide[:, :6] = dev(rays)
    a, b = run(ds, wide[:, :6], 2, faces="both"), run(ds, dev(rays), 2, faces="both")
    assert all(np.array_equal(a[o], b[o], equal_nan=True) for o in NAMES) and (a["n"] == 2).any()
    ds.close()


def test_empty_scene_is_refused(gpu):
    import torch
    from rayca_amd import Scene, flatten, scenes
    empty = Scene()
    empty.push_model(scenes.create_default_model())   # a camera and lights, nothing to hit
    ds = DeviceScene(flatten(empty), Config())
    r = torch.zeros((64, 6), dtype=torch.float32, device="cuda")
    with pytest.raises(RaycaError) as e:
        ds.hits(r, 2)
    assert e.value.code == abi.ERR_EMPTY_SCENE
    with pytest.raises(RaycaError) as e:   # the struct's and the options' checks come first
        ds.hits(r, 2, context=9)
    assert e.value.code == abi.ERR_BAD_ARG
    ds.close()


# ---- 8: a tree whose stack need exceeds the LDS part ------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
def test_tree_that_needs_the_spill_area(gpu, how):
    ds = make_scene("chain", how)
    depth = ds.info()["max_depth"]
    print(f"chain scene, {how}: stack need {depth}")
    assert depth + 1 > LDS_ENTRIES, "the scene must need more stack entries than k_hits keeps in LDS"
    rays = hc.rays_for("chain")
    rays_d = dev(rays)
    for faces, k in (("front", 1), ("both", 3), ("both", 16)):
        want = want_of("chain", ds, "main", rays, "none", None, faces, k)
        ordered = run(ds, rays_d, k, faces=faces)
        assert_same(ordered, want, f"chain {how} {faces} k={k}")
        assert_same(run(ds, rays_d, k, faces=faces, traversal=abi.TRAVERSAL_EXHAUSTIVE), want, f"chain {how} {faces} k={k}: exhaustive")
    assert (want[4] > 1).any()
    ds.close()


# ---- 9: prim / uv are hit records' --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_surface_takes_the_second_entry(gpu, how):
    """t, prim and uv of entry 1 -- the surface BEHIND the first one -- go to rayca_hip_surface_device as they are: a miss exactly
    where the entry is unused, and at a hit the point the surface call makes from (prim, u, v) is the ray's point o + d t.  On the
    louvre every second entry is the back of quad 1 (RAYCA_HITS_BOTH): its reconstructed point lies in the plane z = 1."""
    import torch
    for name in ("cornell", "louvre"):
        ds = make_scene(name, how)
        rays = hc.rays_for(name)
        rays_d = dev(rays)
        h = ds.hits(rays_d, 2, faces="both")
        t1, prim1, uv1 = h["t"][:, 1].contiguous(), h["prim"][:, 1].contiguous(), h["uv"][:, 1].contiguous()
        s = ds.surface(rays_d, t1, prim1, uv1, want=("point", "color", "material", "flags"))
        torch.cuda.synchronize()
        prim_np, flags = prim1.cpu().numpy().view(np.uint32), s["flags"].cpu().numpy().view(np.uint32)
        miss = prim_np == NONE
        assert 0 < miss.sum() < miss.size and np.array_equal(miss, h["n"].cpu().numpy() < 2)
        assert np.array_equal((flags & np.uint32(abi.SURFACE_HIT)) == 0, miss)
        assert not s["color"].cpu().numpy()[miss].any() and (s["color"].cpu().numpy()[~miss, 3] > 0).all()
        # the hit point from the weights against the ray's own point
        ref = hc.reference(name)
        rank_of_slot = np.empty(ref.flat.size, np.int64)
        rank_of_slot[slot_of_rank(name, ds)] = np.arange(ref.flat.size)
        tri = ref.tris[rank_of_slot[prim_np[~miss]]].astype(np.float64)
        uv = uv1.cpu().numpy()[~miss].astype(np.float64)
        p_uv = uv[:, :1] * tri[:, 0] + uv[:, 1:] * tri[:, 1] + (1 - uv.sum(1, keepdims=True)) * tri[:, 2]
        r = rays[~miss].astype(np.float64)
        p_ray = r[:, :3] + r[:, 3:] * t1.cpu().numpy()[~miss].astype(np.float64)[:, None]
        scale = max(1.0, float(np.abs(p_ray).max()))
        assert np.abs(p_uv - p_ray).max() <= 1e-5 * scale
        if name == "louvre":
            first = ~miss[:256]
            assert first.all() and (h["face"][:256, 1].cpu().numpy() == 1).all() and np.array_equal(p_uv[:256, 2], np.ones(256))
        ds.close()


# ---- 10: statistics ---------------------------------------------------------------------------------------------------------------
def test_statistics_and_the_cull(gpu):
    """With a small k the search is culled by the k-th hit, count_all only by tmax: fewer triangles on the louvre, whose forty
    quads lie behind each other.  The inequality only."""
    ds = make_scene("louvre", "sah")
    rays_d = dev(hc.louvre_rays(256))
    small = ds.hits(rays_d, 1, collect_stats=True)["stats"]
    every = ds.hits(rays_d, 1, count_all=True, collect_stats=True)["stats"]
    crossings = ds.hits(rays_d, 0, count_all=True, outputs=("n",), collect_stats=True)["stats"]
    uncut = ds.hits(rays_d, 1, collect_stats=True, traversal=abi.TRAVERSAL_EXHAUSTIVE)["stats"]
    plain = ds.hits(rays_d, 1, want_stats=True)["stats"]
    print({key: (small[key], every[key], uncut[key]) for key in ("boxes_tested", "triangles_tested")})
    for st in (small, every, crossings, uncut, plain):
        assert st["kernel_launches"] == 1 and st["kernel_ms"] > 0 and st["rays_primary"] == 256
        assert st["class_launches"][abi.KERNEL_OTHER] == 1 and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
    assert plain["boxes_tested"] == 0 and plain["triangles_tested"] == 0
    assert 0 < small["triangles_tested"] < every["triangles_tested"] <= uncut["triangles_tested"]
    assert small["boxes_tested"] < every["boxes_tested"] and every["triangles_tested"] == crossings["triangles_tested"]
    ds.close()
