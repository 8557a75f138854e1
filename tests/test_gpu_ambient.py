"""rayca_hip_ambient_device / DeviceScene.ambient: hemisphere visibility at points in device memory.

Expected values never come from the code under test.  They are the rays of tests/ambient_literal.py (the header's text in numpy
f32) put through DeviceScene.query(kind="occluded", tmax=radius), which test_gpu_query.py pins bit for bit on every kernel path,
folded by the literal.  Every comparison is of bits: the mask words, hits, and open / bent by their bit patterns.  The inputs are
tests/ambient_cases.py's, which test_ambient_cpu.py checks on the oracle: neither answer is rare.  Each scene is run three ways:
RAYCA_BUILDER_REFERENCE, RAYCA_BUILDER_SAH after finish() and RAYCA_BUILDER_SAH right after creation."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as ac
import ambient_literal as al
import oracle_lib as ol
import ray_edges as R
from rayca_amd import Config, DeviceScene, Scene, Trs, abi, flatten, lib, scenes
from rayca_amd.ambient import cosine_directions, pixel_rotations
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
HOW = ["reference", "sah", "sah_unfinished"]
WANT = ("mask", "hits", "open", "bent")
FLT_MAX = float(ac.FLT_MAX)


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


_RAYS = {}


def literal_rays(key, p, n, rot, table, samples, bias, dir_first=0):
    """the literal's (o, d), once per input set"""
    if key not in _RAYS:
        _RAYS[key] = al.rays(p, n, rot, table, samples, bias, dir_first)
    return _RAYS[key]


def expected(ds, key, p, n, rot, table, samples, bias, radius, dir_first=0):
    """(mask, hits, open, bent) as the specification has them: the literal's rays through the occlusion query, the literal's fold.
    radius: None, a float, or a per-point f32 array."""
    import torch
    act = al.active(p, n)
    o, d = literal_rays(key, p, n, rot, table, samples, bias, dir_first)
    count = p.shape[0]
    r = np.concatenate([o, d], 2).reshape(-1, 6).copy()
    r[~np.repeat(act, samples)] = [0, 0, 0, 1, 0, 0]          # (rows of inactive points: traced, never read)
    tmax = dev(np.repeat(radius, samples)) if isinstance(radius, np.ndarray) else radius
    occ = ds.query(dev(r), kind="occluded", tmax=tmax)
    torch.cuda.synchronize()
    occ = occ.cpu().numpy().reshape(count, samples) != 0
    return al.fold(occ, act, d, samples), occ & act[:, None], act


def run(ds, p_d, n_d, want=WANT, **kw):
    import torch
    got = ds.ambient(p_d, n_d, want=want, **kw)
    torch.cuda.synchronize()
    out = {}
    for k in want:
        v = got[k].cpu().numpy()
        out[k] = v.view(np.uint64) if k == "mask" else (v.view(np.uint32) if k == "hits" else v)
    if "stats" in got:
        out["stats"] = got["stats"]
    return out


def assert_same(got, want, what=""):
    mask, hits, opened, bent = want
    if "mask" in got:
        bad = np.flatnonzero(got["mask"] != mask)
        assert bad.size == 0, f"{what}: {bad.size} of {mask.size} masks differ, first at {bad[:5]}: got {[hex(int(x)) for x in got['mask'][bad[:5]]]}, want {[hex(int(x)) for x in mask[bad[:5]]]}"
    if "hits" in got:
        assert np.array_equal(got["hits"], hits), f"{what}: hits differ at {np.flatnonzero(got['hits'] != hits)[:5]}"
    if "open" in got:
        assert got["open"].dtype == np.float32 and np.array_equal(bits(got["open"]), bits(opened)), f"{what}: open differs at {np.flatnonzero(bits(got['open']) != bits(opened))[:5]}"
    if "bent" in got:
        bad = np.flatnonzero((bits(got["bent"]) != bits(bent)).any(axis=1))
        assert got["bent"].shape == bent.shape and bad.size == 0, f"{what}: {bad.size} bent sums differ, first at {bad[:5]}: got {got['bent'][bad[:3]]}, want {bent[bad[:3]]}"


def radius_arg(radius):
    return dev(radius) if isinstance(radius, np.ndarray) else (None if radius is None else float(radius))


# ---- 1: four scenes, three builds, four sample counts, rotations, both kinds of radius ---------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", ac.SCENES)
def test_all_outputs_match_the_specification(gpu, name, how):
    desc = R.scene_desc(name)
    ds = make_scene(desc, how)
    if name == "spheres":
        assert ds.info()["sphere_count"] > 0
    p, n, diag = ac.points_for(name)
    p_d, n_d = dev(p), dev(n)
    rot = ac.rotations()
    rot_d = dev(rot)
    table = ac.table(64)
    table_d = dev(table)
    bias = ac.bias(name)
    for samples in (1, 5, 16, 64):
        for rotated in (False, True):
            for what, radius in (("radius_all", ac.radius_all(name)), ("per point", ac.radius_per_point(name))):
                key = (name, samples, rotated)
                want, occ, act = expected(ds, key, p, n, rot if rotated else None, table, samples, bias, radius)
                got = run(ds, p_d, n_d, samples=samples, radius=radius_arg(radius), bias=float(bias), dirs=table_d, rotations=rot_d if rotated else None)
                assert_same(got, want, f"{name} {how} S={samples} rotated={rotated} {what}")
                if samples == 16:   # what the inputs are there for (test_ambient_cpu.py test_inputs_leave_both_answers)
                    assert 0.10 <= occ[act].mean() <= 0.90, (name, what, occ[act].mean())
                # inactive points: mask 0, hits 0, open 1, bent 0 -- and a dead radius leaves every sample unoccluded
                idx = ac.inactive_index()
                assert not got["mask"][idx].any() and not got["hits"][idx].any() and (got["open"][idx] == 1.0).all() and not got["bent"][idx].any()
                if what == "per point":
                    dead = ~(radius > 0)
                    assert dead.sum() > 50 and not got["mask"][dead].any() and (got["open"][dead] == 1.0).all()
    ds.close()


# ---- 2: tiny batches, the empty batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_tiny_batches(gpu, how):
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    p, n, _ = ac.points_for(name)
    table = ac.table(64)
    for count, samples in ((1, 1), (3, 5), (13, 5), (64, 1), (65, 1)):
        want, _, _ = expected(ds, (name, "tiny", count, samples), p[:count], n[:count], None, table, samples, ac.bias(name), ac.radius_all(name))
        got = run(ds, dev(p[:count]), dev(n[:count]), samples=samples, radius=float(ac.radius_all(name)), bias=float(ac.bias(name)), dirs=dev(table))
        assert_same(got, want, f"{count} points x {samples}")
    empty = ds.ambient(dev(p[:0]), dev(n[:0]), want=WANT, want_stats=True)
    assert [tuple(empty[k].shape) for k in WANT] == [(0,), (0,), (0,), (0, 3)] and empty["stats"]["kernel_launches"] == 0
    ds.close()


# ---- 3: the special radii, for every point at once ---------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_special_radii(gpu, how):
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    p, n, _ = ac.points_for(name)
    p_d, n_d, table = dev(p), dev(n), ac.table(64)
    free, occ, act = expected(ds, (name, 16, False), p, n, None, table, 16, ac.bias(name), None)
    assert 0.10 <= occ[act].mean() <= 0.90
    for radius in (float("inf"), FLT_MAX, None):
        assert_same(run(ds, p_d, n_d, samples=16, radius=radius, bias=float(ac.bias(name)), dirs=dev(table)), free, f"radius {radius}")
    for radius in (float("nan"), 0.0, -0.0, -1.5, float("-inf")):
        got = run(ds, p_d, n_d, samples=16, radius=radius, bias=float(ac.bias(name)), dirs=dev(table))
        want, _, _ = expected(ds, (name, 16, False), p, n, None, table, 16, ac.bias(name), np.float32(radius))
        assert_same(got, want, f"radius {radius}")
        assert not got["mask"].any() and (got["open"] == 1.0).all()
    ds.close()


# ---- 4: dir_first -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_dir_first_splits_a_sample_set(gpu, how):
    name = "soup1k"
    ds = make_scene(R.scene_desc(name), how)
    p, n, _ = ac.points_for(name)
    p_d, n_d, table = dev(p), dev(n), ac.table(16)
    table_d, rot = dev(table), ac.rotations()
    kw = dict(radius=float(ac.radius_all(name)), bias=float(ac.bias(name)), dirs=table_d, rotations=dev(rot))
    whole = run(ds, p_d, n_d, samples=16, **kw)
    m0 = run(ds, p_d, n_d, samples=8, dir_first=0, **kw)
    m1 = run(ds, p_d, n_d, samples=8, dir_first=8, **kw)
    assert np.array_equal(m0["mask"] | (m1["mask"] << np.uint64(8)), whole["mask"]) and whole["mask"].any()
    assert np.array_equal(m0["hits"] + m1["hits"], whole["hits"])
    want, _, _ = expected(ds, (name, "first8"), p, n, rot, table, 8, ac.bias(name), ac.radius_all(name), dir_first=8)
    assert_same(m1, want, "dir_first 8")
    ds.close()


# ---- 5: output subsets and guard words -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_output_subsets_and_guards(gpu, how):
    import torch
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    p, n, _ = ac.points_for(name)
    count = ac.COUNT - 5                                                   # (not a multiple of 64)
    p, n = p[:count], n[:count]
    p_d, n_d, table = dev(p), dev(n), ac.table(16)
    table_d, rot = dev(table), ac.rotations(count)
    rot_d = dev(rot)
    radius, bias = float(ac.radius_all(name)), float(ac.bias(name))
    want, _, _ = expected(ds, (name, "guards"), p, n, rot, table, 16, ac.bias(name), ac.radius_all(name))
    by_name = dict(zip(WANT, want))
    sentinel = {"mask": 0x5A5A5A5A5A5A5A5A, "hits": 0x5A5A5A5A, "open": -7.0, "bent": -7.0}
    big = {"mask": torch.full((count + 128,), sentinel["mask"], dtype=torch.int64, device="cuda"), "hits": torch.full((count + 128,), sentinel["hits"], dtype=torch.int32, device="cuda"),
           "open": torch.full((count + 128,), -7.0, dtype=torch.float32, device="cuda"), "bent": torch.full((count + 128, 3), -7.0, dtype=torch.float32, device="cuda")}

    def check(asked, what):
        for k in WANT:
            if k in asked:
                got = big[k][64:-64].cpu().numpy()
                got = got.view(np.uint64) if k == "mask" else (got.view(np.uint32) if k == "hits" else got)
                assert_same({k: got}, want, what)
                assert bool((big[k][:64] == sentinel[k]).all()) and bool((big[k][-64:] == sentinel[k]).all()), (what, k, "guard words")
            else:
                assert bool((big[k] == sentinel[k]).all()), (what, k, "an output that was not asked for")
            big[k].fill_(sentinel[k])

    # through the wrapper: all four, each alone (bent alone: the mask words live in the context's scratch), a pair
    for asked in (WANT, ("mask",), ("hits",), ("open",), ("bent",), ("open", "bent")):
        r = ds.ambient(p_d, n_d, samples=16, radius=radius, bias=bias, dirs=table_d, rotations=rot_d, want=asked, out={k: big[k][64:-64] for k in asked})
        torch.cuda.synchronize()
        assert all(r[k].data_ptr() == big[k][64:-64].data_ptr() for k in asked)
        check(asked, f"want={asked}")
    # through the C ABI: every subset of the four pointers
    for subset in range(1, 16):
        a = abi.RaycaAmbient()
        a.count, a.samples, a.dir_count, a.radius_all, a.bias = count, 16, 16, radius, bias
        a.points, a.normals, a.dirs, a.rotations = p_d.data_ptr(), n_d.data_ptr(), table_d.data_ptr(), rot_d.data_ptr()
        asked = tuple(k for j, k in enumerate(WANT) if subset >> j & 1)
        for k in asked:
            setattr(a, k + "_out", big[k][64:-64].data_ptr())
        o = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
        st = abi.RaycaStats()
        lib.check(gpu.rayca_hip_ambient_device(ds.handle, C.byref(o), C.byref(a), C.byref(st)))   # (no stream: the call waits)
        assert st.kernel_launches == (1 if asked == ("mask",) else 2) and st.rays_shadow == count * 16
        check(asked, f"subset {subset}")
    assert by_name["hits"].sum() > 0
    ds.close()


# ---- 6: repeatability, another stream and context ------------------------------------------------------------------------------------
def test_repeatable_and_on_other_streams_and_contexts(gpu):
    import torch
    name = "soup1k"
    ds = make_scene(R.scene_desc(name), "sah")
    p, n, _ = ac.points_for(name)
    p_d, n_d, table = dev(p), dev(n), ac.table(64)
    rot = ac.rotations()
    kw = dict(samples=64, radius=dev(ac.radius_per_point(name)), bias=float(ac.bias(name)), dirs=dev(table), rotations=dev(rot))
    want, _, _ = expected(ds, (name, 64, True), p, n, rot, table, 64, ac.bias(name), ac.radius_per_point(name))
    first, second = run(ds, p_d, n_d, **kw), run(ds, p_d, n_d, **kw)
    assert_same(first, want, "first call")
    assert_same(second, want, "second call")
    assert all(np.array_equal(bits(first[k]) if k != "mask" else first[k], bits(second[k]) if k != "mask" else second[k]) for k in WANT)
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    res = [ds.ambient(p_d, n_d, want=WANT, stream=s, context=k + 1, **kw) for k, s in enumerate(streams)]
    raw = ds.ambient(p_d, n_d, want=("bent",), stream=streams[0].cuda_stream, context=7, **kw)      # (scratch mask words of context 7)
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        got = {"mask": r["mask"].cpu().numpy().view(np.uint64), "hits": r["hits"].cpu().numpy().view(np.uint32), "open": r["open"].cpu().numpy(), "bent": r["bent"].cpu().numpy()}
        assert_same(got, want, f"context {k + 1}")
    assert_same({"bent": raw["bent"].cpu().numpy()}, want, "context 7, a raw stream handle")
    with pytest.raises(RaycaError):
        ds.ambient(p_d, n_d, context=8, **kw)
    ds.close()


# ---- 7: a tree whose stack need exceeds the LDS part ------------------------------------------------------------------------------
def chain_scene() -> Scene:
    """test_gpu_nearest.py's chain: a soup, and twenty-nine soups a tenth of its size in and around it -- one TLAS leaf whose BLASes
    hang behind each other, a stack need of 28 entries and more: the entries beyond the LDS part of either trace kernel are used."""
    scene = scenes.soup_scene(24, seed=0xC4A10, extent=0.2)
    for k in range(1, 30):
        other = scenes.soup_scene(24, seed=0xC4A10 + k, extent=0.2)
        m = scene.push_model(other.models[0])
        scene.nodes[m].trs = Trs(translation=(0.45 * (k % 6) - 0.9, 0.45 * ((k // 6) % 3) - 0.4, 0.45 * (k // 18)), scale=(0.1, 0.1, 0.1))
    return scene


_CHAIN = {}


def chain_inputs():
    if not _CHAIN:
        desc = flatten(chain_scene())
        orc = ol.OracleScene(desc, Config())
        tris = orc.world_triangles(orc.primitive_count).astype(np.float64).reshape(-1, 3, 3)
        orc.close()
        tris = tris[np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1) > 0]
        v = tris.reshape(-1, 3)
        _CHAIN.update(desc=desc, points=ac.points_on(tris), diag=float(np.linalg.norm(v.max(0) - v.min(0))))
    return _CHAIN["desc"], _CHAIN["points"], _CHAIN["diag"]


@pytest.mark.parametrize("how", HOW)
def test_tree_that_needs_the_spill_area(gpu, how):
    desc, (p, n), diag = chain_inputs()
    ds = make_scene(desc, how)
    depth = ds.info()["max_depth"]
    print(f"chain scene, {how}: stack need {depth}")
    assert depth + 1 > 24, "the scene must need more stack entries than either trace kernel keeps in LDS"
    table, rot = ac.table(16), ac.rotations()
    bias = np.float32(1e-4 * diag)
    for what, radius in (("unbounded", None), ("half a diagonal", np.float32(0.5 * diag))):
        want, occ, act = expected(ds, ("chain", what), p, n, rot, table, 16, bias, radius)
        got = run(ds, dev(p), dev(n), samples=16, radius=radius_arg(radius), bias=float(bias), dirs=dev(table), rotations=dev(rot))
        assert_same(got, want, f"chain {how} {what}")
        assert occ.any() and not occ[act].all()
    ds.close()


# ---- 8: statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_statistics(gpu, how):
    """rays_shadow = count x S, the time under RAYCA_KERNEL_OTHER, kernel_launches = the kernels launched; under collect_stats the
    boxes and triangles the rays cost -- the same traversal as the occlusion query's on the same rays, so the same counts."""
    import torch
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    p, n, _ = ac.points_for(name)
    act = al.active(p, n)
    p, n = p[act], n[act]                                                   # (the query below has no notion of an inactive point)
    count, samples = p.shape[0], 16
    p_d, n_d, table = dev(p), dev(n), ac.table(16)
    radius = ac.radius_per_point(name)[act]
    kw = dict(samples=samples, radius=dev(radius), bias=float(ac.bias(name)), dirs=dev(table))
    plain = ds.ambient(p_d, n_d, want=WANT, want_stats=True, **kw)["stats"]
    only_mask = ds.ambient(p_d, n_d, want=("mask",), want_stats=True, **kw)["stats"]
    counted = ds.ambient(p_d, n_d, want=("open",), collect_stats=True, **kw)["stats"]
    for st, launches in ((plain, 2), (only_mask, 1), (counted, 2)):
        assert st["rays_shadow"] == count * samples and st["rays_primary"] == 0
        assert st["kernel_launches"] == launches and st["kernel_ms"] > 0
        assert st["class_launches"][abi.KERNEL_OTHER] == launches and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
    assert plain["boxes_tested"] == 0 and plain["triangles_tested"] == 0
    o, d = al.rays(p, n, None, table, samples, ac.bias(name))
    _, qst = ds.query(dev(np.concatenate([o, d], 2).reshape(-1, 6)), kind="occluded", tmax=dev(np.repeat(radius, samples)), collect_stats=True)
    torch.cuda.synchronize()
    print({k: (counted[k], qst[k]) for k in ("boxes_tested", "triangles_tested")})
    assert counted["boxes_tested"] == qst["boxes_tested"] > 0 and counted["triangles_tested"] == qst["triangles_tested"] > 0
    assert counted["node_format"] == qst["node_format"], "the trace kernel is chosen by the query's rule: the same nodes"
    if how == "sah":
        assert counted["node_format"] & 2048 == 0 and counted["node_format"] & 1, "a finished SAH scene runs the lane-refill form on the 4-wide nodes"
    ds.close()


# ---- 9: the wrappers -------------------------------------------------------------------------------------------------------------------
def test_render_ambient_is_gbuffer_then_ambient(gpu):
    import torch
    ds = make_scene(R.scene_desc("cornell"), "sah")
    cfg, w, h = Config(), 64, 36
    img = ds.render_ambient(cfg, w, h, samples=16, radius=1.0, bias=1e-3)
    g = ds.gbuffer(cfg, w, h, want=("point", "normal"))
    rot = torch.from_numpy(pixel_rotations(w, h).reshape(-1, 2)).cuda()
    a = ds.ambient(g["point"].reshape(-1, 3), g["normal"].reshape(-1, 3), samples=16, radius=1.0, bias=1e-3, rotations=rot, want=("open", "mask"))
    torch.cuda.synchronize()
    assert img.shape == (h, w) and img.dtype == torch.float32
    assert np.array_equal(bits(img.cpu().numpy()), bits(a["open"].reshape(h, w).cpu().numpy()))
    miss = (g["prim"] == -1).cpu().numpy()
    assert 0 < miss.sum() < miss.size and (img.cpu().numpy()[miss] == 1.0).all() and not a["mask"].reshape(h, w).cpu().numpy()[miss].any()
    inside = img.cpu().numpy()[~miss]
    assert 0.0 < inside.mean() < 1.0 and inside.min() < 0.7, "a room's corners are not open"
    # the default table is cosine_directions(samples); against the specification on the same G-buffer
    p, n = g["point"].reshape(-1, 3).cpu().numpy(), g["normal"].reshape(-1, 3).cpu().numpy()
    want, _, _ = expected(ds, ("render", w, h), p, n, rot.cpu().numpy(), cosine_directions(16), 16, np.float32(1e-3), np.float32(1.0))
    assert np.array_equal(bits(a["open"].cpu().numpy()), bits(want[2])) and np.array_equal(a["mask"].cpu().numpy().view(np.uint64), want[0])
    ds.close()


def test_wrapper_checks(gpu):
    import torch
    ds = make_scene(R.scene_desc("box"), "sah")
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    n = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    n[:, 2] = 1.0
    with pytest.raises(ValueError):
        ds.ambient(p.cpu(), n)
    with pytest.raises(ValueError):
        ds.ambient(p, n.cpu())
    with pytest.raises(TypeError):
        ds.ambient(p.double(), n)
    with pytest.raises(TypeError):
        ds.ambient(np.zeros((64, 3), np.float32), n)
    with pytest.raises(ValueError):
        ds.ambient(p.reshape(-1, 6), n)
    with pytest.raises(ValueError):
        ds.ambient(p, n[:63])
    with pytest.raises(ValueError):
        ds.ambient(p, n, samples=65)
    with pytest.raises(ValueError):
        ds.ambient(p, n, samples=0)
    with pytest.raises(ValueError):
        ds.ambient(p, n, samples=16, dirs=torch.zeros((16, 3), device="cuda"), dir_first=1)
    with pytest.raises(ValueError):
        ds.ambient(p, n, radius=torch.ones(65, device="cuda"))
    with pytest.raises(TypeError):
        ds.ambient(p, n, rotations=torch.ones((64, 2), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ds.ambient(p, n, want=("open", "shadow"))
    with pytest.raises(ValueError):
        ds.ambient(p, n, want=())
    with pytest.raises(TypeError):
        ds.ambient(p, n, want=("mask",), out={"mask": torch.zeros(64, device="cuda", dtype=torch.int32)})
    with pytest.raises(RaycaError) as e:
        ds.ambient(p, n, bias=float("nan"))
    assert e.value.code == abi.ERR_BAD_ARG and "bias" in str(e.value)
    # a strided input is made contiguous; every sample of a box seen from outside its top face is unoccluded
    wide = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    wide[:, 2] = 0.75
    a = ds.ambient(wide[:, :3], n, want=("hits", "open"))
    torch.cuda.synchronize()
    assert not a["hits"].cpu().numpy().any() and (a["open"].cpu().numpy() == 1.0).all()
    ds.close()
