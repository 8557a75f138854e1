"""rayca_hip_probe_lookup_device / DeviceScene.probe_lookup: the light at points in device memory from a grid of SH9 probes.

Expected values never come from the code under test.  They are the rays of tests/probes_literal.py (the header's text in numpy f32)
put through DeviceScene.query(kind="occluded", tmax=1.0), which test_gpu_query.py pins bit for bit on every kernel path, folded by
the literal.  Every comparison is of bits.  The inputs are tests/probes_cases.py's, which test_probes_cpu.py checks on the oracle:
neither answer is rare, and some points take the fallback.  Each scene is run three ways: RAYCA_BUILDER_REFERENCE, RAYCA_BUILDER_SAH
after finish() and RAYCA_BUILDER_SAH right after creation."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as ac
import oracle_lib as ol
import probes_cases as pc
import probes_literal as pl
import ray_edges as R
from rayca_amd import Config, DeviceScene, Scene, Trs, abi, flatten, lib, scenes
from rayca_amd.ambient import sphere_directions
from rayca_amd.lib import RaycaError
from rayca_amd.probes import ProbeGrid

pytestmark = pytest.mark.gpu
HOW = ["reference", "sah", "sah_unfinished"]
OUTPUTS = ("irradiance", "sh", "mask", "radiance")
FLAGS = [0, pl.VISIBILITY, pl.NORMAL_TERM, pl.VISIBILITY | pl.NORMAL_TERM]


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


def probe_grid(g):
    return ProbeGrid(g.origin, g.cell, g.dims)


def occlusion(ds, g, p, n, bias):
    """[N, 8] bool: what the occlusion query answers, tmax = 1, for the literal's ray of every corner of every active point
    (corners that are no candidates included: the literal's fold does not read them)"""
    import torch
    act = pl.active(p, n)
    _, c, _, _ = pl.corners(g, pl.cells(g, p))
    o, d = pl.rays(p, n, c, bias)
    r = np.concatenate([o, d], 2).reshape(-1, 6).copy()
    r[~np.repeat(act, 8)] = [0, 0, 0, 1, 0, 0]                    # (rows of inactive points: traced, never read)
    occ = ds.query(dev(r), kind="occluded", tmax=1.0)
    torch.cuda.synchronize()
    return occ.cpu().numpy().reshape(-1, 8) != 0


def shading(count, seed=801):
    """(albedo, base) [count, 4] f32, hashed"""
    return R._unit(seed, count, 4).astype(np.float32), (2.0 * R._unit(seed + 1, count, 4)).astype(np.float32)


def run(ds, p_d, n_d, g, sh_d, outputs=OUTPUTS, **kw):
    import torch
    got = ds.probe_lookup(p_d, n_d, probe_grid(g), sh_d, outputs=outputs, **kw)
    torch.cuda.synchronize()
    out = {k: got[k].cpu().numpy() for k in outputs}
    if "mask" in out:
        out["mask"] = out["mask"].view(np.uint32)
    if "stats" in got:
        out["stats"] = got["stats"]
    return out


def assert_same(got, want, what=""):
    for k in OUTPUTS:
        if k in got:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
            a, b = bits(got[k]).reshape(got[k].shape[0], -1), bits(want[k]).reshape(got[k].shape[0], -1)
            bad = np.flatnonzero((a != b).any(1))
            assert bad.size == 0, f"{what}: {bad.size} of {a.shape[0]} rows of {k} differ, first at {bad[:5]}: got {got[k][bad[:2]]}, want {want[k][bad[:2]]}"


def flag_args(flags):
    return dict(visibility=bool(flags & pl.VISIBILITY), normal_term=bool(flags & pl.NORMAL_TERM))


# ---- 1: four scenes, three builds, four flag combinations, with and without kept -------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", pc.SCENES)
def test_all_outputs_match_the_specification(gpu, name, how):
    ds = make_scene(R.scene_desc(name), how)
    if name == "spheres":
        assert ds.info()["sphere_count"] > 0
    inp = pc.inputs_for(name)
    p, n, g, sh, bias = inp["points"], inp["normals"], inp["grid"], inp["sh"], inp["bias"]
    act = pl.active(p, n)
    albedo, base = shading(inp["count"])
    p_d, n_d, sh_d, alb_d, base_d = dev(p), dev(n), dev(sh), dev(albedo), dev(base)
    occ = occlusion(ds, g, p, n, bias)
    for kept in (inp["kept"], None):
        kept_d = dev(kept.view(np.int32)) if kept is not None else None
        for flags in FLAGS:
            what = f"{name} {how} flags={flags} kept={'given' if kept is not None else 'NULL'}"
            want = pl.fold(occ, g, p, n, sh, kept, flags, albedo, base)
            got = run(ds, p_d, n_d, g, sh_d, kept=kept_d, bias=float(bias), albedo=alb_d, base=base_d, **flag_args(flags))
            assert_same(got, want, what)
            idx = np.flatnonzero(~act)
            assert idx.size == 5 and not got["irradiance"][idx].any() and not got["sh"][idx].any() and not got["mask"][idx].any()
            assert np.array_equal(got["radiance"][idx], base[idx])
            if flags == pl.VISIBILITY | pl.NORMAL_TERM and kept is not None:   # what the inputs are there for (test_probes_cpu.py)
                cand, occluded = got["mask"] & 0xFF, got["mask"] >> 8 & 0xFF
                frac = sum(bin(int(x)).count("1") for x in occluded) / sum(bin(int(x)).count("1") for x in cand)
                fb = int((got["mask"] >> 16 & 1).sum())
                assert 0.10 <= frac <= 0.90 and 1 <= fb < act.sum() / 2, (what, frac, fb)
            if not flags & pl.VISIBILITY:
                assert not (got["mask"] >> 8 & 0xFF).any()
    ds.close()


# ---- 2: without visibility the scene is not read -------------------------------------------------------------------------------------
def test_without_visibility_the_literal_alone_and_an_empty_scene(gpu):
    import torch
    inp = pc.inputs_for("cornell")
    p, n, g, sh, kept = inp["points"], inp["normals"], inp["grid"], inp["sh"], inp["kept"]
    albedo, _ = shading(inp["count"])
    nothing = Scene()
    nothing.push_model(scenes.create_default_model())              # a camera and lights, nothing to hit
    empty = DeviceScene(flatten(nothing), Config())
    full = make_scene(R.scene_desc("cornell"), "sah")
    assert empty.info()["triangle_count"] == 0 and empty.info()["sphere_count"] == 0
    for flags in (0, pl.NORMAL_TERM):
        want = pl.fold(None, g, p, n, sh, kept, flags, albedo)
        for ds in (empty, full):
            got = run(ds, dev(p), dev(n), g, dev(sh), kept=dev(kept.view(np.int32)), albedo=dev(albedo), want_stats=True, **flag_args(flags))
            assert_same(got, want, f"flags={flags}")
            assert got["stats"]["kernel_launches"] == 1 and got["stats"]["rays_shadow"] == 0
    with pytest.raises(RaycaError) as e:
        empty.probe_lookup(dev(p), dev(n), probe_grid(g), dev(sh))
    assert e.value.code == abi.ERR_EMPTY_SCENE
    torch.cuda.synchronize()
    empty.close()
    full.close()


# ---- 3: tiny batches, the empty batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_tiny_batches(gpu, how):
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    inp = pc.inputs_for(name)
    g, sh, kept, bias = inp["grid"], inp["sh"], inp["kept"], inp["bias"]
    p, n = inp["points"][200:], inp["normals"][200:]               # (point 233 is inactive)
    albedo, base = shading(65)
    occ = occlusion(ds, g, p[:65], n[:65], bias)
    for count in (1, 7, 8, 9, 63, 64, 65):
        want = pl.fold(occ[:count], g, p[:count], n[:count], sh, kept, pl.VISIBILITY | pl.NORMAL_TERM, albedo[:count], base[:count])
        got = run(ds, dev(p[:count]), dev(n[:count]), g, dev(sh), kept=dev(kept.view(np.int32)), bias=float(bias), albedo=dev(albedo[:count]),
                  base=dev(base[:count]))
        assert_same(got, want, f"{count} points")
    none = ds.probe_lookup(dev(p[:0]), dev(n[:0]), probe_grid(g), dev(sh), albedo=dev(albedo[:0]), outputs=OUTPUTS, want_stats=True)
    assert [tuple(none[k].shape) for k in OUTPUTS] == [(0, 4), (0, 9, 4), (0,), (0, 4)] and none["stats"]["kernel_launches"] == 0
    ds.close()


# ---- 4: grids with a single probe on an axis; an origin so far away that p - g overflows ---------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_degenerate_grids(gpu, how):
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    inp = pc.inputs_for(name)
    p, n, bias = inp["points"], inp["normals"], inp["bias"]
    cases = [(pc.grid_for(name, dims), p, n) for dims in pc.DEGENERATE_DIMS] + [pc.far_origin_grid()]
    for g, p, n in cases:
        sh, kept = pc.coefficients(g), None
        occ = occlusion(ds, g, p, n, bias)
        for flags in FLAGS:
            want = pl.fold(occ, g, p, n, sh, kept, flags)
            got = run(ds, dev(p), dev(n), g, dev(sh), outputs=OUTPUTS[:3], bias=float(bias), **flag_args(flags))
            assert_same(got, want, f"dims {g.dims} flags={flags}")
            alive = sum(1 << k for k in range(8) if all(d > 1 or not k >> a & 1 for a, d in enumerate(g.dims)))   # an axis of one probe: b = 0 alone
            assert not (got["mask"] & np.uint32(0xFF & ~alive)).any() and (got["mask"] & np.uint32(0xFF)).any()
    ds.close()


# ---- 5: output subsets and guard words; radiance with and without base ----------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_output_subsets_and_guards(gpu, how):
    import torch
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    inp = pc.inputs_for(name)
    count = inp["count"] - 4                                       # (599: no multiple of 8 or 64)
    p, n, g, sh, kept, bias = inp["points"][:count], inp["normals"][:count], inp["grid"], inp["sh"], inp["kept"], inp["bias"]
    albedo, base = shading(count)
    p_d, n_d, sh_d, kept_d, alb_d, base_d = dev(p), dev(n), dev(sh), dev(kept.view(np.int32)), dev(albedo), dev(base)
    occ = occlusion(ds, g, p, n, bias)
    flags = pl.VISIBILITY | pl.NORMAL_TERM
    want = {True: pl.fold(occ, g, p, n, sh, kept, flags, albedo, base), False: pl.fold(occ, g, p, n, sh, kept, flags, albedo, None)}
    assert not np.array_equal(want[True]["radiance"], want[False]["radiance"]) and (want[False]["radiance"][:, 3] == 1).all()
    shape = {"irradiance": (4,), "sh": (9, 4), "mask": (), "radiance": (4,)}
    sentinel = {"irradiance": -7.0, "sh": -7.0, "mask": 0x5A5A5A5A, "radiance": -7.0}
    big = {k: torch.full((count + 128, *shape[k]), sentinel[k], dtype=torch.int32 if k == "mask" else torch.float32, device="cuda") for k in OUTPUTS}

    def check(asked, with_base, what):
        for k in OUTPUTS:
            if k in asked:
                got = big[k][64:-64].cpu().numpy()
                assert_same({k: got.view(np.uint32) if k == "mask" else got}, want[with_base], what)
                assert bool((big[k][:64] == sentinel[k]).all()) and bool((big[k][-64:] == sentinel[k]).all()), (what, k, "guard words")
            else:
                assert bool((big[k] == sentinel[k]).all()), (what, k, "an output that was not asked for")
            big[k].fill_(sentinel[k])

    # through the wrapper: all four, each alone (the mask words live in the context's scratch unless "mask" is asked for), a pair
    for asked in (OUTPUTS, ("irradiance",), ("sh",), ("mask",), ("radiance",), ("irradiance", "radiance")):
        for with_base in (True, False):
            r = ds.probe_lookup(p_d, n_d, probe_grid(g), sh_d, kept=kept_d, bias=float(bias), albedo=alb_d, base=base_d if with_base else None,
                                outputs=asked, out={k: big[k][64:-64] for k in asked})
            torch.cuda.synchronize()
            assert all(r[k].data_ptr() == big[k][64:-64].data_ptr() for k in asked)
            check(asked, with_base, f"outputs={asked} base={with_base}")
    # through the C ABI: every subset of the four pointers
    for subset in range(1, 16):
        a = abi.RaycaProbeLookup()
        a.count, a.flags, a.bias = count, flags, float(bias)
        a.origin[:], a.cell[:], a.dims[:] = g.origin.tolist(), g.cell.tolist(), g.dims
        a.points, a.normals, a.sh, a.kept, a.albedo, a.base = (x.data_ptr() for x in (p_d, n_d, sh_d, kept_d, alb_d, base_d))
        asked = tuple(k for j, k in enumerate(OUTPUTS) if subset >> j & 1)
        for k in asked:
            setattr(a, k + "_out", big[k][64:-64].data_ptr())
        o = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
        st = abi.RaycaStats()
        lib.check(gpu.rayca_hip_probe_lookup_device(ds.handle, C.byref(o), C.byref(a), C.byref(st)))   # (no stream: the call waits)
        assert st.kernel_launches == 2 and st.rays_shadow == count * 8
        check(asked, True, f"subset {subset}")
    ds.close()


# ---- 6: repeatability, another stream and context ------------------------------------------------------------------------------------
def test_repeatable_and_on_other_streams_and_contexts(gpu):
    import torch
    name = "soup1k"
    ds = make_scene(R.scene_desc(name), "sah")
    inp = pc.inputs_for(name)
    p, n, g, sh, kept, bias = inp["points"], inp["normals"], inp["grid"], inp["sh"], inp["kept"], inp["bias"]
    albedo, base = shading(inp["count"])
    p_d, n_d, sh_d = dev(p), dev(n), dev(sh)
    kw = dict(kept=dev(kept.view(np.int32)), bias=float(bias), albedo=dev(albedo), base=dev(base))
    want = pl.fold(occlusion(ds, g, p, n, bias), g, p, n, sh, kept, pl.VISIBILITY | pl.NORMAL_TERM, albedo, base)
    first, second = run(ds, p_d, n_d, g, sh_d, **kw), run(ds, p_d, n_d, g, sh_d, **kw)
    assert_same(first, want, "first call")
    assert_same(second, want, "second call")
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    res = [ds.probe_lookup(p_d, n_d, probe_grid(g), sh_d, outputs=OUTPUTS, stream=s, context=k + 1, **kw) for k, s in enumerate(streams)]
    raw = ds.probe_lookup(p_d, n_d, probe_grid(g), sh_d, outputs=("radiance",), stream=streams[0].cuda_stream, context=7, **kw)   # (scratch mask words of context 7)
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        got = {name: r[name].cpu().numpy() for name in OUTPUTS}
        got["mask"] = got["mask"].view(np.uint32)
        assert_same(got, want, f"context {k + 1}")
    assert_same({"radiance": raw["radiance"].cpu().numpy()}, want, "context 7, a raw stream handle")
    with pytest.raises(RaycaError):
        ds.probe_lookup(p_d, n_d, probe_grid(g), sh_d, context=8, **kw)
    ds.close()


# ---- 7: a tree whose stack need exceeds the LDS part ------------------------------------------------------------------------------
def chain_scene() -> Scene:
    """test_gpu_ambient.py's chain, rebuilt: a soup, and twenty-nine soups a tenth of its size in and around it -- one TLAS leaf whose
    BLASes hang behind each other, a stack need of 28 entries and more: the entries beyond the LDS part of either trace kernel are used."""
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
        lo, hi = v.min(0), v.max(0)
        cell = (hi - lo) / (np.array(pc.DIMS) - 1)
        _CHAIN.update(desc=desc, points=ac.points_on(tris), diag=float(np.linalg.norm(hi - lo)),
                      grid=pl.Grid(lo.astype(np.float32), cell.astype(np.float32), pc.DIMS))
    return _CHAIN["desc"], _CHAIN["points"], _CHAIN["diag"], _CHAIN["grid"]


@pytest.mark.parametrize("how", HOW)
def test_tree_that_needs_the_spill_area(gpu, how):
    desc, (p, n), diag, g = chain_inputs()
    ds = make_scene(desc, how)
    depth = ds.info()["max_depth"]
    print(f"chain scene, {how}: stack need {depth}")
    assert depth + 1 > 24, "the scene must need more stack entries than either trace kernel keeps in LDS"
    sh, bias = pc.coefficients(g), np.float32(1e-4 * diag)
    occ = occlusion(ds, g, p, n, bias)
    want = pl.fold(occ, g, p, n, sh, None, pl.VISIBILITY | pl.NORMAL_TERM)
    got = run(ds, dev(p), dev(n), g, dev(sh), outputs=OUTPUTS[:3], bias=float(bias))
    assert_same(got, want, f"chain {how}")
    occluded = got["mask"] >> 8 & 0xFF
    assert occluded.any() and (occluded != (got["mask"] & 0xFF)).any()
    ds.close()


# ---- 8: statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_statistics(gpu, how):
    """rays_shadow = count x 8 with visibility and 0 without, the time under RAYCA_KERNEL_OTHER, kernel_launches = the kernels
    launched; under collect_stats the boxes and triangles the candidate rays cost."""
    name = "cornell"
    ds = make_scene(R.scene_desc(name), how)
    inp = pc.inputs_for(name)
    p, n, g, sh = inp["points"], inp["normals"], inp["grid"], inp["sh"]
    count = inp["count"]
    kw = dict(bias=float(inp["bias"]))
    plain = ds.probe_lookup(dev(p), dev(n), probe_grid(g), dev(sh), want_stats=True, **kw)["stats"]
    counted = ds.probe_lookup(dev(p), dev(n), probe_grid(g), dev(sh), collect_stats=True, **kw)["stats"]
    fold_only = ds.probe_lookup(dev(p), dev(n), probe_grid(g), dev(sh), visibility=False, collect_stats=True, **kw)["stats"]
    for st, launches, rays in ((plain, 2, count * 8), (counted, 2, count * 8), (fold_only, 1, 0)):
        assert st["rays_shadow"] == rays and st["rays_primary"] == 0
        assert st["kernel_launches"] == launches and st["kernel_ms"] > 0
        assert st["class_launches"][abi.KERNEL_OTHER] == launches and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
    assert plain["boxes_tested"] == 0 and plain["triangles_tested"] == 0 and fold_only["boxes_tested"] == 0
    assert counted["boxes_tested"] > 0 and counted["triangles_tested"] > 0
    if how == "sah":
        assert counted["node_format"] & 2048 == 0 and counted["node_format"] & 1, "a finished SAH scene runs the lane-refill form on the 4-wide nodes"
    else:
        assert counted["node_format"] & 1 == 0
    ds.close()


# ---- 9: the wrappers -------------------------------------------------------------------------------------------------------------------
def test_bake_is_the_gather_it_stands_for(gpu):
    import torch
    ds = make_scene(R.scene_desc("cornell"), "sah")
    cfg = Config(max_depth=1)
    grid = ProbeGrid.around([-1, 0, -1], [1, 2, 1], (3, 3, 2), margin=-0.25)
    sh, kept = grid.bake(ds, cfg, samples=16, sample=3)
    p = dev(grid.positions())
    n = torch.zeros_like(p)
    n[:, 2] = 1.0
    want = ds.gather(p, n, cfg, samples=16, dirs=dev(sphere_directions(16)), weights=dev(np.full(16, 4.0 * np.pi, np.float32)), sample=3,
                     outputs=("sh", "kept"))
    torch.cuda.synchronize()
    assert sh.shape == (18, 9, 4) and sh.dtype == torch.float32 and kept.shape == (18,) and kept.dtype == torch.int32
    assert np.array_equal(bits(sh.cpu().numpy()), bits(want["sh"].cpu().numpy())) and np.array_equal(kept.cpu().numpy(), want["kept"].cpu().numpy())
    assert bool((kept > 0).all()) and float(sh[:, 0, :3].min()) > 0, "every probe of a lit room receives light"
    # the lookup takes them as they are
    out = ds.probe_lookup(p[:4] + 0.01, n[:4], grid, sh, kept=kept, bias=1e-3)
    torch.cuda.synchronize()
    assert float(out["irradiance"][:, :3].min()) > 0
    ds.close()


def test_render_probe_lit_is_gbuffer_then_probe_lookup(gpu):
    import torch
    ds = make_scene(R.scene_desc("cornell"), "sah")
    cfg, w, h = Config(), 64, 36
    g = pc.grid_for("cornell")
    grid, sh, kept = probe_grid(g), dev(pc.coefficients(g)), dev(pc.kept(g).view(np.int32))
    base = dev((2.0 * R._unit(811, h * w, 4)).astype(np.float32).reshape(h, w, 4))
    for b in (None, base):
        img = ds.render_probe_lit(w, h, grid, sh, config=cfg, kept=kept, bias=1e-3, base=b)
        gb = ds.gbuffer(cfg, w, h, want=("point", "normal", "color"))
        r = ds.probe_lookup(gb["point"].reshape(-1, 3), gb["normal"].reshape(-1, 3), grid, sh, kept=kept, bias=1e-3, albedo=gb["color"].reshape(-1, 4),
                            base=b.reshape(-1, 4) if b is not None else None, outputs=("radiance", "mask"))
        torch.cuda.synchronize()
        assert img.shape == (h, w, 4) and img.dtype == torch.float32
        assert np.array_equal(bits(img.cpu().numpy()), bits(r["radiance"].reshape(h, w, 4).cpu().numpy()))
        miss = (gb["prim"] == -1).cpu().numpy()
        assert 0 < miss.sum() < miss.size and not r["mask"].reshape(h, w).cpu().numpy()[miss].any()
        want_miss = base.cpu().numpy()[miss] if b is not None else np.tile(np.float32([0, 0, 0, 1]), (miss.sum(), 1))
        assert np.array_equal(img.cpu().numpy()[miss], want_miss)
        assert img.cpu().numpy()[~miss][:, :3].max() > 0
    # against the specification on the same G-buffer
    p, n, alb = (gb[k].reshape(-1, gb[k].shape[-1]).cpu().numpy() for k in ("point", "normal", "color"))
    want = pl.fold(occlusion(ds, g, p, n, np.float32(1e-3)), g, p, n, pc.coefficients(g), pc.kept(g), pl.VISIBILITY | pl.NORMAL_TERM, alb, base.reshape(-1, 4).cpu().numpy())
    assert_same({"radiance": img.reshape(-1, 4).cpu().numpy(), "mask": r["mask"].cpu().numpy().view(np.uint32)}, want, "render_probe_lit")
    ds.close()


def test_wrapper_checks(gpu):
    import torch
    ds = make_scene(R.scene_desc("box"), "sah")
    grid = ProbeGrid([0, 0, 0], [1, 1, 1], (2, 2, 2))
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    n = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    n[:, 2] = 1.0
    sh = torch.ones((8, 9, 4), dtype=torch.float32, device="cuda")
    alb = torch.ones((64, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ds.probe_lookup(p.cpu(), n, grid, sh)
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n.cpu(), grid, sh)
    with pytest.raises(TypeError):
        ds.probe_lookup(p.double(), n, grid, sh)
    with pytest.raises(TypeError):
        ds.probe_lookup(np.zeros((64, 3), np.float32), n, grid, sh)
    with pytest.raises(ValueError):
        ds.probe_lookup(p.reshape(-1, 6), n, grid, sh)
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n[:63], grid, sh)
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n, grid, sh[:7])
    with pytest.raises(TypeError):
        ds.probe_lookup(p, n, grid, sh, kept=torch.ones(8, device="cuda"))
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n, grid, sh, kept=torch.ones(9, device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n, grid, sh, outputs=("irradiance", "shadow"))
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n, grid, sh, outputs=())
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n, grid, sh, outputs=("radiance",))
    with pytest.raises(ValueError):
        ds.probe_lookup(p, n, grid, sh, outputs=("radiance",), albedo=alb[:63])
    with pytest.raises(TypeError):
        ds.probe_lookup(p, n, grid, sh, outputs=("mask",), out={"mask": torch.zeros(64, device="cuda", dtype=torch.int64)})
    with pytest.raises(ValueError):
        ds.render_probe_lit(8, 8, grid, sh, albedo="specular")
    with pytest.raises(RaycaError) as e:
        ds.probe_lookup(p, n, grid, sh, bias=float("nan"))
    assert e.value.code == abi.ERR_BAD_ARG and "bias" in str(e.value)
    # a strided input is made contiguous; constant probes give a constant answer
    wide = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = 0.5
    a = ds.probe_lookup(wide[:, :3], n, grid, sh, visibility=False, normal_term=False, outputs=("sh", "irradiance"))
    torch.cuda.synchronize()
    assert (a["sh"][:, :, :3].cpu().numpy() == 1.0).all() and (a["irradiance"][:, 3].cpu().numpy() == 1.0).all()
    ds.close()
