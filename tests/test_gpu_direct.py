"""rayca_hip_direct_device / DeviceScene.direct: the direct light of the scene's point and quad lights at points in device memory.

Expected values never come from the code under test.  They are the samples of tests/direct_literal.py (the header's text in numpy
f32) made from DeviceScene.lights() records (which one test pins to the authored dicts of tests/direct_cases.py), put through
DeviceScene.query(kind="occluded", tmax=dist) for a point light and query(kind="closest") + surface() flags for a quad light --
both pinned bit for bit by their own tests -- and folded by the literal.  Every comparison of an output is of bits."""
import ctypes as C

import numpy as np
import pytest

import direct_cases as dc
import direct_literal as dl
from rayca_amd import Config, DeviceScene, abi, lib
from rayca_amd.lib import RaycaError
from rayca_amd.probes import ProbeGrid

pytestmark = pytest.mark.gpu
HOW = ["reference", "sah", "sah_unfinished"]
OUT_HEMI = ("irradiance", "mask", "counts")
OUT_SPHERE = ("irradiance", "sh", "mask", "counts")
# light_samples, stratify per scene: N = lights x light_samples is 2, 64, 3 and 8
SAMPLING = {"points": (1, False), "quad": (64, True), "qpq": (1, False), "dim": (4, True)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_scene(name, how):
    ds = DeviceScene(dc.scene_desc(name), Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    if how == "sah":
        ds.finish()
    return ds


def config(name, seed=11):
    ls, strat = SAMPLING[name]
    return Config(light_samples=ls, light_stratify=strat, seed=seed, max_depth=1)


def literal_samples(ds, cfg, p, n, **kw):
    return dl.samples(ds.lights(), p, n, light_samples=cfg.light_samples, stratify=cfg.light_stratify, seed=cfg.seed, **kw)


def visibility(ds, s):
    """[P, N] bool: what the two queries answer for the literal's ray of every traced sample"""
    import torch
    P, N = s["tmax"].shape
    rays = np.concatenate([s["o"], s["omega"]], 2).reshape(-1, 6).copy()
    traced = s["traced"].reshape(-1)
    rays[~traced] = [0, 0, 0, 1, 0, 0]                            # (never read below)
    tmax = s["tmax"].reshape(-1).copy()
    tmax[~traced] = 1.0
    quad = np.tile(s["quad"], P)
    rays_d = dev(rays)
    occ = ds.query(rays_d, kind="occluded", tmax=dev(np.where(quad, np.float32(1.0), tmax).astype(np.float32)))
    t, prim, uv = ds.query(rays_d)
    flags = ds.surface(None, t, prim, uv, want=("flags",))["flags"]
    torch.cuda.synchronize()
    emissive = (flags.cpu().numpy().view(np.uint32) & 4) != 0     # (a miss has flags 0)
    lit = np.where(quad, emissive, occ.cpu().numpy() == 0)
    return lit.reshape(P, N)


def expected(ds, cfg, p, n, sh=False, **kw):
    s = literal_samples(ds, cfg, p, n, **kw)
    return dl.fold(s, visibility(ds, s), sh=sh), s


def run(ds, cfg, p, n, want, **kw):
    import torch
    got = ds.direct(dev(p), dev(n) if n is not None else None, cfg, want=want, **kw)
    torch.cuda.synchronize()
    out = {k: got[k].cpu().numpy() for k in want}
    if "mask" in out:
        out["mask"] = out["mask"].view(np.uint64)
    if "counts" in out:
        out["counts"] = out["counts"].view(np.uint32)
    if "stats" in got:
        out["stats"] = got["stats"]
    return out


def assert_same(got, want, what=""):
    for k in OUT_SPHERE:
        if k in got:
            g = got[k][:, 0] if k == "mask" and got[k].ndim == 2 else got[k]
            assert g.shape == want[k].shape and g.dtype == want[k].dtype, (what, k, g.shape, g.dtype, want[k].shape, want[k].dtype)
            a, b = bits(g).reshape(g.shape[0], -1), bits(want[k]).reshape(g.shape[0], -1)
            bad = np.flatnonzero((a != b).any(1))
            assert bad.size == 0, f"{what}: {bad.size} of {a.shape[0]} rows of {k} differ, first at {bad[:5]}: got {g[bad[:2]]}, want {want[k][bad[:2]]}"


# ---- 0: the light records ----------------------------------------------------------------------------------------------------------
def test_lights_are_the_authored_records_and_follow_an_update(gpu):
    for name in ("points", "qpq", "dim", "quad"):
        ds = make_scene(name, "reference")
        got, want = ds.lights(), dc.lights_of(name)
        assert len(got) == len(want) == ds.info()["light_count"]
        for g, w in zip(got, want):
            assert int(g["kind"]) == w["kind"] and g["intensity"] == w["intensity"] and g["area"] == w["area"], name
            for f, k in (("color", 4), ("position", 3), ("ab", 3), ("ac", 3), ("normal", 3)):
                assert np.array_equal(g[f][:k], w[f][:k]), (name, f, g[f], w[f])
            if w["kind"] == dc.POINT:
                assert np.array_equal(g["attenuation"][:3], w["attenuation"]) and g["attenuation"][3] == 0
            else:
                assert int(g["material"]) != 0xFFFFFFFF
            assert g["position"][3] == 1.0
        ds.close()
    moved = [dict(L) for L in dc.LIGHTS["points"]]
    moved[0].update(position=np.float32([0.1, 1.2, -0.3]), intensity=np.float32(2.5), color=np.float32([1, 0.5, 0.25, 0.75]))
    moved[1].update(attenuation=np.float32([0.25, 0.5, 0.125]))
    ds = make_scene("points", "sah")
    from rayca_amd import flatten
    ds.update(flatten(dc.build_scene("points", moved)))
    got = ds.lights()
    for g, w in zip(got, moved):
        assert g["intensity"] == w["intensity"] and np.array_equal(g["color"], w["color"]) and np.array_equal(g["position"][:3], w["position"])
        assert np.array_equal(g["attenuation"][:3], w["attenuation"])
    # and the call reads the updated table
    cfg = config("points")
    p, n = dc.surface_points("points", 65)
    want, _ = expected(ds, cfg, p, n, bias=dc.BIAS)
    assert_same(run(ds, cfg, p, n, OUT_HEMI, bias=float(dc.BIAS)), want, "after an update")
    ds.close()


# ---- 1: four scenes, three builds, both modes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", dc.SCENES)
def test_all_outputs_match_the_specification(gpu, name, how):
    ds = make_scene(name, how)
    if name == "quad":
        assert ds.info()["sphere_count"] == 1
    cfg = config(name)
    p, n = dc.surface_points(name)
    want, s = expected(ds, cfg, p, n, bias=dc.BIAS)
    got = run(ds, cfg, p, n, OUT_HEMI, bias=float(dc.BIAS))
    assert_same(got, want, f"{name} {how} hemisphere")
    idx = np.array(sorted(dc.INACTIVE))
    assert not got["irradiance"][idx].any() and not got["mask"][idx].any() and not got["counts"][idx].any()
    lit, traced = int((got["counts"] & 0xFFFF).sum()), int(s["traced"].sum())
    print(f"{name} {how}: {traced} of {s['tmax'].size} samples traced, {lit} lit, {int(s['dropped'].sum())} dropped, {int(s['void'].sum())} void")
    assert 0.1 * traced <= lit <= 0.97 * traced, "neither answer may be rare (on the CPU oracle 83 % .. 94 % of the traced samples are lit)"
    assert s["void"].sum() > 0
    if any(L["kind"] == dc.POINT for L in dc.lights_of(name)):
        assert got["counts"][dc.ON_LIGHT] >> 16 >= cfg.light_samples, "the point on the light drops that light's samples"
    v = dc.volume_points(name)
    want, s = expected(ds, cfg, v, None, sh=True)
    got = run(ds, cfg, v, None, OUT_SPHERE)
    assert_same(got, want, f"{name} {how} sphere")
    assert (got["sh"][:, :, 3] == 0).all() and s["traced"].sum() > 0
    ds.close()


# ---- 2: tiny batches, N = 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_counts_and_single_samples(gpu, how):
    import torch
    name = "qpq"
    ds = make_scene(name, how)
    cfg = config(name)
    p, n = dc.surface_points(name)
    want, _ = expected(ds, cfg, p[:65], n[:65], bias=dc.BIAS)
    for count in dc.COUNTS[:4]:
        got = run(ds, cfg, p[:count], n[:count], OUT_HEMI, bias=float(dc.BIAS))
        assert_same(got, {k: v[:count] for k, v in want.items()}, f"{count} points")
    for li in range(3):                                            # N = 1: one light, one sample
        w1, _ = expected(ds, cfg, p[:65], n[:65], bias=dc.BIAS, light_first=li, light_count=1)
        assert_same(run(ds, cfg, p[:65], n[:65], OUT_HEMI, bias=float(dc.BIAS), light_first=li, light_count=1), w1, f"light {li} alone")
    none = ds.direct(dev(p[:0]), dev(n[:0]), cfg, want=OUT_HEMI, want_stats=True)
    assert [tuple(none[k].shape) for k in OUT_HEMI] == [(0, 4), (0, 1), (0,)] and none["stats"]["kernel_launches"] == 0
    torch.cuda.synchronize()
    ds.close()


# ---- 3: light ranges and point chunks give what one call gives ------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_light_ranges_and_point_chunks(gpu, how):
    name = "qpq"
    ds = make_scene(name, how)
    cfg = Config(light_samples=4, light_stratify=True, seed=5, max_depth=1)
    p, n = dc.surface_points(name, 65)
    p, n = np.tile(p, (3, 1))[:130], np.tile(n, (3, 1))[:130]
    full = run(ds, cfg, p, n, ("mask", "irradiance"), bias=float(dc.BIAS), first_index=1000)
    want, _ = expected(ds, cfg, p, n, bias=dc.BIAS, first_index=1000)
    assert_same(full, want, "the full call")
    for first, cnt in ((0, 1), (1, 2), (2, 1), (0, 2)):
        part = run(ds, cfg, p, n, ("mask",), bias=float(dc.BIAS), first_index=1000, light_first=first, light_count=cnt)
        sel = (full["mask"][:, 0] >> np.uint64(4 * first)) & np.uint64((1 << 4 * cnt) - 1)
        assert np.array_equal(part["mask"][:, 0], sel), f"lights {first} .. {first + cnt}: the rows of the full call"
    # the quad draws of the second copy of the points differ from the first copy's: the stream is the point index's
    assert not np.array_equal(full["irradiance"][:65], full["irradiance"][65:130])
    for a, b in ((0, 64), (64, 130)):
        chunk = run(ds, cfg, p[a:b], n[a:b], ("mask", "irradiance"), bias=float(dc.BIAS), first_index=1000 + a)
        assert_same(chunk, {k: v[a:b] for k, v in want.items()}, f"points {a} .. {b}")
    # first_index + i wraps at 2^32 only in the key
    top = run(ds, cfg, p[:4], n[:4], ("irradiance", "mask"), bias=float(dc.BIAS), first_index=(1 << 32) - 4)
    assert_same(top, expected(ds, cfg, p[:4], n[:4], bias=dc.BIAS, first_index=(1 << 32) - 4)[0], "the last four indices")
    ds.close()


# ---- 4: more than 64 samples: the wrapper chunks over lights ------------------------------------------------------------------------------
def test_wrapper_chunks_long_light_ranges(gpu):
    name = "qpq"
    ds = make_scene(name, "sah")
    cfg = Config(light_samples=32, light_stratify=False, seed=2, max_depth=1)
    v = dc.volume_points(name, 257)
    got = run(ds, cfg, v, None, OUT_SPHERE)
    assert got["mask"].shape == (257, 2)                           # lights 0 .. 1 and light 2
    a, _ = expected(ds, cfg, v, None, sh=True, light_first=0, light_count=2)
    b, _ = expected(ds, cfg, v, None, sh=True, light_first=2, light_count=1)
    assert np.array_equal(got["mask"][:, 0], a["mask"]) and np.array_equal(got["mask"][:, 1], b["mask"])
    assert np.array_equal(bits(got["irradiance"][:, :3]), bits(a["irradiance"][:, :3] + b["irradiance"][:, :3]))
    assert np.array_equal(bits(got["sh"]), bits(a["sh"] + b["sh"])) and np.array_equal(got["counts"], a["counts"] + b["counts"])
    lit = (a["counts"] & 0xFFFF) + (b["counts"] & 0xFFFF)
    assert np.abs(got["irradiance"][:, 3] - lit / 96.0).max() < 1e-6
    ds.close()


# ---- 5: output subsets and guard words -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_output_subsets_and_guards(gpu, how):
    import torch
    name = "qpq"
    ds = make_scene(name, how)
    cfg = config(name)
    count = 599
    v = dc.volume_points(name, count)
    want, s = expected(ds, cfg, v, None, sh=True)
    shape = {"irradiance": (4,), "sh": (9, 4), "mask": (), "counts": ()}
    dtype = {"irradiance": torch.float32, "sh": torch.float32, "mask": torch.int64, "counts": torch.int32}
    sentinel = {"irradiance": -7.0, "sh": -7.0, "mask": 0x5A5A5A5A5A5A5A5A, "counts": 0x5A5A5A5A}
    big = {k: torch.full((count + 128, *shape[k]), sentinel[k], dtype=dtype[k], device="cuda") for k in OUT_SPHERE}
    v_d = dev(v)
    for subset in range(1, 16):
        d = abi.RaycaDirect()
        d.count, d.light_first, d.light_count, d.points = count, 0, 3, v_d.data_ptr()
        asked = tuple(k for j, k in enumerate(OUT_SPHERE) if subset >> j & 1)
        for k in asked:
            setattr(d, k + "_out", big[k][64:-64].data_ptr())
        o = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
        st = abi.RaycaStats()
        c = cfg.to_abi()
        lib.check(gpu.rayca_hip_direct_device(ds.handle, C.byref(c), C.byref(o), C.byref(d), C.byref(st)))   # (no stream: the call waits)
        assert st.kernel_launches == (1 if asked == ("mask",) else 2) and st.rays_shadow == int(s["traced"].sum())
        for k in OUT_SPHERE:
            if k in asked:
                got = big[k][64:-64].cpu().numpy()
                assert_same({k: got.view(np.uint64) if k == "mask" else got.view(np.uint32) if k == "counts" else got}, want, f"subset {subset}")
                assert bool((big[k][:64] == sentinel[k]).all()) and bool((big[k][-64:] == sentinel[k]).all()), (subset, k, "guard words")
            else:
                assert bool((big[k] == sentinel[k]).all()), (subset, k, "an output that was not asked for")
            big[k].fill_(sentinel[k])
    ds.close()


# ---- 6: another stream and context; refusals that need the scene -------------------------------------------------------------------------
def test_other_streams_contexts_and_scene_refusals(gpu):
    import torch
    name = "qpq"
    ds = make_scene(name, "sah")
    cfg = config(name)
    p, n = dc.surface_points(name, 257)
    want, _ = expected(ds, cfg, p, n, bias=dc.BIAS)
    p_d, n_d = dev(p), dev(n)
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    res = [ds.direct(p_d, n_d, cfg, want=OUT_HEMI, bias=float(dc.BIAS), stream=s, context=k + 1) for k, s in enumerate(streams)]
    raw = ds.direct(p_d, n_d, cfg, want=("irradiance",), bias=float(dc.BIAS), stream=streams[0].cuda_stream, context=7)   # (scratch mask words)
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        assert_same({"irradiance": r["irradiance"].cpu().numpy(), "mask": r["mask"].cpu().numpy().view(np.uint64),
                     "counts": r["counts"].cpu().numpy().view(np.uint32)}, want, f"context {k + 1}")
    assert_same({"irradiance": raw["irradiance"].cpu().numpy()}, want, "context 7, a raw stream handle")
    with pytest.raises(RaycaError):
        ds.direct(p_d, n_d, cfg, context=8)
    with pytest.raises(ValueError):
        ds.direct(p_d, n_d, cfg, light_first=2, light_count=2)
    with pytest.raises(ValueError):
        ds.direct(p_d, n_d, cfg, want=("sh",))
    d = abi.RaycaDirect()
    d.count, d.light_first, d.light_count, d.points, d.counts_out = 4, 3, 1, p_d.data_ptr(), dev(np.zeros(4, np.int32)).data_ptr()
    c = cfg.to_abi()
    assert gpu.rayca_hip_direct_device(ds.handle, C.byref(c), None, C.byref(d), None) == abi.ERR_BAD_ARG and "lights" in lib.last_error()
    ds.close()


# ---- 7: a tree whose stack need exceeds the LDS part ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
def test_tree_that_needs_the_spill_area(gpu, how):
    from test_gpu_probes import chain_inputs
    desc, (p, n), diag, _ = chain_inputs()
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    if how == "sah":
        ds.finish()
    assert ds.info()["max_depth"] + 1 > 24 and ds.info()["light_count"] >= 1
    cfg = Config(light_samples=1, seed=1, max_depth=1)
    bias = np.float32(1e-4 * diag)
    want, s = expected(ds, cfg, p, n, bias=bias)
    got = run(ds, cfg, p, n, OUT_HEMI, bias=float(bias))
    assert_same(got, want, f"chain {how}")
    lit = got["counts"] & 0xFFFF
    assert lit.any() and int(lit.sum()) < int(s["traced"].sum())
    ds.close()


# ---- 8: statistics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_statistics(gpu, how):
    name = "qpq"
    ds = make_scene(name, how)
    cfg = config(name)
    p, n = dc.surface_points(name, 599)
    s = literal_samples(ds, cfg, p, n, bias=dc.BIAS)
    traced = int(s["traced"].sum())
    assert 0 < traced < s["tmax"].size
    plain = run(ds, cfg, p, n, ("irradiance",), bias=float(dc.BIAS), want_stats=True)["stats"]
    counted = run(ds, cfg, p, n, ("irradiance",), bias=float(dc.BIAS), collect_stats=True)["stats"]
    for st in (plain, counted):
        assert st["rays_shadow"] == traced and st["rays_primary"] == 0
        assert st["kernel_launches"] == 2 and st["kernel_ms"] > 0
        assert st["class_launches"][abi.KERNEL_OTHER] == 2 and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
    assert plain["boxes_tested"] == 0 and plain["triangles_tested"] == 0
    assert counted["boxes_tested"] > 0 and counted["triangles_tested"] > 0
    if how == "sah":
        assert counted["node_format"] & 2048 == 0 and counted["node_format"] & 1, "a finished SAH scene runs the lane-refill form on the 4-wide nodes"
    else:
        assert counted["node_format"] & 1 == 0
    ds.close()


# ---- 9: the product's own path vertex -------------------------------------------------------------------------------------------------------
def test_radiance_at_depth_one_is_kd_over_pi_times_e(gpu):
    """radiance() at max_depth 1 under NEE along rays aimed at the room's Phong surfaces (ks = 0, shininess 0), against
    kd / pi * E at the hit points.  Per term the pixel rounds le * brdf, * ndot, * d_omega, * alpha and brdf = kd * (1 / pi); the
    call rounds le * ndot, * d_omega, * alpha, and the test kd * (1 / pi), * E: five each; both sum N terms (N - 1 roundings).
    Every term is >= 0 for the surfaces below the lamps, so the bound is relative: (2 N + 8) roundings of 2^-24, times 1 + 2^-20
    for their products."""
    import torch
    name = "points"
    ds = make_scene(name, "sah")
    cfg = Config(light_samples=1, seed=9, max_depth=1)
    w, h = 48, 36
    rays = ds.camera_rays(cfg, w, h)
    g = ds.gbuffer(cfg, w, h, want=("point", "normal", "diffuse", "flags"))
    pix = ds.radiance(rays.reshape(-1, 6), cfg)
    e = ds.direct(g["point"].reshape(-1, 3), g["normal"].reshape(-1, 3), cfg, bias=1e-4, want=("irradiance", "counts"))
    torch.cuda.synchronize()
    pix, kd, flags = pix.cpu().numpy(), g["diffuse"].reshape(-1, 4).cpu().numpy(), g["flags"].reshape(-1).cpu().numpy().view(np.uint32)
    E, counts = e["irradiance"].cpu().numpy(), e["counts"].cpu().numpy().view(np.uint32)
    keep = (flags >> 31 == 1) & (flags & 4 == 0) & (counts >> 16 == 0)
    N = 2
    want = (kd[:, :3] * np.float32(0.318309873342514038086)) * E[:, :3]
    bound = (2 * N + 8) * 2.0 ** -24 * (1 + 2.0 ** -20)
    err = np.abs(pix[keep, :3].astype(np.float64) - want[keep]) / np.maximum(want[keep].astype(np.float64), 1e-30)
    err[want[keep] == pix[keep, :3]] = 0
    print(f"{int(keep.sum())} pixels, largest relative difference {err.max():.3e}, bound {bound:.3e}")
    assert keep.sum() > 1000 and (E[keep, :3] > 0).any()
    assert err.max() <= bound
    ds.close()


# ---- 10: the probe bake -------------------------------------------------------------------------------------------------------------------
def test_bake_with_direct_adds_the_sphere_mode_projection(gpu):
    import torch
    ds = make_scene("points", "sah")
    cfg = Config(max_depth=1, seed=4)
    grid = ProbeGrid.around([-1, 0, -1], [1, 2, 1], (3, 3, 2), margin=-0.25)
    sh0, kept0 = grid.bake(ds, cfg, samples=16, sample=3)
    sh1, kept1 = grid.bake(ds, cfg, samples=16, sample=3, direct=True)
    d = ds.direct(dev(grid.positions()), None, cfg, sample=3, want=("sh",))
    torch.cuda.synchronize()
    assert np.array_equal(bits((sh0 + d["sh"]).cpu().numpy()), bits(sh1.cpu().numpy())) and np.array_equal(kept0.cpu().numpy(), kept1.cpu().numpy())
    assert float(d["sh"][:, 0, :3].min()) > 0, "every probe of the room sees a point light"
    assert np.array_equal(bits(grid.bake(ds, cfg, samples=16, sample=3)[0].cpu().numpy()), bits(sh0.cpu().numpy()))
    ds.close()
