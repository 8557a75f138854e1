"""rayca_hip_denoise_variance_device (DeviceScene.denoise_variance, Film.resolve(denoise="variance")) on the GPU.

Every comparison is bit for bit (the float words as uint32, the RGBA8 bytes, and variance_out): against the literal
numpy-float32 restatement of the filter (tests/denoise_variance_literal.py -- the filter is +, -, x, / and max only, each
rounded once, so the restatement has the kernels' bits), against rayca_hip_denoise_device for the output stage, and between the
ways of making one call (in place, another stream, another frame context, through Film)."""
import os

import numpy as np
import pytest

import denoise_literal as dl
import denoise_variance_literal as dv
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, abi, flatten, lib, scenes
from rayca_amd import model as M
from rayca_amd import sdtf
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
GUIDES = ("albedo", "normal", "point", "id")
SIGMA_PLANE = 0.5
SIZES = [(1, 1), (1, 40), (40, 1), (3, 3), (61, 37), (65, 5), (130, 70)]   # (width, height)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_desc(name):
    scene = M.Scene()
    if name == "box":
        scene.push_model(scenes.load_gltf(os.path.join(G, "box.gltf")))
        scene.push_model(M.create_default_model())
    else:
        sdtf.push_sdtf_from_path(scene, os.path.join(G, name + ".sdtf"))
    return flatten(scene)


@pytest.fixture(scope="module")
def ds(gpu):
    """the scene whose handle the synthetic calls go through (its contents are not read)"""
    s = DeviceScene(make_desc("box"), Config())
    yield s
    s.close()


_FRAMES = {}


def frame(width, height):
    """the synthetic frame of a size with its specials (NaN, +inf, denormal colours, zero normals), plus a variance with a NaN,
    a +inf and negative values at fixed pixels and a length mixed below and above 4 with a zero and a NaN; made once, read-only"""
    key = (width, height)
    if key not in _FRAMES:
        s = dl.synthetic(width, height, 977 + 131 * width + height, specials=True)
        rng = np.random.default_rng(5 + 17 * width + height)
        lum = dv.lum(s["clean"])
        variance = (F(0.5) * lum * lum * rng.gamma(2.0, 0.5, size=(height, width))).astype(F)
        length = rng.integers(1, 12, size=(height, width)).astype(F)

        def at(py, px):
            return (py % height, px % width)

        variance[at(3, 5)] = np.nan
        variance[at(6, 20)] = np.inf
        variance[at(8, 1)] = -0.25
        variance[at(1, 44)] = -np.inf
        length[at(10, 7)] = 0.0
        length[at(12, 33)] = np.nan
        length[at(0, 0)] = 3.0     # (a 1 x 1 frame takes the spatial estimate of its one pixel)
        s.update(variance=variance, length=length)
        for a in s.values():
            a.setflags(write=False)
        _FRAMES[key] = s
    return _FRAMES[key]


def dev(a):
    import torch
    a = np.array(a)   # (a writable copy: the shared frames are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def guide_kw(s, which, on_device):
    kw = {k: (dev(s[k]) if on_device else s[k]) for k in which}
    if "point" in which:
        kw["sigma_plane"] = SIGMA_PLANE
    return kw


def run(ds, s, which, *, length=True, **kw):
    """(rgba32f, rgba8, variance_out) of DeviceScene.denoise_variance as numpy"""
    import torch
    out, out8, var = ds.denoise_variance(dev(s["color"]), dev(s["variance"]), length=dev(s["length"]) if length else None, rgba8=True,
                                         variance_out=True, **guide_kw(s, which, True), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out8.cpu().numpy(), var.cpu().numpy()


def literal(s, which, *, length=True, **kw):
    return dv.denoise_variance(s["color"], s["variance"], length=s["length"] if length else None, **guide_kw(s, which, False), **kw)


def assert_same(got, want, what):
    (g32, g8, gv), (w32, w8, wv) = got, want
    bad = np.argwhere((bits(g32) != bits(w32)).any(-1))
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {g32[tuple(bad[0])]} want {w32[tuple(bad[0])]}"
    assert np.array_equal(g8, w8), f"{what}: RGBA8 differs at {np.argwhere((g8 != w8).any(-1))[:4].tolist()}"
    bad = np.argwhere(bits(gv) != bits(wv))
    assert bad.size == 0, f"{what}: variance_out differs at {len(bad)} pixels, first (y, x) {bad[:4].tolist()}: got {gv[tuple(bad[0])]} want {wv[tuple(bad[0])]}"


# ---- 1: against the literal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SIZES)
def test_every_size_equals_the_literal(ds, width, height):
    """widths around a wave and a block edge, steps larger than the image, step 16 in the 130 x 70 frame; the spatial estimate in
    the lanes whose length is below 4, also where its 7 x 7 taps leave the image"""
    s = frame(width, height)
    for iterations in (3, 5):
        got = run(ds, s, GUIDES, iterations=iterations)
        assert_same(got, literal(s, GUIDES, iterations=iterations), f"{width} x {height}, {iterations} iterations")


SUBSETS = {"none": (), "normal": ("normal",), "normal_point": ("normal", "point"), "id": ("id",), "albedo": ("albedo",), "all": GUIDES}


@pytest.mark.parametrize("name", list(SUBSETS))
def test_every_guide_subset_equals_the_literal(ds, name):
    which = SUBSETS[name]
    s = frame(61, 37)
    for npow, sigma_luminance in ((0, 4.0), (7, 1.5)):
        kw = dict(iterations=4, normal_power_log2=npow, sigma_luminance=sigma_luminance)
        assert_same(run(ds, s, which, **kw), literal(s, which, **kw), f"{name}, normal_power_log2 {npow}")


@pytest.mark.parametrize("name,length,min_history", [("no length", False, 4), ("no fallback", True, 0), ("mixed lengths", True, 4), ("all short", True, 100)])
def test_every_length_variant_equals_the_literal(ds, name, length, min_history):
    """without a length (min_history does not apply), with a length and no fallback, with lengths mixed below and above
    min_history, a zero and a NaN among them, and with every lane in the spatial estimate"""
    s = frame(61, 37)
    for which in (GUIDES, ("id",), ()):
        kw = dict(iterations=3, min_history=min_history, variance_floor=1e-6)
        assert_same(run(ds, s, which, length=length, **kw), literal(s, which, length=length, **kw), f"{name}, guides {which}")


def test_special_values_stay_where_they_are(ds):
    """the fixed pixels of the frame: the NaN and the +inf colour pass through and reach no neighbour, a zero normal passes its
    pixel through; a NaN, a +inf or a negative variance leaves no NaN in variance_out"""
    s = frame(61, 37)
    assert np.isnan(s["color"][2, 3, 0]) and np.isinf(s["color"][5, 17, 1]) and 0 < s["color"][11, 30, 0] < 1.2e-38
    assert np.isnan(s["variance"][3, 5]) and np.isinf(s["variance"][6, 20]) and s["variance"][8, 1] < 0 and np.isnan(s["length"][12, 33])
    for min_history in (0, 4):
        g32, _, gv = run(ds, s, ("normal", "point", "id"), iterations=5, min_history=min_history)
        assert np.array_equal(np.argwhere(~np.isfinite(g32)), np.array([[2, 3, 0], [5, 17, 1]]))
        for y, x in ((2, 3), (5, 17), (4, 8), (9, 2)):   # NaN, inf, and the two zero normals
            assert np.array_equal(bits(g32[y, x]), bits(s["color"][y, x])), (y, x)
        assert (bits(g32) != bits(s["color"])).any(-1).mean() > 0.95
        assert not np.isnan(gv).any() and (gv >= 0).all()
    g32, _, gv = run(ds, s, GUIDES, iterations=5)
    assert not np.isnan(gv).any() and np.array_equal(np.argwhere(np.isnan(g32)), np.array([[2, 3, 0]]))


# ---- 2: the ways of making one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 4])
def test_in_place_equals_out_of_place(ds, iterations):
    import torch
    s = frame(61, 37)
    for which in (GUIDES, ()):
        want = run(ds, s, which, iterations=iterations)
        color, variance = dev(s["color"]), dev(s["variance"])
        out, out8, var = ds.denoise_variance(color, variance, length=dev(s["length"]), out=color, variance_out=variance, rgba8=True,
                                             iterations=iterations, **guide_kw(s, which, True))
        torch.cuda.synchronize()
        assert out is color and var is variance
        assert_same((color.cpu().numpy(), out8.cpu().numpy(), variance.cpu().numpy()), want, f"in place, {iterations} iterations, guides {which}")


def test_strided_inputs_equal_contiguous_ones(ds):
    """an input that is not contiguous reaches the kernels as a contiguous copy: the contiguous call's bits"""
    import torch
    from strided import strided
    s = frame(65, 5)
    want = run(ds, s, GUIDES, iterations=2)
    out, out8, var = ds.denoise_variance(strided(dev(s["color"])), strided(dev(s["variance"])), length=strided(dev(s["length"])), rgba8=True,
                                         variance_out=True, iterations=2, **strided(guide_kw(s, GUIDES, True)))
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), out8.cpu().numpy(), var.cpu().numpy()), want, "strided inputs")


def test_stream_and_context_do_not_change_the_result(ds):
    import torch
    s = frame(130, 70)
    want = run(ds, s, GUIDES, iterations=5)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        color, variance, length, kw = dev(s["color"]), dev(s["variance"]), dev(s["length"]), guide_kw(s, GUIDES, True)
    side.synchronize()
    # a small frame first, unwaited: the context's scratch images and variance planes have to grow behind it
    small = frame(65, 5)
    call = dict(rgba8=True, variance_out=True, iterations=5, stream=side, context=1)
    got_small = ds.denoise_variance(dev(small["color"]), dev(small["variance"]), length=dev(small["length"]), **call, **guide_kw(small, GUIDES, True))
    results = [ds.denoise_variance(color, variance, length=length, **call, **kw) for _ in range(3)]   # back to back, unwaited
    torch.cuda.synchronize()
    for r in results:
        assert_same(tuple(x.cpu().numpy() for x in r), want, "side stream, context 1")
    assert_same(tuple(x.cpu().numpy() for x in got_small), literal(small, GUIDES, iterations=5), "65 x 5 in front of 130 x 70")


def test_stats_count_the_launches(ds):
    s = frame(61, 37)
    color, variance, length = dev(s["color"]), dev(s["variance"]), dev(s["length"])
    for which, iterations, launches in ((GUIDES, 5, 8), (("normal",), 5, 7), (GUIDES, 1, 4), ((), 1, 3)):
        out, st = ds.denoise_variance(color, variance, length=length, iterations=iterations, want_stats=True, **guide_kw(s, which, True))
        assert st["kernel_launches"] == launches and st["class_launches"][abi.KERNEL_OTHER] == launches, (which, iterations, st)
        assert st["kernel_ms"] > 0 and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
        assert sum(st["class_launches"]) == launches


def test_guard_cells_stay_untouched(ds):
    import torch
    w, h = 61, 37
    s = frame(w, h)
    n = w * h
    big32 = torch.full((n * 4 + 128,), -7.0, dtype=torch.float32, device="cuda")
    big8 = torch.full((n * 4 + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    bigv = torch.full((n + 128,), -7.0, dtype=torch.float32, device="cuda")
    out, out8, var = big32[64:64 + n * 4].view(h, w, 4), big8[64:64 + n * 4].view(h, w, 4), bigv[64:64 + n].view(h, w)
    ds.denoise_variance(dev(s["color"]), dev(s["variance"]), length=dev(s["length"]), out=out, rgba8=out8, variance_out=var, iterations=3,
                        **guide_kw(s, GUIDES, True))
    torch.cuda.synchronize()
    assert bool((big32[:64] == -7.0).all()) and bool((big32[64 + n * 4:] == -7.0).all())
    assert bool((big8[:64] == 0x5A).all()) and bool((big8[64 + n * 4:] == 0x5A).all())
    assert bool((bigv[:64] == -7.0).all()) and bool((bigv[64 + n:] == -7.0).all())
    assert_same((out.cpu().numpy(), out8.cpu().numpy(), var.cpu().numpy()), literal(s, GUIDES, iterations=3), "guarded outputs")


# ---- 3: the output stage, and the film ---------------------------------------------------------------------------------------
def test_gamma_is_the_output_stage_of_the_plain_denoiser(ds):
    """gamma 2.2 on the call is denoise(iterations=0, gamma=2.2) -- finalize_pixel's gamma and quantisation -- on the gamma-1
    result; the variance does not change with it"""
    import torch
    s = dl.synthetic(61, 37, 977, specials=False)
    f = frame(61, 37)
    args = (dev(s["color"]), dev(f["variance"]))
    kw = dict(length=dev(f["length"]), rgba8=True, variance_out=True, iterations=3, **guide_kw(s, GUIDES, True))
    lin32, _, lin_var = ds.denoise_variance(*args, **kw)
    got32, got8, got_var = ds.denoise_variance(*args, gamma=2.2, **kw)
    want32, want8 = ds.denoise(lin32, iterations=0, gamma=2.2, rgba8=True)
    torch.cuda.synchronize()
    assert torch.equal(got32.view(torch.int32), want32.view(torch.int32)) and torch.equal(got8, want8)
    assert torch.equal(got_var.view(torch.int32), lin_var.view(torch.int32)) and not torch.equal(got32, lin32)


def camera_node(desc):
    return next(n for n in desc._nodes[:desc.c.node_count] if n.camera != abi.NONE)


def test_film_resolve_is_the_call_by_hand(gpu):
    """a few frames, a camera move, a few more: Film.resolve(denoise="variance") is denoise_variance on the film's colour,
    variance, length and G-buffer"""
    import torch
    w, h = 65, 37
    desc = make_desc("cornell_quad")
    scene = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    scene.finish()
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=2.2)
    film = Film(scene, w, h)
    for _ in range(3):
        film.add(cfg)
    cam = camera_node(desc)
    cam.trs.translation[:] = tuple(t + d for t, d in zip(tuple(cam.trs.translation), (0.04, 0.015, -0.02)))
    scene.update(desc)
    for _ in range(2):
        film.add(cfg)
    got32, got8, got_var = film.resolve(denoise="variance", rgba8=True, variance_out=True, iterations=4)
    want32, want8, want_var = scene.denoise_variance(film.color, film.variance, length=film.length, gamma=2.2, rgba8=True, variance_out=True,
                                                     iterations=4, sigma_plane=0.1, **film.gbuffer())
    plain = film.resolve(denoise=True, iterations=4)
    torch.cuda.synchronize()
    assert torch.equal(got32.view(torch.int32), want32.view(torch.int32)) and torch.equal(got8, want8)
    assert torch.equal(got_var.view(torch.int32), want_var.view(torch.int32))
    length = film.length.cpu().numpy()
    print(f"history lengths behind the move: min {length.min()}, max {length.max()}, {float((length < 4).mean()):.3f} of the pixels below 4")
    assert length.max() > 4.5 and (length < 4).any()   # (the fallback's lanes and the others both ran)
    assert not torch.equal(got32, plain) and not np.isnan(got_var.cpu().numpy()).any()
    # ... and against the literal, on what the film holds (gamma 1: the literal's output stage)
    lin32, lin8, lin_var = film.resolve(denoise="variance", gamma=1.0, rgba8=True, variance_out=True, iterations=4)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in film.gbuffer().items()}
    g["id"] = g["id"].view(np.uint32)
    want = dv.denoise_variance(film.color.cpu().numpy(), film.variance.cpu().numpy(), length=length, iterations=4, sigma_plane=0.1, **g)
    assert_same((lin32.cpu().numpy(), lin8.cpu().numpy(), lin_var.cpu().numpy()), want, "the film against the literal")
    with pytest.raises(ValueError):
        film.resolve(denoise="median")
    bare = Film(scene, w, h, moments=False)
    bare.add(cfg)
    with pytest.raises(ValueError):
        bare.resolve(denoise="variance")
    torch.cuda.synchronize()
    scene.close()


# ---- 4: errors --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(gpu, ds):
    import ctypes as C
    import torch
    w, h = 16, 8
    color = torch.rand((h, w, 4), dtype=torch.float32, device="cuda")
    plane = torch.rand((h, w), dtype=torch.float32, device="cuda")
    guide3 = torch.rand((h, w, 3), dtype=torch.float32, device="cuda")
    out = torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda")
    out8 = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device="cuda")
    var = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")

    def call(o_fields=None, **fields):
        d = abi.RaycaDenoiseVariance()
        d.width, d.height, d.iterations, d.normal_power_log2, d.min_history = w, h, 2, 7, 4
        d.sigma_luminance, d.sigma_plane, d.variance_floor, d.gamma = 4.0, SIGMA_PLANE, 1e-10, 1.0
        d.color, d.variance, d.length = color.data_ptr(), plane.data_ptr(), plane.data_ptr()
        d.rgba32f_out, d.rgba8_out, d.variance_out = out.data_ptr(), out8.data_ptr(), var.data_ptr()
        for k, v in fields.items():
            setattr(d, k, v)
        o = abi.RaycaRenderOptions()
        for k, v in (o_fields or {}).items():
            setattr(o, k, v)
        return gpu.rayca_hip_denoise_variance_device(ds.handle, C.byref(o), C.byref(d), None)

    cases = [dict(color=None), dict(variance=None), dict(rgba32f_out=None, rgba8_out=None), dict(iterations=0), dict(iterations=9), dict(length=None),
             dict(point=guide3.data_ptr()), dict(sigma_luminance=0.0), dict(variance_floor=0.0), dict(gamma=float("nan")), dict(reserved=1),
             dict(color=color.data_ptr() + 4), dict(o_fields=dict(context=8)), dict(o_fields=dict(engine=1))]
    for kw in cases:
        assert call(**kw) == abi.ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((out8 == 0x5A).all()) and bool((var == -7.0).all())   # nothing of the above wrote anything
    assert call(point=guide3.data_ptr(), normal=guide3.data_ptr()) == abi.OK
    torch.cuda.synchronize()
    assert bool((out != -7.0).all()) and bool((var != -7.0).all())
    with pytest.raises(RaycaError) as e:
        ds.denoise_variance(color, plane, iterations=0)
    assert e.value.code == abi.ERR_BAD_ARG and "iterations" in lib.last_error()
    with pytest.raises(ValueError):
        ds.denoise_variance(color, plane, normal=guide3, point=guide3)   # (no sigma_plane)
    with pytest.raises(ValueError):
        ds.denoise_variance(color, plane[:, :3])
    with pytest.raises(TypeError):
        ds.denoise_variance(color, plane.double())
    # an empty scene is no error: the scene is not read
    empty = M.Scene()
    empty.push_model(M.create_default_model())
    es = DeviceScene(flatten(empty), Config())
    got = es.denoise_variance(color, plane, length=plane, iterations=2)
    want = ds.denoise_variance(color, plane, length=plane, iterations=2)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    es.close()
