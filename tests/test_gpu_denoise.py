"""rayca_hip_denoise_device (DeviceScene.denoise, .render_denoised) on the GPU.

Every comparison is bit for bit (the float words as uint32, and the RGBA8 bytes): against the literal numpy-float32 restatement
of the filter (tests/denoise_literal.py -- the filter is +, -, x, / and max only, each rounded once, so the restatement has the
kernel's bits), against a render call for the output stage (gamma, quantisation), and between the ways of making one call
(in place, another stream, another frame context, through render_denoised)."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_literal as dl
from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi, flatten, lib, scenes
from rayca_amd import model as M
from rayca_amd import sdtf
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = np.uint32(0xFFFFFFFF)
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


def frame(width, height, specials=True):
    """the synthetic frame of a size, made once and shared read-only"""
    key = (width, height, specials)
    if key not in _FRAMES:
        s = dl.synthetic(width, height, 977 + 131 * width + height, specials=specials)
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


def run(ds, s, which, **kw):
    """(rgba32f, rgba8) of DeviceScene.denoise as numpy"""
    import torch
    out, out8 = ds.denoise(dev(s["color"]), rgba8=True, **guide_kw(s, which, True), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out8.cpu().numpy()


def assert_same(got, want, what):
    (g32, g8), (w32, w8) = got, want
    bad = np.argwhere((bits(g32) != bits(w32)).any(-1))
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {g32[tuple(bad[0])]} want {w32[tuple(bad[0])]}"
    assert np.array_equal(g8, w8), f"{what}: RGBA8 differs at {np.argwhere((g8 != w8).any(-1))[:4].tolist()}"


# ---- 1: against the literal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SIZES)
def test_every_size_equals_the_literal(ds, width, height):
    """widths around a wave and a block edge, steps larger than the image (3 x 3: from step 2 on only the centre tap is inside),
    step 16 in the 130 x 70 frame; NaN, +inf, denormal colours and zero normals at fixed pixels"""
    s = frame(width, height)
    for iterations in (3, 5):
        got = run(ds, s, GUIDES, iterations=iterations)
        assert_same(got, dl.denoise(s["color"], iterations=iterations, **guide_kw(s, GUIDES, False)), f"{width} x {height}, {iterations} iterations")


SUBSETS = {"none": ((), 0.0), "colour": ((), 4.0), "normal": (("normal",), 4.0), "normal_point": (("normal", "point"), 4.0), "id": (("id",), 4.0),
           "albedo": (("albedo",), 4.0), "all": (GUIDES, 4.0), "all_without_colour": (GUIDES, -1.0)}


@pytest.mark.parametrize("name", list(SUBSETS))
def test_every_guide_subset_equals_the_literal(ds, name):
    which, sigma_color = SUBSETS[name]
    s = frame(61, 37)
    for npow in (0, 7):
        got = run(ds, s, which, iterations=4, sigma_color=sigma_color, normal_power_log2=npow)
        want = dl.denoise(s["color"], iterations=4, sigma_color=sigma_color, normal_power_log2=npow, **guide_kw(s, which, False))
        assert_same(got, want, f"{name}, normal_power_log2 {npow}")


def test_special_values_stay_where_they_are(ds):
    """the fixed pixels of denoise_literal.synthetic(specials=True): the NaN and the +inf pass through and reach no neighbour,
    a zero normal passes its pixel through"""
    s = frame(61, 37)
    g32, _ = run(ds, s, ("normal", "point", "id"), iterations=5)
    assert np.isnan(s["color"][2, 3, 0]) and np.isinf(s["color"][5, 17, 1]) and 0 < s["color"][11, 30, 0] < 1.2e-38
    assert np.array_equal(np.argwhere(~np.isfinite(g32)), np.array([[2, 3, 0], [5, 17, 1]]))
    for y, x in ((2, 3), (5, 17), (4, 8), (9, 2)):   # NaN, inf, and the two zero normals
        assert np.array_equal(bits(g32[y, x]), bits(s["color"][y, x])), (y, x)
    changed = (bits(g32) != bits(s["color"])).any(-1)
    assert changed.mean() > 0.95


# ---- 2: the ways of making one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, 4])
def test_in_place_equals_out_of_place(ds, iterations):
    import torch
    s = frame(61, 37)
    for which in (GUIDES, ()):
        want = run(ds, s, which, iterations=iterations)
        color = dev(s["color"])
        out, out8 = ds.denoise(color, out=color, rgba8=True, iterations=iterations, **guide_kw(s, which, True))
        torch.cuda.synchronize()
        assert out is color
        assert_same((color.cpu().numpy(), out8.cpu().numpy()), want, f"in place, {iterations} iterations, guides {which}")
    if iterations == 0:   # and nothing but the output stage ran: the input's bits, the literal's bytes
        assert np.array_equal(bits(want[0]), bits(s["color"])) and np.array_equal(want[1], dl.quantize(s["color"]))


def test_strided_inputs_equal_contiguous_ones(ds):
    """an input that is not contiguous reaches the kernels as a contiguous copy: the contiguous call's bits"""
    import torch
    from strided import strided
    s = frame(65, 5)
    want = run(ds, s, GUIDES, iterations=2)
    out, out8 = ds.denoise(strided(dev(s["color"])), rgba8=True, iterations=2, **strided(guide_kw(s, GUIDES, True)))
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), out8.cpu().numpy()), want, "strided inputs")


def test_stream_and_context_do_not_change_the_result(ds):
    import torch
    s = frame(130, 70)
    want = run(ds, s, GUIDES, iterations=5)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        color, kw = dev(s["color"]), guide_kw(s, GUIDES, True)
    side.synchronize()
    # a small frame first, unwaited: the context's scratch images have to grow behind it for the larger frames that follow
    small = frame(65, 5)
    got_small = ds.denoise(dev(small["color"]), rgba8=True, iterations=5, stream=side, context=1, **guide_kw(small, GUIDES, True))
    results = [ds.denoise(color, rgba8=True, iterations=5, stream=side, context=1, **kw) for _ in range(3)]   # back to back, unwaited
    torch.cuda.synchronize()
    for out, out8 in results:
        assert_same((out.cpu().numpy(), out8.cpu().numpy()), want, "side stream, context 1")
    assert_same((got_small[0].cpu().numpy(), got_small[1].cpu().numpy()), dl.denoise(small["color"], iterations=5, **guide_kw(small, GUIDES, False)), "65 x 5 in front of 130 x 70")


def test_stats_count_the_launches(ds):
    s = frame(61, 37)
    color = dev(s["color"])
    for which, iterations, launches in ((GUIDES, 5, 7), (("normal",), 5, 6), (GUIDES, 1, 3), ((), 0, 1), (GUIDES, 0, 1)):
        out, st = ds.denoise(color, iterations=iterations, want_stats=True, **guide_kw(s, which, True))
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
    out, out8 = big32[64:64 + n * 4].view(h, w, 4), big8[64:64 + n * 4].view(h, w, 4)
    for iterations in (0, 3):
        big32.fill_(-7.0)
        big8.fill_(0x5A)
        ds.denoise(dev(s["color"]), out=out, rgba8=out8, iterations=iterations, **guide_kw(s, GUIDES, True))
        torch.cuda.synchronize()
        assert bool((big32[:64] == -7.0).all()) and bool((big32[64 + n * 4:] == -7.0).all())
        assert bool((big8[:64] == 0x5A).all()) and bool((big8[64 + n * 4:] == 0x5A).all())
        assert_same((out.cpu().numpy(), out8.cpu().numpy()), dl.denoise(s["color"], iterations=iterations, **guide_kw(s, GUIDES, False)), "guarded outputs")


# ---- 3: the output stage against a render call, and the whole chain ---------------------------------------------------------
_SCENES = {}


def rendered(gpu, name):
    if name not in _SCENES:
        _SCENES[name] = DeviceScene(make_desc(name), Config(), builder=abi.BUILDER_SAH)
        _SCENES[name].finish()
    return _SCENES[name]


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("name", ["box", "cornell_quad"])
def test_output_stage_is_a_render_calls(gpu, name, spp):
    """a frame rendered with gamma 1 and passed through denoise(iterations=0, gamma=2.2) is the frame rendered with gamma 2.2:
    gamma and quantisation are finalize_pixel's, without a tolerance"""
    import torch
    scene = rendered(gpu, name)
    w, h = 61, 37
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=spp, gamma=2.2)
    want8, want32, _ = scene.render(cfg, w, h)
    _, linear, _ = scene.render(Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=spp, gamma=1.0), w, h)
    assert not np.array_equal(linear, want32)
    out, out8 = scene.denoise(dev(linear), iterations=0, gamma=2.2, rgba8=True)
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), out8.cpu().numpy()), (want32, want8), f"{name} spp {spp}")


@pytest.mark.parametrize("name", ["cornell_quad", "box"])
def test_render_denoised_is_the_chain_and_the_literal(gpu, name):
    import torch
    scene = rendered(gpu, name)
    w, h = 61, 37
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0)
    got, got8 = scene.render_denoised(cfg, w, h, rgba8=True, sigma_plane=SIGMA_PLANE)
    color = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    scene.render_device(cfg, w, h, 0, color.data_ptr())
    g = scene.gbuffer(cfg, w, h, want=("color", "normal", "point", "material"))
    kw = dict(albedo=g["color"], normal=g["normal"], point=g["point"], id=g["material"], sigma_plane=SIGMA_PLANE)
    chain, chain8 = scene.denoise(color, rgba8=True, **kw)
    torch.cuda.synchronize()
    got, chain = (got.cpu().numpy(), got8.cpu().numpy()), (chain.cpu().numpy(), chain8.cpu().numpy())
    assert_same(got, chain, f"{name}: render_denoised against the chain")
    host = {k: v.cpu().numpy() for k, v in kw.items() if k != "sigma_plane"}
    host["id"] = host["id"].view(np.uint32)
    color_h = color.cpu().numpy()
    assert_same(got, dl.denoise(color_h, sigma_plane=SIGMA_PLANE, **host), f"{name}: render_denoised against the literal")
    miss = g["prim"].cpu().numpy().view(np.uint32) == NONE
    print(f"{name}: {miss.sum()} miss pixels of {miss.size}")
    assert not host["normal"][miss].any()
    assert np.array_equal(bits(got[0][miss]), bits(color_h[miss])), "a miss passes through"
    assert (bits(got[0]) != bits(color_h)).any(-1)[~miss].mean() > 0.5   # ... and what was hit was filtered
    if name == "box":
        assert miss.sum() > 100
    # the same chain with the frame's gamma: render_denoised forces gamma 1 on the render and hands config.gamma to the filter
    cfg22 = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=2.2)
    got22, got22_8 = scene.render_denoised(cfg22, w, h, rgba8=True, sigma_plane=SIGMA_PLANE)
    chain22, chain22_8 = scene.denoise(color, rgba8=True, gamma=2.2, **kw)
    torch.cuda.synchronize()
    assert_same((got22.cpu().numpy(), got22_8.cpu().numpy()), (chain22.cpu().numpy(), chain22_8.cpu().numpy()), f"{name}: gamma 2.2")
    assert not np.array_equal(got22.cpu().numpy(), got[0])


# ---- 4: errors --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(gpu, ds):
    import torch
    w, h = 16, 8
    color = torch.rand((h, w, 4), dtype=torch.float32, device="cuda")
    guide3 = torch.rand((h, w, 3), dtype=torch.float32, device="cuda")
    out = torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda")
    out8 = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device="cuda")

    def call(scene=ds.handle, null_d=False, tile_parts=0, o_fields=None, **fields):
        d = abi.RaycaDenoise()
        d.width, d.height, d.iterations, d.normal_power_log2, d.sigma_color, d.sigma_plane, d.gamma = w, h, 2, 7, 4.0, SIGMA_PLANE, 1.0
        d.color, d.rgba32f_out, d.rgba8_out = color.data_ptr(), out.data_ptr(), out8.data_ptr()
        for k, v in fields.items():
            setattr(d, k, v)
        o = abi.RaycaRenderOptions()
        o.tile.parts = tile_parts
        for k, v in (o_fields or {}).items():
            setattr(o, k, v)
        return gpu.rayca_hip_denoise_device(scene, C.byref(o), None if null_d else C.byref(d), None)

    cases = [dict(scene=None), dict(null_d=True), dict(color=None), dict(rgba32f_out=None, rgba8_out=None), dict(width=0), dict(height=0),
             dict(width=65536, height=65536), dict(iterations=9), dict(normal_power_log2=11), dict(point=guide3.data_ptr()),
             dict(point=guide3.data_ptr(), normal=guide3.data_ptr(), sigma_plane=0.0), dict(point=guide3.data_ptr(), normal=guide3.data_ptr(), sigma_plane=-1.0),
             dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(reserved=1), dict(color=color.data_ptr() + 4),
             dict(o_fields=dict(context=8)), dict(o_fields=dict(traversal=1)), dict(o_fields=dict(collect_stats=1)), dict(o_fields=dict(engine=1)),
             dict(o_fields=dict(camera_rays=1)), dict(o_fields=dict(reserved=1)), dict(tile_parts=2)]
    for kw in cases:
        assert call(**kw) == abi.ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((out8 == 0x5A).all())   # nothing of the above wrote anything
    assert call(point=guide3.data_ptr(), normal=guide3.data_ptr()) == abi.OK
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())
    with pytest.raises(RaycaError) as e:
        ds.denoise(color, iterations=9)
    assert e.value.code == abi.ERR_BAD_ARG and "iterations" in lib.last_error()
    with pytest.raises(ValueError):
        ds.denoise(color, normal=guide3, point=guide3)   # (no sigma_plane)
    with pytest.raises(ValueError):
        ds.denoise(color[:, :, :3])
    with pytest.raises(TypeError):
        ds.denoise(color.double())
    # an empty scene is no error: the scene is not read
    empty = M.Scene()
    empty.push_model(M.create_default_model())
    es = DeviceScene(flatten(empty), Config())
    got = es.denoise(color, iterations=2)
    want = ds.denoise(color, iterations=2)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    es.close()


def test_scenes_are_closed(gpu):
    for s in _SCENES.values():
        s.close()
    _SCENES.clear()
