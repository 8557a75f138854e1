"""rayca_hip_upsample_device (DeviceScene.upsample, .render_upsampled, Film.resolve(upsample=)) on the GPU.

Every comparison of the pass is bit for bit (the float words as uint32, on rgba32f_out, rgba8_out and weight_out): against the
literal numpy-float32 restatement (tests/upsample_literal.py -- the pass is +, -, x, /, floor and max only, each rounded once, so
the restatement has the kernel's bits), against the denoiser's output stage for a gamma other than 1, and between the ways of
making one call (another stream, another frame context, through render_upsampled, through Film)."""
import dataclasses
import itertools
import os

import numpy as np
import pytest

import upsample_literal as ul
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, abi, flatten, scenes
from rayca_amd import model as M
from rayca_amd import sdtf

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
SIGMA_PLANE = 0.1
SCALES = [1, 2, 3, 4, 8]
LOW_SIZES = [(1, 1), (31, 19), (21, 13), (33, 3), (17, 5)]   # (width, height): partial tiles both ways; 33 x 2 = 66 crosses the 64-pixel tile
SUBSETS = [tuple(g for g, on in zip(ul.GUIDES, flags) if on) for flags in itertools.product((False, True), repeat=4)
           if not (flags[2] and not flags[1])]   # every legal subset of the guide pairs: point needs normal


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


_CASES = {}


def case(low_width, low_height, scale):
    """a size's two views with the special values, made once and shared read-only: the NaN and inf pixels of the scene, a -0.0
    channel, a zero albedo at one pixel of either view, a zero colour under a zero albedo"""
    key = (low_width, low_height, scale)
    if key not in _CASES:
        low, high, _ = ul.synthetic_pair(low_width, low_height, scale)
        at = lambda d, y, x: (y % d["id"].shape[0], x % d["id"].shape[1])
        low["color"][at(low, 7, 3)][1] = F(-0.0)
        low["albedo"][at(low, 8, 6)][:3] = 0.0
        low["albedo"][at(low, 11, 14)][:3] = 0.0
        low["color"][at(low, 11, 14)][:3] = 0.0
        high["albedo"][at(high, 17, 9)][:3] = 0.0
        high["albedo"][at(high, 12, 30)][0] = 0.0
        for d in (low, high):
            for a in d.values():
                a.setflags(write=False)
        _CASES[key] = (low, high)
    return _CASES[key]


def dev(a):
    import torch
    a = np.array(a)   # (a writable copy: the shared frames are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def dev_guides(view, which):
    return {g: dev(view[g]) for g in which}


def assert_same(got, want, what):
    for name, g, w in zip(("rgba32f", "rgba8", "weight"), got, want):
        g, w = g.reshape(w.shape[0], w.shape[1], -1), w.reshape(w.shape[0], w.shape[1], -1)
        same = (bits(g) == bits(w)) if g.dtype != np.uint8 else (g == w)
        bad = np.argwhere(~same.all(-1))
        assert bad.size == 0, f"{what}: {name}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def run(ds, low, high, scale, which, *, normal_power_log2=7, gamma=1.0, **kw):
    import torch
    out = ds.upsample(dev(low["color"]), scale, low=dev_guides(low, which), high=dev_guides(high, which), sigma_plane=SIGMA_PLANE,
                      normal_power_log2=normal_power_log2, gamma=gamma, rgba8=True, weight=True, **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in out)


def literal(low, high, scale, which, normal_power_log2=7):
    return ul.upsample(low["color"], scale, low=ul.guides_of(low, which), high=ul.guides_of(high, which), sigma_plane=SIGMA_PLANE,
                       normal_power_log2=normal_power_log2)


# ---- 1: against the literal ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_every_size_and_scale_equals_the_literal(ds, scale):
    """one pixel; partial tiles in both directions; an output row that crosses the tile width; with every guide and with none"""
    for low_width, low_height in LOW_SIZES:
        low, high = case(low_width, low_height, scale)
        for which in (ul.GUIDES, ()):
            assert_same(run(ds, low, high, scale, which), literal(low, high, scale, which), f"{low_width} x {low_height} x {scale}, guides {which}")


@pytest.mark.parametrize("which", SUBSETS, ids=["+".join(s) or "none" for s in SUBSETS])
def test_every_legal_subset_of_the_guides_equals_the_literal(ds, which):
    """... with normal_power_log2 0 and 7, at an even and an odd scale; gamma 2.2 against the denoiser's output stage on the
    literal's gamma-1 frame (iterations=0: finalize_pixel alone, which is what this pass calls)"""
    import torch
    for (low_width, low_height, scale), power in itertools.product(((31, 19, 2), (21, 13, 3)), (0, 7)):
        low, high = case(low_width, low_height, scale)
        want = literal(low, high, scale, which, power)
        what = f"{low_width} x {low_height} x {scale}, guides {which}, normal_power_log2 {power}"
        assert_same(run(ds, low, high, scale, which, normal_power_log2=power), want, what)
        want22, want22_8 = ds.denoise(dev(want[0]), iterations=0, gamma=2.2, rgba8=True)
        torch.cuda.synchronize()
        assert_same(run(ds, low, high, scale, which, normal_power_log2=power, gamma=2.2), (want22.cpu().numpy(), want22_8.cpu().numpy(), want[2]), what + ", gamma 2.2")
        assert not np.array_equal(bits(want22.cpu().numpy()), bits(want[0]))


def test_the_special_values_are_where_the_specification_puts_them(ds):
    """what the bit-for-bit comparisons cover, looked at once: the fallback on the thin feature (weight 0, finite colour), the NaN
    that passes through at an odd scale, a zero albedo (the 1e-3 floor at either resolution)"""
    low, high = case(21, 13, 3)
    out, _, weight = run(ds, low, high, 3, ul.GUIDES)
    thin = high["thin"]
    assert thin.sum() >= 10 and not weight[thin].any() and np.isfinite(out[thin]).all()
    py, px = ul.NAN_PIXELS[0]
    assert np.isnan(out[(py % 13) * 3 + 1, (px % 21) * 3 + 1, 0]) and weight[(py % 13) * 3 + 1, (px % 21) * 3 + 1] == 0
    assert np.isfinite(out).all(-1).sum() == out.shape[0] * out.shape[1] - len(ul.NAN_PIXELS)
    near_nan = np.zeros_like(thin)   # (a pixel with a NaN tap may have lost the only tap that agreed with it)
    for py, px in ul.NAN_PIXELS:
        near_nan[max(0, (py % 13 - 1) * 3):(py % 13 + 2) * 3, max(0, (px % 21 - 1) * 3):(px % 21 + 2) * 3] = True
    assert (weight[~thin & ~near_nan] > 0).all()


def test_strided_inputs_equal_contiguous_ones(ds):
    """an input that is not contiguous reaches the kernel as a contiguous copy: the contiguous call's bits"""
    import torch
    from strided import strided
    low, high = case(65, 5, 2)
    want = run(ds, low, high, 2, ul.GUIDES)
    out = ds.upsample(strided(dev(low["color"])), 2, low=strided(dev_guides(low, ul.GUIDES)), high=strided(dev_guides(high, ul.GUIDES)),
                      sigma_plane=SIGMA_PLANE, rgba8=True, weight=True)
    torch.cuda.synchronize()
    assert_same(tuple(x.cpu().numpy() for x in out), want, "strided inputs")


def test_a_callers_stream_another_context_and_the_statistics(ds):
    import torch
    low, high = case(31, 19, 2)
    want = literal(low, high, 2, ul.GUIDES)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = run(ds, low, high, 2, ul.GUIDES, stream=stream, context=3)
    assert_same(got, want, "a caller's stream, context 3")
    *got, stats = run(ds, low, high, 2, ul.GUIDES, want_stats=True)
    assert_same(got, want, "with statistics")
    assert stats["kernel_launches"] == 1 and stats["class_launches"][abi.KERNEL_OTHER] == 1 and stats["kernel_ms"] > 0
    assert stats["class_ms"][abi.KERNEL_OTHER] == stats["kernel_ms"] and stats["rays_primary"] == 0
    # outputs the caller provides; the float output alone; the uint8 output through the C ABI's rule (at least one of the two)
    out = torch.full((38, 62, 4), -7.0, device="cuda")
    assert ds.upsample(dev(low["color"]), 2, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(ul.upsample(low["color"], 2)[0]))


def test_errors_reach_the_caller(ds):
    import torch
    from rayca_amd.lib import RaycaError
    low, high = case(31, 19, 2)
    color = dev(low["color"])
    with pytest.raises(ValueError, match="normal"):
        ds.upsample(color, 2, low=dev_guides(low, ("normal",)))
    with pytest.raises(ValueError, match="sigma_plane"):
        ds.upsample(color, 2, low=dev_guides(low, ("normal", "point")), high=dev_guides(high, ("normal", "point")))
    with pytest.raises(ValueError, match="scale"):
        ds.upsample(color, 9)
    with pytest.raises(RaycaError, match="point needs normal"):
        ds.upsample(color, 2, low=dev_guides(low, ("point",)), high=dev_guides(high, ("point",)), sigma_plane=SIGMA_PLANE)
    with pytest.raises(RaycaError, match="gamma"):
        ds.upsample(color, 2, gamma=0.0)
    with pytest.raises(ValueError, match="shape"):
        ds.upsample(color, 2, low=dev_guides(low, ("normal",)), high=dev_guides(low, ("normal",)))
    torch.cuda.synchronize()


# ---- 2: real scenes ------------------------------------------------------------------------------------------------------------
_SCENES = {}
LOW_W, LOW_H, SCALE = 64, 36, 2
WANT = ("color", "normal", "point", "material")


def rendered(gpu, name):
    """(scene, the descriptor it was made from) -- a test that moves the camera puts it back"""
    if name not in _SCENES:
        desc = make_desc(name)
        _SCENES[name] = (DeviceScene(desc, Config(), builder=abi.BUILDER_SAH), desc)
        _SCENES[name][0].finish()
    return _SCENES[name]


def host(result):
    return tuple(x.cpu().numpy() for x in result)


def composed(scene, color, scale, gamma, sigma_plane=0.1):
    """upsample() of `color` against the two G-buffers of the scene's camera, made with the public calls"""
    one = Config(samples_per_pixel=1)
    h, w = color.shape[:2]
    low, high = scene.gbuffer(one, w, h, want=WANT), scene.gbuffer(one, w * scale, h * scale, want=WANT)
    return scene.upsample(color, scale, low=low, high=high, sigma_plane=sigma_plane, gamma=gamma, rgba8=True, weight=True), low, high


def test_render_upsampled_is_the_composition_of_the_public_calls(gpu):
    import torch
    scene, _ = rendered(gpu, "cornell_quad")
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=2.2, seed=5)
    got = scene.render_upsampled(cfg, LOW_W * SCALE, LOW_H * SCALE, SCALE, rgba8=True, weight=True)
    color = torch.empty((LOW_H, LOW_W, 4), dtype=torch.float32, device="cuda")
    scene.render_device(dataclasses.replace(cfg, gamma=1.0), LOW_W, LOW_H, 0, color.data_ptr())
    chain, low, high = composed(scene, color, SCALE, 2.2)
    torch.cuda.synchronize()
    assert_same(host(got), host(chain), "render_upsampled against the composition")
    assert got[0].shape == (LOW_H * SCALE, LOW_W * SCALE, 4) and float((got[2] > 0).float().mean()) > 0.9
    # ... and the composition against the literal at gamma 1, on the rendered frame and G-buffers
    lin = scene.upsample(color, SCALE, low=low, high=high, sigma_plane=0.1, rgba8=True, weight=True)
    torch.cuda.synchronize()
    names = dict(albedo="color", normal="normal", point="point", id="material")
    pick = lambda g: {k: (g[v].cpu().numpy().view(np.uint32) if k == "id" else g[v].cpu().numpy()) for k, v in names.items()}
    assert_same(host(lin), ul.upsample(color.cpu().numpy(), SCALE, low=pick(low), high=pick(high), sigma_plane=0.1), "the composition against the literal")
    # with the low frame denoised in between: the a-trous filter at low resolution with the low guides and gamma 1
    got_d = scene.render_upsampled(cfg, LOW_W * SCALE, LOW_H * SCALE, SCALE, denoise=True, rgba8=True, weight=True)
    den = scene.denoise(color.clone(), albedo=low["color"], normal=low["normal"], point=low["point"], id=low["material"], sigma_plane=0.1)
    chain_d, _, _ = composed(scene, den, SCALE, 2.2)
    torch.cuda.synchronize()
    assert_same(host(got_d), host(chain_d), "render_upsampled(denoise=True) against the composition")
    assert not np.array_equal(host(got_d)[0], host(got)[0])


@pytest.mark.parametrize("name", ["cornell_quad", "box"])
def test_a_flat_frame_comes_back_bit_for_bit(gpu, name):
    """The exactness argument on a real scene.  A Flat frame is BLACK + the surface's colour (tests/test_gpu_surface.py pins that
    against the oracle's `+`): at a hit with alpha 1 it has the bits of the albedo guide.  So every tap the guides let through
    demodulates to exactly 1 in a channel where its albedo is at least 1e-3 (x / x), the weighted mean of ones is exactly 1
    (sum and wsum add the same numbers in the same order), and the pixel is the full-size albedo -- the full-size Flat frame --
    whatever the weights were.  Asserted at every hit pixel with weight_out > 0 and all three albedo channels >= 1e-3, and
    channel by channel too: the Cornell room's walls are black to get_color() and the box is pure red, so the first form
    alone would look at few pixels (the id guide keeps a tap's material, and with it its zero channels, the pixel's own)."""
    import torch
    scene, _ = rendered(gpu, name)
    flat = Config(integrator=IntegratorStrategy.Flat, samples_per_pixel=1, gamma=1.0)
    big_w, big_h = LOW_W * SCALE, LOW_H * SCALE
    (out, _, weight), low, high = composed(scene, flat_frame(scene, flat, LOW_W, LOW_H), SCALE, 1.0)
    full = flat_frame(scene, flat, big_w, big_h)
    torch.cuda.synchronize()
    out, weight, full, albedo = out.cpu().numpy(), weight.cpu().numpy(), full.cpu().numpy(), high["color"].cpu().numpy()
    hit = high["prim"].cpu().numpy().view(np.uint32) != np.uint32(0xFFFFFFFF)
    assert (albedo[hit][:, 3] == 1).all()
    channel_ok = (hit & (weight > 0))[..., None] & (albedo[..., :3] >= F(1e-3))
    ok = channel_ok.all(-1)
    print(f"{name} {big_w} x {big_h}: {hit.sum()} hits, {ok.sum()} of them with weight > 0 and albedo >= 1e-3 in every channel, {channel_ok.any(-1).sum()} in some channel")
    assert channel_ok.any(-1).sum() > 100 and (ok.sum() > 100 or name == "box")   # (not vacuous)
    bad = np.argwhere((bits(out) != bits(full)).any(-1) & ok)
    assert bad.size == 0, f"{len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {out[tuple(bad[0])]} want {full[tuple(bad[0])]}"
    bad = np.argwhere((bits(out[..., :3]) != bits(full[..., :3])) & channel_ok)
    assert bad.size == 0, f"{len(bad)} channels differ, first (y, x, channel) {bad[:4].tolist()}"
    assert np.array_equal(out[..., 3][hit & (weight > 0)], full[..., 3][hit & (weight > 0)])


def flat_frame(scene, cfg, w, h):
    import torch
    color = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    scene.render_device(cfg, w, h, 0, color.data_ptr())
    return color


def camera_node(desc):
    return next(n for n in desc._nodes[:desc.c.node_count] if n.camera != abi.NONE)


def test_film_resolve_upsampled_is_its_composition_through_a_camera_move(gpu):
    import torch
    scene, desc = rendered(gpu, "cornell_quad")
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=2.2, seed=11)
    film = Film(scene, LOW_W, LOW_H)

    def check(what):
        got = film.resolve(upsample=SCALE, rgba8=True, upsample_kw=dict(weight=True))
        chain, low, _ = composed(scene, film.color, SCALE, 2.2)
        got_d = film.resolve(upsample=SCALE, denoise=True, rgba8=True, upsample_kw=dict(weight=True))
        den = scene.denoise(film.color, **film.gbuffer(), sigma_plane=0.1)
        chain_d, _, _ = composed(scene, den, SCALE, 2.2)
        torch.cuda.synchronize()
        assert_same(host(got), host(chain), what)
        assert_same(host(got_d), host(chain_d), what + ", denoised")
        assert got[0].shape == (LOW_H * SCALE, LOW_W * SCALE, 4) and film.color.shape == (LOW_H, LOW_W, 4)

    film.add(cfg)
    check("first frame")
    cam = camera_node(desc)
    was = (tuple(cam.trs.translation), tuple(cam.trs.rotation))
    try:
        cam.trs.translation[:] = (was[0][0] + 0.04, was[0][1] + 0.015, was[0][2] - 0.02)
        scene.update(desc)
        film.add(cfg)
        check("after a camera move")
    finally:
        cam.trs.translation[:], cam.trs.rotation[:] = was
        scene.update(desc)
