"""NEE samples that cannot contribute are not traced (trace_core.inc nee_irrelevant: the candidate contribution is zero in
r, g, b and its alpha finite, so "lit" and "not lit" give the same bits).  RAYCA_NEE_SKIP=0, read when a scene is created,
turns the skip off: frames must be bit-equal with and without it on every engine, rays_shadow keeps counting every sample
(the reference's count), only the traversal work drops; exhaustive traversal keeps tracing every sample.

The count tests use RAYCA_BUILDER_REFERENCE scenes: there every engine traverses the same binary nodes, so boxes_tested
means the same thing on all of them.  Frames are compared with the oracle at the bar of the parity tests (1e-4 per channel
in the displayable range, relative above it, <= 1 LSB after quantisation: device libm vs glibc)."""
import math
import os

import numpy as np
import pytest

import oracle_lib as ol
from rayca_amd import Config, DeviceScene, IntegratorStrategy, Light, PbrMaterial, SamplerStrategy, Trs, abi, flatten, scenes

pytestmark = pytest.mark.gpu
I, S = IntegratorStrategy, SamplerStrategy
TOL = 1e-4
ENV = "RAYCA_NEE_SKIP"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_scene(desc, skip, builder):
    """A scene created with the skip on or off (the variable is read by rayca_hip_scene_create)."""
    old = os.environ.get(ENV)
    os.environ[ENV] = "1" if skip else "0"
    try:
        return DeviceScene(desc, Config(), builder=builder)
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old


_cache = {}


def trio(name, make, builder):
    """(scene with the skip on, scene with it off, oracle) -- made once per scene and builder, shared by the tests."""
    key = (name, builder)
    if key not in _cache:
        desc = flatten(make())
        _cache[key] = (device_scene(desc, True, builder), device_scene(desc, False, builder), ol.OracleScene(desc, Config()), desc)
    return _cache[key][:3]


def assert_close(f32, of32, u8, ou8):
    with np.errstate(invalid="ignore"):
        d = np.abs(f32 - of32) / np.maximum(1.0, np.abs(of32))
    d = np.where(np.isnan(f32) & np.isnan(of32), 0.0, np.where(np.isnan(d), np.inf, d))
    assert d.max() <= TOL, f"max diff {d.max():.3e} at {np.unravel_index(d.argmax(), d.shape)}"
    assert np.abs(u8.astype(int) - ou8.astype(int)).max() <= 1


def two_quads(light):
    """Two 2x2-quad panels side by side, both turned towards the camera: the left one also faces a light on the left, the
    right one faces away from it.  light: "point", "quad" (a quad light on the left whose front looks at the panels: the
    right panel still faces away from it), "behind" (the same quad light turned round: both panels see its other side).
    The quad lights take two samples per vertex: a lane that skips one goes on with the next."""
    c, s = 0.5, math.sqrt(3.0) / 2.0
    Y = np.array([0, 1, 0], np.float32)
    left, right = scenes._MeshBuilder(), scenes._MeshBuilder()
    left.grid((-1.1, -0.5, -s / 2), np.array([c, 0, s], np.float32), Y, 2, 2)      # normal (-s, 0, c): towards -x and the camera
    right.grid((0.6, -0.5, s / 2), np.array([c, 0, -s], np.float32), Y, 2, 2)      # normal (+s, 0, c): towards +x and the camera
    parts = [(left.mesh(), PbrMaterial(color=(0.8, 0.7, 0.6, 1), roughness_factor=0.9)),
             (right.mesh(), PbrMaterial(color=(0.6, 0.7, 0.8, 1), roughness_factor=0.5))]
    lights = [((-3.0, 0.2, 0.5), 6.0)] if light == "point" else []
    scene = scenes._single_model_scene(parts, Trs(translation=(0.0, 0.0, 3.0)), math.pi / 4, lights)
    if light != "point":
        model = scene.models[0]
        # ab x ac = +x for "quad" (towards the panels), -x for "behind"
        ab, ac = ((0.0, 0.4, 0.0), (0.0, 0.0, 0.4)) if light == "quad" else ((0.0, 0.0, 0.4), (0.0, 0.4, 0.0))
        lt = model.lights.push(Light.quad(ab=ab, ac=ac, intensity=6.0))
        model.root.children.append(model.nodes.push(scenes.Node(light=lt, trs=Trs(translation=(-3.0, 0.0, 0.3)))))
    return scene


def dark_cornell():
    """The Cornell room with its light at intensity 0: no sample can contribute."""
    scene = scenes.cornell_scene()
    for lt in scene.models[0].lights:
        lt.set_intensity(0.0)
    return scene


def light_in_the_wall():
    """A 2x2-quad wall in the plane z = 0, seen head-on, with a point light in the wall's own plane (on its middle vertex):
    n . omega is 0 up to the rounding of the hit point, so samples that clamp to 0 (skipped) and samples a few ulps above
    it (traced) lie side by side.  The distance-0 sample itself cannot be reached by a camera ray here: a ray through the
    middle vertex has zero x and y components, and such a ray misses the root box (the reference's zero-direction quirk,
    tests/test_gpu_parity.py); the non-finite samples of non_finite_light() below do not depend on an exact hit point."""
    wall = scenes._MeshBuilder()
    wall.grid((-1, -1, 0), np.array([2, 0, 0], np.float32), np.array([0, 2, 0], np.float32), 2, 2)
    return scenes._single_model_scene([(wall.mesh(), PbrMaterial(color=(0.7, 0.7, 0.7, 1), roughness_factor=1.0))],
                                      Trs(translation=(0.0, 0.0, 3.0)), math.pi / 4, [((0.0, 0.0, 0.0), 2.0)])


def non_finite_light(kind):
    """The two panels with their point light made non-finite.  "nan_rgb": intensity inf, so on the panel that faces away
    the candidate contribution is inf * (n . omega = 0) = NaN in r, g, b.  "inf_alpha": the light's colour has alpha inf,
    so on that panel the contribution is (0, 0, 0, inf): zero where the rule looks first, and `0 * inf` = NaN once it is
    added as lit.  With a finite light exactly these samples are skipped (test_two_panels_one_facing_away); here the guard
    must leave every one of them traced."""
    scene = two_quads("point")
    for lt in scene.models[0].lights:
        if kind == "nan_rgb":
            lt.set_intensity(float("inf"))
        else:
            lt.color = (1.0, 1.0, 1.0, float("inf"))
    return scene


CORNELL = [
    # (config, engine, compared with the oracle?)  Depth 1 has no bounce directions from acos / sin / cos: the parity tests
    # hold it to tolerance without exceptions; so does test_gpu_general.py for the light_samples=2 frame of the stack machine.
    (Config(max_depth=1), abi.ENGINE_FUSED, True),
    (Config(max_depth=3, seed=3), abi.ENGINE_FUSED, False),
    (Config(max_depth=1), abi.ENGINE_WAVEFRONT, True),
    (Config(max_depth=3, seed=3), abi.ENGINE_WAVEFRONT, False),
    (Config(max_depth=3, light_samples=2, seed=8), abi.ENGINE_AUTO, True),           # k_general: several samples with bounces
]


@pytest.mark.parametrize("case", range(len(CORNELL)))
def test_frames_are_bit_equal_with_and_without_the_skip(gpu, case):
    cfg, engine, against_oracle = CORNELL[case]
    on, off, orc = trio("cornell", scenes.cornell_scene, abi.BUILDER_SAH)
    u8a, fa, sa = on.render(cfg, 128, 72, engine=engine, collect_stats=True)
    u8b, fb, sb = off.render(cfg, 128, 72, engine=engine, collect_stats=True)
    assert np.array_equal(bits(fa), bits(fb)), f"max abs diff {np.abs(fa - fb).max():.3e}"
    assert np.array_equal(u8a, u8b)
    for k in ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded"):
        assert sa[k] == sb[k], k
    assert sa["boxes_tested"] < sb["boxes_tested"]      # the short box's front looks away from the light behind it
    assert float(fa[..., :3].max()) > 0.0
    if against_oracle:
        ou8, of32, ost = orc.render(cfg, 128, 72)
        assert_close(fa, of32, u8a, ou8)
        assert sa["rays_shadow"] == ost["rays_shadow"]


def test_mis_records_a_skipped_sample(gpu):
    """MIS on the stack machine keeps every light sample for its weights, skipped or not (the Cornell room's Pbr materials
    reach a todo!() of the reference under MIS: the quad-light room of test_gpu_general.py instead)."""
    import test_gpu_general as G
    on, off, _ = trio("room_phong", lambda: G.quad_light_room("phong"), abi.BUILDER_SAH)
    cfg = Config(max_depth=2, light_samples=2, direct_sampler=S.Mis, indirect_sampler=S.Brdf, seed=10)
    u8a, fa, sa = on.render(cfg, 96, 72, collect_stats=True)
    u8b, fb, sb = off.render(cfg, 96, 72, collect_stats=True)
    assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(u8a, u8b)
    for k in ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded"):
        assert sa[k] == sb[k], k
    assert sa["boxes_tested"] <= sb["boxes_tested"]


@pytest.mark.parametrize("light", ["point", "quad", "behind"])
def test_two_panels_one_facing_away(gpu, light):
    on, off, orc = trio("two_quads_" + light, lambda: two_quads(light), abi.BUILDER_REFERENCE)
    cfg = Config(max_depth=1, light_samples=2) if light != "point" else Config(max_depth=1)
    ou8, of32, ost = orc.render(cfg, 64, 64)
    boxes = {}
    for engine in (abi.ENGINE_FUSED, abi.ENGINE_WAVEFRONT):
        u8a, fa, sa = on.render(cfg, 64, 64, engine=engine, collect_stats=True)
        u8b, fb, sb = off.render(cfg, 64, 64, engine=engine, collect_stats=True)
        assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(u8a, u8b), engine
        assert_close(fa, of32, u8a, ou8)
        assert sa["rays_shadow"] == sb["rays_shadow"] == ost["rays_shadow"] > 0
        assert sa["boxes_tested"] < sb["boxes_tested"], engine
        assert sa["triangles_tested"] <= sb["triangles_tested"]
        boxes[engine] = (sa["boxes_tested"], sb["boxes_tested"])
    assert boxes[abi.ENGINE_FUSED] == boxes[abi.ENGINE_WAVEFRONT]
    if light == "point":
        assert float(fa[:, :32, :3].max()) > 0.0        # the left panel is lit (no emissive surface stands for the quad lights)


def test_every_sample_skipped_leaves_the_camera_rays_alone(gpu):
    on, off, orc = trio("dark_cornell", dark_cornell, abi.BUILDER_REFERENCE)
    cfg = Config(max_depth=1)
    ou8, of32, ost = orc.render(cfg, 128, 72)
    for engine in (abi.ENGINE_FUSED, abi.ENGINE_WAVEFRONT):
        _, _, flat = on.render(Config(integrator=I.Flat), 128, 72, engine=engine, collect_stats=True)
        u8a, fa, sa = on.render(cfg, 128, 72, engine=engine, collect_stats=True)
        u8b, fb, sb = off.render(cfg, 128, 72, engine=engine, collect_stats=True)
        assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(u8a, u8b)
        assert_close(fa, of32, u8a, ou8)
        assert sa["rays_shadow"] == sb["rays_shadow"] == ost["rays_shadow"] == sa["hits_shaded"] > 0
        assert sa["boxes_tested"] == flat["boxes_tested"] and sa["triangles_tested"] == flat["triangles_tested"]
        assert sb["boxes_tested"] > flat["boxes_tested"]


@pytest.mark.parametrize("kind", ["nan_rgb", "inf_alpha"])
def test_non_finite_sample_is_still_traced(gpu, kind):
    on, off, _ = trio("non_finite_" + kind, lambda: non_finite_light(kind), abi.BUILDER_REFERENCE)
    cfg = Config(max_depth=1)
    for engine in (abi.ENGINE_FUSED, abi.ENGINE_WAVEFRONT, abi.ENGINE_GENERAL):
        _, _, flat = on.render(Config(integrator=I.Flat), 64, 64, engine=engine, collect_stats=True)
        u8a, fa, sa = on.render(cfg, 64, 64, engine=engine, collect_stats=True)
        u8b, fb, sb = off.render(cfg, 64, 64, engine=engine, collect_stats=True)
        assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(u8a, u8b), engine
        assert not np.isfinite(fb[..., :3]).all()       # the light really is non-finite
        # no sample is skipped: the traversal work with the skip on is the work with it off, shadow rays included
        assert sa["rays_shadow"] == sb["rays_shadow"] == sa["hits_shaded"] > 0
        assert sa["boxes_tested"] == sb["boxes_tested"] >= flat["boxes_tested"] + sa["rays_shadow"], engine
        assert sa["triangles_tested"] == sb["triangles_tested"]


def test_light_in_the_surface_plane(gpu):
    on, off, _ = trio("light_in_the_wall", light_in_the_wall, abi.BUILDER_REFERENCE)
    cfg = Config(max_depth=1)
    for engine in (abi.ENGINE_FUSED, abi.ENGINE_WAVEFRONT):
        u8a, fa, sa = on.render(cfg, 65, 65, engine=engine, collect_stats=True)
        u8b, fb, sb = off.render(cfg, 65, 65, engine=engine, collect_stats=True)
        assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(u8a, u8b)
        assert sa["boxes_tested"] <= sb["boxes_tested"]
        assert sa["rays_shadow"] == sb["rays_shadow"] == sa["hits_shaded"]


@pytest.mark.parametrize("builder", [abi.BUILDER_REFERENCE, abi.BUILDER_SAH])
def test_exhaustive_traversal_traces_every_sample(gpu, builder):
    on, off, _ = trio("cornell", scenes.cornell_scene, builder)
    for cfg in (Config(max_depth=1), Config(max_depth=3, seed=3)):
        u8a, fa, sa = on.render(cfg, 128, 72, traversal=abi.TRAVERSAL_EXHAUSTIVE, collect_stats=True)
        u8b, fb, sb = off.render(cfg, 128, 72, traversal=abi.TRAVERSAL_EXHAUSTIVE, collect_stats=True)
        assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(u8a, u8b)
        for k in ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded", "boxes_tested", "triangles_tested"):
            assert sa[k] == sb[k], k
