"""The resident draw() on the MI355X: rayca_hip_renderer_draw reuses, updates or rebuilds the scene of the previous call, and
whichever it does the frame is bit-identical (RGBA8 and RGBA32F) to that of a scene created from the same descriptor with the
same builder.  The only timing-related facts asserted are structural: a reused or updated draw spent nothing on a build."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import test_gpu_fullsize as fullsize
from parity_report import check_outliers
from rayca_amd import (Config, DeviceScene, Image, IntegratorStrategy, Renderer, SoftRenderer, abi, flatten, scenes)
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
FLAT = Config(integrator=IntegratorStrategy.Flat)
DEPTH2 = Config(max_depth=2, seed=3)
bits = fullsize.bits


def fresh_frame(desc, cfg, w=W, h=H, builder=abi.BUILDER_SAH, **opts):
    ds = DeviceScene(desc, cfg, builder=builder)
    try:
        u8, f32, _ = ds.render(cfg, w, h, **opts)
    finally:
        ds.close()
    return u8, f32


def assert_same_frame(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: RGBA8 differs"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: RGBA32F differs"


def assert_no_build(info, builds):
    assert info["ms"]["build"] == 0.0 and info["builds"] == builds


def nodes(desc):
    return desc._nodes[:desc.c.node_count]


def node_with(desc, field):
    return next(n for n in nodes(desc) if getattr(n, field) != abi.NONE)


def place_camera(desc, k, centre, radius):
    """pose k of eight: yaw 45 deg * k on a circle round `centre`, looking at it; yfov pi/4 and pi/3 in turn"""
    cam = node_with(desc, "camera")
    th = math.radians(45.0 * k)
    cam.trs.translation[:] = (centre[0] + radius * math.sin(th), centre[1], centre[2] + radius * math.cos(th))
    cam.trs.rotation[:] = (0.0, math.sin(th / 2), 0.0, math.cos(th / 2))
    desc._cameras[cam.camera].yfov_radians = math.pi / 4 if k % 2 == 0 else math.pi / 3


def test_same_descriptor_three_times(gpu):
    desc = flatten(scenes.cornell_scene())
    r = Renderer()
    cfg = Config()      # the reference's default: Pathtracer, depth 5
    frames, actions = [], []
    for _ in range(3):
        u8, f32, st, info = r.draw(desc, cfg, 640, 360)
        frames.append((u8, f32))
        actions.append(info["action"])
    assert actions == [abi.DRAW_REBUILT, abi.DRAW_REUSED, abi.DRAW_REUSED]
    assert (info["builds"], info["updates"], info["reuses"]) == (1, 0, 2) and info["kept_bytes"] > desc.positions.nbytes
    assert_no_build(info, 1)
    assert st["rays_primary"] == 640 * 360 and r.scene is not None
    want = fresh_frame(desc, cfg, 640, 360)
    for f in frames:
        assert_same_frame(f, want, "cornell depth 5")
    # against the oracle, under the name (hence the bound) tests/test_gpu_parity.py checks this config with
    orc = ol.OracleScene(desc, Config())
    _, of32, _ = orc.render(cfg, 640, 360)
    check_outliers("cornell_640x360_depth5", frames[2][1], of32)
    # a second flatten of the same scene is the same descriptor in other memory: still reused; Flat is bit-exact to the oracle
    again = flatten(scenes.cornell_scene())
    u8, f32, _, info = r.draw(again, FLAT, 640, 360)
    assert info["action"] == abi.DRAW_REUSED
    ou8, of32, _ = orc.render(FLAT, 640, 360)
    assert np.array_equal(bits(f32), bits(of32)) and np.array_equal(u8, ou8)
    orc.close()
    r.close()


@pytest.mark.parametrize("cfg", [FLAT, DEPTH2], ids=["flat", "path2"])
def test_orbit_light_and_material_edits_are_updates(gpu, cfg):
    desc = flatten(scenes.cornell_scene())
    r = Renderer()
    _, _, _, info = r.draw(desc, cfg, W, H)
    assert info["action"] == abi.DRAW_REBUILT
    seen = []

    def step(what):
        u8, f32, _, info = r.draw(desc, cfg, W, H)
        assert info["action"] == abi.DRAW_UPDATED, what
        assert_no_build(info, 1)
        assert_same_frame((u8, f32), fresh_frame(desc, cfg), what)
        seen.append(f32)
        return info

    for k in range(8):
        place_camera(desc, k, (0.0, 1.0, 0.0), 0.8)
        step(f"pose {k}")
    assert any(not np.array_equal(seen[0], s) for s in seen[1:]), "the orbit shows"
    light = next(desc._lights[i] for i in range(desc.c.light_count) if desc._lights[i].kind == abi.LIGHT_POINT)
    light.color[:] = (1.0, 0.6, 0.3, 1.0)
    step("light colour")
    desc._materials[0].color[:] = (0.2, 0.3, 0.9, 1.0)      # floor, ceiling and back wall
    info = step("material colour")
    assert (info["builds"], info["updates"], info["reuses"]) == (1, 10, 0)
    if cfg is DEPTH2:
        assert not np.array_equal(seen[-3], seen[-2]), "the light edit shows in the shaded frame"
    assert not np.array_equal(seen[-2], seen[-1]), "the material edit shows"
    r.close()


def test_moved_mesh_node_rebuilds(gpu):
    desc = flatten(scenes.cornell_scene())
    r = Renderer()
    first = r.draw(desc, DEPTH2, W, H)
    node_with(desc, "mesh").trs.translation[0] += 0.3
    u8, f32, _, info = r.draw(desc, DEPTH2, W, H)
    assert info["action"] == abi.DRAW_REBUILT and info["builds"] == 2 and info["ms"]["build"] > 0.0
    assert_same_frame((u8, f32), fresh_frame(desc, DEPTH2), "moved mesh")
    assert not np.array_equal(first[1], f32)
    u8b, f32b, _, info = r.draw(desc, DEPTH2, W, H)
    assert info["action"] == abi.DRAW_REUSED
    assert_no_build(info, 2)
    assert_same_frame((u8b, f32b), (u8, f32), "the draw after the rebuild")
    r.close()


def test_a_descriptor_that_cannot_be_drawn_evicts_nothing(gpu):
    good = flatten(scenes.cornell_scene())
    r = Renderer()
    u8, f32, _, _ = r.draw(good, DEPTH2, W, H)
    # no camera: the error of scene_create + render on that descriptor
    blind = flatten(scenes.cornell_scene())
    node_with(blind, "camera").camera = abi.NONE
    with pytest.raises(RaycaError) as e:
        fresh_frame(blind, DEPTH2)
    with pytest.raises(RaycaError) as e2:
        r.draw(blind, DEPTH2, W, H)
    assert e2.value.code == e.value.code == abi.ERR_NO_CAMERA
    # a create that fails inside rayca_hip_scene_create: a mesh whose primitive range runs past the table
    broken = flatten(scenes.cornell_scene())
    broken._meshes[0].primitive_count += 1000
    with pytest.raises(RaycaError) as e:
        DeviceScene(broken, DEPTH2, builder=abi.BUILDER_SAH)
    with pytest.raises(RaycaError) as e2:
        r.draw(broken, DEPTH2, W, H)
    assert e2.value.code == e.value.code == abi.ERR_BAD_ARG
    u8b, f32b, _, info = r.draw(good, DEPTH2, W, H)
    assert info["action"] == abi.DRAW_REUSED and info["builds"] == 1
    assert_same_frame((u8b, f32b), (u8, f32), "the old scene survived")
    r.close()


def test_bvh_toggle_rebuilds(gpu):
    desc = flatten(scenes.cornell_scene())
    r = Renderer()
    on = r.draw(desc, Config(max_depth=2, seed=3, bvh=True), W, H)
    off_cfg = Config(max_depth=2, seed=3, bvh=False)
    u8, f32, _, info = r.draw(desc, off_cfg, W, H)
    assert info["action"] == abi.DRAW_REBUILT and info["builds"] == 2
    assert_same_frame((u8, f32), fresh_frame(desc, off_cfg), "bvh off")
    _, _, _, info = r.draw(desc, off_cfg, W, H)
    assert info["action"] == abi.DRAW_REUSED
    u8, f32, _, info = r.draw(desc, Config(max_depth=2, seed=3, bvh=True), W, H)
    assert info["action"] == abi.DRAW_REBUILT and info["builds"] == 3
    assert_same_frame((u8, f32), on[:2], "bvh on again")
    r.close()


def test_invalidate_and_reference_builder(gpu):
    desc = flatten(scenes.cornell_scene())
    r = Renderer(builder=abi.BUILDER_REFERENCE)
    a = r.draw(desc, DEPTH2, W, H)
    r.invalidate()
    b = r.draw(desc, DEPTH2, W, H)
    assert b[3]["action"] == abi.DRAW_REBUILT and b[3]["builds"] == 2
    assert_same_frame(b[:2], a[:2], "rebuilt on request")
    assert_same_frame(b[:2], fresh_frame(desc, DEPTH2, builder=abi.BUILDER_REFERENCE), "reference builder")
    assert r.draw(desc, DEPTH2, W, H)[3]["action"] == abi.DRAW_REUSED
    r.close()


def test_python_and_cpp_soft_renderer_draw_twice(gpu, tmp_path):
    import __graft_entry__ as g
    renderer = SoftRenderer(Config())
    images = [Image(256, 256), Image(256, 256)]
    for image in images:
        renderer.draw(scenes.box_scene(), image)       # a new Scene object per call
    assert renderer.last_draw["action"] == abi.DRAW_REUSED and renderer.last_draw["builds"] == 1
    assert renderer.last_stats["rays_primary"] == 256 * 256
    assert np.array_equal(images[0].data, images[1].data) and images[0].data[..., :3].any()
    renderer.close()
    exe = g.build_cpp_host("resident_draw")
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "box.gltf"), str(tmp_path)], check=True, capture_output=True, text=True).stdout
    lines = [l.split() for l in out.strip().splitlines()]
    assert lines == [["before", str(abi.NONE), "0", "0"], ["first", str(abi.DRAW_REBUILT), "1", "0"], ["second", str(abi.DRAW_REUSED), "1", "1"]]
    first, second = ((tmp_path / f"{n}.bin").read_bytes() for n in ("first", "second"))
    assert first == second == images[0].data.tobytes()


def test_atrium_1080p_rebuilt_reused_updated(gpu):
    """The benchmark scene at the benchmark's size, Flat and primary + shadow: the rows tests/test_gpu_fullsize.py checks
    against the oracle (every 27th of 1080), checked the same way on the frames of the three kinds of draw."""
    desc = flatten(scenes.atrium_scene())
    orc = ol.OracleScene(desc, Config(), build=ol.BUILD_BINNED)
    r = Renderer()
    tile = (0, 27, 1)
    depth1 = Config(max_depth=1)

    def against_the_oracle(what):
        ou8, of32, ost = orc.render(FLAT, 1920, 1080, tile=tile)
        u8, f32, st, _ = r.draw(desc, FLAT, 1920, 1080)
        assert ost["rows_rendered"] == 40
        assert np.array_equal(bits(f32[0::27][:40]), bits(of32)) and np.array_equal(u8[0::27][:40], ou8), what
        assert (f32[..., :3].sum(-1) > 0).mean() > 0.5
        ou8, of32, ost = orc.render(depth1, 1920, 1080, tile=tile)
        u8, f32, st, info = r.draw(desc, depth1, 1920, 1080)
        rows, rows8 = f32[0::27][:40], u8[0::27][:40]
        assert np.array_equal(rows == 0, of32 == 0), what
        check_outliers("config2_atrium_1080p_depth1_rows", rows, of32)
        assert int(np.abs(rows8.astype(int) - ou8.astype(int)).max()) <= 1
        return (u8, f32), info

    _, _, _, info = r.draw(desc, depth1, 1920, 1080)
    assert info["action"] == abi.DRAW_REBUILT and info["ms"]["build"] > 0.0
    second, info = against_the_oracle("reused")
    assert info["action"] == abi.DRAW_REUSED and info["reuses"] == 2
    assert_no_build(info, 1)
    assert_same_frame(second, fresh_frame(desc, depth1, 1920, 1080), "atrium reused")
    # a camera move: the oracle follows through a scene of its own
    place_camera(desc, 1, (0.0, 2.2, 0.3), 5.0)
    orc.close()
    orc = ol.OracleScene(desc, Config(), build=ol.BUILD_BINNED)
    _, _, _, info = r.draw(desc, depth1, 1920, 1080)
    assert info["action"] == abi.DRAW_UPDATED
    assert_no_build(info, 1)
    third, info = against_the_oracle("updated")
    assert info["action"] == abi.DRAW_REUSED and info["builds"] == 1 and info["updates"] == 1
    assert_same_frame(third, fresh_frame(desc, depth1, 1920, 1080), "atrium updated")
    assert not np.array_equal(second[1], third[1])
    orc.close()
    r.close()
