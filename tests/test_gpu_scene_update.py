"""rayca_hip_scene_update on the MI355X: after an edit of the camera, the lights or the materials, every frame of the updated
handle is bit-identical (RGBA8 and RGBA32F, error codes too) to the frame of a scene created from the edited descriptor;
edits that would move geometry are refused and change nothing; frames in flight render the state they were issued under."""
import math
import os
import statistics
import time

import numpy as np
import pytest

from rayca_amd import (Config, DeviceScene, Image, IntegratorStrategy, Mesh, Model, Node, PbrMaterial, Primitive,
                       SamplerStrategy, Scene, SoftRenderer, Texture, TriangleMesh, Trs, abi, flatten, scenes, sdtf)
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 96, 64
I, S = IntegratorStrategy, SamplerStrategy
FLAT = Config(integrator=I.Flat)
# Flat (fused camera rays / resolve), the generation kernels (depth 2 + NEE), the wavefront engine (depth 3, its default
# from three generations) and the stack machine (MIS is only offered there)
ORBIT_CONFIGS = [(FLAT, abi.ENGINE_AUTO), (Config(integrator=I.Flat, samples_per_pixel=4), abi.ENGINE_AUTO),
                 (Config(max_depth=2, seed=3), abi.ENGINE_AUTO), (Config(max_depth=3, seed=4), abi.ENGINE_AUTO),
                 (Config(direct_sampler=S.Mis, indirect_sampler=S.Brdf, max_depth=2, seed=5), abi.ENGINE_AUTO)]


def frame(ds, cfg, engine=abi.ENGINE_AUTO, w=W, h=H):
    """('ok', rgba8, rgba32f bits) or ('err', code)"""
    try:
        u8, f32, _ = ds.render(cfg, w, h, engine=engine)
    except RaycaError as e:
        return ("err", e.code)
    return ("ok", u8, np.ascontiguousarray(f32).view(np.uint32))


def assert_same(a, b, what=""):
    assert a[0] == b[0], f"{what}: {a[0]} vs {b[0]} ({a[1] if a[0] == 'err' else b[1]})"
    if a[0] == "err":
        assert a[1] == b[1], what
    else:
        assert np.array_equal(a[1], b[1]), f"{what}: RGBA8 differs"
        assert np.array_equal(a[2], b[2]), f"{what}: RGBA32F differs"


def assert_matches_fresh(ds, desc, configs, builder, bvh=True, what=""):
    """every config: the updated handle == a scene created from `desc` now"""
    fresh = DeviceScene(desc, Config(bvh=bvh), builder=builder)
    try:
        out = []
        for cfg, engine in configs:
            a, b = frame(ds, cfg, engine), frame(fresh, cfg, engine)
            assert_same(a, b, f"{what} {cfg} engine {engine}")
            out.append(a)
        return out
    finally:
        fresh.close()


def nodes(desc):
    return desc._nodes[:desc.c.node_count]


def node_with(desc, field):
    return next(i for i, n in enumerate(nodes(desc)) if getattr(n, field) != abi.NONE)


def yaw(theta):
    return (0.0, math.sin(theta / 2), 0.0, math.cos(theta / 2))


def set_trs(node, translation=None, rotation=None, scale=None):
    if translation is not None:
        node.trs.translation[:] = translation
    if rotation is not None:
        node.trs.rotation[:] = rotation
    if scale is not None:
        node.trs.scale[:] = scale


def place_camera(desc, k, centre, radius):
    """pose k of eight: yaw 45 deg * k on a circle round `centre`, looking at it; yfov pi/4 and pi/3 in turn"""
    cam = nodes(desc)[node_with(desc, "camera")]
    th = math.radians(45.0 * k)
    set_trs(cam, (centre[0] + radius * math.sin(th), centre[1], centre[2] + radius * math.cos(th)), yaw(th))
    desc._cameras[cam.camera].yfov_radians = math.pi / 4 if k % 2 == 0 else math.pi / 3


ORBITS = [("cornell", scenes.cornell_scene, abi.BUILDER_SAH, (0.0, 1.0, 0.0), 0.8),
          ("cornell", scenes.cornell_scene, abi.BUILDER_REFERENCE, (0.0, 1.0, 0.0), 0.8),
          ("atrium6", lambda: scenes.atrium_scene(detail=6), abi.BUILDER_SAH, (0.0, 2.2, 0.3), 5.0)]


@pytest.mark.parametrize("case", range(len(ORBITS)), ids=[f"{o[0]}-{'sah' if o[2] else 'ref'}" for o in ORBITS])
def test_camera_orbit_equals_fresh_scenes(gpu, case):
    name, make, builder, centre, radius = ORBITS[case]
    desc = flatten(make())
    ds = DeviceScene(desc, Config(), builder=builder)
    rendered = 0
    for k in range(8):
        place_camera(desc, k, centre, radius)
        ds.update(desc)
        got = assert_matches_fresh(ds, desc, ORBIT_CONFIGS, builder, what=f"{name} pose {k}")
        rendered += sum(g[0] == "ok" for g in got)
        assert got[0][0] == "ok" and got[0][1][..., :3].max() > 0, "the Flat frame shows the scene"
    assert rendered >= 4 * 8
    ds.close()
    # one pose with Config(bvh=False): one leaf per model
    flat_desc = flatten(make())
    nb = DeviceScene(flat_desc, Config(bvh=False), builder=builder)
    place_camera(flat_desc, 3, centre, radius)
    nb.update(flat_desc)
    assert_matches_fresh(nb, flat_desc, ORBIT_CONFIGS[:3], builder, bvh=False, what=f"{name} bvh=False")
    nb.close()


NEE_PATH = [(FLAT, abi.ENGINE_AUTO), (Config(max_depth=2, seed=7), abi.ENGINE_AUTO), (Config(max_depth=3, seed=8), abi.ENGINE_AUTO),
            (Config(max_depth=2, seed=9), abi.ENGINE_GENERAL)]


def test_point_light_edits(gpu):
    desc = flatten(scenes.cornell_scene())
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    ln = nodes(desc)[node_with(desc, "light")]
    light = desc._lights[ln.light]
    assert light.kind == abi.LIGHT_POINT
    before = assert_matches_fresh(ds, desc, NEE_PATH, abi.BUILDER_SAH, what="unchanged")
    set_trs(ln, (0.3, 1.7, -0.2))
    light.intensity, light.color[:], light.attenuation[:] = 7.5, (1.0, 0.8, 0.6, 1.0), (0.5, 0.25, 1.0)
    ds.update(desc)
    moved = assert_matches_fresh(ds, desc, NEE_PATH, abi.BUILDER_SAH, what="point light edited")
    assert not np.array_equal(before[1][2], moved[1][2]), "the edit shows in the NEE frame"
    # point -> directional: the NEE path configs fail as the reference's todo!() does (nee.rs:178), Flat still renders
    light.kind = abi.LIGHT_DIRECTIONAL
    set_trs(ln, rotation=yaw(0.6))
    ds.update(desc)
    got = assert_matches_fresh(ds, desc, NEE_PATH, abi.BUILDER_SAH, what="directional")
    assert got[0][0] == "ok" and got[1] == ("err", abi.ERR_UNSUPPORTED)
    light.kind = abi.LIGHT_POINT
    ds.update(desc)
    back = assert_matches_fresh(ds, desc, NEE_PATH, abi.BUILDER_SAH, what="back to point")
    assert back[1][0] == "ok"
    ds.close()


def test_quad_light_edits_and_refusals(gpu):
    scene = Scene()
    _, scfg = sdtf.push_sdtf_from_path(scene, os.path.join(G, "cornell_quad.sdtf"))
    desc = flatten(scene)
    cfg = sdtf.apply(Config(seed=11), scfg)
    configs = [(FLAT, abi.ENGINE_AUTO), (cfg, abi.ENGINE_AUTO), (Config(max_depth=2, seed=12), abi.ENGINE_AUTO)]
    qi = next(i for i in range(desc.c.light_count) if desc._lights[i].kind == abi.LIGHT_QUAD)
    qn = nodes(desc)[next(i for i, n in enumerate(nodes(desc)) if n.light == qi)]
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    desc._lights[qi].intensity *= 0.5
    desc._lights[qi].color[:] = (0.9, 0.7, 0.4, 1.0)
    ds.update(desc)
    kept = assert_matches_fresh(ds, desc, configs, abi.BUILDER_SAH, what="quad light dimmed")
    assert kept[1][0] == "ok"
    old_t, old_ab = tuple(qn.trs.translation), tuple(desc._lights[qi].ab)
    qn.trs.translation[1] -= 0.1
    with pytest.raises(RaycaError) as e:
        ds.update(desc)
    assert e.value.code == abi.ERR_UNSUPPORTED and "light" in str(e.value)
    qn.trs.translation[:] = old_t
    desc._lights[qi].ab[:] = (old_ab[0] + 0.25, old_ab[1] * 1.5, old_ab[2] * 1.5)
    with pytest.raises(RaycaError) as e:
        ds.update(desc)
    assert e.value.code == abi.ERR_UNSUPPORTED
    desc._lights[qi].ab[:] = old_ab
    for (c, eng), k in zip(configs, kept):   # the refused edits changed nothing
        assert_same(frame(ds, c, eng), k, "after the refusals")
    ds.close()


def test_material_edits(gpu):
    desc = flatten(scenes.cornell_scene())
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    configs = NEE_PATH + [(Config(direct_sampler=S.Mis, indirect_sampler=S.Brdf, max_depth=2, seed=13), abi.ENGINE_AUTO)]
    m = desc._materials
    assert all(m[i].kind == abi.MATERIAL_PBR for i in range(desc.c.material_count))
    m[1].color[:] = (0.2, 0.3, 0.9, 1.0)
    m[3].roughness_factor, m[3].metallic_factor = 0.3, 0.8
    ds.update(desc)
    assert_matches_fresh(ds, desc, configs, abi.BUILDER_SAH, what="pbr factors")
    # PBR -> Phong with an emission: the emissive flag is recomputed
    m[0].kind = abi.MATERIAL_PHONG
    m[0].diffuse[:], m[0].specular[:], m[0].shininess = (0.6, 0.6, 0.6, 1.0), (0.1, 0.1, 0.1, 1.0), 16.0
    m[0].emission[:] = (0.3, 0.25, 0.2, 1.0)
    ds.update(desc)
    assert_matches_fresh(ds, desc, configs, abi.BUILDER_SAH, what="phong emissive")
    # PBR -> GGX on the stack machine
    m[2].kind = abi.MATERIAL_GGX
    m[2].diffuse[:], m[2].specular[:], m[2].roughness_factor = (0.1, 0.5, 0.1, 1.0), (0.3, 0.3, 0.3, 1.0), 0.4
    ds.update(desc)
    assert_matches_fresh(ds, desc, [(Config(max_depth=2, seed=14), abi.ENGINE_GENERAL), (FLAT, abi.ENGINE_AUTO)], abi.BUILDER_SAH, what="ggx")
    # a texture index out of range is refused
    m[1].albedo_texture = 0
    with pytest.raises(RaycaError) as e:
        ds.update(desc)
    assert e.value.code == abi.ERR_BAD_ARG
    m[1].albedo_texture = abi.NONE
    ds.close()


def textured_quad_scene():
    model = Model()
    tex = np.random.RandomState(5).randint(0, 256, (8, 8, 4)).astype(np.uint8)
    tex[..., 3] = 255
    t = model.textures.push(Texture(image=model.images.push(Image(8, 8, abi.COLOR_RGBA8, tex))))
    mat = model.materials.push(PbrMaterial(color=(0.9, 0.8, 0.7, 1.0), albedo=t, roughness_factor=0.8))
    g = model.geometries.push(TriangleMesh.quad(uv_scale=(3.0, 2.0)))
    p = model.primitives.push(Primitive(geometry=g, material=mat))
    model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=[p])), trs=Trs(scale=(3.0, 3.0, 1.0)))))
    scene = Scene()
    scene.push_model(model)
    scene.push_model(SoftRenderer.create_default_model())
    return scene


def test_albedo_texture_off_and_on(gpu):
    desc = flatten(textured_quad_scene())
    ds = DeviceScene(desc, Config())
    configs = [(FLAT, abi.ENGINE_AUTO), (Config(max_depth=1, seed=15), abi.ENGINE_AUTO)]
    mi = next(i for i in range(desc.c.material_count) if desc._materials[i].albedo_texture != abi.NONE)
    with_tex = assert_matches_fresh(ds, desc, configs, abi.BUILDER_REFERENCE, what="textured")
    saved = desc._materials[mi].albedo_texture
    desc._materials[mi].albedo_texture = abi.NONE
    ds.update(desc)
    without = assert_matches_fresh(ds, desc, configs, abi.BUILDER_REFERENCE, what="texture off")
    assert not np.array_equal(with_tex[0][2], without[0][2])
    desc._materials[mi].albedo_texture = saved
    ds.update(desc)
    again = assert_matches_fresh(ds, desc, configs, abi.BUILDER_REFERENCE, what="texture on again")
    assert_same(again[0], with_tex[0], "texture back")
    ds.close()


def test_refused_edits_change_nothing(gpu):
    desc = flatten(scenes.cornell_scene())
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    configs = [(FLAT, abi.ENGINE_AUTO), (Config(max_depth=2, seed=16), abi.ENGINE_AUTO)]
    before = [frame(ds, c, e) for c, e in configs]
    ns = nodes(desc)
    mesh_node = node_with(desc, "mesh")
    model_root = ns[mesh_node].parent
    assert model_root >= 0 and ns[model_root].mesh == abi.NONE

    def attempt(edit, undo, code, who=None):
        edit()
        try:
            with pytest.raises(RaycaError) as e:
                ds.update(desc)
            assert e.value.code == code, str(e.value)
            if who is not None:
                assert who in str(e.value), str(e.value)
        finally:
            undo()
        for (c, eng), b in zip(configs, before):
            assert_same(frame(ds, c, eng), b, "after a refused edit")

    t0 = tuple(ns[mesh_node].trs.translation)
    attempt(lambda: set_trs(ns[mesh_node], (t0[0] + 0.25, t0[1], t0[2])), lambda: set_trs(ns[mesh_node], t0), abi.ERR_UNSUPPORTED,
            f"node {mesh_node} ")
    r0 = tuple(ns[model_root].trs.translation)
    attempt(lambda: set_trs(ns[model_root], (r0[0], r0[1] + 1.0, r0[2])), lambda: set_trs(ns[model_root], r0), abi.ERR_UNSUPPORTED)
    p0 = ns[mesh_node].parent

    def reparent(v):
        ns[mesh_node].parent = v
    attempt(lambda: reparent(0), lambda: reparent(p0), abi.ERR_BAD_ARG)
    m0 = ns[mesh_node].mesh

    def remesh(v):
        ns[mesh_node].mesh = v
    attempt(lambda: remesh((m0 + 1) % desc.c.mesh_count), lambda: remesh(m0), abi.ERR_BAD_ARG)
    lc = desc.c.light_count

    def light_count(v):
        desc.c.light_count = v
    attempt(lambda: light_count(lc - 1), lambda: light_count(lc), abi.ERR_BAD_ARG)
    # a camera move together with a refused mesh move: the camera does not move either
    cam = ns[node_with(desc, "camera")]
    c0 = tuple(cam.trs.translation)
    attempt(lambda: (set_trs(cam, (0.2, 1.1, 3.0)), set_trs(ns[mesh_node], (t0[0], t0[1] + 0.5, t0[2]))),
            lambda: (set_trs(cam, c0), set_trs(ns[mesh_node], t0)), abi.ERR_UNSUPPORTED)
    ds.close()


def test_frames_in_flight_render_the_state_they_were_issued_under(gpu):
    import torch
    desc = flatten(scenes.cornell_scene())
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    w, h = 256, 192
    cfg = Config(max_depth=3, samples_per_pixel=4, seed=17)
    bufs = [(torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"))
            for _ in range(8)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def issue(first):
        for k in range(4):
            u8, f32 = bufs[first + k]
            ds.render_device(cfg, w, h, u8.data_ptr(), f32.data_ptr(), stream=stream.cuda_stream, context=k)

    def fresh_frame(d):
        fresh = DeviceScene(d, Config(), builder=abi.BUILDER_SAH)
        u8, f32, _ = fresh.render(cfg, w, h)
        fresh.close()
        return u8, f32.view(np.uint32)

    issue(0)                                   # pose A
    place_camera(desc, 2, (0.0, 1.0, 0.0), 0.8)
    desc._materials[1].color[:] = (0.1, 0.2, 0.8, 1.0)
    ds.update(desc)
    issue(4)                                   # pose B
    stream.synchronize()
    got = [(u8.cpu().numpy(), f32.cpu().numpy().view(np.uint32)) for u8, f32 in bufs]
    want_a, want_b = fresh_frame(flatten(scenes.cornell_scene())), fresh_frame(desc)
    assert not np.array_equal(want_a[1], want_b[1])
    for i, (u8, f32) in enumerate(got):
        want = want_a if i < 4 else want_b
        assert np.array_equal(u8, want[0]) and np.array_equal(f32, want[1]), f"frame {i} (context {i % 4})"
    ds.close()


def test_host_cost_of_updates(gpu):
    desc = flatten(scenes.atrium_scene())
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    ds.finish()
    build_ms = ds.info()["build_ms"]
    ds.render(FLAT, W, H)
    cam = nodes(desc)[node_with(desc, "camera")]
    t0 = tuple(cam.trs.translation)
    cam_ms = []
    for k in range(50):
        set_trs(cam, (t0[0] + 0.01 * (k + 1), t0[1], t0[2]))
        a = time.perf_counter()
        ds.update(desc)
        cam_ms.append((time.perf_counter() - a) * 1e3)
    light = desc._lights[nodes(desc)[node_with(desc, "light")].light]
    table_ms = []
    for k in range(20):
        light.intensity *= 1.01
        desc._materials[k % desc.c.material_count].roughness_factor = 0.3 + 0.01 * k
        a = time.perf_counter()
        ds.update(desc)
        table_ms.append((time.perf_counter() - a) * 1e3)
    cam_med, table_med = statistics.median(cam_ms), statistics.median(table_ms)
    print(f"\nscene_update host cost on the atrium: camera-only median {cam_med:.4f} ms, lights + materials median "
          f"{table_med:.4f} ms, build_ms {build_ms:.2f}")
    assert cam_med < 1.0
    assert table_med < 5.0
    assert cam_med < build_ms / 10 and table_med < build_ms / 4
    # and the frames after all those edits are a fresh scene's
    assert_matches_fresh(ds, desc, [(FLAT, abi.ENGINE_AUTO), (Config(max_depth=2, seed=18), abi.ENGINE_AUTO)], abi.BUILDER_SAH,
                         what="atrium after 70 edits")
    ds.close()
