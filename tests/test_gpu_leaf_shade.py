"""The traversal, leaf, shading and BRDF code of every kernel is compiled without packed f32 arithmetic (kernels.hip
RAYCA_NO_PK_F32): only the instructions that carry the operations change, never an operand or an order, so every frame and
every hit record keeps its bits and the traversal performs the same tests.

Frames (64x64; box.gltf, the Cornell room, spheres.sdtf, a room under a quad light; max_depth 1-3 -- depth 2 and 3 run a
generation that queues rays and the last one in one frame -- x samples_per_pixel 1-2 x light_samples 1-2): the fused engine's
frame equals the wavefront engine's, the RAYCA_BUILDER_REFERENCE scene's and its own counting instantiation's bit for bit,
and the counters equal those recorded before the change (tests/golden/leaf_shade_counters.json, written by
tests/make_leaf_shade_golden.py).

Hit records (t, prim, u, v) through DeviceScene.query and trace_rays against the oracle, bit for bit, on rays aimed at chosen
primitive slots of the 48-B record array, a 64-primitive leaf, a root that is a leaf, exact depth ties, sphere slots, rays
through triangle corners and far rays whose nearer triangle the reference-leaf filter refuses; see leaf_shade_cases.py."""
import json
import os

import numpy as np
import pytest

import leaf_shade_cases as L
import oracle_lib as ol
import test_gpu_query as Q
from rayca_amd import Config, DeviceScene, abi, flatten

pytestmark = pytest.mark.gpu
NONE = L.NONE
HOW = ["reference", "sah", "sah_unfinished"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame_counters(name, make_scene=DeviceScene):
    """{builder: {config: counters}} of the fused engine's counting instantiation, and the frames it rendered"""
    desc = L.frame_desc(name)
    out, frames = {}, {}
    for bname, builder in (("sah", abi.BUILDER_SAH), ("reference", abi.BUILDER_REFERENCE)):
        ds = make_scene(desc, Config(), builder=builder)
        ds.finish()
        out[bname] = {}
        for cname, cfg in L.CONFIGS:
            u8, f32, st = ds.render(cfg, *L.FRAME, engine=abi.ENGINE_FUSED, collect_stats=True)
            out[bname][cname] = {k: int(st[k]) for k in L.COUNTER_KEYS}
            frames[bname, cname] = (u8, f32)
        ds.close()
    return out, frames


def test_the_scenes_have_a_point_light_and_a_quad_light():
    kinds = {name: L.light_kinds(L.frame_desc(name)) for name in L.FRAME_SCENES}
    assert L.LIGHT_POINT in kinds["cornell"] and L.LIGHT_QUAD in kinds["quad_room"] and len(kinds["spheres"]) == 2, kinds


@pytest.mark.parametrize("name", list(L.FRAME_SCENES))
def test_frames_and_counters(gpu, name):
    golden = json.load(open(os.path.join(L.G, "leaf_shade_counters.json")))[name]
    counters, counted = frame_counters(name)
    desc = L.frame_desc(name)
    sah = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    sah.finish()
    ref = DeviceScene(desc, Config(), builder=abi.BUILDER_REFERENCE)
    lit = 0.0
    for cname, cfg in L.CONFIGS:
        u8, f32, _ = sah.render(cfg, *L.FRAME, engine=abi.ENGINE_FUSED)          # (no counters: the production instantiations)
        for what, (ou8, of32) in (("wavefront", sah.render(cfg, *L.FRAME, engine=abi.ENGINE_WAVEFRONT)[:2]),
                                  ("reference builder", ref.render(cfg, *L.FRAME, engine=abi.ENGINE_FUSED)[:2]),
                                  ("counting instantiation", counted["sah", cname]),
                                  ("counting instantiation, reference builder", counted["reference", cname])):
            assert np.array_equal(bits(f32), bits(of32)), f"{name} {cname} vs {what}: max abs diff {np.nanmax(np.abs(f32 - of32)):.3e}"
            assert np.array_equal(u8, ou8), f"{name} {cname} vs {what}"
        lit = max(lit, float(f32[..., :3].max()))
        for b in ("sah", "reference"):
            assert counters[b][cname] == golden[b][cname], f"{name} {b} {cname}"
    assert lit > 0.0
    sah.close()
    ref.close()


# ---- hit records -------------------------------------------------------------------------------------------------------
def device_records(ds, rays):
    """the records of both ray-query entry points (asserted equal)"""
    got = Q.run_closest(ds, Q.dev(rays), None)
    t, prim, uv, _ = ds.trace_rays(rays)
    Q.assert_records(got, (t, prim, uv), "query vs trace_rays")
    return got


def slots_of_leaves(ds):
    """(first slot, count) of every leaf the 64-B binary nodes refer to"""
    refs = ds.read_nodes(0)[:, 12:14].reshape(-1)
    leaves = refs[(refs & np.uint32(0x80000000)) != 0]
    return leaves & np.uint32(0x01FFFFFF), ((leaves >> np.uint32(25)) & np.uint32(63)) + np.uint32(1)


@pytest.mark.parametrize("how", HOW)
def test_rays_aimed_at_slots(gpu, how):
    """soup1k: every slot is aimed at; slots 0, 1, 2, the last one and one with index = 2 mod 8 (its 48-B record starts at byte 96
    of a 128-B line and ends in the next) must be among the recorded hits."""
    desc, orc, tri = L.hit_desc("soup1k"), L.oracle("soup1k"), L.triangles("soup1k")
    ds = Q.make_scene(desc, how)
    order = ds.primitive_order()
    n = order.size
    slots = np.array(sorted({0, 1, 2, 10, 98, n - 1} | set(range(2, n, 8))), np.int64)
    rays = L.aimed_rays(tri[order[slots]]).reshape(-1, 6)
    ot, oprim, ouv, _ = orc.trace_rays(rays)
    want = (ot, Q.in_slots(ds, desc, oprim, "leaf_shade_soup1k"), ouv)
    Q.assert_records(device_records(ds, rays), want, f"soup1k {how}")
    landed = set(want[1][want[1] == np.repeat(slots, 4).astype(np.uint32)].tolist())
    assert {0, 1, 2, n - 1} <= landed and any(s % 8 == 2 and s > 2 for s in landed), sorted(landed)[:12]
    ds.close()


@pytest.mark.parametrize("how", HOW)
def test_a_64_primitive_leaf_and_exact_depth_ties(gpu, how):
    desc, orc, tri = L.hit_desc("coincident"), L.oracle("coincident"), L.triangles("coincident")
    ds = Q.make_scene(desc, how)
    if how != "reference":
        _, count = slots_of_leaves(ds)
        assert count.max() == 64, count.max()
    rays = L.aimed_rays(tri).reshape(-1, 6)
    ot, oprim, ouv, _ = orc.trace_rays(rays)
    flat = orc.primitive_order()[oprim[oprim != NONE]]
    assert (flat < 70).sum() >= 4 * 70 and (flat >= 70).sum() >= 40      # the copies all resolve to one of them; the others are hit too
    assert np.unique(flat[flat < 70]).size == 1
    Q.assert_records(device_records(ds, rays), (ot, Q.in_slots(ds, desc, oprim, "leaf_shade_coincident"), ouv), f"coincident {how}")
    ds.close()


@pytest.mark.parametrize("how", HOW)
def test_a_root_that_is_a_leaf(gpu, how):
    desc, orc, tri = L.hit_desc("one_triangle"), L.oracle("one_triangle"), L.triangles("one_triangle")
    assert tri.shape[0] == 1
    ds = Q.make_scene(desc, how)
    rays = np.concatenate([L.aimed_rays(tri).reshape(-1, 6), L.grazing_rays("one_triangle", 16)])
    ot, oprim, ouv, _ = orc.trace_rays(rays)
    assert (oprim != NONE).sum() >= 4 and (oprim == NONE).sum() >= 4
    Q.assert_records(device_records(ds, rays), (ot, Q.in_slots(ds, desc, oprim, "leaf_shade_one_triangle"), ouv), f"one triangle {how}")
    ds.close()


@pytest.mark.parametrize("how", HOW)
def test_sphere_slots(gpu, how):
    desc = flatten(L.spheres_scene())
    orc = ol.OracleScene(desc, Config())
    i = np.arange(512)
    from rayca_amd import scenes
    o = np.stack([(scenes.hash_unit(31 + a, i) * 2 - 1) * np.float32(3.0) for a in range(3)], 1).astype(np.float32)
    d = np.stack([scenes.hash_unit(41 + a, i) * 2 - 1 for a in range(3)], 1).astype(np.float32) * np.float32(0.5) - o
    rays = np.concatenate([o, d], 1).astype(np.float32)
    ot, oprim, ouv, _ = orc.trace_rays(rays)
    hit = oprim != NONE
    assert hit.sum() >= 64 and (ouv[hit] == 0).all(axis=1).sum() >= 16     # spheres report u = v = 0
    ds = Q.make_scene(desc, how)
    Q.assert_records(device_records(ds, rays), (ot, Q.in_slots(ds, desc, oprim, "leaf_shade_spheres"), ouv), f"spheres {how}")
    ds.close()
    orc.close()


@pytest.mark.parametrize("how", HOW)
def test_soup_fixture_and_grazing_rays(gpu, how):
    """The soup fixture's rays, 18 000 rays through triangle corners and the far rays, among them 65 that pass the triangle test
    on a nearer triangle whose reference leaf refuses it (picked on the CPU: leaf_shade_cases.nearer_passes;
    test_leaf_shade_cpu.py asserts that they are there).  The RAYCA_BUILDER_REFERENCE scene takes all 12 000 far rays.  The
    RAYCA_BUILDER_SAH scenes, where the refusal is the work of reference_candidate inside test_leaf, take the refused ones:
    of the other far rays the conservative steering tests lose about forty hits at this distance (10^6 units, directions not
    normalised) -- before this change exactly as after it, see DESIGN section 7 -- and steering is not what this file is about."""
    desc, orc = L.hit_desc("soup1k"), L.oracle("soup1k")
    rays, n_near, refused = L.soup_set()[:3]
    assert refused.size >= 2 and (refused >= n_near).all()
    if how != "reference":
        rays = rays[np.concatenate([np.arange(n_near), refused])]
    ot, oprim, ouv, _ = orc.trace_rays(rays)
    ds = Q.make_scene(desc, how)
    Q.assert_records(device_records(ds, rays), (ot, Q.in_slots(ds, desc, oprim, "leaf_shade_soup1k"), ouv), f"soup rays {how}")
    ds.close()
