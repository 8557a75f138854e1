"""The path k_generation at five waves per SIMD with the compact parked context (trace_core.inc RAYCA_MIN_WAVES,
RAYCA_CTX_COMPACT; api.inc fused_generation): 96 registers, 104 B of context per lane behind four stack rows.  What is parked and
where changes, what the kernel computes does not.  The fused engine on the tree's library is compared with

(a) the wavefront engine of the same library, whose kernels park nothing: RGBA8 and rgba32f bit for bit, and the four counters
    that count rays and shaded hits;
(b) the variant library build() makes (__graft_entry__.VARIANT_FLAGS: four waves, seven quads behind twelve rows), loaded by a
    fresh child process through RAYCA_HIP_LIB: the same frames and all six counters of the counting instantiation;
(c) on the deep scene, child processes of the tree's library with RAYCA_PATH_LDS_ENTRIES=4 and =12: the stack capped at four LDS
    entries per lane (what the five-wave instantiations get by default) and at twelve (what the kernel had, and what the counting
    and sphere instantiations, which stay at four waves, still get).  So each child differs from the default process in one of
    the two instantiations a case runs: the 12-entry child in the frames, the 4-entry child in the counters.

The cases are five_waves_cases.CASES.  That the condition a case is there for occurs is asserted on the host: from the scene
description (lights, materials, alphas), from the surface records under the frames' own camera rays (Phong walls, PBR block,
emissive panel, a sphere), from the counters (sums of four or two outcomes, a bounce generation), and for the deep frame by walking
its camera rays on the device's tree (entries beyond the fourth LDS row).  Then three contexts in flight, each against its frame
rendered alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import five_waves_cases as V
import leaf_shade_cases as L
import wave_block_cases as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
from rayca_amd.abi import MATERIAL_PBR, MATERIAL_PHONG   # noqa: E402


def child(tmp_path_factory, names=(), **env):
    out = str(tmp_path_factory.mktemp("five_waves") / "frames.npz")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "five_waves_cases.py"), out, *names],
                       env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out)), r.stdout


@pytest.fixture(scope="module")
def here(gpu):
    assert "RAYCA_HIP_LIB" not in os.environ and "RAYCA_PATH_LDS_ENTRIES" not in os.environ
    return V.render_cases()


@pytest.fixture(scope="module")
def wavefront(gpu):
    from rayca_amd import abi
    return V.render_cases(engine=abi.ENGINE_WAVEFRONT)


@pytest.fixture(scope="module")
def earlier(gpu, tmp_path_factory):
    import __graft_entry__ as g
    assert os.path.isfile(g.VARIANT_LIB), "build() makes the variant library"
    assert "-DRAYCA_MIN_WAVES=4" in g.VARIANT_FLAGS and "-DRAYCA_CTX_COMPACT=0" in g.VARIANT_FLAGS
    frames, stdout = child(tmp_path_factory, RAYCA_HIP_LIB=g.VARIANT_LIB)
    assert "library = " + os.path.realpath(g.VARIANT_LIB) in stdout, stdout
    return frames


@pytest.fixture(scope="module", params=(4, 12))
def capped(request, gpu, tmp_path_factory):
    frames, stdout = child(tmp_path_factory, V.DEEP, RAYCA_PATH_LDS_ENTRIES=str(request.param))
    assert f"RAYCA_PATH_LDS_ENTRIES = {request.param}" in stdout
    return frames


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same(a, b, name, counters):
    assert np.array_equal(a[name + "/u8"], b[name + "/u8"]), name
    assert same_bits(a[name + "/f32"], b[name + "/f32"]), name
    ca, cb = a[name + "/counters"], b[name + "/counters"]
    print(name, dict(zip(V.COUNTER_KEYS, ca.tolist())))
    assert np.array_equal(ca[:counters], cb[:counters]), f"{name}: {ca} vs {cb}"


def test_the_mixed_room_fills_every_shortened_word():
    """from the scene description: two lights, one of them a quad light; a Phong and a PBR material; a material colour and vertex
    colours whose alpha is not 1; an emissive material"""
    c = V.frame_desc("mixed_room").c
    assert sorted(L.light_kinds(V.frame_desc("mixed_room"))) == [L.LIGHT_POINT, L.LIGHT_QUAD]
    mats = [c.materials[i] for i in range(c.material_count)]
    assert {MATERIAL_PBR, MATERIAL_PHONG} <= {int(m.kind) for m in mats}
    assert any(int(m.kind) == MATERIAL_PBR and abs(m.color[3] - V.MATERIAL_ALPHA) < 1e-6 for m in mats)
    assert any(int(m.kind) == MATERIAL_PHONG and m.shininess == 8.0 for m in mats)
    quad = [c.lights[i] for i in range(c.light_count) if int(c.lights[i].kind) == L.LIGHT_QUAD][0]
    assert quad.material < c.material_count and tuple(mats[quad.material].emission)[:3] == (1.0, 1.0, 1.0)   # the emissive panel's
    alphas = np.ctypeslib.as_array(c.colors, (c.vertex_count, 4))[:, 3]
    assert np.isclose(alphas, V.VERTEX_ALPHA).any() and np.isclose(alphas, 1.0).any()


def test_camera_rays_meet_what_the_cases_are_for(gpu):
    """the surface under every pixel of the cases' frames (DeviceScene.gbuffer: camera rays -> closest hits -> surface records): at
    every size the mixed room's camera rays shade the Phong walls AND the PBR block, some of them a surface whose diffuse alpha
    is not 1; at 67 x 45 they also see the emissive panel; the sphere fixture has spheres and its camera rays hit them"""
    from rayca_amd import DeviceScene, abi
    ds = DeviceScene(V.frame_desc("mixed_room"), V.Config(), builder=abi.BUILDER_SAH)
    for w, h in V.SIZES:
        g = ds.gbuffer(V.CASES[f"mixed_{w}x{h}_d1"][3], w, h, want=("diffuse", "flags"))
        flags, alpha = g["flags"].cpu().numpy().view(np.uint32).reshape(-1), g["diffuse"].cpu().numpy().reshape(-1, 4)[:, 3]
        hit = (flags & abi.SURFACE_HIT) != 0
        lit_kind = flags[hit & ((flags & abi.SURFACE_EMISSIVE) == 0)] & abi.SURFACE_KIND_MASK
        n_phong, n_pbr, n_emissive = int((lit_kind == MATERIAL_PHONG).sum()), int((lit_kind == MATERIAL_PBR).sum()), int((hit & ((flags & abi.SURFACE_EMISSIVE) != 0)).sum())
        print(f"mixed room {w} x {h}: {n_phong} Phong, {n_pbr} PBR, {n_emissive} emissive pixels; diffuse alphas {sorted(set(np.round(alpha[hit], 4).tolist()))}")
        assert n_phong > 0 and n_pbr > 0
        assert (np.abs(alpha[hit] - 1.0) > 0.1).any()
        assert (w, h) != V.SIZES[-1] or n_emissive > 0
    ds.close()
    ds = DeviceScene(V.frame_desc("spheres"), V.Config(), builder=abi.BUILDER_SAH)
    assert ds.info()["sphere_count"] > 0   # the SPH instantiations run: view is the model-space direction
    _, w, h, cfg = V.CASES["spheres_d1"]
    flags = ds.gbuffer(cfg, w, h, want=("flags",))["flags"].cpu().numpy().view(np.uint32)
    on_sphere = int(((flags & abi.SURFACE_SPHERE) != 0).sum())
    print(f"spheres {w} x {h}: {on_sphere} pixels on a sphere")
    assert on_sphere > 0
    ds.close()


def test_the_deep_frame_crosses_four_lds_rows(gpu):
    """the 64 x 45 deep frame of the cases, as test_gpu_node_step.py shows it for its 64 x 64 one: the scene plans more stack entries
    than four rows and a register hold, and camera rays of THIS frame, walked on the device's own 48-B records by the restatement of
    the pipelined node loop (node_step_cases.ch_walk), store entries beyond LDS entry 3 -- in the spill column"""
    from rayca_amd import DeviceScene, abi
    import node_step_cases as N
    import oracle_lib as ol
    _, w, h, cfg = V.CASES["deep_d1"]
    ds = DeviceScene(V.frame_desc("deep_soup"), V.Config(), builder=abi.BUILDER_SAH)
    ds.finish()
    assert ds.info()["max_depth"] >= N.SPILL_ENTRIES + 2, ds.info()["max_depth"]
    nodes, order = ds.read_nodes(1), ds.primitive_order()
    cam = ds.camera_rays(cfg, w, h).cpu().numpy()
    ds.close()
    assert cam.shape == (w * h, 6)
    orc = ol.OracleScene(V.frame_desc("deep_soup"), V.Config())
    tri = orc.world_triangles(orc.primitive_count).reshape(-1, 3, 3)
    orc.close()
    root = (tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0))
    # (the restatement divides by the direction: not the middle row, whose rays have dy = 0.  Every seventh ray: about as many as
    # test_gpu_node_step.py walks of its 64 x 64 frame, for the same bar of eight)
    rays = cam[(cam[:, 3:] != 0).all(1)][5::7]
    assert rays.shape[0] >= 372
    for slack_form in (False, True):   # generation 0 of a path frame takes either form, wave by wave
        walks = [N.ch_walk(nodes, root, tri[order], r, slack_form=slack_form) for r in rays]
        crossing = sum(x["spilled"] > 0 for x in walks)
        print(f"slack form {slack_form}: deepest stack {max(x['max_stack'] for x in walks)}, {crossing} of {len(walks)} camera rays store entries beyond LDS entry 3")
        assert crossing >= 8


@pytest.mark.parametrize("name", list(V.CASES))
def test_fused_frames_are_the_wavefront_engines(here, wavefront, name):
    assert_same(here, wavefront, name, V.RAY_COUNTERS)
    c = here[name + "/counters"].astype(np.int64)
    scene, w, h, cfg = V.CASES[name]
    assert c[0] == w * h and c[3] > 0 and c[4] > c[0] and c[5] > 0   # every pixel a camera ray; something was hit and shaded
    rgb = here[name + "/f32"][..., :3]
    assert float(rgb.max()) > 0.0
    if cfg.max_depth == 3:
        assert c[2] > 0   # a bounce generation ran on the fused engine (push_ray)
    if scene == "mixed_room" and cfg.max_depth == 1:
        # every shaded hit that is not emissive traces lights x light_samples shadow rays, so its sum takes four or two outcomes;
        # and at 67 x 45 (the panel is two rows high there) the camera saw the emissive panel
        per_vertex = 2 * cfg.light_samples
        assert c[1] % per_vertex == 0 and 0 < c[1] // per_vertex <= c[3]
        assert w < 67 or c[1] // per_vertex < c[3]
        # lit and not lit: some shaded pixels stay black (the block's shadow, faces turned away), most do not
        assert (rgb.max(-1) == 0.0).any() and (rgb.max(-1) > 0.0).sum() > w * h // 4


@pytest.mark.parametrize("name", list(V.CASES))
def test_fused_frames_are_those_of_the_earlier_kernel(here, earlier, name):
    assert_same(here, earlier, name, len(V.COUNTER_KEYS))


@pytest.mark.parametrize("name", V.DEEP)
def test_deep_scene_with_four_and_twelve_lds_entries(here, earlier, capped, name):
    assert_same(capped, here, name, len(V.COUNTER_KEYS))
    assert_same(capped, earlier, name, len(V.COUNTER_KEYS))


def test_three_contexts_in_flight(here):
    import torch
    from rayca_amd import DeviceScene, abi
    dev = torch.device("cuda", 0)
    names = list(V.IN_FLIGHT)
    ds = DeviceScene(V.frame_desc("mixed_room"), V.Config(), builder=abi.BUILDER_SAH)
    ds.finish()
    streams = [torch.cuda.Stream(dev) for _ in names]
    outs = [torch.zeros((V.CASES[n][2], V.CASES[n][1], 4), dtype=torch.float32, device=dev) for n in names]
    for _ in range(4):
        for i, n in enumerate(names):
            _, w, h, cfg = V.CASES[n]
            ds.render_device(cfg, w, h, 0, outs[i].data_ptr(), stream=streams[i].cuda_stream, context=i, engine=abi.ENGINE_FUSED,
                             camera_rays=abi.CAMERA_GENERATION)
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        assert same_bits(outs[i].cpu().numpy(), here[n + "/f32"]), n
    ds.close()
