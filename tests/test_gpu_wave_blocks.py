"""k_generation as one-wave workgroups (trace_core.inc kGenBlock; select.inc grid_policy) that read their cold arguments where they
are used (kernels.hip GenArgs / GEN_COLD; trace_core.inc cold_arg): how the kernel is laid out, scheduled and fed its arguments
changes, what it computes does not.  The fused engine on the tree's library is compared with

(a) the wavefront engine of the same library, whose kernels keep their 256-thread blocks and their argument lists: RGBA8 and
    rgba32f bit for bit, and the four counters that count rays and shaded hits (boxes_tested and triangles_tested are each
    engine's own traversal: the goldens of test_gpu_node_step.py differ between the engines on every scene but the box);
(b) the variant library build() makes with -DRAYCA_GEN_WAVES_PER_BLOCK=4 -DRAYCA_COLD_ARGS=0, the kernel as it was, loaded by a
    fresh child process through RAYCA_HIP_LIB: RGBA8, rgba32f and all six counters of the counting instantiation.

The cases are wave_block_cases.CASES: 8x8, 24x16 and 67x45 frames (one tile, fewer tiles than waves, ragged right and bottom
tiles) at max_depth 1 and 3, a Flat frame, two light samples, a scene with a sphere, and the deep scene.  A second child, on the
tree's library with RAYCA_PATH_LDS_ENTRIES=4, renders the deep scene with the stack capped at four LDS entries per lane: its
camera rays store entries beyond them (test_gpu_node_step.py::test_the_deep_scene_crosses_the_spill_boundary), in the spill column
whose stride is now the grid's waves x 64.  Then three contexts in flight, each against its frame rendered alone, and a frame in
three bands against the whole."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wave_block_cases as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def child(tmp_path_factory, names=(), **env):
    out = str(tmp_path_factory.mktemp("wave_blocks") / "frames.npz")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "wave_block_cases.py"), out, *names],
                       env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out)), r.stdout


@pytest.fixture(scope="module")
def here(gpu):
    assert "RAYCA_HIP_LIB" not in os.environ and "RAYCA_PATH_LDS_ENTRIES" not in os.environ
    return W.render_cases()


@pytest.fixture(scope="module")
def wavefront(gpu):
    from rayca_amd import abi
    return W.render_cases(engine=abi.ENGINE_WAVEFRONT)


@pytest.fixture(scope="module")
def earlier(gpu, tmp_path_factory):
    import __graft_entry__ as g
    assert os.path.isfile(g.VARIANT_LIB), "build() makes the variant library"
    frames, stdout = child(tmp_path_factory, RAYCA_HIP_LIB=g.VARIANT_LIB)
    assert "library = " + os.path.realpath(g.VARIANT_LIB) in stdout, stdout
    return frames


@pytest.fixture(scope="module")
def capped(gpu, tmp_path_factory):
    frames, stdout = child(tmp_path_factory, W.DEEP, RAYCA_PATH_LDS_ENTRIES=str(W.SPILL_ENTRIES))
    assert f"RAYCA_PATH_LDS_ENTRIES = {W.SPILL_ENTRIES}" in stdout
    return frames


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same(a, b, name, counters):
    assert np.array_equal(a[name + "/u8"], b[name + "/u8"]), name
    assert same_bits(a[name + "/f32"], b[name + "/f32"]), name
    ca, cb = a[name + "/counters"], b[name + "/counters"]
    print(name, dict(zip(W.COUNTER_KEYS, ca.tolist())))
    assert np.array_equal(ca[:counters], cb[:counters]), f"{name}: {ca} vs {cb}"


@pytest.mark.parametrize("name", list(W.CASES))
def test_fused_frames_are_the_wavefront_engines(here, wavefront, name):
    assert_same(here, wavefront, name, W.RAY_COUNTERS)
    c = here[name + "/counters"]
    _, w, h, cfg = W.CASES[name]
    assert c[0] == w * h and c[3] > 0 and c[4] > c[0] and c[5] > 0   # every pixel a camera ray; something was hit and shaded
    if cfg.max_depth == 3:
        assert c[2] > 0   # bounce rays went through push_ray
    assert float(here[name + "/f32"][..., :3].max()) > 0.0


@pytest.mark.parametrize("name", list(W.CASES))
def test_fused_frames_are_those_of_the_earlier_kernel(here, earlier, name):
    assert_same(here, earlier, name, len(W.COUNTER_KEYS))


@pytest.mark.parametrize("name", W.DEEP)
def test_spill_column_with_four_lds_entries(here, earlier, capped, name):
    assert_same(capped, here, name, len(W.COUNTER_KEYS))
    assert_same(capped, earlier, name, len(W.COUNTER_KEYS))


def test_three_contexts_in_flight(here):
    import torch
    from rayca_amd import DeviceScene, abi
    import node_step_cases as N
    dev = torch.device("cuda", 0)
    names = ["cornell_67x45_d3", "cornell_67x45_d1", "cornell_flat"]
    ds = DeviceScene(N.frame_desc("cornell"), W.Config(), builder=abi.BUILDER_SAH)
    ds.finish()
    streams = [torch.cuda.Stream(dev) for _ in names]
    outs = [torch.zeros((45, 67, 4), dtype=torch.float32, device=dev) for _ in names]
    for _ in range(4):
        for i, n in enumerate(names):
            ds.render_device(W.CASES[n][3], 67, 45, 0, outs[i].data_ptr(), stream=streams[i].cuda_stream, context=i, engine=abi.ENGINE_FUSED,
                             camera_rays=abi.CAMERA_GENERATION)
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        assert same_bits(outs[i].cpu().numpy(), here[n + "/f32"]), n
    ds.close()


def test_banded_tile_against_the_whole_frame(here):
    from rayca_amd import DeviceScene, abi
    import node_step_cases as N
    name = "cornell_67x45_d3"
    _, w, h, cfg = W.CASES[name]
    ds = DeviceScene(N.frame_desc("cornell"), W.Config(), builder=abi.BUILDER_SAH)
    frame, frame8 = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.uint8)
    for part in range(3):
        u8, f32, _ = ds.render(cfg, w, h, tile=(part, 3, 8), engine=abi.ENGINE_FUSED)
        rows = [y for y in range(h) if (y // 8) % 3 == part]
        assert f32.shape[0] == len(rows)
        frame[rows], frame8[rows] = f32, u8
    ds.close()
    assert same_bits(frame, here[name + "/f32"]) and np.array_equal(frame8, here[name + "/u8"])
