"""k_generation's last-vertex form (kernels.hip LAST; select.inc last_form, pick_kernel; api.inc fused_generation): the generation
behind which no vertex of a path samples a bounce runs a kernel whose tail takes the direct sum back and writes the vertex's
record -- no bounce sampler, no surf_brdf, no factor record, no push_ray, no bounce counter, no fetch of the parked context.  What
a frame computes does not change.  The fused engine's frames of last_vertex_cases.CASES (61 x 35, both builders) are compared with

(a) a fresh child process with RAYCA_LAST_FORM=0, where the host picks the general form everywhere: RGBA8 and rgba32f bit for bit
    and all six counters of the counting instantiation;
(b) the wavefront engine of this process: RGBA8, rgba32f and the four counters that count rays and shaded hits (boxes_tested and
    triangles_tested are each engine's own traversal).

Which generations ran the form is read from RaycaStats.node_format (bit 16 + g), for the production and the counting frame:
generation 0 at max_depth 1 under NEE, the last generation alone at max_depth 2 and 3, none without a direct sampler, none in the
child.  rayca_hip_selftest holds the same rule and the picker's table (select.inc selftest_kernel_selection) without a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import last_vertex_cases as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def here(gpu):
    assert "RAYCA_LAST_FORM" not in os.environ and "RAYCA_HIP_LIB" not in os.environ
    return V.render_cases()


@pytest.fixture(scope="module")
def wavefront(gpu):
    from rayca_amd import abi
    return V.render_cases(engine=abi.ENGINE_WAVEFRONT)


@pytest.fixture(scope="module")
def general_form(gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("last_vertex") / "frames.npz")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "last_vertex_cases.py"), out],
                       env=dict(os.environ, RAYCA_LAST_FORM="0"), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAYCA_LAST_FORM = 0" in r.stdout, r.stdout
    return dict(np.load(out))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same(a, b, key, counters):
    assert np.array_equal(a[key + "/u8"], b[key + "/u8"]), key
    assert same_bits(a[key + "/f32"], b[key + "/f32"]), key
    ca, cb = a[key + "/counters"], b[key + "/counters"]
    print(key, dict(zip(V.COUNTER_KEYS, ca.tolist())))
    assert np.array_equal(ca[:counters], cb[:counters]), f"{key}: {ca} vs {cb}"


@pytest.mark.parametrize("key", V.keys())
def test_frames_are_those_of_the_general_form(here, general_form, key):
    assert_same(here, general_form, key, len(V.COUNTER_KEYS))
    cfg = V.CASES[key.split("/")[0]][1]
    c = here[key + "/counters"]
    assert c[0] == V.W * V.H * cfg.samples_per_pixel and c[3] > 0 and c[4] > c[0] and c[5] > 0   # every pixel a camera ray; something was hit and shaded
    assert (c[1] > 0) == (V.last_generations(cfg) != 0)   # shadow rays exactly under NEE: the form's own counter
    if cfg.max_depth == 3:
        assert c[2] > 0   # bounce rays went through the general form's push_ray
    assert float(here[key + "/f32"][..., :3].max()) > 0.0


@pytest.mark.parametrize("key", V.keys())
def test_frames_are_the_wavefront_engines(here, wavefront, key):
    assert_same(here, wavefront, key, V.RAY_COUNTERS)


@pytest.mark.parametrize("key", V.keys())
def test_the_host_picks_the_form_for_the_last_generation_only(here, general_form, wavefront, key):
    want = V.last_generations(V.CASES[key.split("/")[0]][1])
    assert here[key + "/forms"].tolist() == [want, want], "the production and the counting frame run the same form"
    assert general_form[key + "/forms"].tolist() == [0, 0], "RAYCA_LAST_FORM=0: the general form everywhere"
    assert wavefront[key + "/forms"].tolist() == [0, 0], "the wavefront engine has no such form"
