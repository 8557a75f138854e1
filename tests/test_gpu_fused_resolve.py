"""The depth-1 path frame in one launch (kernels.hip k_generation FUSED with GEN0 && LAST; select.inc fuse_resolve, pick_kernel;
api.inc frame_begin, fused_generation): the last vertex writes the pixel, there is no record and no k_resolve, and the launch zeroes
the work-counter set it does not draw from, so that neither this frame nor a fused Flat frame needs a fill launch in front of it.
What a frame computes does not change.

Frames (fused_resolve_cases.CASES, 61 x 35, both builders): RGBA8 and rgba32f bit for bit against

(a) a fresh child process with RAYCA_FUSE_RESOLVE=0, where every path frame is generation + k_resolve -- and the ray and
    shaded-hit counters of the production frames against the child's;
(b) this process's counting frame (collect_stats: still two launches);
(c) the wavefront engine of this process.

Between them the cases have lanes of all four kinds -- a miss, an emissive first hit, a lit vertex whose light is visible and one in
shadow (established with the CPU oracle: fused_resolve_cases.py) -- of which the tests assert the cheap proxies: pixels of +0.0 and
pixels above it, and the emission colour in the quad-light room.

Where the form is picked is read from RaycaStats: node_format bit 13 and kernel_launches == 1 for the cases; neither the bit nor
a changed launch count for four samples, deeper paths, no direct sampler, counting frames, the wavefront engine, a radiance query,
and anything in the child.

Counter bookkeeping: one scene and one context run fused path frames of two sizes, a fused Flat frame, a depth-3 frame, a wavefront
frame, a four-sample frame, a counting frame and a ray query in an order with one, two and three fused frames in a row, every
output buffer pre-filled with a sentinel byte, and each frame must be the bits of the same frame from a fresh scene: a set of
counters that was not zero hands out too few tiles and leaves the sentinel standing.  The same with two contexts on two streams
in turn."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_resolve_cases as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def here(gpu):
    assert not any(v in os.environ for v in ("RAYCA_FUSE_RESOLVE", "RAYCA_LAST_FORM", "RAYCA_HIP_LIB"))
    return F.render_cases()


@pytest.fixture(scope="module")
def counting(gpu):
    return F.render_cases(collect_stats=True)


@pytest.fixture(scope="module")
def wavefront(gpu):
    from rayca_amd import abi
    return F.render_cases(engine=abi.ENGINE_WAVEFRONT)


@pytest.fixture(scope="module")
def unfused(gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fused_resolve") / "frames.npz")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "fused_resolve_cases.py"), out],
                       env=dict(os.environ, RAYCA_FUSE_RESOLVE="0"), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAYCA_FUSE_RESOLVE = 0" in r.stdout, r.stdout
    return dict(np.load(out))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same_frame(a, b, key):
    kw = F.CASES[key.split("/")[0]][2]
    assert (key + "/u8" in a) == kw.get("want_rgba8", True) and (key + "/f32" in a) == kw.get("want_f32", True), key
    if key + "/u8" in a:
        assert np.array_equal(a[key + "/u8"], b[key + "/u8"]), key
    if key + "/f32" in a:
        assert same_bits(a[key + "/f32"], b[key + "/f32"]), key


@pytest.mark.parametrize("key", F.keys())
def test_frames_are_those_of_generation_and_resolve(here, unfused, key):
    assert_same_frame(here, unfused, key)
    ca, cb = here[key + "/counters"], unfused[key + "/counters"]
    print(key, dict(zip(F.COUNTER_KEYS, ca.tolist())))
    assert np.array_equal(ca, cb), f"{key}: {ca} vs {cb}"
    # the proxies of the four kinds: +0.0 pixels (misses, vertices in shadow) and pixels above zero (lit vertices, emitters)
    img = here[key + "/f32"][..., :3] if key + "/f32" in here else here[key + "/u8"][..., :3]
    flat = img.reshape(-1, 3)
    assert (flat == 0).all(axis=1).any() and (flat > 0).any(), key
    if key + "/f32" in here:
        assert (here[key + "/f32"][..., 3] == 1.0).all(), key
    if key.startswith("quad/"):
        assert (flat == 1.0).all(axis=1).sum() >= 10, "the emitter's pixels: the emission colour as it is"


@pytest.mark.parametrize("key", F.keys())
def test_frames_are_the_counting_frames(here, counting, key):
    assert_same_frame(here, counting, key)


@pytest.mark.parametrize("key", F.keys())
def test_frames_are_the_wavefront_engines(here, wavefront, key):
    assert_same_frame(here, wavefront, key)


@pytest.mark.parametrize("key", F.keys())
def test_the_form_is_picked_for_the_cases(here, counting, wavefront, unfused, key):
    launches, trace, fmt = here[key + "/stats"].tolist()
    assert (launches, trace) == (1, 1) and fmt & F.FUSED_BIT, "one launch, and it says so"
    assert fmt >> 16 == 1, "generation 0 on the last-vertex form"
    launches, trace, fmt = counting[key + "/stats"].tolist()
    assert (launches, trace) == (2, 1) and not fmt & F.FUSED_BIT and fmt >> 16 == 1, "a counting frame: generation + k_resolve"
    launches, trace, fmt = unfused[key + "/stats"].tolist()
    assert (launches, trace) == (2, 1) and not fmt & F.FUSED_BIT and fmt >> 16 == 1, "RAYCA_FUSE_RESOLVE=0: generation + k_resolve"
    assert not wavefront[key + "/stats"][2] & F.FUSED_BIT and wavefront[key + "/stats"][0] > 2, "the wavefront engine has no such form"


@pytest.mark.parametrize("key", F.off_keys())
def test_the_form_is_not_picked_elsewhere(here, unfused, key):
    want = F.OFF[key.split("/")[0]][3]
    for side in (here, unfused):
        launches, _, fmt = side["off/" + key + "/stats"].tolist()
        assert launches == want and not fmt & F.FUSED_BIT, key
    assert np.array_equal(here["off/" + key + "/u8"], unfused["off/" + key + "/u8"]), key
    assert same_bits(here["off/" + key + "/f32"], unfused["off/" + key + "/f32"]), key


def test_a_radiance_query_keeps_its_launches(gpu):
    import torch
    from rayca_amd import Config
    scenes = F.scenes_of("sah", ["cornell"])
    ds, cfg = scenes["cornell"], Config(max_depth=1, seed=81)
    rays = ds.camera_rays(cfg, F.W, F.H)
    _, st = ds.radiance(rays, cfg, want_stats=True)
    torch.cuda.synchronize()
    assert st["kernel_launches"] == 5 and not st["node_format"] & F.FUSED_BIT   # enqueue, trace + shade + shadow, k_resolve
    for s in scenes.values():
        s.close()


# ---- counter bookkeeping --------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def sequence_steps():
    """(name, what) in an order with one, two and three fused frames in a row and something else between the runs, so that a fused
    frame finds its counters in every state: both sets clean, either one, neither"""
    from rayca_amd import Config, IntegratorStrategy
    small, large = (F.W, F.H), (200, 120)
    path = lambda seed: Config(max_depth=1, seed=seed)   # noqa: E731
    fused = lambda i, size: (f"path_{i}", dict(cfg=path(100 + i), size=size, launches=1))   # noqa: E731
    flat = lambda i: (f"flat_{i}", dict(cfg=Config(integrator=IntegratorStrategy.Flat, seed=120 + i), size=small, launches=1))   # noqa: E731
    return [
        fused(0, small),
        ("depth_3", dict(cfg=Config(max_depth=3, seed=130), size=small, launches=4)),
        fused(1, large), fused(2, small),
        ("wavefront", dict(cfg=path(131), size=small, engine="WAVEFRONT", launches=4)),
        fused(3, small), flat(0), fused(4, large),
        ("four_samples", dict(cfg=Config(max_depth=1, samples_per_pixel=4, seed=132), size=small, launches=8)),
        fused(5, large),
        ("counting", dict(cfg=path(133), size=small, collect_stats=True, launches=2)),
        flat(1), fused(6, small),
        ("query", dict(query=True)),
        fused(7, small), fused(8, large), flat(2),
        ("query_again", dict(query=True)),
        flat(3),
    ]


def run_step(ds, what, context, stream):
    """one step on `context`: (rgba8, rgba32f, launches) of a frame rendered into sentinel-filled device buffers, or the query's t"""
    import torch
    from rayca_amd import Config, abi
    if what.get("query"):
        rays = ds.camera_rays(Config(), F.W, F.H, stream=stream, context=context)
        t, _, _ = ds.query(rays, stream=stream, context=context)
        stream.synchronize()
        return (t.cpu().numpy(),)
    w, h = what["size"]
    u8 = torch.full((h, w, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    f32 = torch.full((h, w, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    st = ds.render_device(what["cfg"], w, h, u8.data_ptr(), f32.data_ptr(), stream=stream.cuda_stream, context=context, want_stats=True,
                          collect_stats=what.get("collect_stats", False), engine=getattr(abi, "ENGINE_" + what.get("engine", "FUSED")))
    stream.synchronize()
    return u8.cpu().numpy(), f32.cpu().numpy().view(np.float32), int(st["kernel_launches"])


def fresh(step):
    """the same step on a scene of its own, context 0"""
    import torch
    ds = F.scenes_of("sah", ["cornell"])
    try:
        return run_step(ds["cornell"], step, 0, torch.cuda.current_stream())
    finally:
        for s in ds.values():
            s.close()


@pytest.fixture(scope="module")
def expected(gpu):
    return {name: fresh(what) for name, what in sequence_steps()}


def check_step(name, what, got, want):
    if what.get("query"):
        assert same_bits(got[0], want[0]), name
        return
    assert got[2] == what["launches"], f"{name}: {got[2]} launches"
    assert np.array_equal(got[0], want[0]), f"{name}: rgba8 ({int((got[0] == SENTINEL).all(axis=-1).sum())} pixels still hold the sentinel)"
    assert same_bits(got[1], want[1]), f"{name}: rgba32f"


def test_counters_over_a_sequence_on_one_context(gpu, expected):
    import torch
    scenes = F.scenes_of("sah", ["cornell"])
    ds = scenes["cornell"]
    stream = torch.cuda.Stream()
    for name, what in sequence_steps():
        check_step(name, what, run_step(ds, what, 3, stream), expected[name])
    for s in scenes.values():
        s.close()


def test_counters_over_a_sequence_on_two_contexts(gpu, expected):
    import torch
    scenes = F.scenes_of("sah", ["cornell"])
    ds = scenes["cornell"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    steps = sequence_steps()
    # context 0 runs the sequence forwards, context 1 backwards, in turn: each context's own history decides what it finds clean
    for i in range(len(steps)):
        for c, (name, what) in ((0, steps[i]), (1, steps[len(steps) - 1 - i])):
            check_step(name, what, run_step(ds, what, c, streams[c]), expected[name])
    for s in scenes.values():
        s.close()
