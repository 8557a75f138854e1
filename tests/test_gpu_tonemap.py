"""rayca_hip_meter_device and rayca_hip_tonemap_device (DeviceScene.meter, .tonemap, Film.resolve(tonemap=)) on the GPU.

Every comparison is bit for bit -- the 260 histogram words, the exposure record's float words, rgba32f_out as uint32 and rgba8_out
-- against the literal restatement (tests/tonemap_literal.py: the passes are +, -, x, / and integer arithmetic only, each float
operation rounded once, so the restatement has the kernels' bits), against the denoiser's output stage for a gamma other than 1,
and between the ways of making one call (an exposure record or a host scale, another stream and context, through Film)."""
import os

import numpy as np
import pytest

import tonemap_literal as tl
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, abi, flatten, scenes
from rayca_amd import model as M
from rayca_amd import sdtf

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
SIZES = [(1, 1), (7, 3), (64, 4), (65, 5), (256, 1), (333, 77)]   # (width, height): one pixel, partial tiles and blocks both ways, 26 meter blocks
TRIMS = [(0, 1000), (10, 990), (500, 501), (0, 1), (999, 1000)]
OPS = ("linear", "reinhard", "aces")


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


def special_values():
    """the channel values a frame of this pass can hold and the ones that sit on the seams of the bins: NaN, +-inf, +-0,
    negatives, denormals, values below 2^-16 and above 2^16, and every bin edge (1 + j / 8) 2^e of three octaves (the first, the
    one around 1, the last) with its two neighbours"""
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -1e-3, -3e38, 1e-45, 1e-42, 1.1e-38, -1e-40, 2.0 ** -20, 2.0 ** -17, 1e-6, 2.0 ** 16, 2.0 ** 17, 1e9, 3e38]
    for e in (-16, 0, 15):
        for j in range(9):   # (j = 8: the octave's end, the next one's first edge)
            edge = F((1 + j / 8) * 2.0 ** e)
            v += [edge, np.nextafter(edge, F(0)), np.nextafter(edge, F(np.inf))]
    return np.array(v, F)


_FRAMES = {}


def frame(width, height, specials=True):
    """a size's frame, made once and shared read-only: coloured log-normal radiance (sigma 2: five decades), alpha in [0, 2], and --
    as far as the size has room -- the special values as grey pixels, then each once in a single channel of a lit pixel"""
    key = (width, height, specials)
    if key not in _FRAMES:
        rng = np.random.default_rng(width * 1000 + height)
        c = np.exp(rng.normal(-1.0, 2.0, (height * width, 4))).astype(F)
        c[:, 3] = rng.uniform(0.0, 2.0, height * width).astype(F)
        if specials:
            v = special_values()
            at = rng.permutation(height * width)
            n = min(len(v), len(at))
            c[at[:n], :3] = v[:n, None]
            m = min(len(v), len(at) - n)
            c[at[n:n + m], np.arange(m) % 3] = v[:m]
        c = c.reshape(height, width, 4)
        c.setflags(write=False)
        _FRAMES[key] = c
    return _FRAMES[key]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a writable copy: the shared frames are read-only)


def host(x):
    return x.cpu().numpy()


def metered(ds, color, **kw):
    """DeviceScene.meter on a host frame: (hist as uint32, the record) on the host"""
    import torch
    hist, exposure = ds.meter(dev(color) if isinstance(color, np.ndarray) else color, **kw)[:2]
    torch.cuda.synchronize()
    return host(hist).view(np.uint32), host(exposure)


def assert_meter(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: histogram words {np.flatnonzero(got[0] != want[0])[:8].tolist()} differ"
    assert bits(got[1]).tolist() == bits(want[1]).tolist(), f"{what}: exposure {got[1].tolist()}, literal {want[1].tolist()}"


def assert_picture(got, want, what):
    """(rgba32f, rgba8) pairs, either member None where it was not asked for"""
    for name, g, w in zip(("rgba32f", "rgba8"), got, want):
        if g is None:
            continue
        same = (bits(g) == bits(w)) if g.dtype != np.uint8 else (g == w)
        bad = np.argwhere(~same.all(-1))
        assert bad.size == 0, f"{what}: {name}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


# ---- 1: metering -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SIZES)
def test_the_meter_equals_the_literal_at_every_size(ds, width, height):
    c = frame(width, height)
    assert_meter(metered(ds, c), tl.meter(c), f"{width} x {height}")


def test_every_block_strides_more_than_once(ds):
    """1024 x 1024 pixels are 1024 blocks' worth of 1024 lanes (kMeterBlock); the grid is capped at 256 blocks (kMeterMaxGrid), so
    every block takes four strides of its loop.  A frame without special values: all of them counted, in a hundred-odd bins."""
    c = frame(1024, 1024, specials=False)
    want = tl.meter(c)
    assert want[0][tl.COUNTED] == 1 << 20 and (want[0][:256] > 0).sum() > 100
    assert_meter(metered(ds, c), want, "1024 x 1024")


def test_special_values_and_every_trim(ds):
    c = frame(37, 11)
    hist = tl.histogram(c)
    v = special_values()
    assert hist[tl.NOT_FINITE] >= 6 and hist[tl.BLACK] >= 6 and hist[0] >= 5 and hist[255] >= 5 and len(v) * 2 <= 37 * 11   # (they are all in)
    for width, height in ((37, 11), (333, 77)):
        c = frame(width, height)
        for low, high in TRIMS:
            kw = dict(low_permille=low, high_permille=high, key=0.5, min_scale=2.0 ** -4, max_scale=2.0 ** 4)
            assert_meter(metered(ds, c, **kw), tl.meter(c, **kw), f"{width} x {height}, trim {low} / {high}")
    # fewer than 1000 counted pixels: the two narrow trims keep nothing, the fallback; of 25 thousand they keep a few dozen
    assert tl.trimmed(hist, 0, 1) == (0, 0) and tl.trimmed(hist, 500, 501) == (0, 0)
    assert all(0 < tl.trimmed(tl.histogram(c), low, high)[0] < 60 for low, high in ((0, 1), (500, 501), (999, 1000)))


def test_frames_with_nothing_to_count(ds):
    for name, c in (("black", np.zeros((5, 9, 4), F)), ("not finite", np.full((5, 9, 4), np.nan, F)), ("negative", -np.ones((5, 9, 4), F))):
        want = tl.meter(c)
        assert want[1].tolist() == [1.0, 1.0, 0.0, 0.0]
        assert_meter(metered(ds, c), want, name)
        prev = np.array([0.75, 3.0, 3.0, 3.0], F)
        assert_meter(metered(ds, c, prev=dev(prev), rate=0.25), tl.meter(c, prev=prev, rate=0.25), name + ", with a previous record")


def test_the_previous_record_and_the_rate(ds):
    import torch
    c = frame(65, 5)
    for rate in (1.0, 0.5, 2.0 ** -6):
        prev = np.array([3.25, 0.0, 0.0, 0.0], F)
        assert_meter(metered(ds, c, prev=dev(prev), rate=rate), tl.meter(c, prev=prev, rate=rate), f"rate {rate}")
    jump = tl.meter(c)
    for bad in (np.nan, 0.0, np.inf, -2.0):
        prev = np.array([bad, 1.0, 1.0, 1.0], F)
        got = metered(ds, c, prev=dev(prev), rate=0.5)
        assert_meter(got, tl.meter(c, prev=prev, rate=0.5), f"prev {bad}")
        assert bits(got[1]).tolist() == bits(jump[1]).tolist()
    # in place: exposure_out is exposure_prev, three steps towards the target
    record, hist = dev(np.array([3.25, 0.0, 0.0, 0.0], F)), torch.empty(260, dtype=torch.int32, device="cuda")
    want = np.array([3.25, 0.0, 0.0, 0.0], F)
    color = dev(c)
    for step in range(3):
        assert ds.meter(color, prev=record, out=(hist, record), rate=0.5)[1] is record
        want = tl.meter(c, prev=want, rate=0.5)[1]
    torch.cuda.synchronize()
    assert bits(host(record)).tolist() == bits(want).tolist() and want[0] != want[1]


def test_two_calls_give_the_same_words_and_garbage_is_overwritten(ds):
    import torch
    c = frame(333, 77)
    want = tl.meter(c)
    color = dev(c)
    first = metered(ds, color)
    hist = torch.full((260,), -559038737, dtype=torch.int32, device="cuda")
    record = torch.full((4,), float("nan"), device="cuda")
    second = metered(ds, color, out=(hist, record))
    assert_meter(first, want, "first call")
    assert_meter(second, want, "second call, into a histogram full of garbage")
    # the histogram alone (no exposure_out) through the C ABI's rule: every word is still written
    import ctypes as C
    hist.fill_(-1)
    m = abi.RaycaMeter()
    m.width, m.height, m.low_permille, m.high_permille, m.key, m.min_scale, m.max_scale, m.rate = 333, 77, 10, 990, 0.18, 0.5, 2.0, 1.0
    m.color, m.hist_out = color.data_ptr(), hist.data_ptr()
    st = abi.RaycaStats()
    assert ds._lib.rayca_hip_meter_device(ds.handle, None, C.byref(m), C.byref(st)) == abi.OK
    assert np.array_equal(host(hist).view(np.uint32), want[0])
    assert st.kernel_launches == 2 and st.class_launches[abi.KERNEL_OTHER] == 2 and st.kernel_ms > 0


# ---- 2: tone mapping ---------------------------------------------------------------------------------------------------------------
def mapped(ds, color, op, *, float_out=True, **kw):
    """DeviceScene.tonemap on a host frame: (rgba32f or None, rgba8 or None) on the host"""
    import torch
    out = ds.tonemap(dev(color) if isinstance(color, np.ndarray) else color, op, out=None if float_out else False, **kw)
    torch.cuda.synchronize()
    out = out if isinstance(out, tuple) else (out,)
    out = tuple(host(x) for x in out)
    if not float_out:
        return (None,) + out
    return out if len(out) == 2 else out + (None,)


@pytest.mark.parametrize("op", OPS)
def test_every_operator_with_a_record_and_with_a_host_scale(ds, op):
    """... at every size, both outputs; the record's word 0 and the host's scale are the same float32, so are the bits"""
    for width, height in SIZES:
        c = frame(width, height)
        scale = F(0.37)
        want = tl.tonemap(c, op, scale=scale)
        record = dev(np.array([scale, 9.0, 9.0, 9.0], F))
        assert_picture(mapped(ds, c, op, scale=float(scale), rgba8=True), want, f"{op}, {width} x {height}, host scale")
        assert_picture(mapped(ds, c, op, exposure=record, scale=123.0, rgba8=True), want, f"{op}, {width} x {height}, exposure record")


@pytest.mark.parametrize("op", OPS)
def test_output_subsets_white_points_and_in_place(ds, op):
    import torch
    c = frame(65, 5)
    whites = (0.0, 4.0) if op == "reinhard" else (0.0,)
    for white in whites:
        want = tl.tonemap(c, op, scale=2.0, white=white)
        what = f"{op}, white {white}"
        assert_picture(mapped(ds, c, op, scale=2.0, white=white), want, what + ", float only")
        assert_picture(mapped(ds, c, op, scale=2.0, white=white, rgba8=True, float_out=False), want, what + ", RGBA8 only")
        assert_picture(mapped(ds, c, op, scale=2.0, white=white, rgba8=True), want, what + ", both")
        color = dev(c)
        assert ds.tonemap(color, op, scale=2.0, white=white, out=color) is color
        torch.cuda.synchronize()
        assert_picture((host(color), None), want, what + ", in place")
    if op == "reinhard":
        assert not np.array_equal(bits(tl.tonemap(c, op, scale=2.0)[0]), bits(tl.tonemap(c, op, scale=2.0, white=4.0)[0]))


def test_the_special_values_come_out_as_the_arithmetic_has_them(ds):
    """what the bit-for-bit comparisons cover, looked at once on the literal: alpha untouched, NaN and inf channels stay not finite,
    a -0 stays a -0 under every operator"""
    c = frame(37, 11)
    for op in OPS:
        out, _ = tl.tonemap(c, op, scale=0.5)
        assert np.array_equal(bits(out[..., 3]), bits(c[..., 3]))
        assert not np.isfinite(out[~np.isfinite(c)]).any()
        grey_zero = (bits(c[..., :3]) == 0x80000000).all(-1)
        assert grey_zero.any() and (bits(out[grey_zero][:, :3]) == 0x80000000).all()
        assert_picture(mapped(ds, c, op, scale=0.5, rgba8=True), tl.tonemap(c, op, scale=0.5), op)


@pytest.mark.parametrize("op", OPS)
def test_gamma_is_the_denoisers_output_stage(ds, op):
    """gamma 2.2 against DeviceScene.denoise(iterations=0, gamma=2.2) -- finalize_pixel alone, which is what this pass calls -- on
    the literal's gamma-1 float output"""
    import torch
    c = frame(65, 5)
    lin = tl.tonemap(c, op, scale=1.5)[0]
    want, want8 = ds.denoise(dev(lin), iterations=0, gamma=2.2, rgba8=True)
    torch.cuda.synchronize()
    assert_picture(mapped(ds, c, op, scale=1.5, gamma=2.2, rgba8=True), (host(want), host(want8)), f"{op}, gamma 2.2")
    assert not np.array_equal(bits(host(want)), bits(lin))


# ---- 3: both entries ---------------------------------------------------------------------------------------------------------------
def test_a_strided_frame_equals_a_contiguous_one(ds):
    """a frame that is not contiguous reaches the kernels as a contiguous copy: the contiguous calls' words and bits"""
    from strided import strided
    c = frame(65, 5)
    assert_meter(metered(ds, strided(dev(c))), metered(ds, c), "strided frame")
    assert_picture(mapped(ds, strided(dev(c)), "reinhard", scale=2.0, rgba8=True), mapped(ds, c, "reinhard", scale=2.0, rgba8=True), "strided frame")


def test_a_callers_stream_another_context_and_the_statistics(ds):
    import torch
    c = frame(333, 77)
    want_m, want_t = tl.meter(c), tl.tonemap(c, "aces", scale=0.25)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        color = dev(c)
        hist, record = ds.meter(color, stream=stream, context=3)
        out, out8 = ds.tonemap(color, "aces", scale=0.25, rgba8=True, stream=stream, context=3)
    stream.synchronize()
    assert_meter((host(hist).view(np.uint32), host(record)), want_m, "a caller's stream, context 3")
    assert_picture((host(out), host(out8)), want_t, "a caller's stream, context 3")
    hist, record, stats = ds.meter(color, want_stats=True)
    assert_meter((host(hist).view(np.uint32), host(record)), want_m, "with statistics")
    assert stats["kernel_launches"] == 3 and stats["class_launches"][abi.KERNEL_OTHER] == 3 and stats["kernel_ms"] > 0
    out, stats = ds.tonemap(color, "aces", scale=0.25, want_stats=True)
    assert_picture((host(out), None), want_t, "with statistics")
    assert stats["kernel_launches"] == 1 and stats["class_launches"][abi.KERNEL_OTHER] == 1 and stats["kernel_ms"] > 0
    assert stats["class_ms"][abi.KERNEL_OTHER] == stats["kernel_ms"] and stats["rays_primary"] == 0


def test_meter_then_tonemap_on_one_stream_without_a_host_wait(ds):
    """the record never leaves the device: the operator reads what the meter wrote, ordered by the stream alone"""
    import torch
    c = frame(333, 77)
    want_m = tl.meter(c, key=0.25)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        color = dev(c)
        for op in OPS:   # (three chains back to back: each meter call rewrites the histogram and the record the last operator read)
            hist, record = ds.meter(color, key=0.25, stream=stream)
            out, out8 = ds.tonemap(color, op, exposure=record, rgba8=True, stream=stream)
    stream.synchronize()
    assert_meter((host(hist).view(np.uint32), host(record)), want_m, "the chain's meter")
    assert_picture((host(out), host(out8)), tl.tonemap(c, OPS[-1], scale=want_m[1][0]), "the chain's picture")


def test_errors_reach_the_caller(ds):
    import torch
    from rayca_amd.lib import RaycaError
    color = dev(frame(7, 3))
    with pytest.raises(ValueError, match="op"):
        ds.tonemap(color, "filmic")
    with pytest.raises(RaycaError, match="white"):
        ds.tonemap(color, "aces", white=2.0)
    with pytest.raises(RaycaError, match="rate"):
        ds.meter(color, rate=0.0)
    with pytest.raises(ValueError, match="shape"):
        ds.meter(color, prev=torch.zeros(3, device="cuda"))
    torch.cuda.synchronize()


# ---- 4: the film -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def film(gpu):
    """the Cornell fixture at 128 x 72, two frames in"""
    scene = DeviceScene(make_desc("cornell_quad"), Config(), builder=abi.BUILDER_SAH)
    f = Film(scene, 128, 72)
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=2.2, seed=3)
    f.add(cfg)
    f.add(cfg)
    yield f
    scene.close()


def test_film_resolve_tonemapped_is_the_same_steps_made_by_hand(film):
    import torch
    scene = film.scene
    film._exposure = None
    got, got8 = film.resolve(tonemap="aces", exposure="auto", rgba8=True)
    hist, record = scene.meter(film.color)
    want, want8 = scene.tonemap(film.color, "aces", exposure=record, gamma=2.2, rgba8=True)
    torch.cuda.synchronize()
    assert_picture((host(got), host(got8)), (host(want), host(want8)), "resolve(tonemap='aces', exposure='auto')")
    assert bits(host(film.exposure)).tolist() == bits(host(record)).tolist()
    # ... and against the literal: the meter's words, and the picture with gamma 1
    c = host(film.color)
    assert_meter((host(hist).view(np.uint32), host(record)), tl.meter(c), "the film's colour")
    lin = film.resolve(tonemap="aces", exposure=float(host(record)[0]), gamma=1.0, rgba8=True)
    torch.cuda.synchronize()
    assert_picture((host(lin[0]), host(lin[1])), tl.tonemap(c, "aces", scale=host(record)[0]), "resolve(tonemap='aces', exposure=float)")
    assert 0.0 < float(host(record)[2]) < 10.0 and got.shape == (72, 128, 4)
    # behind the denoiser the same steps: the filter with gamma 1, then the meter and the operator on its result
    before = film.exposure   # (the record the next resolve steps from; it writes the other one)
    got = film.resolve(tonemap="reinhard", exposure="auto", denoise=True, tonemap_kw=dict(white=4.0, rate=0.75))
    den = film.resolve(denoise=True, gamma=1.0)
    _, record = scene.meter(den, prev=before, rate=0.75)
    want = scene.tonemap(den, "reinhard", exposure=record, white=4.0, gamma=2.2)
    torch.cuda.synchronize()
    assert_picture((host(got), None), (host(want), None), "behind the denoiser")


def test_two_resolves_walk_the_exposure_as_the_literal_does(film):
    import torch
    film._exposure = None
    assert film.exposure is None
    c = host(film.color)
    kw = dict(rate=0.5, key=0.3)
    film.resolve(tonemap="linear", exposure="auto", tonemap_kw=kw)
    first = film.exposure
    film.resolve(tonemap="linear", exposure="auto", tonemap_kw=kw)
    second = film.exposure
    got = film.resolve(tonemap="linear", exposure="auto", gamma=1.0, tonemap_kw=kw)
    torch.cuda.synchronize()
    want = [tl.meter(c, **kw)[1]]   # the first resolve has no previous record: the target
    for _ in range(2):
        want.append(tl.meter(c, prev=want[-1], **kw)[1])
    assert first is not second and film.exposure is first   # (the two records change roles)
    assert bits(host(second)).tolist() == bits(want[1]).tolist()
    assert bits(host(film.exposure)).tolist() == bits(want[2]).tolist()
    assert_picture((host(got), None), tl.tonemap(c, "linear", scale=want[2][0]), "the third resolve's picture")
    film.reset()
    assert film.exposure is None
    film.add(Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=2.2, seed=3))   # (the fixture is shared)


def test_resolve_without_tonemap_is_what_it_was(film):
    """the output stage alone on the film's colour, with the gamma of the config last added"""
    import torch
    got, got8 = film.resolve(rgba8=True)
    want, want8 = film.scene.denoise(film.color, iterations=0, gamma=2.2, rgba8=True)
    torch.cuda.synchronize()
    assert_picture((host(got), host(got8)), (host(want), host(want8)), "resolve()")
    with pytest.raises(ValueError, match="only with tonemap"):
        film.resolve(exposure="auto")
