"""Exposure metering and tone mapping without a GPU: what their specification promises, checked on the literal restatement
(tests/tonemap_literal.py), and what rayca_hip_meter_device and rayca_hip_tonemap_device refuse, checked through the C ABI in
front of any GPU work (any non-NULL value will do for the scene handle, as in tests/test_upsample_cpu.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tonemap_literal as tl
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def grey(values, alpha=1.0):
    """an (N, 1, 4) frame with r = g = b = values"""
    v = np.asarray(values, F).reshape(-1, 1, 1)
    return np.concatenate([v, v, v, np.full_like(v, alpha)], -1)


def lognormal(seed=7, shape=(48, 64), mu=-1.5, sigma=1.5):
    """the firefly case's frame: a grey log-normal frame"""
    rng = np.random.default_rng(seed)
    return grey(np.exp(rng.normal(mu, sigma, shape[0] * shape[1]))).reshape(shape[0], shape[1], 4)


# ---- the meter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.18, 1.0, 1.0625, 1.99, 3e-4, 4000.0, 2.0 ** -15, 2.0 ** 16 * 0.99])
def test_a_uniform_frame_meters_its_luminance_within_half_a_bin(value):
    """every pixel in one bin i: Q = (2 i + 1) << 12, the bin's centre -- within 1/16 of any luminance of the bin"""
    frame = np.broadcast_to(grey([value]), (5, 7, 4))
    y = float(tl.luminance(F(value), F(value), F(value)))
    hist, exp = tl.meter(frame)
    assert hist[tl.COUNTED] == 35 and hist[:256].max() == 35
    assert abs(float(exp[2]) / y - 1.0) <= 1.0 / 16.0
    if value == 0.18:
        assert float(exp[2]) == 0.1796875
    assert exp[0] == exp[1] == min(max(F(F(0.18) / exp[2]), F(2.0 ** -10)), F(2.0 ** 10)) and exp[3] == 0


def test_a_power_of_two_moves_the_metered_luminance_exactly():
    """x 2^k moves every counted pixel by 8 k bins (everything stays inside 2^+-16), so T moves by 16 k K and Q by k << 16"""
    frame = lognormal()
    assert 2.0 ** -11 < frame[..., 0].min() and frame[..., 0].max() < 2.0 ** 11
    _, base = tl.meter(frame, key=1.0, min_scale=2.0 ** -30, max_scale=2.0 ** 30)
    for k in (-5, -1, 1, 3, 5):
        _, e = tl.meter(frame * F(2.0 ** k), key=1.0, min_scale=2.0 ** -30, max_scale=2.0 ** 30)
        assert e[2] == base[2] * F(2.0 ** k)
        assert e[1] == base[1] / F(2.0 ** k) and e[0] == e[1]


def test_permuting_the_pixels_leaves_the_histogram_unchanged():
    frame = lognormal(3)
    frame[5, 6, 0], frame[7, 8, 1], frame[9, 10] = np.nan, np.inf, 0.0
    perm = np.random.default_rng(1).permutation(48 * 64)
    shuffled = frame.reshape(-1, 4)[perm].reshape(64, 48, 4)
    assert np.array_equal(tl.histogram(frame), tl.histogram(shuffled))
    h = tl.histogram(frame)
    assert (h[tl.COUNTED], h[tl.BLACK], h[tl.NOT_FINITE], h[259]) == (48 * 64 - 3, 1, 2, 0) and h[:256].sum() == h[tl.COUNTED]


def test_trimming_keeps_fireflies_out_of_the_metered_luminance():
    """fifteen pixels of 1e4 in a 64 x 48 log-normal frame (mu -1.5, sigma 1.5): the frame metered at 10 / 990 is nearer the clean
    frame's luminance than the same frame metered at 0 / 1000"""
    clean = lognormal()
    dirty = clean.copy()
    at = np.random.default_rng(11).choice(48 * 64, 15, replace=False)
    dirty.reshape(-1, 4)[at, :3] = 1e4
    want = float(tl.meter(clean)[1][2])
    trim = float(tl.meter(dirty)[1][2])
    full = float(tl.meter(dirty, low_permille=0, high_permille=1000)[1][2])
    print(f"clean {want:.4f}, with fireflies: trimmed {trim:.4f}, untrimmed {full:.4f}")
    assert abs(trim - want) < abs(full - want)


def test_bins_edges_and_the_three_classes():
    """a luminance on a bin edge (1 + j / 8) 2^e belongs to the bin it opens, its predecessor to the one below -- against the bin
    worked out another way, from frexp; below 2^-16 (denormals too) the first bin, from 2^16 the last; -0, 0 and negatives are
    black; NaN and inf (and the NaN of inf - inf in the luminance) are not finite"""
    seen = set()
    for e, j in ((-16, 0), (-16, 1), (-3, 5), (0, 0), (0, 7), (15, 7)):
        edge = F((1 + j / 8) * 2.0 ** e)
        for value in (edge, np.nextafter(edge, F(0)), np.nextafter(edge, F(np.inf)), edge * F(1.0000005), edge * F(0.9999995)):
            pixel = np.array([[[value, value, value, 1.0]]], F)
            lum = tl.luminance(pixel[0, 0, 0], pixel[0, 0, 1], pixel[0, 0, 2])   # (the value to a rounding or two: either side of the edge)
            mant, exp = np.frexp(np.float64(lum))   # lum = mant 2^exp, mant in [0.5, 1)
            want = (int(exp) - 1 + 16) * 8 + int((mant * 2 - 1) * 8)
            h = tl.histogram(pixel)
            assert h[min(max(want, 0), 255)] == 1 and h[tl.COUNTED] == 1, (e, j, value)
            seen.add(want - ((e + 16) * 8 + j))
    assert seen == {-1, 0}   # (both sides of an edge were met)
    for value, word in ((1e-42, 0), (2.0 ** -17, 0), (2.0 ** 16, 255), (3e38, 255)):
        h = tl.histogram(grey([value]))
        assert h[word] == 1 and h[tl.COUNTED] == 1, value
    for value in (0.0, -0.0, -1.0, -1e-40):
        assert tl.histogram(grey([value]))[tl.BLACK] == 1, value
    for pixel in ((np.nan, 1, 1, 1), (1, np.inf, 1, 1), (1, 1, -np.inf, 1), (np.inf, 1, -np.inf, 1)):
        assert tl.histogram(np.array([[pixel]], F))[tl.NOT_FINITE] == 1, pixel
    assert tl.histogram(np.array([[(1, 1, 1, np.nan)]], F))[tl.COUNTED] == 1   # (alpha is not looked at)


@pytest.mark.parametrize("frame", [np.zeros((4, 6, 4), F), np.full((4, 6, 4), np.nan, F), -np.ones((4, 6, 4), F)], ids=["black", "nan", "negative"])
def test_nothing_counted_falls_back(frame):
    """K = 0: L = 0, the target is the usable previous scale, else 1"""
    hist, e = tl.meter(frame)
    assert hist[tl.COUNTED] == 0 and tl.trimmed(hist, 10, 990) == (0, 0)
    assert e.tolist() == [1.0, 1.0, 0.0, 0.0]
    _, e = tl.meter(frame, prev=np.array([0.75, 9, 9, 9], F), rate=0.25)
    assert e.tolist() == [0.75, 0.75, 0.0, 0.0]
    _, e = tl.meter(frame, prev=np.array([np.nan, 9, 9, 9], F), rate=0.25)
    assert e.tolist() == [1.0, 1.0, 0.0, 0.0]


def test_a_trim_that_keeps_nothing_falls_back_too():
    """(0, 1) of fewer than 1000 counted pixels: b = 0, K = 0"""
    hist, e = tl.meter(lognormal()[:10, :10], low_permille=0, high_permille=1)
    assert hist[tl.COUNTED] == 100 and e.tolist() == [1.0, 1.0, 0.0, 0.0]


def test_rate_and_the_previous_record():
    frame = np.broadcast_to(grey([0.36]), (3, 3, 4))
    _, jump = tl.meter(frame)
    target = jump[1]
    for bad in (0.0, -2.0, np.nan, np.inf, -np.inf):   # an unusable prev is ignored, whatever the rate
        _, e = tl.meter(frame, prev=np.array([bad, 0, 0, 0], F), rate=0.5)
        assert bits(e).tolist() == bits(jump).tolist(), bad
    prev = np.array([4.0, 0, 0, 0], F)
    _, e = tl.meter(frame, prev=prev, rate=1.0)   # rate 1 gives the target: p + (t - p) is t here, both being small dyadic values
    assert e[0] == F(4.0) + (target - F(4.0)) and e[1] == target
    assert abs(float(e[0]) - float(target)) <= float(np.spacing(F(4.0)))
    _, e = tl.meter(frame, prev=prev, rate=0.5)
    assert e[0] == F(4.0) + (target - F(4.0)) * F(0.5) and e[1] == target and e[2] == jump[2]
    _, e = tl.meter(frame, prev=prev, rate=2.0 ** -6)
    assert e[0] == F(4.0) + (target - F(4.0)) * F(2.0 ** -6)


def test_the_target_is_clamped():
    dark, bright = np.broadcast_to(grey([1e-4]), (2, 2, 4)), np.broadcast_to(grey([1e4]), (2, 2, 4))
    assert tl.meter(dark)[1][1] == F(2.0 ** 10) and tl.meter(bright)[1][1] == F(2.0 ** -10)
    assert tl.meter(dark, max_scale=8.0)[1][1] == F(8.0) and tl.meter(bright, min_scale=0.5, max_scale=0.5)[1][1] == F(0.5)
    assert tl.meter(dark, max_scale=2.0 ** 20)[1][1] == F(F(0.18) / tl.meter(dark)[1][2])


# ---- the operators -----------------------------------------------------------------------------------------------------------------
def grid():
    """0, then (1 + j / 8) 2^e up to 2^8 and whole octaves from there to 2^16.  Spacing against rounding: an operator is a handful
    of float32 operations (ACES: eight), so a computed value lies within about eight half-ulps, 5e-7 relative, of the true one.
    Neighbouring true values differ by far more: Reinhard and ACES approach their limit like c / x (c = 1 and 0.238), so the
    steps are c (1 / x0 - 1 / x1): at 2^8 with x1 = 1.125 x0 at least 1e-4, over the last octave 3.6e-6 (ACES, the smaller), both
    well above 5e-7 of a value near 1; below 1 the operators grow about linearly, a step of 1/9 of the value."""
    fine = [(1 + j / 8) * 2.0 ** e for e in range(-16, 8) for j in range(8)]
    return np.array([0.0] + fine + [2.0 ** e for e in range(8, 17)], F)


@pytest.mark.parametrize("op,white", [("linear", 0.0), ("reinhard", 0.0), ("reinhard", 4.0), ("aces", 0.0)])
def test_every_operator_is_monotone(op, white):
    x = grid()
    out, _ = tl.tonemap(grey(x), op, white=white)
    for k in range(3):
        assert (np.diff(out[:, 0, k].astype(np.float64)) > 0).all(), (op, k)
    assert np.array_equal(out[:, 0, 3], np.ones(len(x), F))
    # ... in a coloured pixel too, along its ray (scale is what the exposure moves)
    pixel = np.array([[[0.9, 0.3, 0.05, 0.5]]], F)
    along = np.concatenate([tl.tonemap(pixel, op, scale=s, white=white)[0] for s in x[1:]])
    assert (np.diff(along[:, 0, :3].astype(np.float64), axis=0) > 0).all() and (along[:, 0, 3] == F(0.5)).all()


def test_linear_at_scale_one_is_the_output_stage_alone():
    frame = lognormal(5)
    frame[0, 0], frame[1, 1, 1], frame[2, 2, 2], frame[3, 3, 0] = (-0.0, 0.0, 2.5, -3.0), np.nan, np.inf, 1e-42
    frame[..., 3] = np.linspace(0, 2, 48 * 64, dtype=F).reshape(48, 64)
    out, out8 = tl.tonemap(frame, "linear")
    assert np.array_equal(bits(out), bits(frame)) and np.array_equal(out8, tl.quantize(frame))   # (x * 1.0f is x, a -0 and a NaN too)


def test_reinhard_maps_its_white_point_to_one():
    """Y = w: m = (1 + w / w^2) / (1 + w) is (1 + 1 / w) / (1 + w) = 1 / w, so x m = 1 for a grey pixel x = w -- to the roundings on
    the way, each at most 2^-24 relative: five in the luminance (the float32 weights sum to 1 to one more), w w, its reciprocal,
    Y inv_white2, the two sums, the quotient and the final product: twelve, 12 x 2^-24 in all"""
    for w in (1.0, 4.0, 7.3, 100.0, 0.37):
        x = F(w)   # a grey pixel's luminance is x to two roundings (the weights sum to 1 to a rounding)
        out, _ = tl.tonemap(grey([x]), "reinhard", white=w)
        assert abs(float(out[0, 0, 0]) - 1.0) <= 12 * 2.0 ** -24, (w, out[0, 0])
        assert out[0, 0, 0] == out[0, 0, 1] == out[0, 0, 2]
    # (That bound is wider than "the rounding of its three operations" because a pixel's Y is itself five rounded operations away
    # from w.)  With the white point set to the pixel's own float32 luminance, Y = w exactly, and what is left is the operator's
    # own arithmetic: m = (1 + Y inv_white2) / (1 + Y) -- a product, two sums and the quotient, four roundings -- on top of the
    # host's inv_white2 = 1 / (w w), two more: Y m, the mapped luminance, is 1 to 6 x 2^-24 (the last product taken in double)
    for pixel in ((0.9, 0.3, 0.05), (4.0, 4.0, 4.0), (0.01, 7.0, 120.0), (0.2, 0.1, 0.4)):
        r, g, b = (F(v) for v in pixel)
        y = tl.luminance(r, g, b)
        inv = F(1) / (y * y)
        m = (F(1) + y * inv) / (F(1) + y)
        assert type(m) is F and abs(float(y) * float(m) - 1.0) <= 6 * 2.0 ** -24, (pixel, float(y) * float(m))
        out, _ = tl.tonemap(np.array([[[r, g, b, 1.0]]], F), "reinhard", white=float(y))
        assert bits(out[0, 0, :3]).tolist() == bits(np.array([r * m, g * m, b * m], F)).tolist()
    # without a white point the operator is x / (1 + Y), and a pixel that is not lit passes through
    out, _ = tl.tonemap(np.array([[[2.0, 2.0, 2.0, 1.0], [0.0, -0.0, 0.0, 1.0], [-1.0, -1.0, -1.0, 1.0]]], F), "reinhard")
    y = tl.luminance(F(2), F(2), F(2))
    assert out[0, 0, 0] == F(2) * ((F(1) + y * F(0)) / (F(1) + y))
    assert bits(out[0, 1]).tolist() == bits(np.array([0.0, -0.0, 0.0, 1.0], F)).tolist() and out[0, 2].tolist() == [-1, -1, -1, 1]


def test_aces_on_its_landmarks():
    """0 maps to 0 (the numerator's factor x); the limit is 2.51 / 2.43; a channel that is not finite comes out as the arithmetic has it"""
    out, out8 = tl.tonemap(np.array([[[0.0, 1.0, 2.0 ** 16, 0.25], [np.nan, np.inf, -0.0, 2.0]]], F), "aces")
    one = (F(1) * (F(2.51) * F(1) + F(0.03))) / (F(1) * (F(2.43) * F(1) + F(0.59)) + F(0.14))
    assert out[0, 0, 0] == 0 and out[0, 0, 1] == one and abs(float(out[0, 0, 2]) - 2.51 / 2.43) < 1e-5
    assert np.isnan(out[0, 1, 0]) and np.isnan(out[0, 1, 1]) and bits(out[0, 1, 2]) == bits(F(-0.0)) and out[0, 1, 3] == 2
    assert out8[0, 0].tolist() == [0, int(float(out[0, 0, 1]) * 255), 255, 63] and out8[0, 1].tolist() == [0, 0, 0, 255]


# ---- refusals through the C ABI --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calls(product_lib):
    """(meter, tonemap): call(options fields, **changes of the arguments); the arguments pass every check unless changed.  ptr
    stands for device pointers (nothing is launched): ptr(i) are distinct 16-byte aligned addresses."""
    dummy = C.create_string_buffer(1024)
    scene, base = C.cast(dummy, C.c_void_p), (C.addressof(dummy) + 15) // 16 * 16

    def ptr(i):
        return base + 16 * i

    def options(o_fields):
        o = abi.RaycaRenderOptions()
        for name, v in (o_fields or {}).items():
            target, _, leaf = name.rpartition(".")
            setattr(getattr(o, target) if target else o, leaf, v)
        return o

    def meter(o_fields=None, **fields):
        m = abi.RaycaMeter()
        m.width, m.height, m.low_permille, m.high_permille = 16, 8, 10, 990
        m.key, m.min_scale, m.max_scale, m.rate = 0.18, 2.0 ** -10, 2.0 ** 10, 1.0
        m.color, m.hist_out, m.exposure_out, m.exposure_prev = ptr(0), ptr(1), ptr(2), ptr(3)
        for k, v in fields.items():
            setattr(m, k, v)
        o = options(o_fields)
        return product_lib.rayca_hip_meter_device(scene, C.byref(o), C.byref(m), None)

    def tonemap(o_fields=None, **fields):
        t = abi.RaycaTonemap()
        t.width, t.height, t.op, t.scale, t.white, t.gamma = 16, 8, abi.TONEMAP_REINHARD, 1.0, 0.0, 1.0
        t.color, t.exposure, t.rgba32f_out, t.rgba8_out = ptr(0), ptr(2), ptr(4), ptr(5)
        for k, v in fields.items():
            setattr(t, k, v)
        o = options(o_fields)
        return product_lib.rayca_hip_tonemap_device(scene, C.byref(o), C.byref(t), None)

    meter.ptr = tonemap.ptr = ptr
    meter.keep = tonemap.keep = dummy
    return meter, tonemap


NAN, INF = float("nan"), float("inf")


def test_the_meter_refuses_bad_arguments_in_front_of_any_gpu_work(calls):
    meter, _ = calls
    ptr = meter.ptr
    cases = [(dict(color=None), "color"), (dict(hist_out=None), "hist_out"), (dict(width=0), "width"), (dict(height=0), "height"),
             (dict(width=65536, height=65536), "pixels"), (dict(reserved=1), "reserved"),
             (dict(low_permille=990, high_permille=990), "low_permille"), (dict(low_permille=991), "low_permille"), (dict(high_permille=1001), "high_permille"),
             (dict(low_permille=1000, high_permille=1000), "high_permille"), (dict(high_permille=0, low_permille=0), "high_permille"),
             (dict(color=ptr(0) + 4), "alignment"), (dict(color=ptr(0) + 8), "alignment"), (dict(exposure_out=ptr(2) + 4), "alignment"),
             (dict(hist_out=ptr(1) + 2), "alignment"), (dict(exposure_prev=ptr(3) + 1), "alignment"),
             (dict(hist_out=ptr(0)), "aliasing"), (dict(hist_out=ptr(2)), "aliasing"), (dict(hist_out=ptr(3)), "aliasing"), (dict(exposure_out=ptr(0)), "aliasing")]
    cases += [(dict(key=bad), "key") for bad in (0.0, -1.0, NAN)]
    cases += [(dict(min_scale=bad), "min_scale") for bad in (0.0, -1.0, NAN, INF)]
    cases += [(dict(max_scale=bad), "max_scale") for bad in (2.0 ** -11, -1.0, NAN, INF)]
    cases += [(dict(rate=bad), "rate") for bad in (0.0, -0.5, 1.0000001, NAN, INF)]
    for fields, word in cases:
        assert meter(**fields) == abi.ERR_BAD_ARG, fields
        assert word in last_error(), (fields, last_error())
    assert meter(width=2, height=1 << 26) == abi.ERR_UNSUPPORTED and "tiles" in last_error()


def test_the_tonemap_refuses_bad_arguments_in_front_of_any_gpu_work(calls):
    _, tonemap = calls
    ptr = tonemap.ptr
    cases = [(dict(color=None), "color"), (dict(width=0), "width"), (dict(height=0), "height"), (dict(width=65536, height=65536), "pixels"),
             (dict(reserved=1), "reserved"), (dict(op=3), "op"), (dict(op=0xFFFFFFFF), "op"), (dict(rgba32f_out=None, rgba8_out=None), "output"),
             (dict(op=abi.TONEMAP_ACES, white=4.0), "white"), (dict(op=abi.TONEMAP_LINEAR, white=1.0), "white"),
             (dict(color=ptr(0) + 4), "alignment"), (dict(rgba32f_out=ptr(4) + 8), "alignment"), (dict(rgba8_out=ptr(5) + 1), "alignment"),
             (dict(exposure=ptr(2) + 2), "alignment"), (dict(rgba8_out=ptr(0)), "aliasing"), (dict(rgba8_out=ptr(4)), "aliasing"),
             (dict(rgba8_out=ptr(2)), "aliasing"), (dict(rgba32f_out=ptr(2)), "aliasing"), (dict(exposure=ptr(0)), "aliasing")]
    cases += [(dict(white=bad), "white") for bad in (-1.0, NAN, INF)]
    cases += [(dict(exposure=None, scale=bad), "scale") for bad in (0.0, -1.0, NAN, INF)]
    cases += [(dict(gamma=bad), "gamma") for bad in (0.0, -1.0, NAN)]
    for fields, word in cases:
        assert tonemap(**fields) == abi.ERR_BAD_ARG, fields
        assert word in last_error(), (fields, last_error())
    assert tonemap(width=2, height=1 << 26) == abi.ERR_UNSUPPORTED and "tiles" in last_error()


def test_null_arguments(product_lib, calls):
    scene, o = C.cast(calls[0].keep, C.c_void_p), abi.RaycaRenderOptions()
    for fn, args in ((product_lib.rayca_hip_meter_device, abi.RaycaMeter()), (product_lib.rayca_hip_tonemap_device, abi.RaycaTonemap())):
        assert fn(None, C.byref(o), C.byref(args), None) == abi.ERR_BAD_ARG and "null" in last_error()
        assert fn(scene, C.byref(o), None, None) == abi.ERR_BAD_ARG and "null" in last_error()


OPTION_FIELDS = ("traversal", "collect_stats", "tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved")


def test_nothing_else_is_refused(calls):
    """The options are the last thing a call checks before it touches the scene handle (a dummy here): a struct that is refused for
    context 8 -- and for nothing else -- has passed every check of its own.  The ends of every range, every optional pointer
    absent, the overlaps that are allowed."""
    meter, tonemap = calls
    ptr = meter.ptr
    last = dict(context=8)
    valid_meter = [dict(), dict(exposure_out=None), dict(exposure_prev=None), dict(exposure_out=None, exposure_prev=None), dict(exposure_prev=ptr(2)),
                   dict(exposure_prev=ptr(3) + 4), dict(hist_out=ptr(1) + 4), dict(low_permille=0, high_permille=1000), dict(low_permille=0, high_permille=1),
                   dict(low_permille=999, high_permille=1000), dict(low_permille=500, high_permille=501), dict(key=1e-30), dict(key=INF), dict(rate=1e-30),
                   dict(min_scale=1e-38, max_scale=3e38), dict(min_scale=2.0, max_scale=2.0), dict(width=1, height=1), dict(width=1 << 16, height=(1 << 12) - 1)]
    for fields in valid_meter:
        assert meter(last, **fields) == abi.ERR_BAD_ARG and "context out of range" in last_error(), (fields, last_error())
    valid_tonemap = [dict(op=op) for op in (abi.TONEMAP_LINEAR, abi.TONEMAP_REINHARD, abi.TONEMAP_ACES)]
    valid_tonemap += [dict(white=4.0), dict(white=1e-30), dict(exposure=None), dict(exposure=None, scale=1e-30), dict(scale=0.0), dict(scale=NAN),
                      dict(rgba32f_out=None), dict(rgba8_out=None), dict(rgba32f_out=ptr(0)), dict(rgba32f_out=ptr(0), rgba8_out=None), dict(gamma=2.2),
                      dict(rgba8_out=ptr(5) + 4, exposure=ptr(2) + 4), dict(width=1, height=1), dict(width=1 << 16, height=(1 << 12) - 1)]
    for fields in valid_tonemap:
        assert tonemap(last, **fields) == abi.ERR_BAD_ARG and "context out of range" in last_error(), (fields, last_error())
    # ... while the options that every pass takes are taken, and the ones these passes do not take are refused
    for call in calls:
        assert call(dict(context=8, stream=1, wait_event=1, record_event=1)) == abi.ERR_BAD_ARG and "context out of range" in last_error()
        for field in OPTION_FIELDS:
            assert call({field: 1}) == abi.ERR_BAD_ARG, field
            assert "must be zero" in last_error() and field.partition(".")[0] in last_error(), (field, last_error())


# ---- the structs' layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("RaycaMeter", 72), ("RaycaTonemap", 64)])
def test_struct_layout_matches_header(name, size):
    struct = getattr(abi, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             f'printf("{name} %zu\\n", sizeof({name}));']
    for field, _ in struct._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof({name}, {field}));')
    lines.append('printf("ops %d %d %d\\n", RAYCA_TONEMAP_LINEAR, RAYCA_TONEMAP_REINHARD, RAYCA_TONEMAP_ACES);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    *rows, ops = out.strip().splitlines()
    want = dict(l.split() for l in rows)
    assert C.sizeof(struct) == int(want[name]) == size
    for field, _ in struct._fields_:
        assert getattr(struct, field).offset == int(want[field]), field
    assert len(want) == len(struct._fields_) + 1
    assert ops.split()[1:] == [str(v) for v in (abi.TONEMAP_LINEAR, abi.TONEMAP_REINHARD, abi.TONEMAP_ACES)]
    assert abi.TONEMAP_NAMES == ("linear", "reinhard", "aces") == tuple(k for k, _ in sorted(tl.OPS.items(), key=lambda kv: kv[1]))
