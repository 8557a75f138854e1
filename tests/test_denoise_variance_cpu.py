"""The variance-guided a-trous filter without a GPU: what its specification promises, checked on the literal restatement
(tests/denoise_variance_literal.py), and what rayca_hip_denoise_variance_device refuses, checked through the C ABI in front of
any GPU work (any non-NULL value will do for the scene handle, as in tests/test_pass_options_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import denoise_literal as dl
import denoise_variance_literal as dv
from rayca_amd import abi
from rayca_amd.lib import last_error

W, H = 61, 37
SIGMA_PLANE = 0.5
GUIDES = ("albedo", "normal", "point", "id")
_FRAMES = {}


def frame(samples):
    """the film-like frame of a history length, made once and shared read-only"""
    if samples not in _FRAMES:
        s = dv.film_like(W, H, 4242, samples)
        for a in s.values():
            a.setflags(write=False)
        _FRAMES[samples] = s
    return _FRAMES[samples]


def guides(s):
    return dict({k: s[k] for k in GUIDES}, sigma_plane=SIGMA_PLANE)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


# ---- 1-4: properties of the specification ------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [8, 32])
def test_ordering_against_the_input_and_the_plain_filter(samples):
    """a lighting checker that no guide shows, under noise that differs between the halves: the variance-guided filter improves
    the frame, the plain one (same guides, sigma_color 4) blurs the checker away and makes it worse than its input"""
    s = frame(samples)
    guided, _, _ = dv.denoise_variance(s["color"], s["variance"], length=s["length"], **guides(s))
    plain, _ = dl.denoise(s["color"], sigma_color=4.0, **guides(s))
    e_in, e_guided, e_plain = rmse(s["color"], s["clean"]), rmse(guided, s["clean"]), rmse(plain, s["clean"])
    print(f"N = {samples}: RMSE input {e_in:.4f}, plain {e_plain:.4f}, variance-guided {e_guided:.4f}")
    assert e_guided < e_in < e_plain
    half = H // 2   # ... and it improves the noisy half and the calm half each
    for rows in (slice(0, half), slice(half, H)):
        assert rmse(guided[rows], s["clean"][rows]) < rmse(s["color"][rows], s["clean"][rows])


def test_a_clean_frame_is_left_alone():
    """no noise, variance 0, a history at least min_history long: every tap across a luminance step weighs 1 / (1 + d^2 / floor),
    so what is left is a 25-tap mean of (nearly) equal values: one rounding per product, sum and quotient"""
    s = frame(8)
    zero = np.zeros((H, W), dl.F)
    for iterations in (1, 5):
        out, _, var_out = dv.denoise_variance(s["clean"], zero, length=s["length"], min_history=4, iterations=iterations, **guides(s))
        rel = float((np.abs(out[..., :3] - s["clean"][..., :3]) / np.abs(s["clean"][..., :3])).max())
        print(f"{iterations} iterations: max relative change {rel:.3g}")
        assert rel <= iterations * 64 * 2.0 ** -24
        assert np.array_equal(out[..., 3], s["clean"][..., 3])
        assert not var_out.any()


def test_the_filter_backs_off_as_the_history_grows():
    s = frame(8)
    moved = []
    for length in (4, 16, 64, 256, 1024):
        out, _, _ = dv.denoise_variance(s["color"], s["variance"], length=np.full((H, W), length, dl.F), min_history=4, **guides(s))
        moved.append(float(np.abs(out[..., :3] - s["color"][..., :3]).mean()))
    print("mean |out - in| over the lengths:", moved)
    assert all(a > b for a, b in zip(moved, moved[1:])), moved


def test_the_variance_shrinks_with_the_iterations():
    s = frame(8)
    means, errors = [], {}
    for iterations in (1, 2, 3, 5):
        out, _, var_out = dv.denoise_variance(s["color"], s["variance"], length=s["length"], iterations=iterations, **guides(s))
        means.append(float(var_out.astype(np.float64).mean()))
        errors[iterations] = rmse(out, s["clean"])
    print("mean variance_out:", means, "RMSE:", errors)
    assert all(a > b for a, b in zip(means, means[1:])), means
    assert errors[5] < rmse(s["color"], s["clean"])   # (the RMSE itself is not monotone in the iteration count)


def test_a_short_history_takes_the_spatial_estimate():
    """min_history decides per pixel: below it the 7 x 7 estimate, at or above it the temporal one; a NaN length fails the
    comparison and keeps the temporal one"""
    s = frame(8)
    length = np.array(s["length"])
    length[:, : W // 2] = 2.0
    length[5, 40] = np.nan
    c = np.array(s["color"])
    c[..., :3] = c[..., :3] / np.fmax(s["albedo"][..., :3], dl.F(1e-3))
    kw = dict(normal=s["normal"], point=s["point"], id=s["id"], sigma_plane=SIGMA_PLANE)
    ld = dv.lum(np.fmax(s["albedo"][..., :3], dl.F(1e-3)))
    with_fallback = dv.initial_variance(c, s["variance"], ld=ld, length=length, min_history=4, **kw)
    without = dv.initial_variance(c, s["variance"], ld=ld, length=length, min_history=0, **kw)
    differs = with_fallback != without
    assert differs[:, : W // 2].mean() > 0.99 and not differs[:, W // 2:].any()
    assert not np.isnan(with_fallback).any() and with_fallback[5, 40] == without[5, 40]


# ---- 5: refusals through the C ABI -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options fields, **changes of the arguments): the arguments pass every check unless changed"""
    dummy = C.create_string_buffer(256)
    scene, ptr = C.cast(dummy, C.c_void_p), (C.addressof(dummy) + 15) // 16 * 16   # (ptr stands for a device pointer: nothing is launched)

    def run(o_fields=None, **fields):
        d = abi.RaycaDenoiseVariance()
        d.width, d.height, d.iterations, d.normal_power_log2, d.min_history = 8, 8, 2, 7, 4
        d.sigma_luminance, d.sigma_plane, d.variance_floor, d.gamma = 4.0, SIGMA_PLANE, 1e-10, 1.0
        d.color, d.variance, d.length, d.rgba32f_out = ptr, ptr, ptr, ptr
        for k, v in fields.items():
            setattr(d, k, v)
        o = abi.RaycaRenderOptions()
        for name, v in (o_fields or {}).items():
            target, _, leaf = name.rpartition(".")
            setattr(getattr(o, target) if target else o, leaf, v)
        return product_lib.rayca_hip_denoise_variance_device(scene, C.byref(o), C.byref(d), None)

    run.ptr, run.keep = ptr, dummy
    return run


def test_bad_arguments_are_refused_in_front_of_any_gpu_work(call):
    ptr = call.ptr
    cases = [(dict(color=None), "color"), (dict(variance=None), "variance"), (dict(rgba32f_out=None, rgba8_out=None), "output"),
             (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(length=None), "length"),
             (dict(point=ptr), "normal"), (dict(point=ptr, normal=ptr, sigma_plane=0.0), "sigma_plane"),
             (dict(normal_power_log2=11), "normal_power_log2"), (dict(width=0), "width"), (dict(height=0), "height"),
             (dict(width=65536, height=65536), "pixels"), (dict(reserved=1), "reserved"),
             (dict(color=ptr + 4), "alignment"), (dict(rgba32f_out=ptr + 8), "alignment"), (dict(variance=ptr + 2), "alignment"),
             (dict(variance_out=ptr + 1), "alignment"), (dict(length=ptr + 2), "alignment")]
    for field in ("sigma_luminance", "variance_floor", "gamma"):
        cases += [(dict({field: bad}), field) for bad in (0.0, -1.0, float("nan"))]
    for fields, word in cases:
        assert call(**fields) == abi.ERR_BAD_ARG, fields
        assert word in last_error(), (fields, last_error())
    assert call(length=None, min_history=0, o_fields=dict(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()   # (no length without a fallback is fine)


def test_a_field_the_pass_does_not_take_must_be_zero(call):
    assert call(dict(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(dict(context=0xFFFFFFFF)) == abi.ERR_BAD_ARG and "context" in last_error()
    refused = ("traversal", "collect_stats", "tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved")
    for field in refused:
        for value in (1, 0xFFFFFFFF):
            assert call({field: value}) == abi.ERR_BAD_ARG, (field, value)
            assert "must be zero" in last_error() and field.partition(".")[0] in last_error(), (field, value, last_error())
    # the fields every pass takes do not shield one that it does not
    assert call(dict(context=7, stream=1, wait_event=1, record_event=1, engine=1)) == abi.ERR_BAD_ARG and "must be zero" in last_error()


def test_null_arguments_and_oversize_frames(product_lib, call):
    o = abi.RaycaRenderOptions()
    d = abi.RaycaDenoiseVariance()
    assert product_lib.rayca_hip_denoise_variance_device(None, C.byref(o), C.byref(d), None) == abi.ERR_BAD_ARG
    assert product_lib.rayca_hip_denoise_variance_device(C.cast(call.keep, C.c_void_p), C.byref(o), None, None) == abi.ERR_BAD_ARG
    # 2^24 tiles of 64 x 4 pixels: one launch cannot cover the frame
    assert call(width=1, height=1 << 26) == abi.ERR_UNSUPPORTED and "tiles" in last_error()
