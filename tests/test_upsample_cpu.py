"""Guided upsampling without a GPU: what its specification promises, checked on the literal restatement
(tests/upsample_literal.py), and what rayca_hip_upsample_device refuses, checked through the C ABI in front of any GPU work (any
non-NULL value will do for the scene handle, as in tests/test_denoise_variance_cpu.py)."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import upsample_literal as ul
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIGMA_PLANE = 0.1
PAIRS = [(48, 30, 2), (31, 19, 3)]   # (low width, low height, scale): an even scale, and an odd one (a pixel centre on a low centre)
_PAIRS = {}


def pair(low_width, low_height, scale):
    """a size's low and full-size view, made once and shared read-only"""
    key = (low_width, low_height, scale)
    if key not in _PAIRS:
        low, high, k = ul.synthetic_pair(low_width, low_height, scale)
        for d in (low, high):
            for a in d.values():
                a.setflags(write=False)
        _PAIRS[key] = (low, high, k)
    return _PAIRS[key]


def guided(low, high, scale, which=ul.GUIDES, **kw):
    return ul.upsample(low["color"], scale, low=ul.guides_of(low, which), high=ul.guides_of(high, which), sigma_plane=SIGMA_PLANE, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rmse(a, b, mask):
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2
    return float(np.sqrt(d[mask].mean()))


# ---- a-f: properties of the specification ---------------------------------------------------------------------------------------
def test_scale_one_without_albedo_is_the_identity():
    """(a) one tap with b = 1: 0 + 1 * c is c for every finite c but -0.0 (which the sum from +0 returns as +0.0: the frame here
    has none), and the weight is 1; with the id guide too -- both views are the same view.  (A normal guide weighs the tap
    with (n . n)^128, which is 1 only for a normal whose float32 length is exactly 1.)"""
    low, _, _ = ul.synthetic_pair(37, 23, 1, specials=False)
    for which in ((), ("id",)):
        out, out8, weight = guided(low, low, 1, which)
        assert np.array_equal(bits(out), bits(low["color"])), which
        assert np.array_equal(weight, np.ones_like(weight)), which
        assert np.array_equal(out8, ul.quantize(low["color"]))


@pytest.mark.parametrize("scale", [1, 2, 3, 4, 5, 8])
def test_without_guides_it_is_plain_bilinear(scale):
    """(b) bit for bit against the independent resampler, whose association is the literal's (see its docstring): NaN and inf
    pixels included, which both leave out of the footprint"""
    low, _, _ = ul.synthetic_pair(31, 19, scale)
    out, _, weight = ul.upsample(low["color"], scale)
    want = ul.bilinear(low["color"], scale)
    assert np.array_equal(bits(out), bits(want))
    assert (weight[np.isfinite(out).all(-1)] > 0).all()


@pytest.mark.parametrize("low_width,low_height,scale", PAIRS)
def test_a_demodulated_colour_of_one_returns_the_albedo(low_width, low_height, scale):
    """(c) color = albedo_low: every tap is exactly 1 (x / x), a weighted mean of ones is sum / wsum with sum == wsum, and
    1 * albedo is the albedo -- the texture comes from the full-size surface data alone, bit for bit"""
    low, high, _ = pair(low_width, low_height, scale)
    out, _, weight = ul.upsample(low["albedo"], scale, low=ul.guides_of(low), high=ul.guides_of(high), sigma_plane=SIGMA_PLANE)
    ok = (weight > 0)[..., None] & (high["albedo"][..., :3] >= F(1e-3))
    assert ok.mean() > 0.9
    assert np.array_equal(bits(out[..., :3])[ok], bits(high["albedo"][..., :3])[ok])
    assert np.array_equal(out[..., 3][weight > 0], np.ones_like(weight)[weight > 0])


@pytest.mark.parametrize("low_width,low_height,scale", PAIRS)
def test_the_guided_result_is_nearer_the_full_size_frame_than_plain_bilinear(low_width, low_height, scale):
    """(d) over the whole image and over the band within `scale` pixels of the plane edge"""
    low, high, k = pair(low_width, low_height, scale)
    out, _, _ = guided(low, high, scale)
    plain = ul.bilinear(low["color"], scale)
    y, x = np.mgrid[0:low_height * scale, 0:low_width * scale]
    band = np.abs((x + 0.5) - ul.edge_x(k, y + 0.5)) <= scale
    finite = np.isfinite(out).all(-1) & np.isfinite(plain).all(-1)
    for name, mask in (("whole image", finite), ("edge band", finite & band)):
        e_guided, e_plain = rmse(out, high["clean"], mask), rmse(plain, high["clean"], mask)
        print(f"{low_width} x {low_height} x {scale}, {name}: RMSE guided {e_guided:.5f}, plain bilinear {e_plain:.5f}")
        assert e_guided < e_plain
    # ... and on the edge band, where plain bilinear mixes the two planes' irradiance, by more than a factor of ten
    assert rmse(out, high["clean"], finite & band) * 10 < rmse(plain, high["clean"], finite & band)


@pytest.mark.parametrize("low_width,low_height,scale", PAIRS)
def test_a_miss_next_to_the_object_takes_only_miss_taps(low_width, low_height, scale):
    """(e) the sky is one colour and every hit differs from it: a miss pixel with a hit tap in its footprint still has the sky's bits"""
    low, high, k = pair(low_width, low_height, scale)
    out, _, weight = guided(low, high, scale, ("normal",))
    miss = (high["normal"] == 0).all(-1)
    boundary = miss & np.roll(~miss, -scale, axis=0)   # within `scale` rows above the first row of hits: a footprint that crosses
    assert boundary.any() and (weight[boundary] > 0).all()
    sky = np.array(ul.SKY, F)
    # (a weighted mean of equal values: sum / wsum with sum = wsum * v rounded per term; equal to v to a rounding or two)
    assert np.abs(out[boundary] - sky).max() <= 2 * np.spacing(F(1.0))
    plain = ul.bilinear(low["color"], scale)
    assert np.abs(plain[boundary] - sky).max() > 0.01   # (what the guide prevents)


@pytest.mark.parametrize("low_width,low_height,scale", PAIRS)
def test_the_fallback_covers_the_thin_feature_and_nothing_else(low_width, low_height, scale):
    """(f) no low pixel centre lies on the thin feature, so none of its pixels has an agreeing tap: weight 0, plain bilinear
    colour.  Everywhere else a tap agrees, except where the one tap of a pixel is not finite: at an odd scale the pixel in
    the middle of a low pixel has that low pixel as its only tap (tx = ty = 0), and the NaN passes through."""
    low, high, _ = pair(low_width, low_height, scale)
    assert high["thin"].sum() >= 10 and not low["thin"].any()
    for which in (ul.GUIDES, ("normal",), ("id",), ("normal", "point")):
        out, _, weight = guided(low, high, scale, which)
        fallback = weight == 0
        want = high["thin"].copy()
        if scale % 2:
            for py, px in ul.NAN_PIXELS:
                want[(py % low_height) * scale + scale // 2, (px % low_width) * scale + scale // 2] = True
        assert np.array_equal(fallback, want), (which, np.argwhere(fallback != want).tolist())
        assert np.isfinite(out[high["thin"]]).all()
        assert np.isfinite(out).all(-1).sum() == out.shape[0] * out.shape[1] - (len(ul.NAN_PIXELS) if scale % 2 else 0)
    # the fallback's colour is the unguided pass's
    plain, _, _ = ul.upsample(low["color"], scale)
    out, _, _ = guided(low, high, scale, ("normal", "point", "id"))
    assert np.array_equal(bits(out[high["thin"]]), bits(plain[high["thin"]]))


# ---- g: refusals through the C ABI -----------------------------------------------------------------------------------------------
PAIR_FIELDS = ("albedo", "normal", "point", "id")


@pytest.fixture(scope="module")
def call(product_lib):
    """call(options fields, **changes of the arguments): the arguments pass every check unless changed.  ptr stands for device
    pointers (nothing is launched): ptr(i) are distinct 16-byte aligned addresses."""
    dummy = C.create_string_buffer(1024)
    scene, base = C.cast(dummy, C.c_void_p), (C.addressof(dummy) + 15) // 16 * 16

    def ptr(i):
        return base + 16 * i

    def run(o_fields=None, **fields):
        u = abi.RaycaUpsample()
        u.width, u.height, u.scale, u.normal_power_log2 = 16, 8, 2, 7
        u.sigma_plane, u.gamma = SIGMA_PLANE, 1.0
        u.color, u.rgba32f_out = ptr(0), ptr(1)
        for k, v in fields.items():
            setattr(u, k, v)
        o = abi.RaycaRenderOptions()
        for name, v in (o_fields or {}).items():
            target, _, leaf = name.rpartition(".")
            setattr(getattr(o, target) if target else o, leaf, v)
        return product_lib.rayca_hip_upsample_device(scene, C.byref(o), C.byref(u), None)

    run.ptr, run.keep = ptr, dummy
    return run


def all_guides(ptr):
    return {name: ptr(4 + n) for n, name in enumerate(f + s for f in PAIR_FIELDS for s in ("", "_low"))}


def test_bad_arguments_are_refused_in_front_of_any_gpu_work(call):
    ptr = call.ptr
    g = all_guides(ptr)
    cases = [(dict(color=None), "color"), (dict(scale=0), "scale"), (dict(scale=9), "scale"), (dict(scale=3), "divisible"),
             (dict(width=17), "divisible"), (dict(height=7), "divisible"), (dict(width=0), "width"), (dict(height=0), "height"),
             (dict(width=65536, height=65536), "pixels"), (dict(g, point=None, point_low=None, normal_low=None), "normal_low"),
             (dict(point=ptr(2), point_low=ptr(3)), "point needs normal"), (dict(g, sigma_plane=0.0), "sigma_plane"),
             (dict(g, sigma_plane=-1.0), "sigma_plane"), (dict(g, sigma_plane=float("nan")), "sigma_plane"),
             (dict(normal_power_log2=11), "normal_power_log2"), (dict(rgba32f_out=None), "output"), (dict(reserved=1), "reserved"),
             (dict(color=ptr(0) + 4), "alignment"), (dict(rgba32f_out=ptr(1) + 8), "alignment"), (dict(weight_out=ptr(2) + 2), "alignment"),
             (dict(rgba8_out=ptr(2) + 1), "alignment"), (dict(g, albedo=g["albedo"] + 4), "alignment"), (dict(g, id_low=g["id_low"] + 2), "alignment"),
             (dict(rgba32f_out=ptr(0)), "aliasing"), (dict(g, rgba8_out=g["id"]), "aliasing"), (dict(g, weight_out=g["normal_low"]), "aliasing"),
             (dict(scale=1, rgba32f_out=ptr(0)), "aliasing")]
    for name in PAIR_FIELDS:   # half a guide pair, either half
        for half in (name, name + "_low"):
            cases.append(({k: v for k, v in g.items() if k != half}, name + " and " + name + "_low"))
    cases += [(dict(gamma=bad), "gamma") for bad in (0.0, -1.0, float("nan"))]
    for fields, word in cases:
        assert call(**fields) == abi.ERR_BAD_ARG, fields
        assert word in last_error(), (fields, last_error())
    # 2^24 tiles of 64 x 4 pixels: one launch cannot cover the frame
    assert call(width=2, height=1 << 26) == abi.ERR_UNSUPPORTED and "tiles" in last_error()


def test_null_arguments(product_lib, call):
    o, u = abi.RaycaRenderOptions(), abi.RaycaUpsample()
    assert product_lib.rayca_hip_upsample_device(None, C.byref(o), C.byref(u), None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert product_lib.rayca_hip_upsample_device(C.cast(call.keep, C.c_void_p), C.byref(o), None, None) == abi.ERR_BAD_ARG and "null" in last_error()


def test_nothing_else_is_refused(call):
    """The options are the last thing the call checks before it touches the scene handle (which is a dummy here, and on a machine
    with a device would be launched on): a struct that is refused for context 8 -- and for nothing else -- has passed every check
    of its own.  Every legal subset of the guide pairs, every scale, both outputs, the weight, the parameter ranges' ends."""
    ptr = call.ptr
    g = all_guides(ptr)
    last = dict(context=8)
    valid = []
    for albedo, normal, point, ident in itertools.product((False, True), repeat=4):
        if point and not normal:
            continue
        which = [n for n, on in zip(PAIR_FIELDS, (albedo, normal, point, ident)) if on]
        valid.append({k: v for k, v in g.items() if k.replace("_low", "") in which})
    valid += [dict(scale=s, width=8 * s, height=3 * s) for s in range(1, 9)]
    valid += [dict(rgba32f_out=None, rgba8_out=ptr(2)), dict(rgba8_out=ptr(2) + 4, weight_out=ptr(3) + 4), dict(g, normal_power_log2=0),
              dict(g, normal_power_log2=10), dict(gamma=2.2), dict(sigma_plane=0.0), dict(g, point=None, point_low=None, sigma_plane=-1.0),
              dict(width=1, height=1, scale=1), dict(width=1 << 16, height=(1 << 12) - 1, scale=1), dict(g, normal=g["normal"] + 4, id=g["id"] + 4)]
    for fields in valid:
        assert call(last, **fields) == abi.ERR_BAD_ARG and "context out of range" in last_error(), (fields, last_error())
    # ... while the options that every pass takes are taken, and the ones it does not take are refused
    assert call(dict(context=8, stream=1, wait_event=1, record_event=1)) == abi.ERR_BAD_ARG and "context out of range" in last_error()
    for field in ("traversal", "collect_stats", "tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call({field: 1}) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error(), (field, last_error())


# ---- h: the struct's layout ----------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaUpsample %zu\\n", sizeof(RaycaUpsample));']
    for name, _ in abi.RaycaUpsample._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(RaycaUpsample, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaUpsample) == int(want["RaycaUpsample"]) == 128
    for name, _ in abi.RaycaUpsample._fields_:
        assert getattr(abi.RaycaUpsample, name).offset == int(want[name]), name
    assert len(want) == len(abi.RaycaUpsample._fields_) + 1
