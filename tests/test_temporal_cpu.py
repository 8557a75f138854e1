"""rayca_hip_scene_camera and rayca_hip_accumulate_device without a GPU: the symbols, the layouts of RaycaCameraPose and
RaycaAccumulate against the header, the argument errors that need no scene, the pass-options rule, and the properties of the
accumulation as specified, on the literal restatement (tests/temporal_literal.py) that the GPU tests compare the kernel with bit
for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import temporal_literal as tl
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
POSE_FIELDS = ["origin", "angle", "right", "reserved0", "up", "reserved1", "back", "reserved2"]
FIELDS = ["width", "height", "max_history", "reserved", "normal_min", "plane_max", "prev_camera", "color", "point", "normal", "id",
          "hist_color", "hist_length", "hist_moments", "prev_normal", "prev_point", "prev_id", "color_out", "length_out", "moments_out",
          "variance_out"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_entries(product_lib):
    for name in ("rayca_hip_scene_camera", "rayca_hip_accumulate_device"):
        assert name in abi.PRODUCT_SYMBOLS
        assert getattr(product_lib, name) is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # (no layout changed: the version stays)


def test_struct_layouts_match_header():
    """The rule of test_abi.py: a C program prints sizeof / offsetof from the header, ctypes must agree."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){"]
    for s, fields in (("RaycaCameraPose", POSE_FIELDS), ("RaycaAccumulate", FIELDS)):
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for name in fields:
            lines.append(f'printf("{s}.{name} %zu\\n", offsetof({s}, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    for s, fields, size in (("RaycaCameraPose", POSE_FIELDS, 64), ("RaycaAccumulate", FIELDS, 6 * 4 + 15 * 8)):
        cls = getattr(abi, s)
        assert [n for n, _ in cls._fields_] == fields
        assert C.sizeof(cls) == int(want[s]) == size
        for name in fields:
            assert getattr(cls, name).offset == int(want[f"{s}.{name}"]), f"{s}.{name}"


def opts(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields) with a dummy scene handle and dummy `device` pointers: every check these tests reach is
    decided before the handle is looked at, and nothing is launched"""
    dummy = C.create_string_buffer(4096)
    base = (C.addressof(dummy) + 63) & ~63
    scene = C.cast(dummy, C.c_void_p)
    pose = abi.RaycaCameraPose()

    def ptr(i):
        return base + 64 * i   # (distinct, 16-byte aligned)

    def run(o=None, null_scene=False, null_args=False, **kw):
        a = abi.RaycaAccumulate()
        a.width, a.height, a.normal_min, a.plane_max = 8, 8, 0.9, 0.1
        a.color, a.color_out, a.length_out = ptr(0), ptr(1), ptr(2)
        for k, v in kw.items():
            setattr(a, k, v)
        return product_lib.rayca_hip_accumulate_device(None if null_scene else scene, C.byref(o) if o is not None else None,
                                                       None if null_args else C.byref(a), None)

    run.ptr, run.pose, run._keep = ptr, C.pointer(pose), (dummy, pose)
    return run


def test_argument_errors_that_need_no_scene(product_lib, call):
    ptr, pose = call.ptr, call.pose

    def bad(word, **kw):
        rc = call(**kw)
        assert rc == abi.ERR_BAD_ARG and word in last_error(), (kw, rc, last_error())

    reproject = dict(prev_camera=pose, point=ptr(3), normal=ptr(4))
    history = dict(hist_color=ptr(5), hist_length=ptr(6))
    bad("null", null_scene=True)
    bad("null", null_args=True)
    bad("empty image", width=0)
    bad("empty image", height=0)
    bad("2^32", width=65536, height=65536)
    bad("reserved", reserved=1)
    bad("color", color=None)
    bad("color_out", color_out=None)
    bad("length_out", length_out=None)
    # required with the previous camera, forbidden without it
    bad("point and normal are required", prev_camera=pose)
    bad("point and normal are required", prev_camera=pose, point=ptr(3))
    bad("point and normal are required", prev_camera=pose, normal=ptr(4))
    bad("must be NULL without prev_camera", point=ptr(3))
    bad("must be NULL without prev_camera", normal=ptr(4))
    bad("id and prev_id", **reproject, id=ptr(7))
    bad("id and prev_id", **reproject, prev_id=ptr(7))
    # the history: colour and length together, moments only with them
    bad("hist_color and hist_length", hist_color=ptr(5))
    bad("hist_color and hist_length", hist_length=ptr(6))
    bad("hist_moments", hist_moments=ptr(7))
    bad("prev_normal", **reproject, **history)
    bad("moments_out needs hist_moments", **history, moments_out=ptr(8))
    bad("variance_out needs moments_out", variance_out=ptr(9))
    for v in (0.0, -0.5, float("nan")):
        bad("normal_min", **reproject, normal_min=v)
        bad("plane_max", **reproject, **history, prev_normal=ptr(8), prev_point=ptr(9), plane_max=v)
    # alignment: 16 bytes for the float4 images, 4 for the rest
    for name in ("color", "hist_color", "color_out"):
        kw = dict(history)
        kw[name] = ptr(10) + 4
        bad("alignment", **kw)
    for name in ("hist_length", "length_out", "moments_out", "variance_out", "hist_moments"):
        kw = dict(history, hist_moments=ptr(7), moments_out=ptr(8), variance_out=ptr(9))
        kw[name] = ptr(10) + 2
        bad("alignment", **kw)
    for name in ("point", "normal", "id", "prev_id", "prev_normal", "prev_point"):
        kw = dict(reproject, **history, prev_normal=ptr(8), prev_point=ptr(9), id=ptr(11), prev_id=ptr(12))
        kw[name] = ptr(10) + 1
        bad("alignment", **kw)
    # aliasing: in reprojection mode no output may be an image the taps read
    full = dict(reproject, **history, hist_moments=ptr(7), prev_normal=ptr(8), prev_point=ptr(9), id=ptr(11), prev_id=ptr(12), moments_out=ptr(13),
                variance_out=ptr(14))
    for out in ("color_out", "length_out", "moments_out", "variance_out"):
        for src in ("hist_color", "hist_length", "hist_moments", "prev_normal", "prev_point", "prev_id"):
            kw = dict(full)
            kw[out] = full[src]
            bad("aliasing", **kw)
    # ... and the options
    bad("context", o=opts(context=8))
    for name in ("traversal", "collect_stats", "engine", "camera_rays", "reserved"):
        bad("must be zero", o=opts(**{name: 1}))
    bad("tile", o=opts(**{"tile.parts": 2}))
    # 2^24 tiles or more: one launch cannot cover the frame (behind every argument check, in front of the scene)
    assert call(width=1, height=(1 << 26)) == abi.ERR_UNSUPPORTED and "tiles" in last_error()
    # the camera entry's own
    assert product_lib.rayca_hip_scene_camera(None, call.pose) == abi.ERR_BAD_ARG and "null" in last_error()
    assert product_lib.rayca_hip_scene_camera(C.cast(call._keep[0], C.c_void_p), None) == abi.ERR_BAD_ARG and "null" in last_error()


GROUPS = {"traversal": ("traversal",), "collect_stats": ("collect_stats",),
          "tile": ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved"),
          "engine": ("engine",), "camera_rays": ("camera_rays",), "reserved": ("reserved",)}


def test_a_field_the_pass_does_not_take_must_be_zero(call):
    """the rule of test_pass_options_cpu.py for the new entry, which takes stream, context and the two events only"""
    refused = [f for fields in GROUPS.values() for f in fields]
    assert len(refused) == 9
    for field in refused:
        for value in (1, 0xFFFFFFFF):
            assert call(o=opts(**{field: value})) == abi.ERR_BAD_ARG, (field, value)
            assert "must be zero" in last_error() and field.partition(".")[0] in last_error(), (field, value, last_error())
    assert call(o=opts(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(o=opts(context=0xFFFFFFFF)) == abi.ERR_BAD_ARG and "context" in last_error()
    # the fields every pass takes do not shield one that it does not
    assert call(o=opts(context=7, stream=1, wait_event=1, record_event=1, engine=1)) == abi.ERR_BAD_ARG and "must be zero" in last_error()


# ---- the accumulation as specified: properties of the literal ----------------------------------------------------------------
W, H, SEED = 64, 48, 4100
POSE_A = tl.make_pose((0.2, 0.1, 2.0))
POSE_B = tl.make_pose((0.9, 0.1, 2.0))   # a sideways shift


@pytest.fixture(scope="module")
def frames():
    """16 frames of one view: clean x noise, each with its own seed"""
    views = [tl.synthetic_view(POSE_A, W, H, SEED + k) for k in range(16)]
    for v in views:
        for a in v.values():
            a.setflags(write=False)
    return views


def film(colors, **kw):
    hist = None
    for c in colors:
        r = tl.accumulate(c, history=hist, **kw)
        hist = tl.as_history(r)
    return r


def test_running_mean_is_the_mean(frames):
    """max_history 0: three roundings per step (c - h, x a, + h) and the errors do not grow, e_n <= e_{n-1} (1 - 1/n) + 3 ulp"""
    n = len(frames)
    colors = [v["color"] for v in frames]
    r = film(colors)
    assert np.array_equal(r["length"], np.full((H, W), n, F))
    mean = np.mean(np.stack(colors).astype(np.float64), axis=0)
    bound = 3 * n * 2.0 ** -24 * max(float(np.abs(c).max()) for c in colors)
    err = float(np.abs(r["color"].astype(np.float64) - mean).max())
    print(f"max |film - mean| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    lum = np.stack([tl.luminance(c) for c in colors]).astype(np.float64)
    assert np.allclose(r["moments"][..., 0], lum.mean(0), atol=1e-4) and np.allclose(r["moments"][..., 1], (lum * lum).mean(0), atol=1e-3)
    assert np.allclose(r["variance"], lum.var(0), atol=1e-3) and (r["variance"] >= 0).all()


def test_max_history_caps_the_length(frames):
    hist, longest = None, 0.0
    for k, v in enumerate(frames[:9]):
        r = tl.accumulate(v["color"], history=hist, max_history=4)
        hist = tl.as_history(r)
        assert np.array_equal(r["length"], np.full((H, W), min(k + 1, 4), F))
        longest = max(longest, float(r["length"].max()))
    assert longest == 4.0
    # the tail is exponential: the newest frame has weight 1/4
    want = hist["color"]
    prev = film([v["color"] for v in frames[:8]], max_history=4)["color"]
    assert np.array_equal(bits(want), bits(prev + (frames[8]["color"] - prev) * F(0.25)))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_sample_that_is_not_finite_stays_out_of_the_film(frames, value):
    colors = [v["color"].copy() for v in frames[:6]]
    k, (y, x) = 3, (20, 31)
    colors[k][y, x, 1] = value
    r = film(colors)
    assert np.isfinite(r["color"]).all() and np.isfinite(r["moments"]).all()
    assert r["length"][y, x] == 5.0 and r["length"][y, x + 1] == 6.0 and r["length"][y + 1, x] == 6.0
    others = film(colors[:k] + colors[k + 1:])
    assert np.array_equal(bits(r["color"][y, x]), bits(others["color"][y, x]))   # the pixel is the film of the other five frames
    # as the very first sample it leaves length 0, the validity channel: the next frame starts the pixel over
    first = tl.accumulate(colors[k])
    assert first["length"][y, x] == 0.0 and not np.isfinite(first["color"][y, x]).all() and first["moments"][y, x].tolist() == [0.0, 0.0]
    second = tl.accumulate(colors[0], history=tl.as_history(first))
    assert second["length"][y, x] == 1.0 and np.array_equal(bits(second["color"][y, x]), bits(colors[0][y, x]))


def reproject(now, then, hist, pose_then, which=("normal", "point", "id"), **kw):
    ident = now["id"] if "id" in which else None
    return tl.accumulate(now["color"], history=hist, prev=tl.as_prev(then, which), prev_camera=pose_then, point=now["point"],
                         normal=now["normal"], id=ident, **kw)


def test_reprojection_onto_the_same_pose_keeps_every_hit(frames):
    """the pixel itself is one of the four taps and passes every check against its own record"""
    a, b = frames[0], frames[1]
    r = reproject(b, a, tl.first_history(a), POSE_A)
    hit = a["id"] != 0
    assert 0.5 < hit.mean() < 0.95
    assert (r["length"][hit] > 1.5).all()
    assert (r["length"][~hit] == 1.0).all()
    assert np.array_equal(bits(r["color"][~hit]), bits(b["color"][~hit]))


def dilate(mask, n=1):
    out = mask.copy()
    h, w = mask.shape
    for dy in range(-n, n + 1):
        for dx in range(-n, n + 1):
            out[max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)] |= mask[max(0, -dy):h + min(0, -dy), max(0, -dx):w + min(0, -dx)]
    return out


def test_a_sideways_shift_disoccludes_a_strip_of_the_far_plane():
    w, h = 130, 70
    a, b = tl.synthetic_view(POSE_A, w, h, 1), tl.synthetic_view(POSE_B, w, h, 2)
    hist = tl.first_history(a)
    r = reproject(b, a, hist, POSE_A)
    hit = b["id"] != 0
    fresh = hit & (r["length"] == 1.0)
    assert fresh.sum() > 20
    assert (b["id"][fresh] == tl.ID_FAR).all()
    # what the two poses predict: a far-plane point that the near plane hid from A, or that A's image did not hold
    fx, fy, front = tl.project(POSE_A, b["point"], w, h)
    hidden = tl.hidden_by_near(POSE_A["origin"], b["point"].astype(np.float64))
    outside = ~front | (fx <= -1) | (fx >= w) | (fy <= -1) | (fy >= h)
    predicted = (b["id"] == tl.ID_FAR) & (hidden | outside)
    assert predicted.sum() > 20 and (predicted & hidden).sum() > 20
    assert not (fresh & ~dilate(predicted, 1)).any(), np.argwhere(fresh & ~dilate(predicted, 1))[:4]
    # ... and the strip is covered: a predicted pixel two or more pixels inside it has no tap that A saw on the far plane
    inner = predicted & ~dilate(~predicted, 2)
    assert inner.sum() > 5 and not (inner & ~fresh).any()
    # no tap crosses an id: other colours on A's near plane leave the far plane's bits alone
    rng = np.random.default_rng(9)
    hist2 = {k: v.copy() for k, v in hist.items()}
    near_a = a["id"] == tl.ID_NEAR
    hist2["color"][near_a] = rng.uniform(0.0, 50.0, size=hist2["color"][near_a].shape).astype(F)
    hist2["moments"][near_a] = rng.uniform(0.0, 50.0, size=hist2["moments"][near_a].shape).astype(F)
    r2 = reproject(b, a, hist2, POSE_A)
    far_b, near_b = b["id"] == tl.ID_FAR, b["id"] == tl.ID_NEAR
    for k in r:
        assert np.array_equal(bits(r[k][far_b]), bits(r2[k][far_b])), k
    assert not np.array_equal(bits(r["color"][near_b]), bits(r2["color"][near_b]))
    # without ids and points the normals alone cannot tell the planes apart (they are parallel): the far plane changes
    r3, r4 = reproject(b, a, hist, POSE_A, which=("normal",)), reproject(b, a, hist2, POSE_A, which=("normal",))
    assert not np.array_equal(bits(r3["color"][far_b]), bits(r4["color"][far_b]))


@pytest.mark.parametrize("width,height", [(130, 70), (61, 37)])
def test_pose_convention(width, height):
    """Pixel-centre points project back to their own pixel.  Rounding is of the order 1e-4 pixel at these sizes; an error of
    convention (half-pixel offset, flipped y, aspect on the wrong axis) is 0.5 pixel or more."""
    for pose in (POSE_A, tl.make_pose((-0.4, 0.3, 1.0), yaw=0.12, pitch=-0.07, yfov=0.7), tl.make_pose((0.0, 0.0, 3.0), yaw=-0.05, scale=(1.5, 0.8, 2.0))):
        v = tl.synthetic_view(pose, width, height, 5)
        hit = v["id"] != 0
        assert hit.sum() > width * height // 3
        fx, fy, front = tl.project(pose, v["point"], width, height)
        y, x = np.mgrid[0:height, 0:width]
        assert front[hit].all()
        ex, ey = float(np.abs(fx - x)[hit].max()), float(np.abs(fy - y)[hit].max())
        print(f"{width} x {height}: max |fx - x| {ex:.2g}, max |fy - y| {ey:.2g}")
        assert ex <= 1 / 64 and ey <= 1 / 64


def test_specials_are_where_the_gpu_tests_expect_them():
    w, h = 61, 37
    a = tl.synthetic_view(POSE_A, w, h, 1)
    b = tl.synthetic_view(POSE_B, w, h, 2, specials=POSE_A)
    assert np.isnan(b["color"][2, 3, 0]) and np.isinf(b["color"][5, 17, 1])
    fx, fy, front = tl.project(POSE_A, b["point"], w, h)
    assert not front[3, 6]
    assert fx[8, 1] >= w and fy[1, 9] < -1
    assert -1 <= fx[10, 4] < 0 and 0 <= fy[10, 4] < h - 1
    assert -1 <= fy[12, 7] < 0 and 0 <= fx[12, 7] < w - 1
    assert -1 <= fx[13, 11] < 0 and -1 <= fy[13, 11] < 0
    hist = tl.first_history(a, specials=True)
    assert hist["length"][6, 5] == 0.0
    r = reproject(b, a, hist, POSE_A)
    for at in ((3, 6), (8, 1), (1, 9)):
        assert r["length"][at] == 1.0, at
    for at in ((10, 4), (12, 7), (13, 11)):   # one column, one row, one tap inside: still a history (A saw the far plane there)
        assert r["length"][at] == 2.0, at
    assert r["length"][2, 3] in (0.0, 1.0) and np.isfinite(r["color"]).sum() >= r["color"].size - 2
