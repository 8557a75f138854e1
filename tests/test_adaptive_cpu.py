"""rayca_hip_sample_plan_device and rayca_hip_film_fold_device without a GPU: the symbols, the layouts of RaycaSamplePlan and
RaycaFilmFold against the header, every refusal the structs alone decide, in the documented order, and the properties of the plan
and the fold as specified, on the literal restatement (tests/adaptive_literal.py) that the GPU tests compare the kernels with bit
for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_literal as al
import temporal_literal as tl
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PLAN_FIELDS = ["width", "height", "budget", "jitter", "first_stratum", "base_weight", "fresh_weight", "min_history", "target", "lum_floor",
               "reserved", "color", "variance", "length", "weight_out", "offset_out", "rays_out", "pixel_out"]
FOLD_FIELDS = ["width", "height", "max_history", "reserved", "samples", "offset", "hist_color", "hist_length", "hist_moments", "color_out",
               "length_out", "moments_out", "variance_out"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_entries(product_lib):
    for name in ("rayca_hip_sample_plan_device", "rayca_hip_film_fold_device"):
        assert name in abi.PRODUCT_SYMBOLS
        assert getattr(product_lib, name) is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # (no layout changed: the version stays)


def test_struct_layouts_match_header():
    """The rule of test_abi.py: a C program prints sizeof / offsetof from the header, ctypes must agree."""
    structs = (("RaycaSamplePlan", PLAN_FIELDS, 12 * 4 + 7 * 8), ("RaycaFilmFold", FOLD_FIELDS, 4 * 4 + 9 * 8))
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){"]
    for s, fields, _ in structs:
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
    for s, fields, size in structs:
        cls = getattr(abi, s)
        assert [n for n, _ in cls._fields_] == fields
        assert C.sizeof(cls) == int(want[s]) == size   # (RaycaSamplePlan: eleven words and four bytes of padding in front of the pointers)
        for name in fields:
            assert getattr(cls, name).offset == int(want[f"{s}.{name}"]), f"{s}.{name}"


def opts(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


@pytest.fixture(scope="module")
def calls(product_lib):
    """plan(options | None, **fields) and fold(...) with a dummy scene handle and dummy `device` pointers: every check these tests
    reach is decided before the handle is looked at, and nothing is launched"""
    dummy = C.create_string_buffer(4096)
    base = (C.addressof(dummy) + 63) & ~63
    scene = C.cast(dummy, C.c_void_p)

    def ptr(i):
        return base + 64 * i   # (distinct, 16-byte aligned)

    def run(fn, a, o, null_scene, null_args, kw):
        for k, v in kw.items():
            setattr(a, k, v)
        return fn(None if null_scene else scene, C.byref(o) if o is not None else None, None if null_args else C.byref(a), None)

    def plan(o=None, null_scene=False, null_args=False, **kw):
        a = abi.RaycaSamplePlan()
        a.width, a.height, a.budget, a.jitter, a.target, a.lum_floor = 8, 8, 64, 1, 0.05, 1e-3
        a.color, a.variance, a.length, a.offset_out = ptr(0), ptr(1), ptr(2), ptr(3)
        return run(product_lib.rayca_hip_sample_plan_device, a, o, null_scene, null_args, kw)

    def fold(o=None, null_scene=False, null_args=False, **kw):
        a = abi.RaycaFilmFold()
        a.width, a.height = 8, 8
        a.samples, a.offset, a.hist_color, a.hist_length, a.color_out, a.length_out = (ptr(i) for i in range(6))
        return run(product_lib.rayca_hip_film_fold_device, a, o, null_scene, null_args, kw)

    plan.ptr = fold.ptr = ptr
    plan._keep = dummy
    return plan, fold


def refusals(call):
    def bad(word, code=abi.ERR_BAD_ARG, **kw):
        rc = call(**kw)
        assert rc == code and word in last_error(), (kw, rc, last_error())
    return bad


def common_option_refusals(bad):
    bad("context", o=opts(context=8))
    for name in ("traversal", "collect_stats", "engine", "camera_rays", "reserved"):
        bad("must be zero", o=opts(**{name: 1}))
        bad(name, o=opts(**{name: 1}))
    bad("tile", o=opts(**{"tile.parts": 2}))


def test_plan_refusals_that_need_no_scene(calls):
    plan, _ = calls
    ptr, bad = plan.ptr, refusals(plan)
    bad("null", null_scene=True)
    bad("null", null_args=True)
    bad("reserved", reserved=1)
    bad("empty image", width=0)
    bad("empty image", height=0)
    bad("2^32", width=65536, height=65536)
    # width x height x 256 > 2^32: the sum of the weights would not fit 32 bits
    bad("256", code=abi.ERR_UNSUPPORTED, width=4097, height=4096)
    assert plan(width=4096, height=4096, budget=(1 << 31) + 1) == abi.ERR_BAD_ARG   # (2^24 pixels pass; the next check speaks)
    bad("budget", budget=(1 << 31) + 1)
    bad("jitter", jitter=0)
    bad("jitter", jitter=9)
    bad("base_weight", base_weight=256)
    bad("fresh_weight", fresh_weight=256)
    for v in (0.0, -1.0, float("nan")):
        bad("target", target=v)
        bad("lum_floor", lum_floor=v)
    for name in ("color", "variance", "length", "offset_out"):
        bad(name, **{name: None})
    bad("alignment", color=ptr(9) + 4)
    for name in ("variance", "length", "weight_out", "offset_out", "rays_out", "pixel_out"):
        bad("alignment", **{name: ptr(9) + 2})
    common_option_refusals(bad)


def test_plan_refusals_come_in_the_documented_order(calls):
    """each later refusal is reached only once the earlier ones are out of the way"""
    plan, _ = calls
    wrong = [("reserved", dict(reserved=1)), ("empty image", dict(width=0)), ("256", dict(width=4097, height=4096)), ("budget", dict(budget=(1 << 31) + 1)),
             ("jitter", dict(jitter=9)), ("base_weight", dict(base_weight=256)), ("fresh_weight", dict(fresh_weight=256)), ("target", dict(target=0.0)),
             ("lum_floor", dict(lum_floor=0.0)), ("color", dict(color=None)), ("variance", dict(variance=None)), ("length", dict(length=None)),
             ("offset_out", dict(offset_out=None)), ("alignment", dict(pixel_out=plan.ptr(9) + 2)), ("context", dict(o=opts(context=8)))]
    for i, (word, _) in enumerate(wrong):
        kw = {}
        for _, later in reversed(wrong[i:]):   # (the earliest of those that are left wins; an earlier entry's fields overwrite a later one's)
            kw.update(later)
        assert plan(**kw) in (abi.ERR_BAD_ARG, abi.ERR_UNSUPPORTED) and word in last_error(), (word, last_error())


def test_fold_refusals_that_need_no_scene(calls):
    _, fold = calls
    ptr, bad = fold.ptr, refusals(fold)
    bad("null", null_scene=True)
    bad("null", null_args=True)
    bad("reserved", reserved=1)
    bad("empty image", width=0)
    bad("empty image", height=0)
    bad("2^32", width=65536, height=65536)
    for name in ("samples", "offset", "color_out", "length_out"):
        bad("null " + name, **{name: None})
    bad("hist_color and hist_length", hist_color=None)
    bad("hist_color and hist_length", hist_length=None)
    bad("moments_out needs hist_moments", moments_out=ptr(8))
    bad("variance_out needs moments_out", variance_out=ptr(9))
    full = dict(hist_moments=ptr(7), moments_out=ptr(8), variance_out=ptr(9))
    for name in ("samples", "hist_color", "color_out"):
        bad("alignment", **{**full, name: ptr(10) + 4})
    for name in ("offset", "hist_length", "hist_moments", "length_out", "moments_out", "variance_out"):
        bad("alignment", **{**full, name: ptr(10) + 2})
    common_option_refusals(bad)
    assert fold(width=1, height=(1 << 26)) == abi.ERR_UNSUPPORTED and "tiles" in last_error()
    # the order: of two things wrong the earlier one in the list is named
    order = [("reserved", dict(reserved=1)), ("empty image", dict(height=0)), ("null samples", dict(samples=None)), ("null offset", dict(offset=None)),
             ("null color_out", dict(color_out=None)), ("null length_out", dict(length_out=None)), ("hist_color and hist_length", dict(hist_length=None)),
             ("moments_out needs", dict(moments_out=ptr(8))), ("alignment", dict(length_out=ptr(10) + 2)),
             ("context", dict(o=opts(context=8)))]
    for (word, first), (_, second) in zip(order, order[1:]):
        assert fold(**{**second, **first}) == abi.ERR_BAD_ARG and word in last_error(), (word, last_error())


# ---- the plan as specified: properties of the literal ----------------------------------------------------------------------------
W, H = 23, 11
BUDGETS = (0, 1, W * H - 1, W * H, 3 * W * H + 7)


@pytest.fixture(scope="module")
def film():
    f = al.synthetic_film(W, H, 7100)
    for a in f.values():
        a.setflags(write=False)
    return f


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("kw", [dict(), dict(base_weight=1, fresh_weight=0), dict(target=1e30, fresh_weight=0)])
def test_offsets_deal_out_exactly_the_budget(film, budget, kw):
    w = al.weights(**film, **kw)
    off = al.offsets(w, budget).astype(np.int64)
    assert off.shape == (W * H + 1,) and off[0] == 0 and off[-1] == budget
    n = np.diff(off)
    assert (n >= 0).all() and int(n.sum()) == budget          # monotone, and the total is exact
    flat = w.reshape(-1).astype(np.int64)
    if flat.sum() == 0:
        flat = np.ones_like(flat)
    # |n_p - w_p B / S| < 1, in integers: |n_p S - w_p B| < S
    assert (np.abs(n * int(flat.sum()) - flat * budget) < int(flat.sum())).all()
    pixel = al.ray_pixels(off)
    assert pixel.shape == (budget,) and (np.diff(pixel.astype(np.int64)) >= 0).all()
    assert np.array_equal(np.bincount(pixel, minlength=W * H), n)


def test_the_noisy_half_gets_the_rays(film):
    w = al.weights(**film, target=0.02, fresh_weight=0)
    calm, noisy = w[:, :W // 2], w[:, W // 2:]
    print(f"weights: calm median {np.median(calm)}, sum {calm.sum()}; noisy median {np.median(noisy)}, sum {noisy.sum()}")
    assert np.median(calm) == 0 and np.median(noisy) >= 4     # (the calm half holds the film's special pixels, one of them at 255)
    n = np.diff(al.offsets(w, 4 * W * H).astype(np.int64)).reshape(H, W)
    assert n[:, W // 2:].sum() > 0.8 * 4 * W * H


def test_all_zero_weights_give_the_uniform_plan():
    z = np.zeros((H, W), F)
    color = np.ones((H, W, 4), F)
    w = al.weights(color, z, np.full((H, W), 9, F), fresh_weight=0)
    assert not w.any()
    for budget in BUDGETS:
        assert np.array_equal(al.offsets(w, budget), al.offsets(np.ones((H, W), np.uint32), budget))
    assert np.array_equal(al.offsets(w, W * H), np.arange(W * H + 1, dtype=np.uint32))
    assert np.array_equal(np.diff(al.offsets(w, 3 * W * H).astype(np.int64)), np.full(W * H, 3))


def test_fresh_weight_overrides_a_zero_variance_on_a_short_history(film):
    assert film["variance"][2, 7] == 0.0 and film["length"][2, 7] == 1.0
    assert al.weights(**film)[2, 7] == 255
    assert al.weights(**film, fresh_weight=17)[2, 7] == 17
    assert al.weights(**film, fresh_weight=17, min_history=1)[2, 7] == 0          # L >= min_history: a history like any other
    assert al.weights(**film, fresh_weight=17, base_weight=40)[2, 7] == 40        # max(w, fresh), not fresh
    # lengths 0, fractional and NaN are short histories too (a NaN fails L >= min_history)
    for at in ((3, 1), (3, 4), (4, 3)):
        assert al.weights(**film, fresh_weight=99, target=1e30)[at] == 99, at


def test_a_nan_anywhere_never_makes_a_weight_that_is_not_a_number(film):
    for kw in (dict(), dict(fresh_weight=0, min_history=0), dict(base_weight=255), dict(target=1e-30), dict(lum_floor=1e-30, fresh_weight=0)):
        w = al.weights(**film, **kw)
        assert w.dtype == np.uint32 and w.max() <= 255
    w = al.weights(**film, fresh_weight=0, min_history=0)
    assert w[0, 0] == 0            # NaN variance: max(NaN, 0) = 0
    assert w[1, 2] == 0            # negative variance
    assert w[2, 5] == 255          # infinite variance: min(inf, 255)
    everything = {k: np.full_like(v, np.nan) for k, v in film.items()}
    assert not al.weights(**everything, fresh_weight=0, min_history=0).any()
    assert (al.weights(**everything, fresh_weight=3) == 3).all()


def test_strata_wrap_around_a_pixels_rays():
    off = np.array([0, 6, 6, 7], np.uint32)
    assert al.ray_pixels(off).tolist() == [0] * 6 + [2]
    assert al.ray_strata(off, 2, first_stratum=3).tolist() == [3, 0, 1, 2, 3, 0, 3]
    assert al.ray_strata(off, 1, first_stratum=5).tolist() == [0] * 7


# ---- the fold ----------------------------------------------------------------------------------------------------------------------
def random_frames(rng, count, w, h):
    frames = rng.uniform(0.0, 3.0, size=(count, h, w, 4)).astype(F)
    frames[..., 3] = 1.0
    return frames


@pytest.mark.parametrize("max_history", [0, 3])
def test_one_sample_a_pixel_is_the_temporal_literal_in_identity_mode(max_history):
    w, h = 13, 7
    rng = np.random.default_rng(7200)
    frames = random_frames(rng, 5, w, h)
    frames[1, 2, 3, 0] = np.nan        # a sample that is not finite into a history
    frames[0, 4, 5, 2] = np.inf        # ... and as a first sample: length 0, the next one starts the pixel over
    frames[1, 4, 5, 1] = np.nan
    hist = tl.as_history(tl.accumulate(frames[0], max_history=max_history))
    assert hist["length"][4, 5] == 0.0
    one_each = np.arange(w * h + 1, dtype=np.uint32)
    for c in frames[1:]:
        want = tl.accumulate(c, history=hist, max_history=max_history)
        got = al.fold(c.reshape(-1, 4), one_each, hist, max_history=max_history)
        for k in ("length", "moments", "variance", "color"):
            assert np.array_equal(bits(got[k]), bits(want[k])), k
        hist = tl.as_history(want)


def test_a_ragged_list_is_that_many_accumulations():
    """frame k holds each pixel's k-th sample and NaN where it has none: the construction the GPU test uses"""
    w, h = 9, 5
    rng = np.random.default_rng(7300)
    n = rng.integers(0, 6, size=w * h)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    samples = random_frames(rng, 1, int(off[-1]), 1).reshape(-1, 4)
    samples[3, 1] = np.nan
    hist = tl.as_history(tl.accumulate(random_frames(rng, 1, w, h)[0]))
    hist["length"][1, 1] = 0.0
    got = al.fold(samples, off, hist, max_history=3)
    want = hist
    for k in range(int(n.max())):
        frame = np.full((w * h, 4), np.nan, F)
        has = n > k
        frame[has] = samples[off[:-1][has] + k]
        want = tl.as_history(tl.accumulate(frame.reshape(h, w, 4), history=want, max_history=3))
    alive = got["length"] > 0
    assert alive.sum() >= w * h - 3 and np.array_equal(bits(got["length"]), bits(want["length"]))
    assert np.array_equal(bits(got["moments"]), bits(want["moments"]))
    assert np.array_equal(bits(got["color"][alive]), bits(want["color"][alive]))
    # a pixel without samples keeps its history as it stands
    none = (n == 0).reshape(h, w)
    assert none.any() and np.array_equal(bits(got["color"][none]), bits(hist["color"][none]))
