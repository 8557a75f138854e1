"""rayca_hip_surface_cdf_device / rayca_hip_surface_sample_device without a GPU: the symbols, the layout of RaycaSurfaceCdf and
RaycaSurfaceSample in all three descriptions of the ABI (the header, the ctypes mirror, the Rust shim), the refusals that need no
scene with their messages and their order, the empty batch, the library's self-test (the picker of k_sample_surface is one of
its families); and the properties of the specification as tests/sample_literal.py restates it."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sample_cases as sc
import sample_literal as sl
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"RaycaSurfaceCdf": (24, ["include", "cdf_out", "flags", "reserved"]),
           "RaycaSurfaceSample": (64, ["count", "seed", "sample", "first_index", "cdf", "prim_out", "uv_out", "point_out", "normal_out", "reserved"])}
F = np.float32


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries(product_lib):
    for sym in ("rayca_hip_surface_cdf_device", "rayca_hip_surface_sample_device"):
        assert sym in abi.PRODUCT_SYMBOLS and getattr(product_lib, sym) is not None
    # two functions and their structs are added and no layout changes, so by the header's rule the version stays: every
    # descriptor that a host built against the previous header fills is still the one this library reads
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "rayca_hip.h")).read()
    note = header[header.index("#define RAYCA_ABI_VERSION"):header.index("#define RAYCA_NONE")]
    for name in ("RaycaSurfaceCdf", "rayca_hip_surface_cdf_device", "RaycaSurfaceSample", "rayca_hip_surface_sample_device"):
        assert name in note, name


def test_struct_layouts_match_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){"]
    for s in STRUCTS:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for name, _ in getattr(abi, s)._fields_:
            lines.append(f'printf("{s}.{name} %zu\\n", offsetof({s}, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    for s, (size, _) in STRUCTS.items():
        cls = getattr(abi, s)
        assert C.sizeof(cls) == int(want[s]) == size, s
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == int(want[f"{s}.{name}"]), f"{s}.{name}"


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_shim_structs_list_the_headers_fields(struct):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct %s \{(.*?)\};" % struct, header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)$", decl).groups()
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else {"uint32_t": "u32", "float": "f32"}[ctype]))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s \{(.*?)\n\}" % struct, shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in getattr(abi, struct)._fields_] == [n for n, _ in c_fields] == STRUCTS[struct][1]
    entry, arg = {"RaycaSurfaceCdf": ("rayca_hip_surface_cdf_device", "table"), "RaycaSurfaceSample": ("rayca_hip_surface_sample_device", "draw")}[struct]
    assert re.search(r"pub fn %s\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, %s: \*const %s, stats_out: \*mut RaycaStats\) -> i32;"
                     % (entry, arg, struct), shim)


def test_selftest_covers_the_new_picker(product_lib):
    from rayca_amd import lib
    lib.check(product_lib.rayca_hip_selftest())
    assert "pick_sample_kernel(geom)" in open(os.path.join(ROOT, "rayca_amd", "csrc", "select.inc")).read()


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calls(product_lib):
    """(table, draw): calls that pass every check unless a field says otherwise.  The scene handle is any non-NULL value: every
    refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(64)
    scene, ptr = C.cast(dummy, C.c_void_p), C.addressof(dummy)   # (ptr stands for a device pointer: nothing is launched)
    assert ptr % 8 == 0

    def run(fn, a, o, scene, args, stats):
        return fn(scene, C.byref(o) if o is not None else None, C.byref(a) if args else None, C.byref(stats) if stats is not None else None)

    def table(o=None, scene=scene, args=True, stats=None, **fields):
        a = abi.RaycaSurfaceCdf()
        a.cdf_out = ptr
        for name, v in fields.items():
            setattr(a, name, v)
        return run(product_lib.rayca_hip_surface_cdf_device, a, o, scene, args, stats)

    def draw(o=None, scene=scene, args=True, stats=None, **fields):
        a = abi.RaycaSurfaceSample()
        a.count, a.cdf, a.prim_out = 4, ptr, ptr
        for name, v in fields.items():
            setattr(a, name, v)
        return run(product_lib.rayca_hip_surface_sample_device, a, o, scene, args, stats)
    table.ptr = draw.ptr = ptr
    table.keep = dummy
    return table, draw


def options(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


def test_struct_level_refusals_with_their_messages(calls):
    table, draw = calls
    for call, struct in ((table, "RaycaSurfaceCdf"), (draw, "RaycaSurfaceSample")):
        assert call(scene=None) == abi.ERR_BAD_ARG and "null scene" in last_error()
        assert call(args=False) == abi.ERR_BAD_ARG and "null scene or " + struct in last_error()
        assert call(reserved=1) == abi.ERR_BAD_ARG and struct + ".reserved must be zero" in last_error()
    assert table(flags=1) == abi.ERR_BAD_ARG and "RaycaSurfaceCdf.flags must be zero" in last_error()
    assert table(cdf_out=None) == abi.ERR_BAD_ARG and "RaycaSurfaceCdf.cdf_out: null" in last_error()
    assert table(cdf_out=table.ptr + 4) == abi.ERR_BAD_ARG and "RaycaSurfaceCdf.cdf_out: alignment" in last_error()
    assert draw(cdf=None) == abi.ERR_BAD_ARG and "RaycaSurfaceSample.cdf: null" in last_error()
    assert draw(cdf=draw.ptr + 4) == abi.ERR_BAD_ARG and "RaycaSurfaceSample.cdf: alignment" in last_error()
    assert draw(prim_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()
    for field in ("prim_out", "uv_out", "point_out", "normal_out"):
        assert field in last_error()                                  # every field is named
    for only in ("prim_out", "uv_out", "point_out", "normal_out"):   # any one of the four will do: the call gets as far as the options
        assert draw(options(context=8), **{"prim_out": None, only: draw.ptr}) == abi.ERR_BAD_ARG and "context" in last_error(), only
    assert table(options(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()


def test_refusals_come_in_the_documented_order(calls):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    table, draw = calls
    bad_opts = options(context=8, engine=1)
    chains = ((table, [({"reserved": 5}, "reserved"), ({"flags": 2}, "flags"), ({"cdf_out": None}, "null cdf_out")]),
              (table, [({"flags": 2}, "flags"), ({"cdf_out": table.ptr + 1}, "alignment")]),
              (draw, [({"reserved": 5}, "reserved"), ({"cdf": None}, "null cdf"), ({"prim_out": None}, "no output")]),
              (draw, [({"cdf": draw.ptr + 2}, "alignment"), ({"prim_out": None}, "no output")]))
    for call, chain in chains:
        for k in range(len(chain)):
            fields = {}
            for f, _ in chain[k:]:
                fields.update(f)
            assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), chain[k][1]
        assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
        assert call(options(engine=1, traversal=1)) == abi.ERR_BAD_ARG and "traversal" in last_error()


def test_options_that_do_not_apply_are_refused(calls):
    for call, what in zip(calls, ("surface-table call", "surface-sampling call")):
        for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved", "traversal"):
            assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
            assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and what in last_error(), last_error()


def test_empty_batch_is_ok_and_launches_nothing(calls):
    """count == 0 returns RAYCA_OK behind the struct's and the options' checks, without a look at the scene (here: 64 bytes of
    zeros) or the device (there is none), and zeroes the statistics it is handed."""
    _, draw = calls
    assert draw(count=0) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.rays_primary = 7, 7
    assert draw(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.rays_primary == 0
    assert draw(count=0, reserved=1) == abi.ERR_BAD_ARG   # (checked as for any batch)
    assert draw(count=0, prim_out=None) == abi.ERR_BAD_ARG


# ---- the literal ----------------------------------------------------------------------------------------------------------------
N = 1 << 20
UNIT = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)


@pytest.fixture(scope="module")
def soup():
    """the soup, its table and 2^20 draws with seed 7, made once and shared (read-only)"""
    tris = sc.soup_triangles()
    table = sl.cdf(tris)
    prim, uv, point, normal = sl.draw(tris, table, N, seed=7)
    return dict(tris=tris, table=table, prim=prim, uv=uv, point=point, normal=normal)


def test_hash_matches_the_library(product_lib):
    """the first floats of a stream as the kernels draw them: rng_f32 keeps its bits with rng_word in between (values fixed by
    the arithmetic of rayca_math.hpp, restated here on Python integers)"""
    def mix(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B & 0xFFFFFFFF
        h ^= h >> 13
        h = h * 0xC2B2AE35 & 0xFFFFFFFF
        return h ^ h >> 16

    def hash2(a, b):
        return mix(a * 0x9E3779B1 + mix(b + 0x7F4A7C15 & 0xFFFFFFFF) & 0xFFFFFFFF)
    for seed, index, sample in ((0, 0, 0), (7, 12345, 3), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        key = hash2(hash2(seed, index), sample)
        assert int(sl.rng_root(seed, np.array([index], np.uint32), sample)[0]) == key
        for dim in range(4):
            assert int(sl.rng_word(np.array([key], np.uint32), dim)[0]) == hash2(key ^ 0xA511E9B3, dim)
    text = open(os.path.join(ROOT, "rayca_amd", "csrc", "rayca_math.hpp")).read()
    assert "return rng_hash2(key ^ 0xA511E9B3u, dim)" in text and "const uint32_t u = rng_word(key, dim);" in text


def test_barycentrics_stay_in_the_triangle(soup):
    key = sl.keys(N, seed=7)
    s, t = sl.barycentrics(key)
    assert (s >= 0).all() and (t >= 0).all() and (s.astype(np.float64) + t.astype(np.float64) <= 1).all()
    u = (F(1) - s) - t
    assert (u >= 0).all() and (u.astype(np.float64) + s + t == 1).all()   # every operation of the tail is exact
    # the four mid-point sub-triangles: a quarter each
    which = np.where(s > 0.5, 1, np.where(t > 0.5, 2, np.where(s + t < 0.5, 0, 3)))
    sigma = np.sqrt(N * 0.25 * 0.75)
    for k in range(4):
        z = ((which == k).sum() - N / 4) / sigma
        print(f"sub-triangle {k}: z = {z:+.2f}")
        assert abs(z) < 5


def test_slots_are_drawn_by_area(soup):
    """every slot with an expected count of at least 20 within |z| < 5 of its share (a binomial's sigma)"""
    tris, table, prim = soup["tris"], soup["table"], soup["prim"]
    area = np.linalg.norm(np.cross((tris[:, 1] - tris[:, 0]).astype(np.float64), (tris[:, 2] - tris[:, 0]).astype(np.float64)), axis=1)
    share = area / area.sum()
    w = np.diff(np.array(table, dtype=object)).astype(np.float64)
    assert np.abs(w / w.sum() - share).max() < 1e-7   # the integer weights are the areas' shares
    count = np.bincount(prim, minlength=tris.shape[0])
    often = share * N >= 20
    z = (count - share * N) / np.sqrt(N * share * (1 - share))
    chi2 = float((z[often] ** 2).mean())
    print(f"{often.sum()} slots with an expected count >= 20: max |z| = {np.abs(z[often]).max():.2f}, chi^2 per slot = {chi2:.3f}")
    assert often.sum() > 500 and np.abs(z[often]).max() < 5
    assert 0.8 < chi2 < 1.25


def test_points_and_normals_belong_to_the_slot(soup):
    tris, prim, uv, point, normal = (soup[k] for k in ("tris", "prim", "uv", "point", "normal"))
    a, b, c = (tris[prim, k].astype(np.float64) for k in range(3))
    w0, w1 = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    want = a * w0[:, None] + b * w1[:, None] + c * (1 - w0 - w1)[:, None]
    assert np.abs(point - want).max() < 8 * 2.0 ** -24 * np.abs(tris).max()
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    big = np.linalg.norm(np.cross(b - a, c - a), axis=1) > 1e-6   # (needles' normals cancel in f32: checked by length only)
    assert np.abs(normal[big] - n[big]).max() < 1e-3
    assert np.abs(np.linalg.norm(normal.astype(np.float64), axis=1) - 1).max() < 4 * 2.0 ** -24


def test_triangles_without_area_are_never_drawn():
    tris, drawable = sc.degenerate_triangles()
    extra = np.array([[[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]],            # NaN
                      [[0, 0, 0], [3e30, 0, 0], [0, 3e30, 0]],          # the products overflow: n.z = +inf
                      [[1e30, 0, 0], [-3e38, 0, 0], [0, 3e38, 0]]], F)  # b - a overflows
    tris, drawable = np.concatenate([tris, extra]), np.concatenate([drawable, [False] * 3])
    w = sl.weights(tris)
    assert [x > 0 for x in w] == drawable.tolist()
    assert max(w) >= 1 << 31            # the largest area's weight has its top bit set
    prim = sl.draw(tris, sl.cdf(tris), 1 << 16, seed=3)[0]
    assert set(np.unique(prim)) == set(np.flatnonzero(drawable))


def test_a_slot_below_2_to_the_minus_32_of_the_largest_weighs_nothing():
    big = F(1.5)
    # amax = 1.5 = 0.75 * 2^1, so the shift is 2^31: the second area is 1.5 x ratio and its weight floor(1.5 x ratio x 2^31)
    for ratio, weight in ((2.0 ** -29, 6), (2.0 ** -30, 3), (2.0 ** -31, 1), (2.0 ** -32, 0), (2.0 ** -33, 0), (2.0 ** -60, 0)):
        tris = np.array([[[0, 0, 0], [big, 0, 0], [0, 1, 0]], [[0, 0, 0], [big * F(ratio), 0, 0], [0, 1, 0]]], F)
        assert sl.weights(tris) == [3 << 30, weight], ratio
    # the weights follow the largest area's exponent, whatever the scene's scale
    for scale in (2.0 ** -30, 1.0, 2.0 ** 30):
        tris = (np.array([[[0, 0, 0], [1.5, 0, 0], [0, 1, 0]], [[0, 0, 0], [0.75, 0, 0], [0, 1, 0]]]) * scale).astype(F)
        assert sl.weights(tris) == [3 << 30, 3 << 29], scale


def test_masks(soup):
    tris = soup["tris"]
    none = sl.cdf(tris, np.zeros(tris.shape[0], np.uint8))
    assert not any(none)
    prim, uv, point, normal = sl.draw(tris, none, 1000, seed=1)
    assert (prim == sl.NONE).all() and not uv.any() and not point.any() and not normal.any()
    keep = np.arange(tris.shape[0]) % 3 == 1
    prim = sl.draw(tris, sl.cdf(tris, keep), 1 << 14, seed=1)[0]
    assert keep[prim].all()
    # the maximum is taken over the slots that count: dropping the largest rescales the others
    largest = int(np.argmax(sl.areas(tris)))
    keep = np.ones(tris.shape[0], bool)
    keep[largest] = False
    assert max(np.diff(np.array(sl.cdf(tris, keep), dtype=object))) >= 1 << 31


def test_prefix_and_chunks(soup):
    tris, table = soup["tris"], soup["table"]
    whole = sl.draw(tris, table, 1000, seed=7)
    for got, want in zip(whole, (soup[k] for k in ("prim", "uv", "point", "normal"))):
        assert np.array_equal(got.view(np.uint32), want[:1000].view(np.uint32))   # sample j does not depend on count
    parts = [sl.draw(tris, table, n, seed=7, first_index=first) for first, n in ((0, 1), (1, 63), (64, 500), (564, 436))]
    for k in range(4):
        assert np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint32), whole[k].view(np.uint32))
    wrap = sl.draw(tris, table, 8, seed=7, first_index=0xFFFFFFFC)   # the index wraps at 2^32
    assert np.array_equal(wrap[0][4:], whole[0][:4])
    assert not np.array_equal(sl.draw(tris, table, 1000, seed=7, sample=1)[0], whole[0])
