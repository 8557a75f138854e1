"""rayca_hip_direct_device and rayca_hip_scene_read_lights without a GPU: the symbols, the layout of RaycaDirect and
RaycaLightRecord in the header, the ctypes mirror and the Rust shim, the refusals that need no scene with their messages and their
order, the empty batch; the properties of the specification as tests/direct_literal.py restates it; and the literal pinned to the
CPU oracle's depth-1 NEE frame."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import direct_cases as dc
import direct_literal as dl
from rayca_amd import Config, abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FIELDS = ["count", "light_first", "light_count", "sample", "first_index", "bias", "reserved", "points", "normals", "irradiance_out", "sh_out",
          "mask_out", "counts_out"]
RECORD = ["kind", "material", "intensity", "area", "color", "attenuation", "position", "ab", "ac", "normal"]


def f32(*x):
    return np.array(x, F)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries(product_lib):
    for sym in ("rayca_hip_direct_device", "rayca_hip_scene_read_lights"):
        assert sym in abi.PRODUCT_SYMBOLS and getattr(product_lib, sym) is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # additions only: no new version


def test_struct_layouts_match_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){"]
    for s in ("RaycaDirect", "RaycaLightRecord"):
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
    assert C.sizeof(abi.RaycaDirect) == int(want["RaycaDirect"]) == 80 and C.sizeof(abi.RaycaLightRecord) == int(want["RaycaLightRecord"]) == 112
    for s in ("RaycaDirect", "RaycaLightRecord"):
        for name, _ in getattr(abi, s)._fields_:
            assert getattr(getattr(abi, s), name).offset == int(want[f"{s}.{name}"]), (s, name)
    assert [n for n, _ in abi.RaycaDirect._fields_] == FIELDS and [n for n, _ in abi.RaycaLightRecord._fields_] == RECORD


def test_shim_structs_list_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    for s, names in (("RaycaDirect", FIELDS), ("RaycaLightRecord", RECORD)):
        body = re.search(r"struct %s \{(.*?)\};" % s, header, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if decl:
                const, ctype, ptr, name, _, n = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)(\[(\d+)\])?$", decl).groups()
                scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
                c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else (f"[{scalar}; {n}]" if n else scalar)))
        rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s \{(.*?)\n\}" % s, shim, flags=re.S).group(1)
        r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
        assert r_fields == c_fields and [n for n, _ in c_fields] == names, s
    assert re.search(r"pub fn rayca_hip_direct_device\(scene: \*mut RaycaScene, cfg: \*const RaycaConfig, opts: \*const RaycaRenderOptions, "
                     r"direct: \*const RaycaDirect, stats_out: \*mut RaycaStats\) -> i32;", shim)
    assert re.search(r"pub fn rayca_hip_scene_read_lights\(scene: \*mut RaycaScene, out: \*mut RaycaLightRecord, capacity: u32, count_out: \*mut u32\) -> i32;", shim)


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaDirect): a call that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(128)
    ptr = (C.addressof(dummy) + 15) // 16 * 16                     # (stands for a device pointer: nothing is launched)
    scene = C.c_void_p(ptr)

    def run(o=None, scene=scene, struct=True, cfg=True, stats=None, light_samples=1, **fields):
        a = abi.RaycaDirect()
        a.count, a.light_count, a.points, a.normals, a.irradiance_out = 4, 1, ptr, ptr, ptr
        for name, v in fields.items():
            if isinstance(v, tuple):
                getattr(a, name)[:] = v
            else:
                setattr(a, name, v)
        c = Config(light_samples=light_samples).to_abi()
        return product_lib.rayca_hip_direct_device(scene, C.byref(c) if cfg else None, C.byref(o) if o is not None else None,
                                                   C.byref(a) if struct else None, C.byref(stats) if stats is not None else None)
    run.ptr = ptr
    run.keep = dummy
    return run


def options(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


def test_struct_level_refusals_with_their_messages(call):
    bad = abi.ERR_BAD_ARG
    assert call(scene=None) == bad and "null scene" in last_error()
    assert call(struct=False) == bad and "null" in last_error()
    assert call(cfg=False) == bad and "null" in last_error()
    assert call(points=None) == bad and "null points" in last_error()
    assert call(light_count=0) == bad and "light_count" in last_error()
    assert call(light_samples=0) == bad and "light_samples" in last_error()
    for lc, ls in ((65, 1), (1, 65), (2, 33), (0xFFFFFFFF, 0xFFFFFFFF), (1 << 16, 1 << 16)):
        assert call(light_count=lc, light_samples=ls) == bad and "64" in last_error(), (lc, ls)
    assert call(options(context=8), light_count=2, light_samples=32) == bad and "context" in last_error()    # (64 samples are allowed)
    assert call(reserved=(1, 0)) == bad and "reserved must be zero" in last_error()
    assert call(reserved=(0, 1)) == bad and "reserved must be zero" in last_error()
    assert call(irradiance_out=None) == bad and "no output" in last_error()
    for only in ("irradiance_out", "mask_out", "counts_out"):      # any one will do: the call gets as far as the options
        assert call(options(context=8), **{"irradiance_out": None, only: call.ptr}) == bad and "context" in last_error(), only
    assert call(options(context=8), normals=None, irradiance_out=None, sh_out=call.ptr) == bad and "context" in last_error()
    assert call(sh_out=call.ptr) == bad and "sh_out" in last_error() and "normals" in last_error()
    for v in (1e-4, -1.0, float("nan"), float("inf")):
        assert call(normals=None, bias=v) == bad and "bias must be 0" in last_error(), v
    assert call(options(context=8), normals=None, bias=-0.0) == bad and "context" in last_error()
    for field, align in (("irradiance_out", 16), ("sh_out", 16), ("mask_out", 8), ("counts_out", 4)):
        for off in (1, 2, 4, 8):
            rc = call(**{"normals": None, field: call.ptr + off})
            if off % align:
                assert rc == bad and field in last_error() and "aligned" in last_error(), (field, off)
    assert call(options(context=8), mask_out=call.ptr + 8, counts_out=call.ptr + 4) == bad and "context" in last_error()
    for v in (float("nan"), float("inf"), float("-inf")):
        assert call(bias=v) == bad and "not finite" in last_error()
    assert call(first_index=0xFFFFFFFF, count=2) == bad and "first_index" in last_error()
    assert call(options(context=8), first_index=0xFFFFFFFE, count=2) == bad and "context" in last_error()
    assert call(count=1 << 26, light_count=64) == bad and "2^32" in last_error()
    assert call(options(context=8), count=(1 << 26) - 1, light_count=64) == bad and "context" in last_error()


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)
    chain = [({"points": None}, "null points"), ({"light_count": 0}, "light_count"), ({"light_samples": 0}, "light_samples"),
             ({"reserved": (0, 3)}, "reserved"), ({"irradiance_out": None}, "no output")]
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), (chain[k][1], last_error())
    # the rules that cannot be broken together with "no output" or with each other
    assert call(bad_opts, light_count=65, reserved=(1, 0)) == abi.ERR_BAD_ARG and "64" in last_error()
    tail = [({"sh_out": call.ptr + 4}, "not with normals"), ({"counts_out": call.ptr + 2}, "counts_out"), ({"bias": float("inf")}, "not finite"),
            ({"first_index": 0xFFFFFFFF, "count": 0xFFFFFFFF}, "first_index")]
    for k in range(len(tail)):
        fields = {}
        for f, _ in tail[k:]:
            fields.update(f)
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and tail[k][1] in last_error(), (tail[k][1], last_error())
    assert call(bad_opts, normals=None, bias=float("nan"), sh_out=call.ptr + 4) == abi.ERR_BAD_ARG and "bias must be 0" in last_error()
    assert call(bad_opts, normals=None, sh_out=call.ptr + 4, mask_out=call.ptr + 4) == abi.ERR_BAD_ARG and "sh_out" in last_error()
    assert call(bad_opts, count=1 << 26, light_count=64) == abi.ERR_BAD_ARG and "2^32" in last_error()
    assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_BAD_ARG and "engine" in last_error()
    # behind the options: EXHAUSTIVE has no form (the empty batch returns behind it, before the scene is read)
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), count=0) == abi.ERR_UNSUPPORTED and "exhaustive" in last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_UNSUPPORTED


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "direct-light call" in last_error(), last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    assert call(count=0) == abi.OK
    assert call(None, count=0, normals=None, sh_out=call.ptr) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.rays_shadow = 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.rays_shadow == 0
    assert call(count=0, reserved=(1, 0)) == abi.ERR_BAD_ARG      # (checked as for any batch)


def test_read_lights_refusals(product_lib):
    dummy = C.create_string_buffer(256)
    n = C.c_uint32(0)
    assert product_lib.rayca_hip_scene_read_lights(None, None, 0, C.byref(n)) == abi.ERR_BAD_ARG and "null scene" in last_error()
    assert product_lib.rayca_hip_scene_read_lights(C.c_void_p(C.addressof(dummy)), None, 0, None) == abi.ERR_BAD_ARG and "count_out" in last_error()
    assert product_lib.rayca_hip_scene_read_lights(None, None, 0, None) == abi.ERR_BAD_ARG and "null scene" in last_error()


# ---- the literal ---------------------------------------------------------------------------------------------------------------
def test_point_light_over_a_plane_is_the_closed_form():
    """E = I c cos / (fallof r^2) with cos = h / r: the reference's intensity over its own fall-off, times its extra 1 / r^2"""
    L = dc.point_light((0.25, 2.0, -0.5), (4, 3, 2), (0.5, 0.25, 0.125), intensity=1.5)
    x, z = np.meshgrid(np.linspace(-3, 3, 25), np.linspace(-3, 3, 25))
    p = np.stack([x.ravel(), np.zeros(x.size), z.ravel()], 1).astype(F)
    n = np.tile(f32(0, 1, 0), (p.shape[0], 1))
    s = dl.samples([L], p, n)
    out = dl.fold(s, np.ones((p.shape[0], 1), bool))
    d = L["position"].astype(np.float64) - p
    r = np.linalg.norm(d, axis=1)
    want = 1.5 * np.array([4, 3, 2.0])[None] / (0.5 + 0.25 * r + 0.125 * r * r)[:, None] * (2.0 / r)[:, None] / (r * r)[:, None]
    assert np.abs(out["irradiance"][:, :3] / want - 1).max() < 16 * 2.0 ** -24     # a dozen roundings from the inputs to y
    assert (out["irradiance"][:, 3] == 1).all() and (out["mask"] == 1).all() and (out["counts"] == 1).all()
    assert np.allclose(s["tmax"][:, 0], r, rtol=1e-6) and not s["quad"].any()
    # sphere mode: the same without the cosine; its SH9 band 0 is Y0 times it
    s2 = dl.samples([L], p, None)
    o2 = dl.fold(s2, np.ones((p.shape[0], 1), bool), sh=True)
    assert np.abs(o2["irradiance"][:, :3] * (2.0 / r)[:, None] / want - 1).max() < 16 * 2.0 ** -24
    assert np.array_equal(o2["sh"][:, 0, :3], (o2["irradiance"][:, :3] * F(0.2820948)).astype(F)) and (o2["sh"][:, :, 3] == 0).all()


def rect_form_factor_integral(p, a, ab, ac, m=400):
    """the integral of cos_light / r^2 over the rectangle a + s ab + t ac seen from p, with the reference's unnegated
    dot(normal, omega): midpoint rule in float64"""
    s = (np.arange(m) + 0.5) / m
    x = a[None, None] + s[:, None, None] * ab[None, None] + s[None, :, None] * ac[None, None]
    v = x - p
    r2 = (v * v).sum(-1)
    nl = np.cross(ab, ac)
    area = np.linalg.norm(nl)
    nl = nl / area
    return ((v @ nl) / np.sqrt(r2) / r2).mean() * area


def test_quad_light_mean_is_the_area_integral():
    """2^16 keys at one point under the lamp, sphere mode, all lit: the mean of le area dot(N, omega) / r^2 over uniform points of
    the quad is le times the integral above.  Held within 5 standard errors of the literal's own sample variance."""
    L = dc.LAMP_UP
    n_keys = 1 << 16
    p = np.tile(f32(0.2, 0.6, -0.1), (n_keys, 1))
    s = dl.samples([L], p, None, seed=21)
    assert s["quad"].all() and s["traced"].all() and np.isinf(s["tmax"]).all()
    y = s["y"][:, 0, 0].astype(np.float64)
    want = 6.0 * rect_form_factor_integral(p[0].astype(np.float64), *(L[k].astype(np.float64) for k in ("position", "ab", "ac")))
    se = y.std(ddof=1) / math.sqrt(n_keys)
    print(f"mean {y.mean():.6f}, integral {want:.6f}, standard error {se:.2e}")
    assert want > 0 and abs(y.mean() - want) <= 5 * se
    # from above the lamp the unnegated dot is negative: the contribution is negative, not void
    above = dl.samples([L], f32(0.0, 1.995, 0.0)[None], None, seed=21)
    assert (above["y"] < 0).all() and above["traced"].all()


def test_dimension_rule_light_ranges_are_rows_of_the_full_call():
    L = dc.LIGHTS["qpq"]
    p, n = dc.surface_points("qpq", 65)
    for ls, strat in ((1, False), (4, True), (3, False)):
        kw = dict(light_samples=ls, stratify=strat, seed=5, first_index=77, sample=2, bias=dc.BIAS)
        full = dl.samples(L, p, n, **kw)
        for first, cnt in ((0, 1), (1, 1), (2, 1), (1, 2), (0, 2)):
            part = dl.samples(L, p, n, light_first=first, light_count=cnt, **kw)
            sl = slice(first * ls, (first + cnt) * ls)
            for k in ("y", "omega", "tmax"):
                assert np.array_equal(part[k].view(np.uint32), full[k][:, sl].view(np.uint32)), (ls, first, cnt, k)
        # the second quad light draws behind the first one's 2 ls dimensions, the point light draws none: put first, it draws the same
        alone = dl.samples([L[2], L[1], L[0]], p, n, light_first=0, light_count=1, **kw)
        assert not np.array_equal(alone["omega"], full["omega"][:, 2 * ls:])
        shifted = dl.samples([L[0], L[2]], p, n, light_first=1, light_count=1, **kw)
        assert np.array_equal(shifted["omega"].view(np.uint32), full["omega"][:, 2 * ls:].view(np.uint32))
    # the stream is the point index's: first_index + i names it, the sample number separates streams
    a = dl.samples(L, p, n, light_samples=1, seed=5, first_index=100)
    b = dl.samples(L, p[10:], n[10:], light_samples=1, seed=5, first_index=110)
    assert np.array_equal(a["y"][10:].view(np.uint32), b["y"].view(np.uint32))
    assert not np.array_equal(a["y"], dl.samples(L, p, n, light_samples=1, seed=5, first_index=100, sample=1)["y"])


def test_stratification_puts_sample_k_in_its_cell():
    L = dc.LAMP_UP
    p = np.tile(f32(0.1, 0.5, 0.2), (512, 1))
    assert dl.strate_count(4, True) == 2 and dl.strate_count(8, True) == 2 and dl.strate_count(64, True) == 8 and dl.strate_count(64, False) == 1
    s = dl.samples([L], p, None, light_samples=4, stratify=True, seed=3)
    a, ab, ac = (L[k].astype(np.float64) for k in ("position", "ab", "ac"))
    t = (a[1] - p[0, 1]) / s["omega"][..., 1].astype(np.float64)                                     # the lamp's plane y = 1.98
    hit = p[:, None, :].astype(np.float64) + s["omega"].astype(np.float64) * t[..., None]
    u = (hit - a) @ ab / (ab @ ab)
    v = (hit - a) @ ac / (ac @ ac)
    for k in range(4):
        assert (np.floor(u[:, k] * 2 + 1e-6).clip(0, 1) == k % 2).all() and (np.floor(v[:, k] * 2 + 1e-6).clip(0, 1) == k // 2).all(), k
    plain = dl.samples([L], p, None, light_samples=4, stratify=False, seed=3)
    pu = ((p[:, None, :] + plain["omega"].astype(np.float64) * ((a[1] - p[0, 1]) / plain["omega"][..., 1].astype(np.float64))[..., None]) - a) @ ab / (ab @ ab)
    assert pu.min() < 0.1 and pu.max() > 0.9                       # without stratification every sample covers the whole quad


def test_dropped_void_and_inactive_samples():
    L = dc.LIGHTS["dim"]                                           # intensity 0; alpha 0.5
    p, n = dc.surface_points("dim", 65)
    s = dl.samples(L, p, n, light_samples=2, bias=dc.BIAS)
    act = dl.active(p, n)
    assert act.sum() == 60 and not s["traced"][~act].any() and not s["dropped"][~act].any() and not s["void"][~act].any()
    assert s["void"][act][:, :2].sum() >= 59 * 2                   # the light of intensity 0: every sample but the one on it
    assert s["dropped"][dc.ON_LIGHT].tolist() == [True, True, False, False]      # 0 * inf on the light itself
    flipped = act & (np.arange(65) % 2 == 1)
    front = (np.einsum("ij,ij->i", n, L[1]["position"][None] - p) > 1e-3) & act
    assert s["void"][~front & act][:, 2:].all() and s["traced"][front][:, 2:].all() and flipped.any()
    out = dl.fold(s, np.ones((65, 4), bool))
    assert not out["irradiance"][~act].any() and not out["mask"][~act].any() and not out["counts"][~act].any()
    assert out["counts"][dc.ON_LIGHT] == 2 << 16 | (2 if front[dc.ON_LIGHT] else 0)
    assert np.array_equal(out["mask"][front], np.full(front.sum(), 0b1100, np.uint64))
    # lit is read for traced samples alone
    assert all(np.array_equal(out[k], dl.fold(s, s["traced"])[k]) for k in out)
    # sphere mode: only the coordinates decide
    v = dc.volume_points("dim", 65)
    s2 = dl.samples(L, v, None)
    assert s2["active"].sum() == 63 and s2["dropped"][dc.ON_LIGHT, 0] and s2["void"][s2["active"]][:, 0].sum() == 62


def test_alpha_weighs_the_sum():
    p, n = dc.surface_points("dim", 65)
    half = dl.samples(dc.LIGHTS["dim"], p, n, bias=dc.BIAS)
    whole = dl.samples([dc.LIGHTS["dim"][0], dict(dc.LIGHTS["dim"][1], color=f32(1, 2, 3, 1))], p, n, bias=dc.BIAS)
    t = half["traced"][:, 1]
    assert t.sum() > 20 and np.array_equal(half["traced"], whole["traced"])
    assert np.array_equal(half["y"][t, 1], (whole["y"][t, 1] * F(0.5)).astype(F))


# ---- the literal against the oracle's path vertex -----------------------------------------------------------------------------------
def oracle_visibility(orc, s):
    P, N = s["tmax"].shape
    rays = np.concatenate([s["o"], s["omega"]], 2).reshape(-1, 6).copy()
    traced = s["traced"].reshape(-1)
    rays[~traced] = [0, 0, 0, 1, 0, 0]
    t, prim, uv, _ = orc.trace_rays(rays)
    hit = prim != 0xFFFFFFFF
    emissive = (orc.surface(None, t, prim, uv, want=("flags",))["flags"] & 4) != 0
    return np.where(np.tile(s["quad"], P), hit & emissive, ~(hit & (t < s["tmax"].reshape(-1)))).reshape(P, N)


@pytest.mark.parametrize("light_samples,stratify", [(1, False), (4, True)])
def test_literal_is_the_oracles_path_vertex(light_samples, stratify):
    """A depth-1 Pathtracer NEE frame of the oracle, gamma 1, on the room of Phong surfaces with ks = 0 and shininess 0 under a
    quad, a point and a second quad light: every pixel whose surface is not emissive against kd / pi * E, E the literal's at the
    oracle's own hit point and normal with the oracle's own visibility.  Per term the frame rounds brdf = kd * (1 / pi), le * brdf,
    * ndot, * d_omega, * alpha; the literal rounds le * ndot, * d_omega, * alpha and the test kd * (1 / pi), * E: five each.  Both
    sum N terms.  Pixels all of whose terms are >= 0 are held to the relative bound (2 N + 8) 2^-24 (1 + 2^-20); where a term is
    negative (behind the back-wall lamp's plane) the bound is that fraction of the sum of the terms' magnitudes."""
    name = "qpq"
    orc = dc.oracle_scene(name)
    cfg = Config(max_depth=1, light_samples=light_samples, light_stratify=stratify, gamma=1.0, seed=13)
    w, h = 48, 36
    _, frame, _ = orc.render(cfg, w, h, want_rgba8=False)
    rays = orc.camera_rays(cfg, w, h)
    t, prim, uv, _ = orc.trace_rays(rays)
    g = orc.surface(rays, t, prim, uv, want=("point", "normal", "diffuse", "specular", "rough", "flags"))
    hit = prim != 0xFFFFFFFF
    keep = hit & ((g["flags"] & 4) == 0)
    assert keep.sum() > 1000 and not g["specular"][keep][:, :3].any() and not g["rough"][keep][:, 1].any()
    p, n = g["point"][keep], g["normal"][keep]
    idx = np.flatnonzero(keep)
    L = dc.lights_of(name)
    N = len(L) * light_samples
    E = np.zeros((idx.size, 3), F)
    mag = np.zeros((idx.size, 3), np.float64)
    lit_total = 0
    for k, i in enumerate(idx):      # (one call per pixel: first_index names the pixel's stream)
        s = dl.samples(L, p[k:k + 1], n[k:k + 1], light_samples=light_samples, stratify=stratify, seed=cfg.seed, first_index=int(i), bias=1e-4)
        lit = oracle_visibility(orc, s)
        out = dl.fold(s, lit)
        assert out["counts"][0] >> 16 == 0
        E[k] = out["irradiance"][0, :3]
        mag[k] = np.abs(s["y"][0][lit[0] & s["traced"][0]].astype(np.float64)).sum(0)
        lit_total += int(out["counts"][0] & 0xFFFF)
    kd = g["diffuse"][keep][:, :3]
    want = (kd * F(0.318309873342514038086)) * E
    got = frame.reshape(-1, 4)[keep][:, :3]
    bound = (2 * N + 8) * 2.0 ** -24 * (1 + 2.0 ** -20)
    scale = (kd.astype(np.float64) / np.pi) * mag
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = np.where(scale > 0, err / np.maximum(scale, 1e-300), err)
    print(f"{idx.size} pixels, {lit_total} lit samples, largest difference / sum of magnitudes {rel.max():.3e}, bound {bound:.3e}")
    assert lit_total > idx.size and (E > 0).any()
    assert rel.max() <= bound
