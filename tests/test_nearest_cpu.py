"""rayca_hip_nearest_device without a GPU: the symbol, the layout of RaycaNearest in all three descriptions of the ABI (the
header, the ctypes mirror, the Rust shim), the refusals that need no scene with their messages and their order, the empty batch;
and the properties of the specification as tests/nearest_literal.py restates it, on hand-made triangles."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nearest_literal as nl
from rayca_amd import abi, flatten, scenes
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, CC = np.float32([0, 0, 0]), np.float32([4, 0, 0]), np.float32([0, 4, 0])   # a right triangle in the plane z = 0


def f32(*x):
    return np.array(x, np.float32)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_nearest_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_nearest_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # no layout changed: no new version


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaNearest %zu\\n", sizeof(RaycaNearest));',
             'printf("kinds %d\\n", RAYCA_NEAREST_CLOSEST * 10 + RAYCA_NEAREST_WITHIN);']
    for name, _ in abi.RaycaNearest._fields_:
        lines.append(f'printf("RaycaNearest.{name} %zu\\n", offsetof(RaycaNearest, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaNearest) == int(want["RaycaNearest"]) == 72
    for name, _ in abi.RaycaNearest._fields_:
        assert getattr(abi.RaycaNearest, name).offset == int(want[f"RaycaNearest.{name}"]), name
    assert int(want["kinds"]) == abi.NEAREST_CLOSEST * 10 + abi.NEAREST_WITHIN == 1


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaNearest \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)$", decl).groups()
            scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else scalar))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaNearest \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaNearest._fields_] == [n for n, _ in c_fields]
    assert [n for n, _ in c_fields] == ["kind", "count", "points", "radius", "radius_all", "reserved", "dist2_out", "prim_out", "point_out",
                                        "uv_out", "within_out"]
    assert re.search(r"pub fn rayca_hip_nearest_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, query: \*const RaycaNearest, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)
    assert "pub const RAYCA_NEAREST_CLOSEST: u32 = 0;" in shim and "pub const RAYCA_NEAREST_WITHIN: u32 = 1;" in shim


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaNearest): a query that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(64)
    scene, ptr = C.cast(dummy, C.c_void_p), C.addressof(dummy)   # (ptr stands for a device pointer: nothing is launched)

    def run(o=None, scene=scene, query=True, stats=None, **fields):
        q = abi.RaycaNearest()
        q.kind, q.count, q.points, q.radius_all = abi.NEAREST_CLOSEST, 4, ptr, float("inf")
        q.dist2_out, q.within_out = ptr, ptr
        for name, v in fields.items():
            setattr(q, name, v)
        return product_lib.rayca_hip_nearest_device(scene, C.byref(o) if o is not None else None, C.byref(q) if query else None,
                                                    C.byref(stats) if stats is not None else None)
    run.keep = dummy
    return run


def options(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


def test_struct_level_refusals_with_their_messages(call):
    assert call(scene=None) == abi.ERR_BAD_ARG and "null scene" in last_error()
    assert call(query=False) == abi.ERR_BAD_ARG and "null" in last_error()
    assert call(points=None) == abi.ERR_BAD_ARG and "null points" in last_error()
    for kind in (2, 7, 0xFFFFFFFF):
        assert call(kind=kind) == abi.ERR_BAD_ARG and "unknown kind" in last_error()
    assert call(reserved=1) == abi.ERR_BAD_ARG and "reserved must be zero" in last_error()
    assert call(dist2_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()               # CLOSEST does not write within_out
    assert call(kind=abi.NEAREST_WITHIN, within_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()   # nor WITHIN dist2_out
    for only in ("dist2_out", "prim_out", "point_out", "uv_out"):   # any one of the four will do: the call gets as far as the options
        fields = {"dist2_out": None, only: C.addressof(call.keep)}
        assert call(options(context=8), **fields) == abi.ERR_BAD_ARG and "context" in last_error(), only


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1)
    chain = [({"points": None}, "null points"), ({"kind": 9}, "unknown kind"), ({"reserved": 5}, "reserved"), ({"dist2_out": None}, "no output")]
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), chain[k][1]
    assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE), kind=abi.NEAREST_WITHIN) == abi.ERR_BAD_ARG and "engine" in last_error()
    # behind the options: EXHAUSTIVE has no WITHIN form, and is taken for CLOSEST (the empty batch returns before the scene is read)
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), kind=abi.NEAREST_WITHIN, count=0) == abi.ERR_UNSUPPORTED and "exhaustive" in last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), count=0) == abi.OK


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "nearest-point query" in last_error(), last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    """count == 0 returns RAYCA_OK behind the struct's and the options' checks, without a look at the scene (here: 64 bytes of
    zeros) or the device (there is none), and zeroes the statistics it is handed."""
    assert call(count=0) == abi.OK
    assert call(None, count=0, kind=abi.NEAREST_WITHIN) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.boxes_tested = 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.boxes_tested == 0
    assert call(count=0, reserved=1) == abi.ERR_BAD_ARG   # (checked as for any batch)


# ---- the literal on hand-made triangles --------------------------------------------------------------------------------------
REGION_CASES = [   # p, region, (s, t), q
    (f32(-1, -2, 3), 0, (0, 0), A),            # vertex a
    (f32(6, -1, 1), 1, (1, 0), B),             # vertex b
    (f32(1, -3, 2), 2, (0.25, 0), f32(1, 0, 0)),   # edge ab
    (f32(-1, 7, -1), 3, (0, 1), CC),           # vertex c
    (f32(-2, 3, 0.5), 4, (0, 0.75), f32(0, 3, 0)),   # edge ac
    (f32(4, 2, 1), 5, (0.75, 0.25), f32(3, 1, 0)),   # edge bc: t = 2 / 8
    (f32(1, 2, -3), 6, (0.25, 0.5), f32(1, 2, 0)),   # interior
]


@pytest.mark.parametrize("case", range(7))
def test_all_seven_regions(case):
    p, region, (s, t), q = REGION_CASES[case]
    gs, gt, gq, d2, greg = nl.on_triangle(A, B, CC, p)
    assert int(greg) == region
    assert (float(gs), float(gt)) == (s, t)
    assert np.array_equal(gq, q)
    assert d2 == np.float32(((p - q).astype(np.float64) ** 2).sum())   # (small integers and quarters: exact in f32)
    # the same through the brute force: one slot, every output
    dist2, prim, point, uv, within = nl.closest(np.stack([A, B, CC])[None], p[None])
    assert dist2[0] == d2 and prim[0] == 0 and within[0] == 1 and np.array_equal(point[0], q)
    assert np.array_equal(uv[0], f32((1 - s) - t, s))   # the weights of vertex 0 and vertex 1


def test_regions_do_not_depend_on_the_vertex_order():
    """Every rotation and reflection of the triangle gives the same nearest point (these inputs are exact in f32)."""
    for p, _, _, q in REGION_CASES:
        for a, b, c in ((B, CC, A), (CC, A, B), (A, CC, B), (CC, B, A), (B, A, CC)):
            _, _, gq, d2, _ = nl.on_triangle(a, b, c, p)
            assert np.array_equal(gq, q) and d2 == np.float32(((p - q).astype(np.float64) ** 2).sum())


def test_points_on_the_triangle():
    """dist2 == 0 on the surface; at a vertex and in a vertex region q is the vertex itself, whatever a + (b - a) rounds to."""
    a, b, c = f32(0.1, 0.2, 0.3), f32(1.7, 0.3, 0.9), f32(0.4, 2.3, -0.6)   # a + (b - a) != b in f32 for such coordinates
    for k, v in enumerate((a, b, c)):
        s, t, q, d2, region = nl.on_triangle(a, b, c, v)
        assert int(region) == (0, 1, 3)[k] and np.array_equal(q, v) and d2 == 0
        away = (v + (v - (a + b + c) / np.float32(3)) * np.float32(2)).astype(np.float32)   # beyond the vertex, seen from the centroid
        s, t, q, d2, region = nl.on_triangle(a, b, c, away)
        assert int(region) == (0, 1, 3)[k] and np.array_equal(q, v)
    for p in (f32(1, 1, 0), f32(2, 0, 0), f32(0, 3, 0), f32(2, 2, 0)):   # inside and on each edge of the right triangle
        _, _, q, d2, _ = nl.on_triangle(A, B, CC, p)
        assert d2 == 0 and np.array_equal(q, p)


def test_degenerate_triangle_is_skipped():
    """Two equal vertices and a point in the region of their edge: s = 0 / 0, dist2 is NaN, the slot is no candidate -- the
    next one wins, and alone it is a miss.  A triangle whose products overflow is skipped the same way."""
    a, c, p = f32(3, 2, 0), f32(5, 0, 1), f32(3, -3, 3)
    assert np.isnan(nl.on_triangle(a, a, c, p)[3])
    good = np.stack([A, B, CC])
    dist2, prim, point, uv, within = nl.closest(np.stack([np.stack([a, a, c]), good]), p[None])
    want = nl.closest(good[None], p[None])
    assert prim[0] == 1 and dist2[0] == want[0][0] and np.array_equal(point[0], want[2][0]) and within[0] == 1
    dist2, prim, point, uv, within = nl.closest(np.stack([a, a, c])[None], p[None])
    assert prim[0] == nl.NONE and dist2[0] == nl.FLT_MAX and not point.any() and not uv.any() and within[0] == 0
    huge = np.float32(1e30) * np.eye(3, dtype=np.float32)
    assert np.isnan(nl.on_triangle(huge[0], huge[1], huge[2], f32(0, 0, 0))[3])
    assert nl.closest(np.stack([huge, good]), f32(1, 1, 1)[None])[1][0] == 1


def box_triangles():
    """The Box glTF's twelve triangles in world space, from its descriptor (no build, no device)."""
    import oracle_lib as ol
    from rayca_amd import Config
    orc = ol.OracleScene(flatten(scenes.box_scene()), Config())
    t = orc.world_triangles(orc.primitive_count).reshape(-1, 3, 3)
    orc.close()
    return t


def cube_triangles(h=0.5):
    """The twelve triangles of the axis-aligned cube [-h, h]^3."""
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (-h, h):
            corner = np.zeros((4, 3), np.float32)
            corner[:, axis] = side
            corner[:, u] = [-h, h, h, -h]
            corner[:, v] = [-h, -h, h, h]
            out += [corner[[0, 1, 2]], corner[[0, 2, 3]]]
    return np.stack(out)


def strict_bound(tris, p, dist2):
    """radius * radius == dist2 misses, the next float above that radius hits"""
    r = np.float32(np.sqrt(np.float64(dist2)))
    while r * r > dist2:
        r = np.nextafter(r, np.float32(0))
    while np.nextafter(r, np.float32(np.inf)) ** 2 <= dist2:
        r = np.nextafter(r, np.float32(np.inf))
    above = np.nextafter(r, np.float32(np.inf))
    assert r * r <= dist2 < above * above
    miss = nl.closest(tris, p, radius=r)
    assert miss[1][0] == nl.NONE and miss[0][0] == nl.FLT_MAX and miss[4][0] == 0 and not miss[2].any() and not miss[3].any()
    hit, free = nl.closest(tris, p, radius=above), nl.closest(tris, p)
    assert hit[1][0] == free[1][0] and hit[0][0] == dist2 == free[0][0] and hit[4][0] == 1
    return r


def test_strict_bound_on_a_box():
    """A box at the origin, the cube [-0.5, 0.5]^3: from p = (0, 0, 1) the top face is 0.5 away and dist2 == 0.25 exactly.  The
    bound is strict: radius 0.5 (r2 == 0.25) misses, the next float above hits.  The centre is a six-way tie for the lowest slot.
    (The Box glTF's world-space vertices are +-0.49999994, its node carries a rotation: the same on it, with its own dist2.)"""
    tris = cube_triangles()
    p = f32(0, 0, 1)[None]
    dist2, prim, point, uv, within = nl.closest(tris, p)
    assert dist2[0] == np.float32(0.25) and np.array_equal(point[0], f32(0, 0, 0.5)) and within[0] == 1
    assert strict_bound(tris, p, np.float32(0.25)) == np.float32(0.5)
    box = box_triangles()
    assert box.shape == (12, 3, 3) and np.abs(np.abs(box) - 0.5).max() < 1e-6
    d2 = nl.closest(box, p)[0][0]
    assert abs(float(d2) - 0.25) < 1e-6
    strict_bound(box, p, d2)
    for t in (tris, box):
        centre = nl.closest(t, f32(0, 0, 0)[None])
        d2_all = nl.on_triangle(t[:, 0], t[:, 1], t[:, 2], f32(0, 0, 0))[3]
        ties = np.flatnonzero(d2_all == d2_all.min())
        assert ties.size >= 6 and centre[0][0] == d2_all.min() and centre[1][0] == ties[0]


def test_radii_and_points_that_give_a_miss():
    tris = np.stack([A, B, CC])[None]
    p = f32(1, 1, 2)[None]                                 # dist2 == 4
    for radius, found in ((None, 1), (np.inf, 1), (nl.FLT_MAX, 1), (2.0, 0), (np.nextafter(np.float32(2), np.float32(3)), 1), (0.0, 0), (-3.0, 0), (np.nan, 0),
                          (-np.inf, 0)):
        assert nl.closest(tris, p, radius=radius)[4][0] == found, radius
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            q = p.copy()
            q[0, axis] = bad
            got = nl.closest(tris, q)
            assert got[1][0] == nl.NONE and got[0][0] == nl.FLT_MAX and got[4][0] == 0
    # a candidate whose dist2 overflows to +inf never counts, not even unbounded
    far = f32(3e19, 3e19, 3e19)[None]
    assert np.isinf(nl.on_triangle(A, B, CC, far[0])[3]) and nl.closest(tris, far)[4][0] == 0
    per_point = nl.closest(tris, np.repeat(p, 4, 0), radius=f32(3, 2, np.nan, np.inf))
    assert per_point[4].tolist() == [1, 0, 0, 1]


def test_the_point_stays_on_the_triangle_whatever_the_rounding():
    """Far above a triangle, and beside a needle, the products cancel badly; whatever s and t come out, 0 <= s, 0 <= t,
    t <= 1 - s (the quotients of the edge regions by their operands' signs, the interior branch by its selects): q stays within
    13 x 2^-24 x the largest coordinate of the triangle's extent, which is what the kernel's cull rests on."""
    rng = np.random.default_rng(7)
    n = 6000
    a, b = rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    c = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    c[::3] = (a[::3] + (b[::3] - a[::3]) * np.float32(0.5) + rng.uniform(-1e-5, 1e-5, (n // 3, 3)).astype(np.float32)).astype(np.float32)   # needles
    w = rng.uniform(0.05, 1, (n, 3))
    w /= w.sum(1, keepdims=True)
    nrm = np.cross((b - a).astype(np.float64), (c - a).astype(np.float64))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    p = (a * w[:, :1] + b * w[:, 1:2] + c * w[:, 2:] + nrm * 10.0 ** rng.integers(0, 8, (n, 1))).astype(np.float32)
    p[1::2] = (rng.uniform(-1, 1, (n // 2, 3)) * 10.0 ** rng.integers(0, 7, (n // 2, 1))).astype(np.float32)
    s, t, q, d2, region = nl.on_triangle(a, b, c, p)
    ok = ~np.isnan(d2)
    assert ok.sum() > n - 50 and (region[ok] == 6).sum() > 1000 and all((region[ok] == k).sum() > 20 for k in range(6))
    assert (s[ok] >= 0).all() and (t[ok] >= 0).all() and (s[ok] <= 1).all() and (t[ok] <= (np.float32(1) - s[ok]) + np.float32(2.0 ** -23)).all()
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    slack = np.float32(13 * 2.0 ** -24) * np.maximum(np.abs(lo), np.abs(hi)).max()
    assert (q[ok] >= lo[ok] - slack).all() and (q[ok] <= hi[ok] + slack).all()
