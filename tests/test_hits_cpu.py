"""rayca_hip_hits_device without a GPU: the symbol, the layout of RaycaHits in all three descriptions of the ABI (the header, the
ctypes mirror, the Rust shim), every refusal that needs no scene with its message and its place in the order, the empty batch;
the literal of tests/hits_literal.py pinned to the oracle (its box and triangle tests bit for bit, its first FRONT entry bit for
bit the oracle's closest hit); the properties of the specification on the literal; and what the shared ray sets must contain so
that the GPU tests cannot pass vacuously."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import hits_cases as hc
import hits_literal as hl
import ray_edges as R
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["count", "k", "rays", "tmax", "tmax_all", "faces", "count_all", "reserved", "t_out", "prim_out", "uv_out", "face_out", "n_out"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_hits_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_hits_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # a function is added: no new version


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaHits %zu\\n", sizeof(RaycaHits));',
             'printf("consts %u\\n", RAYCA_HITS_MAX * 100u + RAYCA_HITS_FRONT * 10u + RAYCA_HITS_BOTH);']
    for name, _ in abi.RaycaHits._fields_:
        lines.append(f'printf("RaycaHits.{name} %zu\\n", offsetof(RaycaHits, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaHits) == int(want["RaycaHits"]) == 80
    for name, _ in abi.RaycaHits._fields_:
        assert getattr(abi.RaycaHits, name).offset == int(want[f"RaycaHits.{name}"]), name
    assert int(want["consts"]) == abi.HITS_MAX * 100 + abi.HITS_FRONT * 10 + abi.HITS_BOTH == 1601


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaHits \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, names = re.match(r"(const )?(\w+)\s*(\*)?\s*([\w, ]+)$", decl).groups()
            scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
            for name in names.split(","):
                c_fields.append((name.strip(), f"*{'const' if const else 'mut'} c_void" if ptr else scalar))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaHits \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaHits._fields_] == [n for n, _ in c_fields] == FIELDS
    assert re.search(r"pub fn rayca_hip_hits_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, query: \*const RaycaHits, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)
    for line in ("pub const RAYCA_HITS_FRONT: u32 = 0;", "pub const RAYCA_HITS_BOTH: u32 = 1;", "pub const RAYCA_HITS_MAX: u32 = 16;"):
        assert line in shim


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaHits): a query that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(64)
    scene, ptr = C.cast(dummy, C.c_void_p), C.addressof(dummy)   # (ptr stands for a device pointer: nothing is launched)

    def run(o=None, scene=scene, query=True, stats=None, **fields):
        q = abi.RaycaHits()
        q.count, q.k, q.rays, q.tmax_all = 4, 3, ptr, float("inf")
        q.t_out, q.n_out = ptr, ptr
        for name, v in fields.items():
            setattr(q, name, v)
        return product_lib.rayca_hip_hits_device(scene, C.byref(o) if o is not None else None, C.byref(q) if query else None,
                                                 C.byref(stats) if stats is not None else None)
    run.ptr, run.keep = ptr, dummy
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
    assert call(rays=None) == abi.ERR_BAD_ARG and "null rays" in last_error()
    for k in (17, 64, 0xFFFFFFFF):
        assert call(k=k) == abi.ERR_BAD_ARG and "RAYCA_HITS_MAX" in last_error()
    for faces in (2, 7, 0xFFFFFFFF):
        assert call(faces=faces) == abi.ERR_BAD_ARG and "unknown faces" in last_error()
    assert call(count_all=2) == abi.ERR_BAD_ARG and "count_all must be 0 or 1" in last_error()
    assert call(reserved=1) == abi.ERR_BAD_ARG and "reserved must be zero" in last_error()
    assert call(k=0, t_out=None) == abi.ERR_BAD_ARG and "needs count_all" in last_error()
    assert call(t_out=None, n_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()
    assert call(k=0, count_all=1, t_out=None, n_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()
    for record in ("t_out", "prim_out", "uv_out", "face_out"):   # k == 0 has no entries to write: n_out alone
        fields = {"t_out": None, record: call.ptr}
        assert call(k=0, count_all=1, **fields) == abi.ERR_BAD_ARG and "no output" in last_error() and "k == 0" in last_error(), record
    for only in ("t_out", "prim_out", "uv_out", "face_out", "n_out"):   # any one output will do: the call gets as far as the options
        fields = {"t_out": None, "n_out": None, only: call.ptr}
        assert call(options(context=8), **fields) == abi.ERR_BAD_ARG and "context" in last_error(), only
    assert call(options(context=8), k=16, faces=abi.HITS_BOTH, count_all=1) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(context=8), k=0, count_all=1, t_out=None) == abi.ERR_BAD_ARG and "context" in last_error()


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1)
    chain = [({"rays": None}, "null rays"), ({"k": 17}, "RAYCA_HITS_MAX"), ({"faces": 9}, "unknown faces"), ({"count_all": 3}, "count_all"),
             ({"reserved": 5}, "reserved"), ({"t_out": None, "n_out": None}, "no output")]
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), chain[k][1]
    # k == 0 without count_all stands in front of the outputs, and both in front of the options
    assert call(bad_opts, k=0, t_out=None, n_out=None) == abi.ERR_BAD_ARG and "needs count_all" in last_error()
    assert call(bad_opts, k=0, reserved=1) == abi.ERR_BAD_ARG and "reserved" in last_error()
    assert call(bad_opts, k=0, count_all=1) == abi.ERR_BAD_ARG and "no output" in last_error()       # (t_out is given: a record output)
    assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_BAD_ARG and "engine" in last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), count=0) == abi.OK   # (the empty batch returns before the scene is read)


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "multi-hit query" in last_error(), last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    """count == 0 returns RAYCA_OK behind the struct's and the options' checks, without a look at the scene (here: 64 bytes of
    zeros) or the device (there is none), and zeroes the statistics it is handed."""
    assert call(count=0) == abi.OK
    assert call(None, count=0, k=0, count_all=1, t_out=None) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.boxes_tested, st.rays_primary = 7, 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.boxes_tested == 0 and st.rays_primary == 0
    assert call(count=0, reserved=1) == abi.ERR_BAD_ARG   # (checked as for any batch)
    assert call(count=0, k=17) == abi.ERR_BAD_ARG


# ---- the literal pinned to the oracle --------------------------------------------------------------------------------------------
def c3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def test_literal_box_test_is_the_oracles():
    """hits_literal.slab against oracle_aabb_intersects (tmin, or f32::MAX for a miss) bit for bit: the soup's leaves under its
    benign rays, axis-parallel rays (a zero component misses), tiny and denormal components."""
    ref = hc.reference("soup1k")
    lib = hc.oracle("soup1k").lib
    rays = np.concatenate([hc.soup_rays()[::37], R.family("soup1k", "axis")[::41]])
    leaves = np.arange(0, ref.lo.shape[0], 3)
    ok, tmin = hl.slab(ref.lo[None, leaves], ref.hi[None, leaves], rays[:, None, :3], rays[:, None, 3:])
    accepted = 0
    for i, r in enumerate(rays):
        for j, leaf in enumerate(leaves):
            want = np.float32(lib.oracle_aabb_intersects(c3(ref.lo[leaf]), c3(ref.hi[leaf]), c3(r[:3]), c3(r[3:])))
            got = tmin[i, j] if ok[i, j] else hl.FLT_MAX
            assert bits(np.float32(got)) == bits(want), (i, leaf, got, want)
            accepted += bool(ok[i, j])
    assert 50 < accepted < rays.shape[0] * leaves.size - 50


@pytest.mark.parametrize("name", ["soup1k", "cornell"])
def test_literal_triangle_test_is_the_oracles(name):
    """hits_literal.tri_test against oracle_scene_primitive_intersects, verdict, t and (u, v) bit for bit"""
    ref, orc = hc.reference(name), hc.oracle(name)
    rays = hc.rays_for(name)[::9]
    ranks = np.arange(ref.tris.shape[0])
    tr = ref.tris[ranks]
    ok, t, u, v, _ = hl.tri_test(tr[None, :, 0], tr[None, :, 1], tr[None, :, 2], rays[:, None, :3], rays[:, None, 3:])
    hits = 0
    tt, uv = C.c_float(), (C.c_float * 2)()
    cand = np.argwhere(ok | (np.arange(ok.size).reshape(ok.shape) % 29 == 0))   # every accepted pair and some of the others
    for i, j in cand:
        got = orc.lib.oracle_scene_primitive_intersects(orc.handle, int(ref.flat[ranks[j]]), c3(rays[i, :3]), c3(rays[i, 3:]), C.byref(tt), uv)
        assert got == int(ok[i, j]), (i, j)
        if got:
            hits += 1
            assert bits(np.float32(tt.value)) == bits(t[i, j]) and bits(np.float32(uv[0])) == bits(u[i, j]) and bits(np.float32(uv[1])) == bits(v[i, j]), (i, j)
    assert hits > 40


def golden_rays(name):
    if name == "soup1k":
        return np.load(os.path.join(R.G, "soup1k_rays.npz"))["rays"].astype(np.float32)[:1024]
    return hc.rays_for(name)


@pytest.mark.parametrize("name", ["soup1k", "box", "cornell", "twoblas", "spheres"])
def test_literal_first_front_entry_is_the_oracles_closest_hit(name):
    """FRONT, k = 1, unbounded: t, prim (as a rank: the oracle's own numbering), (u, v) bit for bit oracle_trace_rays' record,
    on the committed soup rays and on the other scenes' ray sets -- leaves, ties and spheres included."""
    rays = golden_rays(name)
    t, rank, uv, face, n = hl.hits(hc.reference(name), rays, 1)
    ot, oprim, ouv, _ = hc.oracle(name).trace_rays(rays)
    finite = np.isfinite(rays).all(1)
    same = (bits(t[:, 0]) == bits(ot)) & (rank[:, 0] == oprim) & (bits(uv[:, 0]) == bits(ouv)).all(1)
    assert same[finite].all(), np.flatnonzero(~same & finite)[:8]
    assert np.array_equal(n > 0, oprim != hl.NONE) or not finite.all()
    assert (oprim != hl.NONE).sum() > rays.shape[0] // 4 and not face.any()


# ---- properties of the specification, on the literal ---------------------------------------------------------------------------
def test_louvre_lists_are_the_analytic_ones():
    rays = hc.louvre_rays(256)
    ref = hc.reference("louvre")
    for faces, ts in (("front", np.arange(0, 40, 2) + 1.0), ("both", np.arange(40) + 1.0)):
        t, rank, uv, face, total = hl.all_hits(ref, rays, None, faces)
        assert (total == ts.size).all()
        m = min(ts.size, hl.K_MAX)
        assert np.array_equal(t[:, :m], np.broadcast_to(ts[:m].astype(np.float32), (256, m)))   # t = i + 1 exactly
        assert np.array_equal(face[:, :m], np.broadcast_to((np.arange(m) % 2 if faces == "both" else np.zeros(m)).astype(np.uint8), (256, m)))
        assert (rank[:, :m] != hl.NONE).all() and (np.diff(t[:, :m].astype(np.float64), axis=1) > 0).all()
        # bounded: exactly the hits in front of the bound, which is strict
        for bound, count in ((1.0, 0), (1.5, 1), (5.0, 2 if faces == "front" else 4), (np.nextafter(np.float32(5), np.float32(6)), 3 if faces == "front" else 5)):
            tb = hl.all_hits(ref, rays[:8], bound, faces)
            assert (tb[4] == count).all(), (faces, bound)
            assert np.array_equal(tb[0][:, :count], t[:8, :count]) and (tb[0][:, count:] == hl.FLT_MAX).all() and (tb[1][:, count:] == hl.NONE).all()
    # from behind the odd quads show their front
    back = hc.rays_for("louvre")[256:384]
    t, _, _, face, total = hl.all_hits(ref, back, None, "front")
    assert (total == 20).all() and np.array_equal(t[:, :3], np.broadcast_to(np.float32([1, 3, 5]), (128, 3)))


@pytest.mark.parametrize("name", ["coplanar", "soup1k"])
def test_prefix_property_and_n(name):
    """the first k entries of the call with k' > k are the call with k; n = min(hits, k), or all of them with count_all"""
    ref, rays = hc.reference(name), hc.rays_for(name)[::3]
    for faces in ("front", "both"):
        big = hl.hits(ref, rays, 16, None, faces)
        total = hl.hits(ref, rays, 0, None, faces, count_all=True)[4]
        for k in (1, 3, 8):
            small = hl.hits(ref, rays, k, None, faces)
            for a, b in zip(small[:4], big[:4]):
                assert np.array_equal(bits(a), bits(b[:, :k])) if a.dtype != np.uint8 else np.array_equal(a, b[:, :k])
            assert np.array_equal(small[4], np.minimum(total, k)) and np.array_equal(hl.hits(ref, rays, k, None, faces, count_all=True)[4], total)
            unused = np.arange(k)[None] >= small[4][:, None]
            assert (small[0][unused] == hl.FLT_MAX).all() and (small[1][unused] == hl.NONE).all() and not small[2][unused].any() and not small[3][unused].any()
            assert (small[1][~unused] != hl.NONE).all()


def test_ties_are_ordered_by_rank_and_k_cuts_through_a_group():
    """The doubled quads: every hit on them is an exact tie of two or four primitives.  Within a group the ranks ascend, and a k
    that ends inside a group keeps its lowest ranks."""
    ref, rays = hc.reference("coplanar"), hc.rays_for("coplanar")
    t, rank, uv, face, total = hl.all_hits(ref, rays, None, "front")
    valid = rank != hl.NONE
    tie = valid[:, 1:] & valid[:, :-1] & (t[:, 1:] == t[:, :-1])
    assert tie.sum() > 500
    assert (rank[:, 1:][tie].astype(np.int64) > rank[:, :-1][tie].astype(np.int64)).all()
    assert (t[:, 1:][valid[:, 1:]] >= t[:, :-1][valid[:, 1:]]).all()
    cut = np.flatnonzero(tie[:, 0])          # entries 0 and 1 tie: k = 1 ends inside the group
    assert cut.size > 100
    one = hl.hits(ref, rays[cut], 1)
    assert np.array_equal(one[1][:, 0], rank[cut, 0]) and (rank[cut, 0] < rank[cut, 1]).all()
    cut3 = np.flatnonzero(tie[:, 2] & (total > 3))   # entries 2 and 3 tie: k = 3
    assert cut3.size > 0 and np.array_equal(hl.hits(ref, rays[cut3], 3)[1], rank[cut3, :3])


@pytest.mark.parametrize("name", ["louvre", "cornell", "soup1k"])
def test_uv_of_both_faces_reconstructs_the_hit_point(name):
    """(u, v) are the weights of vertex 0 and vertex 1 on either face: u v0 + v v1 + (1 - u - v) v2 is the point o + d t, to the
    tolerance test_nearest_cpu.py holds its points to -- 13 x 2^-24 x the largest coordinate involved -- on each axis, with the
    conditioning of this problem on top: the ray's point carries the rounding of t times |d|."""
    ref, rays = hc.reference(name), hc.rays_for(name)
    t, rank, uv, face, total = hl.all_hits(ref, rays, None, "both")
    i, e = np.nonzero(rank != hl.NONE)
    assert face[i, e].sum() > 50 and (face[i, e] == 0).sum() > 50
    tri = ref.tris[rank[i, e]].astype(np.float64)
    keep = ~ref.sphere[rank[i, e]]
    u, v = uv[i, e, 0].astype(np.float64), uv[i, e, 1].astype(np.float64)
    p_uv = u[:, None] * tri[:, 0] + v[:, None] * tri[:, 1] + (1 - u - v)[:, None] * tri[:, 2]
    o, d = rays[i, :3].astype(np.float64), rays[i, 3:].astype(np.float64)
    p_ray = o + d * t[i, e].astype(np.float64)[:, None]
    big = np.maximum(np.abs(tri).max((1, 2)), np.maximum(np.abs(o).max(1), np.abs(d).max(1) * t[i, e]))
    tol = 13 * 2.0 ** -24 * big
    err = np.abs(p_uv - p_ray).max(1)
    assert (err[keep] <= tol[keep]).all(), (float((err / tol)[keep].max()), int((err > tol)[keep].sum()))


def test_dead_rays_have_no_hits():
    ref = hc.reference("louvre")
    rays = hc.louvre_rays(8)
    for tmax, n in ((None, 20), (np.inf, 20), (hl.FLT_MAX, 20), (0.0, 0), (-3.0, 0), (np.nan, 0), (-np.inf, 0)):
        assert (hl.all_hits(ref, rays, tmax)[4] == n).all(), tmax
    for bad in (np.nan, np.inf, -np.inf):
        for c in range(6):
            r = rays.copy()
            r[:, c] = bad
            t, rank, uv, face, total = hl.all_hits(ref, r, None, "both")
            assert not total.any() and (t == hl.FLT_MAX).all() and (rank == hl.NONE).all() and not uv.any() and not face.any()
    per_ray = hl.all_hits(ref, rays[:4], np.float32([3.5, 1.0, np.nan, np.inf]), "both")
    assert per_ray[4].tolist() == [3, 0, 0, 40]
    zero = rays.copy()          # a direction component of exactly zero: the reference's boxes are all missed
    zero[:, 3:5] = 0
    assert not hl.all_hits(ref, zero, None, "both")[4].any()


# ---- what the shared ray sets must contain -----------------------------------------------------------------------------------
def test_soup_rays_have_long_lists_and_ties():
    """so that k = 3 and k = 8 cut lists short on the GPU, and the tie rule is exercised where nothing is constructed to tie"""
    rays = hc.soup_rays()
    assert rays.shape[0] <= 4096
    t, rank, _, _, total = hl.all_hits(hc.reference("soup1k"), rays, None, "both")
    assert (total > 3).sum() >= 50 and (total > 8).sum() >= 3, ((total > 3).sum(), (total > 8).sum())
    valid = rank != hl.NONE
    tie = valid[:, 1:] & (t[:, 1:] == t[:, :-1])
    assert tie.any(1).sum() >= 5
    front = hl.all_hits(hc.reference("soup1k"), rays, None, "front")[4]
    assert (front > 3).sum() >= 10


@pytest.mark.parametrize("name", hc.SCENES)
def test_every_scene_exercises_what_it_is_there_for(name):
    rays = hc.rays_for(name)
    assert 0 < rays.shape[0] <= 4096
    sets = hc.tmax_sets(name, rays)
    none = hc.full_lists(name, "main", rays, "none", None, "both")
    per = hc.full_lists(name, "main", rays, "per_ray", sets["per_ray"], "both")
    assert (none[4] > 0).sum() > rays.shape[0] // 5
    cut = (per[4] < none[4]).sum()           # a boundary exactly on a hit's t removes that hit
    assert cut > 50, cut
    if name == "spheres":
        assert hc.reference(name).sphere.sum() == 3 and hc.reference(name).sphere[none[1][none[1] != hl.NONE]].sum() > 100


# ---- the same refusals from C++ ---------------------------------------------------------------------------------------------------
def test_stand_alone_refusal_program(product_lib):
    """tests/cpp/hits_refusals.cpp against the library as built: the program DESIGN 4.17's sanitizer run links against a build
    whose host code is instrumented."""
    import __graft_entry__ as g
    exe = g.build_cpp_host("hits_refusals")
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
