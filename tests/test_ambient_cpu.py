"""rayca_hip_ambient_device without a GPU: the symbol, the layout of RaycaAmbient in all three descriptions of the ABI (the header,
the ctypes mirror, the Rust shim), the refusals that need no scene with their messages and their order, the empty batch; the
properties of the specification as tests/ambient_literal.py restates it (the frame on 200 000 hashed unit normals plus the poles and
axes, the inactive rule, the fold); a closed room on the CPU oracle; and the check that the inputs of test_gpu_ambient.py
(tests/ambient_cases.py) leave both answers common enough for its comparison to mean something."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ambient_cases as ac
import ambient_literal as al
import ray_edges as R
from rayca_amd import Config, Mesh, Model, Node, PbrMaterial, Primitive, Scene, abi, flatten, scenes
from rayca_amd.ambient import cosine_directions, pixel_rotations
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["count", "samples", "points", "normals", "rotations", "radius", "dirs", "dir_count", "dir_first", "radius_all", "bias", "reserved",
          "mask_out", "hits_out", "open_out", "bent_out"]


def f32(*x):
    return np.array(x, np.float32)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_ambient_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_ambient_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # no layout changed: no new version


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaAmbient %zu\\n", sizeof(RaycaAmbient));']
    for name, _ in abi.RaycaAmbient._fields_:
        lines.append(f'printf("RaycaAmbient.{name} %zu\\n", offsetof(RaycaAmbient, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaAmbient) == int(want["RaycaAmbient"]) == 104
    for name, _ in abi.RaycaAmbient._fields_:
        assert getattr(abi.RaycaAmbient, name).offset == int(want[f"RaycaAmbient.{name}"]), name
    assert abi.RaycaAmbient.mask_out.offset == 72   # (reserved at 64, four bytes of padding in front of the pointers)


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaAmbient \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)$", decl).groups()
            scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else scalar))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaAmbient \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaAmbient._fields_] == [n for n, _ in c_fields] == FIELDS
    assert re.search(r"pub fn rayca_hip_ambient_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, ambient: \*const RaycaAmbient, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaAmbient): a call that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(64)
    scene, ptr = C.cast(dummy, C.c_void_p), C.addressof(dummy)   # (ptr stands for a device pointer: nothing is launched)
    assert ptr % 8 == 0

    def run(o=None, scene=scene, struct=True, stats=None, **fields):
        a = abi.RaycaAmbient()
        a.count, a.samples, a.points, a.normals, a.dirs, a.dir_count, a.radius_all, a.open_out = 4, 16, ptr, ptr, ptr, 16, float("inf"), ptr
        for name, v in fields.items():
            setattr(a, name, v)
        return product_lib.rayca_hip_ambient_device(scene, C.byref(o) if o is not None else None, C.byref(a) if struct else None,
                                                    C.byref(stats) if stats is not None else None)
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
    assert call(scene=None) == abi.ERR_BAD_ARG and "null scene" in last_error()
    assert call(struct=False) == abi.ERR_BAD_ARG and "null" in last_error()
    for field in ("points", "normals", "dirs"):
        assert call(**{field: None}) == abi.ERR_BAD_ARG and f"null {field}" in last_error(), field
    for samples in (0, 65, 0xFFFFFFFF):
        assert call(samples=samples, dir_count=0xFFFFFFFF) == abi.ERR_BAD_ARG and "samples" in last_error() and "64" in last_error()
    # dir_first + samples > dir_count, computed without overflow
    for first, count in ((1, 16), (0, 15), (17, 16), (0xFFFFFFF8, 16), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert call(dir_first=first, dir_count=count) == abi.ERR_BAD_ARG and "dir_count" in last_error(), (first, count)
    assert call(o=options(context=8), dir_first=0xFFFFFFEF, dir_count=0xFFFFFFFF) == abi.ERR_BAD_ARG and "context" in last_error()   # (fits exactly)
    assert call(reserved=1) == abi.ERR_BAD_ARG and "reserved must be zero" in last_error()
    assert call(open_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()
    for only in ("mask_out", "hits_out", "open_out", "bent_out"):   # any one of the four will do: the call gets as far as the options
        assert call(options(context=8), **{"open_out": None, only: call.ptr}) == abi.ERR_BAD_ARG and "context" in last_error(), only
    assert call(mask_out=call.ptr + 4) == abi.ERR_BAD_ARG and "aligned" in last_error()
    for bias in (float("nan"), float("inf"), float("-inf")):
        assert call(bias=bias) == abi.ERR_BAD_ARG and "bias" in last_error()
    for count, samples in ((1 << 26, 64), (0xFFFFFFFF, 2), (0x80000000, 2)):
        assert call(count=count, samples=samples, dir_count=64) == abi.ERR_BAD_ARG and "2^32" in last_error()
    assert call(o=options(context=8), count=0xFFFFFFFF, samples=1) == abi.ERR_BAD_ARG and "context" in last_error()   # 2^32 - 1 rays are allowed


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)
    chain = [({"points": None}, "null points"), ({"normals": None}, "null normals"), ({"dirs": None}, "null dirs"), ({"samples": 65}, "samples"),
             ({"dir_first": 9}, "dir_count"), ({"reserved": 5}, "reserved"), ({"open_out": None}, "no output"), ({"bias": float("nan")}, "bias"),
             ({"count": 0xFFFFFFFF}, "2^32")]
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        if "samples" in fields and k > 3:
            del fields["samples"]   # (count x samples needs a legal sample count to be reached)
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), (chain[k][1], last_error())
    assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_BAD_ARG and "engine" in last_error()
    # behind the options: EXHAUSTIVE has no form (the empty batch returns behind it, before the scene is read)
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), count=0) == abi.ERR_UNSUPPORTED and "exhaustive" in last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_UNSUPPORTED


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "ambient call" in last_error(), last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    """count == 0 returns RAYCA_OK behind the struct's and the options' checks, without a look at the scene (here: 64 bytes of
    zeros) or the device (there is none), and zeroes the statistics it is handed."""
    assert call(count=0) == abi.OK
    assert call(None, count=0, samples=64, dir_count=64, mask_out=call.ptr) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.rays_shadow = 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.rays_shadow == 0
    assert call(count=0, reserved=1) == abi.ERR_BAD_ARG   # (checked as for any batch)


# ---- the literal: frame and directions -------------------------------------------------------------------------------------------
def unit_normals():
    """200 000 hashed unit normals (f64, rounded to f32) plus the poles, the axes and normals a hair off the poles"""
    n = 200_000
    u = scenes.hash_unit(501, np.arange(2 * n, dtype=np.uint32)).astype(np.float64).reshape(n, 2)
    z, phi = 2.0 * u[:, 0] - 1.0, 2.0 * np.pi * u[:, 1]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    v = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    special = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 0, -0.0], [0, 1, -0.0], [-0.0, -0.0, 1]]
    for eps in (1e-3, 1e-5, 1e-7):
        for s in (1.0, -1.0):
            special += [[eps, 0, s * np.sqrt(1 - eps * eps)], [0, -eps, s * np.sqrt(1 - eps * eps)], [eps * 0.6, eps * 0.8, s * np.sqrt(1 - eps * eps)]]
    return np.concatenate([v, np.array(special, np.float64)]).astype(np.float32)


def dot(a, b):
    return (a.astype(np.float64) * b.astype(np.float64)).sum(-1)


def test_frame_is_orthonormal():
    """T.T - 1, B.B - 1, T.B, T.n, B.n: 2.2e-7 at worst on such a set (f32 normals are unit to 1e-7 themselves); asserted below 1e-6."""
    n = unit_normals()
    t, b = al.frame(n)
    assert t.dtype == np.float32 and b.dtype == np.float32 and np.isfinite(t).all() and np.isfinite(b).all()
    worst = max(np.abs(dot(t, t) - 1).max(), np.abs(dot(b, b) - 1).max(), np.abs(dot(t, b)).max(), np.abs(dot(t, n)).max(), np.abs(dot(b, n)).max())
    print(f"frame: worst deviation {worst:.3g}")
    assert worst < 1e-6
    # right-handed: T x B = n
    assert np.abs(np.cross(t.astype(np.float64), b.astype(np.float64)) - n).max() < 1e-6


def test_directions_are_unit_and_stay_in_the_hemisphere():
    """|d| against 1: 2.9e-7 at worst; d.n - lz: -2.3e-7 at worst; no NaN.  Asserted: 1e-6, d.n >= lz - 1e-6, none."""
    n = unit_normals()
    table = cosine_directions(64)
    assert table.dtype == np.float32 and table.shape == (64, 3) and np.abs(np.linalg.norm(table.astype(np.float64), axis=1) - 1).max() < 1e-6
    rng = np.random.default_rng(11)
    angle = rng.uniform(0, 2 * np.pi, n.shape[0])
    rot = np.stack([np.cos(angle), np.sin(angle)], 1).astype(np.float32)
    p = rng.uniform(-3, 3, n.shape).astype(np.float32)
    worst_len, worst_dn = 0.0, 0.0
    for j in range(64):
        for r in (rot, None):
            o, d = al.ambient_ray(p, n, r, table, j, 0.0)
            assert d.dtype == np.float32 and not np.isnan(d).any()
            assert np.array_equal(o, p)                      # bias 0: p + n * 0
            worst_len = max(worst_len, np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max())
            worst_dn = min(worst_dn, (dot(d, n) - np.float64(table[j, 2])).min())
    print(f"directions: | |d| - 1 | <= {worst_len:.3g}, d.n - lz >= {worst_dn:.3g}")
    assert worst_len < 1e-6 and worst_dn >= -1e-6


def test_poles_and_signed_zero():
    """n.z = -1 exactly: sg = -1, a = 1/2 -- no division by zero; n.z = -0.0 compares >= 0: sg = 1, a = -1."""
    t, b = al.frame(f32(0, 0, -1))
    assert np.array_equal(t, f32(1, 0, 0)) and np.array_equal(b, f32(0, -1, 0))
    t, b = al.frame(f32(0, 0, 1))
    assert np.array_equal(t, f32(1, 0, 0)) and np.array_equal(b, f32(0, 1, 0))
    t, b = al.frame(f32(1, 0, -0.0))
    assert np.isfinite(t).all() and np.isfinite(b).all() and np.array_equal(t, f32(0, 0, -1)) and np.array_equal(np.abs(b), f32(0, 1, 0))
    t, b = al.frame(f32(0.6, 0.8, -0.0))
    assert np.isfinite(t).all() and np.isfinite(b).all()
    _, d = al.ambient_ray(f32(0, 0, 0)[None], f32(0, 0, -1)[None], None, f32(0, 0, 1)[None], 0, 0.0)
    assert np.array_equal(d[0], f32(0, 0, -1))             # the table's pole is the normal
    o, _ = al.ambient_ray(f32(1, 2, 3)[None], f32(0, 0, -1)[None], None, f32(0, 0, 1)[None], 0, 0.5)
    assert np.array_equal(o[0], f32(1, 2, 2.5))


def test_every_clause_of_the_inactive_rule():
    p, n = f32(1, 2, 3), f32(0, 0.6, 0.8)
    assert al.active(p, n)
    assert not al.active(p, f32(0, 0, 0)) and not al.active(p, f32(-0.0, 0.0, -0.0))
    assert al.active(p, f32(0, 0, 1e-30)) and al.active(p, f32(0, -1e-45, 0))       # tiny and denormal are not zero
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            q, m = p.copy(), n.copy()
            q[k] = bad
            m[k] = bad
            assert not al.active(q, n) and not al.active(p, m), (k, bad)
    assert al.active(f32(0, 0, 0), n) and al.active(f32(3e38, -3e38, 0), f32(3e38, 0, 0))   # large but finite is active
    # an inactive point has every sample unoccluded, whatever the rays would have met
    d = np.ones((2, 4, 3), np.float32)
    mask, hits, opened, bent = al.fold(np.ones((2, 4), bool), np.array([False, True]), d, 4)
    assert mask.tolist() == [0, 15] and hits.tolist() == [0, 4] and opened.tolist() == [1.0, 0.0] and not bent.any()


def test_fold():
    """S = 64 uses bit 63; hits is the popcount; open = float(S - hits) / float(S); bent is the j-ordered sum of the unoccluded d."""
    occ = np.zeros((3, 64), bool)
    occ[0, 63] = True
    occ[1, [0, 5, 63]] = True
    occ[2, :] = True
    d = np.zeros((3, 64, 3), np.float32)
    d[:, :, 0] = 1.0
    mask, hits, opened, bent = al.fold(occ, np.ones(3, bool), d, 64)
    assert mask.dtype == np.uint64 and mask.tolist() == [1 << 63, (1 << 63) | 33, (1 << 64) - 1]
    assert hits.dtype == np.uint32 and hits.tolist() == [1, 3, 64]
    assert opened.dtype == np.float32 and opened.tolist() == [63 / 64, 61 / 64, 0.0]
    assert bent[:, 0].tolist() == [63.0, 61.0, 0.0]
    assert al.fold(np.array([[True, False, False]]), np.ones(1, bool), np.zeros((1, 3, 3), np.float32), 3)[2][0] == np.float32(2) / np.float32(3)
    # the order of the sum: 2^24, then 1 and 1 -- each 1 is lost on its own; 1 + 1 first would survive
    d = np.zeros((1, 3, 3), np.float32)
    d[0, :, 0] = [2.0 ** 24, 1, 1]
    assert al.fold(np.zeros((1, 3), bool), np.ones(1, bool), d, 3)[3][0, 0] == np.float32(2.0 ** 24)
    d[0, :, 0] = [1, 1, 2.0 ** 24]
    assert al.fold(np.zeros((1, 3), bool), np.ones(1, bool), d, 3)[3][0, 0] == np.float32(2.0 ** 24 + 2)
    # an occluded sample stays out of the sum
    d[0, :, 0] = [1, 2, 4]
    assert al.fold(np.array([[False, True, False]]), np.ones(1, bool), d, 3)[3][0, 0] == 5.0


def test_tables():
    for n in (1, 5, 16, 64):
        t = cosine_directions(n)
        assert t.shape == (n, 3) and t.dtype == np.float32 and (t[:, 2] > 0).all()
    t = cosine_directions(64).astype(np.float64)
    assert abs(t[:, 2].mean() - 2 / 3) < 0.01 and np.abs(t[:, :2].mean(0)).max() < 1e-6   # cosine-weighted: E[z] = 2/3; balanced about the pole
    r = pixel_rotations(7, 5)
    assert r.shape == (5, 7, 2) and r.dtype == np.float32 and np.abs((r.astype(np.float64) ** 2).sum(-1) - 1).max() < 1e-6
    assert len({tuple(x) for x in r.reshape(-1, 2).tolist()}) == 35                                  # every pixel its own angle


# ---- a closed room on the CPU oracle ----------------------------------------------------------------------------------------------
def room_scene() -> Scene:
    """The cube [-1, 1]^3 as six quads that face inward (back faces are culled: from inside, every ray meets a front face)."""
    scene = Scene("room")
    model = Model("room")
    mat = model.materials.push(PbrMaterial(color=(0.8, 0.8, 0.8, 1), roughness_factor=1.0))
    b = scenes._MeshBuilder()
    e = np.eye(3, dtype=np.float32)
    for axis in range(3):
        u, v = e[(axis + 1) % 3] * 2, e[(axis + 2) % 3] * 2          # u x v = +axis
        b.grid(-e[axis] - u / 2 - v / 2, u, v, 1, 1)                  # the wall at -1 faces +axis: inward
        b.grid(e[axis] - u / 2 - v / 2, v, u, 1, 1)                   # the wall at +1 faces -axis
    prim = model.primitives.push(Primitive(geometry=model.geometries.push(b.mesh()), material=mat))
    model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=[prim])))))
    scene.push_model(model)
    scene.push_model(scenes.create_default_model())
    return scene


def oracle_occlusion(orc, o, d, act, radius):
    """[N, S] bool: the oracle's record of every active ray under t < radius (per point [N] or one value; +inf / FLT_MAX unbounded,
    NaN or <= 0 never)"""
    n, s = o.shape[:2]
    r = np.concatenate([o, d], 2).reshape(-1, 6).copy()
    r[~np.repeat(act, s)] = [0, 0, 0, 1, 0, 0]                         # (never read below)
    t, prim, _, _ = orc.trace_rays(r)
    radius = np.broadcast_to(np.asarray(radius, np.float32), (n,))
    with np.errstate(invalid="ignore"):
        unbounded, dead = radius >= ac.FLT_MAX, ~(radius > 0)
        found = (prim != R.NONE).reshape(n, s) & (unbounded[:, None] | (t.reshape(n, s) < radius[:, None]))
    return found & ~dead[:, None] & act[:, None]


def test_closed_room_on_the_oracle():
    import oracle_lib as ol
    orc = ol.OracleScene(flatten(room_scene()), Config())
    samples = 16
    table = cosine_directions(samples)
    p = f32([0, 0, 0], [0, 0, 0], [0.5, -0.25, 0.125])
    n = f32([0, 0, 1], [0.6, 0, -0.8], [0, 1, 0])
    act = al.active(p, n)
    o, d = al.rays(p, n, None, table, samples, 0.0)
    for radius, want in ((0.99, [0, 0, None]), (np.inf, [16, 16, 16]), (ac.FLT_MAX, [16, 16, 16]), (0.0, [0, 0, 0]), (np.nan, [0, 0, 0])):
        occ = oracle_occlusion(orc, o, d, act, radius)
        mask, hits, opened, bent = al.fold(occ, act, d, samples)
        for k, w in enumerate(want):
            if w is not None:   # (a radius below the nearest wall: nothing; unbounded: every ray ends on a wall)
                assert hits[k] == w and opened[k] == np.float32(samples - w) / np.float32(samples), (radius, k, hits[k])
        if want[0] == 0:
            assert np.array_equal(bent[0], d[0].sum(0, dtype=np.float32)) or np.abs(bent[0] - d[0].astype(np.float64).sum(0)).max() < 1e-5
        if want[0] == 16:
            assert not bent.any() and (mask == (1 << 16) - 1).all()
    # the off-centre point, 0.5 from its nearest wall in x: a radius of 0.99 catches some rays and not others
    occ = oracle_occlusion(orc, o, d, act, 0.99)
    assert 0 < occ[2].sum() < samples
    orc.close()


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.SCENES)
def test_inputs_leave_both_answers(name):
    """For each scene, radius and bias test_gpu_ambient.py uses: of the active rays the oracle finds at least 10 % occluded and at
    least 10 % unoccluded.  Otherwise the GPU comparison could pass on masks that are all zero (or all one)."""
    p, n, diag = ac.points_for(name)
    act = al.active(p, n)
    assert act.sum() == ac.COUNT - len(ac.INACTIVE) and not act[ac.inactive_index()].any()
    orc = R.oracle_scene(name)
    samples = 16
    for rot in (None, ac.rotations()):
        o, d = al.rays(p, n, rot, ac.table(samples), samples, ac.bias(name))
        for what, radius in (("radius_all", ac.radius_all(name)), ("per point", ac.radius_per_point(name))):
            occ = oracle_occlusion(orc, o, d, act, radius)
            frac = float(occ[act].mean())
            print(f"{name}, {'rotated' if rot is not None else 'plain'}, {what}: {frac:.3f} of the active rays occluded")
            assert 0.10 <= frac <= 0.90, (name, what, frac)
