"""rayca_hip_probe_lookup_device without a GPU: the symbol, the layout of RaycaProbeLookup in all three descriptions of the ABI (the
header, the ctypes mirror, the Rust shim), the refusals that need no scene with their messages and their order, the empty batch; the
properties of the specification as tests/probes_literal.py restates it; two closed rooms on the CPU oracle; and the check that the
inputs of test_gpu_probes.py (tests/probes_cases.py) leave both answers common enough for its comparison to mean something."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import probes_cases as pc
import probes_literal as pl
import ray_edges as R
from rayca_amd import Config, Mesh, Model, Node, PbrMaterial, Primitive, Scene, abi, flatten, scenes
from rayca_amd.ambient import sh9_irradiance
from rayca_amd.lib import last_error
from rayca_amd.probes import ProbeGrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["count", "flags", "origin", "cell", "dims", "bias", "reserved", "points", "normals", "sh", "kept", "albedo", "base",
          "irradiance_out", "sh_out", "mask_out", "radiance_out"]
BOTH = pl.VISIBILITY | pl.NORMAL_TERM


def f32(*x):
    return np.array(x, np.float32)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_probe_lookup_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_probe_lookup_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # no layout changed: no new version
    assert (abi.PROBE_VISIBILITY, abi.PROBE_NORMAL_TERM) == (pl.VISIBILITY, pl.NORMAL_TERM) == (1, 2)


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaProbeLookup %zu\\n", sizeof(RaycaProbeLookup));',
             'printf("flags %d %d\\n", RAYCA_PROBE_VISIBILITY, RAYCA_PROBE_NORMAL_TERM);']
    for name, _ in abi.RaycaProbeLookup._fields_:
        lines.append(f'printf("RaycaProbeLookup.{name} %zu\\n", offsetof(RaycaProbeLookup, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = [l.split() for l in out.strip().splitlines()]
    assert ["flags", "1", "2"] in rows
    want = {r[0]: r[1] for r in rows if len(r) == 2}
    assert C.sizeof(abi.RaycaProbeLookup) == int(want["RaycaProbeLookup"]) == 136
    for name, _ in abi.RaycaProbeLookup._fields_:
        assert getattr(abi.RaycaProbeLookup, name).offset == int(want[f"RaycaProbeLookup.{name}"]), name
    assert abi.RaycaProbeLookup.points.offset == 56 and abi.RaycaProbeLookup.reserved.offset == 48


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaProbeLookup \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name, _, n = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)(\[(\d+)\])?$", decl).groups()
            scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else (f"[{scalar}; {n}]" if n else scalar)))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaProbeLookup \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaProbeLookup._fields_] == [n for n, _ in c_fields] == FIELDS
    assert re.search(r"pub fn rayca_hip_probe_lookup_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, lookup: \*const RaycaProbeLookup, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)
    assert "pub const RAYCA_PROBE_VISIBILITY: u32 = 1;" in shim and "pub const RAYCA_PROBE_NORMAL_TERM: u32 = 2;" in shim


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaProbeLookup): a call that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(128)
    ptr = (C.addressof(dummy) + 15) // 16 * 16                     # (stands for a device pointer: nothing is launched)
    scene = C.c_void_p(ptr)

    def run(o=None, scene=scene, struct=True, stats=None, **fields):
        a = abi.RaycaProbeLookup()
        a.count, a.flags, a.points, a.normals, a.sh, a.irradiance_out = 4, BOTH, ptr, ptr, ptr, ptr
        a.cell[:], a.dims[:] = (1.0, 1.0, 1.0), (2, 2, 2)
        for name, v in fields.items():
            if isinstance(v, tuple):
                getattr(a, name)[:] = v
            else:
                setattr(a, name, v)
        return product_lib.rayca_hip_probe_lookup_device(scene, C.byref(o) if o is not None else None, C.byref(a) if struct else None,
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
    bad = abi.ERR_BAD_ARG
    assert call(scene=None) == bad and "null scene" in last_error()
    assert call(struct=False) == bad and "null" in last_error()
    for field in ("points", "normals", "sh"):
        assert call(**{field: None}) == bad and f"null {field}" in last_error(), field
    for flags in (4, 8, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == bad and "unknown flag bits" in last_error()
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (0, 0, 0)):
        assert call(dims=dims) == bad and "zero dim" in last_error()
    for dims in ((1 << 24, 2, 1), (1 << 12, 1 << 12, 2), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1 << 16, 1 << 16, 1 << 16), (1 << 31, 2, 1)):
        assert call(dims=dims) == bad and "2^24" in last_error(), dims
    assert call(options(context=8), dims=(1 << 12, 1 << 12, 1)) == bad and "context" in last_error()   # (2^24 probes are allowed)
    for v in (0.0, -0.0, -1.0, float("nan"), float("inf")):
        for axis in range(3):
            cell = [1.0, 1.0, 1.0]
            cell[axis] = v
            assert call(cell=tuple(cell)) == bad and "cell" in last_error(), (v, axis)
    for v in (float("nan"), float("inf"), float("-inf")):
        for axis in range(3):
            origin = [0.0, 0.0, 0.0]
            origin[axis] = v
            assert call(origin=tuple(origin)) == bad and "origin" in last_error(), (v, axis)
        assert call(bias=v) == bad and "bias" in last_error()
    assert call(reserved=(1, 0)) == bad and "reserved must be zero" in last_error()
    assert call(reserved=(0, 1)) == bad and "reserved must be zero" in last_error()
    assert call(irradiance_out=None) == bad and "no output" in last_error()
    for only in ("irradiance_out", "sh_out", "mask_out"):          # any one will do: the call gets as far as the options
        assert call(options(context=8), **{"irradiance_out": None, only: call.ptr}) == bad and "context" in last_error(), only
    assert call(options(context=8), irradiance_out=None, radiance_out=call.ptr, albedo=call.ptr) == bad and "context" in last_error()
    assert call(radiance_out=call.ptr) == bad and "needs albedo" in last_error()
    for field in ("irradiance_out", "sh_out", "radiance_out", "albedo", "base", "sh"):
        for off in (4, 8):
            assert call(**{"albedo": call.ptr, field: call.ptr + off}) == bad and field in last_error() and "16-byte aligned" in last_error(), field
    assert call(mask_out=call.ptr + 2) == bad and "mask_out" in last_error() and "aligned" in last_error()
    assert call(options(context=8), mask_out=call.ptr + 4) == bad and "context" in last_error()
    for count in (1 << 29, 0xFFFFFFFF):
        assert call(count=count) == bad and "2^32" in last_error()
    assert call(options(context=8), count=(1 << 29) - 1) == bad and "context" in last_error()


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)
    chain = [({"points": None}, "null points"), ({"normals": None}, "null normals"), ({"sh": None}, "null sh"), ({"flags": 4}, "unknown flag bits"),
             ({"dims": (2, 0, 2)}, "zero dim"), ({"cell": (1.0, float("nan"), 1.0)}, "cell"), ({"origin": (float("inf"), 0.0, 0.0)}, "origin"),
             ({"bias": float("nan")}, "bias"), ({"reserved": (0, 3)}, "reserved"), ({"irradiance_out": None}, "no output"),
             ({"count": 0xFFFFFFFF}, "2^32")]
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        if k > 2 and "sh" in fields:
            del fields["sh"]
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), (chain[k][1], last_error())
    # the rules that cannot be broken together with the ones above: too many probes behind a zero dim, albedo and alignment behind "no output"
    assert call(bad_opts, dims=(1 << 24, 2, 1), cell=(0.0, 1.0, 1.0)) == abi.ERR_BAD_ARG and "2^24" in last_error()
    assert call(bad_opts, radiance_out=call.ptr + 4, count=0xFFFFFFFF) == abi.ERR_BAD_ARG and "needs albedo" in last_error()
    assert call(bad_opts, radiance_out=call.ptr + 4, albedo=call.ptr, count=0xFFFFFFFF) == abi.ERR_BAD_ARG and "16-byte" in last_error()
    assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_BAD_ARG and "engine" in last_error()
    # behind the options: EXHAUSTIVE has no form (the empty batch returns behind it, before the scene is read)
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), count=0) == abi.ERR_UNSUPPORTED and "exhaustive" in last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_UNSUPPORTED
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), flags=0) == abi.ERR_UNSUPPORTED


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "probe lookup" in last_error(), last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    """count == 0 returns RAYCA_OK behind the struct's and the options' checks, without a look at the scene (here: zeros) or the
    device (there is none), and zeroes the statistics it is handed."""
    assert call(count=0) == abi.OK
    assert call(None, count=0, flags=0, mask_out=call.ptr) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.rays_shadow = 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.rays_shadow == 0
    assert call(count=0, reserved=(1, 0)) == abi.ERR_BAD_ARG   # (checked as for any batch)


# ---- the literal ---------------------------------------------------------------------------------------------------------------
def unit_grid(dims=(4, 3, 3)):
    return pl.Grid([0, 0, 0], [1, 1, 1], dims)


def hashed_points(grid, n, seed):
    span = (np.array(grid.dims, np.float32) - 1) * grid.cell
    return (grid.origin + R._unit(seed, n, 3).astype(np.float32) * span).astype(np.float32)


def hashed_normals(n, seed):
    z = 2.0 * R._unit(seed, n)[:, 0] - 1.0
    phi = 2.0 * np.pi * R._unit(seed + 1, n)[:, 0]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)


def test_weights_are_the_trilinear_weights():
    g = pl.Grid([-1.5, 0.25, 2.0], [0.7, 1.3, 0.45], (5, 4, 3))
    p = hashed_points(g, 4000, 701)
    i0, i1, t = pl.cells(g, p)
    m, c, wt, cand = pl.corners(g, (i0, i1, t))
    assert wt.dtype == np.float32 and (wt >= 0).all() and (t >= 0).all() and (t <= 1).all()
    assert np.abs(wt.astype(np.float64).sum(1) - 1).max() < 8 * 2.0 ** -24        # eight products of three rounded factors
    # exactly the trilinear weights: the weighted corners give the point back (to the rounding of f and of the centres)
    back = (wt.astype(np.float64)[:, :, None] * c.astype(np.float64)).sum(1)
    assert np.abs(back - p).max() < 1e-5
    assert np.array_equal(cand, wt > 0) and (m < 60).all()
    # the corner order: bit 0 is x, bit 1 is y, bit 2 is z
    assert np.array_equal(m[:, 1] - m[:, 0], (i1[:, 0] - i0[:, 0])) and np.array_equal(m[:, 2] - m[:, 0], (i1[:, 1] - i0[:, 1]) * 5)
    assert np.array_equal(m[:, 4] - m[:, 0], (i1[:, 2] - i0[:, 2]) * 20)
    assert np.array_equal(c[:, 0], (g.origin + (i0.astype(np.float32) * g.cell).astype(np.float32)).astype(np.float32))


def test_positions_are_the_specifications_centres():
    g = pl.Grid([-1.5, 0.25, 2.0], [0.7, 1.3, 0.45], (5, 4, 3))
    pos = ProbeGrid(g.origin, g.cell, g.dims).positions()
    assert pos.dtype == np.float32 and pos.shape == (60, 3) and np.array_equal(pos, pc.positions(g))
    m, c, wt, _ = pl.corners(g, pl.cells(g, pos))
    k = wt.argmax(1)
    assert np.array_equal(m[np.arange(60), k], np.arange(60)) and np.array_equal(c[np.arange(60), k], pos)
    a = ProbeGrid.around([-1, 0, -1], [1, 2, 1], (5, 1, 3), margin=0.5)
    assert np.allclose(a.origin, [-1.5, 1.0, -1.5]) and np.allclose(a.cell, [0.75, 1.0, 1.5]) and a.count == 15
    with pytest.raises(ValueError):
        ProbeGrid([0, 0, 0], [1, 0, 1], (2, 2, 2))
    with pytest.raises(ValueError):
        ProbeGrid([0, 0, 0], [1, 1, 1], (2, 0, 2))


def test_constant_field_reproduces_itself():
    """Coefficients of at most 18 significant bits and weights that are multiples of 1/64 (t a multiple of 1/4): every product and
    every partial sum is exact in 24 bits, wsum is exactly 1 and H is the constant, bit for bit.  (A 24-bit constant could not: its
    products with a six-bit weight need 30 bits.)  At hashed points the same holds to rounding; E is sh9_irradiance's to rounding."""
    g = unit_grid()
    const = (np.round(R._unit(702, 9, 3) * 2.0 ** 17) / 2.0 ** 15 - 1.0).astype(np.float32)          # 18 bits in [-1, 3)
    const[0] = np.abs(const[0]) + 1.0
    sh = np.zeros((36, 9, 4), np.float32)
    sh[:, :, :3] = const
    q = np.stack(np.meshgrid(np.arange(0, 3.01, 0.25), np.arange(0, 2.01, 0.25), np.arange(0, 2.01, 0.25), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    n = hashed_normals(q.shape[0], 703)
    for flags in (0, pl.NORMAL_TERM):
        out = pl.fold(None, g, q, n, sh, flags=flags)
        if flags == 0:
            assert (out["irradiance"][:, 3] == 1.0).all() and np.array_equal(out["sh"][:, :, :3], np.broadcast_to(const, (q.shape[0], 9, 3)))
        assert np.abs(out["sh"][:, :, :3] - const).max() <= 16 * 2.0 ** -24 * 4
        want = np.maximum(sh9_irradiance(out["sh"][:, :, :3], n), 0)
        assert np.abs(out["irradiance"][:, :3] - want).max() <= 40 * 2.0 ** -24 * np.abs(const).max() * 4   # 9 terms of 3 roundings, A Y <= 4
        assert not (out["mask"] >> 16).any() or flags
    p = hashed_points(g, 2000, 704)
    out = pl.fold(None, g, p, hashed_normals(2000, 705), sh, flags=pl.NORMAL_TERM)
    assert np.abs(out["sh"][:, :, :3] - const).max() <= 16 * 2.0 ** -24 * 4


def test_affine_field_is_reproduced_with_both_flags_off():
    g = pl.Grid([-1.5, 0.25, 2.0], [0.7, 1.3, 0.45], (5, 4, 3))
    pos = pc.positions(g).astype(np.float64)
    a, b = R._unit(706, 27, 3).reshape(9, 3, 3) - 0.5, R._unit(707, 9, 3) + 1.0
    sh = np.zeros((60, 9, 4), np.float32)
    sh[:, :, :3] = np.einsum("mx,jcx->mjc", pos, a) + b
    p = hashed_points(g, 3000, 708)
    out = pl.fold(None, g, p, hashed_normals(3000, 709), sh, flags=0)
    want = np.einsum("mx,jcx->mjc", p.astype(np.float64), a) + b
    assert np.abs(out["sh"][:, :, :3] - want).max() < 2e-5 and (out["mask"] >> 8 == 0).all()
    assert np.abs(out["irradiance"][:, 3] - 1).max() < 8 * 2.0 ** -24


def test_point_at_a_probe_centre_takes_that_probe():
    g = pl.Grid([-1.5, 0.25, 2.0], [0.5, 1.25, 0.25], (5, 4, 3))       # (dyadic: f is the exact index)
    pos, sh = pc.positions(g), pc.coefficients(g)
    n = hashed_normals(60, 710)
    for flags in (0, pl.NORMAL_TERM):
        out = pl.fold(None, g, pos, n, sh, flags=flags)
        if flags == 0:                                             # one corner of weight 1: (1 * s) / 1
            assert np.array_equal(out["sh"][:, :, :3], sh[:, :, :3])
        assert np.abs(out["sh"][:, :, :3] - sh[:, :, :3]).max() <= 2 * 2.0 ** -24 * 8 and (out["sh"][:, :, 3] == 0).all()   # (1.0625 s) / 1.0625
        assert [bin(int(x) & 255).count("1") for x in out["mask"]] == [1] * 60
    # l2 = 0 there: q = 1, wb = 1.0625
    assert (pl.normal_weight(pos, n, pos) == np.float32(1.0625)).all()
    assert np.array_equal(pl.fold(None, g, pos, n, sh, flags=pl.NORMAL_TERM)["irradiance"][:, 3], np.full(60, 1.0625, np.float32))
    # with bias 0 the corner's ray is the zero ray
    _, d = pl.rays(pos, n, pl.corners(g, pl.cells(g, pos))[1], 0.0)
    wt = pl.corners(g, pl.cells(g, pos))[2]
    assert not d[wt == 1].any()


def test_axes_with_one_probe_and_clamping_outside():
    for dims in pc.DEGENERATE_DIMS:
        g = pl.Grid([0.5, -1, 2], [2, 0.5, 1], dims)
        p = f32([0.5, -1, 2], [1.25, -0.75, 2.5], [-9, 40, 2], [1e30, -1e30, 3e38])
        i0, i1, t = pl.cells(g, p)
        m, c, wt, cand = pl.corners(g, (i0, i1, t))
        for a in range(3):
            if dims[a] == 1:
                assert not i0[:, a].any() and not i1[:, a].any() and not t[:, a].any()      # f is clamped to 0: only b = 0 has weight
        assert (m < np.prod(dims)).all() and np.abs(wt.sum(1) - 1).max() < 1e-6
        assert cand.sum(1).max() <= np.prod([min(d, 2) for d in dims])
    g = pl.Grid([0, 0, 0], [1, 1, 1], (3, 3, 3))
    p = f32([-5, 1, 1], [7, 1, 1], [1, -0.001, 1], [1, 1, 1e38], [2, 2, 2], [3.4e38, -3.4e38, 0.5])
    i0, i1, t = pl.cells(g, p)
    assert i0.tolist() == [[0, 1, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 1], [1, 0, 0]]
    assert t.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1], [1, 1, 1], [1, 0, 0.5]]
    assert (i1 == np.minimum(i0 + 1, 2)).all()
    # a point outside takes the nearest boundary cell: what the clamped point inside takes
    sh = pc.coefficients(g)
    n = hashed_normals(6, 711)
    inside = np.clip(p, 0, 2).astype(np.float32)
    assert np.array_equal(pl.fold(None, g, p, n, sh, flags=0)["sh"], pl.fold(None, g, inside, n, sh, flags=0)["sh"])
    # p - g itself overflows: f = inf, clamped
    fg, fp, fn = pc.far_origin_grid()
    i0, i1, t = pl.cells(fg, fp)
    assert i0[:, 0].tolist() == [0, 0, 0] and t[0, 0] == 1.0 and 0.49 < t[1, 0] < 0.51 and t[2, 0] == 1.0


def test_invalid_probes_are_dropped():
    g = unit_grid((2, 2, 2))
    sh = pc.coefficients(g)
    p, n = f32(0.25, 0.5, 0.75)[None], f32(0, 0.6, 0.8)[None]
    full = pl.fold(None, g, p, n, sh, flags=0)
    kept = np.ones(8, np.uint32)
    kept[[1, 6]] = 0
    out = pl.fold(None, g, p, n, sh, kept=kept, flags=0)
    assert out["mask"][0] == 0xFF & ~(1 << 1 | 1 << 6) and full["mask"][0] == 0xFF
    _, _, wt, _ = pl.corners(g, pl.cells(g, p))
    assert abs(out["irradiance"][0, 3] - (1 - wt[0, 1] - wt[0, 6])) < 1e-6
    sh2 = sh.copy()
    sh2[[1, 6]] = np.nan                                           # an invalid probe's record is never read into the blend
    assert np.array_equal(pl.fold(None, g, p, n, sh2, kept=kept, flags=0)["sh"], out["sh"])
    assert np.isnan(pl.fold(None, g, p, n, sh2, flags=0)["sh"][:, :, :3]).all()     # a valid probe's NaN propagates ...
    assert (pl.fold(None, g, p, n, sh2, flags=0)["irradiance"][0, :3] == 0).all()   # ... into H; E = max(NaN, 0) = 0
    for flags in (0, BOTH):
        none = pl.fold(np.zeros((1, 8), bool), g, p, n, sh, kept=np.zeros(8, np.uint32), flags=flags, albedo=f32(1, 1, 1, 1)[None])
        assert not none["irradiance"].any() and not none["sh"].any() and none["mask"][0] == (1 << 16 if flags else 0)
        assert none["radiance"].tolist() == [[0, 0, 0, 1]]


def test_normal_term():
    p, c = np.zeros((181, 3), np.float32), np.tile(f32(0, 0, 2), (181, 1))
    ang = np.radians(np.arange(181.0))
    n = np.stack([np.sin(ang), np.zeros(181), np.cos(ang)], 1).astype(np.float32)
    n[0], n[180] = (0, 0, 1), (0, 0, -1)
    wb = pl.normal_weight(p, n, c)
    assert wb.dtype == np.float32 and wb[0] == np.float32(1.0625) and wb[180] == np.float32(0.0625)
    assert (np.diff(wb) <= 1e-7).all() and wb[90] == pytest.approx(0.3125, abs=1e-6)
    want = ((np.cos(ang) * np.abs(np.cos(ang)) + 1) / 2) ** 2 + 0.0625
    assert np.abs(wb - want).max() < 1e-6


def test_every_clause_of_the_inactive_rule():
    g = unit_grid((2, 2, 2))
    sh = pc.coefficients(g)
    p, n = f32(0.5, 0.5, 0.5), f32(0, 0.6, 0.8)
    rows_p, rows_n = [p], [n]
    for z in (f32(0, 0, 0), f32(-0.0, 0.0, -0.0)):
        rows_p.append(p)
        rows_n.append(z)
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            q, m = p.copy(), n.copy()
            q[k], m[k] = bad, bad
            rows_p += [q, p]
            rows_n += [n, m]
    rows_p.append(p)
    rows_n.append(f32(0, -1e-45, 0))                              # a denormal is not zero
    P, N = np.stack(rows_p), np.stack(rows_n)
    base = (R._unit(712, P.shape[0], 4) + 0.5).astype(np.float32)
    alb = np.ones((P.shape[0], 4), np.float32)
    out = pl.fold(np.ones((P.shape[0], 8), bool), g, P, N, sh, flags=BOTH, albedo=alb, base=base)
    dead = np.arange(1, P.shape[0] - 1)
    assert not out["irradiance"][dead].any() and not out["sh"][dead].any() and not out["mask"][dead].any()
    assert np.array_equal(out["radiance"][dead], base[dead])
    for live in (0, P.shape[0] - 1):
        assert out["mask"][live] == 0x1FFFF and out["irradiance"][live, 3] == 1.0                # all occluded: the fallback
    assert pl.fold(None, g, P, N, sh, flags=0, albedo=alb)["radiance"][dead].tolist() == [[0, 0, 0, 1]] * dead.size


def test_mask_word_and_fallback():
    g = unit_grid((2, 2, 2))
    sh = pc.coefficients(g)
    p, n = f32(0.25, 0.5, 0.75)[None], f32(0, 0.6, 0.8)[None]
    occ = np.zeros((1, 8), bool)
    occ[0, [0, 3, 7]] = True
    out = pl.fold(occ, g, p, n, sh, flags=pl.VISIBILITY)
    assert out["mask"].dtype == np.uint32 and out["mask"][0] == 0xFF | (1 | 8 | 128) << 8
    _, _, wt, _ = pl.corners(g, pl.cells(g, p))
    assert out["irradiance"][0, 3] == ((((wt[0, 1] + wt[0, 2]) + wt[0, 4]) + wt[0, 5]) + wt[0, 6])     # summed in k order
    # occlusion of a corner without weight is not recorded; all candidates occluded: the trilinear blend and bit 16
    edge = f32(0, 0.5, 0.75)[None]                                 # t.x = 0: the four corners with bx = 1 have no weight
    out = pl.fold(np.ones((1, 8), bool), g, edge, n, sh, flags=pl.VISIBILITY)
    assert out["mask"][0] == 0x55 | 0x55 << 8 | 1 << 16
    assert np.array_equal(out["sh"], pl.fold(None, g, edge, n, sh, flags=0)["sh"]) and out["irradiance"][0, 3] == 1.0
    assert pl.fold(np.ones((1, 8), bool), g, edge, n, sh, flags=0)["mask"][0] == 0x55             # without the flag occlusion is not an input
    # radiance: L = albedo * (E * (1 / pi)) + base, alpha = base's
    alb, base = f32(0.5, 0.25, 1.0, 9.0)[None], f32(0.125, 0.0, 2.0, 0.75)[None]
    out = pl.fold(None, g, p, n, sh, flags=0, albedo=alb, base=base)
    e = out["irradiance"][0, :3]
    assert np.array_equal(out["radiance"][0, :3], alb[0, :3] * (e * np.float32(0.31830987)) + base[0, :3]) and out["radiance"][0, 3] == 0.75
    assert pl.fold(None, g, p, n, sh, flags=0, albedo=alb)["radiance"][0, 3] == 1.0


# ---- two closed rooms on the CPU oracle ---------------------------------------------------------------------------------------------
def rooms_scene() -> Scene:
    """The cube [-1, 1]^3 as six quads that face inward, and a wall at x = 0 with a face to either side (back faces are culled)."""
    scene = Scene("rooms")
    model = Model("rooms")
    mat = model.materials.push(PbrMaterial(color=(0.8, 0.8, 0.8, 1), roughness_factor=1.0))
    b = scenes._MeshBuilder()
    e = np.eye(3, dtype=np.float32)
    for axis in range(3):
        u, v = e[(axis + 1) % 3] * 2, e[(axis + 2) % 3] * 2          # u x v = +axis
        b.grid(-e[axis] - u / 2 - v / 2, u, v, 1, 1)                  # the wall at -1 faces +axis: inward
        b.grid(e[axis] - u / 2 - v / 2, v, u, 1, 1)                   # the wall at +1 faces -axis
    b.grid(-e[1] - e[2], e[1] * 2, e[2] * 2, 1, 1)                    # the dividing wall, facing +x ...
    b.grid(-e[1] - e[2], e[2] * 2, e[1] * 2, 1, 1)                    # ... and facing -x
    prim = model.primitives.push(Primitive(geometry=model.geometries.push(b.mesh()), material=mat))
    model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=[prim])))))
    scene.push_model(model)
    scene.push_model(scenes.create_default_model())
    return scene


def oracle_occlusion(orc, grid, p, n, bias, kept=None):
    """[N, 8] bool: the oracle's record of every candidate corner's ray under t < 1"""
    act = pl.active(p, n)
    m, c, wt, cand = pl.corners(grid, pl.cells(grid, p), kept)
    cand &= act[:, None]
    o, d = pl.rays(p, n, c, bias)
    r = np.concatenate([o, d], 2).reshape(-1, 6).copy()
    r[~cand.reshape(-1)] = [0, 0, 0, 1, 0, 0]                       # (never read below)
    t, prim, _, _ = orc.trace_rays(r)
    return ((prim != R.NONE) & (t < np.float32(1))).reshape(-1, 8) & cand, cand


def test_two_rooms_on_the_oracle():
    import oracle_lib as ol
    orc = ol.OracleScene(flatten(rooms_scene()), Config())
    g = pl.Grid([-0.5, 0, 0], [1, 1, 1], (2, 1, 1))                 # one probe in either room
    sh = np.zeros((2, 9, 4), np.float32)
    sh[0, 0, :3], sh[1, 0, :3] = 1.0, 3.0                           # the left room is dim, the right one bright
    p = f32([-0.125, 0.25, -0.5], [0.125, 0.25, -0.5], [-0.25, 0.125, -0.25])
    n = f32([0, 1, 0], [0, 1, 0], [1, 0, 0])
    occ, cand = oracle_occlusion(orc, g, p, n, 0.0)
    assert cand[:, :2].all() and not cand[:, 2:].any()
    assert occ[:, :2].tolist() == [[False, True], [True, False], [False, True]]
    vis = pl.fold(occ, g, p, n, sh, flags=pl.VISIBILITY)
    assert vis["sh"][:, 0, 0].tolist() == [1.0, 3.0, 1.0] and vis["mask"].tolist() == [3 | 2 << 8, 3 | 1 << 8, 3 | 2 << 8]
    leak = pl.fold(None, g, p, n, sh, flags=0)
    assert leak["sh"][:, 0, 0].tolist() == [1.75, 2.25, 1.5] and (leak["mask"] == 3).all()      # without visibility light leaks through the wall
    # a point that sees no probe: the only probe stands in the other room
    one = pl.Grid([0.5, 0, 0], [1, 1, 1], (1, 1, 1))
    occ, cand = oracle_occlusion(orc, one, p[:1], n[:1], 0.0)
    assert cand[0].tolist() == [True] + [False] * 7 and occ[0, 0]
    out = pl.fold(occ, one, p[:1], n[:1], sh[1:], flags=pl.VISIBILITY)
    assert out["mask"][0] == 1 | 1 << 8 | 1 << 16 and out["sh"][0, 0, 0] == 3.0 and out["irradiance"][0, 3] == 1.0
    orc.close()


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.SCENES)
def test_inputs_leave_both_answers(name):
    """For each scene, the grid and the bias test_gpu_probes.py uses: of the candidate rays the oracle finds between 10 % and 90 %
    occluded, and the fallback is taken by at least one point and by fewer than half.  Otherwise the GPU comparison could pass on
    masks that are all zero (or all one)."""
    inp = pc.inputs_for(name)
    p, n, g = inp["points"], inp["normals"], inp["grid"]
    assert inp["count"] == 603 and g.dims == pc.DIMS and (inp["kept"] == 0).sum() >= 3
    act = pl.active(p, n)
    occ, cand = oracle_occlusion(R.oracle_scene(name), g, p, n, inp["bias"], inp["kept"])
    frac = float(occ.sum() / cand.sum())
    out = pl.fold(occ, g, p, n, inp["sh"], inp["kept"], flags=BOTH)
    fb = int((out["mask"] >> 16 & 1).sum())
    print(f"{name}: {frac:.3f} of the {int(cand.sum())} candidate rays occluded, {fb} of {int(act.sum())} points take the fallback")
    assert 0.10 <= frac <= 0.90, (name, frac)
    assert 1 <= fb < act.sum() / 2, (name, fb)
    assert np.isfinite(out["irradiance"]).all() and np.isfinite(out["sh"]).all()
