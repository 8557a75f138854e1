"""rayca_hip_gather_device without a GPU: the symbol, the layout of RaycaGather in all three descriptions of the ABI (the header, the
ctypes mirror, the Rust shim), the refusals that need no scene with their messages and their order, the empty batch; and the
properties of the specification as tests/gather_literal.py restates it (a constant radiance folds to itself, kept counts the finite
samples alone, inactive points, the nine basis functions against their closed forms, the host's helpers)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import gather_literal as gl
from rayca_amd import Config, IntegratorStrategy, abi, scenes
from rayca_amd.ambient import cosine_directions, sh9_basis, sh9_irradiance, sphere_directions
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["count", "samples", "points", "normals", "rotations", "dirs", "weights", "dir_count", "dir_first", "bias", "sample", "first_index",
          "chunk_points", "reserved", "irradiance_out", "sh_out", "kept_out", "samples_out"]
OUTPUTS = ("irradiance_out", "sh_out", "kept_out", "samples_out")


def f32(*x):
    return np.array(x, np.float32)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_gather_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_gather_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # no layout changed: no new version


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaGather %zu\\n", sizeof(RaycaGather));']
    for name, _ in abi.RaycaGather._fields_:
        lines.append(f'printf("RaycaGather.{name} %zu\\n", offsetof(RaycaGather, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaGather) == int(want["RaycaGather"]) == 112
    for name, _ in abi.RaycaGather._fields_:
        assert getattr(abi.RaycaGather, name).offset == int(want[f"RaycaGather.{name}"]), name
    # no padding anywhere: two words, five pointers, eight words, four pointers
    assert [getattr(abi.RaycaGather, n).offset for n in FIELDS] == [0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 80, 88, 96, 104]


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaGather \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name, _, n = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)(\[(\d+)\])?$", decl).groups()
            scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else (f"[{scalar}; {n}]" if n else scalar)))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaGather \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaGather._fields_] == [n for n, _ in c_fields] == FIELDS
    assert re.search(r"pub fn rayca_hip_gather_device\(scene: \*mut RaycaScene, cfg: \*const RaycaConfig, opts: \*const RaycaRenderOptions, "
                     r"gather: \*const RaycaGather, stats_out: \*mut RaycaStats\) -> i32;", shim)


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaGather): a call that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it."""
    dummy = C.create_string_buffer(64 + 16)
    ptr = (C.addressof(dummy) + 15) & ~15                             # (stands for a device pointer: nothing is launched)
    scene = C.c_void_p(ptr)

    def run(o=None, scene=scene, struct=True, stats=None, cfg=Config(), **fields):
        g = abi.RaycaGather()
        g.count, g.samples, g.points, g.normals, g.dirs, g.dir_count, g.irradiance_out = 4, 16, ptr, ptr, ptr, 16, ptr
        for name, v in fields.items():
            if name == "reserved":
                g.reserved[0], g.reserved[1] = v
            else:
                setattr(g, name, v)
        c = cfg.to_abi() if cfg is not None else None
        return product_lib.rayca_hip_gather_device(scene, C.byref(c) if c is not None else None, C.byref(o) if o is not None else None,
                                                   C.byref(g) if struct else None, C.byref(stats) if stats is not None else None)
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
    assert call(cfg=None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert call(struct=False) == abi.ERR_BAD_ARG and "null" in last_error()
    for field in ("points", "normals", "dirs"):
        assert call(**{field: None}) == abi.ERR_BAD_ARG and f"null {field}" in last_error(), field
    for samples in (0, 65, 0xFFFFFFFF):
        assert call(samples=samples, dir_count=0xFFFFFFFF) == abi.ERR_BAD_ARG and "samples" in last_error() and "64" in last_error()
    # dir_first + samples > dir_count, computed without overflow
    for first, count in ((1, 16), (0, 15), (17, 16), (0xFFFFFFF8, 16), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert call(dir_first=first, dir_count=count) == abi.ERR_BAD_ARG and "dir_count" in last_error(), (first, count)
    assert call(o=options(context=8), dir_first=0xFFFFFFEF, dir_count=0xFFFFFFFF) == abi.ERR_BAD_ARG and "context" in last_error()   # (fits exactly)
    for reserved in ((1, 0), (0, 1)):
        assert call(reserved=reserved) == abi.ERR_BAD_ARG and "reserved must be zero" in last_error()
    assert call(irradiance_out=None) == abi.ERR_BAD_ARG and "no output" in last_error()
    for only in OUTPUTS:   # any one of the four will do: the call gets as far as the options
        assert call(options(context=8), **{"irradiance_out": None, only: call.ptr}) == abi.ERR_BAD_ARG and "context" in last_error(), only
    for field in ("irradiance_out", "sh_out", "samples_out"):
        for off in (4, 8, 12):
            assert call(**{field: call.ptr + off}) == abi.ERR_BAD_ARG and field in last_error() and "16-byte aligned" in last_error(), (field, off)
    assert call(options(context=8), kept_out=call.ptr + 4) == abi.ERR_BAD_ARG and "context" in last_error()   # (u32: 4-byte alignment will do)
    for bias in (float("nan"), float("inf"), float("-inf")):
        assert call(bias=bias) == abi.ERR_BAD_ARG and "bias" in last_error()
    # first_index + count x S <= 2^32 and count x S <= 2^31
    for count, samples, first in (((1 << 31) // 64 + 1, 64, 0), (0x80000001, 1, 0), (0xFFFFFFFF, 2, 0)):
        assert call(count=count, samples=samples, dir_count=64, first_index=first) == abi.ERR_BAD_ARG and "2^3" in last_error(), (count, samples)
    assert call(count=4, samples=16, first_index=0xFFFFFFFF - 62) == abi.ERR_BAD_ARG and "first_index" in last_error() and "2^32" in last_error()
    assert call(count=0x80000001, samples=1) == abi.ERR_BAD_ARG and "2^31" in last_error()
    assert call(options(context=8), count=4, samples=16, first_index=0xFFFFFFFF - 63) == abi.ERR_BAD_ARG and "context" in last_error()   # the last index is 2^32 - 1
    assert call(options(context=8), count=1 << 31, samples=1) == abi.ERR_BAD_ARG and "context" in last_error()                         # 2^31 rays are allowed
    assert call(options(context=8), count=1 << 25, samples=64, dir_count=64, first_index=1 << 31) == abi.ERR_BAD_ARG and "context" in last_error()


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)
    bad_cfg = Config(integrator=7, light_samples=0, gamma=2.2)
    # (each marker is in the message of its own rule alone: "samples", say, is also in the dir_count and the 2^32 messages)
    chain = [({"points": None}, "null points"), ({"normals": None}, "null normals"), ({"dirs": None}, "null dirs"), ({"samples": 65}, "1 .. 64 samples"),
             ({"dir_first": 9}, "exceeds dir_count"), ({"reserved": (0, 5)}, "reserved must be zero"), ({"irradiance_out": None}, "no output"),
             ({"sh_out": call.ptr + 4}, "sh_out must be 16-byte aligned"), ({"bias": float("nan")}, "bias is not finite"),
             ({"first_index": 0xFFFFFFFF}, "first_index + count x samples exceeds 2^32")]
    reported = []
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        if "samples" in fields and k > 3:
            del fields["samples"]   # (everything behind it needs a legal sample count to be reached)
        if k == 6:
            del fields["sh_out"]    # (a misaligned sh_out is an output: "no output" needs all four NULL)
        assert call(bad_opts, cfg=bad_cfg, **fields) == abi.ERR_BAD_ARG, (chain[k][1], last_error())
        reported.append(last_error())
        assert chain[k][1] in reported[-1], (chain[k][1], reported[-1])
        assert not any(marker in reported[-1] for j, (_, marker) in enumerate(chain) if j != k), (chain[k][1], reported[-1])
    assert len(set(reported)) == len(chain)
    # the last struct-level rule, behind first_index + count x S: count x S above 2^31 (first_index 0, so the rule before it holds)
    assert call(bad_opts, cfg=bad_cfg, count=0x80000001, samples=1) == abi.ERR_BAD_ARG and "count x samples exceeds 2^31" in last_error()
    assert call(bad_opts, cfg=bad_cfg, count=0x80000001, samples=1, first_index=0x80000000) == abi.ERR_BAD_ARG and "exceeds 2^32" in last_error()
    # 2. the Config's values, 3. the options
    assert call(bad_opts, cfg=bad_cfg) == abi.ERR_BAD_ARG and "integrator" in last_error()
    assert call(bad_opts, cfg=Config(light_samples=0, gamma=2.2)) == abi.ERR_BAD_ARG and "light_samples" in last_error()
    assert call(bad_opts, cfg=Config(gamma=2.2, russian_roulette=True)) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE), cfg=Config(gamma=2.2)) == abi.ERR_BAD_ARG and "engine" in last_error()
    # 4. RAYCA_ERR_UNSUPPORTED: the traversal, the Config's gaps, gamma -- the empty batch returns behind them, before the scene is read
    gaps = Config(gamma=2.2, russian_roulette=True)
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), cfg=gaps, count=0) == abi.ERR_UNSUPPORTED and "traversal" in last_error() and "exhaustive" in last_error()
    assert call(cfg=gaps, count=0) == abi.ERR_UNSUPPORTED and "russian_roulette" in last_error()
    for cfg, field in ((Config(integrator=IntegratorStrategy.Raytracer), "integrator"), (Config(direct_sampler=2), "direct_sampler"),
                       (Config(max_depth=3, light_samples=2), "light_samples")):
        assert call(cfg=cfg, count=0) == abi.ERR_UNSUPPORTED and f"RaycaConfig.{field}" in last_error(), (field, last_error())
    for gamma in (2.2, 0.0, float("nan"), 1.0000001):
        assert call(cfg=Config(gamma=gamma), count=0) == abi.ERR_UNSUPPORTED and "RaycaConfig.gamma" in last_error(), gamma
    assert call(cfg=Config(gamma=1.0), count=0) == abi.OK


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "gather call" in last_error(), last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    """count == 0 returns RAYCA_OK behind the structs' and the options' checks, without a look at the scene (here: 64 bytes of
    zeros) or the device (there is none), and zeroes the statistics it is handed."""
    assert call(count=0) == abi.OK
    assert call(None, count=0, samples=64, dir_count=64, irradiance_out=None, samples_out=call.ptr, cfg=Config(integrator=IntegratorStrategy.Flat)) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.rays_primary = 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0, first_index=0xFFFFFFFF, chunk_points=3) == abi.OK
    assert st.kernel_launches == 0 and st.rays_primary == 0
    assert call(count=0, reserved=(1, 0)) == abi.ERR_BAD_ARG   # (checked as for any batch)


# ---- the literal: the fold ---------------------------------------------------------------------------------------------------
def unit_vectors(n=20_000, seed=611):
    """hashed unit vectors (f64, rounded to f32) plus the poles and the axes"""
    u = scenes.hash_unit(seed, np.arange(2 * n, dtype=np.uint32)).astype(np.float64).reshape(n, 2)
    z, phi = 2.0 * u[:, 0] - 1.0, 2.0 * np.pi * u[:, 1]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    v = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return np.concatenate([v, np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float64)]).astype(np.float32)


@pytest.mark.parametrize("samples", [1, 2, 4, 8, 16, 32, 64])
def test_a_constant_radiance_folds_to_itself(samples):
    """S a power of two and an L of at most 18 significant bits: every partial sum j * L (j <= 64: six more bits) and the division
    by S are exact, so E == L to the bit.  (A full 24-bit L cannot do this in any order: 3 L already rounds.)  H[0] sums the rounded
    product L * Y0, a full-width value, so it is checked against the same loop, not against a closed form."""
    m, e = np.frexp(np.array([0.7310586, 3.1415927, 1e-3, 1.0]))
    value = np.ldexp(np.round(m * 2.0 ** 18) / 2.0 ** 18, e).astype(np.float32)
    assert (np.frexp(value)[0] * 2.0 ** 18 % 1 == 0).all()
    L = np.broadcast_to(value, (3, samples, 4)).copy()
    d = np.broadcast_to(f32(0, 0, 1), (3, samples, 3))
    E, sh, kept, out = gl.fold(L, np.ones(3, bool), d, samples)
    assert E.dtype == np.float32 and sh.dtype == np.float32 and kept.dtype == np.uint32
    assert np.array_equal(E[:, :3], np.broadcast_to(value[:3], (3, 3))) and (E[:, 3] == 1.0).all() and (kept == samples).all()
    acc = np.zeros(3, np.float32)
    for _ in range(samples):
        acc = acc + value[:3] * np.float32(0.2820948)
    assert np.array_equal(sh[:, 0, :3], np.broadcast_to(acc / np.float32(samples), (3, 3))) and not sh[..., 3].any()
    assert sh[:, 2, :3].all() and sh[:, 6, :3].all() and not sh[:, [1, 3, 4, 5, 7, 8]].any()   # d = +z: only the functions of z alone
    assert np.array_equal(out, L)


def test_kept_counts_the_finite_samples_alone():
    L = np.ones((4, 5, 4), np.float32)
    L[0, 1, 0] = np.nan                     # one channel is enough
    L[0, 3, 2] = np.inf
    L[1, :, 1] = -np.inf                    # every sample of point 1
    L[2, 4, 3] = np.nan                     # alpha is not looked at
    L[3, 0, :3] = [2.0, 4.0, 6.0]
    d = np.broadcast_to(f32(0, 0, 1), (4, 5, 3))
    E, sh, kept, out = gl.fold(L, np.ones(4, bool), d, 5)
    assert kept.tolist() == [3, 0, 5, 5]
    assert np.array_equal(E[0], f32(1, 1, 1, np.float32(3) / np.float32(5)))        # the mean of the three that count
    assert not E[1].any() and not sh[1].any()                                         # all out: zeros, not NaN
    assert np.array_equal(E[2], f32(1, 1, 1, 1))
    assert np.array_equal(E[3, :3], f32(6, 8, 10) / np.float32(5))
    assert np.array_equal(out.view(np.uint32), L.view(np.uint32))                     # samples_out is the radiance itself, NaN and all
    all_nan = np.full((2, 7, 4), np.nan, np.float32)
    E, sh, kept, _ = gl.fold(all_nan, np.ones(2, bool), np.zeros((2, 7, 3), np.float32), 7)
    assert not E.any() and not sh.any() and not kept.any() and np.isfinite(E).all() and np.isfinite(sh).all()


def test_inactive_points_give_zeros():
    L = np.full((3, 4, 4), 0.5, np.float32)
    d = np.broadcast_to(f32(0.6, 0, 0.8), (3, 4, 3))
    act = gl.active(f32([0, 0, 0], [1, 2, 3], [np.inf, 0, 0]), f32([0, 0, 1], [0, -0.0, 0], [0, 0, 1]))
    assert act.tolist() == [True, False, False]
    E, sh, kept, out = gl.fold(L, act, d, 4)
    assert kept.tolist() == [4, 0, 0] and E[0].tolist() == [0.5, 0.5, 0.5, 1.0] and not E[1:].any() and not sh[1:].any() and sh[0].any()
    assert np.array_equal(out[0], L[0]) and not out[1:].any() and not np.signbit(out[1:]).any()


def test_the_order_of_the_sum_and_the_weights():
    d = np.broadcast_to(f32(0, 0, 1), (1, 3, 3))
    L = np.zeros((1, 3, 4), np.float32)
    L[0, :, 0] = [2.0 ** 24, 1, 1]                      # each 1 is lost on its own; 1 + 1 first would survive
    assert gl.fold(L, np.ones(1, bool), d, 3)[0][0, 0] == np.float32(2.0 ** 24) / np.float32(3)
    L[0, :, 0] = [1, 1, 2.0 ** 24]
    assert gl.fold(L, np.ones(1, bool), d, 3)[0][0, 0] == np.float32(2.0 ** 24 + 2) / np.float32(3)
    L[0, :, :3] = [[1, 2, 3], [10, 20, 30], [100, 200, 300]]
    w = f32(0.5, 2.0, 0.25)
    E, sh, kept, out = gl.fold(L, np.ones(1, bool), d, 3, weights=w)
    assert np.array_equal(E[0, :3], f32(45.5, 91, 136.5) / np.float32(3)) and kept[0] == 3
    assert np.array_equal(out, L)                                                     # the weights are the fold's, not the samples'
    y2 = np.float32(0.4886025)                                                        # Y2 at the pole
    assert np.array_equal(sh[0, 2, :3], ((f32(0.5, 1, 1.5) * y2 + f32(20, 40, 60) * y2) + f32(25, 50, 75) * y2) / np.float32(3))
    assert not sh[0, [1, 3, 4, 5, 7, 8]].any()                                        # x = y = 0


def test_basis_against_closed_forms():
    """Y_k in f32, operation by operation, against the float64 closed forms: 2.6e-7 at worst on such a set (the constants carry seven
    digits, the polynomials two or three roundings of values <= 1.1); asserted below 1e-6.  And orthonormal on a large stratified
    set: the Gram matrix of the nine functions against the identity."""
    v = unit_vectors()
    y = gl.basis(v)
    assert y.dtype == np.float32 and y.shape == (v.shape[0], 9)
    x, yy, z = (v.astype(np.float64)[:, k] for k in range(3))
    pi = np.pi
    closed = np.stack([np.full(x.shape, 0.5 * np.sqrt(1 / pi)), np.sqrt(3 / (4 * pi)) * yy, np.sqrt(3 / (4 * pi)) * z, np.sqrt(3 / (4 * pi)) * x,
                       0.5 * np.sqrt(15 / pi) * x * yy, 0.5 * np.sqrt(15 / pi) * yy * z, 0.25 * np.sqrt(5 / pi) * (3 * z * z - 1),
                       0.5 * np.sqrt(15 / pi) * x * z, 0.25 * np.sqrt(15 / pi) * (x * x - yy * yy)], 1)
    worst = np.abs(y.astype(np.float64) - closed).max()
    print(f"basis: worst deviation {worst:.3g}")
    assert worst < 1e-6
    assert np.abs(sh9_basis(v) - closed).max() < 1e-12
    grid = sphere_directions(4096).astype(np.float64)
    gram = 4 * pi * (sh9_basis(grid)[:, :, None] * sh9_basis(grid)[:, None, :]).mean(0)
    assert np.abs(gram - np.eye(9)).max() < 2e-3


def test_tables_and_sh9_irradiance():
    for n in (1, 5, 16, 64):
        t = sphere_directions(n)
        assert t.shape == (n, 3) and t.dtype == np.float32 and np.abs(np.linalg.norm(t.astype(np.float64), axis=1) - 1).max() < 1e-6
    t = sphere_directions(64).astype(np.float64)
    assert np.abs(t.mean(0)).max() < 1e-6 and (t[:, 2] > 0).sum() == 32                # balanced: uniform over both hemispheres
    # a constant environment L: its projection is L * 4 pi * Y0 in band 0 and nothing else; the irradiance is pi L for every normal
    L = np.array([0.25, 1.0, 3.0])
    n = unit_vectors(500)
    sh = np.zeros((9, 3))
    sh[0] = L * 4 * np.pi * 0.28209479177387814
    assert np.abs(sh9_irradiance(sh, n) - np.pi * L).max() < 1e-12
    # ... and through the literal's fold: sphere_directions, weights of 4 pi, a constant radiance
    S = 64
    table = sphere_directions(S)
    Lr = np.broadcast_to(np.array([0.25, 1.0, 3.0, 1.0], np.float32), (1, S, 4))
    _, d = gl.rays(f32([0, 0, 0]), f32([0, 0, 1]), None, table, S, 0.0)
    _, coeff, kept, _ = gl.fold(Lr, np.ones(1, bool), d, S, weights=np.full(S, 4 * np.pi, np.float32))
    assert kept[0] == S
    assert np.abs(sh9_irradiance(coeff[0, :, :3], n) - np.pi * L).max() < 0.02 * np.pi * L.max()   # 64 strata: bands 1, 2 cancel to a percent
    # a sky that is 1 above the horizon and black below: bands 0 and 1 give pi / 2 each at the pole, band 2 nothing (the integral of
    # 3 z^2 - 1 over a hemisphere is 0): E(up) = pi, E(down) = pi / 2 - pi / 2 = 0
    up = (table[:, 2] > 0).astype(np.float32)
    sky = np.concatenate([up[:, None] * np.array([1, 1, 1], np.float32), np.ones((S, 1), np.float32)], 1)[None]
    _, coeff, _, _ = gl.fold(sky, np.ones(1, bool), d, S, weights=np.full(S, 4 * np.pi, np.float32))
    e_up, e_down = sh9_irradiance(coeff[0, :, :3], f32(0, 0, 1))[0], sh9_irradiance(coeff[0, :, :3], f32(0, 0, -1))[0]
    assert abs(e_up - np.pi) < 0.05 * np.pi and abs(e_down) < 0.05 * np.pi, (e_up, e_down)
    assert cosine_directions(16).shape == sphere_directions(16).shape
