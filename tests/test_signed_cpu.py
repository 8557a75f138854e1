"""rayca_hip_signed_device without a GPU: the symbol, the layout of RaycaSigned in all three descriptions of the ABI (the header,
the ctypes mirror, the Rust shim), the refusals that need no scene with their messages and their order, the empty batch; and the
properties of the specification as tests/signed_literal.py restates it, on the closed meshes of tests/signed_cases.py against
their analytic insides."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import signed_cases as sc
import signed_literal as sl
from rayca_amd import abi
from rayca_amd.lib import last_error
from rayca_amd.signed import SIGN_DIRECTIONS, checked_directions, checked_grid, grid_points, sign_directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FIELDS = ["count", "source", "points", "radius", "radius_all", "rule", "n_dirs", "reserved", "grid_origin", "grid_step", "grid_dims", "dirs",
          "dist2_out", "prim_out", "point_out", "uv_out", "inside_out", "votes_out", "cross_out"]
DIRS3 = sign_directions(3)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_signed_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_signed_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # no layout changed: no new version


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaSigned %zu\\n", sizeof(RaycaSigned));',
             'printf("consts %d\\n", RAYCA_SIGNED_POINTS * 1000 + RAYCA_SIGNED_GRID * 100 + RAYCA_SIGNED_PARITY * 10 + RAYCA_SIGNED_WINDING);']
    for name, _ in abi.RaycaSigned._fields_:
        lines.append(f'printf("RaycaSigned.{name} %zu %zu\\n", offsetof(RaycaSigned, {name}), sizeof(((RaycaSigned*)0)->{name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.strip().splitlines()}
    assert C.sizeof(abi.RaycaSigned) == want["RaycaSigned"][0] == 192
    for name, _ in abi.RaycaSigned._fields_:
        f = getattr(abi.RaycaSigned, name)
        assert [f.offset, f.size] == want[f"RaycaSigned.{name}"], name
    assert want["consts"][0] == abi.SIGNED_POINTS * 1000 + abi.SIGNED_GRID * 100 + abi.SIGNED_PARITY * 10 + abi.SIGNED_WINDING == 101


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaSigned \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name, dims = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)((?:\[\d+\])*)$", decl).groups()
            rtype = f"*{'const' if const else 'mut'} c_void" if ptr else {"uint32_t": "u32", "float": "f32"}[ctype]
            for n in reversed(re.findall(r"\[(\d+)\]", dims)):   # float dirs[5][3] is [[f32; 3]; 5]
                rtype = f"[{rtype}; {n}]"
            c_fields.append((name, rtype))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaSigned \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaSigned._fields_] == [n for n, _ in c_fields] == FIELDS
    assert dict(c_fields)["dirs"] == "[[f32; 3]; 5]" and dict(c_fields)["grid_dims"] == "[u32; 3]"
    assert re.search(r"pub fn rayca_hip_signed_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, query: \*const RaycaSigned, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)
    for line in ("pub const RAYCA_SIGNED_POINTS: u32 = 0;", "pub const RAYCA_SIGNED_GRID: u32 = 1;", "pub const RAYCA_SIGNED_PARITY: u32 = 0;",
                 "pub const RAYCA_SIGNED_WINDING: u32 = 1;"):
        assert line in shim, line


def test_selftest_knows_the_picker(product_lib):
    """rayca_hip_selftest walks every kernel picker, k_signed's 32 instantiations among them (needs no device)"""
    from rayca_amd import lib
    lib.check(product_lib.rayca_hip_selftest())
    assert "pick_signed_kernel(near, cull, grid, fast, stats)" in open(os.path.join(ROOT, "rayca_amd", "csrc", "select.inc")).read()


# ---- the refusals that need no scene, and their order -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call(product_lib):
    """call(options | None, **fields of RaycaSigned): a query that passes every check unless a field says otherwise.  The scene
    handle is any non-NULL value: every refusal here stands in front of the first look at it.  dirs: an (n, 3) array; grid_dims:
    a 3-tuple."""
    dummy = C.create_string_buffer(64)
    scene, ptr = C.cast(dummy, C.c_void_p), C.addressof(dummy)   # (ptr stands for a device pointer: nothing is launched)

    def run(o=None, scene=scene, query=True, stats=None, dirs=DIRS3, grid_dims=None, **fields):
        q = abi.RaycaSigned()
        q.count, q.source, q.points, q.radius_all, q.rule, q.n_dirs = 4, abi.SIGNED_POINTS, ptr, float("inf"), abi.SIGNED_PARITY, 3
        q.inside_out = ptr
        for j, d in enumerate(np.asarray(dirs, F)):
            for a in range(3):
                q.dirs[j][a] = float(d[a])
        if grid_dims is not None:
            for a in range(3):
                q.grid_dims[a] = grid_dims[a]
        for name, v in fields.items():
            setattr(q, name, v)
        return product_lib.rayca_hip_signed_device(scene, C.byref(o) if o is not None else None, C.byref(q) if query else None,
                                                   C.byref(stats) if stats is not None else None)
    run.keep = dummy
    return run


def options(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


def bad_dirs(j, a, v):
    d = sign_directions(5)
    d[j, a] = v
    return d


def test_struct_level_refusals_with_their_messages(call):
    assert call(scene=None) == abi.ERR_BAD_ARG and "null scene" in last_error()
    assert call(query=False) == abi.ERR_BAD_ARG and "null" in last_error()
    for source in (2, 9, 0xFFFFFFFF):
        assert call(source=source) == abi.ERR_BAD_ARG and "unknown source" in last_error()
    assert call(points=None) == abi.ERR_BAD_ARG and "null points" in last_error()
    grid = dict(source=abi.SIGNED_GRID, points=None)
    assert call(count=0, **grid, grid_dims=(2, 3, 4)) == abi.ERR_BAD_ARG and "nx * ny * nz" in last_error()   # (an empty batch is checked like any other)
    assert call(count=24, **grid, grid_dims=(2, 3, 4), o=options(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()   # a GRID needs no points
    for dims in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        assert call(count=0, **grid, grid_dims=dims) == abi.ERR_BAD_ARG and "dimension is zero" in last_error(), dims
    assert call(count=23, **grid, grid_dims=(2, 3, 4)) == abi.ERR_BAD_ARG and "nx * ny * nz" in last_error()
    # the product in 64 bits: 65536 x 65536 x 1 is 2^32, not 0; 2^16 x 2^16 x 2^16 is 2^48, not 0; 4294967295 x 1 x 1 passes
    assert call(count=0, **grid, grid_dims=(65536, 65536, 1)) == abi.ERR_BAD_ARG and "nx * ny * nz" in last_error()
    assert call(count=0, **grid, grid_dims=(65536, 65536, 65536)) == abi.ERR_BAD_ARG and "nx * ny * nz" in last_error()
    assert call(count=0, **grid, grid_dims=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == abi.ERR_BAD_ARG and "nx * ny * nz" in last_error()
    assert call(count=0xFFFFFFFF, **grid, grid_dims=(0xFFFFFFFF, 1, 1), o=options(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()
    for rule in (2, 7, 0xFFFFFFFF):
        assert call(rule=rule) == abi.ERR_BAD_ARG and "unknown rule" in last_error()
    for n in (0, 2, 4, 6, 7, 0xFFFFFFFF):
        assert call(n_dirs=n) == abi.ERR_BAD_ARG and "1, 3 or 5" in last_error(), n
    for n in (1, 3, 5):
        assert call(options(context=8), n_dirs=n, dirs=sign_directions(5)) == abi.ERR_BAD_ARG and "context" in last_error(), n
    for v in (0.0, -0.0, np.nan, np.inf, -np.inf):
        for j, a in ((0, 0), (1, 2), (2, 1)):
            assert call(dirs=bad_dirs(j, a, v)) == abi.ERR_BAD_ARG and "zero, NaN or infinite" in last_error(), (v, j, a)
        # a direction that is not used is not read
        assert call(options(context=8), dirs=bad_dirs(3, 1, v)) == abi.ERR_BAD_ARG and "context" in last_error(), v
        assert call(n_dirs=5, dirs=bad_dirs(4, 2, v)) == abi.ERR_BAD_ARG and "zero, NaN or infinite" in last_error(), v
    assert call(reserved=1) == abi.ERR_BAD_ARG and "reserved must be zero" in last_error()
    assert call(inside_out=None) == abi.ERR_BAD_ARG and "no sign output" in last_error()
    assert call(inside_out=None, dist2_out=C.addressof(call.keep)) == abi.ERR_BAD_ARG and "nearest-point query" in last_error()   # the distance outputs alone
    for only in ("inside_out", "votes_out", "cross_out"):   # any one of the three will do: the call gets as far as the options
        fields = {"inside_out": None, only: C.addressof(call.keep)}
        assert call(options(context=8), **fields) == abi.ERR_BAD_ARG and "context" in last_error(), only


def test_refusals_come_in_the_documented_order(call):
    """Each call breaks one rule and every rule behind it: the first one broken is the one reported."""
    bad_opts = options(context=8, engine=1)
    chain = [({"source": 5}, "unknown source"), ({"points": None}, "null points"), ({"rule": 9}, "unknown rule"), ({"n_dirs": 4}, "1, 3 or 5"),
             ({"dirs": bad_dirs(0, 1, 0.0)}, "zero, NaN or infinite"), ({"reserved": 5}, "reserved"), ({"inside_out": None}, "no sign output")]
    for k in range(len(chain)):
        fields = {}
        for f, _ in chain[k:]:
            fields.update(f)
        assert call(bad_opts, **fields) == abi.ERR_BAD_ARG and chain[k][1] in last_error(), chain[k][1]
    # the grid's rules stand where the points' rule stands
    behind = {"rule": 9, "n_dirs": 4, "reserved": 5, "inside_out": None}
    assert call(bad_opts, source=abi.SIGNED_GRID, grid_dims=(0, 1, 1), **behind) == abi.ERR_BAD_ARG and "dimension is zero" in last_error()
    assert call(bad_opts, source=abi.SIGNED_GRID, grid_dims=(3, 1, 1), **behind) == abi.ERR_BAD_ARG and "nx * ny * nz" in last_error()
    assert call(bad_opts, source=abi.SIGNED_GRID, count=3, grid_dims=(3, 1, 1), **behind) == abi.ERR_BAD_ARG and "unknown rule" in last_error()
    assert call(bad_opts) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(engine=1, traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_BAD_ARG and "engine" in last_error()
    # behind the options: the empty batch returns before the scene is read, under either traversal
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE), count=0) == abi.OK


def test_options_that_do_not_apply_are_refused(call):
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call(options(**{field: 1})) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error() and "signed query" in last_error(), last_error()
    assert call(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()


def test_empty_batch_is_ok_and_launches_nothing(call):
    """count == 0 returns RAYCA_OK behind the struct's and the options' checks, without a look at the scene (here: 64 bytes of
    zeros) or the device (there is none), and zeroes the statistics it is handed."""
    assert call(count=0) == abi.OK
    assert call(None, count=0, rule=abi.SIGNED_WINDING, n_dirs=5, dirs=sign_directions(5)) == abi.OK
    st = abi.RaycaStats()
    st.kernel_launches, st.boxes_tested, st.rays_primary = 7, 7, 7
    assert call(options(collect_stats=1, context=7), stats=st, count=0) == abi.OK
    assert st.kernel_launches == 0 and st.boxes_tested == 0 and st.rays_primary == 0
    assert call(count=0, reserved=1) == abi.ERR_BAD_ARG   # (checked as for any batch)


# ---- the wrapper's inputs (no device) ---------------------------------------------------------------------------------------------
def test_sign_directions():
    d = sign_directions(5)
    assert d.dtype == F and d.shape == (5, 3) and np.array_equal(d, SIGN_DIRECTIONS)
    assert np.array_equal(d[:3], F([[0.5370, 0.6914, 0.4837], [-0.6533, 0.2706, 0.7071], [0.2113, -0.7887, -0.5774]]))
    assert (d != 0).all() and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-3
    unit = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    cos = unit @ unit.T - np.eye(5)
    assert np.abs(cos).max() < 0.8, "no two are parallel or opposite"
    for n in (1, 3, 5):
        assert np.array_equal(sign_directions(n), d[:n]) and np.array_equal(checked_directions(n), d[:n])
    for n in (0, 2, 4, 6, True, 3.0):
        with pytest.raises(ValueError):
            sign_directions(n)
    d[0, 0] = 9   # a copy: the table stays
    assert SIGN_DIRECTIONS[0, 0] == F(0.5370)
    for bad in (np.ones((2, 3)), np.ones((3, 2)), np.ones(3), [[1, 0, 1]], [[1, np.nan, 1]], [[1, np.inf, 1]]):
        with pytest.raises(ValueError):
            checked_directions(bad)
    assert np.array_equal(checked_directions([[1, 2, -3]]), F([[1, 2, -3]]))
    for bad in (None, (1, 2), ((0, 0), (1, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (2, 0, 2)), ((0, 0, 0), (1, 1, 1), (65536, 65536, 1))):
        with pytest.raises(ValueError):
            checked_grid(bad)
    assert checked_grid(((0, 0, 0), (1, 1, 1), (65535, 65537, 1)))[3] == 0xFFFFFFFF


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
GRIDS = [((-1.0, -0.7, 0.3), (0.1, 0.2, 0.3), (1, 1, 1)), ((-1.0, -0.7, 0.3), (0.1, 0.2, 0.3), (5, 3, 2)), ((0.1, -3.3, 1e-3), (0.03, 0.7, -0.11), (67, 9, 3)),
         ((1000.1, -1000.7, 3.3), (1 / 3, 1e-3, 7.7), (130, 2, 2))]


@pytest.mark.parametrize("grid", GRIDS)
def test_grid_points(grid):
    origin, step, dims = grid
    p = sl.grid_points(origin, step, dims)
    nx, ny, nz = dims
    assert p.dtype == F and p.shape == (nx * ny * nz, 3)
    # an independent f32 restatement: three loops, x fastest, the product and the sum each rounded to f32
    o32, s32 = [F(x) for x in origin], [F(x) for x in step]
    want = np.array([[o32[0] + F(F(ix) * s32[0]), o32[1] + F(F(iy) * s32[1]), o32[2] + F(F(iz) * s32[2])]
                     for iz in range(nz) for iy in range(ny) for ix in range(nx)], F)
    assert np.array_equal(p.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(grid_points(origin, step, dims).view(np.uint32), want.view(np.uint32))   # the package's own helper
    # against origin + i * step in f64: two roundings, of the product and of the sum
    i = np.arange(nx * ny * nz)
    index = np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], 1).astype(np.float64)
    exact = np.array(o32, np.float64) + index * np.array(s32, np.float64)
    prod = np.abs(index * np.array(s32, np.float64))
    bound = 2.0 ** -24 * prod + 2.0 ** -24 * (np.abs(exact) + 2.0 ** -24 * prod) * (1 + 2.0 ** -23)   # half an ulp each
    assert (np.abs(p.astype(np.float64) - exact) <= bound * (1 + 1e-6)).all()


# ---- the rules and the vote ---------------------------------------------------------------------------------------------------------
def test_vote_on_hand_made_counts():
    front = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 2, 2], [0, 2, 1]], np.uint32)
    back = np.array([[0, 0, 0], [0, 0, 0], [0, 2, 1], [2, 2, 2], [1, 1, 1], [1, 3, 1]], np.uint32)
    votes, inside = sl.vote(front, back, sl.PARITY)
    assert votes.tolist() == [0, 1, 0b111, 0b111, 0b111, 0b011] and inside.tolist() == [0, 0, 1, 1, 1, 1]
    votes, inside = sl.vote(front, back, sl.WINDING)
    assert votes.tolist() == [0, 0, 0b110, 0b111, 0, 0b011] and inside.tolist() == [0, 0, 1, 1, 0, 1]
    for n in (1, 5):   # a strict majority of 1 and of 5
        f = np.zeros((6, n), np.uint32)
        b = (np.arange(n)[None, :] < np.arange(6)[:, None]).astype(np.uint32)
        votes, inside = sl.vote(f, b, sl.WINDING)
        pop = np.minimum(np.arange(6), n)
        assert votes.tolist() == [(1 << k) - 1 for k in pop] and inside.tolist() == [int(2 * k > n) for k in pop]


# ---- the closed meshes against their analytic insides ----------------------------------------------------------------------------
def sign_of(name, points, rule, n_dirs=3):
    return sc.cached(("sign", name, points.tobytes(), rule, n_dirs), lambda: sl.sign(sc.reference(name), points, sign_directions(n_dirs), sl.RULES[rule]))


@pytest.mark.parametrize("rule", ["parity", "winding"])
def test_torus_against_the_analytic_torus(rule):
    points = sc.torus_points()
    dist = sc.torus_distance(points)
    keep, share = sc.surface_share(dist)
    inside, votes, cross = sign_of("torus", points, rule)
    print(f"torus, {rule}: {share:.3f} of {points.shape[0]} points within {sc.BAND} of the surface; {(dist < 0).sum()} inside")
    assert 0.03 < share and 300 < (dist[keep] < 0).sum()
    assert np.isin(votes[keep], (0, 7)).all(), "every compared point is unanimous"
    assert np.array_equal(inside[keep], (dist[keep] < 0).astype(np.uint8))
    assert cross.shape == (points.shape[0], 3, 2) and cross.max() <= 4   # a line meets a torus at most four times


def test_two_boxes_rules_differ_exactly_in_the_overlap():
    points = sc.box_points()
    da, db = sc.box_distance(points, sc.BOX_A), sc.box_distance(points, sc.BOX_B)
    keep, share = sc.surface_share(np.minimum(np.abs(da), np.abs(db)))
    in_a, in_b = da < 0, db < 0
    par, par_votes, _ = sign_of("two_boxes", points, "parity")
    win, win_votes, _ = sign_of("two_boxes", points, "winding")
    print(f"two_boxes: {share:.3f} within {sc.BAND} of a face; {(in_a & in_b)[keep].sum()} of {keep.sum()} in the overlap")
    assert (in_a & in_b)[keep].sum() > 20 and (in_a ^ in_b)[keep].sum() > 200
    assert np.isin(par_votes[keep], (0, 7)).all() and np.isin(win_votes[keep], (0, 7)).all()
    assert np.array_equal(win[keep], (in_a | in_b)[keep].astype(np.uint8))     # the union
    assert np.array_equal(par[keep], (in_a ^ in_b)[keep].astype(np.uint8))     # parity calls the overlap outside
    assert np.array_equal((par != win)[keep], (in_a & in_b)[keep])


def test_shell_cavity_is_outside_under_both_rules():
    points = sc.box_points(2000, 41)
    do, di = sc.box_distance(points, sc.SHELL_OUTER), sc.box_distance(points, sc.SHELL_INNER)
    keep, share = sc.surface_share(np.minimum(np.abs(do), np.abs(di)))
    solid = (do < 0) & (di > 0)
    assert (di < 0)[keep].sum() > 50 and solid[keep].sum() > 300
    for rule in ("parity", "winding"):
        inside, votes, _ = sign_of("shell", points, rule)
        assert np.isin(votes[keep], (0, 7)).all()
        assert np.array_equal(inside[keep], solid[keep].astype(np.uint8)), rule
        assert not inside[keep & (di < 0)].any()


def test_holed_torus_shows_disagreement_in_votes():
    points = sc.torus_points(1500, 43)
    inside, votes, _ = sign_of("holed", points, "parity")
    whole = sign_of("torus", points, "parity")
    split = ~np.isin(votes, (0, 7))
    print(f"holed: {split.sum()} of {points.shape[0]} points with votes neither 0 nor all ones")
    assert split.any(), "a ray through the hole loses a crossing: the directions disagree"
    assert (votes != whole[1]).any() and (votes == whole[1]).sum() > 0.9 * points.shape[0]


def test_nonfinite_points_have_all_zero_sign_outputs():
    points = sc.torus_points(9, 47).copy()
    points[:, :] = (0.6, 0.0, 0.0)                                # inside the tube
    for k in range(1, 9):
        points[k, (k - 1) % 3] = [np.nan, np.inf, -np.inf][(k - 1) % 3] if k < 7 else np.nan
    for rule in ("parity", "winding"):
        inside, votes, cross = sl.sign(sc.reference("torus"), points, sign_directions(5), sl.RULES[rule])
        assert inside[0] == 1 and votes[0] == 31
        assert not inside[1:].any() and not votes[1:].any() and not cross[1:].any()


def test_consequences_front_and_both_counts():
    """front_j is the FRONT count of the ray (p, dirs[j]), front_j + back_j the BOTH count: what the GPU test's composition uses"""
    import hits_literal as hl
    points = sc.torus_points(200, 53)
    _, _, cross = sl.sign(sc.reference("torus"), points, sign_directions(5), sl.PARITY)
    for j, d in enumerate(sign_directions(5)):
        rays = np.concatenate([points, np.broadcast_to(d, points.shape)], 1).astype(F)
        assert np.array_equal(cross[:, j, 0], hl.hits(sc.reference("torus"), rays, 0, None, "front", True)[4])
        assert np.array_equal(cross[:, j].sum(1), hl.hits(sc.reference("torus"), rays, 0, None, "both", True)[4])


def test_distance_part_is_the_nearest_literal():
    """signed() hands the distance part to nearest_literal.closest: on the torus the distance agrees with the analytic one to
    within the distance between the mesh and the torus (signed_cases.facet_error)"""
    import nearest_literal as nl
    points = sc.torus_points(400, 59)
    tris = sc.flat_triangles("torus")
    got = sl.signed(sc.reference("torus"), tris, points, DIRS3, sl.PARITY, radius=0.5)
    want = nl.closest(tris, points, 0.5)
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    facet, h1, h2 = sc.facet_error("torus", 24, 12)
    hit = got[1] != nl.NONE
    assert 0 < hit.sum() < hit.size
    err = np.abs(np.sqrt(got[0][hit].astype(np.float64)) - np.abs(sc.torus_distance(points[hit])))
    print(f"torus 24 x 12: mesh and torus lie up to {facet:.4f} apart ({h1:.4f} mesh to torus, {h2:.4f} torus to mesh); "
          f"|mesh distance - analytic| up to {err.max():.4f}")
    # (5 % for the sampling of the two maxima; 1e-6 for the f32 of the literal at distances below 2)
    assert err.max() <= 1.05 * facet + 1e-6 and facet < sc.BAND
