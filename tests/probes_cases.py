"""The inputs the irradiance-volume tests share (helper module; test_probes_cpu.py checks them against the oracle, test_gpu_probes.py
runs them): per scene tests/ambient_cases.py's 576 points plus points that sit where the cell rule has an edge, a 5 x 4 x 3 probe
grid over the scene's bounds, hashed coefficients, a kept array and the bias.  Everything is made from hashes of indices
(rayca_amd.scenes.hash_unit through ray_edges), nothing from a random generator's state."""
import numpy as np

import ambient_cases as ac
import probes_literal as pl
import ray_edges as R

SCENES = ac.SCENES
DIMS = (5, 4, 3)
# The grid's margin and the bias, in scene diagonals: chosen on the oracle (test_probes_cpu.py test_inputs_leave_both_answers) so that
# on every scene between 10 % and 90 % of the candidate rays are occluded and the fallback is taken by some points and by fewer
# than half.  A negative margin puts the outermost probes inside the bounds.  Box is convex and back faces are culled: a ray that
# starts inside it hits nothing, one that starts outside and ends inside always hits.  Its probes all stand inside: the points whose
# normal looks outward (every other one) are lifted out of the box, see no probe and take the fallback; the others see all eight.
MARGIN_OF_DIAG = {"box": -0.02, "cornell": -0.05, "soup1k": -0.05, "spheres": -0.05}
BIAS_OF_DIAG = {"box": 1e-3, "cornell": 1e-3, "soup1k": 1e-3, "spheres": 0.02}
DEGENERATE_DIMS = [(1, 1, 1), (2, 1, 1), (1, 3, 1)]
FLT_MAX = np.float32(3.4028234663852886e38)


def grid_for(name, dims=DIMS):
    """the grid of `dims` whose outermost probes stand the scene's margin outside its bounds (an axis of one probe: the middle)"""
    lo, hi, _, diag = R.bounds(name)
    margin = MARGIN_OF_DIAG[name] * diag
    lo, hi = lo - margin, hi + margin
    d = np.array(dims)
    cell = np.where(d > 1, (hi - lo) / np.maximum(d - 1, 1), 1.0)
    origin = np.where(d > 1, lo, 0.5 * (lo + hi))
    return pl.Grid(origin.astype(np.float32), cell.astype(np.float32), dims)


def far_origin_grid():
    """(grid, points, normals): a grid whose origin is so far away that p - g itself overflows for the first point"""
    g = pl.Grid([-3e38, 0, 0], [1e38, 1, 1], (2, 1, 1))
    p = np.array([[3e38, 0.25, 0.5], [-2.5e38, 0, 0], [0, 0, 0]], np.float32)
    n = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float32)
    return g, p, n


def bias(name):
    return np.float32(BIAS_OF_DIAG[name] * R.bounds(name)[3])


def positions(grid):
    """[M, 3] f32 probe centres in index order: g + float(i) * h"""
    nx, ny, nz = grid.dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    i = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(np.float32)
    return (grid.origin + (i * grid.cell).astype(np.float32)).astype(np.float32)


def probe_count(grid):
    return grid.dims[0] * grid.dims[1] * grid.dims[2]


def coefficients(grid, seed=601):
    """[M, 9, 4] f32: hashed finite values in [-1, 3), a positive band 0; .w holds a value the lookup must ignore"""
    m = probe_count(grid)
    sh = (4.0 * R._unit(seed, m * 9, 4).reshape(m, 9, 4) - 1.0).astype(np.float32)
    sh[:, 0, :3] = np.abs(sh[:, 0, :3]) + 2.0
    sh[:, :, 3] = 123.0
    return sh


def kept(grid, seed=602):
    """[M] u32: gather's kept counts, a hashed tenth of them zero"""
    m = probe_count(grid)
    u = R._unit(seed, m)[:, 0]
    return np.where(u < 0.1, 0, 1 + (u * 63).astype(np.uint32)).astype(np.uint32)


def extra_points(grid, seed=603):
    """(points, normals) f32 that sit on the edges of the cell rule: exactly on grid planes, exactly at probe centres (l2 = 0; with
    bias 0 the zero ray), far outside the grid on each of its six sides, and one point for which (p - g) / h overflows"""
    pos = positions(grid)
    m = pos.shape[0]
    span = (np.array(grid.dims, np.float32) - 1) * grid.cell
    inside = grid.origin + R._unit(seed, 12, 3).astype(np.float32) * span
    on_plane = inside.copy()
    for r in range(12):                                         # one, two or three coordinates exactly on a plane of probes
        for a in range(1 + r % 3):
            axis = (r + a) % 3
            on_plane[r, axis] = pos[R._pick(seed + 1, 12, m)[r], axis]
    centres = pos[R._pick(seed + 2, 8, m)]
    far = np.repeat(inside[:6], 1, 0).copy()
    for r in range(6):
        far[r, r % 3] = grid.origin[r % 3] + (-50.0 if r < 3 else 50.0) * max(float(span[r % 3]), 1.0)
    overflow = inside[:1].copy()
    overflow[0, 0] = 3.4e38
    p = np.concatenate([on_plane, centres, far, overflow]).astype(np.float32)
    z = 2.0 * R._unit(seed + 3, p.shape[0])[:, 0] - 1.0
    phi = 2.0 * np.pi * R._unit(seed + 4, p.shape[0])[:, 0]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    n = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return p, n


def inputs_for(name):
    """dict(points, normals, grid, sh, kept, bias, count): the scene's 576 points and the extra ones, 603 in all"""
    def make():
        p, n, _ = ac.points_for(name)
        grid = grid_for(name)
        ep, en = extra_points(grid)
        p, n = np.concatenate([p, ep]), np.concatenate([n, en])
        return dict(points=p, normals=n, grid=grid, sh=coefficients(grid), kept=kept(grid), bias=bias(name), count=p.shape[0])
    return R._cached(("probe inputs", name), make)


def centre_points(name):
    """the extra points that sit exactly at probe centres: indices into inputs_for(name)["points"]"""
    return np.arange(ac.COUNT + 12, ac.COUNT + 20)
