"""Inputs of DeviceScene.signed (rayca_hip_signed_device) that a host usually makes once: the directions of the crossing-count
rays, and a grid's points as the kernel makes them (numpy only: no torch, no device)."""
import numpy as np

# Five fixed, unit-ish directions.  No component is zero -- the reference's box test gives an axis-aligned ray no hits at all --
# and no two are parallel or opposite (the |cosine| between any two of them is below 0.8), so a feature that fools one ray -- an
# edge seen end-on, a grazing face -- does not fool the next.  None lies in a coordinate plane or on a diagonal of one, where
# the faces and edges of modelled geometry like to lie.  Rows 3 and 4 are (3, -1, 2) / sqrt(14), and (-1, -1, 2) / sqrt(6) turned a
# little off the plane x = y.
SIGN_DIRECTIONS = np.array([[0.5370, 0.6914, 0.4837],
                            [-0.6533, 0.2706, 0.7071],
                            [0.2113, -0.7887, -0.5774],
                            [0.8018, -0.2673, 0.5345],
                            [-0.4352, -0.3811, 0.8157]], np.float32)
SIGN_DIRECTIONS.setflags(write=False)


def sign_directions(n=3):
    """The first n (1, 3 or 5) of the five fixed directions, (n, 3) float32."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n not in (1, 3, 5):
        raise ValueError(f"dirs: 1, 3 or 5 directions, not {n!r}")
    return SIGN_DIRECTIONS[:n].copy()


def checked_directions(dirs):
    """`dirs` of DeviceScene.signed as an (n, 3) float32 array: a number picks from SIGN_DIRECTIONS, an array is checked as the
    library checks it -- 1, 3 or 5 rows, every component finite and not zero."""
    if isinstance(dirs, (int, np.integer)) and not isinstance(dirs, bool):
        return sign_directions(int(dirs))
    d = np.array(dirs, np.float32)
    if d.ndim != 2 or d.shape[1] != 3 or d.shape[0] not in (1, 3, 5):
        raise ValueError(f"dirs: shape {d.shape}, expected (n, 3) with n = 1, 3 or 5")
    if not np.isfinite(d).all() or (d == 0).any():
        raise ValueError("dirs: a component is zero, NaN or infinite (an axis-aligned ray has no hits)")
    return d


def checked_grid(grid):
    """`grid` of DeviceScene.signed, (origin, step, dims), as ((3,) float32, (3,) float32, (nx, ny, nz)) and its point count."""
    try:
        origin, step, dims = grid
        origin, step = np.array(origin, np.float32).reshape(-1), np.array(step, np.float32).reshape(-1)
        dims = tuple(int(x) for x in dims)
    except (TypeError, ValueError):
        raise ValueError(f"grid: (origin, step, dims) with three numbers each is expected, not {grid!r}") from None
    if origin.shape != (3,) or step.shape != (3,) or len(dims) != 3:
        raise ValueError(f"grid: (origin, step, dims) with three numbers each is expected, not {grid!r}")
    if min(dims) < 1:
        raise ValueError(f"grid: dims {dims}: every dimension must be at least 1")
    n = dims[0] * dims[1] * dims[2]
    if n > 0xFFFFFFFF:
        raise ValueError(f"grid: dims {dims}: more than 2**32 - 1 points")
    return origin, step, dims, n


def grid_points(origin, step, dims):
    """The points of a grid as the kernel makes them, (nx * ny * nz, 3) float32 with x running fastest: per axis
    origin + float32(index) * step, the product and the sum each rounded to float32."""
    origin, step, dims, _ = checked_grid((origin, step, dims))
    axes = [(origin[a] + np.arange(dims[a], dtype=np.uint32).astype(np.float32) * step[a]).astype(np.float32) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
