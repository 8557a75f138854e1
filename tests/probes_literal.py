"""rayca_hip_probe_lookup_device restated (helper module; test_probes_cpu.py, test_gpu_probes.py): the header's comment on
RaycaProbeLookup in numpy f32, operation by operation -- every + - * / rounds on its own; floor, min, max (maxNum), |x|,
comparisons, selects and integers; no square root, no trigonometry.  The points run along the arrays' first axis; the corners, the
coefficients and the two passes of the blend are loops in the order the text gives them, never a reduction that could reassociate.
Whether a corner's ray is occluded is an input here (the oracle's records on the CPU, DeviceScene.query(kind="occluded", tmax=1)
on the GPU)."""
import numpy as np

from ambient_literal import active  # noqa: F401  (the inactive rule is RaycaAmbient's: imported, not restated)

F0, F1, HALF = np.float32(0), np.float32(1), np.float32(0.5)
VISIBILITY, NORMAL_TERM = 1, 2
A = [np.float32(3.1415927)] + [np.float32(2.0943952)] * 3 + [np.float32(0.7853982)] * 5
INV_PI = np.float32(0.31830987)


def f32(x):
    return np.asarray(x, np.float32)


class Grid:
    def __init__(self, origin, cell, dims):
        self.origin, self.cell, self.dims = f32(origin), f32(cell), tuple(int(d) for d in dims)


def cells(grid, p):
    """(i0 [N, 3] u32, i1 [N, 3] u32, t [N, 3] f32) of the points p [N, 3]"""
    p = f32(p)
    i0, i1, t = np.zeros(p.shape, np.uint32), np.zeros(p.shape, np.uint32), np.zeros(p.shape, np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            dim = grid.dims[a]
            f = (p[:, a] - grid.origin[a]) / grid.cell[a]
            f = np.fmin(np.fmax(f, F0), np.float32(dim - 1))
            fl = np.floor(f)
            fl = np.where(np.isfinite(fl), fl, F0)          # (an inactive point's NaN: its row is never read)
            i0[:, a] = np.minimum(fl.astype(np.uint32), np.uint32(dim - 2 if dim >= 2 else 0))
            t[:, a] = f - i0[:, a].astype(np.float32)
            i1[:, a] = np.minimum(i0[:, a] + np.uint32(1), np.uint32(dim - 1))
    return i0, i1, t


def corners(grid, cell, kept=None):
    """per corner k = 0..7: (m [N, 8] u32, c [N, 8, 3] f32, wt [N, 8] f32, candidate [N, 8] bool)"""
    i0, i1, t = cell
    n = i0.shape[0]
    m, c, wt = np.zeros((n, 8), np.uint32), np.zeros((n, 8, 3), np.float32), np.zeros((n, 8), np.float32)
    nx, ny, _ = grid.dims
    for k in range(8):
        b = [k & 1, (k >> 1) & 1, (k >> 2) & 1]
        idx = [i1[:, a] if b[a] else i0[:, a] for a in range(3)]
        w = [t[:, a] if b[a] else F1 - t[:, a] for a in range(3)]
        m[:, k] = (idx[2] * np.uint32(ny) + idx[1]) * np.uint32(nx) + idx[0]
        for a in range(3):
            c[:, k, a] = grid.origin[a] + idx[a].astype(np.float32) * grid.cell[a]
        wt[:, k] = (w[0] * w[1]) * w[2]
    cand = wt > F0
    if kept is not None:
        cand &= np.asarray(kept)[m] != 0
    return m, c, wt, cand


def rays(p, n, c, bias):
    """(o [N, 8, 3], d [N, 8, 3]): o = p + n * bias, d = c_k - o"""
    p, n, bias = f32(p), f32(n), np.float32(bias)
    with np.errstate(all="ignore"):
        o = p + n * bias
        o = np.repeat(o[:, None, :], 8, 1).astype(np.float32)
        d = f32(c) - o
    return o, d.astype(np.float32)


def normal_weight(p, n, ck):
    """wb [N] of one corner's centres ck [N, 3]"""
    p, n = f32(p), f32(n)
    with np.errstate(all="ignore"):
        v = ck - p
        s = (v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2]
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        q = np.where(l2 > F0, (s * np.abs(s)) / l2, F1).astype(np.float32)
        wb = (q + F1) * HALF
        wb = wb * wb + np.float32(0.0625)
    return wb.astype(np.float32)


def _blend(p, n, m, c, wt, take, sh, normal_term):
    """one pass over the corners of `take` [N, 8], k ascending: (wsum [N], H [N, 9, 3])"""
    cnt = p.shape[0]
    wsum, h = np.zeros(cnt, np.float32), np.zeros((cnt, 9, 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(8):
            w = wt[:, k]
            if normal_term:
                w = w * normal_weight(p, n, c[:, k])
            counts = take[:, k] & (w > F0)
            rec = sh[m[:, k]]                                  # [N, 9, 4]
            wsum = np.where(counts, wsum + w, wsum).astype(np.float32)
            for j in range(9):
                h[:, j] = np.where(counts[:, None], h[:, j] + w[:, None] * rec[:, j, :3], h[:, j])
    return wsum, h


def evaluate(h, n):
    """E [N, 3]: b_j = A_l(j) * Y_j(n), E = sum over j ascending of b_j * H[j], then max(E, 0)"""
    n = f32(n)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        ys = [np.full(x.shape, np.float32(0.2820948), np.float32), np.float32(0.4886025) * y, np.float32(0.4886025) * z, np.float32(0.4886025) * x,
              np.float32(1.0925484) * (x * y), np.float32(1.0925484) * (y * z), np.float32(0.3153916) * ((np.float32(3.0) * (z * z)) - F1),
              np.float32(1.0925484) * (x * z), np.float32(0.5462742) * ((x * x) - (y * y))]
        e = np.zeros((n.shape[0], 3), np.float32)
        for j in range(9):
            b = (A[j] * ys[j]).astype(np.float32)
            e = e + b[:, None] * h[:, j]
        e = np.fmax(e, F0)
    return e.astype(np.float32)


def fold(occ, grid, p, n, sh, kept=None, flags=VISIBILITY | NORMAL_TERM, albedo=None, base=None):
    """{"irradiance" [N, 4] f32, "sh" [N, 9, 4] f32, "mask" [N] u32, "radiance" [N, 4] f32 (with albedo)} from per-corner occlusion
    occ [N, 8] (None without visibility; ignored for corners that are no candidates and for inactive points)"""
    p, n, sh = f32(p), f32(n), f32(sh)
    cnt = p.shape[0]
    act = active(p, n)
    vis, normal_term = bool(flags & VISIBILITY), bool(flags & NORMAL_TERM)
    m, c, wt, cand = corners(grid, cells(grid, p), kept)
    cand &= act[:, None]
    occ = (np.asarray(occ, bool) & cand) if vis else np.zeros((cnt, 8), bool)
    wsum, h = _blend(p, n, m, c, wt, cand & ~occ, sh, normal_term)
    fallback = act & ~(wsum > F0) if (vis or normal_term) else np.zeros(cnt, bool)
    wsum2, h2 = _blend(p, n, m, c, wt, cand, sh, False)
    wsum = np.where(fallback, wsum2, wsum)
    h = np.where(fallback[:, None, None], h2, h)
    with np.errstate(all="ignore"):
        ok = wsum > F0
        hn = h / wsum[:, None, None]
    h = np.where(ok[:, None, None], hn, F0).astype(np.float32)
    wsum = np.where(ok, wsum, F0).astype(np.float32)
    e = evaluate(h, n)
    h[~act], wsum[~act], e[~act] = 0, 0, 0
    mask = np.zeros(cnt, np.uint32)
    for k in range(8):
        mask |= cand[:, k].astype(np.uint32) << np.uint32(k)
        mask |= occ[:, k].astype(np.uint32) << np.uint32(8 + k)
    mask |= fallback.astype(np.uint32) << np.uint32(16)
    out = {"irradiance": np.concatenate([e, wsum[:, None]], 1).astype(np.float32),
           "sh": np.concatenate([h, np.zeros((cnt, 9, 1), np.float32)], 2).astype(np.float32), "mask": mask}
    if albedo is not None:
        albedo = f32(albedo)
        with np.errstate(all="ignore"):
            l = albedo[:, :3] * (e * INV_PI)
            alpha = np.ones(cnt, np.float32)
            if base is not None:
                base = f32(base)
                l = l + base[:, :3]
                alpha = base[:, 3]
        rad = np.concatenate([l, alpha[:, None]], 1).astype(np.float32)
        rad[~act] = base[~act] if base is not None else f32([0, 0, 0, 1])
        out["radiance"] = rad
    return out
