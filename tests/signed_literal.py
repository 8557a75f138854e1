"""rayca_hip_signed_device restated (helper module; test_signed_cpu.py, test_gpu_signed.py): the header's comment on RaycaSigned
in numpy f32.  The grid's points by the formula; the distance part is nearest_literal.closest; the counts are the totals of
hits_literal.all_hits on the rays (p, dirs[j]) with faces "front" and "both", back = both - front; then the two rules and the vote.
Nothing here knows about a tree, a cull or an order of visits."""
import numpy as np

import hits_literal as hl
import nearest_literal as nl

F = np.float32
PARITY, WINDING = 0, 1
RULES = {"parity": PARITY, "winding": WINDING}


def grid_points(origin, step, dims):
    """(nx * ny * nz, 3) f32: point i has ix = i % nx, iy = (i / nx) % ny, iz = i / (nx * ny); per axis origin + f32(index) * step,
    the product and the sum rounded on their own."""
    origin, step = np.asarray(origin, F), np.asarray(step, F)
    nx, ny, nz = (int(x) for x in dims)
    i = np.arange(nx * ny * nz, dtype=np.uint64)
    index = np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], 1)
    prod = (index.astype(F) * step[None, :]).astype(F)
    return (origin[None, :] + prod).astype(F)


def crossings(ref, points, dirs, chunk=128):
    """(front, back), each (N, n_dirs) uint32: the hits of the ray (p, dirs[j]) with face 0 and with face 1"""
    points, dirs = np.asarray(points, F).reshape(-1, 3), np.asarray(dirs, F).reshape(-1, 3)
    n = points.shape[0]
    front, back = np.zeros((n, dirs.shape[0]), np.uint32), np.zeros((n, dirs.shape[0]), np.uint32)
    for j, d in enumerate(dirs):
        rays = np.concatenate([points, np.broadcast_to(d, (n, 3))], 1).astype(F)
        f = hl.all_hits(ref, rays, None, "front", chunk)[4]
        b = hl.all_hits(ref, rays, None, "both", chunk)[4]
        front[:, j], back[:, j] = f, b - f
    return front, back


def vote(front, back, rule):
    """(votes, inside) uint8 from (N, n_dirs) counts"""
    front, back = np.asarray(front, np.uint32), np.asarray(back, np.uint32)
    n_dirs = front.shape[1]
    v = (back > front) if rule == WINDING else (((front + back) & np.uint32(1)) != 0)
    votes = np.zeros(front.shape[0], np.uint32)
    for j in range(n_dirs):
        votes |= v[:, j].astype(np.uint32) << np.uint32(j)
    pop = v.sum(1)
    return votes.astype(np.uint8), (2 * pop > n_dirs).astype(np.uint8)


def sign(ref, points, dirs, rule):
    """(inside, votes, cross) as the entry writes them; cross is (N, n_dirs, 2) uint32"""
    front, back = crossings(ref, points, dirs)
    votes, inside = vote(front, back, rule)
    return inside, votes, np.stack([front, back], 2)


def signed(ref, slot_tris, points, dirs, rule, radius=None):
    """All seven outputs: (dist2, prim, point, uv, inside, votes, cross).  slot_tris: the triangles by device slot
    (nearest_literal.slot_triangles); ref: hits_literal.Reference of the same scene."""
    d2, prim, point, uv, _ = nl.closest(slot_tris, points, radius)
    return (d2, prim, point, uv, *sign(ref, points, dirs, rule))
