"""The reference's BLAS builder restated in numpy f32 (helper module; test_builder_edges_cpu.py, test_gpu_builder_edges.py).

Blas::set_primitives_recursive with find_best_split_plane and evaluate_sah (rayca-soft/src/bvh/blas.rs:64-123, 261-316), for
both seeds of the candidate boxes: `seed_origin=True` is the reference (AABB::default(), both corners at the origin),
`seed_origin=False` the empty seed of RAYCA_BUILDER_SAH, where a plane with an empty side is no candidate.  No bins anywhere:

* a plane's left set is {p : centroid_p < pos}, its right set the rest, taken from the node's primitives as they are;
  `price_planes_masked` prices each of the 63 x 3 planes by such a pass (a 63 x n mask per axis), `_price` -- what `build`
  runs -- sorts the node's centroids once per axis, so that every left set is a prefix of the sorted sequence whatever the
  planes' positions are, and reads the boxes from running minima / maxima (unions of min / max do not depend on the order).
  `build(audit_every=k)` prices every k-th node both ways and insists on equal bits;
* f32 with every operation rounded on its own: scale = (bmax - bmin) / 64, pos = bmin + i * scale, area = ex*ey + ey*ez + ez*ex
  left to right, cost = lc * area_l + rc * area_r, !(cost > 0) -> FLT_MAX, the first cheapest plane in (axis, plane) order
  (strict `<`), `best > no_split` makes a leaf;
* the swap partition is the loop itself (swap i with j - 1, decrement j); a one-sided result leaves a leaf, after the swaps;
* the depth cap is 255.

The recursion's nodes do not touch each other's ranges, so the nodes of one level are priced together (padded to a common
length, by size class); the nodes are then numbered as the recursion numbers them: children in pairs, the left subtree first.
Centroids and boxes come from world-space triangles with the reference's centroid arithmetic, (v0 + v1 + v2) * 0.3333."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
MAX_DEPTH = 255                      # blas.rs:194
_PLANES = np.arange(1, 64, dtype=np.float32)
_INF = F(np.inf)


def prim_data(tri):
    """tri [n, 3, 3] f32 world-space triangles -> centroid (triangle.rs:59-63), min, max, each [n, 3] f32"""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3, 3)
    cent = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * F(0.3333)
    return cent, tri.min(1), tri.max(1)


def area(lo, hi):
    """aabb.rs:20-23"""
    e = hi - lo
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


def plane_positions(lo, hi):
    """lo, hi [...]: one axis of node boxes -> [..., 63] candidate positions (blas.rs:101-104)"""
    scale = (hi - lo) / F(64)
    return lo[..., None] + _PLANES * scale[..., None]


def _cost(lc, rc, lmin, lmax, rmin, rmax, seed_origin):
    if seed_origin:
        lmin, lmax, rmin, rmax = np.minimum(lmin, F(0)), np.maximum(lmax, F(0)), np.minimum(rmin, F(0)), np.maximum(rmax, F(0))
    k = lc.astype(F) * area(lmin, lmax) + rc.astype(F) * area(rmin, rmax)
    raw = k
    k = np.where(k > 0, k, FLT_MAX)
    if not seed_origin:
        skip = (lc == 0) | (rc == 0)
        k = np.where(skip, FLT_MAX, k)
        raw = np.where(skip, np.nan, raw)
    return k.astype(F), raw


def price_planes_masked(cent, bmin, bmax, ids, nlo, nhi, seed_origin):
    """One node, every plane by a pass over its primitives: cost [3, 63] f32 (FLT_MAX where the axis has no extent)."""
    cost = np.full((3, 63), FLT_MAX, F)
    c, lo, hi = cent[ids], bmin[ids], bmax[ids]
    with np.errstate(all="ignore"):
        for a in range(3):
            if nlo[a] == nhi[a]:
                continue
            pos = plane_positions(nlo[a], nhi[a])
            left = c[None, :, a] < pos[:, None]                    # [63, n]
            lc = left.sum(1)
            rc = ids.size - lc
            lmin = np.where(left[..., None], lo[None], _INF).min(1)
            lmax = np.where(left[..., None], hi[None], -_INF).max(1)
            rmin = np.where(left[..., None], _INF, lo[None]).min(1)
            rmax = np.where(left[..., None], -_INF, hi[None]).max(1)
            cost[a], _ = _cost(lc, rc, lmin, lmax, rmin, rmax, seed_origin)
    return cost


def _price(cent, bmin, bmax, ids, cnt, seed_origin):
    """m nodes padded to P primitives: ids [m, P] (anything beyond cnt), cnt [m] -> the nodes' boxes nlo, nhi [m, 3]
    (BvhNode::new, blas.rs:27-36), cost [m, 3, 63] f32, pos [m, 3, 63] f32, the smallest cost above zero seen (before
    FLT_MAX replaces anything)"""
    m, P = ids.shape
    pad = np.arange(P)[None, :] >= cnt[:, None]
    safe = np.where(pad, 0, ids)
    lo = np.where(pad[..., None], _INF, bmin[safe])
    hi = np.where(pad[..., None], -_INF, bmax[safe])
    nlo, nhi = lo.min(1), hi.max(1)
    cost = np.full((m, 3, 63), FLT_MAX, F)
    pos = np.zeros((m, 3, 63), F)
    rows = np.arange(m)[:, None]
    least = np.inf
    with np.errstate(all="ignore"):
        for a in range(3):
            p = plane_positions(nlo[:, a], nhi[:, a])
            c = np.where(pad, _INF, cent[safe, a])
            s = np.argsort(c, axis=1, kind="stable")
            cs = np.take_along_axis(c, s, 1)
            lc = np.count_nonzero(cs[:, None, :] < p[:, :, None], axis=-1)   # [m, 63]: how many centroids lie left of each plane
            rc = cnt[:, None] - lc
            los, his = np.take_along_axis(lo, s[..., None], 1), np.take_along_axis(hi, s[..., None], 1)
            pmin, pmax = np.minimum.accumulate(los, 1), np.maximum.accumulate(his, 1)
            smin, smax = np.minimum.accumulate(los[:, ::-1], 1)[:, ::-1], np.maximum.accumulate(his[:, ::-1], 1)[:, ::-1]
            li, ri = np.maximum(lc - 1, 0), np.minimum(lc, P - 1)
            none_l, none_r = (lc == 0)[..., None], (rc == 0)[..., None]
            lmin, lmax = np.where(none_l, _INF, pmin[rows, li]), np.where(none_l, -_INF, pmax[rows, li])
            rmin, rmax = np.where(none_r, _INF, smin[rows, ri]), np.where(none_r, -_INF, smax[rows, ri])
            k, raw = _cost(lc, rc, lmin, lmax, rmin, rmax, seed_origin)
            valid = (nlo[:, a] != nhi[:, a])[:, None]
            cost[:, a] = np.where(valid, k, FLT_MAX)
            pos[:, a] = p
            raw = raw[np.broadcast_to(valid, raw.shape) & (raw > 0)]
            if raw.size:
                least = min(least, float(raw.min()))
    return nlo, nhi, cost, pos, least


class Tree:
    """order [n] uint32; per node, numbered as the recursion numbers them (root 0, children in pairs, left subtree first):
    lo / hi [N, 3] f32, offset / size [N] (the node's range), count [N] (0: an inner node), left / right [N] (-1: a leaf),
    level [N];
    stats: depth, largest_leaf, least_cost (the smallest candidate cost above zero), audited (nodes priced both ways)"""

    def oracle_nodes(self):
        """The nodes as oracle_blas_nodes lists them: the unused slot 1 (blas.rs:254-256) in place, an inner node's
        offset = the index of its left child.  -> boxes [N + 1, 6] f32, ranges [N + 1, 2] uint32"""
        N = self.count.size
        at = np.arange(N) + (np.arange(N) > 0)
        boxes = np.zeros((N + 1, 6), F)
        rng = np.zeros((N + 1, 2), np.uint32)
        boxes[at, :3], boxes[at, 3:] = self.lo, self.hi
        inner = self.left >= 0
        rng[at, 0] = np.where(inner, self.left + 1, self.offset)
        rng[at, 1] = self.count
        return boxes, rng


def _range_boxes(bmin, bmax, order, off, size):
    """boxes of the ranges [off, off + size) of `order` (min / max over a range do not depend on its inner order)"""
    n = order.size
    idx = np.stack([off, off + size], 1).reshape(-1)
    lo = np.minimum.reduceat(np.concatenate([bmin[order], bmin[:1]]), idx)[::2]
    hi = np.maximum.reduceat(np.concatenate([bmax[order], bmax[:1]]), idx)[::2]
    assert idx.max() <= n
    return lo, hi


def build(tri, seed_origin, audit_every=0, audit_max=8192):
    """-> Tree.  audit_every = k: every k-th priced node of at most audit_max primitives is priced again by
    price_planes_masked, and the two sets of 189 costs must have equal bits."""
    cent, bmin, bmax = prim_data(tri)
    n = cent.shape[0]
    order = np.arange(n, dtype=np.int64)
    cl = [cent[:, a].astype(np.float64).tolist() for a in range(3)]   # (f32 -> f64 is exact: the same comparisons)
    n_off, n_cnt, n_left, n_right, n_level = [0], [n], [-1], [-1], [0]
    stats = {"least_cost": np.inf, "audited": 0}
    open_nodes, level, priced = [0], 0, 0
    while open_nodes and level < MAX_DEPTH:
        nxt = []
        groups = {}
        for k in open_nodes:   # nodes of about one size are priced together
            c = n_cnt[k]
            groups.setdefault(1 << (c - 1).bit_length() if c <= 512 else -k, []).append(k)
        for key, members in groups.items():
            P = key if key > 0 else n_cnt[members[0]]
            step = max(1, (1 << 22) // (63 * P))
            for g in range(0, len(members), step):
                ks = members[g:g + step]
                off, cnt = np.array([n_off[k] for k in ks]), np.array([n_cnt[k] for k in ks])
                ids = order[np.minimum(off[:, None] + np.arange(P)[None, :], n - 1)]
                nlo, nhi, cost, pos, least = _price(cent, bmin, bmax, ids, cnt, seed_origin)
                stats["least_cost"] = min(stats["least_cost"], least)
                flat = cost.reshape(len(ks), 189)
                first = flat.argmin(1)                      # the first cheapest: what strict `<` in (axis, plane) order keeps
                best = flat[np.arange(len(ks)), first]
                split_pos = pos.reshape(len(ks), 189)[np.arange(len(ks)), first]
                with np.errstate(all="ignore"):
                    no_split = cnt.astype(F) * area(nlo, nhi)
                if audit_every:
                    for r in range(len(ks)):
                        if (priced + r) % audit_every == 0 and cnt[r] <= audit_max:
                            ref = price_planes_masked(cent, bmin, bmax, ids[r, :cnt[r]], nlo[r], nhi[r], seed_origin)
                            assert np.array_equal(ref.view(np.uint32), cost[r].view(np.uint32)), f"node {ks[r]}: the two pricings differ"
                            stats["audited"] += 1
                priced += len(ks)
                none = best == FLT_MAX                       # no plane was ever cheaper than the initial FLT_MAX (blas.rs:94-96)
                axes = np.where(none, 0, first // 63).tolist()
                splits = np.where(none, F(0), split_pos).astype(np.float64).tolist()
                for r in np.flatnonzero(~(best > no_split)).tolist():
                    k, o_at, o_n = ks[r], int(off[r]), int(cnt[r])
                    # blas.rs:279-289
                    o = order[o_at:o_at + o_n].tolist()
                    ca, split = cl[axes[r]], splits[r]
                    i, j = 0, o_n
                    while i < j:
                        if ca[o[i]] < split:
                            i += 1
                        else:
                            o[i], o[j - 1] = o[j - 1], o[i]
                            j -= 1
                    order[o_at:o_at + o_n] = o
                    if i == 0 or i == o_n:
                        continue
                    base = len(n_cnt)
                    n_off += (o_at, o_at + i)
                    n_cnt += (i, o_n - i)
                    n_left += (-1, -1)
                    n_right += (-1, -1)
                    n_level += (level + 1, level + 1)
                    n_left[k], n_right[k] = base, base + 1
                    if i > 1:   # (a single primitive can be neither split nor reordered)
                        nxt.append(base)
                    if o_n - i > 1:
                        nxt.append(base + 1)
        open_nodes, level = nxt, level + 1
    # the recursion's numbering: a node's children are pushed as a pair when it is split, then the left subtree is built
    N = len(n_cnt)
    number = np.full(N, -1, np.int64)
    number[0] = 0
    made, stack = 1, [0]
    while stack:
        k = stack.pop()
        if n_left[k] >= 0:
            number[n_left[k]], number[n_right[k]] = made, made + 1
            made += 2
            stack.append(n_right[k])
            stack.append(n_left[k])
    assert made == N
    inv = np.argsort(number)
    t = Tree()
    t.order = order.astype(np.uint32)
    t.offset, t.level = np.array(n_off, np.int64)[inv], np.array(n_level, np.int64)[inv]
    left, right, t.size = np.array(n_left, np.int64)[inv], np.array(n_right, np.int64)[inv], np.array(n_cnt, np.int64)[inv]
    t.left, t.right = np.where(left >= 0, number[np.maximum(left, 0)], -1), np.where(right >= 0, number[np.maximum(right, 0)], -1)
    t.count = np.where(left >= 0, 0, t.size)
    t.lo, t.hi = _range_boxes(bmin, bmax, order, t.offset, t.size)
    stats["depth"] = int(t.level.max())
    stats["largest_leaf"] = int(t.count.max())
    t.stats = stats
    return t
