"""Cases shared by test_node_step_cpu.py, test_gpu_node_step.py and make_node_step_golden.py (helper module).

The binary node step (trace_core.inc node_step, and the pipelined node loop of trace_search with NodeStack::book) decides between
three things per inner node -- both children hit, one, none -- and moves the per-lane stack accordingly; the pop behind a leaf
does the rest.  Three sets of cases:

* the decision table: a hand-made scene of 26 triangles (three per octant, ever farther from the origin, and two around the
  origin whose boxes overlap and share their top plane) and rays aimed at it.  Two restatements of the ordered binary search
  in f32, operation by operation, report which situations a ray produces: `walk` on the reference's tree (bvh_literal.build,
  what a RAYCA_BUILDER_REFERENCE scene traverses with node_step's if / else-if chain: test_node_step_cpu.py), and `ch_walk`
  on the 48-B centre / half records read back from a RAYCA_BUILDER_SAH scene, with slab_ch's fused multiply-adds -- the tree
  and the arithmetic of the pipelined node loop (test_gpu_node_step.py).  Each asserts that every one of SITUATIONS is
  produced and that the restatement's records (and, on the device's tree, its box and triangle counts) are the real ones;
* the spill boundary: the 64 x 64 frames of leaf_shade_cases.py and of a deeper scene (`deep_soup`: on the small scenes no
  camera ray ever holds the six entries it takes to cross four LDS entries) rendered by a child process whose LDS stack holds
  four entries (`python tests/node_step_cases.py OUT.npz`, started with RAYCA_PATH_LDS_ENTRIES=4: the knob is read once per
  process);
* counters: what the counting instantiations report for those frames (fused, wavefront, reference builder) and for the
  table's ray batch, recorded from the build before the change (tests/golden/node_step_counters.json)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bvh_literal   # noqa: E402
import leaf_shade_cases as L   # noqa: E402
import oracle_lib as ol   # noqa: E402
from rayca_amd import Config, flatten   # noqa: E402

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
NONE = L.NONE
GOLDEN = os.path.join(L.G, "node_step_counters.json")
SITUATIONS = ("both_tie", "both_right_nearer", "only_left", "only_right", "none_empty", "none_one", "none_deeper",
              "any_hit_stop_pending")
SPILL_ENTRIES = 4           # RAYCA_PATH_LDS_ENTRIES of the child process (the smallest value the library takes)
COUNTER_KEYS = L.COUNTER_KEYS
RAY_COUNTER_KEYS = ("boxes_tested", "triangles_tested")
ANY_HIT_TMAX = F(100.0)     # bound of the occlusion queries: beyond every hit of the table's rays

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the decision table's scene ------------------------------------------------------------------------------------------
def _tile(cx, cy, z, h):
    """a triangle seen from +z (normal towards +z), slightly slanted, around (cx, cy, z)"""
    return [[cx - h, cy - h, z + 0.25 * h], [cx + h, cy - h, z - 0.25 * h], [cx - h, cy + h, z - 0.25 * h]]


def table_triangles():
    """[26, 3, 3] f32.  Every triangle faces +z.  The reference's builder prices a split with candidate boxes that contain the
    origin (AABB::default()), so it only splits what lies around the origin or much farther from it than its neighbour: three
    triangles per octant, 1.5, 6 and 24 units out along the octant's diagonal (a chain of splits per octant below the three
    splits that tell the octants apart), and around the origin two triangles whose boxes overlap and share their top plane."""
    tri = []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                for k, dist in enumerate((1.5, 6.0, 24.0)):
                    tri.append(_tile(sx * dist, sy * (dist + 0.25 * k), sz * dist, 0.25 * dist))
    tri.append(_tile(0.0, 0.0, 0.0, 0.5))
    tri.append(_tile(0.3, 0.3, 0.0, 0.5))
    return np.array(tri, F)


def deep_scene():
    """1500 triangles of 0.3 scene units among each other under a point light: a tree some 12 levels deep whose camera rays
    pass many boxes at once, so that a lane holds more entries than the four the spill test leaves in LDS"""
    import math
    from rayca_amd import PbrMaterial, TriangleMesh, Trs, scenes
    n = 1500
    c = (L._unit(0xDEE9, (n, 1, 3)) * F(2) - F(1)) * F(0.9)
    tri = (c + (L._unit(0xDEEA, (n, 3, 3)) * F(2) - F(1)) * F(0.15)).astype(F).reshape(-1, 3)
    col = np.concatenate([L._unit(0xDEEB, (tri.shape[0], 3)) * F(0.7) + F(0.3), np.ones((tri.shape[0], 1), F)], 1).astype(F)
    tm = TriangleMesh(tri, np.arange(tri.shape[0], dtype=np.uint32), colors=col)
    return scenes._single_model_scene([(tm, PbrMaterial(color=(1, 1, 1, 1), roughness_factor=1.0))], Trs(translation=(0.0, 0.0, 3.5)),
                                      math.pi / 4, [((0.5, 2.5, 3.0), 20.0)])


SPILL_SCENES = dict(L.FRAME_SCENES, deep_soup=deep_scene)   # the frame scenes of leaf_shade_cases.py and the deep one


def frame_desc(name):
    return _cached(("fdesc", name), lambda: flatten(SPILL_SCENES[name]()))


def table_scene():
    return L._tri_scene(table_triangles(), camera=(0.0, 0.0, 30.0))


def table_desc():
    return _cached("table_desc", lambda: flatten(table_scene()))


def table_oracle():
    return _cached("table_oracle", lambda: ol.OracleScene(table_desc(), Config()))


def table_world_triangles():
    return _cached("table_tri", lambda: table_oracle().world_triangles(table_oracle().primitive_count).reshape(-1, 3, 3))


def table_tree():
    """the reference's tree of the scene (AABB::default() seeds, as the reference builds)"""
    return _cached("table_tree", lambda: bvh_literal.build(table_world_triangles(), True))


def table_rays():
    """[n, 6] f32, no direction component zero: rays from hashed origins 40 to 60 units out, aimed at the triangles (centroids and
    points near a corner) and at hashed points among them; steep rays from above onto a grid around the origin; and two rays
    through the plane z = 0.125 where the boxes of the pair overlap (the exact tie)."""
    from rayca_amd import scenes
    tri = table_triangles().astype(np.float64)
    targets = [tri.mean(1), 0.8 * tri[:, 0] + 0.1 * tri[:, 1] + 0.1 * tri[:, 2]]
    k = np.arange(1200, dtype=np.uint32)
    targets.append(np.stack([(scenes.hash_unit(0x7AB1 + a, k).astype(np.float64) * 2 - 1) * 26.0 for a in range(3)], 1))
    targets = np.concatenate(targets)
    j = np.arange(targets.shape[0], dtype=np.uint32)
    dirs = np.stack([scenes.hash_unit(0x7AB7 + a, j).astype(np.float64) * 2 - 1 for a in range(3)], 1)
    dirs[:, 2] = np.abs(dirs[:, 2]) * 0.9 + 0.1    # origins above: the triangles face +z
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    o = targets + dirs * (40.0 + 20.0 * scenes.hash_unit(0x7ABD, j).astype(np.float64))[:, None]
    rays = [np.concatenate([o, targets - o], 1)]
    g = np.arange(-3.0, 3.01, 0.4)
    gx, gy = [a.reshape(-1) for a in np.meshgrid(g, g)]
    rays.append(np.stack([gx, gy, np.full_like(gx, 5.0), 0.01 + 0.0 * gx, 0.02 + 0.0 * gx, -1.0 + 0.0 * gx], 1))
    rays.append(np.array([[-0.1, -0.1, 5.0, 0.01, 0.02, -1.0], [0.05, -0.05, 5.0, 0.02, 0.01, -1.0]]))
    rays = np.concatenate(rays).astype(F)
    assert (rays[:, 3:] != 0).all() and rays.shape[0] <= 4096
    return rays


# ---- the ordered binary search on the reference's tree, restated in f32 ---------------------------------------------------------
def _slab(lo, hi, o, rd):
    """trace_core.inc slab: (a - o) * rd per plane, each operation rounded to f32 -> (passes, tmin)"""
    t1, t2 = (lo - o) * rd, (hi - o) * rd
    far = min(min(max(t1[0], t2[0]), max(t1[1], t2[1])), min(max(t1[2], t2[2]), FLT_MAX))
    near = max(max(min(t1[0], t2[0]), min(t1[1], t2[1])), max(min(t1[2], t2[2]), -FLT_MAX))
    return bool(far >= near and far > 0), near


def cull_abs(tree):
    """scene.inc: 2^-10 x the diagonal of the root box, in f32"""
    e = (tree.hi[0] - tree.lo[0]).astype(F)
    return F(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2], dtype=F)) * F(9.765625e-4)


def walk(tree, tri_slots, ray, t_stop=None):
    """One ray through trace_search<ORDERED, !FAST, !WIDE> on `tree`; tri_slots [n, 3, 3]: the triangles in slot order.
    t_stop: the bound of an any-hit search.  -> dict(events, t, prim (slot or NONE), boxes, tris, max_stack)"""
    ray = np.asarray(ray, F)
    o, d = ray[:3], ray[3:]
    assert (d != 0).all()
    with np.errstate(all="ignore"):
        rd = (F(1) / d).astype(F)
        cabs = cull_abs(tree)

        def cull(b):
            return F(F(b + F(abs(b) * F(9.765625e-4))) + cabs)

        ev, boxes, tris, leaves, deepest = [], 1, 0, 0, 0
        best_t, best = F(np.inf), NONE
        any_hit = t_stop is not None
        stop = F(t_stop) if any_hit else FLT_MAX
        limit = cull(stop) if any_hit else F(np.inf)
        stack = []    # the newest entry last (the kernel holds it in a register, the others in LDS)
        cur = 0 if _slab(tree.lo[0], tree.hi[0], o, rd)[0] else None
        while cur is not None:
            while cur is not None and tree.left[cur] >= 0:
                l, r = int(tree.left[cur]), int(tree.right[cur])
                hl, tl = _slab(tree.lo[l], tree.hi[l], o, rd)
                hr, tr = _slab(tree.lo[r], tree.hi[r], o, rd)
                boxes += 2
                hl, hr = hl and bool(tl <= limit), hr and bool(tr <= limit)
                if hl and hr:
                    if tl <= tr:
                        ev.append("both_tie" if tl == tr else "both_left_nearer")
                        stack.append(r)
                        cur = l
                    else:
                        ev.append("both_right_nearer")
                        stack.append(l)
                        cur = r
                    deepest = max(deepest, len(stack))
                elif hl:
                    ev.append("only_left")
                    cur = l
                elif hr:
                    ev.append("only_right")
                    cur = r
                else:
                    ev.append("none_empty" if not stack else ("none_one" if len(stack) == 1 else "none_deeper"))
                    cur = stack.pop() if stack else None
            if cur is None:
                break
            leaves += 1
            first, count = int(tree.offset[cur]), int(tree.count[cur])
            ok, t = L.tri_test_f32(tri_slots[first:first + count], ray[None])
            for k in range(count):
                tris += 1
                if ok[0, k] and t[0, k] < best_t:   # (an exact tie keeps the earlier slot: the scene has none, asserted on the CPU)
                    best_t, best = t[0, k], np.uint32(first + k)
                    limit = cull(min(best_t, stop))
            if any_hit and best_t < stop:
                if leaves == 1 and stack:
                    ev.append("any_hit_stop_pending")
                break
            cur = stack.pop() if stack else None
    return {"events": ev, "t": best_t, "prim": best, "boxes": boxes, "tris": tris, "max_stack": deepest}


# ---- the ordered search on the DEVICE's tree of 48-B centre / half records, restated in f32 (needs the records read back) ---------
def fma32(a, b, c):
    """fmaf on f32 values held in Python floats: the product is exact in f64, the sum's rounding error is recovered (TwoSum)
    and decides where the f64 sum sits exactly halfway between two f32 values: one rounding, as the instruction"""
    p = a * b
    s = p + c
    if s != s or s in (float("inf"), float("-inf")):
        return float(F(s))
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = float(F(s))
    d = s - r
    if d == 0.0 or e == 0.0 or r in (float("inf"), float("-inf")):
        return r
    n = float(np.nextafter(F(r), F(np.inf if d > 0 else -np.inf)))
    if s == (r + n) / 2 and abs(n) != float("inf"):
        return n if (e > 0) == (d > 0) else r
    return r


def _f32(x):
    return float(F(x))


def ch_walk(nodes, root_box, tri_slots, ray, t_stop=None, slack_form=True):
    """One ray through the pipelined node loop of trace_search<ORDERED, FAST> on the 48-B records `nodes` [N, 12] uint32
    (DeviceScene.read_nodes(1); an inner reference is a record's byte offset, the root is record 0): make_fast, slab_ch with its
    fused multiply-adds and the ray's slack (k_trace_rays and k_query_rays always carry it), cull_limit, the decision with
    strict `tl <= tr`.  The reference-leaf filter is left out: it refuses nothing on rays this near (the records are compared
    with the device's).  -> dict(events, t, prim, boxes, tris, max_stack, spilled: entries written beyond 4 LDS entries)"""
    ray = np.asarray(ray, F)
    o, d = [float(x) for x in ray[:3]], [float(x) for x in ray[3:]]
    words = nodes.view(F)
    with np.errstate(all="ignore"):
        rd = [_f32(1.0 / x) for x in d]
        k = [-_f32(o[a] * rd[a]) for a in range(3)]
        ex = [abs(x) for x in rd]
        slack = _f32(max(abs(k[0]), abs(k[1]), abs(k[2])) * 4.76837158203125e-07) if slack_form else 0.0
        lo, hi = root_box
        e = (hi - lo).astype(F)
        cabs = float(F(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2], dtype=F)) * F(9.765625e-4))

        def cull(b):
            v = _f32(_f32(b + _f32(abs(b) * 9.765625e-4)) + cabs)
            return _f32(v + slack) if slack_form else v

        def box(c, h):
            t = [fma32(c[a], rd[a], k[a]) for a in range(3)]
            near = max(max(fma32(-h[0], ex[0], t[0]), fma32(-h[1], ex[1], t[1])), fma32(-h[2], ex[2], t[2]))
            far = min(min(fma32(h[0], ex[0], t[0]), fma32(h[1], ex[1], t[1])), fma32(h[2], ex[2], t[2]))
            tp = _f32(far + slack) if slack_form else far
            return (tp >= near and tp > 0.0), near

        ev, boxes, tris, leaves, deepest, spilled = [], 1, 0, 0, 0, 0
        best_t, best = float("inf"), NONE
        any_hit = t_stop is not None
        stop = float(t_stop) if any_hit else float(FLT_MAX)
        limit = cull(stop) if any_hit else float("inf")
        stack = []
        LEAF = 0x80000000
        root_leaf = nodes.shape[0] == 0
        cur = 0 if _slab(lo.astype(F), hi.astype(F), ray[:3], (F(1) / ray[3:]).astype(F))[0] else None
        assert not root_leaf
        while cur is not None:
            while cur is not None and not (cur & LEAF):
                w, u = words[cur // 48], nodes[cur // 48]
                hl, tl = box([float(w[0]), float(w[1]), float(w[2])], [float(w[3]), float(w[4]), float(w[5])])
                hr, tr = box([float(w[6]), float(w[7]), float(w[8])], [float(w[9]), float(w[10]), float(w[11])])
                lref = ((int(u[4]) & 0xFFFF) << 16) | (int(u[3]) & 0xFFFF)
                rref = ((int(u[10]) & 0xFFFF) << 16) | (int(u[9]) & 0xFFFF)
                boxes += 2
                hl, hr = hl and tl <= limit, hr and tr <= limit
                if hl and hr:
                    if tl <= tr:
                        ev.append("both_tie" if tl == tr else "both_left_nearer")
                        stack.append(rref)
                        cur = lref
                    else:
                        ev.append("both_right_nearer")
                        stack.append(lref)
                        cur = rref
                    deepest = max(deepest, len(stack))
                    if len(stack) >= SPILL_ENTRIES + 2:   # the newest entry in a register, entries 0-3 in LDS, this one beyond
                        spilled += 1
                elif hl:
                    ev.append("only_left")
                    cur = lref
                elif hr:
                    ev.append("only_right")
                    cur = rref
                else:
                    ev.append("none_empty" if not stack else ("none_one" if len(stack) == 1 else "none_deeper"))
                    cur = stack.pop() if stack else None
            if cur is None:
                break
            leaves += 1
            first, count = cur & 0x01FFFFFF, ((cur >> 25) & 63) + 1
            ok, t = L.tri_test_f32(tri_slots[first:first + count], ray[None])
            for j in range(count):
                tris += 1
                if ok[0, j] and float(t[0, j]) < best_t:
                    best_t, best = float(t[0, j]), np.uint32(first + j)
                    limit = cull(min(best_t, stop))
            if any_hit and best_t < stop:
                if leaves == 1 and stack:
                    ev.append("any_hit_stop_pending")
                break
            cur = stack.pop() if stack else None
    return {"events": ev, "t": F(best_t), "prim": best, "boxes": boxes, "tris": tris, "max_stack": deepest, "spilled": spilled}


def table_walks():
    """(rays, closest-hit walks, any-hit walks with ANY_HIT_TMAX) of the table's rays on the reference's tree, made once"""
    def make():
        tree, rays = table_tree(), table_rays()
        slots = table_world_triangles()[tree.order]
        return rays, [walk(tree, slots, r) for r in rays], [walk(tree, slots, r, ANY_HIT_TMAX) for r in rays]
    return _cached("table_walks", make)


def oracle_depth(desc):
    """the deepest leaf of the reference's trees of a scene (edges below the root), from the oracle's nodes"""
    orc = ol.OracleScene(desc, Config())
    deepest = 0
    for b in range(orc.blas_count):
        _, rng = orc.blas_nodes(b)
        todo = [(0, 0)]
        while todo:
            n, lvl = todo.pop()
            deepest = max(deepest, lvl)
            if rng[n, 1] == 0:   # an inner node: its children sit at offset, offset + 1
                todo += [(int(rng[n, 0]), lvl + 1), (int(rng[n, 0]) + 1, lvl + 1)]
    orc.close()
    return deepest


# ---- frames (need a GPU) ----------------------------------------------------------------------------------------------------
NODE_FORMATS = {}   # RaycaStats.node_format of the counting frames render_frames made, by their key


def render_frames(names=None):
    """{"<scene>/<builder>/<config>/u8|f32|counters": array}: the fused engine's frames of leaf_shade_cases (production
    instantiation) and the six counters of its counting instantiation, RAYCA_BUILDER_SAH and RAYCA_BUILDER_REFERENCE"""
    from rayca_amd import DeviceScene, abi
    out = {}
    for name in names or list(SPILL_SCENES):
        desc = frame_desc(name)
        for bname, builder in (("sah", abi.BUILDER_SAH), ("reference", abi.BUILDER_REFERENCE)):
            ds = DeviceScene(desc, Config(), builder=builder)
            ds.finish()
            for cname, cfg in L.CONFIGS:
                u8, f32, _ = ds.render(cfg, *L.FRAME, engine=abi.ENGINE_FUSED)
                st = ds.render(cfg, *L.FRAME, engine=abi.ENGINE_FUSED, collect_stats=True)[2]
                key = f"{name}/{bname}/{cname}/"
                out[key + "u8"], out[key + "f32"] = u8, f32
                out[key + "counters"] = np.array([int(st[k]) for k in COUNTER_KEYS], np.uint64)
                NODE_FORMATS[key] = int(st["node_format"])
            ds.close()
    return out


def frame_counters(name):
    """{engine: {config: counters}} of the counting instantiations: the fused and the wavefront engine on the
    RAYCA_BUILDER_SAH scene, the fused engine on the RAYCA_BUILDER_REFERENCE scene"""
    from rayca_amd import DeviceScene, abi
    desc = frame_desc(name)
    out = {}
    for ename, builder, engine in (("fused", abi.BUILDER_SAH, abi.ENGINE_FUSED), ("wavefront", abi.BUILDER_SAH, abi.ENGINE_WAVEFRONT),
                                   ("reference", abi.BUILDER_REFERENCE, abi.ENGINE_FUSED)):
        ds = DeviceScene(desc, Config(), builder=builder)
        ds.finish()
        out[ename] = {cname: {k: int(ds.render(cfg, *L.FRAME, engine=engine, collect_stats=True)[2][k]) for k in COUNTER_KEYS}
                      for cname, cfg in L.CONFIGS}
        ds.close()
    return out


def table_counters():
    """{how: counters} of the table's ray batch through trace_rays' counting instantiation"""
    import test_gpu_query as Q
    out = {}
    for how in Q.HOW:
        ds = Q.make_scene(table_desc(), how)
        st = ds.trace_rays(table_rays(), collect_stats=True)[3]
        out[how] = {k: int(st[k]) for k in RAY_COUNTER_KEYS}
        ds.close()
    return out


if __name__ == "__main__":   # the child process of the spill-boundary test
    np.savez(sys.argv[1], **render_frames(sys.argv[2:] or None))
    print("wrote", sys.argv[1], "RAYCA_PATH_LDS_ENTRIES =", os.environ.get("RAYCA_PATH_LDS_ENTRIES"))
    # bits 0-3 of RaycaStats.node_format: 4-wide nodes in generation 0 / in bounces, fp16 nodes in generation 0 / in bounces
    print("node formats of the RAYCA_BUILDER_SAH frames:", sorted({v & 15 for k, v in NODE_FORMATS.items() if "/sah/" in k}))
