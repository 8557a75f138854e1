"""What the cases of test_gpu_node_step.py reach on the RAYCA_BUILDER_REFERENCE side, checked on the CPU: node_step_cases.walk
restates the ordered binary search on the reference's tree of the hand-made scene (bvh_literal: the tree a
RAYCA_BUILDER_REFERENCE scene traverses, with the reference's slab arithmetic and node_step's if / else-if chain) in f32.  The
same for the pipelined node loop -- the RAYCA_BUILDER_SAH tree, the 48-B records, slab_ch -- needs the device's records and
is asserted in test_gpu_node_step.py with node_step_cases.ch_walk; the fused multiply-add it rests on is checked here."""
from fractions import Fraction

import json
import os

import numpy as np

import node_step_cases as N


def test_the_restated_search_finds_the_oracles_records(oracle):
    """every ray of the table: the same primitive slot and the same depth, bit for bit -- the restatement takes the search's
    decisions, or it would cull or miss what the oracle finds"""
    rays, closest, _ = N.table_walks()
    ot, oprim, _, _ = N.table_oracle().trace_rays(rays)
    t = np.array([w["t"] for w in closest], np.float32)
    prim = np.array([w["prim"] for w in closest], np.uint32)
    hit = oprim != N.NONE
    assert hit.sum() >= 64 and (~hit).sum() >= 64
    assert np.array_equal(prim, oprim)
    assert np.array_equal(t[hit].view(np.uint32), ot[hit].view(np.uint32)) and np.isinf(t[~hit]).all()
    # no two triangles at one depth along a ray: the restatement (and the records) need no tie rule
    tri = N.table_world_triangles()
    ok, tt = N.L.tri_test_f32(tri, rays)
    tt = np.sort(np.where(ok, tt, np.inf), axis=1)
    assert not (np.isfinite(tt[:, 0]) & (tt[:, 0] == tt[:, 1])).any()


def test_every_situation_of_the_decision_table_is_produced(oracle):
    tree = N.table_tree()
    assert tree.stats["depth"] >= 4 and (tree.left >= 0).sum() >= 8
    rays, closest, any_hit = N.table_walks()
    seen = {s: 0 for s in N.SITUATIONS}
    for w in closest:
        for e in set(w["events"]):
            if e in seen:
                seen[e] += 1
    seen["any_hit_stop_pending"] = sum("any_hit_stop_pending" in w["events"] for w in any_hit)
    print("rays per situation:", seen, "deepest stack:", max(w["max_stack"] for w in closest))
    for s in N.SITUATIONS:
        assert seen[s] >= 1, s
    # the exact tie goes left first, and the ray made for it is one of those that produce it
    assert "both_tie" in closest[-2]["events"] or "both_tie" in closest[-1]["events"]
    # a search that ends an any-hit ray in its first leaf found an occluder in front of the bound
    for w in any_hit:
        if "any_hit_stop_pending" in w["events"]:
            assert w["t"] < N.ANY_HIT_TMAX
    # `none` with a deeper stack: the successor of the popped entry comes from LDS (at least two entries pending)
    assert max(w["max_stack"] for w in closest) >= 3


def test_a_reference_tree_is_deeper_than_the_spill_test_leaves_in_lds(oracle):
    """The child process of the spill-boundary test keeps SPILL_ENTRIES = 4 entries per lane in LDS, the newest in a register:
    a lane crosses the boundary with six entries pending.  This is the reference builder's side (kernels with the if /
    else-if chain): a tree whose deepest leaf lies 6 or more levels below the root.  Whether a RAYCA_BUILDER_SAH frame really
    crosses it in the pipelined loop is asserted on the device's tree, ray by ray (test_gpu_node_step.py)."""
    depth = {name: N.oracle_depth(N.frame_desc(name)) for name in N.SPILL_SCENES}
    print("deepest leaf per scene:", depth)
    assert max(depth.values()) >= N.SPILL_ENTRIES + 2, depth


def test_fma32_rounds_once():
    """node_step_cases.fma32 against exact rational arithmetic: the result is the f32 nearest to a * b + c (cancelling sums
    -- c = -(a * b) rounded, what make_fast and slab_ch produce -- among them)"""
    k = np.arange(30000, dtype=np.uint32)
    from rayca_amd import scenes
    v = [((scenes.hash_unit(0xF3A0 + i, k).astype(np.float64) * 8 - 4) * 2.0 ** ((scenes.hash_unit(0xF3A4 + i, k) * 24).astype(int) - 12)).astype(np.float32)
         for i in range(3)]
    worse = 0
    for i in range(0, k.size, 7):
        a, b, c = float(v[0][i]), float(v[1][i]), float(v[2][i])
        if i % 3 == 0:
            c = -float(np.float32(a * b))
        r = N.fma32(a, b, c)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        err = abs(exact - Fraction(r))
        for n in (np.nextafter(np.float32(r), np.float32(-np.inf)), np.nextafter(np.float32(r), np.float32(np.inf))):
            worse += abs(exact - Fraction(float(n))) < err
    assert worse == 0


def test_the_golden_counters_cover_the_cases():
    g = json.load(open(N.GOLDEN))
    assert set(g["frames"]) == set(N.SPILL_SCENES)
    for name, engines in g["frames"].items():
        assert set(engines) == {"fused", "wavefront", "reference"}
        for e, cfgs in engines.items():
            assert set(cfgs) == {c for c, _ in N.L.CONFIGS}
            for c, k in cfgs.items():
                assert set(k) == set(N.COUNTER_KEYS) and k["boxes_tested"] > 0 and k["rays_primary"] == 64 * 64 * (2 if "_s2_" in c else 1), (name, e, c)
    assert set(g["table_rays"]) == {"reference", "sah", "sah_unfinished"}
    # the reference builder's batch visits what the restated search visits
    _, closest, _ = N.table_walks()
    assert g["table_rays"]["reference"]["boxes_tested"] == sum(w["boxes"] for w in closest)
    assert g["table_rays"]["reference"]["triangles_tested"] == sum(w["tris"] for w in closest)
