"""The pipelined node loop of the 48-B centre / half records (trace_core.inc trace_search, NodeStack::book / pop_late: the
decision as selects, the next node's loads in front of the stack's bookkeeping, the pop's successor read into the register of
the newest entry) changes how a search is executed, never what it visits: every pixel, every hit record and every counter keep
their bits.  Only RAYCA_BUILDER_SAH scenes run that loop (ORDERED, FAST, binary 48-B records); a RAYCA_BUILDER_REFERENCE scene
runs node_step's if / else-if chain as before and is here as the issue's second engine, not as a test of the new code.

* Decision table: the rays of node_step_cases.py through trace_rays and the query entry against the oracle, bit for bit; the
  occlusion form with a bound beyond every hit.  On the RAYCA_BUILDER_SAH scene the 48-B records are read back and
  node_step_cases.ch_walk restates the search on them with slab_ch's arithmetic: every situation of the table must occur on
  THAT tree -- both children hit with tl == tr exactly, both with the right one nearer, only left, only right, none with no,
  one and more entries pending, an any-hit ray that stops in its first leaf with entries pending -- and the restatement's
  records, box count and triangle count must be the device's, so that it is the device's walk that is described.
* Spill boundary: the 64 x 64 frames of leaf_shade_cases.py (box, cornell, spheres, quad_room; depth 1-3) and of deep_soup
  rendered by a child process with RAYCA_PATH_LDS_ENTRIES=4 equal this process's frames (default entries) in RGBA8, rgba32f
  and all six counters.  On the four small scenes no camera ray holds more than four entries (walked: the cold block of
  NodeStack::transfer is entered, no entry goes beyond LDS); deep_soup is there so that entries do: its camera rays are walked
  on the device's tree and must store entries beyond the fourth LDS entry, in both forms of the search.  A second child with
  RAYCA_NODE_FORMAT=2 as well renders the same frames on the binary fp16 nodes (k_generation's kTravFastSpillHalf on deep_soup,
  kTravFastHalf where the stack fits): the same pixels and ray counts, bit for bit.
* Counters: the counting instantiations reproduce tests/golden/node_step_counters.json, recorded from the build before the
  change (tests/make_node_step_golden.py): fused, wavefront and reference-builder frames, and the table's ray batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import node_step_cases as N
import test_gpu_query as Q

pytestmark = pytest.mark.gpu
L = N.L


@pytest.fixture(scope="module")
def golden():
    return json.load(open(N.GOLDEN))


def spill_child(tmp_path_factory, **knobs):
    """(frames, stdout) of a fresh child process whose LDS stack holds SPILL_ENTRIES entries (the knobs are read once per process)"""
    out = str(tmp_path_factory.mktemp("node_step") / "spill.npz")
    env = dict(os.environ, RAYCA_PATH_LDS_ENTRIES=str(N.SPILL_ENTRIES), **knobs)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "node_step_cases.py"), out],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f"RAYCA_PATH_LDS_ENTRIES = {N.SPILL_ENTRIES}" in r.stdout
    return dict(np.load(out)), r.stdout


@pytest.fixture(scope="module")
def spilled_frames(gpu, tmp_path_factory):
    return spill_child(tmp_path_factory)[0]


@pytest.fixture(scope="module")
def spilled_half_frames(gpu, tmp_path_factory):
    """the same child with the binary fp16 nodes pinned for every generation: its path frames run k_generation's kTravFastSpillHalf
    where the stack need exceeds the LDS part (deep_soup: test_the_deep_scene_crosses_the_spill_boundary) and kTravFastHalf elsewhere"""
    frames, stdout = spill_child(tmp_path_factory, RAYCA_NODE_FORMAT="2")
    line = [l for l in stdout.splitlines() if l.startswith("node formats of the RAYCA_BUILDER_SAH frames:")]
    formats = json.loads(line[0].split(":", 1)[1])
    print("half child:", line[0])
    # fp16 nodes in generation 0 (4) and in the bounces (8), never the 4-wide tree (1, 2); 0: a frame of the stack machine
    assert 4 in formats and 12 in formats and set(formats) <= {0, 4, 12}, formats
    return frames


@pytest.mark.parametrize("name", list(N.SPILL_SCENES))
def test_frames_across_the_spill_boundary(gpu, spilled_frames, name):
    assert "RAYCA_PATH_LDS_ENTRIES" not in os.environ
    here = N.render_frames([name])
    keys = [k for k in spilled_frames if k.startswith(name + "/")]
    assert sorted(keys) == sorted(here) and len(keys) == 2 * len(L.CONFIGS) * 3
    lit = 0.0
    for k in keys:
        a, b = here[k], spilled_frames[k]
        if k.endswith("/f32"):
            assert np.array_equal(Q.bits(a), Q.bits(b)), f"{k}: max abs diff {np.nanmax(np.abs(a - b)):.3e}"
            lit = max(lit, float(a[..., :3].max()))
        else:
            assert np.array_equal(a, b), f"{k}: {a if a.size == 6 else ''} vs {b if b.size == 6 else ''}"
    assert lit > 0.0


@pytest.mark.parametrize("name", list(N.SPILL_SCENES))
def test_frames_across_the_spill_boundary_on_fp16_nodes(gpu, spilled_half_frames, name):
    """The fp16 boxes steer the search and never decide a hit (test_gpu_ray_edges.py::test_node_formats holds them to the oracle):
    the frames are this process's, bit for bit -- which test_gpu_leaf_shade.py and the oracle-checked frames above pin.  The box
    and triangle counts are the fp16 tree's own and are not compared; the ray counts are."""
    assert "RAYCA_PATH_LDS_ENTRIES" not in os.environ and "RAYCA_NODE_FORMAT" not in os.environ
    here = N.render_frames([name])
    keys = [k for k in spilled_half_frames if k.startswith(name + "/")]
    assert sorted(keys) == sorted(here) and len(keys) == 2 * len(L.CONFIGS) * 3
    for k in keys:
        a, b = here[k], spilled_half_frames[k]
        if k.endswith("/f32"):
            assert np.array_equal(Q.bits(a), Q.bits(b)), f"{k}: max abs diff {np.nanmax(np.abs(a - b)):.3e}"
        elif k.endswith("/u8"):
            assert np.array_equal(a, b), k
        else:
            assert np.array_equal(a[:4], b[:4]), f"{k}: {a} vs {b}"   # rays_primary, rays_shadow, rays_bounce, hits_shaded


@pytest.mark.parametrize("name", list(N.SPILL_SCENES))
def test_frame_counters_are_those_of_the_build_before(gpu, golden, name):
    got = N.frame_counters(name)
    for engine in ("fused", "wavefront", "reference"):
        for cname, _ in L.CONFIGS:
            assert got[engine][cname] == golden["frames"][name][engine][cname], f"{name} {engine} {cname}"


def test_table_counters_are_those_of_the_build_before(gpu, golden):
    assert N.table_counters() == golden["table_rays"]


@pytest.fixture(scope="module")
def table_records():
    rays = N.table_rays()
    ot, oprim, ouv, _ = N.table_oracle().trace_rays(rays)
    assert (oprim != N.NONE).sum() >= 64
    return rays, ot, oprim, ouv


@pytest.mark.parametrize("how", Q.HOW)
def test_decision_table_records(gpu, table_records, how):
    rays, ot, oprim, ouv = table_records
    desc = N.table_desc()
    ds = Q.make_scene(desc, how)
    want = (ot, Q.in_slots(ds, desc, oprim, "node_step_table"), ouv)
    got = Q.run_closest(ds, Q.dev(rays), None)
    Q.assert_records(got, want, f"table {how} query")
    t, prim, uv, _ = ds.trace_rays(rays)
    Q.assert_records((t, prim, uv), want, f"table {how} trace_rays")
    # the any-hit form: every ray with a hit in front of the bound is occluded, and no other
    assert (ot[oprim != N.NONE] < N.ANY_HIT_TMAX).all()
    Q.check_both(ds, Q.dev(rays), want, N.ANY_HIT_TMAX, float(N.ANY_HIT_TMAX), f"table {how} tmax")
    ds.close()


# ---- what the pipelined loop's own tree and arithmetic reach (the records read back from the device) -----------------------
def test_every_situation_occurs_on_the_device_tree(gpu, table_records):
    rays, ot, oprim, ouv = table_records
    desc = N.table_desc()
    ds = Q.make_scene(desc, "sah")
    info = ds.info()
    nodes = ds.read_nodes(1)
    assert nodes.shape[0] >= 8 and nodes.shape[1] == 12, nodes.shape
    slots = N.table_world_triangles()[ds.primitive_order()]
    tree = N.table_tree()
    root = (tree.lo[0], tree.hi[0])
    closest = [N.ch_walk(nodes, root, slots, r) for r in rays]
    any_hit = [N.ch_walk(nodes, root, slots, r, N.ANY_HIT_TMAX) for r in rays]
    # it is the device's walk: the same records, the same number of box and triangle tests
    t, prim, uv, st = ds.trace_rays(rays, collect_stats=True)
    wt, wprim = np.array([w["t"] for w in closest], np.float32), np.array([w["prim"] for w in closest], np.uint32)
    hit = prim != N.NONE
    assert np.array_equal(wprim, prim) and np.array_equal(Q.bits(wt[hit]), Q.bits(t[hit])) and hit.sum() >= 64
    assert (sum(w["boxes"] for w in closest), sum(w["tris"] for w in closest)) == (int(st["boxes_tested"]), int(st["triangles_tested"]))
    occ = Q.run_occluded(ds, Q.dev(rays), float(N.ANY_HIT_TMAX))
    assert np.array_equal(occ != 0, np.array([w["prim"] != N.NONE for w in any_hit]))
    seen = {s: sum(s in w["events"] for w in closest) for s in N.SITUATIONS}
    seen["any_hit_stop_pending"] = sum("any_hit_stop_pending" in w["events"] for w in any_hit)
    print("device tree:", info, "rays per situation:", seen, "deepest stack:", max(w["max_stack"] for w in closest))
    for s in N.SITUATIONS:
        assert seen[s] >= 1, (s, seen)
    assert max(w["max_stack"] for w in closest) >= 3   # a pop whose successor comes from LDS, not from the register alone
    ds.close()


def test_the_deep_scene_crosses_the_spill_boundary(gpu):
    from rayca_amd import Config, DeviceScene, abi
    import oracle_lib as ol
    depth = {}
    for name in N.SPILL_SCENES:
        ds = DeviceScene(N.frame_desc(name), Config(), builder=abi.BUILDER_SAH)
        ds.finish()
        depth[name] = ds.info()["max_depth"]
        if name == "deep_soup":
            nodes, order = ds.read_nodes(1), ds.primitive_order()
            cam = ds.camera_rays(Config(max_depth=1), *L.FRAME).cpu().numpy()
        ds.close()
    print("stack entries planned per RAYCA_BUILDER_SAH scene:", depth)
    assert depth["deep_soup"] >= N.SPILL_ENTRIES + 2, depth
    orc = ol.OracleScene(N.frame_desc("deep_soup"), Config())
    tri = orc.world_triangles(orc.primitive_count).reshape(-1, 3, 3)
    orc.close()
    root = (tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0))
    for slack_form in (False, True):   # generation 0 of a path frame takes either form, wave by wave
        walks = [N.ch_walk(nodes, root, tri[order], r, slack_form=slack_form) for r in cam[5::11]]
        crossing = sum(w["spilled"] > 0 for w in walks)
        print(f"slack form {slack_form}: deepest stack {max(w['max_stack'] for w in walks)}, {crossing} of {len(walks)} camera rays store entries beyond LDS entry 3")
        assert crossing >= 8
