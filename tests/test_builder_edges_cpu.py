"""The builder edge families of builder_edges.py on the CPU: the numpy restatement of the reference's builder (bvh_literal.py)
is held to the oracle on every origin-seeded scene, and every family has to reach the structure it was built for -- asserted
from the literal tree, for the seed(s) named in builder_edges.py's table -- so that test_gpu_builder_edges.py cannot pass on
scenes that miss the builder's special cases.  Every comparison is bit for bit."""
import numpy as np
import pytest

import builder_edges as be
import bvh_literal
import oracle_lib as ol
from rayca_amd import Config, flatten, scenes

AUDIT_EVERY = 37
# The oracle's BUILD_LITERAL prices 189 planes by a loop over the node's primitives each and needs seconds for these; their
# reference trees come from its binned sweep (BUILD_BINNED), which test_oracle_bvh.py holds to the literal one.
BINNED = {"sizes16384", "sizes16385", "sizes20480", "sizes20481", "duplicates", "flat_grid"}
PLAIN = {"box": scenes.box_scene, "cornell": scenes.cornell_scene, "soup3000": lambda: scenes.soup_scene(3000)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def describe(name, seed_origin, t):
    kids = (int(t.size[t.left[0]]), int(t.size[t.right[0]])) if t.left[0] >= 0 else None
    print(f"{name} {'origin' if seed_origin else 'empty'} seed: {t.order.size} primitives, {t.count.size} nodes, depth {t.stats['depth']}, "
          f"largest leaf {t.stats['largest_leaf']}, root's children {kids}, least cost {t.stats['least_cost']:.3g}, "
          f"{t.stats['audited']} nodes priced both ways")


@pytest.mark.parametrize("name", be.SCENES + sorted(PLAIN))
def test_literal_builder_equals_the_oracle(oracle, name):
    """Primitive order, node ranges and box bits of bvh_literal.build(seed_origin=True) against the oracle's tree: pins the
    restatement, with the way it derives centroids and boxes from the world-space triangles."""
    if name in PLAIN:
        orc = ol.OracleScene(flatten(PLAIN[name]()), Config(), build=ol.BUILD_LITERAL)
        tree = bvh_literal.build(orc.world_triangles(orc.primitive_count).reshape(-1, 3, 3), True, audit_every=AUDIT_EVERY)
    else:
        orc = be.oracle_scene(name) if name in BINNED else ol.OracleScene(be.scene_desc(name), Config(), build=ol.BUILD_LITERAL)
        tree = be.literal(name, True, AUDIT_EVERY)
    describe(name, True, tree)
    assert orc.blas_count == 1
    assert np.array_equal(tree.order, orc.primitive_order())
    boxes, rng = orc.blas_nodes(0)
    lboxes, lrng = tree.oracle_nodes()
    assert np.array_equal(rng, lrng)
    assert np.array_equal(bits(boxes[:, [0, 1, 2, 4, 5, 6]]), bits(lboxes))
    if name not in BINNED:
        orc.close()


@pytest.mark.parametrize("seed_origin", [True, False])
def test_sorted_pricing_equals_a_pass_per_plane_on_a_big_root(oracle, seed_origin):
    """build() audits nodes of at most 8192 primitives; here the root of sizes16385, above the multi-workgroup threshold."""
    cent, bmin, bmax = bvh_literal.prim_data(be.triangles("sizes16385"))
    ids = np.arange(cent.shape[0])
    nlo, nhi, cost, _, _ = bvh_literal._price(cent, bmin, bmax, ids[None, :], np.array([ids.size]), seed_origin)
    ref = bvh_literal.price_planes_masked(cent, bmin, bmax, ids, nlo[0], nhi[0], seed_origin)
    assert np.array_equal(bits(ref), bits(cost[0])) and (ref < bvh_literal.FLT_MAX).sum() > 150


@pytest.mark.parametrize("seed_origin", [True, False])
@pytest.mark.parametrize("name", be.SCENES)
def test_family_reaches_its_structure(oracle, name, seed_origin):
    fam = be.family_of(name)
    t = be.literal(name, seed_origin, AUDIT_EVERY)
    describe(name, seed_origin, t)
    n = t.order.size
    assert seed_origin or t.stats["audited"] > 0
    assert np.array_equal(np.sort(t.order), np.arange(n)) and t.stats["depth"] < bvh_literal.MAX_DEPTH   # (the cap decides nothing)
    inner = t.left >= 0
    kids = (int(t.size[t.left[0]]), int(t.size[t.right[0]])) if inner[0] else None
    if fam == "sizes":
        assert int(t.size[0]) == n == int(name[5:]) and inner[0]
    elif fam == "split_kbig":
        assert kids == (be.K_BIG, be.K_BIG + 1)
    elif fam == "split_small":
        assert kids == (5000, int(name[11:]))
    elif fam == "fullbox":
        if seed_origin:   # every candidate costs exactly no_split: the root is "split", everything lands right, a leaf remains
            assert t.count.size == 1 and np.array_equal(t.order, np.roll(np.arange(n), -1))
        else:
            assert t.stats["depth"] >= 2 * be.K_LEVEL_BATCH + 1
            deep_big = int(((t.size > be.K_BIG) & (t.level >= be.K_LEVEL_BATCH)).sum())
            print(f"{name}: {deep_big} nodes above kBig at level >= {be.K_LEVEL_BATCH}")
            assert deep_big > 0 or n < 40000
    elif fam == "duplicates":
        assert t.stats["largest_leaf"] > be.K_BIG and inner[0]
    elif fam == "flat_grid":
        assert inner[0] and np.array_equal(t.lo[:, 2], t.hi[:, 2]) and (t.lo[:, 2] == 0).all()
        assert int((t.size > be.K_BIG).sum()) >= 1
    else:
        assert fam == "denormal"
        assert inner[0] and 0 < t.stats["least_cost"] < bvh_literal.FLT_MIN


@pytest.mark.parametrize("name", be.SCENES)
def test_ray_batches_hit_and_miss(oracle, name):
    """(denormal: the reference's triangle test computes the normal as a product of two edges, about 2^-146 here, which is
    zero in f32, and rejects |n . dir| < FLT_EPSILON -- no ray can hit a triangle of this scene, whatever its direction's
    length; its batch checks that nothing is hit.)"""
    _, prim, _ = be.oracle_records(name)
    hits, misses = int((prim != be.NONE).sum()), int((prim == be.NONE).sum())
    print(f"{name}: {hits} hits, {misses} misses")
    assert hits + misses == be.N_RAYS
    if be.family_of(name) == "denormal":
        assert hits == 0
    else:
        assert hits >= 100 and misses >= 100
