"""The device BLAS builder (rayca_amd/csrc/bvh_build.hip) on the edge families of builder_edges.py, for both seeds of the
candidate boxes: the scene built on the device against the same scene built by the host recursion (counts, primitive order,
the 64-B node records word for word, hit records and test counts of a ray batch), both against the literal builder of
bvh_literal.py (primitive order) and against the oracle (primitive order of the reference tree, Flat frames under ordered and
exhaustive traversal, hit records).  Everything is compared bit for bit.  test_builder_edges_cpu.py asserts that every family
reaches the special case it was built for, and that the ray batches hold hits and misses."""
import numpy as np
import pytest

import builder_edges as be
from rayca_amd import Config, DeviceScene, abi

pytestmark = pytest.mark.gpu
BUILDERS = {"reference": abi.BUILDER_REFERENCE, "sah": abi.BUILDER_SAH}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def chain_links(scene):
    """The links of the chains that split leaves above 64 primitives, in the 48-B centre / half-extent records a SAH scene's
    conservative kernels traverse: two identical boxes, 64 primitives on the left, the rest of the chain on the right.  A
    chain's stack need is one entry because the left child is entered first, so the left box has to be entered no later than
    the right one, whatever the references stored below the x and y half extents are: left hx, hy >= right hx, hy (hz carries
    no reference and is equal).  Checked BEFORE any ray is traced: a search that enters the right child first keeps a leaf
    pending per link and runs past its stack.  A link's x / y half extents are rounded up to 8 mantissa bits (< 1 step of 2^16
    ulps), the left ones get one step more, the reference is < 1 step: < 3 steps = 3 * 2^-7 of the half extent.
    Returns the number of links (0 where the build has no such records)."""
    n64 = scene.read_nodes(0)
    try:
        n48 = scene.read_nodes(1)
    except Exception:   # a build that traverses the 64-B min / max nodes: identical boxes tie, and ties go left
        return 0
    assert n48.shape[0] == n64.shape[0]
    left, right = n64[:, 12], n64[:, 13]
    link = (n64[:, 0:6] == n64[:, 6:12]).all(1) & ((left >> 31) == 1) & (((left >> 25) & 63) == 63) & ((right >> 31) == 0) & (right != 0x7FFFFFFF)
    hb = n48.reshape(-1, 2, 2, 3)[link][:, :, 1]                   # link, child, half-extent bits xyz (h >= 0: bit order is value order)
    assert (hb[:, 0, :2] >= hb[:, 1, :2]).all() and np.array_equal(hb[:, 0, 2], hb[:, 1, 2])
    L = np.longdouble
    box = n64[link][:, :12].view(np.float32).astype(L).reshape(-1, 2, 2, 3)
    rec = n48[link].view(np.float32).astype(L).reshape(-1, 2, 2, 3)
    lo, hi, c, h = box[:, :, 0], box[:, :, 1], rec[:, :, 0], rec[:, :, 1]
    exact = (hi - lo) / 2 + np.abs(c - (lo + hi) / 2)
    assert np.all(c - h <= lo) and np.all(c + h >= hi) and np.all(h <= exact * L(1 + 3 * 2.0 ** -7) * L(1 + 1e-6) + L(1e-37))
    return int(link.sum())


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", be.SCENES)
def test_device_build_equals_host_build_literal_builder_and_oracle(gpu, name, builder):
    """(sizes4095 is built on the host on both sides, by design: below the threshold nothing changes.)"""
    desc, rays = be.scene_desc(name), be.rays(name)
    a = DeviceScene(desc, Config(), builder=BUILDERS[builder])
    b = DeviceScene(desc, Config(), builder=BUILDERS[builder], build_on_host=True)
    try:
        ia, ib = a.info(), b.info()
        assert ia["node_count"] == ib["node_count"] and ia["blas_count"] == ib["blas_count"] == 1
        order = a.primitive_order()
        assert np.array_equal(order, b.primitive_order())
        # the 64-B records: two boxes, two child references, two padding words that both builders write as zero
        assert np.array_equal(a.read_nodes(0), b.read_nodes(0))
        assert np.array_equal(order, be.literal(name, builder == "reference").order)
        if builder == "reference":
            assert np.array_equal(order, be.oracle_scene(name).primitive_order())
        if builder == "sah":
            links = (chain_links(a), chain_links(b))
            # duplicates: the one traversed tree with a leaf above 64 primitives, 20000 of them = 312 chain nodes, the last
            # of which holds two leaves
            assert links[0] == links[1] and (name != "duplicates" or links[0] in (0, 20000 // 64 - 1))
        ta, pa, ua, sa = a.trace_rays(rays, collect_stats=True)
        tb, pb, ub, sb = b.trace_rays(rays, collect_stats=True)
        assert np.array_equal(pa, pb) and np.array_equal(bits(ta), bits(tb)) and np.array_equal(bits(ua), bits(ub))
        assert sa["boxes_tested"] == sb["boxes_tested"] and sa["triangles_tested"] == sb["triangles_tested"]
        ot, oflat, ouv = be.oracle_records(name)
        hit = pa != be.NONE
        assert np.array_equal(hit, oflat != be.NONE) and np.array_equal(order[pa[hit]], oflat[hit])
        assert np.array_equal(bits(ta), bits(ot)) and np.array_equal(bits(ua), bits(ouv))
        want = be.oracle_frame(name)
        for scene in (a, b):
            for trav in (abi.TRAVERSAL_ORDERED, abi.TRAVERSAL_EXHAUSTIVE):
                _, f32, _ = scene.render(be.FLAT, *be.FRAME, traversal=trav)
                assert np.array_equal(bits(f32), bits(want)), (scene is a, trav)
    finally:
        a.close()
        b.close()
