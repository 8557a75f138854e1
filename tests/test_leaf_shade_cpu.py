"""What the ray sets of test_gpu_leaf_shade.py reach, checked on the CPU with the oracle and a restatement of the triangle
test in f32, operation by operation (leaf_shade_cases.tri_test_f32)."""
import numpy as np

import leaf_shade_cases as L


def test_the_soup_set_has_rays_whose_nearer_triangle_the_reference_leaf_refuses(oracle):
    """A ray "refused" here passes the restated triangle test on a triangle NEARER than the oracle's record (or the oracle
    records a miss): the reference never tested that triangle, because the box of its leaf failed the slab test, and the
    kernels' reference-leaf filter (trace_core.inc reference_candidate, inside test_leaf) has to refuse it likewise.
      - The 2048 rays of tests/golden/soup1k_rays.npz and the 18 000 rays through triangle corners hold NO such ray: with origins
        within a few scene sizes of the boxes, the slab test's rounding (2^-24 relative per plane distance) never outweighs the
        margin by which a ray that meets a triangle inside a box passes that box.  Asserted, not assumed.
      - The 12 000 far rays (origins 10^6 units away) hold such rays of both kinds: the oracle records a farther hit, and the
        oracle records a miss.
    On every other ray of the set the restated nearest depth equals the oracle's record bit for bit: the restatement is the
    kernel's test, and a difference is a refusal, not an error of the restatement."""
    rays, n_near, refused, depth, nearest = L.soup_set()
    assert n_near == 2048 + 18000 and rays.shape[0] == n_near + 12000
    farther = np.isfinite(depth[refused])
    print(f"rays {rays.shape[0]}, hits {np.isfinite(depth).sum()}, refused: {refused.size} ({farther.sum()} with a farther record, {(~farther).sum()} with a miss)")
    assert (refused < n_near).sum() == 0
    assert farther.sum() >= 1 and (~farther).sum() >= 1
    rest = np.ones(rays.shape[0], bool)
    rest[refused] = False
    assert np.array_equal(nearest[rest].view(np.uint32), depth[rest].view(np.uint32))
    assert np.isfinite(depth[:2048]).sum() >= 256 and np.isfinite(depth[2048:n_near]).sum() >= 4096 and np.isfinite(depth[n_near:]).sum() >= 1024


def test_aimed_rays_land_on_their_slots(oracle):
    """soup1k: the rays aimed at reference slots 0, 1, 2, the last one and the slots = 2 mod 8 hit them in the oracle."""
    orc, tri = L.oracle("soup1k"), L.triangles("soup1k")
    order = orc.primitive_order()
    rays = L.aimed_rays(tri[order]).reshape(-1, 6)
    _, oprim, _, _ = orc.trace_rays(rays)
    landed = oprim.reshape(-1, 4) == np.arange(order.size, dtype=np.uint32)[:, None]
    assert landed.any(1).mean() >= 0.9, landed.any(1).mean()


def test_coincident_scene_ties(oracle):
    orc, tri = L.oracle("coincident"), L.triangles("coincident")
    assert tri.shape[0] == 110 and (tri[:70] == tri[0]).all()
    _, oprim, _, _ = orc.trace_rays(L.aimed_rays(tri).reshape(-1, 6))
    flat = orc.primitive_order()[oprim[oprim != L.NONE]]
    assert (flat < 70).sum() >= 4 * 70 and np.unique(flat[flat < 70]).size == 1
