"""The adversarial ray families of ray_edges.py on the CPU oracle: the GPU comparisons of test_gpu_ray_edges.py must not
be able to pass on misses (or on hits) alone, so every (scene, family) pair has to hold both, in the shares asserted
here; the coplanar ties must go to the reference's first primitive; and the conservative box test of the
RAYCA_BUILDER_SAH kernels, restated in numpy, must not steer a single reference hit of the `far` family away."""
import numpy as np
import pytest

import ray_edges as re_

NONE = re_.NONE


def shares(prim):
    hit = prim != NONE
    return hit.mean(), (~hit).mean()


@pytest.mark.parametrize("fam", ["far", "seams", "surface"])
@pytest.mark.parametrize("name", re_.SCENES)
def test_hits_and_misses(oracle, name, fam):
    _, prim, _ = re_.oracle_records(name, fam)
    h, m = shares(prim)
    print(f"{name} {fam}: {prim.size} rays, hits {h:.3f}, misses {m:.3f}")
    assert h >= 0.20 and m >= 0.05, (h, m)


@pytest.mark.parametrize("name", re_.SCENES)
def test_far_cells(oracle, name):
    _, prim, _ = re_.oracle_records(name, "far")
    ri, ki = re_.far_labels()
    assert ri.size == prim.size
    for r in range(len(re_.FAR_R)):
        for k in range(len(re_.FAR_KINDS)):
            h = (prim[(ri == r) & (ki == k)] != NONE).mean()
            print(f"{name} far R={re_.FAR_R[r]:g} {re_.FAR_KINDS[k]}: hits {h:.3f}")
            assert h >= 0.10, (name, re_.FAR_R[r], re_.FAR_KINDS[k], h)


@pytest.mark.parametrize("name", re_.SCENES)
def test_scale(oracle, name):
    _, prim, _ = re_.oracle_records(name, "scale")
    n = prim.size // len(re_.SCALE_K)
    for i, k in enumerate(re_.SCALE_K):
        h, m = shares(prim[i * n:(i + 1) * n])
        print(f"{name} scale 2^{k}: hits {h:.3f}")
        if abs(k) == 20:
            assert h >= 0.20 and m >= 0.05, (k, h, m)


@pytest.mark.parametrize("name", re_.SCENES)
def test_axis(oracle, name):
    rays = re_.family(name, "axis")
    _, prim, _ = re_.oracle_records(name, "axis")
    for g, sl in re_.axis_groups().items():
        hits, misses = int((prim[sl] != NONE).sum()), int((prim[sl] == NONE).sum())
        print(f"{name} axis {g}: hits {hits}, misses {misses}")
        if g in ("zero+", "zero-"):
            d = rays[sl, 3:]
            assert ((d == 0).sum(1) >= 1).all() and (np.signbit(d[d == 0]) == (g == "zero-")).all()
            assert hits == 0, g           # a zero direction component misses everything
        else:
            assert hits >= 16 and misses >= 16, (g, hits, misses)


def test_coplanar_ties_go_to_the_first_primitive(oracle):
    """Every hit on a doubled quad reports the lower-ranked of the primitives that tie: of all slots whose triangle has
    the hit triangle's vertices, the one that comes first in the reference's order."""
    orc = re_.oracle_scene("coplanar")
    tri = orc.world_triangles(orc.primitive_count).reshape(-1, 9)
    order = orc.primitive_order()
    slot_tri = tri[order]                                     # the triangle in each slot of the reference's order
    first_slot = np.array([np.flatnonzero((slot_tri == slot_tri[s]).all(1)).min() for s in range(order.size)])
    assert (np.bincount(first_slot, minlength=order.size)[np.unique(first_slot)] == 4).all()   # each triangle four times
    n_hits = 0
    for fam in ("far", "seams", "surface", "scale"):
        _, prim, _ = re_.oracle_records("coplanar", fam)
        hit = prim[prim != NONE]
        n_hits += hit.size
        assert np.array_equal(first_slot[hit], hit), fam
    assert n_hits > 1000


@pytest.mark.parametrize("name", re_.SCENES)
def test_nonfinite_rays_miss_and_are_few(oracle, name):
    rays = re_.family(name, "nonfinite")
    t, prim, _ = re_.oracle_records(name, "nonfinite")
    bad = ~np.isfinite(rays).all(1)
    assert bad.sum() == min(64, (re_.NONFINITE_AT < rays.shape[0]).sum())
    assert np.isfinite(t).all()                               # a NaN depth never becomes a record
    assert (prim[bad] == NONE).all()                          # (the kernels end such a ray's search at the root: fix_axis)
    h, m = shares(prim[~bad])
    assert h >= 0.20 and m >= 0.05, (h, m)


# ---- the steering test ---------------------------------------------------------------------------------------------------
def test_steering_boxes_keep_every_far_hit(oracle):
    """trace_core.inc slab_fast with the ray's slack, on the padded box of the hit triangle: not one reference hit of the far
    family is rejected, at any of the four distances, on any scene."""
    for name in re_.SCENES:
        for R, (hits, lost) in zip(re_.FAR_R, re_.steering_losses(name, slack=True)):
            print(f"{name} R={R:g}: {hits} reference hits, {lost} rejected by the padded steering box")
            assert hits > 0 and lost == 0, (name, R, hits, lost)


def test_without_the_slack_the_padding_alone_loses_far_hits(oracle):
    """Why the slack is there: the same test without it (the comparison tmax >= tmin && tmax > 0 on boxes whose padding is
    fixed at build time) rejects reference hits once the origin is thousands of scene sizes away, and none at 300."""
    lost_by_r = np.zeros(len(re_.FAR_R), int)
    for name in re_.SCENES:
        for k, (hits, lost) in enumerate(re_.steering_losses(name, slack=False)):
            print(f"{name} R={re_.FAR_R[k]:g}: {hits} reference hits, {lost} rejected without the slack")
            lost_by_r[k] += lost
    assert lost_by_r[2] > 0 and lost_by_r[3] > 0, lost_by_r
