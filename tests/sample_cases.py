"""Triangles and scenes the surface-sampling tests share (tests/test_sample_cpu.py, tests/test_gpu_sample.py,
tests/gpu_sample_probe.py): a soup of 5 000 triangles with log-normal sizes, and a handful of triangles that must never be
drawn.  Everything is fixed: numpy's PCG64 streams of a given seed do not change between versions."""
import math

import numpy as np

from rayca_amd import PbrMaterial, Trs, scenes
from rayca_amd.model import TriangleMesh

SOUP_SLOTS = 5000


def soup_triangles(n=SOUP_SLOTS, seed=20240):
    """(n, 3, 3) f32: centres uniform in [-1, 1]^3, corners = centre + size x uniform offsets, size = 0.02 exp(1.2 N(0, 1)) --
    areas spread over some four decades, so a fifth of the slots carry most of the surface"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, (n, 1, 3))
    size = 0.02 * np.exp(1.2 * rng.standard_normal((n, 1, 1)))
    return (centre + size * rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(np.float32)


def degenerate_triangles():
    """(tris (n, 3, 3) f32, drawable (n,) bool): ordinary triangles among ones whose weight is 0 -- a point, a repeated vertex,
    three collinear vertices, one whose a2 overflows (edges of 5e9: the area is +inf and counts as 0) and one below 2^-32 of the
    largest area.  Every coordinate is an ordinary float: nothing here troubles a tree builder."""
    t, ok = [], []

    def add(a, b, c, drawable):
        t.append([a, b, c])
        ok.append(drawable)
    add((0, 0, 0), (1, 0, 0), (0, 1, 0), True)
    add((2, 2, 2), (2, 2, 2), (2, 2, 2), False)                       # a point
    add((0, 0, 1), (1, 0, 1), (1, 0, 1), False)                       # b == c
    add((-1, -1, -1), (0, 0, 0), (1, 1, 1), False)                    # collinear
    add((0.5, 0.25, 3), (2.5, 0.25, 3), (0.5, 1.75, 3.5), True)       # the largest
    add((0, 0, 0), (5e9, 0, 0), (0, 5e9, 0), False)                   # n = (0, 0, 2.5e19): a2 = +inf
    add((1, 1, 1), (1 + 2e-6, 1, 1), (1, 1 + 2e-6, 1), False)         # area ~ 4e-12 of ~3: below 2^-32 of the largest
    add((-2, 0, 0), (-2, 0.125, 0), (-2, 0, 0.125), True)             # small but drawable
    add((3, 3, 3), (3, 3, 3), (4, 3, 3), False)                       # a == b
    for k in range(7):                                                # enough ordinary ones for more than one leaf
        add((k, -3, 0), (k + 0.5, -3, 0), (k, -3, 0.5 + 0.125 * k), True)
    return np.array(t, np.float32), np.array(ok)


def mesh_scene(tris):
    """one model, one mesh of unshared vertices at the identity; a camera and a point light so that every entry takes it"""
    tris = np.asarray(tris, np.float32)
    tm = TriangleMesh(tris.reshape(-1, 3).copy(), np.arange(tris.shape[0] * 3, dtype=np.uint32))
    return scenes._single_model_scene([(tm, PbrMaterial(color=(1, 1, 1, 1), roughness_factor=1.0))], Trs(translation=(0.0, 0.0, 3.5)),
                                      math.pi / 4, [((0.0, 3.0, 3.0), 64.0)])
