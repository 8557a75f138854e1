"""The inputs the ambient-occlusion tests share (helper module; test_ambient_cpu.py checks them against the oracle, test_gpu_ambient.py
runs them): per scene 576 points on its triangles with face normals, the radii and the bias.  Everything is made from hashes of
indices (rayca_amd.scenes.hash_unit), nothing from a random generator's state."""
import numpy as np

import ray_edges as R
from rayca_amd.ambient import cosine_directions

SCENES = ["box", "cornell", "soup1k", "spheres"]
COUNT = 576                       # x 16 samples = 144 batches of 64; x 5 is no multiple of 64
FLT_MAX = np.float32(3.4028234663852886e38)
# the radius of every point, and the bias, in scene diagonals: chosen on the oracle (test_ambient_cpu.py
# test_inputs_leave_both_answers) so that neither answer is rare on any scene
RADIUS_OF_DIAG = {"box": 0.6, "cornell": 0.35, "soup1k": 0.35, "spheres": 0.25}
# Box and the floor of `spheres` are convex and back faces are culled: from a point ON such a surface no ray of either hemisphere
# hits anything, whatever the radius.  There the bias is negative: the origin of a point with a flipped normal lies outside, in
# front of the face it came from, and its rays run into that face; the other half of the points stays unoccluded.
BIAS_OF_DIAG = {"box": -0.05, "cornell": 1e-4, "soup1k": 1e-4, "spheres": -0.02}
INACTIVE = {7: "zero", 100: "minus_zero", 233: "nan_normal", 400: "inf_position", 575: "zero"}   # point index -> what makes it inactive


def table(n=64):
    return cosine_directions(n)


def points_on(tris, count=COUNT, inactive=INACTIVE):
    """(points [count, 3], normals [count, 3]) f32 on the triangles `tris` [n, 3, 3]: hashed triangles, hashed barycentrics, unit face
    normals, every other one flipped; the points of `inactive` made inactive in their several ways"""
    tri = tris[R._pick(301, count, tris.shape[0])]
    w = R._unit(302, count, 3) + 0.05
    w /= w.sum(1, keepdims=True)
    p = (tri * w[:, :, None]).sum(1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[1::2] *= -1.0
    p, nrm = p.astype(np.float32), nrm.astype(np.float32)
    for i, what in inactive.items():
        if what == "zero":
            nrm[i] = 0.0
        elif what == "minus_zero":
            nrm[i] = np.float32(-0.0)
        elif what == "nan_normal":
            nrm[i, 1] = np.nan
        else:
            p[i, 2] = np.inf
    return p, nrm


def points_for(name):
    """(points [576, 3], normals [576, 3], diag) of a scene of ray_edges, five inactive points among them"""
    return R._cached(("ambient points", name), lambda: (*points_on(R.world_triangles(name)), R.bounds(name)[3]))


def inactive_index():
    return np.array(sorted(INACTIVE))


def radius_all(name):
    return np.float32(RADIUS_OF_DIAG[name] * points_for(name)[2])


def radius_per_point(name):
    """per point: NaN, 0, a negative value, +inf, FLT_MAX at the first five of every sixteen points, ordinary values from half to one
    and a half times radius_all elsewhere"""
    i = np.arange(COUNT)
    r = radius_all(name)
    ordinary = (0.5 + R._unit(303, COUNT)[:, 0]) * r
    special = np.array([np.nan, 0.0, -0.5 * r, np.inf, float(FLT_MAX)])
    return np.where(i % 16 < 5, special[i % 16 % 5], ordinary).astype(np.float32)


def bias(name):
    return np.float32(BIAS_OF_DIAG[name] * points_for(name)[2])


def rotations(n=COUNT, seed=304):
    """[n, 2] f32 (cos, sin) of hashed angles"""
    a = 2.0 * np.pi * R._unit(seed, n)[:, 0]
    return np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)
