"""The inputs the irradiance-gathering tests share (helper module; test_gather_cpu.py, test_gpu_gather.py): tests/ambient_cases.py's
576 points per scene with its five inactive ones, a bias per scene, the Configs, and a table of 64 weights.  Everything is made from
hashes of indices, nothing from a random generator's state."""
import numpy as np

import ambient_cases as ac
import ray_edges as R
from rayca_amd import Config, IntegratorStrategy

SCENES = ["cornell", "box", "spheres"]
COUNT = ac.COUNT
SAMPLE_COUNTS = (1, 5, 16, 64)
# Every other normal of ambient_cases is flipped.  In the Cornell room the rays of a point with an unflipped normal run into the room,
# where the light is; the bias lifts the origin off the wall (in scene diagonals).  Box and `spheres` are convex bodies seen from
# outside: whatever the bias, a ray either leaves the scene or runs into the body it started on.
BIAS_OF_DIAG = {"cornell": 1e-3, "box": 1e-3, "spheres": 1e-3}
CONFIGS = {
    "flat": Config(integrator=IntegratorStrategy.Flat),
    "depth1": Config(max_depth=1),                      # Pathtracer, NEE: direct light alone
    "depth3": Config(max_depth=3, seed=5),              # ... and two cosine bounces
}
PATH_TRACED = ("depth1", "depth3")


def points_for(name):
    """(points [576, 3], normals [576, 3], diag): ambient_cases', five inactive points among them"""
    return ac.points_for(name)


def bias(name):
    return np.float32(BIAS_OF_DIAG[name] * points_for(name)[2])


def table(n=64):
    return ac.table(n)


def rotations(n=COUNT):
    return ac.rotations(n)


def weights(n=64, seed=601):
    """[n] f32 in [0.5, 1.5): hashed, none of them 1"""
    return (0.5 + R._unit(seed, n)[:, 0]).astype(np.float32)


def meaningful(irradiance, kept, act, samples):
    """the condition a path-traced cornell case must meet on its EXPECTED values: at least a quarter of the active points with a
    non-zero E, and at least a quarter with every sample kept.  Returns the two fractions."""
    lit = float((irradiance[act, :3] != 0).any(1).mean())
    full = float((kept[act] == samples).mean())
    return lit, full
