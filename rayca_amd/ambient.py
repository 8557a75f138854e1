"""Inputs of DeviceScene.ambient (rayca_hip_ambient_device) that a host usually makes once: a table of hemisphere directions and a
per-pixel rotation.  Both are plain inputs of the call -- nothing in its specification depends on how they were made -- so they are
computed in float64 numpy on the host and cast to float32 at the end."""
import numpy as np


def _grid(n: int):
    """(a, b) with a * b == n, as square as n's divisors allow"""
    a = int(np.floor(np.sqrt(n)))
    while n % a:
        a -= 1
    return a, n // a


def cosine_directions(n: int) -> np.ndarray:
    """(n, 3) float32 unit directions, z along the normal, cosine-weighted over the hemisphere and stratified: the centres of an
    a x b grid on the unit square (a * b == n, as square as n's divisors allow; 8 x 8 for 64) through the polar
    map r = sqrt(u), phi = 2 pi v, z = sqrt(1 - u).  With these, `open` estimates the cosine-weighted visibility directly."""
    if n < 1:
        raise ValueError("n: at least one direction")
    a, b = _grid(n)
    u = (np.arange(a, dtype=np.float64) + 0.5) / a
    v = (np.arange(b, dtype=np.float64) + 0.5) / b
    u, v = (x.reshape(-1) for x in np.meshgrid(u, v, indexing="ij"))
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], 1).astype(np.float32)


def pixel_rotations(width: int, height: int) -> np.ndarray:
    """(height, width, 2) float32 (cos, sin) of a per-pixel angle 2 pi g(x, y), g the interleaved-gradient hash
    frac(52.9829189 frac(0.06711056 x + 0.00583715 y)) (Jimenez 2014): neighbouring pixels turn the direction table by different
    angles, which trades the banding of a shared table for noise a spatial filter removes."""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64), indexing="xy")
    g = np.mod(52.9829189 * np.mod(0.06711056 * x + 0.00583715 * y, 1.0), 1.0)
    angle = 2.0 * np.pi * g
    return np.stack([np.cos(angle), np.sin(angle)], -1).astype(np.float32)
