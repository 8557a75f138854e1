"""Inputs of DeviceScene.ambient (rayca_hip_ambient_device) and DeviceScene.gather (rayca_hip_gather_device) that a host usually
makes once: a table of hemisphere or sphere directions and a per-pixel rotation.  They are plain inputs of the calls -- nothing in
their specifications depends on how they were made -- so they are computed in float64 numpy on the host and cast to float32 at the
end.  And what a host does with gather's nine coefficients: sh9_basis, sh9_irradiance."""
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


def sphere_directions(n: int) -> np.ndarray:
    """(n, 3) float32 unit directions, uniform over the whole sphere and stratified: the centres of cosine_directions' a x b grid
    through the equal-area map z = 1 - 2 u, phi = 2 pi v.  For probes: with these and weights of 4 pi each, gather's "sh" estimates
    the projection of the incoming radiance onto the nine basis functions, which sh9_irradiance takes."""
    if n < 1:
        raise ValueError("n: at least one direction")
    a, b = _grid(n)
    u = (np.arange(a, dtype=np.float64) + 0.5) / a
    v = (np.arange(b, dtype=np.float64) + 0.5) / b
    u, v = (x.reshape(-1) for x in np.meshgrid(u, v, indexing="ij"))
    z, phi = 1.0 - 2.0 * u, 2.0 * np.pi * v
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)


def sh9_basis(d) -> np.ndarray:
    """(..., 9) float64: the real spherical harmonics of bands 0..2 at the unit directions d (..., 3), in gather's order and with
    its signs: 1, y, z, x, xy, yz, 3 z^2 - 1, xz, x^2 - y^2, each with its normalisation."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full(x.shape, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                     1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 0.31539156525252005 * (3.0 * z * z - 1.0),
                     1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)], -1)


def sh9_irradiance(sh, normals) -> np.ndarray:
    """The irradiance at surfaces with unit `normals` (..., 3) under the radiance whose projections onto the nine basis functions
    are `sh` (..., 9, C): the cosine-convolved expansion of Ramamoorthi and Hanrahan 2001, E(n) = sum_k A_l(k) sh_k Y_k(n) with
    A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4.  Returns (..., C) float64.  `sh` are projections, integrals over the sphere: gather's
    "sh" with sphere_directions and weights of 4 pi."""
    band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return np.einsum("...k,...kc->...c", sh9_basis(normals) * band, np.asarray(sh, np.float64))
