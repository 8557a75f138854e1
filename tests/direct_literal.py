"""The header's text on RaycaDirect (include/rayca_hip.h) in numpy f32: one rounding per operation, in the association the header
writes.  samples() makes every sample of every point -- ray, contribution, class -- from light records (dicts, or the structured
array DeviceScene.lights() returns); fold() sums the lit ones in sample order.  Nothing here traces a ray: `lit` is an input."""
import numpy as np

from sample_literal import rng_f32, rng_root

F = np.float32
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_QUAD = 0, 1, 2
EPS = F(2.0 ** -10)


def _f(x, n=None):
    a = np.asarray(x, F).reshape(-1)
    return a if n is None else a[:n]


def hsum4(a, b, c, d):
    """the ordered four-lane sum of rayca-math, seed -0.0"""
    return (((F(-0.0) + a) + b) + c) + d


def dot(a, b):
    """a, b: (..., 3) f32; the w lane is 0 * 0"""
    return hsum4(a[..., 0] * b[..., 0], a[..., 1] * b[..., 1], a[..., 2] * b[..., 2], F(0) * F(0))


def normalized(v):
    n = np.sqrt(dot(v, v))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where((n > EPS)[..., None], v / n[..., None], v)


def clamp01(v):
    return np.where(v < F(0), F(0), np.where(v > F(1), F(1), v))


def active(p, n=None):
    """the inactive rule: a coordinate that is not finite; with normals also a zero normal or a normal that is not finite"""
    a = np.isfinite(p).all(1)
    if n is not None:
        a &= np.isfinite(n).all(1) & ~(n == 0).all(1)
    return a


def strate_count(light_samples, stratify):
    return int(np.sqrt(F(light_samples))) if stratify else 1


def samples(lights, p, n, *, light_samples=1, stratify=False, seed=0, light_first=0, light_count=None, sample=0, first_index=0, bias=0.0):
    """Every sample of every point.  lights: the WHOLE scene's records (q(li) counts the quad lights in front of li); p: (P, 3)
    f32; n: (P, 3) f32 or None (sphere mode).  Returns a dict: o, omega (P, N, 3), tmax (P, N; +inf for a quad sample), quad (N,)
    bool, y (P, N, 3), dropped, void, traced (P, N) bool, active (P,) bool."""
    p = np.asarray(p, F).reshape(-1, 3)
    sphere = n is None
    if not sphere:
        n = np.asarray(n, F).reshape(-1, 3)
    if light_count is None:
        light_count = len(lights) - light_first
    P, N = p.shape[0], light_count * light_samples
    assert 1 <= N <= 64
    sc_n = strate_count(light_samples, stratify)
    sc = F(sc_n)
    bias = F(bias)
    o = p if sphere else (p + (n * bias).astype(F)).astype(F)
    out = dict(o=np.repeat(o[:, None], N, 1), omega=np.zeros((P, N, 3), F), tmax=np.full((P, N), np.inf, F), quad=np.zeros(N, bool),
               y=np.zeros((P, N, 3), F))
    key = rng_root(seed, (np.uint64(first_index) + np.arange(P, dtype=np.uint64)).astype(np.uint32), sample)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for j in range(N):
            li, k = light_first + j // light_samples, j % light_samples
            L = lights[li]
            kind = int(L["kind"])
            assert kind != LIGHT_DIRECTIONAL
            pos, rgb, alpha, inten = _f(L["position"], 3), _f(L["color"], 3), _f(L["color"])[3], F(L["intensity"])
            if kind == LIGHT_POINT:
                att = _f(L["attenuation"], 3)
                v = (pos - p).astype(F)
                v2 = dot(v, v)
                dist = np.sqrt(v2)
                omega = normalized(v)
                w = (p - pos).astype(F)
                r2 = dot(w, w)
                rr = np.sqrt(r2)
                fallof = hsum4(att[0] * F(1), att[1] * rr, att[2] * r2, F(0) * F(0))
                le = (inten * rgb)[None, :] / fallof[:, None]
                d_omega = F(1) / v2
                out["tmax"][:, j] = dist
            else:
                ab, ac = _f(L["ab"], 3), _f(L["ac"], 3)
                q = sum(1 for m in range(li) if int(lights[m]["kind"]) != LIGHT_POINT)
                D = 2 * (q * light_samples + k)
                u1 = rng_f32(key, D) / sc
                u2 = rng_f32(key, D + 1) / sc
                x1 = (pos[None, :] + u1[:, None] * ab[None, :]) + u2[:, None] * ac[None, :]
                if stratify:
                    x1 = x1 + ((ab / sc) * F(k % sc_n) + (ac / sc) * F(k // sc_n))[None, :]
                v = (x1 - p).astype(F)
                omega = normalized(v)
                le = np.broadcast_to(((inten * rgb) * F(L["area"]))[None, :], (P, 3))
                d_omega = dot(_f(L["normal"], 3)[None, :], omega) / dot(v, v)
                out["quad"][j] = True
            if sphere:
                x = le * d_omega[:, None]
            else:
                x = (le * clamp01(dot(n, omega))[:, None]) * d_omega[:, None]
            out["omega"][:, j] = omega
            out["y"][:, j] = x * alpha
    assert out["y"].dtype == F and out["omega"].dtype == F and out["tmax"].dtype == F
    act = active(p, None if sphere else n)
    out["active"] = act
    out["dropped"] = ~np.isfinite(out["y"]).all(2) & act[:, None]
    out["void"] = (out["y"] == 0).all(2) & ~out["dropped"] & act[:, None]
    out["traced"] = act[:, None] & ~out["dropped"] & ~out["void"]
    return out


def sh9(d):
    """Y_0 .. Y_8 of RaycaGather's comment at directions d (..., 3) f32 -> (..., 9) f32"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full(x.shape, F(0.2820948)), F(0.4886025) * y, F(0.4886025) * z, F(0.4886025) * x, F(1.0925484) * (x * y),
                     F(1.0925484) * (y * z), F(0.3153916) * ((F(3.0) * (z * z)) - F(1.0)), F(1.0925484) * (x * z),
                     F(0.5462742) * ((x * x) - (y * y))], -1).astype(F)


def fold(s, lit, sh=False):
    """s: samples(); lit: (P, N) bool, read for traced samples only.  -> irradiance (P, 4) f32, sh (P, 9, 4) f32 (with sh),
    mask (P,) uint64, counts (P,) uint32"""
    P, N = s["tmax"].shape
    take = np.asarray(lit, bool) & s["traced"]
    e = np.zeros((P, 3), F)
    h = np.zeros((P, 9, 3), F)
    mask = np.zeros(P, np.uint64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(N):
            t = take[:, j]
            y = s["y"][:, j]
            e = np.where(t[:, None], e + y, e)
            if sh:
                yk = sh9(s["omega"][:, j])
                h = np.where(t[:, None, None], h + y[:, None, :] * yk[:, :, None], h)
            mask |= t.astype(np.uint64) << np.uint64(j)
    n_lit = take.sum(1).astype(np.uint32)
    out = {"irradiance": np.concatenate([e, (n_lit.astype(F) / F(N))[:, None]], 1).astype(F), "mask": mask,
           "counts": n_lit | s["dropped"].sum(1).astype(np.uint32) << np.uint32(16)}
    if sh:
        out["sh"] = np.concatenate([h, np.zeros((P, 9, 1), F)], 2).astype(F)
    return out
