"""The shading arithmetic in float64, from the reference's formulas (brdf/ggx.rs, brdf/lambertian.rs, sampler/nee.rs,
light/point.rs and the oracle's citations of them), and the bound a float32 evaluation of it is held to.

What is computed.  A Pathtracer with max_depth = 1, NEE, one light sample and gamma = 1 returns at a non-emissive hit the sum of
its lights' Sample.x; the Whitted Raytracer at depth 1 returns get_color() plus get_radiance() summed over the lights.  Both are
functions of the hit's float32 surface record (point, shading normal, view vector, diffuse, specular, roughness, shininess, kind),
of the light and of nothing else: no random draw with a point or a directional light.  From those float32 inputs this module
computes the pixel in float64 with the MATHEMATICAL formulas -- D = a^2 / (pi cos^4 (a^2 + tan^2)^2), G1 = 2 / (1 + sqrt(1 + a^2
tan^2)) with tan = tan(acos c), F = ks + (1 - ks)(1 - |wi.h|)^5, powf as numpy's float64 power -- never the kernels' closed forms.
Special values follow IEEE as numpy gives them: a negative base with a non-integer exponent is NaN, acos of a cosine above 1 is
NaN, 0 * inf is NaN.  The reference's own quirks are part of the formulas: `normalize` leaves a vector of length <= 2^-10 as it
is (vec3.rs:183-188), D is 0 where its denominator is (ggx.rs:63-65), the bsdf is black where a clamped cosine is 0.

`closed_form_f32` is something else: the numpy-float32 restatement, operation by operation, of what trace_core.inc's header
specifies (the closed forms of RAYCA_GGX_CLOSED_FORM, the Phong lobe, nee_prepare's point-light arm).  It is the "reference alone"
the bound's constants were settled against on the CPU; it is not an expected value for any device output.

The bound.  float32 inputs leave some points ill-conditioned -- D next to the mirror direction at low roughness, h where wi + wo
nearly cancels -- so the tolerance is a conditioning bound taken from the float64 program itself.  The pixel is written as a
function of its cosines; it is evaluated at the nominal cosines and at every corner of c +- delta:

    n.wi, n.wo                          delta = DELTA0
    n.h, wi.h                           delta = DELTA0 (1 + 2 / |wi + wo|)     (the cancellation in the half vector)
    r.wi (the base of the Phong powf)   delta = DELTA_R = 3 DELTA0

and the envelope of the corner values, widened by EPS * max|corner value| for the chain of products, is what a float32 evaluation
has to lie in.  Corners that are not finite are left out of the envelope; a pixel whose nominal value is finite while a corner is
not (or the other way round) sits on the edge of a special case -- r.wi within delta of 0 under a non-integer shininess, n.wo
within delta of 1 -- and is `undecided`: counted, not compared.  A pixel whose envelope is wider than WIDE = 1e-2 of its value
says nothing: `wide`, counted, not compared.  A pixel whose nominal value is NaN or infinite is `special`: the sets are
compared, not the values.

The constants.  A priori: a cosine is a normalize (three products, two sums, a root, three quotients) and a three-term dot of
values <= 1, fewer than eight roundings of at most 2^-25 each, so DELTA0 <= 4 * 2^-24; between the cosines and the pixel lie
about twenty float32 operations (falloff, le, the brdf's products and quotients, the fold) of 2^-24 each, three times that where an
operand is itself a rounded sum (1 - c, 1 + c, a^2 c^2 + ...), so EPS <= 4e-6; reflect is one more dot, scale and subtraction of
unit vectors, then a normalize, then the dot: DELTA_R a small multiple of DELTA0.  Those are worst cases that add every rounding
with the same sign.  The values below are the smallest on the halving ladders DELTA0 = 4, 2, 1, 1/2 x 2^-24, DELTA_R = 4, 3, 2,
1 x DELTA0, EPS = 4, 2, 1, 0.5, 0.25 x 1e-6 at which `closed_form_f32` -- with powf as the host computes it and moved one
float32 step up and down, the accuracy HIP documents for the device's powf -- lies inside at every kept point of families A, B,
C and F of shading_cases.py (test_shading_cpu.py asserts it, and that one step down in any of the three lets it out; 79 014 kept
points of 79 236):

    DELTA0 = 2^-24      at 2^-25 (DELTA_R with it) it leaves at 101 points of A and B
    DELTA_R = 3 DELTA0  at 2 DELTA0 it leaves at 17 Phong points: shininess 1000, and next to r.wi = 0 (B: 45 degrees retro, telephoto)
    EPS = 5e-7          at 2.5e-7 it leaves at 398 steep points of A and B (the chain is about eight roundings deep, not twenty)

With them the worst point of `closed_form_f32` sits at 0.97 of its half envelope (B, telephoto, shininess 1000: the envelope there is
DELTA_R's), the steep points at 0.7 to 0.9 of half envelopes of 6e-7 relative.  The oracle's own frames of B and C, where it spells
what the literal spells, lie inside everywhere as well.  No device output took part in any of this.
"""
import itertools
import math

import numpy as np

DELTA0 = 2.0 ** -24
DELTA_R = 3.0 * DELTA0
EPS = 5e-7
WIDE = 1e-2
NORMALIZE_EPS = 2.0 ** -10      # rayca-math lib.rs:33: FLT_EPSILON * 8192

PHONG, GGX, PBR = "phong", "ggx", "pbr"      # the kinds a record carries (shading_cases.kind_names maps the descriptor's)
POINT, DIRECTIONAL = "point", "directional"


# ---- float64: vectors ------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a * b).sum(-1)


def normalize(v):
    """Vec3::normalize: only when the length exceeds 2^-10"""
    n = np.sqrt(dot(v, v))
    with np.errstate(all="ignore"):
        return np.where((n > NORMALIZE_EPS)[..., None], v / n[..., None], v)


def reflect(a, n):
    return a - 2.0 * dot(a, n)[..., None] * n


def clamp01(c):
    """f32::clamp(0, 1): NaN stays NaN"""
    return np.where(c < 0.0, 0.0, np.where(c > 1.0, 1.0, c))


# ---- float64: the terms, as functions of cosines -----------------------------------------------------------------------------
def ggx_d(a, c):
    """ggx.rs:58-67 with c = h.n"""
    c = clamp01(c)
    with np.errstate(all="ignore"):
        den = c ** 4 * (a * a + np.tan(np.arccos(c)) ** 2) ** 2
        return np.where(den == 0.0, 0.0, a * a / math.pi / den)


def ggx_g1(a, c):
    """ggx.rs:74-83 with c = omega.n, not clamped: above 1 acos is NaN"""
    with np.errstate(all="ignore"):
        return np.where(c <= 0.0, 0.0, 2.0 / (1.0 + np.sqrt(1.0 + a * a * np.tan(np.arccos(c)) ** 2)))


def ggx_f(ks, c):
    """ggx.rs:100-103 with c = omega_i.h; ks (..., 3)"""
    return ks + (1.0 - ks) * ((1.0 - np.abs(c)) ** 5)[..., None]


def ggx_brdf(kd, ks, a, ci, co, ch, cih):
    """kd / pi + F G1 G1 D / (4 ci co)  (ggx.rs:106-129); rgb (..., 3)"""
    cic, coc = clamp01(ci), clamp01(co)
    with np.errstate(all="ignore"):
        bsdf = ggx_f(ks, cih) * (ggx_g1(a, ci) * ggx_g1(a, co) * ggx_d(a, ch) / (4.0 * cic * coc))[..., None]
    black = (cic == 0.0) | (coc == 0.0)
    return kd / math.pi + np.where(black[..., None], 0.0, bsdf)


def phong_brdf(kd, ks, sh, rdot):
    """kd / pi + ks (sh + 2) (r.omega)^sh / 2 pi  (lambertian.rs:7-16)"""
    with np.errstate(all="ignore"):
        lobe = np.power(rdot, sh)
    return kd / math.pi + ks * ((sh + 2.0) * lobe / (2.0 * math.pi))[..., None]


def falloff(att, r):
    """point.rs:41-49"""
    return att[0] + att[1] * r + att[2] * r * r


def point_sample(le, att, r, brdf, ci):
    """Sample.x of get_point_light_sample (nee.rs:127-166): the light's falloff, the reference's extra 1 / r^2, the clamped n.omega"""
    with np.errstate(all="ignore"):
        return (le / falloff(att, r)[..., None]) * brdf * clamp01(ci)[..., None] / (r * r)[..., None]


def whitted_radiance(kind, kd, ks, sh, rough, metallic, albedo, albedo_alpha, intensity, cv, cl, ch, clh):
    """get_radiance of both BRDF modules (ggx.rs:33-52, lambertian.rs:76-81) on Irradiance::new's cosines (hit.rs:263-287);
    albedo = get_color()'s rgb, which F0 takes premultiplied by its alpha (Vec3::from(&Color)) and the diffuse term as it is.
    kind is one string for the whole batch."""
    n_dot_v, n_dot_l, n_dot_h, l_dot_h = clamp01(cv) + 1e-5, clamp01(cl), clamp01(ch), clamp01(clh)
    with np.errstate(all="ignore"):
        if kind == PHONG:
            return (kd * n_dot_l[..., None] + ks * np.power(n_dot_h, sh)[..., None]) * intensity
        a = n_dot_h * rough
        k = rough / (1.0 - n_dot_h * n_dot_h + a * a)
        d = k * k / math.pi
        f0 = 0.04 * (1.0 - metallic)[..., None] + albedo * (albedo_alpha * metallic)[..., None]
        f = f0 + (1.0 - f0) * ((1.0 - l_dot_h) ** 5)[..., None]
        k_d = (1.0 - f) * (1.0 - metallic)[..., None]
        ggxv = n_dot_l * (n_dot_v * (1.0 - rough) + rough)
        ggxl = n_dot_v * (n_dot_l * (1.0 - rough) + rough)
        g = 0.5 / (ggxv + ggxl)
        return ((k_d * albedo / math.pi + (d * g)[..., None] * f) * intensity) * n_dot_l[..., None]


# ---- float64: one light at the records of a frame ---------------------------------------------------------------------------
def _f64(rec, *names):
    return [np.asarray(rec[k], np.float64) for k in names]


def light_terms(rec, light, whitted=False):
    """The cosines of one light at every record, their deltas, and the function of the cosines that is the light's term of the
    pixel (rgb, before the fold's alpha).  Returns (cosines (K, N), deltas (K, N), evaluate(cosines) -> (N, 3), alpha (N,))."""
    p, n, wo, kd4, ks4 = _f64(rec, "point", "normal", "view", "diffuse", "specular")
    rough, sh = _f64(rec, "roughness", "shininess")
    # Color + Color and Color - Color weigh the right operand by its alpha, also inside the BRDFs (ks + (white - ks) x^5, lambertian +
    # specular): with material alphas of 1 those are the plain formulas, and only the light colour's alpha is left to carry
    hit = np.asarray(rec["hit"], bool)
    assert (kd4[hit, 3] == 1.0).all() and (ks4[hit, 3] == 1.0).all() and (np.asarray(rec["color"])[hit, 3] == 1.0).all()
    kd, ks = kd4[:, :3], ks4[:, :3]
    color = np.asarray(light["color"], np.float64)
    le = float(light["intensity"]) * color[:3]
    if light["kind"] == POINT:
        to_light = np.asarray(light["position"], np.float64) - p
        r = np.sqrt(dot(to_light, to_light))
        wi = normalize(to_light)
    else:
        wi = np.broadcast_to(np.asarray(light["direction"], np.float64), p.shape)
        r = None
    with np.errstate(all="ignore"):
        half = wi + wo
        half_len = np.sqrt(dot(half, half))
        h = normalize(half)
        d_half = DELTA0 * (1.0 + 2.0 / half_len)
    d0 = np.full(p.shape[0], DELTA0)
    kinds = rec["kind"]
    if whitted:
        metallic, albedo = _f64(rec, "metallic", "color")
        att = np.asarray(light["attenuation"], np.float64)
        with np.errstate(all="ignore"):
            intensity = le if light["kind"] == DIRECTIONAL else le / falloff(att, r)[:, None]
        cos = np.stack([dot(n, wo), dot(n, wi), dot(n, h), dot(wi, h)])
        deltas = np.stack([d0, d0, d_half, d_half])

        def evaluate(c):
            out = np.zeros((p.shape[0], 3))
            for kind in (PHONG, PBR):
                m = kinds == kind
                if m.any():
                    out[m] = whitted_radiance(kind, kd[m], ks[m], sh[m], rough[m], metallic[m], albedo[m, :3], albedo[m, 3], np.broadcast_to(intensity, kd.shape)[m],
                                              c[0][m], c[1][m], c[2][m], c[3][m])
            return out
        # (fd + fr) * intensity: Color * Color multiplies the alphas; get_color()'s alpha enters through fd's `* albedo`
        alpha = np.where(kinds == PHONG, kd4[:, 3], np.asarray(rec["color"], np.float64)[:, 3]) * color[3]
        return cos, deltas, evaluate, alpha
    att = np.asarray(light["attenuation"], np.float64)
    refl = normalize(reflect(-wo, n))
    phong = kinds == PHONG
    # rows: n.wi, n.wo, then (n.h, wi.h) for the GGX kinds and (r.wi, unused) for Phong
    cos = np.stack([dot(n, wi), dot(n, wo), np.where(phong, dot(refl, wi), dot(n, h)), np.where(phong, 0.0, dot(wi, h))])
    deltas = np.stack([d0, d0, np.where(phong, DELTA_R, d_half), np.where(phong, 0.0, d_half)])

    def evaluate(c):
        brdf = np.where(phong[:, None], phong_brdf(kd, ks, sh, c[2]), ggx_brdf(kd, ks, rough, c[0], c[1], c[2], c[3]))
        return point_sample(le, att, r, brdf, c[0])
    return cos, deltas, evaluate, kd4[:, 3] * color[3]


KEPT, TOO_WIDE, UNDECIDED, SPECIAL, MISS = 0, 1, 2, 3, 4


def pixel(rec, lights, visible, whitted=False):
    """The frame's pixels in float64 with their bound.  `visible[l]`: per record, whether light l's shadow ray is free (an
    occluded sample is black).  Lights fold the way Color + Color does: rgb + b.rgb * b.a.  A Whitted pixel starts from
    get_color().  Returns dict(value, lo, hi (N, 3), status (N,) of KEPT / TOO_WIDE / UNDECIDED / SPECIAL / MISS)."""
    n = rec["point"].shape[0]
    base = np.asarray(rec["color"], np.float64)[:, :3] if whitted else np.zeros((n, 3))
    value, lo, hi = base.copy(), base.copy(), base.copy()
    mag = np.abs(base)
    undecided = np.zeros(n, bool)
    for light, vis in zip(lights, visible):
        cos, deltas, evaluate, alpha = light_terms(rec, light, whitted)
        with np.errstate(all="ignore"):
            nominal = evaluate(cos) * alpha[:, None]
            l_lo, l_hi, l_mag = nominal.copy(), nominal.copy(), np.abs(nominal)
            l_undecided = np.zeros(n, bool)
            for signs in itertools.product((-1.0, 1.0), repeat=cos.shape[0]):
                if any(s > 0 and not deltas[k].any() for k, s in enumerate(signs)):
                    continue   # (a cosine without a delta has one corner, not two)
                corner = evaluate(cos + np.array(signs)[:, None] * deltas) * alpha[:, None]
                finite = np.isfinite(corner)
                l_undecided |= (finite != np.isfinite(nominal)).any(1)
                l_lo = np.where(finite, np.fmin(l_lo, corner), l_lo)
                l_hi = np.where(finite, np.fmax(l_hi, corner), l_hi)
                l_mag = np.where(finite, np.fmax(l_mag, np.abs(corner)), l_mag)
        lit = np.asarray(vis, bool)[:, None]
        undecided |= l_undecided & lit[:, 0]
        value = value + np.where(lit, nominal, 0.0)
        lo, hi, mag = lo + np.where(lit, l_lo, 0.0), hi + np.where(lit, l_hi, 0.0), mag + np.where(lit, l_mag, 0.0)
    if whitted:   # the frame adds the sample to black: rgb * get_color()'s alpha
        a = np.asarray(rec["color"], np.float64)[:, 3:]
        value, lo, hi, mag = value * a, lo * a, hi * a, mag * a
    hit = np.asarray(rec["hit"], bool)
    value, lo, hi = (np.where(hit[:, None], a, 0.0) for a in (value, lo, hi))
    with np.errstate(invalid="ignore"):
        lo, hi = lo - EPS * mag, hi + EPS * mag
    special = ~np.isfinite(value).all(1)
    with np.errstate(all="ignore"):
        wide = ((hi - lo) > WIDE * np.abs(value)).any(1) & ~special
    status = np.full(n, KEPT)
    status[wide] = TOO_WIDE
    status[undecided & hit & ~special] = UNDECIDED
    status[special] = SPECIAL
    status[~hit] = MISS
    return dict(value=value, lo=lo, hi=hi, status=status)


def judge(got, want):
    """`got` (N, 3) float32 pixels against pixel()'s record.  Returns dict(outside: kept pixels with a channel outside the
    envelope, special_differs: special pixels whose NaN / inf pattern (with the infinities' signs) differs from the float64
    value's, worst: the largest distance of a kept channel from the nominal value in units of its half envelope,
    kept / wide / undecided / special / miss: counts)."""
    got = np.asarray(got, np.float64)
    st = want["status"]
    kept = st == KEPT
    with np.errstate(all="ignore"):
        out = ((got < want["lo"]) | (got > want["hi"]) | ~np.isfinite(got)).any(1) & kept
        half = np.maximum(want["hi"] - want["value"], want["value"] - want["lo"])
        units = np.where(half > 0.0, np.abs(got - want["value"]) / half, np.where(got == want["value"], 0.0, np.inf))
    sp = st == SPECIAL
    v = want["value"]
    same = (np.isnan(got) == np.isnan(v)) & (np.isinf(got) == np.isinf(v)) & (np.isnan(v) | ~np.isinf(v) | (np.sign(got) == np.sign(v)))
    differs = sp & ~same.all(1)
    return dict(outside=np.flatnonzero(out), special_differs=np.flatnonzero(differs), worst=float(units[kept].max()) if kept.any() else 0.0,
                kept=int(kept.sum()), wide=int((st == TOO_WIDE).sum()), undecided=int((st == UNDECIDED).sum()), special=int(sp.sum()),
                miss=int((st == MISS).sum()))


# ---- float32: the header's arithmetic, operation by operation ----------------------------------------------------------------
F = np.float32
FRAC_1_PI = F(0.318309873342514038086)
MUTANTS = ("fresnel_x4", "g1_without_one", "d_without_guard", "g1_zero_above_one", "phong_sh_plus_one", "falloff_without_r",
           "second_r2_dropped")


def dot32(a, b):
    """ordered lane sum from -0.0, no FMA (rayca_math.hpp hsum / dot); w lanes are 0"""
    t = a * b
    return ((F(-0.0) + t[..., 0]) + t[..., 1]) + t[..., 2]


def normalized32(a):
    with np.errstate(all="ignore"):
        n = np.sqrt(dot32(a, a))
        return np.where((n > F(NORMALIZE_EPS))[..., None], a / n[..., None], a)


def clamp32(v):
    return np.where(v < F(0), F(0), np.where(v > F(1), F(1), v))


def ggx_d32(a, c, mutant=None):
    """ggx_d of trace_core.inc under RAYCA_GGX_CLOSED_FORM, c = dot(h, n)"""
    a2 = a * a
    c = clamp32(c)
    q = a2 * (c * c) + (F(1) - c) * (F(1) + c)
    den = q * q
    with np.errstate(all="ignore"):
        d = a2 * FRAC_1_PI / den
    zero = (den == F(0)) if mutant == "d_without_guard" else (den == F(0)) | (c == F(0))
    return np.where(zero, F(0), d).astype(F)


def ggx_g132(a, c, mutant=None):
    with np.errstate(all="ignore"):
        tan2 = np.where(c > F(1), F(0) if mutant == "g1_zero_above_one" else F(np.nan), ((F(1) - c) * (F(1) + c)) / (c * c))
        one = F(0) if mutant == "g1_without_one" else F(1)
        g = F(2) / (F(1) + np.sqrt(one + a * a * tan2))
    if mutant == "g1_zero_above_one":
        g = np.where(c > F(1), F(0), g)
    return np.where(c <= F(0), F(0), g).astype(F)


def ggx_f32(ks, c, mutant=None):
    x = F(1) - np.abs(c)
    x2 = x * x
    p = (x2 * x2) if mutant == "fresnel_x4" else (x2 * x2) * x
    return ks + (F(1) - ks) * p[..., None]


TERM_ROUGHNESSES = (1.0, 0.5, 0.1, 0.02, 1e-3)
U = 2.0 ** -24     # the unit roundoff of float32


def term_accuracy():
    """The largest relative error of each GGX term against float64 over float32 cosines from 1e-4 to 1 - 6e-8 (4000 of them,
    crowded towards both ends) and TERM_ROUGHNESSES, for the closed forms and for the reference's libm spelling evaluated in
    numpy float32 (tan(acos c)^2, pow(c, 4), pow(x, 5)): what the header above ggx_d states, measured.  A priori, counting
    roundings of U = 2^-24 along the longest path: the closed D <= 13 U (q in four, squared, a^2 / pi in three, the quotient), the
    closed G1 <= 8 U, x^5 <= 4 U."""
    c = np.unique(np.concatenate([np.geomspace(1e-4, 0.5, 2000), 1.0 - np.geomspace(6e-8, 0.5, 2000)]).astype(F))
    c64 = c.astype(np.float64)
    out = {k: 0.0 for k in ("d_closed", "g1_closed", "x5_closed", "d_libm", "g1_libm", "x5_libm")}

    def rel(got, want):
        return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))
    with np.errstate(all="ignore"):
        for r in TERM_ROUGHNESSES:
            a, a2 = F(r), F(r) * F(r)
            tan2 = np.power(np.tan(np.arccos(c)), F(2))
            out["d_closed"] = max(out["d_closed"], rel(ggx_d32(a, c), ggx_d(float(a), c64)))
            out["g1_closed"] = max(out["g1_closed"], rel(ggx_g132(a, c), ggx_g1(float(a), c64)))
            out["d_libm"] = max(out["d_libm"], rel(a2 * FRAC_1_PI / (np.power(c, F(4)) * np.power(a2 + tan2, F(2))), ggx_d(float(a), c64)))
            out["g1_libm"] = max(out["g1_libm"], rel(F(2) / (F(1) + np.sqrt(F(1) + a * a * tan2)), ggx_g1(float(a), c64)))
        x = F(1) - c
        x2 = x * x
        out["x5_closed"] = rel((x2 * x2) * x, x.astype(np.float64) ** 5)
        out["x5_libm"] = rel(np.power(x, F(5)), x.astype(np.float64) ** 5)
    return out


def closed_form_f32(rec, lights, visible, mutant=None, pow_ulps=0):
    """The Pathtracer pixel (max_depth 1, NEE, point lights) as the header spells it: nee_prepare's point-light arm, surf_brdf,
    the closed forms.  (N, 3) float32.  `pow_ulps`: powf's result moved that many float32 steps up or down -- the one operation
    of the chain that no library rounds correctly; HIP documents 1 ulp for the device's."""
    assert mutant is None or mutant in MUTANTS
    p, n, wo = (np.asarray(rec[k], F) for k in ("point", "normal", "view"))
    kd4, ks4 = np.asarray(rec["diffuse"], F), np.asarray(rec["specular"], F)
    kd, ks = kd4[:, :3], ks4[:, :3]
    a, sh = np.asarray(rec["roughness"], F), np.asarray(rec["shininess"], F)
    phong = rec["kind"] == PHONG
    total = np.zeros((p.shape[0], 3), F)
    with np.errstate(all="ignore"):
        for light, vis in zip(lights, visible):
            x1 = np.asarray(light["position"], F)
            to = x1[None, :] - p
            omega = normalized32(to)
            dvec = p - x1[None, :]
            r2 = dot32(dvec, dvec)
            rr = np.sqrt(r2)
            att = [F(v) for v in light["attenuation"]]
            t = [att[0] * F(1), att[1] * (F(0) * rr if mutant == "falloff_without_r" else rr), att[2] * r2]
            fall = ((F(-0.0) + t[0]) + t[1]) + t[2]
            color = np.asarray(light["color"], F)
            le = (F(light["intensity"]) * color[:3])[None, :] / fall[:, None]
            # surf_brdf
            refl = normalized32((-wo) - (F(2) * dot32(-wo, n))[:, None] * n)
            shp = sh + (F(1) if mutant == "phong_sh_plus_one" else F(2))
            lobe = np.power(dot32(refl, omega), sh).astype(F)
            for _ in range(abs(pow_ulps)):
                lobe = np.nextafter(lobe, F(np.inf if pow_ulps > 0 else -np.inf))
            b_phong = kd * FRAC_1_PI + (((ks * shp[:, None]) * lobe[:, None]) * FRAC_1_PI) / F(2)
            oin, oon = clamp32(dot32(omega, n)), clamp32(dot32(wo, n))
            h = normalized32(omega + wo)
            f = ggx_f32(ks, dot32(omega, h), mutant)
            g = ggx_g132(a, dot32(omega, n), mutant) * ggx_g132(a, dot32(wo, n), mutant)
            d = ggx_d32(a, dot32(h, n), mutant)
            bsdf = ((f * g[:, None]) * d[:, None]) / (F(4) * oin * oon)[:, None]
            b_ggx = kd * FRAC_1_PI + np.where(((oin == F(0)) | (oon == F(0)))[:, None], F(0), bsdf)
            brdf = np.where(phong[:, None], b_phong, b_ggx)
            r_squared = dot32(to, to)
            d_omega = F(1) if mutant == "second_r2_dropped" else F(1) / r_squared
            x = ((le * brdf) * clamp32(dot32(n, omega))[:, None]) * (d_omega * np.ones_like(r2))[:, None]
            alpha = color[3] * kd4[:, 3]
            total = total + np.where(np.asarray(vis, bool)[:, None], x * alpha[:, None], F(0))
    return np.where(np.asarray(rec["hit"], bool)[:, None], total, F(0)).astype(F)
