"""The temporal accumulation of rayca_hip_accumulate_device, restated literally in numpy float32 from its specification
(include/rayca_hip.h) -- not from the kernel.  Vectorised over pixels, a Python loop over the four taps in the stated
order (j = 0, 1 outer, i = 0, 1 inner); every operation is one float32 operation, in the association the specification writes, so
under the library's arithmetic contract (no contraction, no fast math) the kernel gives the same bits.

min() / max() are minNum / maxNum (np.fmin / np.fmax); every comparison is one a NaN fails.

A pose is a dict of float32: origin, right, up, back (3,) and angle -- the fields of RaycaCameraPose."""
import numpy as np

F = np.float32


def pose_from_abi(p):
    return dict(origin=np.array(list(p.origin), F), right=np.array(list(p.right), F), up=np.array(list(p.up), F),
                back=np.array(list(p.back), F), angle=F(p.angle))


def make_pose(origin, yaw=0.0, pitch=0.0, yfov=0.9, scale=(1.0, 1.0, 1.0)):
    """A camera at `origin` looking down -z, turned by yaw about y and then pitch about its x axis (radians): the pose
    rayca_hip_scene_camera would report for that node, formed in float64 and rounded once."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    r = ry @ rx
    return dict(origin=np.array(origin, F), right=(r[:, 0] / scale[0]).astype(F), up=(r[:, 1] / scale[1]).astype(F),
                back=(r[:, 2] / scale[2]).astype(F), angle=F(np.tan(yfov * 0.5)))


def forward_basis(pose):
    """the columns of R S in float64: e with e . right = 1 along right, and so on (right = R e_x / s_x, so R e_x s_x = right / |right|^2)"""
    out = []
    for k in ("right", "up", "back"):
        v = pose[k].astype(np.float64)
        out.append(v / v.dot(v))
    return out


def project(pose, point, width, height):
    """(fx, fy, ok) of world points (..., 3) float32 in the view of `pose`, as the specification writes it: ok = cz < 0"""
    o, r, u, b = pose["origin"], pose["right"], pose["up"], pose["back"]
    fw, fh = F(width), F(height)
    with np.errstate(all="ignore"):
        v0, v1, v2 = point[..., 0] - o[0], point[..., 1] - o[1], point[..., 2] - o[2]
        cx = (r[0] * v0 + r[1] * v1) + r[2] * v2
        cy = (u[0] * v0 + u[1] * v1) + u[2] * v2
        cz = (b[0] * v0 + b[1] * v1) + b[2] * v2
        ok = cz < F(0.0)
        nz = F(0.0) - cz
        aspect = fw / fh
        fx = ((cx / nz) / (pose["angle"] * aspect) + F(1.0)) * F(0.5) * fw - F(0.5)
        fy = (F(1.0) - (cy / nz) / pose["angle"]) * F(0.5) * fh - F(0.5)
    assert fx.dtype == F and fy.dtype == F
    return fx, fy, ok


def luminance(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def accumulate(color, *, history=None, prev=None, prev_camera=None, point=None, normal=None, id=None, max_history=0, normal_min=0.9,
               plane_max=0.1, moments=None):
    """The whole call: a dict color (H, W, 4), length (H, W) and, with moments, moments (H, W, 2) and variance (H, W), float32.
    history: None or a dict color, length[, moments]; prev: normal[, point][, id] of the frame the history belongs to."""
    c = np.ascontiguousarray(color, F)
    assert c.ndim == 3 and c.shape[2] == 4
    hgt, wid = c.shape[:2]
    if moments is None:
        moments = history is None or "moments" in history
    assert not (moments and history is not None and "moments" not in history)
    assert (prev_camera is None) == (point is None) == (normal is None)
    prev = prev or {}
    assert (id is None) == ("id" not in prev)
    zero = F(0.0)
    with np.errstate(all="ignore"):
        d = c - c
        finite = (d[..., 0] == zero) & (d[..., 1] == zero) & (d[..., 2] == zero) & (d[..., 3] == zero)
        lum = luminance(c)
        present = np.zeros((hgt, wid), bool)
        h = np.zeros((hgt, wid, 4), F)
        length = np.zeros((hgt, wid), F)
        m = np.zeros((hgt, wid, 2), F)
        if history is not None and prev_camera is None:
            hl = np.asarray(history["length"], F)
            present = hl > zero
            h = np.where(present[..., None], np.asarray(history["color"], F), zero)
            length = np.where(present, hl, zero)
            if moments:
                m = np.where(present[..., None], np.asarray(history["moments"], F), zero)
        elif history is not None:
            assert normal_min > 0 and ("point" not in prev or plane_max > 0)
            hc, hl = np.asarray(history["color"], F), np.asarray(history["length"], F)
            hm = np.asarray(history["moments"], F) if moments else None
            nq_all = np.asarray(prev["normal"], F)
            n0, n1, n2 = normal[..., 0], normal[..., 1], normal[..., 2]
            ok = ~((n0 == zero) & (n1 == zero) & (n2 == zero))
            fx, fy, front = project(prev_camera, point, wid, hgt)
            ok &= front
            ok &= (fx >= F(-1.0)) & (fx < F(wid)) & (fy >= F(-1.0)) & (fy < F(hgt))
            x0f, y0f = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0f, fy - y0f
            x0 = np.where(ok, x0f, zero).astype(np.int64)
            y0 = np.where(ok, y0f, zero).astype(np.int64)
            wsum = np.zeros((hgt, wid), F)
            sc = np.zeros((hgt, wid, 4), F)
            sl = np.zeros((hgt, wid), F)
            sm = np.zeros((hgt, wid, 2), F)
            for j in (0, 1):
                for i in (0, 1):
                    qy, qx = y0 + j, x0 + i
                    take = ok & (qy >= 0) & (qy < hgt) & (qx >= 0) & (qx < wid)
                    qy, qx = np.clip(qy, 0, hgt - 1), np.clip(qx, 0, wid - 1)
                    b = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                    take &= b > zero
                    lq = hl[qy, qx]
                    take &= lq > zero
                    if id is not None:
                        take &= np.asarray(prev["id"])[qy, qx] == id
                    nq = nq_all[qy, qx]
                    take &= ((n0 * nq[..., 0] + n1 * nq[..., 1]) + n2 * nq[..., 2]) >= F(normal_min)
                    if "point" in prev:
                        e = np.asarray(prev["point"], F)[qy, qx] - point
                        pd = (n0 * e[..., 0] + n1 * e[..., 1]) + n2 * e[..., 2]
                        take &= np.abs(pd) <= F(plane_max)
                    wsum = np.where(take, wsum + b, wsum)
                    hq = hc[qy, qx]
                    for k in range(4):
                        sc[..., k] = np.where(take, sc[..., k] + b * hq[..., k], sc[..., k])
                    sl = np.where(take, sl + b * lq, sl)
                    if moments:
                        mq = hm[qy, qx]
                        for k in range(2):
                            sm[..., k] = np.where(take, sm[..., k] + b * mq[..., k], sm[..., k])
            present = wsum > zero
            h = np.where(present[..., None], sc / wsum[..., None], zero)
            length = np.where(present, sl / wsum, zero)
            if moments:
                m = np.where(present[..., None], sm / wsum[..., None], zero)
        # blend
        n = length + F(1.0)
        if max_history > 0:
            n = np.fmin(n, F(max_history))
        a = F(1.0) / n
        blended = h + (c - h) * a[..., None]
        m1 = m[..., 0] + (lum - m[..., 0]) * a
        m2 = m[..., 1] + (lum * lum - m[..., 1]) * a
        both = present & finite
        out = np.where(both[..., None], blended, np.where(present[..., None], h, c))
        length_out = np.where(both, n, np.where(present, length, np.where(finite, F(1.0), zero)))
        o1 = np.where(both, m1, np.where(present, m[..., 0], np.where(finite, lum, zero)))
        o2 = np.where(both, m2, np.where(present, m[..., 1], np.where(finite, lum * lum, zero)))
        result = dict(color=out, length=length_out)
        if moments:
            result["moments"] = np.stack([o1, o2], -1)
            result["variance"] = np.fmax(o2 - o1 * o1, zero)
    for k, v in result.items():
        assert v.dtype == F, k
    return result


def as_history(result):
    return {k: result[k] for k in ("color", "length", "moments") if k in result}


def as_prev(view, which=("normal", "point", "id")):
    return {k: view[k] for k in which}


# ---- a synthetic view: two parallel planes, a region without any, seen from a pose ------------------------------------------------
Z_FAR, Z_NEAR = -10.0, -4.0
NEAR_X, NEAR_Y = (-0.6, 1.4), (-1.2, 1.0)      # the near plane is this rectangle; the far plane is y > FAR_BOTTOM, else nothing is hit
FAR_BOTTOM = -3.0
ID_FAR, ID_NEAR = np.uint32(3), np.uint32(7)


def hidden_by_near(origin, points):
    """whether the segment from `origin` to each world point (float64) crosses the near rectangle"""
    o = np.asarray(origin, np.float64)
    dz = points[..., 2] - o[2]
    with np.errstate(all="ignore"):
        t = (Z_NEAR - o[2]) / dz
    x, y = o[0] + t * (points[..., 0] - o[0]), o[1] + t * (points[..., 1] - o[1])
    return (t > 0) & (t < 1) & (x >= NEAR_X[0]) & (x <= NEAR_X[1]) & (y >= NEAR_Y[0]) & (y <= NEAR_Y[1])


def clean_color(points, ident):
    """a smooth function of the world point, another one on the near plane; the background where nothing is hit"""
    x, y = points[..., 0], points[..., 1]
    far = np.stack([0.55 + 0.35 * np.sin(0.7 * x + 0.3 * y), 0.5 + 0.3 * np.cos(0.4 * x - 0.6 * y), 0.45 + 0.25 * np.sin(0.5 * y), np.ones_like(x)], -1)
    near = np.stack([0.3 + 0.2 * np.cos(1.1 * x), 0.6 + 0.3 * np.sin(0.9 * y + 0.4 * x), 0.35 + 0.2 * np.cos(0.8 * x + 0.8 * y), np.ones_like(x)], -1)
    sky = np.broadcast_to(np.array([0.1, 0.12, 0.2, 1.0]), far.shape)
    return np.where((ident == ID_NEAR)[..., None], near, np.where((ident == ID_FAR)[..., None], far, sky)).astype(F)


def synthetic_view(pose, width, height, seed, specials=None):
    """The frame and the G-buffer of the two-plane scene from `pose`, analytically: a dict point, normal (H, W, 3), clean, color
    (H, W, 4) float32, id (H, W) uint32 (0 at a miss, whose point and normal are zero as rayca_hip_surface_device writes them).
    color = clean x noise of `seed`.

    `specials` (None, or the pose of the PREVIOUS camera) puts at fixed pixels (modulo the size; where they collide the later
    wins): a NaN and a +inf colour; and points on the far plane aimed at the previous view -- one behind that camera, two
    whose reprojection lands outside its image, and three landing in [-1, 0) in x, in y and in both, so that only one tap
    column, one tap row or one tap is inside."""
    ex, ey, ez = forward_basis(pose)
    o = pose["origin"].astype(np.float64)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    angle, aspect = float(pose["angle"]), width / height
    xx = (2.0 * (x + 0.5) / width - 1.0) * angle * aspect
    yy = (1.0 - 2.0 * (y + 0.5) / height) * angle
    d = xx[..., None] * ex + yy[..., None] * ey - ez
    with np.errstate(all="ignore"):
        t_near, t_far = (Z_NEAR - o[2]) / d[..., 2], (Z_FAR - o[2]) / d[..., 2]
    p_near, p_far = o + t_near[..., None] * d, o + t_far[..., None] * d
    on_near = (t_near > 0) & (p_near[..., 0] >= NEAR_X[0]) & (p_near[..., 0] <= NEAR_X[1]) & (p_near[..., 1] >= NEAR_Y[0]) & (p_near[..., 1] <= NEAR_Y[1])
    on_far = ~on_near & (t_far > 0) & (p_far[..., 1] > FAR_BOTTOM)
    ident = np.where(on_near, ID_NEAR, np.where(on_far, ID_FAR, np.uint32(0))).astype(np.uint32)
    point = np.where(on_near[..., None], p_near, np.where(on_far[..., None], p_far, 0.0)).astype(F)
    normal = np.where((on_near | on_far)[..., None], np.array([0.0, 0.0, 1.0]), 0.0).astype(F)
    if specials is not None:
        px, py, pz = forward_basis(specials)
        po = specials["origin"].astype(np.float64)
        pangle = float(specials["angle"])

        def aimed(fx, fy, behind=False):
            """the point of the far plane that the previous view sees at pixel coordinates (fx, fy)"""
            dd = ((2.0 * (fx + 0.5) / width - 1.0) * pangle * aspect) * px + ((1.0 - 2.0 * (fy + 0.5) / height) * pangle) * py - pz
            s = (Z_FAR - po[2]) / dd[2]
            return po + (-0.5 * s if behind else s) * dd

        row = min(7.3, height - 0.7)
        for (qy, qx), w in (((3, 6), aimed(2.4, 1.3, behind=True)), ((8, 1), aimed(width + 5.3, 1.2)), ((1, 9), aimed(2.6, -2.5)),
                            ((10, 4), aimed(-0.4, row)), ((12, 7), aimed(3.6 % width, -0.7)), ((13, 11), aimed(-0.3, -0.6))):
            at = (qy % height, qx % width)
            point[at], normal[at], ident[at] = w.astype(F), np.array([0.0, 0.0, 1.0], F), ID_FAR
    clean = clean_color(point.astype(np.float64), ident)
    rng = np.random.default_rng(seed)
    color = clean.copy()
    color[..., :3] = clean[..., :3] * rng.gamma(2.0, 0.5, size=(height, width, 3)).astype(F)
    if specials is not None:
        color[2 % height, 3 % width, 0] = np.nan
        color[5 % height, 17 % width, 1] = np.inf
    return dict(point=point, normal=normal, id=ident, clean=clean, color=color)


def first_history(view, specials=False):
    """the history one frame leaves (every finite pixel with length 1); `specials` sets one more pixel's length to 0"""
    hist = as_history(accumulate(view["color"]))
    if specials:
        h, w = hist["length"].shape
        hist["length"][6 % h, 5 % w] = F(0.0)
    return hist
