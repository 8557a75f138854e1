"""The goniometer: small frames whose pixels are one BRDF evaluation each, at the angles, roughnesses and light terms where
shading arithmetic goes wrong.  Everything is a deterministic function of this file; nothing is read from a file.

The scene of a case is a fan: one triangle per material, all with the apex at the origin, in the plane z = 0 (normal +z),
side by side in azimuth around +y.  Seen from a camera above the apex that looks along +y the wedges are columns whatever the
distance, so a telephoto frame aimed at the plane's horizon -- rows sweeping n.wo from 2e-2 down to 1e-4 -- crosses every
material in every row; seen from above at y = AIM_Y they are strips.  There is no other geometry: nothing occludes a light
above the plane, and the plane occludes every light below it.

A case = (fan, camera, lights, config, frame size).  `records()` turns a backend's camera rays, closest hits and surface
records (the oracle's here, the device's in the GPU test) into the float32 inputs shading_literal.pixel() computes from;
light positions, colours and falloffs come from the case, which is also what the scene was built from.

Families
  A  GGX and PBR x point light: roughness 1, 0.5, 0.1, 0.02, 1e-3, 0; PBR with metallic 0 and 1, GgxMaterial with specular 0.04
     and 0.9; cameras down, at 45 degrees and the telephoto; lights at the camera's mirror image (h -> n: the peak of D), at
     the camera (retro), at 90 degrees azimuth, low over the plane
  B  Phong x point light: shininess 0, 1, 2.5 (NaN where r.wi < 0), 3 (a negative lobe), 32, 1000, specular 0.04 and 0.9, and
     specular 0 (Lambert alone); the same cameras and lights
  C  light terms: attenuation (1,0,0), (0,1,0), (0,0,1), (0,0,0) at distances 1e-3, 1, 1e3; intensity 0 (the sample that need
     not be traced); a light below the plane; two lights, one with a colour alpha below 1
  D  the Whitted Raytracer at depth 1 on the PBR and Phong materials with a point and a directional light
  E  a quad light seen from behind and edge-on (d_omega negative and around zero), once with gamma 2.2 (oracle only)
  F  the kept special case: a frame with pixels whose n.wo exceeds 1 in float32 (G1's NaN)
"""
import math

import numpy as np

import shading_literal as sl
from rayca_amd import (Camera, Config, GgxMaterial, IntegratorStrategy, Light, Mesh, Model, Node, PbrMaterial, PhongMaterial,
                       Primitive, Scene, TriangleMesh, Trs, abi, flatten)
from rayca_amd.model import quat_axis_angle

F32 = np.float32
NONE = np.uint32(0xFFFFFFFF)
W, H = 64, 48
PATH = Config(max_depth=1, light_samples=1, samples_per_pixel=1, gamma=1.0)
WHITTED = Config(integrator=IntegratorStrategy.Raytracer, max_depth=1, gamma=1.0)
KIND_NAMES = {abi.MATERIAL_PBR: sl.PBR, abi.MATERIAL_PHONG: sl.PHONG, abi.MATERIAL_GGX: sl.GGX}

FAN_RADIUS = 3.0e4
NARROW, WIDE_FAN = 0.0136, 0.12        # half angles: the telephoto's 64 columns span +-0.0131; family C's near camera +-0.11 at y = 10
ROUGHNESSES = (1.0, 0.5, 0.1, 0.02, 1e-3, 0.0)
SHININESSES = (0.0, 1.0, 2.5, 3.0, 32.0, 1000.0)


def materials_a():
    out = [PbrMaterial(color=(0.5, 0.6, 0.7, 1.0), metallic_factor=m, roughness_factor=r) for m in (0.0, 1.0) for r in ROUGHNESSES]
    return out + [GgxMaterial(diffuse=(0.5, 0.4, 0.3, 1.0), specular=(s, s * 0.9, s * 0.8, 1.0), roughness=r) for s in (0.04, 0.9) for r in ROUGHNESSES]


def materials_b():
    out = [PhongMaterial(diffuse=(0.5, 0.4, 0.6, 1.0), specular=(s, s * 0.9, s * 0.8, 1.0), shininess=sh) for s in (0.04, 0.9) for sh in SHININESSES]
    return out + [PhongMaterial(diffuse=(0.5, 0.4, 0.6, 1.0), specular=(0.0, 0.0, 0.0, 1.0), shininess=1.0)]


def materials_c():
    return [PhongMaterial(diffuse=(0.5, 0.4, 0.6, 1.0), specular=(0.0, 0.0, 0.0, 1.0), shininess=1.0),
            PhongMaterial(diffuse=(0.3, 0.5, 0.4, 1.0), specular=(0.3, 0.2, 0.1, 1.0), shininess=8.0),
            GgxMaterial(diffuse=(0.5, 0.4, 0.3, 1.0), specular=(0.2, 0.3, 0.4, 1.0), roughness=0.4),
            PbrMaterial(color=(0.5, 0.6, 0.7, 1.0), metallic_factor=0.5, roughness_factor=0.7)]


def materials_d():
    """the Raytracer asks a GgxMaterial for PBR's metallic and roughness and panics (material/mod.rs:54-62): PBR and Phong only"""
    return materials_a()[:12] + materials_b()


# ---- cameras: position, pitch about x (0 looks along -z, pi/2 along +y), yfov; `aim`: where the frame's centre meets the plane ----
def _camera(position, pitch, yfov):
    look = np.array([0.0, math.sin(pitch), -math.cos(pitch)])
    position = np.array(position, np.float64)
    aim = position + look * (position[2] / math.cos(pitch))
    return dict(position=tuple(float(F32(v)) for v in position), pitch=pitch, yfov=yfov, aim=aim)


TELE_YFOV = 0.02
# top row 1e-4 above the horizon: the rows' angles are atan((1 - (2 y + 1) / H) tan(yfov / 2))
TELE_PITCH = math.pi / 2 - (math.atan(math.tan(TELE_YFOV / 2) * (1 - 1 / H)) + 1e-4)
AIM_Y = 1000.0


def cameras(aim_y=AIM_Y, height=24.0):
    return {"down": _camera((0.0, aim_y, height), 0.0, math.pi / 4),
            "deg45": _camera((0.0, aim_y - 17.0 * height / 24.0, 17.0 * height / 24.0), math.pi / 4, math.pi / 4),
            "tele": _camera((0.0, 0.0, 1.0), TELE_PITCH, TELE_YFOV)}


# ---- lights ----------------------------------------------------------------------------------------------------------------------
def point_light(position, intensity, attenuation=(0.0, 0.0, 1.0), color=(1.0, 0.9, 0.8, 1.0)):
    f = lambda v: tuple(float(F32(x)) for x in v)
    return dict(kind=sl.POINT, position=f(position), intensity=float(F32(intensity)), attenuation=f(attenuation), color=f(color))


def rotate32(v, q):
    """Vec3::rotate in float32, as rayca_math.hpp spells it"""
    v, q = np.asarray(v, F32), np.asarray(q, F32)
    u, s = q[:3], q[3]
    cross = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], F32)
    return ((F32(2) * sl.dot32(u, v)) * u + (s * s - sl.dot32(u, u)) * v) + (F32(2) * s) * cross


def directional_light(angle, intensity, color=(1.0, 0.9, 0.8, 1.0)):
    """a light whose node is turned by `angle` about y: it travels along rotate(+x), and get_direction() is the negative of that
    (directional.rs:47-51): elevation `angle` above the plane, from -x"""
    q = quat_axis_angle((0.0, 1.0, 0.0), angle)
    f = lambda v: tuple(float(F32(x)) for x in v)
    return dict(kind=sl.DIRECTIONAL, rotation=q, direction=tuple(float(x) for x in -rotate32((1.0, 0.0, 0.0), q)), intensity=float(F32(intensity)),
                attenuation=(0.0, 0.0, 1.0), color=f(color))


def unit_intensity(position, aim, attenuation=(0.0, 0.0, 1.0)):
    """the intensity at which a diffuse 0.5 surface at `aim` comes out near 1"""
    d = np.asarray(position, np.float64) - aim
    r = float(np.linalg.norm(d))
    fall = attenuation[0] + attenuation[1] * r + attenuation[2] * r * r
    if fall == 0.0:
        return 1.0
    return 2.0 * math.pi * fall * r * r / max(d[2] / r, 1e-3)


MIRROR_PIXEL = (25, 29)     # column (in the wedge of roughness 0.02, metallic 1 of family A), row


def pixel_point(cam, x, y, width=W, height=H):
    """where the camera ray of pixel (x, y) meets the plane z = 0, in float64 (scene.rs:125-141)"""
    angle = math.tan(cam["yfov"] / 2)
    d = np.array([(2.0 * (x + 0.5) / width - 1.0) * angle * width / height, (1.0 - 2.0 * (y + 0.5) / height) * angle, -1.0])
    s, c = math.sin(cam["pitch"]), math.cos(cam["pitch"])
    d = np.array([d[0], d[1] * c - d[2] * s, d[1] * s + d[2] * c])
    o = np.array(cam["position"], np.float64)
    return o + d * (o[2] / -d[2])


def light_positions(cam, name):
    """mirror: the camera mirrored at the vertical through the point pixel MIRROR_PIXEL sees -- there h = n to the last bit of the
    inputs, and the neighbours are the flank of D's peak (mirrored at the aim point, between four pixels, a grazing frame never
    comes near it: |wi + wo| is 0.02 there and half a pixel of azimuth tilts h by 0.02); retro: the camera's own position;
    side: at 90 degrees azimuth; low: a thousandth of the distance above the plane"""
    c, aim = np.array(cam["position"], np.float64), cam["aim"]
    rel = c - aim
    d = float(np.linalg.norm(rel))
    hor = rel[:2] if np.linalg.norm(rel[:2]) > 1e-6 * d else np.array([0.0, -d])
    p = pixel_point(cam, *MIRROR_PIXEL)
    return {"mirror": np.array([2.0 * p[0] - c[0], 2.0 * p[1] - c[1], c[2]]),
            "retro": c, "side": aim + np.array([-hor[1], hor[0], rel[2]]), "low": aim + np.array([0.1 * d, 0.05 * d, 1e-3 * d])}[name]


# ---- the scene --------------------------------------------------------------------------------------------------------------------
def fan_scene(materials, half_angle, camera, lights, normal=(0.0, 0.0, 1.0), quads=()):
    model = Model("fan")
    prims = []
    edges = np.linspace(-half_angle, half_angle, len(materials) + 1)
    for i, m in enumerate(materials):
        a, b = edges[i], edges[i + 1]
        # counter-clockwise seen from +z: apex, the edge at the larger azimuth, the edge at the smaller one
        pos = np.array([[0.0, 0.0, 0.0], [FAN_RADIUS * math.sin(b), FAN_RADIUS * math.cos(b), 0.0], [FAN_RADIUS * math.sin(a), FAN_RADIUS * math.cos(a), 0.0]], F32)
        mesh = TriangleMesh(pos, np.array([0, 1, 2], np.uint8), normals=np.tile(np.array([normal], F32), (3, 1)))
        prims.append(model.primitives.push(Primitive(geometry=model.geometries.push(mesh), material=model.materials.push(m))))
    model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=prims)))))
    cam = model.cameras.push(Camera(yfov_radians=camera["yfov"]))
    model.root.children.append(model.nodes.push(Node(camera=cam, trs=Trs(translation=camera["position"],
                                                                         rotation=quat_axis_angle((1.0, 0.0, 0.0), camera["pitch"])))))
    for lt in lights:
        if lt["kind"] == sl.POINT:
            h = model.lights.push(Light(kind=abi.LIGHT_POINT, color=lt["color"], intensity=lt["intensity"], attenuation=lt["attenuation"]))
            model.root.children.append(model.nodes.push(Node(light=h, trs=Trs(translation=lt["position"]))))
        else:
            h = model.lights.push(Light(kind=abi.LIGHT_DIRECTIONAL, color=lt["color"], intensity=lt["intensity"]))
            model.root.children.append(model.nodes.push(Node(light=h, trs=Trs(rotation=lt["rotation"]))))
    for quad in quads:
        emit = model.materials.push(PhongMaterial(emission=(1.0, 1.0, 1.0, 1.0)))
        h = model.lights.push(Light.quad(ab=quad["ab"], ac=quad["ac"], color=(1.0, 0.9, 0.8, 1.0), material=emit, intensity=quad["intensity"]))
        model.root.children.append(model.nodes.push(Node(light=h, trs=Trs(translation=quad["position"]))))
    scene = Scene()
    scene.push_model(model)
    return scene


class Case:
    def __init__(self, family, name, materials, half_angle, camera, lights, config=PATH, width=W, height=H, normal=(0.0, 0.0, 1.0), quads=()):
        self.family, self.name, self.camera, self.lights, self.config, self.width, self.height = family, name, camera, lights, config, width, height
        self.whitted = config.integrator == IntegratorStrategy.Raytracer
        self._build = lambda: flatten(fan_scene(materials, half_angle, camera, lights, normal, quads))
        self._desc = None

    @property
    def desc(self):
        if self._desc is None:
            self._desc = self._build()
        return self._desc

    def __repr__(self):
        return f"{self.family}:{self.name}"


def _lit(cam, light, **kw):
    """(under the low light the term falls like r^-5 away from the aim point: thirty times the unit there keeps more of the frame
    inside the displayable decades)"""
    p = light_positions(cam, light)
    return [point_light(p, (30.0 if light == "low" else 1.0) * unit_intensity(p, cam["aim"]), **kw)]


def family_a():
    return [Case("A", f"{c}-{l}", materials_a(), NARROW, cam, _lit(cam, l)) for c, cam in cameras().items() for l in ("mirror", "retro", "side", "low")]


def family_b():
    return [Case("B", f"{c}-{l}", materials_b(), NARROW, cam, _lit(cam, l)) for c, cam in cameras().items() for l in ("mirror", "retro", "side", "low")]


C_W, C_H = 32, 24


def family_c():
    cam = cameras(10.0, 2.0)["down"]
    aim = cam["aim"]
    mk = lambda name, lights: Case("C", name, materials_c(), WIDE_FAN, cam, lights, width=C_W, height=C_H)
    out = []
    for att in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)):
        for dist in (1e-3, 1.0, 1e3):
            # beside a pixel centre; at distance 1e3 far enough beside that n.wi stays more than a delta below 1; the unit is set
            # 0.3 beside the light's foot, so that the light 1e-3 over the plane lights more than the pixel below it
            p = aim + np.array([0.013 + 0.003 * dist, 0.021, dist])
            out.append(mk("att%d%d%d-dist%g" % (*att, dist), [point_light(p, unit_intensity(p, aim + np.array([0.3, 0.0, 0.0]), att), att)]))
    p = aim + np.array([0.013, 0.021, 1.0])
    out.append(mk("intensity0", [point_light(p, 0.0)]))
    below = aim + np.array([0.2, 0.1, -1.0])
    out.append(mk("below", [point_light(below, 10.0)]))
    q = aim + np.array([-0.4, 0.3, 0.5])
    out.append(mk("two-lights", [point_light(p, 0.6 * unit_intensity(p, aim), color=(1.0, 0.8, 0.6, 0.5)), point_light(q, 0.5 * unit_intensity(q, aim), (0.5, 0.25, 0.25))]))
    return out


def family_d():
    out = []
    for c, cam in cameras().items():
        p = light_positions(cam, "mirror")
        # Whitted: intensity / falloff alone, no second 1 / r^2, no 1 / pi on the specular part
        i = unit_intensity(p, cam["aim"]) / float(np.linalg.norm(p - cam["aim"])) ** 2 / 2.0
        out.append(Case("D", f"{c}-point", materials_d(), NARROW, cam, [point_light(p, i)], config=WHITTED))
        out.append(Case("D", f"{c}-dir60", materials_d(), NARROW, cam, [directional_light(math.radians(60.0), 2.0)], config=WHITTED))
        out.append(Case("D", f"{c}-dir0.5", materials_d(), NARROW, cam, [directional_light(math.radians(0.5), 100.0)], config=WHITTED))
    return out


def materials_e():
    return materials_b()[6:12] + [materials_b()[12]] + materials_c()[2:]


def family_e():
    """Quad lights over the plane.  A quad's own triangles are one-sided, so a quad alone that shows the plane its back lights
    nothing; its samples are lit -- with a negative d_omega -- when their shadow rays, having passed it, end on another
    emissive surface: `behind` hangs a quad with its normal ab x ac towards the plane under a larger one that faces away.
    `front` is that larger one alone (d_omega positive), `edge-on` a vertical quad whose d_omega changes sign inside the
    frame.  `behind` and `edge-on` once more with gamma 2.2: a negative mean through powf."""
    cam = cameras(10.0, 6.0)["deg45"]
    aim = cam["aim"]
    mk = lambda name, quads, **kw: Case("E", name, materials_e(), WIDE_FAN, cam, [], config=Config(max_depth=1, light_samples=1, seed=5, **kw), quads=quads)
    at = lambda *v: tuple(float(x) for x in aim + np.array(v))
    front = dict(ab=(6.0, 0.0, 0.0), ac=(0.0, 6.0, 0.0), position=at(-3.0, -3.0, 4.0), intensity=40.0)
    back = dict(ab=(0.0, 2.0, 0.0), ac=(2.0, 0.0, 0.0), position=at(-1.0, -1.0, 3.0), intensity=40.0)
    edge = dict(ab=(0.0, 2.0, 0.0), ac=(0.0, 0.0, 2.0), position=at(0.1, -1.0, 0.5), intensity=40.0)
    return [mk("front", [front]), mk("behind", [back, front]), mk("edge-on", [edge]), mk("behind-gamma2.2", [back, front], gamma=2.2),
            mk("edge-on-gamma2.2", [edge], gamma=2.2)]


# Family F.  n.wo = dot(normalize(vertex normal), -normalize(camera direction)) exceeds 1 in float32 only where the two unit
# vectors are parallel to the last bit and both a rounding longer than 1.  Found by search on the CPU with the oracle's camera rays
# (the down camera of family C at 32 x 24; vertex normals set to minus the direction of pixel after pixel, until the oracle's own
# frame shows G1's NaN at that pixel): the direction of pixel F_PIXEL, as float32 words.
F_PIXEL = 14
F_NORMAL = (1027924778, 3200036615, 1064151551)


def family_f():
    cam = cameras(10.0, 2.0)["down"]
    p = light_positions(cam, "side")
    return [Case("F", "n.wo-above-1", materials_a()[12:], WIDE_FAN, cam, [point_light(p, unit_intensity(p, cam["aim"]))], width=C_W, height=C_H,
                 normal=tuple(float(v) for v in np.array(F_NORMAL, np.uint32).view(F32)))]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f}


# ---- records ------------------------------------------------------------------------------------------------------------------------
class OracleBackend:
    """camera rays, closest hits and surface records of the CPU oracle"""

    def __init__(self, desc):
        import oracle_lib as ol
        self.orc = ol.OracleScene(desc, Config())

    def surface_records(self, config, width, height):
        rays = self.orc.camera_rays(config, width, height)
        t, prim, uv, _ = self.orc.trace_rays(rays)
        return rays, prim, self.orc.surface(rays, t, prim, uv)

    def render(self, config, width, height):
        return self.orc.render(config, width, height)

    def close(self):
        self.orc.close()


def records(case, backend):
    """the float32 inputs of the literal, one row per pixel of the case's frame"""
    rays, prim, s = backend.surface_records(case.config, case.width, case.height)
    flags = np.asarray(s["flags"]).view(np.uint32)
    hit = (flags & np.uint32(abi.SURFACE_HIT)) != 0
    assert np.array_equal(hit, np.asarray(prim).view(np.uint32) != NONE)
    mat = np.asarray(s["material"]).view(np.uint32)
    mats = case.desc._materials
    kind = np.array([KIND_NAMES[mats[m].kind] if h else sl.PBR for m, h in zip(mat, hit)])
    metallic = np.array([mats[m].metallic_factor if h and mats[m].kind == abi.MATERIAL_PBR else 0.0 for m, h in zip(mat, hit)], F32)
    return dict(point=s["point"], normal=s["normal"], view=-rays[:, 3:6], diffuse=s["diffuse"], specular=s["specular"], color=s["color"],
                roughness=s["rough"][:, 0], shininess=s["rough"][:, 1], kind=kind, metallic=metallic, hit=hit, material=mat)


def visible(case, rec):
    """per light: is the shadow ray free?  A point light above the hit point's plane and every directional light (they all shine
    from above) is; a point light below is behind the plane."""
    return [rec["point"][:, 2] < F32(lt["position"][2]) if lt["kind"] == sl.POINT else np.ones(rec["hit"].shape, bool) for lt in case.lights]


def expected(case, rec):
    return sl.pixel(rec, case.lights, visible(case, rec), whitted=case.whitted)
