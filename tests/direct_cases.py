"""The inputs the direct-light tests share (helper module; test_direct_cpu.py checks the literal on them, test_gpu_direct.py runs
them): small authored scenes -- a room of Phong surfaces with ks = 0 and shininess 0, a two-sided card that throws a shadow, lamp
panels -- written as SDTF text from the light dicts below, so that a test has the lights' parameters without reading them back
from the code under test; and hashed points on the scenes' triangles and inside the room.  tests/golden/cornell_quad.sdtf is
used as it stands (its ball included)."""
import os
import tempfile

import numpy as np

import ambient_cases as ac
import oracle_lib as ol
import ray_edges as R
from rayca_amd import Config, Scene, flatten, sdtf

F = np.float32
POINT, QUAD = 1, 2
SCENES = ["points", "quad", "qpq", "dim"]
COUNTS = [1, 63, 64, 65, 4097]
INACTIVE = {0: "zero", 7: "zero", 40: "minus_zero", 62: "nan_normal", 64: "inf_position", 233: "nan_normal", 4096: "zero"}
ON_LIGHT = 5            # this point of every batch lies on the scene's first point light, where it has one: dropped samples
BIAS = F(1e-4)


def point_light(position, color, attenuation=(1.0, 0.0, 0.0), intensity=1.0, alpha=1.0):
    return dict(kind=POINT, position=F(position), color=F([*color, alpha]), intensity=F(intensity), attenuation=F(attenuation),
                ab=F([0, 0, 0]), ac=F([0, 0, 0]), normal=F([0, 0, 0]), area=F(0))


def quad_light(a, ab, ac, color):
    """axis-aligned edges: the normal is a unit axis and the area |ab| |ac|, both exact in f32 as the host computes them"""
    ab, ac = F(ab), F(ac)
    n = np.cross(ab.astype(np.float64), ac.astype(np.float64))
    la, lc = F(np.abs(ab).max()), F(np.abs(ac).max())
    return dict(kind=QUAD, position=F(a), color=F([*color, 1.0]), intensity=F(1.0), attenuation=F([0, 0, 1]), ab=ab, ac=ac,
                normal=F(n / np.linalg.norm(n)), area=F((F(1.0) * la) * lc))


LAMP_UP = quad_light((-0.3, 1.98, -0.3), (0, 0, 0.6), (0.6, 0, 0), (6, 6, 6))           # ab x ac = +y: counts for points below it
LAMP_BACK = quad_light((-0.2, 1.2, -0.98), (0.4, 0, 0), (0, -0.4, 0), (3, 2, 1))       # ab x ac = -z: counts for points in front of it
LIGHTS = {
    "points": [point_light((0.4, 1.6, 0.3), (4, 3.5, 3), (1.0, 0.1, 0.05)), point_light((-0.5, 0.7, 0.5), (1, 2, 3), (0.0, 0.0, 1.0))],
    "qpq": [LAMP_UP, point_light((0.4, 1.6, 0.3), (2, 2, 2), (1.0, 0.0, 0.25)), LAMP_BACK],
    "dim": [point_light((0.4, 1.6, 0.3), (4, 3.5, 3), intensity=0.0), point_light((-0.5, 0.7, 0.5), (1, 2, 3), (0.5, 0.0, 0.5), alpha=0.5)],
}

_HEAD = """size 48 36
integrator pathtracer
maxdepth 1
lightsamples 1
spp 1
nexteventestimation on
gamma 1
camera 0 1 3.2 0 1 0 0 1 0 45
maxverts 32
vertex -1 0 -1
vertex 1 0 -1
vertex 1 0 1
vertex -1 0 1
vertex -1 2 -1
vertex 1 2 -1
vertex 1 2 1
vertex -1 2 1
vertex -0.3 1.98 -0.3
vertex 0.3 1.98 -0.3
vertex 0.3 1.98 0.3
vertex -0.3 1.98 0.3
vertex -0.2 0.8 -0.98
vertex 0.2 0.8 -0.98
vertex 0.2 1.2 -0.98
vertex -0.2 1.2 -0.98
vertex -0.5 1.0 -0.3
vertex 0.1 1.0 -0.3
vertex 0.1 1.0 0.3
vertex -0.5 1.0 0.3
"""
_ROOM = """specular 0 0 0
shininess 0
diffuse 0.7 0.7 0.7
tri 0 3 2
tri 0 2 1
tri 4 5 6
tri 4 6 7
tri 0 1 5
tri 0 5 4
diffuse 0.7 0.15 0.1
tri 0 4 7
tri 0 7 3
diffuse 0.15 0.6 0.15
tri 1 2 6
tri 1 6 5
diffuse 0.6 0.5 0.1
tri 16 17 18
tri 16 18 19
tri 16 18 17
tri 16 19 18
"""
_LAMPS = """diffuse 0 0 0
emission 6 6 6
tri 8 9 10
tri 8 10 11
emission 3 2 1
tri 12 13 14
tri 12 14 15
emission 0 0 0
"""


def _num(v):
    return " ".join(repr(float(x)) for x in v)


def sdtf_text(name):
    lines = [_HEAD]
    for L in LIGHTS[name]:
        if L["kind"] == POINT:
            lines.append(f"attenuation {_num(L['attenuation'])}\npoint {_num(L['position'])} {_num(L['color'][:3])}\n")
        else:
            lines.append(f"quadLight {_num(L['position'])} {_num(L['ab'])} {_num(L['ac'])} {_num(L['color'][:3])}\n")
    lines.append(_ROOM)
    if any(L["kind"] == QUAD for L in LIGHTS[name]):
        lines.append(_LAMPS)
    return "".join(lines)


def build_scene(name, lights=None) -> Scene:
    """`lights`: other dicts for the same light nodes (kinds as in LIGHTS[name]): what a scene update moves them to"""
    scene = Scene(name)
    if name == "quad":
        sdtf.push_sdtf_from_path(scene, os.path.join(R.G, "cornell_quad.sdtf"))
        return scene
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, name + ".sdtf")
        open(path, "w").write(sdtf_text(name))
        model, _ = sdtf.load_sdtf_path(path)
    for L, ml in zip(lights if lights is not None else LIGHTS[name], model.lights):   # what SDTF cannot say: intensity and alpha
        ml.intensity = float(L["intensity"])
        ml.color = tuple(float(x) for x in L["color"])
        if L["kind"] == POINT:
            ml.attenuation = tuple(float(x) for x in L["attenuation"])
    if lights is not None:
        k = 0
        for node in model.nodes:
            if node.light is not None:
                node.trs.translation = tuple(float(x) for x in lights[k]["position"][:3])
                k += 1
    scene.push_model(model)
    return scene


def lights_of(name):
    if name == "quad":
        return [LAMP_UP]          # cornell_quad.sdtf's quadLight line, restated
    return LIGHTS[name]


def scene_desc(name):
    return R._cached(("direct desc", name), lambda: flatten(build_scene(name)))


def oracle_scene(name):
    return R._cached(("direct oracle", name), lambda: ol.OracleScene(scene_desc(name), Config()))


def world_triangles(name):
    def make():
        orc = oracle_scene(name)
        t = orc.world_triangles(orc.primitive_count).astype(np.float64).reshape(-1, 3, 3)
        return t[np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) > 0]
    return R._cached(("direct tris", name), make)


def surface_points(name, count=COUNTS[-1]):
    """(points, normals) [count, 3] f32 on the scene's triangles, every other normal flipped (those face away from everything the
    face sees: void samples), the INACTIVE ones made inactive, ON_LIGHT moved onto the first point light"""
    def make():
        p, n = ac.points_on(world_triangles(name), count, {k: v for k, v in INACTIVE.items() if k < count})
        first = [L for L in lights_of(name) if L["kind"] == POINT]
        if first:
            p[ON_LIGHT] = first[0]["position"][:3]
        return p, n
    return R._cached(("direct surface points", name, count), make)


def volume_points(name, count=COUNTS[-1]):
    """points [count, 3] f32 hashed inside the room, the INACTIVE ones whose rule needs no normal made non-finite, ON_LIGHT on the
    first point light"""
    def make():
        p = (R._unit(911, count, 3) * [1.9, 1.9, 1.9] + [-0.95, 0.03, -0.95]).astype(F)
        for i, what in INACTIVE.items():
            if i < count and what in ("nan_normal", "inf_position"):
                p[i, i % 3] = np.nan if what == "nan_normal" else np.inf
        first = [L for L in lights_of(name) if L["kind"] == POINT]
        if first:
            p[ON_LIGHT] = first[0]["position"][:3]
        return p
    return R._cached(("direct volume points", name, count), make)
