"""Cases of test_gpu_five_waves.py (helper module, and the program its child processes run).

The path k_generation is compiled for five waves per SIMD and parks a vertex's context in 104 B per lane instead of 112
(trace_core.inc RAYCA_MIN_WAVES, RAYCA_CTX_COMPACT): the running direct sum without its alpha, the pending sample as its three
products x.rgb * x.a, roughness and shininess in one word chosen by the material's kind; behind four stack rows instead of twelve.
None of that may change a bit of a frame or a counter.  The frames are those sizes of wave_block_cases.py -- one tile, fewer tiles
than waves, ragged right and bottom tiles -- of scenes that put something into every shortened word:

mixed_room   walls of a Phong material whose vertex colours have alpha 0.8, a block of a PBR material whose colour has alpha 0.6
             (so kd.a and the sample's alpha differ from 1; roughness for one, shininess for the other in the shared word), an
             emissive panel the camera sees, under a quad light (closest-hit shadow rays, t_stop == FLT_MAX) and a point light
             that the block shadows on the floor (samples lit and not lit, summed over two lights and two light samples)
spheres      the sphere fixture: a sphere's view vector is the model-space direction, which stays parked (the sphere instantiations,
             like the counting ones, stay at four waves and twelve rows: their layout changes, their bound does not)
deep_soup    the deep scene of node_step_cases.py, whose camera rays hold more entries than four LDS rows

python tests/five_waves_cases.py OUT.npz [case ...]: the fused engine's frames and counters of the cases, with the library
RAYCA_HIP_LIB names and the knobs of the environment (both are read once per process)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import node_step_cases as N   # noqa: E402
import wave_block_cases as W   # noqa: E402
from rayca_amd import Config, flatten   # noqa: E402

COUNTER_KEYS, RAY_COUNTERS, SIZES = W.COUNTER_KEYS, W.RAY_COUNTERS, W.SIZES
VERTEX_ALPHA, MATERIAL_ALPHA = 0.8, 0.6


def mixed_room():
    from rayca_amd import PbrMaterial, PhongMaterial, Trs, scenes
    from rayca_amd.model import Light, Mesh, Model, Node, Primitive, Scene
    model = Model()
    wall = model.materials.push(PhongMaterial(diffuse=(0.7, 0.7, 0.7, 1.0), specular=(0.1, 0.1, 0.1, 1.0), shininess=8.0))
    block = model.materials.push(PbrMaterial(color=(0.2, 0.5, 0.7, MATERIAL_ALPHA), metallic_factor=0.5, roughness_factor=0.35))
    emit = model.materials.push(PhongMaterial(emission=(1.0, 1.0, 1.0, 1.0)))
    X, Y, Z = np.array([2, 0, 0], np.float32), np.array([0, 2, 0], np.float32), np.array([0, 0, 2], np.float32)
    room, blk, lamp = scenes._MeshBuilder(), scenes._MeshBuilder(), scenes._MeshBuilder()
    tint = (1.0, 0.9, 0.8, VERTEX_ALPHA)
    room.grid((-1, 0, -1), Z, X, 1, 1, col=tint)
    room.grid((-1, 0, -1), X, Y, 1, 1, col=tint)
    room.grid((-1, 0, -1), Y, Z, 1, 1, col=tint)
    room.grid((1, 0, -1), Z, Y, 1, 1, col=tint)
    blk.box((-0.4, 0, -0.4), (0.2, 0.7, 0.2))
    # the emissive panel the quad light stands for, facing down; low enough that the camera's upper rows see it
    lamp.grid((-0.3, 1.6, -0.3), np.array([0.6, 0, 0], np.float32), np.array([0, 0, 0.6], np.float32), 1, 1)
    for mb, mat in ((room, wall), (blk, block), (lamp, emit)):
        g = model.geometries.push(mb.mesh())
        p = model.primitives.push(Primitive(geometry=g, material=mat))
        model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=[p])))))
    quad = model.lights.push(Light.quad(ab=(0.6, 0.0, 0.0), ac=(0.0, 0.0, 0.6), color=(1, 1, 1, 1), material=emit, intensity=6.0))
    model.root.children.append(model.nodes.push(Node(light=quad, trs=Trs(translation=(-0.3, 1.6, -0.3)))))
    point = Light.point()
    point.set_intensity(3.0)
    model.root.children.append(model.nodes.push(Node(light=model.lights.push(point), trs=Trs(translation=(0.8, 0.9, 0.8)))))
    cam = model.cameras.push(scenes.Camera())
    model.root.children.append(model.nodes.push(Node(camera=cam, trs=Trs(translation=(0.0, 1.0, 3.2)))))
    scene = Scene()
    scene.push_model(model)
    return scene


SCENES = dict(N.SPILL_SCENES, mixed_room=mixed_room)
_DESC = {}


def frame_desc(name):
    if name not in _DESC:
        _DESC[name] = flatten(SCENES[name]())
    return _DESC[name]


# name -> (scene, width, height, Config)
CASES = {}
for _w, _h in SIZES:
    for _d in (1, 3):
        CASES[f"mixed_{_w}x{_h}_d{_d}"] = ("mixed_room", _w, _h, Config(max_depth=_d, seed=50 + _d))
CASES["mixed_two_light_samples"] = ("mixed_room", 24, 16, Config(max_depth=1, light_samples=2, seed=9))
CASES["spheres_d1"] = ("spheres", 67, 45, Config(max_depth=1, seed=6))
CASES["spheres_d3"] = ("spheres", 67, 45, Config(max_depth=3, seed=5))
CASES["deep_d1"] = ("deep_soup", 64, 45, Config(max_depth=1, seed=18))
CASES["deep_d3"] = ("deep_soup", 64, 45, Config(max_depth=3, seed=20))
DEEP = ("deep_d1", "deep_d3")
IN_FLIGHT = ("mixed_67x45_d3", "mixed_67x45_d1", "mixed_24x16_d3")


def render_cases(names=None, engine=None):
    """{"<case>/u8|f32|counters": array}: production frames and the six counters of the counting instantiation"""
    from rayca_amd import DeviceScene, abi
    engine = abi.ENGINE_FUSED if engine is None else engine
    out, scenes = {}, {}
    for name in names or list(CASES):
        scene, w, h, cfg = CASES[name]
        if scene not in scenes:
            scenes[scene] = DeviceScene(frame_desc(scene), Config(), builder=abi.BUILDER_SAH)
            scenes[scene].finish()
        ds = scenes[scene]
        kw = dict(engine=engine, camera_rays=abi.CAMERA_GENERATION if engine == abi.ENGINE_FUSED else abi.CAMERA_AUTO)
        u8, f32, _ = ds.render(cfg, w, h, **kw)
        st = ds.render(cfg, w, h, collect_stats=True, **kw)[2]
        out[name + "/u8"], out[name + "/f32"] = u8, f32
        out[name + "/counters"] = np.array([int(st[k]) for k in COUNTER_KEYS], np.uint64)
    for ds in scenes.values():
        ds.close()
    return out


if __name__ == "__main__":
    from rayca_amd import lib
    np.savez(sys.argv[1], **render_cases(sys.argv[2:] or None))
    print("wrote", sys.argv[1], "library =", os.path.realpath(lib.LIB_PATH), "RAYCA_PATH_LDS_ENTRIES =", os.environ.get("RAYCA_PATH_LDS_ENTRIES"))
