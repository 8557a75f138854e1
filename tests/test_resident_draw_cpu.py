"""The resident draw() without a GPU: the renderer handle's entry points are exported and bound, a renderer can be made,
asked and destroyed with no device present, and the decision rule -- reuse, update or rebuild -- is checked through
rayca_hip_scene_desc_compare, which runs the code rayca_hip_renderer_draw decides with on two descriptors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rayca_amd import (Config, Image, Mesh, Model, Node, PbrMaterial, Primitive, Renderer, Scene, SoftRenderer, Texture,
                       TriangleMesh, Trs, abi, flatten, scenes, sdtf)
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
P = C.POINTER

NEW_SYMBOLS = {
    "rayca_hip_renderer_create": [P(abi.RaycaBuildOptions), P(C.c_void_p)],
    "rayca_hip_renderer_draw": [C.c_void_p, P(abi.RaycaSceneDesc), P(abi.RaycaConfig), C.c_uint32, C.c_uint32, P(abi.RaycaRenderOptions),
                                C.c_void_p, C.c_void_p, P(abi.RaycaStats), P(C.c_uint32)],
    "rayca_hip_renderer_last_draw": [C.c_void_p, P(C.c_uint32), P(C.c_float), P(C.c_uint64)],
    "rayca_hip_renderer_scene": [C.c_void_p, P(C.c_void_p)],
    "rayca_hip_renderer_invalidate": [C.c_void_p],
    "rayca_hip_renderer_destroy": [C.c_void_p],
    "rayca_hip_scene_desc_compare": [P(abi.RaycaSceneDesc), C.c_uint32, P(abi.RaycaSceneDesc), C.c_uint32, P(C.c_uint32)],
}


def test_renderer_symbols_are_exported_and_bound(product_lib):
    for name, argtypes in NEW_SYMBOLS.items():
        assert name in abi.PRODUCT_SYMBOLS
        fn = getattr(product_lib, name)
        assert fn.restype is C.c_int32, name
        assert fn.argtypes == argtypes, name


def test_draw_constants_equal_the_headers():
    header = open(os.path.join(ROOT, "include", "rayca_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    enums = {k: int(v) for k, v in re.findall(r"\b(RAYCA_DRAW_[A-Z0-9_]+)\s*=\s*(\d+)", header)}
    assert len(enums) == 13
    for name, value in enums.items():
        assert getattr(abi, name[len("RAYCA_"):]) == value, name
    assert "RAYCA_ABI_VERSION 2u" in header      # no layout changed


def test_a_renderer_lives_without_a_gpu(product_lib):
    """create / last_draw / scene / invalidate / destroy touch no device.  Before the first draw: action RAYCA_NONE (not one
    of the three actions), every time and counter zero, no resident scene."""
    h = C.c_void_p()
    assert product_lib.rayca_hip_renderer_create(None, C.byref(h)) == abi.OK and h.value
    action, ms, n = C.c_uint32(7), (C.c_float * abi.DRAW_MS_COUNT)(*[1.0] * 4), (C.c_uint64 * abi.DRAW_N_COUNT)(*[9] * 4)
    assert product_lib.rayca_hip_renderer_last_draw(h, C.byref(action), ms, n) == abi.OK
    assert action.value == abi.NONE and action.value not in (abi.DRAW_REUSED, abi.DRAW_UPDATED, abi.DRAW_REBUILT)
    assert list(ms) == [0.0] * 4 and list(n) == [0] * 4
    assert product_lib.rayca_hip_renderer_last_draw(h, None, None, None) == abi.OK
    scene = C.c_void_p(1)
    assert product_lib.rayca_hip_renderer_scene(h, C.byref(scene)) == abi.OK and not scene.value
    assert product_lib.rayca_hip_renderer_invalidate(h) == abi.OK
    assert product_lib.rayca_hip_renderer_destroy(h) == abi.OK
    assert product_lib.rayca_hip_renderer_destroy(None) == abi.OK
    # explicit options; an unknown builder is refused
    o = abi.RaycaBuildOptions()
    o.builder = abi.BUILDER_REFERENCE
    assert product_lib.rayca_hip_renderer_create(C.byref(o), C.byref(h)) == abi.OK
    assert product_lib.rayca_hip_renderer_destroy(h) == abi.OK
    o.builder = 5
    assert product_lib.rayca_hip_renderer_create(C.byref(o), C.byref(h)) == abi.ERR_BAD_ARG and not h.value


def test_null_arguments_are_bad_arguments_with_a_message(product_lib):
    d = flatten(scenes.cornell_scene())
    h = C.c_void_p()
    action = C.c_uint32()
    calls = [lambda: product_lib.rayca_hip_renderer_create(None, None),
             lambda: product_lib.rayca_hip_renderer_draw(None, d.ptr(), None, 8, 8, None, None, None, None, None),
             lambda: product_lib.rayca_hip_renderer_last_draw(None, None, None, None),
             lambda: product_lib.rayca_hip_renderer_scene(None, C.byref(h)),
             lambda: product_lib.rayca_hip_renderer_invalidate(None),
             lambda: product_lib.rayca_hip_scene_desc_compare(None, 1, d.ptr(), 1, C.byref(action)),
             lambda: product_lib.rayca_hip_scene_desc_compare(d.ptr(), 1, None, 1, C.byref(action)),
             lambda: product_lib.rayca_hip_scene_desc_compare(d.ptr(), 1, d.ptr(), 1, None)]
    for call in calls:
        assert call() == abi.ERR_BAD_ARG
        assert "null" in last_error()
    assert product_lib.rayca_hip_renderer_create(None, C.byref(h)) == abi.OK
    assert product_lib.rayca_hip_renderer_draw(h, None, None, 8, 8, None, None, None, None, C.byref(action)) == abi.ERR_BAD_ARG
    assert "null" in last_error() and action.value == abi.NONE
    assert product_lib.rayca_hip_renderer_scene(h, None) == abi.ERR_BAD_ARG
    product_lib.rayca_hip_renderer_destroy(h)


def test_python_mirror(product_lib):
    r = Renderer()
    info = r.last_draw()
    assert info["action"] is None and info["builds"] == info["updates"] == info["reuses"] == info["kept_bytes"] == 0
    assert r.scene is None
    r.invalidate()
    r.close()
    r.close()
    s = SoftRenderer(Config())
    assert s.builder == abi.BUILDER_SAH and s.last_draw is None and s.last_stats is None
    s.close()
    assert SoftRenderer(builder=abi.BUILDER_REFERENCE).builder == abi.BUILDER_REFERENCE


# ---- the decision rule ---------------------------------------------------------------------------------------------------
def cornell():
    return flatten(scenes.cornell_scene())


def cornell_quad():
    scene = Scene()
    sdtf.push_sdtf_from_path(scene, os.path.join(G, "cornell_quad.sdtf"))
    return flatten(scene)


def two_level():
    """a textured quad under a group node under the model root, next to the default model's camera and point lights"""
    model = Model()
    tex = np.random.RandomState(5).randint(0, 256, (8, 8, 4)).astype(np.uint8)
    t = model.textures.push(Texture(image=model.images.push(Image(8, 8, abi.COLOR_RGBA8, tex))))
    mat = model.materials.push(PbrMaterial(color=(0.9, 0.8, 0.7, 1.0), albedo=t))
    g = model.geometries.push(TriangleMesh.quad(uv_scale=(3.0, 2.0)))
    p = model.primitives.push(Primitive(geometry=g, material=mat))
    leaf = model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=[p])), trs=Trs(scale=(3.0, 3.0, 1.0))))
    group = model.nodes.push(Node(children=[leaf], trs=Trs(translation=(0.1, 0.0, -0.5))))
    model.root.children.append(group)
    scene = Scene()
    scene.push_model(model)
    scene.push_model(SoftRenderer.create_default_model())
    return flatten(scene)


SCENES = {"cornell": cornell, "cornell_quad": cornell_quad, "two_level": two_level}


def nodes(d):
    return d._nodes[:d.c.node_count]


def node_with(d, field):
    return next(n for n in nodes(d) if getattr(n, field) != abi.NONE)


def light_of_kind(d, kind):
    return next(d._lights[i] for i in range(d.c.light_count) if d._lights[i].kind == kind)


def flip_bit(array, index=0):
    array.reshape(-1).view(np.uint32)[index] ^= 1


def e_camera_trs(d):
    node_with(d, "camera").trs.translation[0] += 0.25


def e_yfov(d):
    d._cameras[node_with(d, "camera").camera].yfov_radians *= 0.9


def e_light_colour(d):
    light_of_kind(d, abi.LIGHT_POINT).color[1] = 0.5


def e_light_intensity(d):
    light_of_kind(d, abi.LIGHT_POINT).intensity *= 2.0


def e_light_position(d):
    n = next(n for n in nodes(d) if n.light != abi.NONE and d._lights[n.light].kind == abi.LIGHT_POINT)
    n.trs.translation[1] += 0.125


def e_material_colour(d):
    d._materials[0].color[2] = 0.125


def e_quad_light_colour(d):
    light_of_kind(d, abi.LIGHT_QUAD).color[0] *= 0.5


def e_vertex_bit(d):
    flip_bit(d.positions, d.positions.size - 1)


def e_index(d):
    d.index_bytes[d.index_bytes.size // 2] ^= 1


def e_texel(d):
    assert d.image_bytes.size
    d.image_bytes[-1] ^= 0x80


def e_normals_null(d):
    assert d.c.normals
    d.c.normals = None


def e_mesh_node(d):
    node_with(d, "mesh").trs.translation[2] -= 0.5


def e_mesh_parent(d):
    ns = nodes(d)
    parent = ns[node_with(d, "mesh").parent]
    assert parent.mesh == abi.NONE
    parent.trs.translation[0] += 1.0


def e_quad_ab(d):
    light_of_kind(d, abi.LIGHT_QUAD).ab[0] += 0.25


def e_quad_transform(d):
    n = next(n for n in nodes(d) if n.light != abi.NONE and d._lights[n.light].kind == abi.LIGHT_QUAD)
    n.trs.translation[1] -= 0.125


def e_point_to_quad(d):
    l = light_of_kind(d, abi.LIGHT_POINT)
    l.kind, l.ab[:], l.ac[:] = abi.LIGHT_QUAD, (0.5, 0.0, 0.0), (0.0, 0.0, 0.5)


def e_quad_to_point(d):
    light_of_kind(d, abi.LIGHT_QUAD).kind = abi.LIGHT_POINT


def e_one_more_node(d):
    extra = abi.RaycaNode()
    extra.parent, extra.model, extra.mesh, extra.camera, extra.light = 0, abi.NONE, abi.NONE, abi.NONE, abi.NONE
    extra.trs.rotation[3] = 1.0
    extra.trs.scale[:] = (1.0, 1.0, 1.0)
    d._nodes = abi._array(abi.RaycaNode, list(nodes(d)) + [extra])
    d.c.nodes, d.c.node_count = d._nodes, d.c.node_count + 1


def e_node_topology(d):
    node_with(d, "camera").model ^= 1


def e_nothing(d):
    pass


CASES = [
    # (scene, edit, bvh of the next descriptor, expected action)
    ("cornell", e_nothing, 1, abi.DRAW_REUSED),
    ("cornell_quad", e_nothing, 1, abi.DRAW_REUSED),
    ("two_level", e_nothing, 1, abi.DRAW_REUSED),
    ("cornell", e_camera_trs, 1, abi.DRAW_UPDATED),
    ("cornell", e_yfov, 1, abi.DRAW_UPDATED),
    ("cornell", e_light_colour, 1, abi.DRAW_UPDATED),
    ("cornell", e_light_intensity, 1, abi.DRAW_UPDATED),
    ("cornell", e_light_position, 1, abi.DRAW_UPDATED),
    ("cornell", e_material_colour, 1, abi.DRAW_UPDATED),
    ("two_level", e_camera_trs, 1, abi.DRAW_UPDATED),
    ("cornell_quad", e_quad_light_colour, 1, abi.DRAW_UPDATED),
    ("cornell", e_vertex_bit, 1, abi.DRAW_REBUILT),
    ("cornell", e_index, 1, abi.DRAW_REBUILT),
    ("two_level", e_texel, 1, abi.DRAW_REBUILT),
    ("cornell", e_normals_null, 1, abi.DRAW_REBUILT),
    ("cornell", e_mesh_node, 1, abi.DRAW_REBUILT),
    ("two_level", e_mesh_parent, 1, abi.DRAW_REBUILT),
    ("cornell_quad", e_quad_ab, 1, abi.DRAW_REBUILT),
    ("cornell_quad", e_quad_transform, 1, abi.DRAW_REBUILT),
    ("cornell", e_point_to_quad, 1, abi.DRAW_REBUILT),
    ("cornell_quad", e_quad_to_point, 1, abi.DRAW_REBUILT),
    ("cornell", e_one_more_node, 1, abi.DRAW_REBUILT),
    ("cornell", e_node_topology, 1, abi.DRAW_REBUILT),
    ("cornell", e_nothing, 0, abi.DRAW_REBUILT),
]


def compare(lib, resident, resident_bvh, nxt, next_bvh):
    action = C.c_uint32(99)
    rc = lib.rayca_hip_scene_desc_compare(resident.ptr(), resident_bvh, nxt.ptr(), next_bvh, C.byref(action))
    return rc, action.value


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1].__name__[2:]}-bvh{c[2]}" for c in CASES])
def test_decision_rule(product_lib, case):
    name, edit, next_bvh, want = case
    resident, nxt = SCENES[name](), SCENES[name]()
    assert compare(product_lib, resident, 1, nxt, 1) == (abi.OK, abi.DRAW_REUSED), "two flattens of one scene are the same descriptor"
    edit(nxt)
    assert compare(product_lib, resident, 1, nxt, next_bvh) == (abi.OK, want), abi.DRAW_NAMES[want]
    if want != abi.DRAW_REUSED:      # and the rule is symmetric: the edited descriptor resident, the original next
        assert compare(product_lib, nxt, next_bvh, resident, 1) == (abi.OK, want)
    assert compare(product_lib, nxt, next_bvh, nxt, next_bvh) == (abi.OK, abi.DRAW_REUSED)


def test_the_large_arrays_are_compared_whole(product_lib):
    """a million-triangle descriptor (tens of MB, compared in chunks on several threads): one bit flipped in the first, a
    middle and the last word of the positions, and in the last index byte, is found; the untouched copy is REUSED"""
    resident, nxt = flatten(scenes.soup_scene(1 << 18)), flatten(scenes.soup_scene(1 << 18))
    assert resident.positions.nbytes + resident.index_bytes.nbytes > (8 << 20)
    assert compare(product_lib, resident, 1, nxt, 1) == (abi.OK, abi.DRAW_REUSED)
    for at in (0, nxt.positions.size // 2 + 1, nxt.positions.size - 1):
        flip_bit(nxt.positions, at)
        assert compare(product_lib, resident, 1, nxt, 1) == (abi.OK, abi.DRAW_REBUILT), at
        flip_bit(nxt.positions, at)
    nxt.index_bytes[-1] ^= 1
    assert compare(product_lib, resident, 1, nxt, 1) == (abi.OK, abi.DRAW_REBUILT)
    nxt.index_bytes[-1] ^= 1
    assert compare(product_lib, resident, 1, nxt, 1) == (abi.OK, abi.DRAW_REUSED)


def test_a_descriptor_wrong_in_any_scene_is_an_error(product_lib):
    resident = cornell()
    bad = cornell()
    bad._materials[1].albedo_texture = 0      # the scene has no texture
    assert compare(product_lib, resident, 1, bad, 1)[0] == abi.ERR_BAD_ARG and "texture index" in last_error()
    bad = cornell()
    bad.c.abi_version = 1
    assert compare(product_lib, resident, 1, bad, 1)[0] == abi.ERR_BAD_ARG and "abi version" in last_error()
    bad = cornell()
    bad.c.materials = None
    assert compare(product_lib, resident, 1, bad, 1)[0] == abi.ERR_BAD_ARG and "materials is null" in last_error()
    bad = cornell()
    node_with(bad, "mesh").mesh = 1000
    assert compare(product_lib, resident, 1, bad, 1)[0] == abi.ERR_BAD_ARG and "mesh index" in last_error()
    # a count that merely differs is a rebuild, not an error
    more = cornell()
    extra = abi.RaycaMaterial()
    extra.albedo_texture = extra.normal_texture = extra.metallic_roughness_texture = abi.NONE
    more._materials = abi._array(abi.RaycaMaterial, list(more._materials[:more.c.material_count]) + [extra])
    more.c.materials, more.c.material_count = more._materials, more.c.material_count + 1
    assert compare(product_lib, resident, 1, more, 1) == (abi.OK, abi.DRAW_REBUILT)


def test_cpp_soft_renderer_compiles(product_lib, tmp_path):
    """compile only: the C++ mirror's SoftRenderer over the renderer handle -- two draws, last_draw(), move-only"""
    src = tmp_path / "resident.cpp"
    src.write_text(
        '#include <type_traits>\n'
        '#include <utility>\n'
        '#include "rayca.hpp"\n'
        "static_assert(!std::is_copy_constructible<rayca::SoftRenderer>::value, \"move-only\");\n"
        "static_assert(std::is_move_constructible<rayca::SoftRenderer>::value, \"move-only\");\n"
        "uint32_t twice(const rayca::Scene& scene, rayca::Image& image) {\n"
        "  rayca::SoftRenderer renderer = rayca::SoftRenderer::new_with_config(rayca::Config());\n"
        "  renderer.draw(scene, image);\n"
        "  renderer.draw(scene, image);\n"
        "  const rayca::DrawInfo info = renderer.last_draw();\n"
        "  rayca::SoftRenderer other = std::move(renderer);\n"
        "  other.invalidate();\n"
        "  return info.action == RAYCA_DRAW_REUSED ? (uint32_t)info.counters[RAYCA_DRAW_N_BUILDS] : 0u;\n"
        "}\n"
        "int32_t (*entry)(RaycaRenderer*, const RaycaSceneDesc*, const RaycaConfig*, uint32_t, uint32_t, const RaycaRenderOptions*, uint8_t*, float*,\n"
        "                 RaycaStats*, uint32_t*) = &rayca_hip_renderer_draw;\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "resident.o")], check=True)
