"""rayca_hip_surface_device / rayca_hip_camera_rays_device (DeviceScene.surface, .camera_rays, .gbuffer): what is at a hit, and
the rays a frame traces.

Comparisons are bit-exact where the value has one definition in the library (the Flat frame, the sub-sample identity of the
camera rays, o + d * t, the miss record, subsets of outputs, asynchronous against one-at-a-time) and carry a stated bound
where the expectation is computed here in float64 (normals).  Expected material data follows from the descriptor through a
restatement of the flatten order (model by model: mesh nodes in scene-graph order, their primitives' triangles and spheres,
then the model's quad lights, two triangles each) and rayca_hip_scene_primitive_order."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from flatten_order import conj, flat_table, rotate, world_trs
from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi, flatten, lib, scenes
from rayca_amd import model as M
from rayca_amd import sdtf
from rayca_amd.gltf import load_gltf
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = np.uint32(0xFFFFFFFF)
FLAT = Config(integrator=IntegratorStrategy.Flat, samples_per_pixel=1, gamma=1.0)
BUILDERS = [abi.BUILDER_REFERENCE, abi.BUILDER_SAH]
ALL = ("point", "normal", "color", "diffuse", "specular", "rough", "material", "flags")
SCENES = {"box": (61, 37), "cornell_quad": (61, 37), "spheres": (61, 37), "quad_jpg": (64, 48)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_desc(name):
    scene = M.Scene()
    if name == "box":
        scene.push_model(scenes.load_gltf(os.path.join(G, "box.gltf")))
        scene.push_model(M.create_default_model())
    elif name == "quad_jpg":
        expected = np.load(os.path.join(G, "jpeg", "expected.npz"))
        scene.push_model(load_gltf(os.path.join(G, "jpeg", "quad_jpg.gltf"), image_decoder=lambda raw: expected["base_420_odd"]))
        scene.push_model(M.create_default_model())
    else:
        sdtf.push_sdtf_from_path(scene, os.path.join(G, name + ".sdtf"))
    return flatten(scene)


def make_scene(desc, builder):
    ds = DeviceScene(desc, Config(), builder=builder)
    if builder == abi.BUILDER_SAH:
        ds.finish()
    return ds


def host(g):
    import torch
    torch.cuda.synchronize()
    out = {}
    for k, v in g.items():
        a = v.cpu().numpy()
        out[k] = a.view(np.uint32) if a.dtype == np.int32 else a
    return out


_CASES = {}


def case(gpu, name, builder):
    """(desc, rays, gbuffer as numpy) of one scene and builder, made once and shared (read-only) by the tests below"""
    key = (name, builder)
    if key not in _CASES:
        w, h = SCENES[name]
        desc = make_desc(name)
        ds = make_scene(desc, builder)
        rays = ds.camera_rays(FLAT, w, h)
        uv = ds.query(rays)[2]
        g = host(ds.gbuffer(FLAT, w, h))
        u8, f32, _ = ds.render(FLAT, w, h)
        _CASES[key] = dict(desc=desc, rays=rays.cpu().numpy(), uv=uv.cpu().numpy(), g=g, u8=u8, f32=f32, order=ds.primitive_order(), w=w, h=h)
        ds.close()
    return _CASES[key]


def vertex_normal_sum(desc, pi, tri):
    """the three descriptor vertex normals of a triangle, added up (Vertex::default() normal +Z without a normal array)"""
    p = desc._prims[pi]
    width = {abi.INDEX_U8: 1, abi.INDEX_U16: 2, abi.INDEX_U32: 4}[p.index_type]
    raw = desc.index_bytes[p.index_byte_offset + 3 * tri * width: p.index_byte_offset + 3 * (tri + 1) * width]
    idx = raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[width]).astype(np.int64) + p.first_vertex
    return desc.normals[idx].astype(np.float64).sum(0) if desc.normals is not None else np.array([0.0, 0.0, 3.0])


def is_emissive(m):   # phong.rs:54-56: emission not close to BLACK (0, 0, 0, 1)
    eps = np.finfo(np.float32).eps
    e = np.array(list(m.emission), np.float32)
    return m.kind == abi.MATERIAL_PHONG and not (np.abs(e - np.array([0, 0, 0, 1], np.float32)) < eps).all()


def expected_flat(color):
    """BLACK + color with the oracle's alpha-weighted `+`, per pixel; RGBA8 through the oracle's quantiser.  Color::BLACK is
    (0, 0, 0, 1) and `a + b` = (a.rgb + b.rgb * b.a, a.a): a miss, whose surface colour is (0, 0, 0, 0), gives (0, 0, 0, 1), the
    pixel Flat writes for unwrap_or(BLACK)."""
    L = ol.load()
    n = color.shape[0]
    f32, u8 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.uint8)
    black = ol.f4((0.0, 0.0, 0.0, 1.0))
    out, q = (C.c_float * 4)(), (C.c_uint8 * 4)()
    for i in range(n):
        L.oracle_color_add(black, ol.f4(color[i]), out)
        L.oracle_rgba8_from_color(out, q)
        f32[i], u8[i] = out[:], q[:]
    return f32, u8


# ---- 1: Flat equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_flat_frame_equals_black_plus_color(gpu, name, builder):
    c = case(gpu, name, builder)
    g, n = c["g"], c["w"] * c["h"]
    hit = g["prim"].reshape(-1) != NONE
    print(f"{name} builder {builder}: {hit.sum()} of {n} pixels hit")
    assert 0.05 * n < hit.sum() and g["color"].shape == (c["h"], c["w"], 4)
    color = g["color"].reshape(-1, 4)
    assert not bits(color[~hit]).any(), "a miss is (0, 0, 0, 0)"
    f32, u8 = expected_flat(color)
    bad = np.flatnonzero((bits(f32) != bits(c["f32"].reshape(-1, 4))).any(1))
    assert bad.size == 0, f"{bad.size} pixels differ, first {bad[:5]}: frame {c['f32'].reshape(-1, 4)[bad[:3]]} gbuffer {f32[bad[:3]]}"
    assert np.array_equal(u8, c["u8"].reshape(-1, 4))


# ---- 2: sub-samples and tiles of the camera rays ----------------------------------------------------------------------------
def test_sub_samples_are_pixels_of_the_doubled_frame(gpu):
    desc = make_desc("cornell_quad")
    ds = make_scene(desc, abi.BUILDER_REFERENCE)
    W, H = 16, 12
    big = ds.camera_rays(FLAT, 2 * W, 2 * H).cpu().numpy().reshape(2 * H, 2 * W, 6)
    spp4 = Config(integrator=IntegratorStrategy.Flat, samples_per_pixel=4)
    for s in range(4):
        got = ds.camera_rays(spp4, W, H, sample=s).cpu().numpy().reshape(H, W, 6)
        want = big[s // 2::2, s % 2::2]
        assert np.array_equal(bits(got), bits(want)), f"sample {s}: {(bits(got) != bits(want)).sum()} words differ"
    assert not np.array_equal(ds.camera_rays(spp4, W, H, sample=0).cpu().numpy(), ds.camera_rays(spp4, W, H, sample=3).cpu().numpy())
    # a tile: part 1 of 3, bands of 8 rows, of a 16 x 40 frame = rows 8..15 and 32..39 of the whole export
    whole = ds.camera_rays(FLAT, 16, 40).cpu().numpy().reshape(40, 16, 6)
    part = ds.camera_rays(FLAT, 16, 40, tile=(1, 3, 8)).cpu().numpy()
    assert ds.tile_rows((1, 3, 8), 40) == 16 and part.shape == (16 * 16, 6)
    assert np.array_equal(bits(part.reshape(16, 16, 6)), bits(np.concatenate([whole[8:16], whole[32:40]])))
    ds.close()


# ---- 3: geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["box", "cornell_quad", "quad_jpg"])
def test_point_is_origin_plus_t_times_direction(gpu, name, builder):
    c = case(gpu, name, builder)
    g = c["g"]
    flags = g["flags"].reshape(-1)
    tri = ((flags >> 31) == 1) & ((flags & abi.SURFACE_SPHERE) == 0)
    assert tri.sum() > 100
    o, d, t = c["rays"][:, :3], c["rays"][:, 3:], g["t"].reshape(-1)
    want = (o + d * t[:, None]).astype(np.float32)   # float32 throughout: one rounding per operation, as the uncontracted kernel
    assert np.array_equal(bits(g["point"].reshape(-1, 3)[tri]), bits(want[tri]))


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["box", "cornell_quad"])
def test_normals_of_flat_faces(gpu, name, builder):
    c = case(gpu, name, builder)
    desc, g = c["desc"], c["g"]
    table, trs = flat_table(desc), world_trs(desc)
    orc = ol.OracleScene(desc, Config())
    wt = orc.world_triangles(table.shape[0]).astype(np.float64).reshape(-1, 3, 3)
    orc.close()
    flags, prim = g["flags"].reshape(-1), g["prim"].reshape(-1)
    normal = g["normal"].reshape(-1, 3).astype(np.float64)
    hit = (flags >> 31) == 1
    assert np.abs(np.linalg.norm(normal[hit], axis=1) - 1.0).max() <= 1e-6
    tri = np.flatnonzero(hit & ((flags & abi.SURFACE_SPHERE) == 0))
    flat = c["order"][prim[tri]]
    n_geo = np.cross(wt[flat, 1] - wt[flat, 0], wt[flat, 2] - wt[flat, 0])
    n_geo /= np.linalg.norm(n_geo, axis=1)[:, None]
    along = (normal[tri] * n_geo).sum(1)
    print(f"{name}: min |dot(normal, n_geo)| = {np.abs(along).min():.9f} over {tri.size} triangle hits")
    assert np.abs(along).min() >= 1.0 - 1e-5
    checked = 0
    for f in np.unique(flat):
        node, pi, k = table[f, 0], table[f, 1], table[f, 2]
        if pi < 0:
            continue   # (a quad light's triangles have no vertices in the descriptor)
        ref = rotate(vertex_normal_sum(desc, pi, k), trs[node][1])
        sel = flat == f
        assert (np.sign((normal[tri][sel] * ref).sum(1)) == 1).all(), f"flat primitive {f}"
        checked += 1
    assert checked >= 2   # (the Box shows one face: two triangles)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["spheres", "cornell_quad"])
def test_sphere_normals(gpu, name, builder):
    c = case(gpu, name, builder)
    desc, g = c["desc"], c["g"]
    table, trs = flat_table(desc), world_trs(desc)
    flags, prim = g["flags"].reshape(-1), g["prim"].reshape(-1)
    sph = np.flatnonzero((flags & abi.SURFACE_SPHERE) != 0)
    assert sph.size > 30 and ((flags[sph] >> 31) == 1).all()
    flat = c["order"][prim[sph]]
    assert (table[flat, 4] == 1).all()
    point, normal = g["point"].reshape(-1, 3).astype(np.float64)[sph], g["normal"].reshape(-1, 3).astype(np.float64)[sph]
    worst = 0.0
    for i, f in enumerate(flat):
        t, q, s = trs[table[f, 0]]
        p = desc._prims[table[f, 1]]
        local = rotate(point[i] - t, conj(q)) / s - np.array(list(p.sphere_center), np.float64)
        n = rotate(local / np.linalg.norm(local) / s, q)   # transpose(inverse(R S)) = R S^-1
        worst = max(worst, np.abs(normal[i] - n / np.linalg.norm(n)).max())
    print(f"{name}: sphere normals within {worst:.3g}")
    assert worst <= 1e-5


# ---- 4: materials -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_material_records(gpu, name, builder):
    c = case(gpu, name, builder)
    desc, g = c["desc"], c["g"]
    table = flat_table(desc)
    assert table.shape[0] == c["order"].size
    flags, prim, material = g["flags"].reshape(-1), g["prim"].reshape(-1), g["material"].reshape(-1)
    hit = prim != NONE
    assert np.array_equal((flags >> 31) == 1, hit)
    assert (material[~hit] == NONE).all() and (flags[~hit] == 0).all()
    h = np.flatnonzero(hit)
    flat = c["order"][prim[h]]
    want_mat = table[flat, 3].astype(np.uint32)
    assert np.array_equal(material[h], want_mat)
    assert np.array_equal((flags[h] & abi.SURFACE_SPHERE) != 0, table[flat, 4] == 1)
    mats = desc._materials
    kind = np.array([mats[m].kind if m != NONE else abi.MATERIAL_PBR for m in want_mat], np.uint32)
    emissive = np.array([m != NONE and is_emissive(mats[m]) for m in want_mat])
    assert np.array_equal(flags[h] & abi.SURFACE_KIND_MASK, kind)
    assert np.array_equal((flags[h] & abi.SURFACE_EMISSIVE) != 0, emissive)
    if name == "cornell_quad":   # the lamp under the ceiling is seen, and most of the frame is not emissive
        assert emissive.sum() > 10 and (~emissive).sum() > 100
    color, diffuse, specular = (g[k].reshape(-1, 4)[h] for k in ("color", "diffuse", "specular"))
    pbr = kind == abi.MATERIAL_PBR
    assert np.array_equal(bits(diffuse[pbr]), bits(color[pbr]))
    # Phong and GGX: get_diffuse = geometry colour x diffuse, get_specular = specular.  The vertex colours of these scenes are
    # white, so a triangle's geometry colour is (w2 + u) + v in r, g, b (primitive.rs:15-28 interpolates them) and a sphere's is 1
    assert desc.colors is None or (desc.colors == 1.0).all()
    u, v = c["uv"][h, 0], c["uv"][h, 1]
    gc = np.where(table[flat, 4] == 1, np.float32(1.0), ((np.float32(1.0) - u - v) + u) + v).astype(np.float32)
    for i in np.flatnonzero(~pbr):
        m = mats[want_mat[i]]
        d = np.array(list(m.diffuse), np.float32)
        want_d = np.array([gc[i] * d[0], gc[i] * d[1], gc[i] * d[2], d[3]], np.float32)
        assert np.array_equal(bits(diffuse[i]), bits(want_d)), (i, diffuse[i], want_d)
        assert np.array_equal(specular[i], np.array(list(m.specular), np.float32))
    if name in ("cornell_quad", "spheres"):
        assert (~pbr).sum() > 100


@pytest.mark.parametrize("builder", BUILDERS)
def test_quad_light_triangles_are_emissive(gpu, builder):
    """The quad light's two triangles lie in the plane of the lamp mesh, whose triangles come first in the reference's order and
    win the depth tie: no camera ray returns them.  A caller's record may name them all the same."""
    import torch
    c = case(gpu, "cornell_quad", builder)
    desc, table = c["desc"], flat_table(c["desc"])
    light_flat = np.flatnonzero(table[:, 1] < 0)
    assert light_flat.size == 2
    slot_of = np.empty(c["order"].size, np.uint32)
    slot_of[c["order"]] = np.arange(c["order"].size, dtype=np.uint32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ds = make_scene(desc, builder)
    assert np.array_equal(ds.primitive_order(), c["order"])
    got = host(ds.surface(None, dev(np.ones(2, np.float32)), dev(slot_of[light_flat].view(np.int32)), dev(np.full((2, 2), 0.25, np.float32)),
                          want=("color", "material", "flags")))
    ds.close()
    m = int(table[light_flat[0], 3])
    assert m != int(NONE) and is_emissive(desc._materials[m]), "the light's material is emissive in the descriptor"
    assert (got["material"] == np.uint32(m)).all()
    assert (got["flags"] == np.uint32(0x80000000 | abi.SURFACE_EMISSIVE | desc._materials[m].kind)).all()


def test_material_update_shows_in_the_next_records(gpu):
    desc = make_desc("cornell_quad")
    ds = make_scene(desc, abi.BUILDER_SAH)
    w, h = SCENES["cornell_quad"]
    first = host(ds.gbuffer(FLAT, w, h, want=("color", "material")))
    before = first["color"]
    seen = first["material"][first["material"] != NONE]
    m = desc._materials[int(np.bincount(seen).argmax())]   # the material most pixels show
    # get_color: Pbr colour, Phong ambient + emission, Ggx diffuse (material/mod.rs:107-113)
    getattr(m, {abi.MATERIAL_PBR: "color", abi.MATERIAL_PHONG: "ambient", abi.MATERIAL_GGX: "diffuse"}[m.kind])[:] = (0.25, 0.5, 0.125, 1.0)
    ds.update(desc)
    after = host(ds.gbuffer(FLAT, w, h, want=("color",)))["color"]
    u8, f32, _ = ds.render(FLAT, w, h)
    assert not np.array_equal(before, after)
    ef32, eu8 = expected_flat(after.reshape(-1, 4))
    assert np.array_equal(bits(ef32), bits(f32.reshape(-1, 4))) and np.array_equal(eu8, u8.reshape(-1, 4))
    ds.close()


# ---- 5: records that are not hits, guards, subsets of outputs ---------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_non_hits_guards_and_output_subsets(gpu, builder):
    import torch
    c = case(gpu, "cornell_quad", builder)
    desc = c["desc"]
    ds = make_scene(desc, builder)
    n = c["w"] * c["h"]
    g = c["g"]
    t, prim, uv = g["t"].reshape(-1).copy(), g["prim"].reshape(-1).copy(), c["uv"]
    rays_d = torch.from_numpy(c["rays"]).cuda()
    hit = np.flatnonzero(prim != NONE)
    assert hit.size > 300
    # half of the hits become non-hits of three kinds; the frame's genuine misses (if any) stay
    kinds = np.zeros(n, np.int64)
    kinds[hit[1::6]] = 1
    kinds[hit[4::6]] = 2
    prim2 = prim.copy()
    prim2[kinds == 1] = c["order"].size          # prim = prim_count
    prim2[kinds == 2] = 0xFFFFFFFE
    t2 = t.copy()
    miss_extra = hit[2::6]                       # and a third kind: the query's own miss record
    prim2[miss_extra], t2[miss_extra], kinds[miss_extra] = NONE, np.float32(3.4028234663852886e38), 3
    uv2 = uv.copy()
    uv2[miss_extra] = 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # flat buffers: 64 four-byte elements = 256 bytes of guard in front of and behind each output
    width = {k: (w or 1) for k, (_, w) in DeviceScene.SURFACE_OUTPUTS.items()}
    guard = {k: (-7.0 if DeviceScene.SURFACE_OUTPUTS[k][0] == "float32" else 0x5A5A5A5A) for k in ALL}
    big = {k: torch.full((n * width[k] + 128,), guard[k], dtype=getattr(torch, DeviceScene.SURFACE_OUTPUTS[k][0]), device="cuda") for k in ALL}
    out = {k: big[k][64:64 + n * width[k]].view((n, width[k]) if DeviceScene.SURFACE_OUTPUTS[k][1] else (n,)) for k in ALL}
    got = host(ds.surface(rays_d, dev(t2), dev(prim2.view(np.int32)), dev(uv2), out=out))
    nonhit = (kinds != 0) | (prim == NONE)
    assert all((kinds == k).sum() > 50 for k in (1, 2, 3)) and (~nonhit).sum() > 150
    for k in ALL:
        assert bool((big[k][:64] == guard[k]).all()) and bool((big[k][64 + n * width[k]:] == guard[k]).all()), k
        if k == "material":
            assert (got[k][nonhit] == NONE).all()
        else:
            assert not bits(got[k][nonhit]).any(), k
        # the hits are what they are without the bad neighbours
        assert np.array_equal(bits(got[k][~nonhit]), bits(g[k].reshape(n, -1)[~nonhit].reshape(got[k][~nonhit].shape))), k
    # every output on its own gives the values it has among all eight
    for k in ALL:
        rays_arg = rays_d if k in ("point", "normal") else None
        one = host(ds.surface(rays_arg, dev(t2), dev(prim2.view(np.int32)), dev(uv2), want=(k,)))
        assert list(one) == [k] and np.array_equal(bits(one[k]), bits(got[k])), k
    # a colour output that is only 4-byte aligned (the guarded ones above are 16-byte aligned) holds the same values
    odd = torch.full((n * 4 + 128,), -7.0, dtype=torch.float32, device="cuda")
    one = host(ds.surface(None, dev(t2), dev(prim2.view(np.int32)), dev(uv2), want=("color",), out={"color": odd[65:65 + n * 4].view(n, 4)}))
    assert odd[65:].data_ptr() % 16 == 4 and np.array_equal(bits(one["color"]), bits(got["color"]))
    assert bool((odd[:65] == -7.0).all()) and bool((odd[65 + n * 4:] == -7.0).all())
    ds.close()


# ---- 6: asynchrony ----------------------------------------------------------------------------------------------------------
def test_four_contexts_back_to_back_on_a_side_stream(gpu):
    import torch
    desc = make_desc("cornell_quad")
    ds = make_scene(desc, abi.BUILDER_SAH)
    sizes = [(61, 37), (64, 48), (33, 70), (80, 45)]
    solo = []
    for k, (w, h) in enumerate(sizes):
        solo.append(host(ds.gbuffer(FLAT, w, h, context=k)))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = []
    for k, (w, h) in enumerate(sizes):
        rays = ds.camera_rays(FLAT, w, h, stream=side, context=k)
        t, prim, uv = ds.query(rays, stream=side, context=k)
        s = ds.surface(rays, t, prim, uv, stream=side, context=k)
        s["t"], s["prim"] = t, prim
        res.append(s)
    for k, (w, h) in enumerate(sizes):
        got = host(res[k])
        for name, want in solo[k].items():
            assert np.array_equal(bits(got[name]).reshape(-1), bits(want).reshape(-1)), f"context {k} {name}"
    ds.close()


def test_surface_beside_a_frame_in_flight(gpu):
    import torch
    ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
    ds.finish()
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, max_depth=3)
    W, H = 1920, 1080
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    frame_solo = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    frame = torch.zeros_like(frame_solo)
    rays = ds.camera_rays(FLAT, 640, 360)
    t, prim, uv = ds.query(rays)
    torch.cuda.synchronize()
    for _ in range(20):   # (past the scene's format calibration, as test_query_beside_a_frame_in_flight)
        ds.render_device(cfg, W, H, frame_solo.data_ptr(), stream=s0.cuda_stream, context=0)
    torch.cuda.synchronize()
    solo = host(ds.surface(rays, t, prim, uv, stream=s1, context=1))
    ds.render_device(cfg, W, H, frame.data_ptr(), stream=s0.cuda_stream, context=0)
    beside = ds.surface(rays, t, prim, uv, stream=s1, context=1)
    torch.cuda.synchronize()
    assert torch.equal(frame, frame_solo) and int(frame.max()) > 0
    beside = host(beside)
    for k in ALL:
        assert np.array_equal(bits(beside[k]), bits(solo[k])), k
    assert ((solo["flags"] >> 31) == 1).mean() > 0.5
    ds.close()


# ---- 7: errors with a scene -------------------------------------------------------------------------------------------------
def test_errors_with_a_scene(gpu):
    import torch
    desc = make_desc("box")
    ds = make_scene(desc, abi.BUILDER_SAH)
    rays = ds.camera_rays(FLAT, 8, 8)
    t, prim, uv = ds.query(rays)
    n = 64
    color = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    normal = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")

    def call(count=n, with_rays=True, want_normal=False, tile_parts=0, **o_fields):
        q = abi.RaycaSurfaceQuery()
        q.count, q.t, q.prim, q.uv, q.color_out = count, t.data_ptr(), prim.data_ptr(), uv.data_ptr(), color.data_ptr()
        q.rays = rays.data_ptr() if with_rays else None
        q.normal_out = normal.data_ptr() if want_normal else None
        o = abi.RaycaRenderOptions()
        o.tile.parts = tile_parts
        for k, v in o_fields.items():
            setattr(o, k, v)
        return gpu.rayca_hip_surface_device(ds.handle, C.byref(o), C.byref(q), None)

    assert call(context=8) == abi.ERR_BAD_ARG and "context" in lib.last_error()
    assert call(traversal=abi.TRAVERSAL_EXHAUSTIVE) == abi.ERR_BAD_ARG
    assert call(engine=abi.ENGINE_WAVEFRONT) == abi.ERR_BAD_ARG
    assert call(tile_parts=2) == abi.ERR_BAD_ARG and "tile" in lib.last_error()
    assert call(with_rays=False, want_normal=True) == abi.ERR_BAD_ARG and "rays" in lib.last_error()
    assert call(count=0) == abi.OK
    torch.cuda.synchronize()
    assert bool((color == -7.0).all()) and bool((normal == -7.0).all())   # nothing of the above wrote anything
    assert call(with_rays=False) == abi.OK and call(want_normal=True) == abi.OK
    assert bool((color != -7.0).all()) and bool((normal != -7.0).all())
    with pytest.raises(RaycaError) as e:
        ds.camera_rays(Config(samples_per_pixel=4), 8, 8, sample=4)
    assert e.value.code == abi.ERR_BAD_ARG
    with pytest.raises(RaycaError) as e:
        ds.camera_rays(FLAT, 8, 8, context=8)
    assert e.value.code == abi.ERR_BAD_ARG
    with pytest.raises(ValueError):
        ds.surface(None, t, prim, uv, want=("normal",))
    with pytest.raises(ValueError):
        ds.surface(rays, t, prim, uv, want=("albedo",))
    with pytest.raises(TypeError):
        ds.surface(rays, t, prim.float(), uv)
    assert ds.surface(rays[:0], t[:0], prim[:0], uv[:0])["color"].shape == (0, 4)
    ds.close()
    # an empty scene: a camera and nothing to hit
    empty = M.Scene()
    empty.push_model(M.create_default_model())
    es = DeviceScene(flatten(empty), Config())
    q = abi.RaycaSurfaceQuery()
    q.count, q.t, q.prim, q.uv, q.color_out = n, t.data_ptr(), prim.data_ptr(), uv.data_ptr(), color.data_ptr()
    assert gpu.rayca_hip_surface_device(es.handle, None, C.byref(q), None) == abi.ERR_EMPTY_SCENE
    es.close()
