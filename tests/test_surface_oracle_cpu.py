"""oracle_surface (OracleScene.surface) pinned before the GPU tests use it as their reference, and the image-range refusals, all
without a GPU.

The hook is checked from two sides: against the oracle's own Flat render (the colour of the record under every camera ray is
the pixel), and against arithmetic written here in float64 numpy from the descriptor alone -- interpolated normals, the TBN
product with the decoded texel, the texel address of the wrap rule, metallic = b and roughness = r, kd, ks and the Phong
roughness.  Bounds: 1e-6 absolute on unit vectors (what the existing normal tests allow), 4 ulp on products of two or three
f32 factors, exact where the value is a word of the descriptor or one f32 operation on it."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import surface_cases as sc
from flatten_order import flat_table, rotate, world_trs
from rayca_amd import Config, abi, flatten, scenes, sdtf
from rayca_amd import model as M
from rayca_amd.lib import last_error

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = sc.NONE
ALL = tuple(ol.OracleScene.SURFACE_OUTPUTS)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def zoo():
    desc = sc.zoo_desc()
    orc = ol.OracleScene(desc, Config())
    rec = sc.records(desc, orc)
    prim = sc.slots(rec, orc.primitive_order())
    out = orc.surface(rec["rays"], rec["t"], prim, rec["uv"])
    yield dict(desc=desc, orc=orc, rec=rec, prim=prim, out=out)
    orc.close()


def test_every_branch_is_reached(zoo):
    counts = sc.branch_counts(zoo["desc"], zoo["rec"])
    print("\n".join(f"{k:32s} {v}" for k, v in counts.items()))
    assert all(v > 0 for v in counts.values()), {k: v for k, v in counts.items() if v <= 0}
    assert 15000 <= counts["records"] <= 25000
    assert flat_table(zoo["desc"]).shape[0] <= 300


def test_the_images_sit_at_non_trivial_offsets(zoo):
    desc = zoo["desc"]
    images = [(i.width, i.height, i.color_type, i.byte_offset) for i in desc._images[:desc.c.image_count]]
    # 45 bytes of RGB8 twice: the image behind each starts on the next word, where flatten() pads to
    assert images == [(5, 3, abi.COLOR_RGB8, 0), (1, 1, abi.COLOR_RGBA8, 48), (8, 8, abi.COLOR_RGBA8, 52), (7, 2, abi.COLOR_RGBA32F, 308),
                      (3, 5, abi.COLOR_RGB8, 532), (3, 2, abi.COLOR_RGBA32F, 580)]
    assert desc.image_bytes.size == 580 + 3 * 2 * 16
    f = desc.image_bytes[308:308 + 7 * 2 * 16].view(np.float32)
    assert (f < 0).any() and (f > 255).any() and (f != np.floor(f)).all()
    assert len(set(desc.image_bytes[52:308].reshape(-1, 4)[:, 3])) > 20   # the 8 x 8 image's alpha


def test_color_of_the_camera_rays_records_is_the_flat_frame(zoo):
    orc, L = zoo["orc"], ol.load()
    rays = orc.camera_rays(sc.FLAT, sc.W, sc.H)
    t, prim, uv, _ = orc.trace_rays(rays)
    color = orc.surface(None, t, prim, uv, want=("color",))["color"]
    _, f32, _ = orc.render(sc.FLAT, sc.W, sc.H)
    assert 500 < (prim != NONE).sum() < sc.W * sc.H and np.unique(prim).size == orc.primitive_count + 1   # every primitive is seen, and the background
    black, out = ol.f4((0.0, 0.0, 0.0, 1.0)), (C.c_float * 4)()
    want = np.zeros((sc.W * sc.H, 4), np.float32)
    for i in range(want.shape[0]):
        L.oracle_color_add(black, ol.f4(color[i]), out)
        want[i] = out[:]
    bad = np.flatnonzero((bits(want) != bits(f32.reshape(-1, 4))).any(1))
    assert bad.size == 0, f"{bad.size} pixels differ, first {bad[:5]}"


def world_attributes(desc):
    """float64 per vertex: normals under R S^-1 (the transpose of the inverse of R S), tangents and bitangents under R S, of the
    node each vertex's triangles hang under (every vertex of the zoo belongs to one node)"""
    table, trs = flat_table(desc), world_trs(desc)
    corners = sc.corner_vertices(desc, table)
    n, t, b = (np.zeros((desc.positions.shape[0], 3)) for _ in range(3))
    for f in np.flatnonzero(corners[:, 0] >= 0):
        _, q, s = trs[table[f, 0]]
        for v in corners[f]:
            n[v] = rotate(desc.normals[v].astype(np.float64) / s, q)
            t[v] = rotate(desc.tangents[v].astype(np.float64) * s, q)
            b[v] = rotate(desc.bitangents[v].astype(np.float64) * s, q)
    return table, corners, n, t, b


def unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def within_ulps(got, want, ulps=4):
    want = np.asarray(want, np.float64)
    err = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float32).tiny).astype(np.float32))
    return float(err.max()) if err.size else 0.0, ulps


def geometry_color(colors, corners, uv):
    """BvhGeometry::get_color in float32: the corners' colours scaled by their weights (Mul<f32> keeps alpha) and added with the
    colours' own `+`, a.rgb + b.rgb * b.a with a's alpha (color/mod.rs) -- so not a plain interpolation once alphas differ"""
    u, v = uv[:, :1], uv[:, 1:]
    w2 = np.float32(1.0) - u - v
    c2, c0, c1 = (colors[corners[:, k]] for k in (2, 0, 1))
    rgb = (c2[:, :3] * w2 + (c0[:, :3] * u) * c0[:, 3:]) + (c1[:, :3] * v) * c1[:, 3:]
    return np.concatenate([rgb, c2[:, 3:]], 1)


def test_records_against_float64_arithmetic_from_the_descriptor(zoo):
    desc, rec, out = zoo["desc"], zoo["rec"], zoo["out"]
    table, corners, wn, wt, wb = world_attributes(desc)
    u, v = rec["uv"][:, 0], rec["uv"][:, 1]
    # the sample: every lattice record inside its triangle, corners and edges included (outside, a weight is negative and the
    # interpolated vectors may cancel: no bound on a unit vector follows from the formats there)
    sample = np.flatnonzero((rec["what"] == 0) & (u >= 0) & (v >= 0) & (u + v <= 1))
    assert sample.size > 5000
    flat = rec["flat"][sample]
    c3 = corners[flat]
    uv64 = rec["uv"][sample].astype(np.float64)
    w = np.stack([uv64[:, 0], uv64[:, 1], 1.0 - uv64[:, 0] - uv64[:, 1]], 1)
    interp64 = lambda a: sum(a[c3[:, k]] * w[:, k:k + 1] for k in range(3))
    normal, tangent, bitangent = unit(interp64(wn)), unit(interp64(wt)), unit(interp64(wb))
    tex_uv = sc.interpolate(desc.uvs, c3, rec["uv"][sample])                 # float32, as both sides spell it: it decides the texel
    gc = geometry_color(desc.colors, c3, rec["uv"][sample]).astype(np.float64)
    mat = table[flat, 3].astype(np.uint32)
    got = {k: a[sample] for k, a in out.items()}
    assert np.array_equal(got["material"], mat) and set(mat.tolist()) == set(range(9)) | {10, int(NONE)}   # (9 is the sphere's)
    worst = {}

    def note(name, pair):
        err, bound = pair
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= bound, (name, err)

    for m in np.unique(mat):
        s = mat == m
        mm = desc._materials[m] if m != NONE else None
        kind = mm.kind if mm is not None else abi.MATERIAL_PBR
        f64 = lambda name: np.array(list(getattr(mm, name)), np.float32).astype(np.float64)
        assert (got["flags"][s] & abi.SURFACE_KIND_MASK == kind).all() and (got["flags"][s] >> 31 == 1).all()
        want_normal = normal[s]
        if kind == abi.MATERIAL_PBR:
            base = np.tile(f64("color") if mm is not None else np.ones(4), (s.sum(), 1))
            metallic = np.full(s.sum(), np.float32(mm.metallic_factor if mm is not None else 0.0), np.float32)
            roughness = np.full(s.sum(), np.float32(mm.roughness_factor if mm is not None else 1.0), np.float32)
            if mm is not None and mm.albedo_texture != abi.NONE:
                base = base * (sc.texel(desc, mm.albedo_texture, tex_uv[s])[0] / 255.0)
            if mm is not None and mm.metallic_roughness_texture != abi.NONE:
                words = sc.texel(desc, mm.metallic_roughness_texture, tex_uv[s])[0].astype(np.float32)
                metallic, roughness = words[:, 2] / np.float32(255.0), words[:, 0] / np.float32(255.0)   # (b, r): one f32 division each
            if mm is not None and mm.normal_texture != abi.NONE:
                c = sc.texel(desc, mm.normal_texture, tex_uv[s])[0] / 255.0
                sn = c[:, :3] * c[:, 3:] * 2.0 - 1.0
                product = tangent[s] * sn[:, :1] + bitangent[s] * sn[:, 1:2] + normal[s] * sn[:, 2:]
                want_normal = unit(product)
            note("pbr color", within_ulps(got["color"][s], gc[s] * base))
            assert np.array_equal(bits(got["diffuse"][s]), bits(got["color"][s]))
            # f32 * Color scales rgb and keeps the colour's alpha
            note("pbr specular", within_ulps(got["specular"][s], np.concatenate([metallic.astype(np.float64)[:, None] * base[:, :3], base[:, 3:]], 1)))
            assert np.array_equal(bits(got["rough"][s, 0]), bits(roughness)), m          # the texel address, exactly
            assert not bits(got["rough"][s, 1]).any()
        else:
            if kind == abi.MATERIAL_PHONG:   # ambient + emission, the colours' alpha-weighted sum (color/mod.rs)
                a, e = f64("ambient"), f64("emission")
                mc = np.append(a[:3] + e[:3] * e[3], a[3])
                want_rough = np.clip(np.sqrt(2.0 / (np.float64(np.float32(mm.shininess)) + 2.0)), 0.0, 1.0)
                note("phong roughness", within_ulps(got["rough"][s, 0], np.full(s.sum(), want_rough)))
                assert (got["rough"][s, 1] == np.float32(mm.shininess)).all()
            else:
                mc = f64("diffuse")
                assert (got["rough"][s, 0] == np.float32(mm.roughness_factor)).all() and (got["rough"][s, 1] == np.float32(mm.shininess)).all()
            note("color", within_ulps(got["color"][s], gc[s] * mc))
            note("kd", within_ulps(got["diffuse"][s], gc[s] * f64("diffuse")))
            assert (got["specular"][s] == np.array(list(mm.specular), np.float32)).all()
        err = float(np.abs(got["normal"][s].astype(np.float64) - want_normal).max())
        worst["normal"] = max(worst.get("normal", 0.0), err)
        assert err <= 1e-6, (m, err)
    print({k: float(f"{v:.3g}") for k, v in worst.items()})
    # point = o + d * t, one rounding per operation
    o, d, t = rec["rays"][sample, :3], rec["rays"][sample, 3:], rec["t"][sample]
    assert np.array_equal(bits(got["point"]), bits((o + d * t[:, None]).astype(np.float32)))


def test_sphere_records(zoo):
    """the sphere ignores its material's normal texture: the normal is the float64 sphere normal of test_sphere_normals, and the
    material terms are the factors"""
    desc, rec, out = zoo["desc"], zoo["rec"], zoo["out"]
    table, trs = flat_table(desc), world_trs(desc)
    sph = np.flatnonzero((rec["what"] == 1) & (out["flags"] & abi.SURFACE_SPHERE != 0))
    assert sph.size > 100
    row = table[rec["flat"][sph[0]]]
    t, q, s = trs[row[0]]
    p, mm = desc._prims[row[1]], desc._materials[row[3]]
    assert mm.normal_texture != abi.NONE and row[4] == 1
    from flatten_order import conj
    worst = 0.0
    for i in sph:
        local = rotate(out["point"][i].astype(np.float64) - t, conj(q)) / s - np.array(list(p.sphere_center), np.float64)
        n = rotate(local / np.linalg.norm(local) / s, q)
        worst = max(worst, np.abs(out["normal"][i] - n / np.linalg.norm(n)).max())
    print(f"sphere normals within {worst:.3g}")
    assert worst <= 1e-5
    assert (out["color"][sph] == np.array(list(mm.color), np.float32)).all() and np.array_equal(out["diffuse"][sph], out["color"][sph])
    assert (out["rough"][sph] == np.array([mm.roughness_factor, 0.0], np.float32)).all()
    assert (out["flags"][sph] == np.uint32(0x80000000 | abi.SURFACE_SPHERE | abi.MATERIAL_PBR)).all()


def test_misses_and_null_outputs(zoo):
    orc, rec, prim, out = zoo["orc"], zoo["rec"], zoo["prim"], zoo["out"]
    miss = prim >= orc.primitive_count
    assert all(((rec["what"] == 2) & (prim == p)).sum() > 20 for p in (orc.primitive_count, 0xFFFFFFFE, 0xFFFFFFFF))
    for k in ALL:
        if k == "material":
            assert (out[k][miss] == NONE).all() and (out[k][~miss] != NONE).sum() > 10000
        else:
            assert not bits(out[k][miss]).any(), k
    assert (out["flags"][~miss] >> 31 == 1).all()
    # every output alone, and the `full = false` trio without rays, give the values they have among all eight
    for want in [(k,) for k in ALL] + [("color", "material", "flags")]:
        rays = rec["rays"] if set(want) & {"point", "normal"} else None
        one = orc.surface(rays, rec["t"], prim, rec["uv"], want=want)
        assert tuple(one) == want
        for k in want:
            assert np.array_equal(bits(one[k]), bits(out[k])), k
    L = ol.load()
    n = rec["t"].size
    assert L.oracle_surface(orc.handle, n, None, rec["t"].ctypes.data, prim.ctypes.data, rec["uv"].ctypes.data, *([None] * 8)) == abi.ERR_BAD_ARG
    assert b"no output" in L.oracle_last_error()
    buf = np.zeros((n, 3), np.float32)
    assert L.oracle_surface(orc.handle, n, None, rec["t"].ctypes.data, prim.ctypes.data, rec["uv"].ctypes.data, None, buf.ctypes.data, *([None] * 6)) == abi.ERR_BAD_ARG
    assert b"rays" in L.oracle_last_error()
    assert L.oracle_surface(orc.handle, n, None, None, prim.ctypes.data, rec["uv"].ctypes.data, *([buf.ctypes.data] + [None] * 7)) == abi.ERR_BAD_ARG
    assert orc.surface(rec["rays"][:0], rec["t"][:0], prim[:0], rec["uv"][:0])["color"].shape == (0, 4)


# ---- the image rules of RaycaImage (include/rayca_hip.h) -------------------------------------------------------------------
def bad_images():
    """(name, edit of a fresh zoo descriptor, words the refusal names)"""
    def color_type(d):
        d._images[1].color_type = 3

    def short_bytes(d):        # the last image ends one byte beyond image_byte_count
        d.c.image_byte_count -= 1

    def offset_beyond(d):      # an image no texture refers to is checked all the same
        d._images[1].byte_offset = d.c.image_byte_count

    def overflow(d):           # 2^32 - 1 squared texels of 16 bytes: beyond 64 bits as a product
        d._images[3].width = d._images[3].height = 0xFFFFFFFF

    def offset_overflow(d):
        d._images[2].byte_offset = 2 ** 64 - 8

    def unaligned_floats(d):   # what packing back to back gave the image behind 45 bytes of RGB8
        d._images[5].byte_offset = 577

    return [("color_type", color_type, ("image 1", "color_type")), ("short", short_bytes, ("image 5", "image_byte_count")),
            ("offset", offset_beyond, ("image 1", "image_byte_count")), ("overflow", overflow, ("image 3", "image_byte_count")),
            ("offset_overflow", offset_overflow, ("image 2", "image_byte_count")), ("unaligned", unaligned_floats, ("image 5", "multiple of 4"))]


def compare(lib, a, b):
    action = C.c_uint32(99)
    return lib.rayca_hip_scene_desc_compare(a.ptr(), 1, b.ptr(), 1, C.byref(action)), action.value


@pytest.mark.parametrize("case", bad_images(), ids=[c[0] for c in bad_images()])
def test_a_bad_image_is_refused_before_any_device_call(product_lib, case):
    _, edit, words = case
    good, bad = sc.zoo_desc(), sc.zoo_desc()
    assert compare(product_lib, good, bad) == (abi.OK, abi.DRAW_REUSED)
    edit(bad)
    for pair in ((good, bad), (bad, good)):
        assert compare(product_lib, *pair)[0] == abi.ERR_BAD_ARG
        assert all(w in last_error() for w in words), last_error()
    h = C.c_void_p()                           # scene creation refuses it before it looks for a device
    assert product_lib.rayca_hip_scene_create(bad.ptr(), None, None, C.byref(h)) == abi.ERR_BAD_ARG and not h.value
    assert all(w in last_error() for w in words), last_error()
    with pytest.raises(ol.OracleError) as e:   # and the CPU side refuses the same descriptor instead of reading past the bytes
        ol.OracleScene(bad, Config())
    assert e.value.code == abi.ERR_BAD_ARG and words[0] in str(e.value)


def test_images_at_the_very_end_and_of_no_texels_are_accepted(product_lib):
    d = sc.zoo_desc()
    last = d._images[d.c.image_count - 1]
    assert last.byte_offset + last.width * last.height * 16 == d.c.image_byte_count   # the bound is inclusive
    assert compare(product_lib, d, d) == (abi.OK, abi.DRAW_REUSED)
    d._images[1].byte_offset = d.c.image_byte_count     # no texel: nothing to read (the scene build refuses an empty image a texture uses)
    d._images[1].width = 0
    assert compare(product_lib, d, d)[0] == abi.OK
    d._images[3].byte_offset += 4                       # a float image may sit on any word
    d._images[3].height = 1
    assert compare(product_lib, d, d)[0] == abi.OK


def test_flatten_starts_every_image_on_a_word(product_lib):
    def scene(order):
        model = M.Model()
        for w, h, ct in order:
            model.images.push(M.Image(w, h, ct))
        s = M.Scene()
        s.push_model(model)
        s.push_model(M.create_default_model())
        return flatten(s)

    d = scene([(5, 3, abi.COLOR_RGB8), (2, 2, abi.COLOR_RGBA32F), (1, 1, abi.COLOR_RGB8), (1, 1, abi.COLOR_RGBA8), (3, 1, abi.COLOR_RGB8)])
    assert [i.byte_offset for i in d._images[:5]] == [0, 48, 112, 116, 120] and d.image_bytes.size == 129
    assert compare(product_lib, d, d) == (abi.OK, abi.DRAW_REUSED)


def test_the_golden_descriptors_still_load(product_lib):
    descs = []
    for name in ("cornell_quad", "spheres"):
        s = M.Scene()
        sdtf.push_sdtf_from_path(s, os.path.join(G, name + ".sdtf"))
        descs.append(flatten(s))
    s = M.Scene()
    s.push_model(scenes.load_gltf(os.path.join(G, "box.gltf")))
    descs.append(flatten(s))
    expected = np.load(os.path.join(G, "jpeg", "expected.npz"))
    from rayca_amd.gltf import load_gltf
    s = M.Scene()
    s.push_model(load_gltf(os.path.join(G, "jpeg", "quad_jpg.gltf"), image_decoder=lambda raw: expected["base_420_odd"]))
    descs.append(flatten(s))
    assert descs[-1].c.image_count >= 1
    for d in descs:
        assert compare(product_lib, d, d) == (abi.OK, abi.DRAW_REUSED), last_error()
        ol.OracleScene(d, Config()).close()
