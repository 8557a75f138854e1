"""The material zoo: one small scene that reaches every branch of a surface record (shade_hit in trace_core.inc, HitInfo in the
oracle), and the hit records the CPU and GPU tests evaluate on it.  Everything is a deterministic function of a seed; nothing
is read from a file.

The scene: smooth-shaded 2 x 2 patches (eight triangles each) whose vertex normals, tangents and bitangents differ across
every triangle and are not unit length, whose vertex colours differ in all four channels and whose UVs run from -2.5 to 3 with
exact integers among them; one patch per material (PBR with every combination of textures the paths distinguish, the default
material, Phong, GGX, an emissive Phong), a sphere whose material carries a normal texture, and a second model with images of
its own.  Every mesh node has a rotation and a non-uniform scale and hangs under a model root with its own TRS.

The records name primitives in FLATTEN order (`flat`); `slots()` maps them to a scene's post-build order."""
import numpy as np

from flatten_order import flat_table
from rayca_amd import (Config, GgxMaterial, Image, IntegratorStrategy, Mesh, Model, Node, PbrMaterial, PhongMaterial, Primitive,
                       Scene, Sphere, Texture, TriangleMesh, Trs, abi, create_default_model, flatten)
from rayca_amd.model import quat_axis_angle

SEED = 20240607
NONE = np.uint32(0xFFFFFFFF)
FLT_MAX = np.float32(3.4028234663852886e38)
W, H = 64, 48
FLAT = Config(integrator=IntegratorStrategy.Flat, samples_per_pixel=1, gamma=1.0)
GRID = 2                      # a patch is GRID x GRID cells, two triangles each
TEXEL_BYTES = {abi.COLOR_RGB8: 3, abi.COLOR_RGBA8: 4, abi.COLOR_RGBA32F: 16}


def _patch(rs, index_dtype):
    """a GRID x GRID patch over [-0.5, 0.5]^2, counter-clockwise seen from +z, every attribute varying from vertex to vertex"""
    n = GRID + 1
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, n), np.linspace(-0.5, 0.5, n))
    count = n * n
    pos = np.stack([gx.ravel(), gy.ravel(), rs.uniform(-0.05, 0.05, count)], 1).astype(np.float32)
    # a well-conditioned frame (tangent near +x, bitangent near +y, normal near +z), perturbed and of lengths 0.5 .. 2
    frame = []
    for axis in range(3):
        v = rs.uniform(-0.35, 0.35, (count, 3))
        v[:, axis] = 1.0
        frame.append((v * rs.uniform(0.5, 2.0, (count, 1))).astype(np.float32))
    colors = rs.uniform(0.2, 1.0, (count, 4)).astype(np.float32)
    uvs = rs.uniform(-2.5, 3.0, (count, 2)).astype(np.float32)
    uvs[0], uvs[4], uvs[8] = (-1.0, 2.0), (0.0, 1.0), (1.0, -2.0)   # exact integers: the wrap's own boundary
    # one ulp below a texel boundary, which a corner record reproduces exactly: the fraction + 1.0f rounds up to the boundary and the
    # texel is the next one -- the only place where the `+ 1.0f` of Sampler::sample shows
    uvs[2], uvs[6] = (1.0 - 2.0 ** -24, 0.5 - 2.0 ** -25), (-2.0 + 0.25 - 2.0 ** -24, 2.0 - 2.0 ** -23)
    idx = []
    for j in range(GRID):
        for i in range(GRID):
            a = j * n + i
            idx += [a, a + 1, a + n + 1, a, a + n + 1, a + n]
    return TriangleMesh(pos, np.array(idx, index_dtype), colors=colors, normals=frame[2], tangents=frame[0], bitangents=frame[1], uvs=uvs)


def _images(rs, second):
    """(width, height, colour type, data) in the order the model holds them: the sizes make every later offset non-trivial"""
    def rgb8(w, h, lo=0, hi=256):
        return Image(w, h, abi.COLOR_RGB8, rs.randint(lo, hi, (h, w, 3)).astype(np.uint8))

    def f32(w, h):
        data = rs.uniform(0.0, 255.0, (h, w, 4))          # fractional throughout,
        data.reshape(-1)[::5] = rs.uniform(-64.0, 0.0, data.reshape(-1)[::5].shape)      # a fifth of the words below 0
        data.reshape(-1)[2::7] = rs.uniform(255.0, 320.0, data.reshape(-1)[2::7].shape)  # and a seventh above 255
        return Image(w, h, abi.COLOR_RGBA32F, data.astype(np.float32))

    if second:   # 45 bytes of RGB8 in front of floats: the float image needs the padding flatten() gives it
        return [rgb8(3, 5, 26, 231), f32(3, 2)]
    return [rgb8(5, 3, 26, 231),                                                       # (26 .. 230: roughness 0.1 .. 0.9 as a metallic-roughness map)
            Image(1, 1, abi.COLOR_RGBA8, np.array([[[200, 90, 30, 180]]], np.uint8)),
            Image(8, 8, abi.COLOR_RGBA8, rs.randint(0, 256, (8, 8, 4)).astype(np.uint8)),   # alpha anywhere in 0 .. 255
            f32(7, 2)]


def zoo_scene(seed=SEED):
    rs = np.random.RandomState(seed)
    zoo, second = Model("zoo"), Model("second")
    for im in _images(rs, False):
        zoo.textures.push(Texture(image=zoo.images.push(im)))
    RGB8, ONE, RGBA8, F32 = 0, 1, 2, 3   # texture handles of the zoo = its image handles
    mats = [PbrMaterial(color=(0.9, 0.8, 0.7, 1.0), albedo=RGB8, roughness_factor=0.8),
            PbrMaterial(color=(0.8, 0.9, 0.6, 1.0), albedo=F32, normal=RGBA8, metallic_factor=0.3, roughness_factor=0.6),
            PbrMaterial(color=(0.7, 0.6, 0.9, 0.75), albedo=RGBA8, normal=F32, metallic_roughness=RGB8),
            PbrMaterial(color=(0.6, 0.7, 0.8, 1.0), normal=RGBA8, metallic_factor=0.7, roughness_factor=0.4),
            PbrMaterial(color=(0.5, 0.9, 0.7, 1.0), metallic_factor=0.2, roughness_factor=0.9),
            None,                                                                  # Material::DEFAULT
            PhongMaterial(ambient=(0.1, 0.2, 0.15, 1.0), diffuse=(0.6, 0.5, 0.4, 1.0), specular=(0.3, 0.2, 0.1, 1.0), shininess=12.0),
            GgxMaterial(diffuse=(0.4, 0.6, 0.5, 0.9), specular=(0.2, 0.3, 0.4, 1.0), roughness=0.45),
            PhongMaterial(ambient=(0.05, 0.05, 0.1, 1.0), emission=(0.8, 0.7, 0.3, 1.0), diffuse=(0.3, 0.3, 0.3, 1.0), specular=(0.1, 0.1, 0.1, 1.0),
                          shininess=300.0),
            PbrMaterial(color=(0.9, 0.9, 0.9, 1.0), albedo=ONE, metallic_roughness=RGBA8)]
    cells = [(-1.6 + 0.8 * (k % 5), 0.85 - 0.85 * (k // 5), 0.0) for k in range(15)]

    def place(model, geometry, material, cell, k, scale=None):
        axis = np.array([0.3 * np.sin(k), 0.3 * np.cos(2.0 * k), 1.0])
        trs = Trs(translation=cell, rotation=quat_axis_angle(axis / np.linalg.norm(axis), 0.25 + 0.11 * k),
                  scale=scale or (0.62 + 0.01 * k, 0.55 - 0.01 * k, 0.8 + 0.03 * k))
        p = model.primitives.push(Primitive(geometry=model.geometries.push(geometry), material=material))
        model.root.children.append(model.nodes.push(Node(mesh=model.meshes.push(Mesh(primitives=[p])), trs=trs)))

    for k, m in enumerate(mats):
        place(zoo, _patch(rs, (np.uint8, np.uint16, np.uint32)[k % 3]), None if m is None else zoo.materials.push(m), cells[k], k)
    ball = zoo.materials.push(PbrMaterial(color=(0.9, 0.5, 0.4, 1.0), normal=ONE, metallic_factor=0.5, roughness_factor=0.3))
    # Every world scale of the sphere is above 1.  Sphere::intersects keeps the inverse-transformed ray in its Hit, so the view vector
    # of a sphere is the world direction divided by the scale; longer than 1 it drives n . v past 1 and acos() to NaN in the
    # reference's GGX terms, and a frame with NaN pixels cannot be compared at a tolerance.  Integral Phong shininess above for the
    # same reason: powf(negative, 12.5) is NaN.
    place(zoo, Sphere(center=(0.1, -0.05, 0.0), radius=0.2), ball, cells[len(mats)], len(mats), scale=(1.6, 1.3, 1.9))
    zoo.root.trs = Trs(translation=(0.05, -0.03, 0.1), rotation=quat_axis_angle((0.0, 0.0, 1.0), 0.1), scale=(1.1, 0.9, 1.05))
    for im in _images(rs, True):
        second.textures.push(Texture(image=second.images.push(im)))
    both = second.materials.push(PbrMaterial(color=(0.8, 0.8, 0.9, 1.0), albedo=1, normal=0, metallic_roughness=0))
    place(second, _patch(rs, np.uint16), both, cells[len(mats) + 1], len(mats) + 1)
    second.root.trs = Trs(translation=(-0.02, 0.04, -0.1), rotation=quat_axis_angle((0.0, 1.0, 0.0), -0.15), scale=(0.95, 1.05, 1.0))
    scene = Scene()
    scene.push_model(zoo)
    scene.push_model(second)
    scene.push_model(create_default_model())
    return scene


def zoo_desc(seed=SEED):
    return flatten(zoo_scene(seed))


def corner_vertices(desc, table):
    """(flat, 3) descriptor vertex numbers of every flattened triangle; -1 for a sphere and a quad light's triangles"""
    out = np.full((table.shape[0], 3), -1, np.int64)
    for f, (_, pi, tri, _, sphere) in enumerate(table):
        if pi < 0 or sphere:
            continue
        p = desc._prims[pi]
        width = {abi.INDEX_U8: 1, abi.INDEX_U16: 2, abi.INDEX_U32: 4}[p.index_type]
        raw = desc.index_bytes[p.index_byte_offset + 3 * tri * width: p.index_byte_offset + 3 * (tri + 1) * width]
        out[f] = raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[width]).astype(np.int64) + p.first_vertex
    return out


def lattice(rs):
    """barycentric (u, v) of the records of one triangle: the 1/8 lattice over [-1/4, 5/4]^2 -- corners, edge midpoints, (0, 0),
    interior points, points outside the triangle on every side -- some random interior points, and one record with u = 3e38"""
    k = np.arange(-2, 11, dtype=np.float32) / np.float32(8.0)
    u, v = (a.ravel() for a in np.meshgrid(k, k))
    inside = rs.dirichlet((1.0, 1.0, 1.0), 50).astype(np.float32)[:, :2]
    return np.concatenate([np.stack([u, v], 1), inside, np.array([[3e38, 0.25]], np.float32)]).astype(np.float32)


def records(desc, orc, seed=SEED):
    """dict of rays (n, 6), t, flat (flatten-order primitive; NONE, the primitive count or 0xFFFFFFFE for the non-hits), uv (n, 2),
    what (0 lattice, 1 sphere ray, 2 non-hit).  `orc` is an OracleScene of `desc`: the sphere's records are real hits of rays
    aimed at it (and of those that miss it)."""
    rs = np.random.RandomState(seed + 1)
    table = flat_table(desc)
    tri = np.flatnonzero(table[:, 4] == 0)
    per = lattice(rs)
    flat = np.repeat(tri, per.shape[0]).astype(np.uint32)
    uv = np.tile(per, (tri.size, 1))
    n = flat.size
    d = rs.normal(size=(n, 3))
    rays = np.concatenate([rs.uniform(-1.0, 1.0, (n, 3)), d / np.linalg.norm(d, axis=1)[:, None]], 1).astype(np.float32)
    t = rs.uniform(0.1, 5.0, n).astype(np.float32)
    what = np.zeros(n, np.int64)
    # the sphere: rays from around the camera through a disc around its world centre
    sphere = int(np.flatnonzero(table[:, 4] == 1)[0])
    order = orc.primitive_order()
    m = 600
    eye = np.array([0.0, 0.0, 4.0]) + rs.uniform(-0.3, 0.3, (m, 3))
    target = np.array(_sphere_world_centre(desc, table[sphere])) + rs.uniform(-0.45, 0.45, (m, 3)) * np.array([1.0, 1.0, 0.0])
    sd = target - eye
    srays = np.concatenate([eye, sd / np.linalg.norm(sd, axis=1)[:, None]], 1).astype(np.float32)
    st, sprim, suv, _ = orc.trace_rays(srays)
    sflat = np.where(sprim == NONE, NONE, order[np.minimum(sprim, order.size - 1)]).astype(np.uint32)
    # the three kinds of non-hit: the primitive count, an arbitrary large index, the query's own miss record
    k = 96
    pick = rs.randint(0, n, k)
    nflat = np.array([order.size, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)[np.arange(k) % 3]
    nt, nuv = t[pick].copy(), uv[pick].copy()
    nt[nflat == NONE], nuv[nflat == NONE] = FLT_MAX, 0.0
    return dict(rays=np.concatenate([rays, srays, rays[pick]]), t=np.concatenate([t, st, nt]), flat=np.concatenate([flat, sflat, nflat]),
                uv=np.concatenate([uv, suv, nuv]), what=np.concatenate([what, np.full(m, 1), np.full(k, 2)]), prim_count=order.size)


def _sphere_world_centre(desc, row):
    from flatten_order import rotate, world_trs
    t, q, s = world_trs(desc)[row[0]]
    return t + rotate(s * np.array(list(desc._prims[row[1]].sphere_center), np.float64), q)


def slots(rec, order):
    """the records' primitives in a scene's post-build order (`order`: slot -> flatten index); non-hits stay what they are"""
    slot_of = np.empty(order.size, np.uint32)
    slot_of[order] = np.arange(order.size, dtype=np.uint32)
    flat = rec["flat"]
    hit = flat < order.size
    return np.where(hit, slot_of[np.minimum(flat, order.size - 1)], flat).astype(np.uint32)


def interpolate(attr, corners, uv):
    """(a2 * (1 - u - v) + a0 * u) + a1 * v in float32, operation for operation as both sides spell it (bvh/triangle.rs:33-77)"""
    u, v = uv[:, :1], uv[:, 1:]
    w2 = np.float32(1.0) - u - v
    with np.errstate(all="ignore"):
        return (attr[corners[:, 2]] * w2 + attr[corners[:, 0]] * u) + attr[corners[:, 1]] * v


def wrap(u, size):
    """Sampler::sample's texel coordinate (sampler.rs:11-30): ((u - floor(u) + 1) * size) as u32 (saturating, NaN -> 0) % size"""
    with np.errstate(all="ignore"):
        x = (u - np.floor(u) + np.float32(1.0)) * np.float32(size)
    x = np.where(np.isnan(x) | (x <= 0), 0.0, np.minimum(x.astype(np.float64), 4294967295.0))
    return np.floor(x).astype(np.uint64) % np.uint64(size)


def texel(desc, texture, uv):
    """(n, 4) float64 RGBA words of the texels `uv` (float32, n x 2) addresses in a texture, before the division by 255, and the
    byte address of each; straight from image_bytes"""
    im = desc._images[desc._textures[texture].image]
    x, y = wrap(uv[:, 0], im.width), wrap(uv[:, 1], im.height)
    size = TEXEL_BYTES[im.color_type]
    address = im.byte_offset + (y * np.uint64(im.width) + x) * np.uint64(size)
    out = np.empty((uv.shape[0], 4), np.float64)
    for i, a in enumerate(address.astype(np.int64)):
        raw = desc.image_bytes[a:a + size]
        out[i] = raw.view(np.float32) if im.color_type == abi.COLOR_RGBA32F else (list(raw) + [255])[:4]
    return out, address


ROLES = ("albedo_texture", "normal_texture", "metallic_roughness_texture")


def branch_counts(desc, rec):
    """how many records reach each branch of a surface record, from the descriptor alone"""
    table = flat_table(desc)
    corners = corner_vertices(desc, table)
    flat = rec["flat"]
    hit = np.flatnonzero(flat < table.shape[0])
    row = table[flat[hit]]
    sphere = row[:, 4] == 1
    mat = row[:, 3].astype(np.uint32)
    default = (mat == NONE) | (mat >= desc.c.material_count)
    kind = np.array([abi.MATERIAL_PBR if d else desc._materials[m].kind for m, d in zip(mat, default)])
    uv = np.where(sphere[:, None], np.float32(0.0), interpolate(desc.uvs, np.maximum(corners[flat[hit]], 0), rec["uv"][hit]))
    c = {"records": flat.size, "triangle": int((~sphere).sum()), "sphere": int(sphere.sum()), "default_material": int(default.sum()),
         "non_hit_prim_count": int((flat == table.shape[0]).sum()), "non_hit_large": int((flat == 0xFFFFFFFE).sum()), "non_hit_none": int((flat == NONE).sum()),
         "pbr": int((kind == abi.MATERIAL_PBR).sum()), "phong": int((kind == abi.MATERIAL_PHONG).sum()), "ggx": int((kind == abi.MATERIAL_GGX).sum()),
         "uv_not_finite": int((~np.isfinite(uv)).any(1).sum()), "emissive": 0, "sphere_with_normal_texture": 0}
    c.update({k: 0 for k in ("rgb8", "rgba8", "rgba32f", "image_beyond_first", "image_of_second_model", "alpha_below_255_in_normal_map",
                             "wrap_x_below_0", "wrap_x_above_1", "wrap_y_below_0", "wrap_y_above_1", "uv_exact_integer", "wrap_plus_one_rounds_up") + ROLES})
    eps = np.finfo(np.float32).eps
    model = np.array([desc._nodes[n].model for n in row[:, 0]])
    for m in np.unique(mat[~default]):
        mm = desc._materials[m]
        sel = mat == m
        e = np.array(list(mm.emission), np.float32)
        if mm.kind == abi.MATERIAL_PHONG and not (np.abs(e - np.array([0, 0, 0, 1], np.float32)) < eps).all():
            c["emissive"] += int(sel.sum())
        if mm.kind != abi.MATERIAL_PBR:
            continue
        if mm.normal_texture != abi.NONE:
            c["sphere_with_normal_texture"] += int((sel & sphere).sum())
        for role in ROLES:
            tex = getattr(mm, role)
            s = sel & ~sphere if role == "normal_texture" else sel   # (the sphere path has no normal map)
            if tex == abi.NONE or not s.any():
                continue
            im = desc._images[desc._textures[tex].image]
            c[role] += int(s.sum())
            c[("rgb8", "rgba8", "rgba32f")[im.color_type]] += int(s.sum())
            c["image_beyond_first"] += int(s.sum()) if im.byte_offset else 0
            c["image_of_second_model"] += int((s & (model != model.min())).sum())
            with np.errstate(invalid="ignore"):
                if im.width > 1:
                    c["wrap_x_below_0"] += int((uv[s, 0] < 0).sum())
                    c["wrap_x_above_1"] += int((uv[s, 0] >= 1).sum())
                if im.height > 1:
                    c["wrap_y_below_0"] += int((uv[s, 1] < 0).sum())
                    c["wrap_y_above_1"] += int((uv[s, 1] >= 1).sum())
                c["uv_exact_integer"] += int(((uv[s] == np.floor(uv[s])).any(1)).sum())
                for axis, size in ((0, im.width), (1, im.height)):
                    frac = uv[s, axis] - np.floor(uv[s, axis])
                    c["wrap_plus_one_rounds_up"] += int((wrap(uv[s, axis], size) != np.floor(frac * np.float32(size)).astype(np.uint64) % np.uint64(size))[np.isfinite(frac)].sum())
            if role == "normal_texture" and im.color_type != abi.COLOR_RGB8:
                c["alpha_below_255_in_normal_map"] += int((texel(desc, tex, uv[s])[0][:, 3] < 255).sum())
    return c
