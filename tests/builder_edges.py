"""Edge-case geometry for the BLAS builders (helper module; test_builder_edges_cpu.py, test_gpu_builder_edges.py).

The uniform soups and the atrium of test_gpu_parity.py never reach most of the device builder's special cases: the size
thresholds, one-sided partitions of nodes that many workgroups partition, exact cost ties, inseparable sets above the
multi-workgroup threshold, children of awkward sizes, deep skewed trees, a zero-extent axis, denormal costs.  Each family
here is built to reach some of them; test_builder_edges_cpu.py asserts from the literal builder's tree (bvh_literal.py) that
it does.  Every scene is one model without textures and a camera outside it, a deterministic function of its name; oracle
scenes, literal trees, ray batches and oracle records are made once per process and shared by the tests."""
import math

import numpy as np

import bvh_literal
import oracle_lib as ol
from rayca_amd import Config, IntegratorStrategy, PbrMaterial, TriangleMesh, Trs, flatten, scenes

# The builder's constants, written down here on purpose (nothing is imported from the library):
K_DEVICE_BUILD_MIN = 4096   # host_scene.cpp kDeviceBuildMin: BLASes below it are built on the host
K_BIG = 16384               # bvh_build.hip kBig (RAYCA_KBIG): nodes above it are binned and partitioned by many workgroups
K_CHUNK = 4096              # bvh_build.hip kChunk: positions per workgroup of a big node
K_SEQ = 16                  # bvh_build.hip kSeq: subtrees of at most this many primitives are left to k_build_small
K_LEVEL_BATCH = 8           # bvh_build.hip kLevelBatch: levels queued between two read-backs of the level records

NONE = np.uint32(0xFFFFFFFF)
FLAT = Config(integrator=IntegratorStrategy.Flat)
FRAME = (64, 48)
N_RAYS = 2000
SIZES = [K_DEVICE_BUILD_MIN - 1, K_DEVICE_BUILD_MIN, K_DEVICE_BUILD_MIN + 1, K_BIG, K_BIG + 1, 5 * K_CHUNK, 5 * K_CHUNK + 1]
SMALL_K = [1, 2, K_SEQ, K_SEQ + 1]
FULLBOX_N = [20000, 40000]
DENORMAL_SCALE = 2.0 ** -68

FAMILIES = {
    "sizes": [f"sizes{n}" for n in SIZES],
    "split_kbig": ["split_kbig"],
    "split_small": [f"split_small{k}" for k in SMALL_K],
    "fullbox": [f"fullbox{n}" for n in FULLBOX_N],
    "duplicates": ["duplicates"],
    "flat_grid": ["flat_grid"],
    "denormal": ["denormal"],
}
SCENES = [s for names in FAMILIES.values() for s in names]


def family_of(name):
    return next(f for f, names in FAMILIES.items() if name in names)


def _unit(seed, shape):
    return scenes.hash_unit(seed, np.arange(int(np.prod(shape)), dtype=np.uint32)).reshape(shape)


def _soup(n, seed, extent, centre=(0.0, 0.0, 0.0), half=1.0):
    """[n, 3, 3] f32: triangle centres uniform in centre +- half, corners within +-extent of them"""
    f = np.float32
    c = (_unit(seed, (n, 1, 3)) * f(2) - f(1)) * f(half) + np.asarray(centre, f)
    return (c + (_unit(seed + 1, (n, 3, 3)) * f(2) - f(1)) * f(extent)).astype(f)


def _scene(tri, camera=(0.0, 0.0, 3.5)):
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 3)
    rgb = np.repeat(_unit(0xC0105, (tri.shape[0] // 3, 3)) * np.float32(0.8) + np.float32(0.2), 3, axis=0)
    col = np.concatenate([rgb, np.ones((tri.shape[0], 1), np.float32)], 1)
    tm = TriangleMesh(tri, np.arange(tri.shape[0], dtype=np.uint32), colors=col)
    return scenes._single_model_scene([(tm, PbrMaterial(color=(1, 1, 1, 1), roughness_factor=1.0))], Trs(translation=tuple(camera)),
                                      math.pi / 4)


def build_scene(name):
    fam = family_of(name)
    if fam == "sizes":
        return scenes.soup_scene(int(name[5:]), extent=0.03)
    if fam == "split_kbig":
        # two soups far apart on x; the y and z extents are those of one soup, so that no y or z plane separates anything
        return _scene(np.concatenate([_soup(K_BIG, 0x51DE0, 0.02, (-3.0, 0.0, 0.0)), _soup(K_BIG + 1, 0x51DE2, 0.02, (3.0, 0.0, 0.0))]),
                      camera=(0.0, 0.0, 9.0))
    if fam == "split_small":
        k = int(name[11:])
        return _scene(np.concatenate([_soup(5000, 0x5A110, 0.03), _soup(k, 0x5A112, 0.03, (40.0, 0.0, 0.0), 0.05)]))
    if fam == "fullbox":
        n = int(name[7:])
        tri = np.empty((n, 3, 3), np.float32)
        tri[:, 0], tri[:, 1], tri[:, 2] = -1.0, 1.0, _unit(0xF0B0, (n, 3)) * np.float32(2) - np.float32(1)
        return _scene(tri)
    if fam == "duplicates":
        one = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.05], [0.0, 0.25, 0.05]], np.float32)
        return _scene(np.concatenate([np.broadcast_to(one, (20000, 3, 3)), _soup(5000, 0xD0B1E, 0.03)]))
    if fam == "flat_grid":
        b = scenes._MeshBuilder()
        b.grid((-1.0, -1.0, 0.0), np.array([2, 0, 0], np.float32), np.array([0, 2, 0], np.float32), 128, 128)
        m = b.mesh()
        return _scene(m.positions[m.indices.astype(np.int64)])
    assert fam == "denormal"
    return _scene((_soup(4200, 0xDE40, 0.03) + np.array([1.5, 1.0, 0.5], np.float32)) * np.float32(DENORMAL_SCALE))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def scene_desc(name):
    return _cached(("desc", name), lambda: flatten(build_scene(name)))


def oracle_scene(name):
    """The reference's tree by the oracle's binned sweep (test_oracle_bvh.py holds it to the literal one); the CPU file
    builds the literal one itself where it compares trees."""
    return _cached(("oracle", name), lambda: ol.OracleScene(scene_desc(name), Config(), build=ol.BUILD_BINNED))


def triangles(name):
    """[n, 3, 3] f32, world space, flatten order (oracle_scene_world_triangles)"""
    return _cached(("tri", name), lambda: oracle_scene(name).world_triangles(oracle_scene(name).primitive_count).reshape(-1, 3, 3))


def literal(name, seed_origin, audit_every=0):
    """bvh_literal.Tree of the scene (the first call of a process decides about the audit)"""
    return _cached(("literal", name, bool(seed_origin)), lambda: bvh_literal.build(triangles(name), bool(seed_origin), audit_every=audit_every))


def rays(name):
    """N_RAYS rays: half from outside the geometry at centroids of primitives picked at random, half with origins uniform
    in the doubled bounding box and uniform directions of the box's size (so the batch scales with the scene)."""
    def make():
        tri = triangles(name).astype(np.float64)
        lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
        centre, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
        rs = np.random.RandomState(0xED6E5 + SCENES.index(name))
        h = N_RAYS // 2
        target = tri[rs.randint(0, tri.shape[0], h)].mean(1)
        d = rs.normal(size=(h, 3))
        o = centre + d / np.linalg.norm(d, axis=1, keepdims=True) * 2.0 * diag
        aimed = np.concatenate([o, target - o], 1)
        o2 = centre + rs.uniform(-1, 1, (N_RAYS - h, 3)) * (hi - lo)
        d2 = rs.uniform(-1, 1, (N_RAYS - h, 3)) * diag
        return np.concatenate([aimed, np.concatenate([o2, d2], 1)]).astype(np.float32)
    return _cached(("rays", name), make)


def oracle_records(name):
    """(t, prim as a flatten index or NONE, uv) of rays(name) in the oracle"""
    def make():
        orc = oracle_scene(name)
        t, prim, uv, _ = orc.trace_rays(rays(name))
        flat = np.array(prim, np.uint32)
        hit = flat != NONE
        flat[hit] = orc.primitive_order()[flat[hit]]
        return t, flat, uv
    return _cached(("records", name), make)


def oracle_frame(name):
    return _cached(("frame", name), lambda: oracle_scene(name).render(FLAT, *FRAME)[1])
