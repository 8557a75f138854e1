"""rayca_hip_surface_cdf_device / rayca_hip_surface_sample_device (DeviceScene.surface_cdf, .sample_surface): area-weighted
points on the scene's triangles, in device memory.

Every comparison with tests/sample_literal.py is bit-exact: the table word for word, prim directly, uv, point and normal by
their bits.  The triangles the literal reads are the oracle's world-space triangles permuted by DeviceScene.primitive_order(),
as tests/test_gpu_nearest.py reads them.  Each scene is sampled under both builders: their slots differ, the weight of a
triangle does not.  tests/golden/cornell_quad.sdtf holds a ball, and a scene with spheres is refused: the Cornell room here is
that file without its `sphere` line (its quad light, whose two triangles are slots, is what it is sampled for), and the file as
it stands is one of the scenes the refusal is shown on."""
import os
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
import sample_cases as sc
import sample_literal as sl
from rayca_amd import Config, DeviceScene, abi, flatten, scenes
from rayca_amd import model as M
from rayca_amd import sdtf
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["box", "cornell_quad", "soup", "degenerate"]
BUILDERS = {"reference": abi.BUILDER_REFERENCE, "sah": abi.BUILDER_SAH}
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, (1 << 16) + 1]
ALL = ("prim", "uv", "point", "normal")
WIDTH = {"prim": 0, "uv": 2, "point": 3, "normal": 3}
SEED = 7


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_desc(name):
    if name == "box":
        return flatten(scenes.box_scene())
    if name == "soup":
        return flatten(sc.mesh_scene(sc.soup_triangles()))
    if name == "degenerate":
        return flatten(sc.mesh_scene(sc.degenerate_triangles()[0]))
    scene = M.Scene()
    if name == "cornell_quad":   # without the ball
        text = open(os.path.join(G, "cornell_quad.sdtf")).read().splitlines()
        assert sum(l.split()[:1] == ["sphere"] for l in text) == 1
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "cornell_quad_no_ball.sdtf")
            open(path, "w").write("\n".join(l for l in text if l.split()[:1] != ["sphere"]) + "\n")
            sdtf.push_sdtf_from_path(scene, path)
    else:
        sdtf.push_sdtf_from_path(scene, os.path.join(G, name.replace("_with_ball", "") + ".sdtf"))
    return flatten(scene)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def flat_triangles(name):
    def make():
        desc = make_desc(name)
        orc = ol.OracleScene(desc, Config())
        t = orc.world_triangles(orc.primitive_count).astype(np.float32).reshape(-1, 3, 3)
        orc.close()
        return desc, t
    return cached(("flat", name), make)


def case(gpu, name, how):
    """one scene under one builder, made once and shared (read-only): the handle, its slots' triangles, the literal's table and
    the literal's draws for the largest count (every smaller count is a prefix of them)"""
    def make():
        desc, flat = flat_triangles(name)
        ds = DeviceScene(desc, Config(), builder=BUILDERS[how])
        if how == "sah":
            ds.finish()
        order = ds.primitive_order()
        assert np.array_equal(np.sort(order), np.arange(flat.shape[0]))
        tris = flat[order]
        table = sl.cdf(tris)
        return dict(ds=ds, order=order, tris=tris, table=table, draws=sl.draw(tris, table, COUNTS[-1], seed=SEED))
    return cached(("case", name, how), make)


def host(result):
    import torch
    torch.cuda.synchronize()
    out = {}
    for k, v in result.items():
        if k != "stats":
            a = v.cpu().numpy()
            out[k] = a.view(np.uint32) if a.dtype == np.int32 else a
    return out


def assert_draws(got, want, n, what, first=0):
    """got: a host() dict; want: the literal's (prim, uv, point, normal), rows first .. first + n"""
    for k, name in enumerate(ALL):
        if name in got:
            g, w = got[name], want[k][first:first + n]
            assert g.shape == w.shape, (what, name, g.shape)
            bad = np.flatnonzero((bits(g) != bits(w)).reshape(n, -1).any(axis=1)) if n else np.zeros(0, int)
            assert bad.size == 0, f"{what}: {name} differs in {bad.size} of {n} rows, first at {bad[:5]}: got {g[bad[:3]]}, want {w[bad[:3]]}"


# ---- 1: the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(BUILDERS))
@pytest.mark.parametrize("name", NAMES)
def test_table_word_for_word(gpu, name, how):
    import torch
    c = case(gpu, name, how)
    table, stats = c["ds"].surface_cdf(want_stats=True)
    assert table.dtype == torch.int64 and table.shape == (c["tris"].shape[0] + 1,)
    got = table.cpu().numpy().view(np.uint64)
    want = np.array(c["table"], np.uint64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {want.size} entries differ, first at {bad[:5]}: got {got[bad[:5]]}, want {want[bad[:5]]}"
    assert got[0] == 0 and got[-1] > 0 and int(got[-1]) < 1 << 57
    assert stats["kernel_launches"] == 3 and stats["class_launches"][abi.KERNEL_NAMES.index("other")] == 3
    assert all(stats[k] == 0 for k in stats if k.startswith("rays_"))


@pytest.mark.parametrize("name", NAMES)
def test_weights_do_not_depend_on_the_builder(gpu, name):
    """slots differ between the builders (where the scene has more than a leaf); a triangle's weight, through
    primitive_order(), does not"""
    by_flat = {}
    for how in BUILDERS:
        c = case(gpu, name, how)
        w = np.diff(c["ds"].surface_cdf().cpu().numpy().view(np.uint64))
        by_flat[how] = np.zeros_like(w)
        by_flat[how][c["order"]] = w
    assert np.array_equal(by_flat["reference"], by_flat["sah"])
    if name == "soup":
        assert not np.array_equal(case(gpu, name, "reference")["order"], case(gpu, name, "sah")["order"])
    if name == "degenerate":
        assert np.array_equal(by_flat["sah"] > 0, sc.degenerate_triangles()[1])


# ---- 2: the draws ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(BUILDERS))
@pytest.mark.parametrize("name", NAMES)
def test_draws_bit_for_bit(gpu, name, how):
    import torch
    c = case(gpu, name, how)
    for n in COUNTS:
        r = c["ds"].sample_surface(n, seed=SEED, want_stats=True)
        assert r["prim"].dtype == torch.int32 and r["uv"].shape == (n, 2) and r["point"].shape == (n, 3) and r["normal"].shape == (n, 3)
        assert r["stats"]["kernel_launches"] == (1 if n else 0) and all(r["stats"][k] == 0 for k in r["stats"] if k.startswith("rays_"))
        assert_draws(host(r), c["draws"], n, f"{name} {how} count {n}")
    prim = c["draws"][0]
    w = np.diff(np.array(c["table"], dtype=object))
    assert (w[prim] > 0).all()                       # a slot of weight 0 is never drawn
    if name == "soup":
        assert np.unique(prim).size > 1000
    if name == "cornell_quad":                       # every slot with an area is drawn, the quad light's two triangles among them
        assert np.unique(prim).size == np.count_nonzero(w)


def test_every_output_subset_with_guards(gpu):
    """each of the 15 subsets writes what the full call writes, and nothing in front of or behind its rows"""
    import torch
    c = case(gpu, "soup", "sah")
    n, guard = 257, 64
    dtype = {"prim": torch.int32, "uv": torch.float32, "point": torch.float32, "normal": torch.float32}
    for mask in range(1, 16):
        want = tuple(name for k, name in enumerate(ALL) if mask >> k & 1)
        buf = {name: torch.full((n + 2 * guard, WIDTH[name]) if WIDTH[name] else (n + 2 * guard,), -77, dtype=dtype[name], device="cuda") for name in want}
        r = c["ds"].sample_surface(n, seed=SEED, want=want, out={name: buf[name][guard:guard + n] for name in want})
        assert set(r) == set(want) and all(r[name].data_ptr() == buf[name][guard:].data_ptr() for name in want)
        assert_draws(host(r), c["draws"], n, f"subset {want}")
        for name in want:
            b = buf[name].cpu().numpy()
            assert (b[:guard] == -77).all() and (b[guard + n:] == -77).all(), (want, name)


def test_chunks_against_one_call(gpu):
    c = case(gpu, "soup", "reference")
    first = 0
    for n in (1, 63, 64, 129, 1000):
        r = c["ds"].sample_surface(n, seed=SEED, first_index=first)
        assert_draws(host(r), c["draws"], n, f"chunk at {first}", first=first)
        first += n
    # the index wraps at 2^32: samples 4 .. 7 of a call that starts at 2^32 - 4 are samples 0 .. 3
    r = host(c["ds"].sample_surface(8, seed=SEED, first_index=0xFFFFFFFC))
    assert_draws({k: v[4:] for k, v in r.items()}, c["draws"], 4, "wrap")
    # another stream of the same seed is another set of samples
    other = host(c["ds"].sample_surface(1000, seed=SEED, sample=1))
    want = sl.draw(c["tris"], c["table"], 1000, seed=SEED, sample=1)
    assert_draws(other, want, 1000, "sample 1")
    assert not np.array_equal(other["prim"], c["draws"][0][:1000])


def test_another_stream_and_another_context(gpu):
    import torch
    c = case(gpu, "cornell_quad", "sah")
    n = 4097
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        table = c["ds"].surface_cdf(stream=stream, context=3)
        r = c["ds"].sample_surface(n, cdf=table, seed=SEED, stream=stream, context=3)
    stream.synchronize()
    assert np.array_equal(table.cpu().numpy().view(np.uint64), np.array(c["table"], np.uint64))
    assert_draws(host(r), c["draws"], n, "stream, context 3")
    r = c["ds"].sample_surface(n, seed=SEED, context=5)   # the kept table of all slots, on torch's current stream
    assert_draws(host(r), c["draws"], n, "context 5")


# ---- 3: masks ----------------------------------------------------------------------------------------------------------------
def slot_materials(ds, slots):
    import torch
    prim = torch.arange(slots, dtype=torch.int32, device="cuda")
    zeros = torch.zeros(slots, device="cuda")
    return ds.surface(None, zeros, prim, torch.zeros((slots, 2), device="cuda"), want=("material",))["material"]


@pytest.mark.parametrize("how", list(BUILDERS))
def test_include_by_material(gpu, how):
    """a mask taken from surface(..., want=("material",)): the table is the literal's for that mask and every drawn slot has
    that material; an all-zero mask gives misses"""
    import torch
    c = case(gpu, "cornell_quad", how)
    ds, slots = c["ds"], c["tris"].shape[0]
    material = slot_materials(ds, slots)
    ids, counts = torch.unique(material, return_counts=True)
    assert ids.numel() >= 2
    pick = int(ids[torch.argmin(counts)])
    include = material == pick                      # (bool: one byte an element)
    table = ds.surface_cdf(include)
    want_table = sl.cdf(c["tris"], include.cpu().numpy())
    assert np.array_equal(table.cpu().numpy().view(np.uint64), np.array(want_table, np.uint64))
    n = 4099
    r = ds.sample_surface(n, cdf=table, seed=3)
    assert (material[r["prim"].long()] == pick).all()
    assert_draws(host(r), sl.draw(c["tris"], want_table, n, seed=3), n, f"material {pick}")
    empty = ds.surface_cdf(torch.zeros(slots, dtype=torch.uint8, device="cuda"))
    assert not empty.any()
    miss = host(ds.sample_surface(300, cdf=empty, seed=3))
    assert (miss["prim"] == sl.NONE).all() and not any(bits(miss[k]).any() for k in ("uv", "point", "normal"))


# ---- 4: into the other queries -----------------------------------------------------------------------------------------------
def test_prim_and_uv_go_to_surface_as_they_are(gpu):
    import torch
    c = case(gpu, "cornell_quad", "sah")
    ds, slots = c["ds"], c["tris"].shape[0]
    n = 5000
    r = ds.sample_surface(n, seed=SEED, want=("prim", "uv"))
    g = ds.surface(None, torch.zeros(n, device="cuda"), r["prim"], r["uv"], want=("color", "material", "flags"))
    torch.cuda.synchronize()
    flags = g["flags"].cpu().numpy().view(np.uint32)
    assert (flags & abi.SURFACE_HIT != 0).all() and (flags & abi.SURFACE_SPHERE == 0).all()
    assert torch.equal(g["material"], slot_materials(ds, slots)[r["prim"].long()])
    assert torch.isfinite(g["color"]).all() and (flags & abi.SURFACE_EMISSIVE != 0).any()   # the lamp's two triangles are drawn too


@pytest.mark.parametrize("name", ["box", "cornell_quad"])
def test_points_lie_on_the_surface_for_nearest(gpu, name):
    """point -> nearest(): prim may differ (a point on a shared edge is a tie, and a neighbour may be nearer by rounding);
    dist2 is bounded.  With u = 2^-24 and M the largest coordinate magnitude of the scene: the sample is (a + ab*s) + ac*t in
    f32, the expression nearest() forms q with, so by DESIGN 4.15 it lies within 13 u M per axis of a point of its triangle; so
    does the q that nearest() finds on that triangle.  On these scenes' right triangles (legs no shorter than M / 8) the
    projection's dot products carry at most 29 u M |ab| of error each (the 13 u M of the point, three roundings of a dot
    product), its quotients twice that relative to |ab|^2: under 100 u M along the legs.  13 + 13 + 100 < 128, so the computed
    offset is below 2^-17 M per axis and dist2 <= 3 (2^-17 M)^2 (1 + 4 u).  The winner's dist2 is no larger than that of the
    sample's own triangle."""
    c = case(gpu, name, "sah")
    n = 1 << 14
    r = c["ds"].sample_surface(n, seed=SEED, want=("prim", "point"))
    d2, prim, q, _ = c["ds"].nearest(r["point"])
    d2, prim, own = d2.cpu().numpy(), prim.cpu().numpy().view(np.uint32), r["prim"].cpu().numpy().view(np.uint32)
    m = float(np.abs(c["tris"]).max())
    bound = 3.0 * (2.0 ** -17 * m) ** 2 * (1 + 2.0 ** -22)
    print(f"{name}: M = {m}, largest dist2 = {d2.max():.3e} (bound {bound:.3e}), {np.count_nonzero(prim != own)} of {n} points nearer to another slot")
    assert (prim != sl.NONE).all()
    assert d2.max() <= bound


def test_a_scene_with_spheres_is_refused_and_the_next_call_works(gpu):
    import torch
    for name in ("spheres", "cornell_quad_with_ball"):
        ds = DeviceScene(make_desc(name), Config(), builder=abi.BUILDER_SAH)
        assert ds.info()["sphere_count"] > 0
        slots = ds.info()["triangle_count"] + ds.info()["sphere_count"]
        with pytest.raises(RaycaError) as e:
            ds.surface_cdf()
        assert e.value.code == abi.ERR_UNSUPPORTED and "spheres" in str(e.value)
        with pytest.raises(RaycaError) as e:
            ds.sample_surface(16, cdf=torch.zeros(slots + 1, dtype=torch.int64, device="cuda"))
        assert e.value.code == abi.ERR_UNSUPPORTED and "spheres" in str(e.value)
        with pytest.raises(RaycaError) as e:
            ds.sample_surface(16)                      # (the table of all slots cannot be made either)
        assert e.value.code == abi.ERR_UNSUPPORTED
        ds.close()
    c = case(gpu, "box", "reference")
    assert_draws(host(c["ds"].sample_surface(65, seed=SEED)), c["draws"], 65, "box after the refusal")
