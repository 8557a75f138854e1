"""rayca_hip_radiance_device / DeviceScene.radiance and Film.add(jitter=n): radiance along caller-supplied rays in device memory.

The contract is bit-level: a frame's own camera rays give the frame (either engine, f32 and RGBA8, and its ray counts), chunks
with matching first_index give what one call gives, and Flat depends on the ray alone -- query + surface colour on a hit, a
render's miss pixel on a miss -- whatever the ray (an orthographic grid, a shuffled one, the adversarial families of
ray_edges.py).  Small scenes (test_gpu_general.py's), both builders; a RAYCA_BUILDER_SAH scene before and after finish()."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import ray_edges as re_
import test_gpu_general as G
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, SamplerStrategy, abi, flatten, lib, scenes
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
I, S = IntegratorStrategy, SamplerStrategy
FLAT = Config(integrator=I.Flat)
ONE = Config(samples_per_pixel=1)
COUNTS = ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded")
_DESCS, _SCENES = {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(x):
    return x.cpu().numpy()


def desc_of(name):
    if name not in _DESCS:
        _DESCS[name] = re_.scene_desc(name[6:]) if name.startswith("edges:") else flatten(G.SCENES[name]())
    return _DESCS[name]


def scene(name, how):
    """the module's scenes, one per (scene, builder); SAH scenes are finished (the frame test makes its own unfinished ones)"""
    if (name, how) not in _SCENES:
        ds = DeviceScene(desc_of(name), Config(), builder=abi.BUILDER_SAH if how == "sah" else abi.BUILDER_REFERENCE)
        if how == "sah":
            ds.finish()
        _SCENES[(name, how)] = ds
    return _SCENES[(name, how)]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _SCENES.values():
        ds.close()
    _SCENES.clear()


def frame_and_radiance(ds, cfg, w, h, **kw):
    """(render's u8, f32, stats), (radiance's u8, f32, stats) of a frame's own camera rays, as host arrays shaped (h, w, 4)"""
    import torch
    rays = ds.camera_rays(ONE, w, h)
    f32, u8, st = ds.radiance(rays, cfg, rgba8=True, collect_stats=True, **kw)
    torch.cuda.synchronize()
    ru8, rf32, rst = ds.render(cfg, w, h, engine=abi.ENGINE_FUSED, collect_stats=True)
    return (ru8, rf32, rst), (host(u8).reshape(h, w, 4), host(f32).reshape(h, w, 4), st)


def assert_same_frame(got, want, what):
    (u8, f32, st), (ru8, rf32, rst) = got, want
    bad = np.flatnonzero((bits(f32) != bits(rf32)).any(axis=-1))
    assert bad.size == 0, f"{what}: {bad.size} pixels differ, first {bad[:4]}: {f32.reshape(-1, 4)[bad[:2]]} vs {rf32.reshape(-1, 4)[bad[:2]]}"
    assert np.array_equal(u8, ru8), what
    assert {k: st[k] for k in COUNTS} == {k: rst[k] for k in COUNTS}, what


# ---- 1: a frame's own camera rays give the frame ------------------------------------------------------------------------------
FRAMES = [
    ("cornell", FLAT, 61, 35),                                   # ragged: 2135 rays, no multiple of 64 or 256
    ("cornell", Config(max_depth=1), 64, 36),
    ("cornell", Config(max_depth=4, seed=3), 64, 36),
    ("cornell", Config(max_depth=3, indirect_sampler=S.Hemisphere, gamma=2.2), 48, 27),
    ("room_phong", Config(max_depth=3, direct_sampler=S.NONE), 48, 27),   # the other collect_emissive arm
    ("room_phong", Config(max_depth=1, light_samples=4, light_stratify=True), 48, 36),
    ("sphere", Config(max_depth=2), 32, 32),
    ("textured", Config(max_depth=2), 32, 32),
]


@pytest.mark.parametrize("how", ["reference", "sah"])
@pytest.mark.parametrize("case", range(len(FRAMES)))
def test_a_frames_camera_rays_give_the_frame(gpu, case, how):
    name, cfg, w, h = FRAMES[case]
    if how == "reference":
        want, got = frame_and_radiance(scene(name, how), cfg, w, h)
        assert_same_frame(got, want, f"{name} {cfg}")
    else:
        # a fresh scene: the first call meets a scene whose other node formats may still be in the making
        ds = DeviceScene(desc_of(name), Config(), builder=abi.BUILDER_SAH)
        try:
            want, early = frame_and_radiance(ds, cfg, w, h)
            ds.finish()
            _, late = frame_and_radiance(ds, cfg, w, h)
            assert_same_frame(early, want, f"{name} {cfg} before finish()")
            assert_same_frame(late, want, f"{name} {cfg} after finish()")
        finally:
            ds.close()
    assert float(want[1][..., :3].max()) > 0.01, "the case renders nothing"
    assert want[2]["rays_primary"] == w * h and (cfg.integrator == I.Flat or cfg.max_depth < 2 or want[2]["rays_bounce"] > 0)


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_fewer_rays_than_a_wave(gpu, how):
    import torch
    ds, cfg, w, h = scene("cornell", how), Config(max_depth=4, seed=3), 64, 36
    rays = ds.camera_rays(ONE, w, h)
    f32, u8 = ds.radiance(rays[:5], cfg, rgba8=True)
    torch.cuda.synchronize()
    ru8, rf32, _ = ds.render(cfg, w, h, engine=abi.ENGINE_FUSED)
    assert np.array_equal(bits(host(f32)), bits(rf32.reshape(-1, 4)[:5])) and np.array_equal(host(u8), ru8.reshape(-1, 4)[:5])


# ---- 2: a ray that sees the light directly --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [Config(max_depth=3), Config(max_depth=3, direct_sampler=S.NONE)])
def test_a_pixel_that_sees_the_light_gets_its_emission(gpu, cfg):
    import torch
    # (the quad-light room: its lamp is an emissive panel, 16 pixels of this frame on the CPU oracle; the Cornell room is lit
    # by a point light and has no emissive surface to see)
    ds, w, h = scene("room_phong", "sah"), 64, 36
    rays = ds.camera_rays(ONE, w, h)
    t, prim, uv = ds.query(rays)
    s = ds.surface(rays, t, prim, uv, want=("flags", "color"))
    f32 = ds.radiance(rays, cfg)
    torch.cuda.synchronize()
    lit = (host(s["flags"]).view(np.uint32) & abi.SURFACE_EMISSIVE) != 0
    assert lit.sum() >= 1, "no pixel of this frame sees the light"
    _, rf32, _ = ds.render(cfg, w, h, engine=abi.ENGINE_FUSED)
    got, emission = host(f32)[lit], np.float32(0) + host(s["color"])[lit][:, :3]
    assert np.array_equal(got[:, :3], emission) and (got[:, 3] == 1).all() and float(emission.max()) > 0
    assert np.array_equal(bits(got), bits(rf32.reshape(-1, 4)[lit]))


# ---- 3: chunks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_chunks_with_first_index_give_what_one_call_gives(gpu, how):
    import torch
    ds, cfg, w, h = scene("cornell", how), Config(max_depth=3, seed=11), 64, 36
    rays = ds.camera_rays(ONE, w, h)
    n = w * h
    whole, whole8 = ds.radiance(rays, cfg, rgba8=True)
    parts, parts8 = torch.full((n, 4), -7.0, device="cuda"), torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    cuts = [0, 700, 701, n]   # uneven, one of a single ray, none a multiple of 64
    for a, b in zip(cuts, cuts[1:]):
        ds.radiance(rays[a:b], cfg, first_index=a, out=parts[a:b], rgba8=parts8[a:b])
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(parts)), bits(host(whole))) and np.array_equal(host(parts8), host(whole8))
    # ... and first_index is read: the same rays as pixels 1000.. of the frame are other paths
    other = ds.radiance(rays[:700], cfg, first_index=1000)
    torch.cuda.synchronize()
    assert not np.array_equal(bits(host(other)), bits(host(whole)[:700]))


# ---- 4: Flat on rays no camera makes ----------------------------------------------------------------------------------------------
def miss_pixel():
    """what a render writes for a camera ray that hits nothing (gamma 1): a corner of the box frame"""
    ds = scene("box", "reference")
    _, f32, _ = ds.render(FLAT, 32, 32)
    t, prim, _ = ds.query(ds.camera_rays(ONE, 32, 32)[:1])
    assert int(prim[0]) == -1
    return f32[0, 0]


def assert_flat_is_query_plus_surface(ds, rays, what):
    import torch
    rays_d = dev(rays)
    t, prim, uv = ds.query(rays_d)
    color = ds.surface(rays_d, t, prim, uv, want=("color",))["color"]
    f32, u8 = ds.radiance(rays_d, FLAT, rgba8=True)
    torch.cuda.synchronize()
    hit, got, color = host(prim) != -1, host(f32), host(color)
    with np.errstate(invalid="ignore"):
        want_rgb = np.float32(0) + color[:, :3]
    assert np.array_equal(got[hit][:, :3], want_rgb[hit], equal_nan=True), what
    assert np.array_equal(bits(got[~hit]), np.broadcast_to(bits(miss_pixel()), got[~hit].shape)), what
    return hit, got, host(u8)


def ortho_grid(nx=40, ny=30, half=1.0, dist=4.0, d=(-0.2, -0.3, -1.0)):
    """an orthographic camera on the box (which fills [-0.5, 0.5]^3): parallel rays from a plane, 32 % of them hits on the CPU
    oracle.  Tilted: a ray along an axis has zero direction components, whose reciprocal the reference takes as 0, and misses
    every box -- that grid is the `axis_grid` below, for which the query says "miss" 1200 times."""
    d = np.array(d, np.float64)
    d /= np.linalg.norm(d)
    right = np.cross(d, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, d)
    u, v = np.meshgrid(np.linspace(-half, half, nx), np.linspace(half, -half, ny))
    o = -dist * d + u.reshape(-1, 1) * right + v.reshape(-1, 1) * up
    return np.concatenate([o, np.broadcast_to(d, o.shape)], 1).astype(np.float32)


def axis_grid(nx=40, ny=30, half=1.0):
    x, y = np.meshgrid(np.linspace(-half, half, nx, dtype=np.float32), np.linspace(half, -half, ny, dtype=np.float32))
    o = np.stack([x.ravel(), y.ravel(), np.full(nx * ny, 3.0, np.float32)], 1)
    return np.concatenate([o, np.broadcast_to(np.array([0, 0, -1], np.float32), o.shape)], 1).astype(np.float32)


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_flat_on_an_orthographic_grid_and_its_shuffle(gpu, how):
    ds, rays = scene("box", how), ortho_grid()
    hit, got, got8 = assert_flat_is_query_plus_surface(ds, rays, "orthographic grid")
    assert 0.1 < hit.mean() < 0.9, "the grid should see the box and the background"
    perm = np.random.default_rng(5).permutation(rays.shape[0])
    _, shuffled, shuffled8 = assert_flat_is_query_plus_surface(ds, rays[perm], "shuffled grid")
    assert np.array_equal(bits(shuffled), bits(got[perm])) and np.array_equal(shuffled8, got8[perm])
    # a direction that is not normalised is the query's ray too
    assert_flat_is_query_plus_surface(ds, rays * np.array([1, 1, 1, 7, 7, 7], np.float32), "scaled directions")
    assert_flat_is_query_plus_surface(ds, axis_grid(), "rays along -z")


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_flat_on_the_adversarial_families(gpu, how):
    ds = scene("edges:cornell", how)
    for fam in re_.FAMILIES:
        rays = re_.family("cornell", fam)
        rays = rays[::max(1, rays.shape[0] // 300)]   # a few hundred of each
        hit, _, _ = assert_flat_is_query_plus_surface(ds, rays, fam)
        print(fam, rays.shape[0], "rays,", int(hit.sum()), "hits")


# ---- 5: sample -----------------------------------------------------------------------------------------------------------------
def test_sample_selects_the_stream_and_runs_repeat(gpu):
    import torch
    ds, cfg = scene("cornell", "sah"), Config(max_depth=3)
    rays = ds.camera_rays(ONE, 64, 36)
    a0, b0, a1, b1 = (ds.radiance(rays, cfg, sample=k) for k in (0, 1, 0, 1))
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(a0)), bits(host(a1))) and np.array_equal(bits(host(b0)), bits(host(b1)))
    assert (bits(host(a0)) != bits(host(b0))).any(axis=1).mean() > 0.25


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------
def test_configs_off_the_generation_kernels_are_refused(gpu):
    import torch
    ds = scene("cornell", "sah")
    rays = ds.camera_rays(ONE, 32, 18)
    before = ds.render(Config(max_depth=3), 32, 18)[1]
    for cfg, field in ((Config(integrator=I.Raytracer), "integrator"), (Config(russian_roulette=True), "russian_roulette"),
                       (Config(direct_sampler=S.Mis), "direct_sampler"), (Config(max_depth=3, light_samples=2), "light_samples")):
        with pytest.raises(RaycaError) as e:
            ds.radiance(rays, cfg)
        assert e.value.code == abi.ERR_UNSUPPORTED and field in str(e.value), (cfg, str(e.value))
    out = torch.full((32 * 18, 4), -7.0, device="cuda")
    r = abi.RaycaRadiance()
    r.count, r.rays, r.rgba32f_out = 32 * 18, rays.data_ptr(), out.data_ptr()
    o, c = ds._opts(abi.TRAVERSAL_EXHAUSTIVE, False, None, None), Config(max_depth=3).to_abi()
    assert gpu.rayca_hip_radiance_device(ds.handle, C.byref(c), C.byref(o), C.byref(r), None) == abi.ERR_UNSUPPORTED
    assert "traversal" in lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert np.array_equal(bits(ds.render(Config(max_depth=3), 32, 18)[1]), bits(before))


# ---- 7: another stream and context --------------------------------------------------------------------------------------------
def test_a_query_on_its_own_context_beside_frames_in_flight(gpu):
    import torch
    ds, cfg, w, h = scene("cornell", "sah"), Config(max_depth=3, seed=2), 64, 36
    rays = ds.camera_rays(ONE, w, h)
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    frame_solo = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    frames = [torch.zeros_like(frame_solo) for _ in range(4)]
    torch.cuda.synchronize()
    ds.render_device(cfg, w, h, 0, frame_solo.data_ptr(), stream=s0.cuda_stream, context=0)
    torch.cuda.synchronize()
    solo = ds.radiance(rays, cfg, sample=1, stream=s1, context=1)
    torch.cuda.synchronize()
    for f in frames:
        ds.render_device(cfg, w, h, 0, f.data_ptr(), stream=s0.cuda_stream, context=0)
    beside = ds.radiance(rays, cfg, sample=1, stream=s1, context=1)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(beside)), bits(host(solo))) and float(solo[:, :3].max()) > 0
    for f in frames:
        assert torch.equal(f, frame_solo)
    assert not torch.equal(solo.view(h, w, 4), frame_solo)   # (sample 1 is another stream than the frame's sample 0)


# ---- 8: a jittered film -------------------------------------------------------------------------------------------------------
# On the CPU oracle (Flat, 64 x 64, 4 spp against 1 spp, a channel apart by more than 0.05): cornell 128 pixels, box 0 -- the
# box's silhouette is axis-aligned and falls on pixel boundaries at this size, so all four sub-samples of every pixel agree and
# the two frames are equal to 1.8e-7.  The box therefore checks the film against the supersampled frame; that jitter changes
# what a geometric edge converges to is checked where there are such edges, on the Cornell room.
@pytest.mark.parametrize("name,edges", [("box", False), ("cornell", True)])
def test_a_jittered_film_converges_to_the_supersampled_frame(gpu, name, edges):
    """Four adds with jitter=2 are the four sub-samples of a 4-spp frame.  The film's running mean and the frame's sum / 4 are
    means of the same four f32 values in [0, 1] in different associations: each of the film's three updates and each of the
    frame's three additions and its division rounds once, an error of at most half an ulp of a value <= 4, i.e. 2^-22 for the
    sums and 2^-25 .. 2^-24 for the means -- a few units of 2^-24 in all, under 1e-6 (= 16.8 x 2^-24)."""
    import torch
    ds, n = scene(name, "sah"), 64
    film, plain = Film(ds, n, n), Film(ds, n, n)
    for _ in range(4):
        film.add(FLAT, jitter=2)
        plain.add(FLAT)
    torch.cuda.synchronize()
    _, spp4, _ = ds.render(dataclasses.replace(FLAT, samples_per_pixel=4), n, n)
    _, spp1, _ = ds.render(FLAT, n, n)
    edge = (np.abs(spp4 - spp1)[..., :3] > 0.05).any(axis=-1)
    got, flat = host(film.color), host(plain.color)
    print(name, "pixels where 4 spp and 1 spp differ by more than 0.05:", int(edge.sum()))
    print("max |film - 4 spp|:", float(np.abs(got - spp4).max()), " max |plain film - 1 spp|:", float(np.abs(flat - spp1).max()))
    assert float(spp4[..., :3].max()) > 0.1
    assert float(np.abs(got - spp4).max()) <= 1e-6
    assert float(np.abs(flat - spp1).max()) <= 1e-6          # the un-jittered film is the 1-spp frame: it keeps the stair
    if edges:
        assert edge.sum() >= 1, "no geometric edge in this frame"
        assert float(np.abs(got - spp1)[edge].max()) > 0.05 - 1e-6
    with pytest.raises(ValueError):
        film.add(FLAT, jitter=9)
    with pytest.raises(RaycaError) as e:
        film.add(Config(russian_roulette=True), jitter=2)
    assert e.value.code == abi.ERR_UNSUPPORTED


def test_a_film_without_jitter_is_the_film_it_was(gpu):
    """jitter=None: render_device + accumulate with the film's seed rule, as before"""
    import torch
    ds, n, cfg = scene("cornell", "sah"), 32, Config(max_depth=2, seed=5, gamma=2.2)
    film = Film(ds, n, n)
    frame = torch.empty((n, n, 4), dtype=torch.float32, device="cuda")
    hist = None
    for k in range(3):
        film.add(cfg)
        ds.render_device(dataclasses.replace(cfg, gamma=1.0, seed=cfg.seed + k), n, n, 0, frame.data_ptr(), stream=ds.stream_handle() or None)
        hist = ds.accumulate(frame, history=hist, moments=True)
        hist = {k_: v for k_, v in hist.items() if k_ != "variance"}
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(film.color)), bits(host(hist["color"]))) and np.array_equal(bits(host(film.length)), bits(host(hist["length"])))
    assert float(film.color[..., :3].max()) > 0
