"""rayca_hip_gather_device / DeviceScene.gather: the light that arrives at points in device memory.

Expected values never come from the code under test.  They are the rays of tests/ambient_literal.py (the header's text in numpy
f32) put through DeviceScene.radiance(rays, cfg, sample=, first_index=), which test_gpu_radiance.py pins bit for bit against a
frame, folded by tests/gather_literal.py.  Every comparison is of bits, on all four outputs.  The inputs are tests/gather_cases.py's:
ambient_cases' 576 points per scene, five of them inactive.  Each scene is run three ways: RAYCA_BUILDER_REFERENCE, RAYCA_BUILDER_SAH
after finish() and RAYCA_BUILDER_SAH right after creation.

The meaningfulness condition (asserted once per path-traced Cornell case, on the expected values): at least a quarter of the active
points have a non-zero E and at least a quarter keep every sample -- a comparison of zeros cannot pass for parity."""
import ctypes as C

import numpy as np
import pytest

import ambient_literal as al
import gather_cases as gc
import gather_literal as gl
import ray_edges as R
from rayca_amd import Config, DeviceScene, IntegratorStrategy, SamplerStrategy, abi, lib
from rayca_amd.ambient import cosine_directions, pixel_rotations
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
HOW = ["reference", "sah", "sah_unfinished"]
WANT = ("irradiance", "sh", "kept", "samples")
_SCENES, _RAYS = {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_scene(name, how):
    ds = DeviceScene(R.scene_desc(name), Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    if how == "sah":
        ds.finish()
    return ds


def scene(name, how):
    """the module's scenes, one per (scene, builder); the unfinished ones are made by the test that wants them"""
    assert how in ("reference", "sah")
    if (name, how) not in _SCENES:
        _SCENES[(name, how)] = make_scene(name, how)
    return _SCENES[(name, how)]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _SCENES.values():
        ds.close()
    _SCENES.clear()
    _RAYS.clear()


def literal_rays(key, p, n, rot, table, samples, bias, dir_first=0):
    """the literal's (o, d), once per input set"""
    if key not in _RAYS:
        _RAYS[key] = al.rays(p, n, rot, table, samples, bias, dir_first)
    return _RAYS[key]


def expected(ds, key, p, n, cfg, samples, *, rot=None, table=None, weights=None, dir_first=0, bias=0.0, sample=0, first_index=0):
    """((irradiance, sh, kept, samples), act) as the specification has them: the literal's rays through DeviceScene.radiance with the
    call's `sample` and the ray's pixel index, the literal's fold"""
    import torch
    table = gc.table(64) if table is None else table
    act = al.active(p, n)
    o, d = literal_rays(key, p, n, rot, table, samples, bias, dir_first)
    r = np.concatenate([o, d], 2).reshape(-1, 6).copy()
    r[~np.repeat(act, samples)] = 0.0                       # (rows of inactive points: traced, never read)
    L = ds.radiance(dev(r), cfg, sample=sample, first_index=first_index)
    torch.cuda.synchronize()
    L = L.cpu().numpy().reshape(p.shape[0], samples, 4)
    w = None if weights is None else weights[dir_first:dir_first + samples]
    return gl.fold(L, act, d, samples, w), act


def run(ds, p_d, n_d, cfg, outputs=WANT, **kw):
    import torch
    got = ds.gather(p_d, n_d, cfg, outputs=outputs, **kw)
    torch.cuda.synchronize()
    out = {k: got[k].cpu().numpy() for k in outputs}
    if "kept" in out:
        out["kept"] = out["kept"].view(np.uint32)
    if "stats" in got:
        out["stats"] = got["stats"]
    return out


def assert_same(got, want, what=""):
    for k, w in zip(WANT, want):
        if k in got:
            g = got[k]
            assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype)
            bad = np.flatnonzero((bits(g) != bits(w)).reshape(w.shape[0], -1).any(axis=1))
            assert bad.size == 0, f"{what}: {k} differs at {bad.size} of {w.shape[0]} points, first {bad[:5]}: got {g[bad[:2]]}, want {w[bad[:2]]}"


def assert_meaningful(want, act, samples, what):
    lit, full = gc.meaningful(want[0], want[2], act, samples)
    print(f"{what}: {lit:.3f} of the active points with E != 0, {full:.3f} with kept == S")
    assert lit >= 0.25 and full >= 0.25, (what, lit, full)


# ---- 1: three scenes, three builds, four sample counts, three Configs ----------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", gc.SCENES)
def test_all_outputs_match_the_specification(gpu, name, how):
    ds = make_scene(name, how) if how == "sah_unfinished" else scene(name, how)
    try:
        if name == "spheres":
            assert ds.info()["sphere_count"] > 0
        p, n, _ = gc.points_for(name)
        p_d, n_d = dev(p), dev(n)
        rot, table, weights, bias = gc.rotations(), gc.table(64), gc.weights(64), gc.bias(name)
        rot_d, table_d, weights_d = dev(rot), dev(table), dev(weights)
        idx = gc.ac.inactive_index()
        for cname, cfg in gc.CONFIGS.items():
            for samples in gc.SAMPLE_COUNTS:
                what = f"{name} {how} {cname} S={samples}"
                got = run(ds, p_d, n_d, cfg, samples=samples, bias=float(bias), dirs=table_d, rotations=rot_d, weights=weights_d, sample=3, first_index=1000)
                want, act = expected(ds, (name, samples, "rot"), p, n, cfg, samples, rot=rot, table=table, weights=weights, bias=bias, sample=3, first_index=1000)
                assert_same(got, want, what)
                if name == "cornell" and cname in gc.PATH_TRACED:
                    assert_meaningful(want, act, samples, what)
                assert not got["irradiance"][idx].any() and not got["sh"][idx].any() and not got["kept"][idx].any() and not bits(got["samples"][idx]).any()
                assert act.sum() == gc.COUNT - idx.size and np.isfinite(got["irradiance"]).all() and np.isfinite(got["sh"]).all()
    finally:
        if how == "sah_unfinished":
            ds.close()


# ---- 2: tiny batches, the empty batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_tiny_batches(gpu, how):
    name, cfg = "cornell", gc.CONFIGS["depth3"]
    ds = scene(name, how)
    p, n, _ = gc.points_for(name)
    table, bias = gc.table(64), gc.bias(name)
    for count in (1, 37, 63):
        want, _ = expected(ds, (name, "tiny", count), p[:count], n[:count], cfg, 5, table=table, bias=bias)
        got = run(ds, dev(p[:count]), dev(n[:count]), cfg, samples=5, bias=float(bias), dirs=dev(table))
        assert_same(got, want, f"{count} points x 5")
    empty = ds.gather(dev(p[:0]), dev(n[:0]), cfg, samples=5, outputs=WANT, want_stats=True)
    assert [tuple(empty[k].shape) for k in WANT] == [(0, 4), (0, 9, 4), (0,), (0, 5, 4)] and empty["stats"]["kernel_launches"] == 0


# ---- 3: chunks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_chunk_points_changes_no_bit(gpu, how):
    name, cfg, count, samples = "cornell", gc.CONFIGS["depth3"], 37, 5
    ds = scene(name, how)
    p, n, _ = gc.points_for(name)
    p, n = p[:count], n[:count]
    table, bias, rot = gc.table(64), gc.bias(name), gc.rotations(count)
    want, act = expected(ds, (name, "chunks"), p, n, cfg, samples, rot=rot, table=table, bias=bias, first_index=77)
    assert_meaningful(want, act, samples, "chunks")
    launches = {}
    for chunk in (0, 1, 7, 100):
        got = run(ds, dev(p), dev(n), cfg, samples=samples, bias=float(bias), dirs=dev(table), rotations=dev(rot), first_index=77, chunk_points=chunk, want_stats=True)
        assert_same(got, want, f"chunk_points {chunk}")
        st = got["stats"]
        frames = 1 if chunk in (0, 100) else -(-count // chunk)
        assert st["rows_rendered"] == frames and st["rays_primary"] == count * samples, (chunk, st)
        assert st["class_launches"][abi.KERNEL_OTHER] >= 2 * frames and st["kernel_ms"] > 0       # the enqueue and the fold of every frame
        launches[chunk] = st["kernel_launches"]
    assert launches[1] > launches[7] > launches[0] == launches[100], launches
    # without samples_out the records live in the context's scratch, sized by the chunk: the same bits
    for chunk in (0, 7):
        got = run(ds, dev(p), dev(n), cfg, outputs=("irradiance", "sh", "kept"), samples=samples, bias=float(bias), dirs=dev(table), rotations=dev(rot), first_index=77,
                  chunk_points=chunk)
        assert_same(got, want, f"chunk_points {chunk}, scratch records")


# ---- 4: the last pixel index, dir_first, weights and rotations -------------------------------------------------------------------------
def test_first_index_up_to_the_last_stream(gpu):
    name, cfg, count, samples = "cornell", gc.CONFIGS["depth3"], 37, 5
    ds = scene(name, "sah")
    p, n, _ = gc.points_for(name)
    p, n = p[:count], n[:count]
    first = (1 << 32) - count * samples                       # the last ray's index is 2^32 - 1
    want, _ = expected(ds, (name, "last"), p, n, cfg, samples, bias=gc.bias(name), first_index=first)
    got = run(ds, dev(p), dev(n), cfg, samples=samples, bias=float(gc.bias(name)), dirs=dev(gc.table(64)), first_index=first, chunk_points=10)
    assert_same(got, want, "first_index 2^32 - count x S")
    other, _ = expected(ds, (name, "last"), p, n, cfg, samples, bias=gc.bias(name), first_index=0)
    assert (bits(other[3]) != bits(want[3])).any(), "first_index must select other streams"
    with pytest.raises(ValueError):
        ds.gather(dev(p), dev(n), cfg, samples=samples, first_index=first + 1)


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_dir_first_splits_a_table(gpu, how):
    name, cfg = "cornell", gc.CONFIGS["depth1"]
    ds = scene(name, how)
    p, n, _ = gc.points_for(name)
    p_d, n_d, table, weights, rot, bias = dev(p), dev(n), gc.table(64), gc.weights(64), gc.rotations(), gc.bias(name)
    kw = dict(bias=float(bias), dirs=dev(table), weights=dev(weights), rotations=dev(rot))
    for first, samples in ((0, 24), (24, 40), (63, 1)):
        want, _ = expected(ds, (name, "split", first), p, n, cfg, samples, rot=rot, table=table, weights=weights, dir_first=first, bias=bias)
        got = run(ds, p_d, n_d, cfg, samples=samples, dir_first=first, **kw)
        assert_same(got, want, f"dir_first {first}, {samples} samples")
    with pytest.raises(ValueError):
        ds.gather(p_d, n_d, cfg, samples=2, dir_first=63, **kw)


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_with_and_without_weights_and_rotations(gpu, how):
    name, cfg, samples = "cornell", gc.CONFIGS["depth3"], 16
    ds = scene(name, how)
    p, n, _ = gc.points_for(name)
    p_d, n_d, table, weights, rot, bias = dev(p), dev(n), gc.table(64), gc.weights(64), gc.rotations(), gc.bias(name)
    seen = []
    for rotated in (False, True):
        for weighted in (False, True):
            want, act = expected(ds, (name, samples, "rot" if rotated else "plain"), p, n, cfg, samples, rot=rot if rotated else None, table=table,
                                 weights=weights if weighted else None, bias=bias)
            got = run(ds, p_d, n_d, cfg, samples=samples, bias=float(bias), dirs=dev(table), rotations=dev(rot) if rotated else None,
                      weights=dev(weights) if weighted else None)
            assert_same(got, want, f"rotated {rotated}, weighted {weighted}")
            assert_meaningful(want, act, samples, f"rotated {rotated}, weighted {weighted}")
            seen.append(want[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])    # both inputs are read


# ---- 5: output subsets and guard words ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_output_subsets_and_guards(gpu, how):
    import torch
    name, cfg, samples = "cornell", gc.CONFIGS["depth1"], 5
    ds = scene(name, how)
    p, n, _ = gc.points_for(name)
    count = gc.COUNT - 5                                                  # (not a multiple of 64)
    p, n = p[:count], n[:count]
    p_d, n_d, table, rot = dev(p), dev(n), gc.table(16), gc.rotations(count)
    table_d, rot_d, bias = dev(table), dev(rot), gc.bias(name)
    want, _ = expected(ds, (name, "guards"), p, n, cfg, samples, rot=rot, table=table, bias=bias)
    shape = {"irradiance": (4,), "sh": (9, 4), "kept": (), "samples": (samples, 4)}
    sentinel = {"irradiance": -7.0, "sh": -7.0, "kept": 0x5A5A5A5A, "samples": -7.0}
    big = {k: torch.full((count + 128, *shape[k]), sentinel[k], dtype=torch.int32 if k == "kept" else torch.float32, device="cuda") for k in WANT}

    def check(asked, what):
        for k in WANT:
            if k in asked:
                got = big[k][64:-64].cpu().numpy()
                assert_same({k: got.view(np.uint32) if k == "kept" else got}, want, what)
                assert bool((big[k][:64] == sentinel[k]).all()) and bool((big[k][-64:] == sentinel[k]).all()), (what, k, "guard words")
            else:
                assert bool((big[k] == sentinel[k]).all()), (what, k, "an output that was not asked for")
            big[k].fill_(sentinel[k])

    # through the wrapper: all four, and one alone
    for asked in (WANT, ("sh",)):
        r = ds.gather(p_d, n_d, cfg, samples=samples, bias=float(bias), dirs=table_d, rotations=rot_d, outputs=asked, out={k: big[k][64:-64] for k in asked}, chunk_points=200)
        torch.cuda.synchronize()
        assert all(r[k].data_ptr() == big[k][64:-64].data_ptr() for k in asked)
        check(asked, f"outputs={asked}")
    # through the C ABI: every subset of the four pointers
    c = cfg.to_abi()
    for subset in range(1, 16):
        g = abi.RaycaGather()
        g.count, g.samples, g.dir_count, g.bias, g.chunk_points = count, samples, 16, float(bias), 200 if subset & 1 else 0
        g.points, g.normals, g.dirs, g.rotations = p_d.data_ptr(), n_d.data_ptr(), table_d.data_ptr(), rot_d.data_ptr()
        asked = tuple(k for j, k in enumerate(WANT) if subset >> j & 1)
        for k in asked:
            setattr(g, k + "_out", big[k][64:-64].data_ptr())
        o = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
        st = abi.RaycaStats()
        lib.check(gpu.rayca_hip_gather_device(ds.handle, C.byref(c), C.byref(o), C.byref(g), C.byref(st)))   # (no stream: the call waits)
        assert st.rays_primary == count * samples and st.rows_rendered == (3 if subset & 1 else 1)
        check(asked, f"subset {subset}")


# ---- 6: repeatability, `sample`, another stream and context ---------------------------------------------------------------------------
def test_repeatable_and_sample_selects_the_stream(gpu):
    name = "cornell"
    ds = scene(name, "sah")
    p, n, _ = gc.points_for(name)
    p_d, n_d = dev(p), dev(n)
    kw = dict(samples=16, bias=float(gc.bias(name)), dirs=dev(gc.table(64)))
    path, flat = gc.CONFIGS["depth3"], gc.CONFIGS["flat"]
    a0, b0, a1, b1 = (run(ds, p_d, n_d, path, sample=k, **kw) for k in (0, 1, 0, 1))
    for k in WANT:
        assert np.array_equal(bits(a0[k]), bits(a1[k])) and np.array_equal(bits(b0[k]), bits(b1[k])), k
    act = al.active(p, n)
    assert (bits(a0["irradiance"]) != bits(b0["irradiance"])).any(axis=1)[act].mean() > 0.25, "another sample is another set of paths"
    f0, f1 = (run(ds, p_d, n_d, flat, sample=k, **kw) for k in (0, 1))
    for k in WANT:
        assert np.array_equal(bits(f0[k]), bits(f1[k])), k                 # Flat draws no random numbers
    assert f0["irradiance"][act, :3].any()


def test_on_another_stream_and_context_beside_a_frame_in_flight(gpu):
    import torch
    name, cfg, w, h = "cornell", gc.CONFIGS["depth3"], 64, 36
    ds = scene(name, "sah")
    p, n, _ = gc.points_for(name)
    p_d, n_d = dev(p), dev(n)
    kw = dict(samples=16, bias=float(gc.bias(name)), dirs=dev(gc.table(64)), rotations=dev(gc.rotations()), chunk_points=100)
    want, _ = expected(ds, (name, 16, "rot"), p, n, cfg, 16, rot=gc.rotations(), bias=gc.bias(name))
    s0, streams = torch.cuda.Stream(), [torch.cuda.Stream() for _ in range(2)]
    frame_solo = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    frames = [torch.zeros_like(frame_solo) for _ in range(4)]
    torch.cuda.synchronize()
    ds.render_device(cfg, w, h, 0, frame_solo.data_ptr(), stream=s0.cuda_stream, context=0)
    torch.cuda.synchronize()
    for f in frames:
        ds.render_device(cfg, w, h, 0, f.data_ptr(), stream=s0.cuda_stream, context=0)
    res = [ds.gather(p_d, n_d, cfg, outputs=WANT, stream=s, context=k + 1, **kw) for k, s in enumerate(streams)]
    raw = ds.gather(p_d, n_d, cfg, outputs=("irradiance", "sh"), stream=streams[0].cuda_stream, context=7, **kw)   # (scratch records of context 7)
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        got = {x: r[x].cpu().numpy() for x in WANT}
        got["kept"] = got["kept"].view(np.uint32)
        assert_same(got, want, f"context {k + 1}")
    assert_same({x: raw[x].cpu().numpy() for x in ("irradiance", "sh")}, want, "context 7, a raw stream handle")
    for f in frames:
        assert torch.equal(f, frame_solo)
    with pytest.raises(RaycaError):
        ds.gather(p_d, n_d, cfg, context=8, **kw)


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------
def test_configs_the_call_does_not_serve_are_refused(gpu):
    import torch
    I, S = IntegratorStrategy, SamplerStrategy
    name = "cornell"
    ds = scene(name, "sah")
    p, n, _ = gc.points_for(name)
    p_d, n_d = dev(p), dev(n)
    out = torch.full((gc.COUNT, 4), -7.0, device="cuda")
    for cfg, field in ((Config(integrator=I.Raytracer), "integrator"), (Config(russian_roulette=True), "russian_roulette"),
                       (Config(direct_sampler=S.Mis), "direct_sampler"), (Config(max_depth=3, light_samples=2), "light_samples"),
                       (Config(max_depth=3, gamma=2.2), "gamma"), (Config(integrator=I.Flat, gamma=0.5), "gamma")):
        with pytest.raises(RaycaError) as e:
            ds.gather(p_d, n_d, cfg, samples=16, out={"irradiance": out})
        assert e.value.code == abi.ERR_UNSUPPORTED and f"RaycaConfig.{field}" in str(e.value), (cfg, str(e.value))
    g = abi.RaycaGather()
    table_d = dev(gc.table(16))
    g.count, g.samples, g.dir_count = gc.COUNT, 16, 16
    g.points, g.normals, g.dirs, g.irradiance_out = p_d.data_ptr(), n_d.data_ptr(), table_d.data_ptr(), out.data_ptr()
    o, c = ds._opts(abi.TRAVERSAL_EXHAUSTIVE, False, None, None), Config(max_depth=3).to_abi()
    assert gpu.rayca_hip_gather_device(ds.handle, C.byref(c), C.byref(o), C.byref(g), None) == abi.ERR_UNSUPPORTED
    assert "traversal" in lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- 8: statistics -------------------------------------------------------------------------------------------------------------------
def test_statistics_are_the_radiance_calls(gpu):
    """The same rays through the same kernels: rays_shadow, rays_bounce and hits_shaded are what the radiance call reports for the
    literal's rays (inactive points queue the zero ray, which misses: rays_primary counts them, nothing else does)."""
    import torch
    name, cfg, samples = "cornell", gc.CONFIGS["depth3"], 16
    ds = scene(name, "sah")
    p, n, _ = gc.points_for(name)
    act = al.active(p, n)
    o, d = al.rays(p, n, None, gc.table(64), samples, gc.bias(name))
    r = np.concatenate([o, d], 2).reshape(-1, 6).copy()
    r[~np.repeat(act, samples)] = 0.0
    _, want = ds.radiance(dev(r), cfg, collect_stats=True)
    got = ds.gather(dev(p), dev(n), cfg, samples=samples, bias=float(gc.bias(name)), dirs=dev(gc.table(64)), collect_stats=True)["stats"]
    torch.cuda.synchronize()
    for k in ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["rays_primary"] == gc.COUNT * samples and got["rays_bounce"] > 0 and got["boxes_tested"] > 0
    assert got["kernel_launches"] == want["kernel_launches"] + 1 and got["class_launches"][abi.KERNEL_OTHER] == want["class_launches"][abi.KERNEL_OTHER] + 1   # the fold


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_the_zero_ray_of_an_inactive_point_hits_nothing(gpu, how):
    """The comparison above feeds the radiance call the same zero rays, so it cannot show that they miss.  This does: a batch of
    inactive points alone -- every way ambient_cases has of making one -- shades no hit, evaluates no light sample and bounces
    nothing, under Flat and at depth 3; and under Flat, where a ray's result depends on the ray alone (no pixel index), the shaded
    hits of the whole batch are those of its active points.  On the reference tree the root's slab test is the specification's
    (every plane distance 0, tmax > 0 false), so there no triangle is tested either; the conservative steering test of a SAH tree
    may pass boxes that the reference-leaf filter then rejects, and what it counts on the way is not asserted."""
    import torch
    name, samples = "cornell", 16
    ds = scene(name, how)
    p, n, _ = gc.points_for(name)
    act = al.active(p, n)
    idx = gc.ac.inactive_index()
    kw = dict(samples=samples, bias=float(gc.bias(name)), dirs=dev(gc.table(64)), rotations=None, collect_stats=True)
    for cname in ("flat", "depth3"):
        r = ds.gather(dev(p[idx]), dev(n[idx]), gc.CONFIGS[cname], outputs=WANT, **kw)
        torch.cuda.synchronize()
        st = r["stats"]
        assert st["rays_primary"] == idx.size * samples, st
        for k in ("hits_shaded", "rays_shadow", "rays_bounce") + (("triangles_tested",) if how == "reference" else ()):
            assert st[k] == 0, (cname, k, st[k])
        print(f"{how} {cname}: boxes {st['boxes_tested']}, triangles {st['triangles_tested']} for {idx.size * samples} zero rays")
        assert not any(bits(r[k].cpu().numpy()).any() for k in WANT), cname
    whole = ds.gather(dev(p), dev(n), gc.CONFIGS["flat"], **kw)["stats"]
    active_only = ds.gather(dev(p[act]), dev(n[act]), gc.CONFIGS["flat"], **kw)["stats"]
    torch.cuda.synchronize()
    assert whole["hits_shaded"] == active_only["hits_shaded"] > 0
    assert how != "reference" or whole["triangles_tested"] == active_only["triangles_tested"] > 0
    assert whole["rays_primary"] - active_only["rays_primary"] == idx.size * samples


# ---- 9: the wrappers -----------------------------------------------------------------------------------------------------------------
def test_render_irradiance_is_gbuffer_then_gather(gpu):
    import torch
    ds = scene("cornell", "sah")
    cfg, w, h = Config(max_depth=2), 64, 36
    img = ds.render_irradiance(cfg, w, h, samples=16, bias=1e-3, outputs=("irradiance", "sh", "kept"))
    g = ds.gbuffer(cfg, w, h, want=("point", "normal"))
    rot = torch.from_numpy(pixel_rotations(w, h).reshape(-1, 2)).cuda()
    a = ds.gather(g["point"].reshape(-1, 3), g["normal"].reshape(-1, 3), cfg, samples=16, bias=1e-3, rotations=rot, outputs=("irradiance", "sh", "kept"))
    torch.cuda.synchronize()
    assert img["irradiance"].shape == (h, w, 4) and img["sh"].shape == (h, w, 9, 4) and img["kept"].shape == (h, w)
    for k in ("irradiance", "sh", "kept"):
        assert np.array_equal(bits(img[k].cpu().numpy().reshape(a[k].shape)), bits(a[k].cpu().numpy())), k
    miss = (g["prim"] == -1).cpu().numpy()
    e = img["irradiance"].cpu().numpy()
    assert 0 < miss.sum() < miss.size and not e[miss].any() and not img["kept"].cpu().numpy()[miss].any()
    assert (e[~miss][:, 3] == 1.0).all() and (e[~miss][:, :3] > 0).any(axis=1).mean() > 0.5, "a lit room"
    # the default table is cosine_directions(samples); against the specification on the same G-buffer
    p, n = g["point"].reshape(-1, 3).cpu().numpy(), g["normal"].reshape(-1, 3).cpu().numpy()
    want, _ = expected(ds, ("render", w, h), p, n, cfg, 16, rot=rot.cpu().numpy(), table=cosine_directions(16), bias=np.float32(1e-3))
    got = {k: a[k].cpu().numpy() for k in ("irradiance", "sh", "kept")}
    got["kept"] = got["kept"].view(np.uint32)
    assert_same(got, want, "render_irradiance")


def test_wrapper_checks(gpu):
    import torch
    ds = scene("box", "sah")
    cfg = gc.CONFIGS["flat"]
    p = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    n = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    n[:, 2] = 1.0
    with pytest.raises(ValueError):
        ds.gather(p.cpu(), n, cfg, samples=16)
    with pytest.raises(TypeError):
        ds.gather(p.double(), n, cfg, samples=16)
    with pytest.raises(TypeError):
        ds.gather(np.zeros((64, 3), np.float32), n, cfg, samples=16)
    with pytest.raises(ValueError):
        ds.gather(p, n[:63], cfg, samples=16)
    for samples in (0, 65):
        with pytest.raises(ValueError):
            ds.gather(p, n, cfg, samples=samples)
    with pytest.raises(ValueError):
        ds.gather(p, n, cfg, samples=16, dirs=torch.zeros((16, 3), device="cuda"), dir_first=1)
    with pytest.raises(ValueError):
        ds.gather(p, n, cfg, samples=16, dirs=torch.zeros((16, 3), device="cuda"), weights=torch.ones(15, device="cuda"))
    with pytest.raises(TypeError):
        ds.gather(p, n, cfg, samples=16, rotations=torch.ones((64, 2), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ds.gather(p, n, cfg, samples=16, outputs=("irradiance", "open"))
    with pytest.raises(ValueError):
        ds.gather(p, n, cfg, samples=16, outputs=())
    with pytest.raises(TypeError):
        ds.gather(p, n, cfg, samples=16, outputs=("kept",), out={"kept": torch.zeros(64, device="cuda", dtype=torch.int64)})
    with pytest.raises(RaycaError) as e:
        ds.gather(p, n, cfg, samples=16, bias=float("nan"))
    assert e.value.code == abi.ERR_BAD_ARG and "bias" in str(e.value)
    # a strided input is made contiguous; from above the box's top face every ray leaves the scene: a render's miss colour, kept = S
    wide = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    wide[:, 2] = 0.75
    a = ds.gather(wide[:, :3], n, cfg, samples=16, outputs=("irradiance", "kept", "samples"))
    torch.cuda.synchronize()
    assert (a["kept"].cpu().numpy() == 16).all() and (a["irradiance"].cpu().numpy()[:, 3] == 1.0).all()
    s = a["samples"].cpu().numpy()
    assert np.array_equal(bits(s), np.broadcast_to(bits(s[0, 0]), s.shape))
