"""rayca_hip_query_device / DeviceScene.query: closest-hit and occlusion queries on rays in device memory, with tmax.

Every comparison is bit-exact: `prim` directly, `t` / `uv` by their bits (as test_hit_records_bit_exact compares trace_rays).
Expected results follow from committed oracle records (tests/golden) or from records made in the test (the oracle, or
DeviceScene.trace_rays, whose kernel the existing suite pins to the oracle) under "a hit counts iff t < tmax, strictly".
Each scene is queried three ways: RAYCA_BUILDER_REFERENCE (one ray per lane, the reference's slabs), RAYCA_BUILDER_SAH after
finish() (the lane-refill kernel) and RAYCA_BUILDER_SAH right after creation (whichever the formats thread allows)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi, flatten, lib, scenes
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLT_MAX = np.float32(3.4028234663852886e38)
NONE = np.uint32(0xFFFFFFFF)
HOW = ["reference", "sah", "sah_unfinished"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_scene(desc, how):
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH)
    ds.builder = abi.BUILDER_REFERENCE if how == "reference" else abi.BUILDER_SAH
    if how == "sah":
        ds.finish()
    return ds


def golden(name):
    if name == "soup1k":
        return np.load(os.path.join(G, "soup1k_rays.npz")), flatten(scenes.soup_scene(1000, extent=0.12))
    if name == "box":
        return np.load(os.path.join(G, "box_256.npz")), flatten(scenes.box_scene())
    return np.load(os.path.join(G, "cornell_128x72.npz")), flatten(scenes.cornell_scene())


_REF_ORDER = {}


def in_slots(ds, desc, prim, key):
    """Oracle / golden primitive numbers (slots of the reference's build) as slots of `ds`: both builds publish which
    flattened primitive sits in which slot, and a RAYCA_BUILDER_SAH scene orders its slots differently.  On a
    RAYCA_BUILDER_REFERENCE scene this is the identity (asserted), i.e. `prim` is compared directly."""
    if key not in _REF_ORDER:
        orc = ol.OracleScene(desc, Config())
        _REF_ORDER[key] = orc.primitive_order()
        orc.close()
    ref_order, order = _REF_ORDER[key], ds.primitive_order()
    slot_of = np.empty(order.size, np.uint32)
    slot_of[order] = np.arange(order.size, dtype=np.uint32)
    if ds.builder == abi.BUILDER_REFERENCE:
        assert np.array_equal(order, ref_order)
    out = np.array(prim, np.uint32)
    hit = out != NONE
    out[hit] = slot_of[ref_order[out[hit]]]
    return out


def golden_records(ds, desc, g, name):
    return g["t"], in_slots(ds, desc, g["prim"], name), g["uv"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def expected(t, prim, uv, tmax):
    """The records under a bound: kept where the record is a hit with t < tmax (strictly), else the miss record."""
    tmax = np.broadcast_to(np.asarray(tmax, np.float32), t.shape)
    keep = (prim != NONE) & (t < tmax)
    return (np.where(keep, t, FLT_MAX).astype(np.float32), np.where(keep, prim, NONE).astype(np.uint32),
            np.where(keep[:, None], uv, np.float32(0)).astype(np.float32), keep.astype(np.uint8))


def run_closest(ds, rays_d, tmax=None, **kw):
    import torch
    t, prim, uv = ds.query(rays_d, tmax=tmax, kind="closest", **kw)
    torch.cuda.synchronize()
    assert t.dtype == torch.float32 and prim.dtype == torch.int32 and uv.dtype == torch.float32
    return t.cpu().numpy(), prim.cpu().numpy().view(np.uint32), uv.cpu().numpy()


def run_occluded(ds, rays_d, tmax=None, **kw):
    import torch
    occ = ds.query(rays_d, tmax=tmax, kind="occluded", **kw)
    torch.cuda.synchronize()
    assert occ.dtype == torch.uint8
    return occ.cpu().numpy()


def assert_records(got, want, what=""):
    (t, prim, uv), (et, eprim, euv) = got, want[:3]
    bad = np.flatnonzero((prim != eprim) | (bits(t) != bits(et)) | (bits(uv) != bits(euv)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {t.size} records differ, first at {bad[:5]}: got {t[bad[:5]]} {prim[bad[:5]]}, want {et[bad[:5]]} {eprim[bad[:5]]}"


def check_both(ds, rays_d, rec, tmax_np, tmax_arg, what):
    want = expected(*rec, tmax_np)
    assert_records(run_closest(ds, rays_d, tmax_arg), want, what + " closest")
    occ = run_occluded(ds, rays_d, tmax_arg)
    assert np.array_equal(occ, want[3]), f"{what} occluded: {(occ != want[3]).sum()} differ"


# ---- 1-3: the golden rays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", ["box", "cornell", "soup1k"])
def test_golden_closest_hits_unbounded(gpu, name, how):
    g, desc = golden(name)
    ds = make_scene(desc, how)
    rays_d = dev(g["rays"])
    rec = golden_records(ds, desc, g, name)
    for tmax in (None, float("inf"), float(FLT_MAX)):
        assert_records(run_closest(ds, rays_d, tmax), rec, f"{name} {how} tmax={tmax}")
    if how != "sah_unfinished":   # (exhaustive traversal: one ray per lane, closest hits only)
        assert_records(run_closest(ds, rays_d, None, traversal=abi.TRAVERSAL_EXHAUSTIVE), rec, f"{name} {how} exhaustive")
    occ = run_occluded(ds, rays_d, None)
    assert np.array_equal(occ, (g["prim"] != NONE).astype(np.uint8))
    ds.close()


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", ["box", "cornell", "soup1k"])
def test_one_tmax_for_all(gpu, name, how):
    g, desc = golden(name)
    t, prim = g["t"], g["prim"]
    hit = prim != NONE
    shares = np.array([(hit & (t < np.float32(0.9))).mean(), (hit & ~(t < np.float32(0.9))).mean(), (~hit).mean()])
    print(f"{name}: hit in range / hit beyond / miss = {shares}")
    assert (shares >= 0.10).all(), shares   # the test cannot pass on misses alone
    ds = make_scene(desc, how)
    check_both(ds, dev(g["rays"]), golden_records(ds, desc, g, name), np.float32(0.9), 0.9, f"{name} {how} tmax_all=0.9")
    ds.close()


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", ["box", "cornell", "soup1k"])
def test_the_boundary_per_ray(gpu, name, how):
    g, desc = golden(name)
    t, prim, uv = g["t"], g["prim"], g["uv"]
    hit = prim != NONE
    i = np.arange(t.size)
    tmax = np.where(hit, np.where(i % 2 == 0, t, np.nextafter(t, np.float32(np.inf), dtype=np.float32)), np.float32(1.0)).astype(np.float32)
    want = expected(t, prim, uv, tmax)
    # strict `<`: tmax = t is a miss, the next float above t is the golden record
    assert not want[3][hit & (i % 2 == 0)].any() and want[3][hit & (i % 2 == 1)].all() and not want[3][~hit].any()
    assert (hit & (i % 2 == 0)).sum() > 20 and (hit & (i % 2 == 1)).sum() > 20
    ds = make_scene(desc, how)
    rays_d = dev(g["rays"])
    prim = in_slots(ds, desc, prim, name)
    check_both(ds, rays_d, (t, prim, uv), tmax, dev(tmax), f"{name} {how} per-ray boundary")
    # single rays: the first golden hit under the special bounds
    k = int(np.flatnonzero(hit)[0])
    one = dev(g["rays"][k:k + 1])
    rec1 = (t[k:k + 1], prim[k:k + 1], uv[k:k + 1])
    for special, is_hit in ((float("nan"), False), (0.0, False), (-1.0, False), (float("inf"), True), (float(FLT_MAX), True)):
        want1 = expected(*rec1, np.float32(np.inf)) if is_hit else expected(*rec1, np.float32(0.0))
        for arg in (special, dev(np.array([special], np.float32))):
            assert_records(run_closest(ds, one, arg), want1, f"{name} {how} tmax={special}")
            assert run_occluded(ds, one, arg)[0] == int(is_hit), f"{name} {how} tmax={special}"
    ds.close()


# ---- 4: spheres --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOW)
def test_spheres(gpu, how):
    from rayca_amd import model as M, sdtf
    scene = M.Scene()
    sdtf.push_sdtf_from_path(scene, os.path.join(G, "spheres.sdtf"))
    desc = flatten(scene)
    orc = ol.OracleScene(desc, Config())
    n = 640
    i = np.arange(n)
    d = np.stack([scenes.hash_unit(11 + a, i) * 2 - 1 for a in range(3)], 1).astype(np.float32)
    d[np.abs(d).sum(1) == 0] = 1.0
    o = np.stack([(scenes.hash_unit(21 + a, i) * 2 - 1) * np.float32(3.0) for a in range(3)], 1).astype(np.float32)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    ot, oprim, ouv, _ = orc.trace_rays(rays)
    hit = oprim != NONE
    assert hit.sum() >= 64 and (~hit).sum() >= 64, hit.mean()
    ds = make_scene(desc, how)
    rays_d = dev(rays)
    rec = (ot, in_slots(ds, desc, oprim, "spheres"), ouv)
    check_both(ds, rays_d, rec, np.float32(np.inf), None, f"spheres {how} unbounded")
    med = np.float32(np.median(ot[hit]))
    assert (ot[hit] < med).sum() >= 16 and (ot[hit] >= med).sum() >= 16
    check_both(ds, rays_d, rec, med, float(med), f"spheres {how} tmax=median")
    ds.close()
    orc.close()


# ---- 5: a large incoherent batch ---------------------------------------------------------------------------------------
N_BIG = 2 ** 20 + 37


def atrium_rays(n, seed=0):
    i = np.arange(n)
    lo, hi = np.array([-14.0, 0.3, -5.2], np.float32), np.array([14.0, 9.0, 5.2], np.float32)   # inside the hall (30 x 10 x 12)
    o = np.stack([lo[a] + scenes.hash_unit(seed + 101 + a, i) * (hi[a] - lo[a]) for a in range(3)], 1).astype(np.float32)
    z = scenes.hash_unit(seed + 111, i) * 2 - 1
    phi = scenes.hash_unit(seed + 112, i) * np.float32(2 * np.pi)
    r = np.sqrt(np.maximum(0, 1 - z * z))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return np.concatenate([o, d], 1).astype(np.float32)


@pytest.fixture(scope="module")
def atrium_desc():
    return flatten(scenes.atrium_scene())


@pytest.fixture(scope="module")
def atrium_sah(gpu, atrium_desc):
    ds = DeviceScene(atrium_desc, Config(), builder=abi.BUILDER_SAH)
    ds.finish()
    yield ds
    ds.close()


@pytest.mark.parametrize("how", HOW)
def test_large_incoherent_batch(gpu, atrium_desc, how):
    rays = atrium_rays(N_BIG)
    ds = make_scene(atrium_desc, how)
    rays_d = dev(rays)
    # the query first: on "sah_unfinished" it may run before the formats thread has finished (trace_rays waits for it)
    got = run_closest(ds, rays_d, None)
    t, prim, uv, _ = ds.trace_rays(rays)
    rec = (t, prim, uv)
    assert_records(got, rec, f"atrium {how} unbounded vs trace_rays")
    hit = prim != NONE
    half = (scenes.hash_u32(7, np.arange(N_BIG)) & 1).astype(bool)
    tmax = np.where(hit, t * np.where(half, np.float32(0.5), np.float32(2.0)), np.float32(1.0)).astype(np.float32)
    in_range, beyond = (hit & (t < tmax)).sum(), (hit & ~(t < tmax)).sum()
    print(f"atrium {how}: hits {hit.mean():.3f}, in range {in_range / hit.sum():.3f}, beyond {beyond / hit.sum():.3f}")
    assert hit.mean() >= 0.10 and in_range >= 0.25 * hit.sum() and beyond >= 0.25 * hit.sum()
    check_both(ds, rays_d, rec, tmax, dev(tmax), f"atrium {how} per-ray tmax")
    if how == "sah":
        sub = (scenes.hash_u32(9, np.arange(4096)) % np.uint32(N_BIG)).astype(np.int64)
        orc = ol.OracleScene(atrium_desc, Config())
        _REF_ORDER["atrium"] = orc.primitive_order()
        ot, oprim, ouv, _ = orc.trace_rays(rays[sub])
        assert_records((got[0][sub], got[1][sub], got[2][sub]), (ot, in_slots(ds, atrium_desc, oprim, "atrium"), ouv), "atrium 4096-ray subsample vs the oracle")
        orc.close()
    ds.close()


# ---- 6: asynchrony, contexts, guards -----------------------------------------------------------------------------------
def test_four_contexts_back_to_back(atrium_sah):
    import torch
    ds = atrium_sah
    n = 200_003
    batches = [dev(atrium_rays(n, seed=1000 * (k + 1))) for k in range(4)]
    tm = [None, 3.0, dev(np.full(n, 2.0, np.float32)), 5.0]
    solo = []
    for k in range(4):
        solo.append(run_closest(ds, batches[k], tm[k]) if k % 2 == 0 else run_occluded(ds, batches[k], tm[k]))
    streams = [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    res = []
    for k in range(4):
        res.append(ds.query(batches[k], tmax=tm[k], kind="closest" if k % 2 == 0 else "occluded", stream=streams[k], context=k))
    torch.cuda.synchronize()
    for k in range(4):
        if k % 2 == 0:
            got = (res[k][0].cpu().numpy(), res[k][1].cpu().numpy().view(np.uint32), res[k][2].cpu().numpy())
            assert_records(got, solo[k], f"context {k}")
        else:
            assert np.array_equal(res[k].cpu().numpy(), solo[k]), f"context {k}"
            assert 0 < solo[k].sum() < n


def test_query_beside_a_frame_in_flight(atrium_sah):
    import torch
    ds = atrium_sah
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, max_depth=3)
    W, H = 1920, 1080
    rays_d = dev(atrium_rays(300_001, seed=77))
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    frame_solo = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    frame = torch.zeros_like(frame_solo)
    torch.cuda.synchronize()
    for _ in range(20):   # (past the scene's format calibration: all formats give the same bits, this keeps the two frames alike anyway)
        ds.render_device(cfg, W, H, frame_solo.data_ptr(), stream=s0.cuda_stream, context=0)
    torch.cuda.synchronize()
    solo = run_closest(ds, rays_d, 4.0, stream=s1, context=1)
    ds.render_device(cfg, W, H, frame.data_ptr(), stream=s0.cuda_stream, context=0)
    t, prim, uv = ds.query(rays_d, tmax=4.0, stream=s1, context=1)
    torch.cuda.synchronize()
    assert torch.equal(frame, frame_solo) and int(frame.max()) > 0
    assert_records((t.cpu().numpy(), prim.cpu().numpy().view(np.uint32), uv.cpu().numpy()), solo, "query beside a frame")


@pytest.mark.parametrize("how", ["reference", "sah"])
def test_guards_around_the_outputs_stay_intact(gpu, how):
    import torch
    g, desc = golden("soup1k")
    ds = make_scene(desc, how)
    n = g["rays"].shape[0] - 5   # (not a multiple of 64)
    rays_d = dev(g["rays"][:n])
    big_t = torch.full((n + 128,), -7.0, dtype=torch.float32, device="cuda")
    big_p = torch.full((n + 128,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    big_uv = torch.full((n + 128, 2), -7.0, dtype=torch.float32, device="cuda")
    big_o = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    out = (big_t[64:-64], big_p[64:-64], big_uv[64:-64])
    r = ds.query(rays_d, tmax=0.9, out=out)
    o = ds.query(rays_d, tmax=0.9, kind="occluded", out=big_o[64:-64])
    torch.cuda.synchronize()
    assert r[0].data_ptr() == out[0].data_ptr() and o.data_ptr() == big_o[64:-64].data_ptr()
    want = expected(g["t"][:n], in_slots(ds, desc, g["prim"][:n], "soup1k"), g["uv"][:n], np.float32(0.9))
    assert_records((r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32), r[2].cpu().numpy()), want, "guarded outputs")
    assert np.array_equal(o.cpu().numpy(), want[3])
    for big, sentinel in ((big_t, -7.0), (big_p, 0x5A5A5A5A), (big_uv, -7.0), (big_o, 0xA5)):
        assert bool((big[:64] == sentinel).all()) and bool((big[-64:] == sentinel).all())
    # only some of the closest-hit outputs: the others are not touched
    big_t.fill_(-7.0)
    big_p.fill_(0x5A5A5A5A)
    q = abi.RaycaQuery()
    q.kind, q.count, q.rays, q.tmax_all, q.prim_out = abi.QUERY_CLOSEST, n, rays_d.data_ptr(), 0.9, big_p[64:-64].data_ptr()
    o2 = ds._opts(abi.TRAVERSAL_ORDERED, False, None, None)
    lib.check(gpu.rayca_hip_query_device(ds.handle, C.byref(o2), C.byref(q), None))   # (no stream: the call waits)
    assert np.array_equal(big_p[64:-64].cpu().numpy().view(np.uint32), want[1]) and bool((big_t == -7.0).all())
    ds.close()


# ---- 7: statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "sah"])
def test_statistics(gpu, how):
    g, desc = golden("soup1k")
    ds = make_scene(desc, how)
    rays_d = dev(g["rays"])
    n = g["rays"].shape[0]
    *_, st_c = ds.query(rays_d, tmax=0.9, collect_stats=True)
    _, st_o = ds.query(rays_d, tmax=0.9, kind="occluded", collect_stats=True)
    *_, st_u = ds.query(rays_d, collect_stats=True)
    *_, st_plain = ds.query(rays_d, tmax=0.9, want_stats=True)
    assert (st_c["rays_primary"], st_c["rays_shadow"]) == (n, 0) and (st_o["rays_primary"], st_o["rays_shadow"]) == (0, n)
    for st in (st_c, st_o, st_u, st_plain):
        assert st["kernel_launches"] >= 1 and st["kernel_ms"] > 0
        assert st["class_launches"][abi.KERNEL_OTHER] == st["kernel_launches"] and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]
    assert st_plain["boxes_tested"] == 0 and st_c["boxes_tested"] > 0
    print({k: (st_o[k], st_c[k], st_u[k]) for k in ("boxes_tested", "triangles_tested")})
    # a ray's ordered search under a bound is a subset of its unbounded search, and OCCLUDED's ends earlier still
    for k in ("boxes_tested", "triangles_tested"):
        assert st_o[k] <= st_c[k], k
        assert st_o[k] < st_u[k], k
    ds.close()


# ---- 8: errors ---------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    import torch
    g, desc = golden("box")
    ds = make_scene(desc, "sah")
    n = 64
    rays_d = dev(g["rays"][:n])
    t = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    occ = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(kind=abi.QUERY_CLOSEST, count=n, reserved=0, t_out=True, occ_out=False, context=0, traversal=abi.TRAVERSAL_ORDERED, engine=0, rays=True):
        q = abi.RaycaQuery()
        q.kind, q.count, q.reserved, q.tmax_all = kind, count, reserved, float("inf")
        q.rays = rays_d.data_ptr() if rays else None
        q.t_out = t.data_ptr() if t_out else None
        q.occluded_out = occ.data_ptr() if occ_out else None
        o = ds._opts(traversal, False, None, None, engine=engine, context=context)
        return gpu.rayca_hip_query_device(ds.handle, C.byref(o), C.byref(q), None)

    assert call(kind=2) == abi.ERR_BAD_ARG and "kind" in lib.last_error()
    assert call(reserved=1) == abi.ERR_BAD_ARG and "reserved" in lib.last_error()
    assert call(t_out=False) == abi.ERR_BAD_ARG and "output" in lib.last_error()
    assert call(kind=abi.QUERY_OCCLUDED, t_out=True, occ_out=False) == abi.ERR_BAD_ARG   # (t_out is not OCCLUDED's output)
    assert call(rays=False) == abi.ERR_BAD_ARG
    assert call(context=8) == abi.ERR_BAD_ARG and "context" in lib.last_error()
    assert call(engine=abi.ENGINE_WAVEFRONT) == abi.ERR_BAD_ARG
    assert call(kind=abi.QUERY_OCCLUDED, occ_out=True, traversal=abi.TRAVERSAL_EXHAUSTIVE) == abi.ERR_UNSUPPORTED
    assert call(count=0) == abi.OK and call(kind=abi.QUERY_OCCLUDED, occ_out=True, count=0) == abi.OK
    torch.cuda.synchronize()
    assert bool((t == -7.0).all()) and bool((occ == 0xA5).all())   # nothing of the above wrote anything
    assert call() == abi.OK and call(kind=abi.QUERY_OCCLUDED, occ_out=True) == abi.OK
    assert bool((t != -7.0).all()) and bool((occ != 0xA5).all())
    # the wrapper's own checks, before the native call
    with pytest.raises(ValueError):
        ds.query(rays_d.cpu())                                   # wrong device
    with pytest.raises(TypeError):
        ds.query(rays_d.double())                                # wrong dtype
    with pytest.raises(ValueError):
        ds.query(rays_d.reshape(-1, 3))                          # wrong shape
    with pytest.raises(ValueError):
        ds.query(rays_d, tmax=torch.ones(n + 1, device="cuda"))  # tmax of another length
    with pytest.raises(TypeError):
        ds.query(rays_d, tmax=torch.ones(n, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ds.query(rays_d, kind="nearest")
    with pytest.raises(TypeError):
        ds.query(rays_d, kind="occluded", out=torch.zeros(n, device="cuda"))   # the mask is uint8
    with pytest.raises(TypeError):
        ds.query(g["rays"][:n])                                  # numpy: host memory
    empty = ds.query(rays_d[:0])
    assert empty[0].shape == (0,) and empty[2].shape == (0, 2)
    # a strided input is made contiguous, nothing else is copied
    wide = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    wide[:, :6] = rays_d
    a = run_closest(ds, wide[:, :6], 0.9)
    assert_records(a, expected(g["t"][:n], in_slots(ds, desc, g["prim"][:n], "box"), g["uv"][:n], np.float32(0.9)), "strided rays")
    ds.close()
    with pytest.raises(RaycaError):
        DeviceScene(flatten(scenes.box_scene()), Config()).query(rays_d, context=9)
