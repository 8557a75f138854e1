"""The counting instantiations (RaycaRenderOptions.collect_stats) of every kernel family, next to the production ones: statistics
never change a result.  For each traversal a scene can be asked for -- ordered and exhaustive, on both builders, with and without
spheres -- the frame, the hit records and the query results with collect_stats are, bit for bit, those without, which
test_gpu_parity.py, test_gpu_engines.py and test_gpu_query.py check against the oracle; and the two generation engines agree with
and without the counters.  This reaches, with statistics on AND off at one shape, the flavours kTravExact / kTravExactAll
(RAYCA_BUILDER_REFERENCE) and kTravFast / kTravFastWide / kTravFastAll (RAYCA_BUILDER_SAH) of k_generation, k_trace_rays and
k_query_rays, k_wf_trace / k_wf_shadow / k_queue_refill / k_shadow_refill / k_query_refill / k_flat_refill and k_general.

test_gpu_launch_counts.py's shape: test_gpu_general.py's scenes, 61 x 35 pixels, batches of 37 and 2135 rays."""
import numpy as np
import pytest

import test_gpu_general as G
from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi, flatten

pytestmark = pytest.mark.gpu
I = IntegratorStrategy
W, H = 61, 35
ONE = Config(samples_per_pixel=1)
NAMES, HOW = ["cornell", "sphere_boxes"], ["reference", "sah"]
TRAVERSALS = [abi.TRAVERSAL_ORDERED, abi.TRAVERSAL_EXHAUSTIVE]
_SCENES = {}


def scene(name, how):
    if (name, how) not in _SCENES:
        ds = DeviceScene(flatten(G.SCENES[name]()), Config(), builder=abi.BUILDER_SAH if how == "sah" else abi.BUILDER_REFERENCE)
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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_frame(a, b, what):
    assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[0], b[0]), what


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", NAMES)
def test_frames_with_and_without_statistics(gpu, name, how):
    ds = scene(name, how)
    for cfg in (Config(integrator=I.Flat), Config(max_depth=2, seed=3), Config(integrator=I.Flat, samples_per_pixel=4)):
        for trav in TRAVERSALS:
            plain = ds.render(cfg, W, H, traversal=trav, engine=abi.ENGINE_FUSED)
            assert float(plain[1][..., :3].max()) > 0.0
            counted = ds.render(cfg, W, H, traversal=trav, engine=abi.ENGINE_FUSED, collect_stats=True)
            same_frame(plain, counted, f"{name} {how} fused traversal {trav}")
            assert counted[2]["boxes_tested"] > 0
            if trav == abi.TRAVERSAL_ORDERED:   # (the wavefront engine has no exhaustive form)
                for stats in (False, True):
                    same_frame(plain, ds.render(cfg, W, H, engine=abi.ENGINE_WAVEFRONT, collect_stats=stats), f"{name} {how} wavefront stats {stats}")
                if how == "sah" and cfg.samples_per_pixel == 1 and cfg.integrator == I.Flat:
                    for stats in (False, True):
                        same_frame(plain, ds.render(cfg, W, H, camera_rays=abi.CAMERA_REFILL, collect_stats=stats), f"{name} lane refill stats {stats}")
    # the per-pixel stack machine
    cfg = Config(integrator=I.Raytracer, max_depth=2)
    same_frame(ds.render(cfg, W, H), ds.render(cfg, W, H, collect_stats=True), f"{name} {how} stack machine")


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("count", [37, W * H])
def test_ray_batches_with_and_without_statistics(gpu, count, name, how):
    ds = scene(name, how)
    rays_d = ds.camera_rays(ONE, W, H)[:count].contiguous()
    rays = rays_d.cpu().numpy()
    for trav in TRAVERSALS:
        t, prim, uv, _ = ds.trace_rays(rays, traversal=trav)
        ct, cprim, cuv, st = ds.trace_rays(rays, traversal=trav, collect_stats=True)
        assert np.array_equal(bits(t), bits(ct)) and np.array_equal(prim, cprim) and np.array_equal(bits(uv), bits(cuv)), f"trace_rays traversal {trav}"
        assert st["boxes_tested"] > 0 and (prim != np.uint32(0xFFFFFFFF)).any()
        qt, qprim, quv = ds.query(rays_d, traversal=trav)
        ct, cprim, cuv, st = ds.query(rays_d, traversal=trav, collect_stats=True)
        assert np.array_equal(bits(qt.cpu().numpy()), bits(ct.cpu().numpy())) and np.array_equal(qprim.cpu().numpy(), cprim.cpu().numpy())
        assert np.array_equal(bits(quv.cpu().numpy()), bits(cuv.cpu().numpy())), f"query traversal {trav}"
        assert st["boxes_tested"] > 0
    occ = ds.query(rays_d, kind="occluded", tmax=1e3)
    cocc, st = ds.query(rays_d, kind="occluded", tmax=1e3, collect_stats=True)
    assert np.array_equal(occ.cpu().numpy(), cocc.cpu().numpy()) and st["boxes_tested"] > 0 and occ.any()
