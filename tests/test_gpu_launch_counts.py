"""The launch sequence of a frame and of a radiance query, as RaycaStats counts it: kernel_launches, trace_kernel_launches and the
per-class counts, for every driver path (fused and wavefront engine, the stack machine, caller-supplied rays).

S = samples per pixel, D = max_depth, L = 1 when NEE has at least one light sample (shadow rays are traced), else 0:

    Flat frame, ENGINE_FUSED, S = 1        1 launch (the generation kernel writes the pixel), 1 of them traversal
    Flat frame, ENGINE_FUSED, S = 4        per sample k_generation + k_resolve: 8, 4
    Flat frame, ENGINE_WAVEFRONT, S = 1    trace + shade: 2, 1
    Path frame, ENGINE_FUSED               per sample D generations + k_resolve: S (D + 1), S D
    Path frame, ENGINE_WAVEFRONT           per generation trace + shade (+ shadow): S (D (2 + L) + 1), S D (1 + L)
    stack-machine frame                    per sample k_general + k_resolve, all under KERNEL_OTHER: 2 S, S
    radiance, Flat                         enqueue + trace + shade: 3, 1; the enqueue is the one launch under KERNEL_OTHER
    radiance, Path                         [D > 0] + D (2 + L) + 1, D (1 + L); under KERNEL_OTHER the enqueue (D > 0 only: a
                                           max_depth = 0 query has no generation to feed and launches k_resolve alone) and k_resolve

Small scenes (test_gpu_general.py's), both builders, SAH scenes after finish(); frames of 61 x 35 pixels (ragged, more than one
block, far below the 65536 pixels at which a scene starts timing its node formats), batches of 37 rays (fewer than a wave) and of
a whole frame's 2135."""
import os

import pytest

import test_gpu_general as G
from rayca_amd import Config, DeviceScene, IntegratorStrategy, SamplerStrategy, abi, flatten

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(v in os.environ for v in ("RAYCA_WF_REFILL", "RAYCA_WF_SHADOW_REFILL", "RAYCA_REFILL", "RAYCA_WAVEFRONT",
                                                               "RAYCA_NODE_FORMAT", "RAYCA_WIDE")),
                                 reason="an engine or node-format override is set: the launch sequence is pinned for the defaults")]
I, S = IntegratorStrategy, SamplerStrategy
W, H = 61, 35
ONE = Config(samples_per_pixel=1)
HOW = ["reference", "sah"]
# (scene, what the case sets of the Config beside depth and samples, L)
LIT = [("cornell", dict(seed=3), 1),                                # a point light under NEE
       ("room_phong", dict(direct_sampler=S.NONE, seed=4), 0)]      # NEE off: no shadow rays
DEPTHS, SAMPLES = (0, 1, 3), (1, 4)
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


def check(st, launches, trace, what, other=None):
    print(what, "kernel_launches", st["kernel_launches"], "trace_kernel_launches", st["trace_kernel_launches"], "class_launches", st["class_launches"])
    assert st["kernel_launches"] == launches, what
    assert st["trace_kernel_launches"] == trace, what
    assert sum(st["class_launches"]) == st["kernel_launches"], what
    if other is not None:
        assert st["class_launches"][abi.KERNEL_OTHER] == other, what


def frame(ds, cfg, engine):
    return ds.render(cfg, W, H, engine=engine, collect_stats=True, want_rgba8=False)[2]


@pytest.mark.parametrize("how", HOW)
def test_flat_frames(gpu, how):
    ds, flat = scene("cornell", how), Config(integrator=I.Flat)
    check(frame(ds, flat, abi.ENGINE_FUSED), 1, 1, "fused, S = 1")
    check(frame(ds, Config(integrator=I.Flat, samples_per_pixel=4), abi.ENGINE_FUSED), 8, 4, "fused, S = 4")
    check(frame(ds, flat, abi.ENGINE_WAVEFRONT), 2, 1, "wavefront, S = 1")


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("lit", range(len(LIT)))
def test_path_frames(gpu, lit, how):
    name, kw, L = LIT[lit]
    ds = scene(name, how)
    for D in DEPTHS:
        for spp in SAMPLES:
            cfg = Config(max_depth=D, samples_per_pixel=spp, **kw)
            check(frame(ds, cfg, abi.ENGINE_FUSED), spp * (D + 1), spp * D, f"{name} fused D = {D} S = {spp}")
            check(frame(ds, cfg, abi.ENGINE_WAVEFRONT), spp * (D * (2 + L) + 1), spp * D * (1 + L), f"{name} wavefront D = {D} S = {spp}")


@pytest.mark.parametrize("how", HOW)
def test_stack_machine_frames(gpu, how):
    ds = scene("cornell", how)
    for spp in SAMPLES:
        st = frame(ds, Config(integrator=I.Raytracer, max_depth=2, samples_per_pixel=spp), abi.ENGINE_AUTO)
        check(st, 2 * spp, spp, f"Raytracer S = {spp}", other=2 * spp)


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("count", [37, W * H])
def test_radiance(gpu, count, how):
    import torch
    for name, kw, L in LIT:
        ds = scene(name, how)
        rays = ds.camera_rays(ONE, W, H)[:count].contiguous()
        _, st = ds.radiance(rays, Config(integrator=I.Flat), collect_stats=True)
        check(st, 3, 1, f"{name} radiance Flat, {count} rays", other=1)
        for D in DEPTHS:
            _, st = ds.radiance(rays, Config(max_depth=D, **kw), collect_stats=True)
            fed = 1 if D > 0 else 0
            check(st, fed + D * (2 + L) + 1, D * (1 + L), f"{name} radiance D = {D}, {count} rays", other=fed + 1)
    torch.cuda.synchronize()
