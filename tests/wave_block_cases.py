"""Cases of test_gpu_wave_blocks.py (helper module, and the program its child processes run).

k_generation runs as one-wave workgroups (trace_core.inc kGenBlock): the rows of the per-lane node stack, the spill column and the
parked ShadeCtx are strided by the workgroup's 64 threads, and the persistent grid is counted in waves (select.inc grid_policy).
Its cold arguments are read from the kernel-argument segment
where they are used (kernels.hip GEN_COLD).  None of that may change a pixel, a ray count or a traversal counter.  The frames here are small on purpose -- one tile, fewer
tiles than the grid has waves, ragged right and bottom tiles -- and cover what the fused engine's generation kernel does beyond the
camera ray: bounce generations (push_ray), a Flat frame, two light samples, a sphere slot, and the deep scene of
node_step_cases.py, which crosses the LDS part of the stack when a process caps it at four entries (RAYCA_PATH_LDS_ENTRIES=4).

python tests/wave_block_cases.py OUT.npz [case ...]: the fused engine's frames and counters of the cases, with the library
RAYCA_HIP_LIB names and the knobs of the environment (both are read once per process)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import leaf_shade_cases as L   # noqa: E402
import node_step_cases as N   # noqa: E402
from rayca_amd import Config, IntegratorStrategy   # noqa: E402

COUNTER_KEYS = L.COUNTER_KEYS
RAY_COUNTERS = 4   # the first four of COUNTER_KEYS count rays and shaded hits; the last two are the traversal's own
SIZES = ((8, 8), (24, 16), (67, 45))   # one tile; six tiles, fewer than a CU's waves; 9 x 6 tiles, the last column and row ragged
FLAT = Config(integrator=IntegratorStrategy.Flat)

# name -> (scene of node_step_cases.SPILL_SCENES, width, height, Config)
CASES = {}
for _w, _h in SIZES:
    for _d in (1, 3):
        CASES[f"cornell_{_w}x{_h}_d{_d}"] = ("cornell", _w, _h, Config(max_depth=_d, seed=40 + _d))
CASES["cornell_flat"] = ("cornell", 67, 45, FLAT)
CASES["cornell_two_light_samples"] = ("cornell", 24, 16, Config(max_depth=1, light_samples=2, seed=7))
CASES["spheres_d3"] = ("spheres", 67, 45, Config(max_depth=3, seed=5))
CASES["deep_d1"] = ("deep_soup", 64, 64, Config(max_depth=1, seed=18))
CASES["deep_d3"] = ("deep_soup", 64, 64, Config(max_depth=3, seed=20))
DEEP = ("deep_d1", "deep_d3")
SPILL_ENTRIES = N.SPILL_ENTRIES


def render_cases(names=None, engine=None):
    """{"<case>/u8|f32|counters": array}: production frames and the six counters of the counting instantiation"""
    from rayca_amd import DeviceScene, abi
    engine = abi.ENGINE_FUSED if engine is None else engine
    out, scenes = {}, {}
    for name in names or list(CASES):
        scene, w, h, cfg = CASES[name]
        if scene not in scenes:
            scenes[scene] = DeviceScene(N.frame_desc(scene), Config(), builder=abi.BUILDER_SAH)
            scenes[scene].finish()
        ds = scenes[scene]
        kw = dict(engine=engine, camera_rays=abi.CAMERA_GENERATION if engine == abi.ENGINE_FUSED else abi.CAMERA_AUTO)
        u8, f32, _ = ds.render(cfg, w, h, **kw)
        st = ds.render(cfg, w, h, collect_stats=True, **kw)[2]
        out[name + "/u8"], out[name + "/f32"] = u8, f32
        out[name + "/counters"] = np.array([int(st[k]) for k in COUNTER_KEYS], np.uint64)
    for ds in scenes.values():
        ds.close()
    return out


if __name__ == "__main__":
    from rayca_amd import lib
    np.savez(sys.argv[1], **render_cases(sys.argv[2:] or None))
    print("wrote", sys.argv[1], "library =", os.path.realpath(lib.LIB_PATH), "RAYCA_PATH_LDS_ENTRIES =", os.environ.get("RAYCA_PATH_LDS_ENTRIES"))
