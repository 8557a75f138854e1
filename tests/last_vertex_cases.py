"""Cases of test_gpu_last_vertex.py (helper module, and the program its child process runs).

k_generation has a last-vertex form (kernels.hip LAST; select.inc last_form): the generation behind which no vertex samples a
bounce runs a kernel without the bounce code, which writes the records the general form writes for such a vertex.  The host
chooses it from the Config; RAYCA_LAST_FORM=0 in the environment (read once per process) keeps every generation on the general
form.  Neither may change a pixel or a counter.  The scenes are test_gpu_general.py's -- the Cornell room (a point light), the
room lit by a quad light, the spheres among boxes (the SPH instantiations) -- at 61 x 35 pixels, one ragged tile column and row,
under both builders.

python tests/last_vertex_cases.py OUT.npz: the fused engine's frames, counters and RaycaStats.node_format of the cases, with the
knobs of the environment."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from rayca_amd import Config, SamplerStrategy   # noqa: E402

COUNTER_KEYS = ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded", "boxes_tested", "triangles_tested")
RAY_COUNTERS = 4   # the first four count rays and shaded hits; the last two are each engine's own traversal
W, H = 61, 35
BUILDERS = ("reference", "sah")

# name -> (scene of test_gpu_general.SCENES, Config).  Where a path bounces the generation kernels take one light sample
# (select.inc generation_kernels_gap), so two light samples go with max_depth 1.
CASES = {}
for _d in (1, 2, 3):
    for _s in (1, 4):
        CASES[f"cornell_d{_d}_s{_s}"] = ("cornell", Config(max_depth=_d, samples_per_pixel=_s, seed=30 + 4 * _d + _s))
CASES["cornell_two_light_samples"] = ("cornell", Config(max_depth=1, light_samples=2, seed=7))
CASES["quad_d1"] = ("room_phong", Config(max_depth=1, seed=51))
CASES["quad_d1_two_light_samples"] = ("room_phong", Config(max_depth=1, light_samples=2, seed=52))
CASES["quad_d3"] = ("room_phong", Config(max_depth=3, seed=53))
CASES["spheres_d1"] = ("sphere_boxes", Config(max_depth=1, seed=61))
CASES["spheres_d3"] = ("sphere_boxes", Config(max_depth=3, seed=63))
CASES["no_direct_d1"] = ("room_phong", Config(max_depth=1, direct_sampler=SamplerStrategy.NONE, seed=71))
CASES["no_direct_d3"] = ("room_phong", Config(max_depth=3, direct_sampler=SamplerStrategy.NONE, seed=73))


def last_generations(cfg):
    """the generations of a frame that run the last-vertex form, a bit each: the host's rule restated"""
    if cfg.direct_sampler == SamplerStrategy.NONE:
        return 0
    return 1 << (cfg.max_depth - 1)


def keys():
    return [f"{name}/{b}" for name in CASES for b in BUILDERS]


def render_cases(engine=None):
    """{"<case>/<builder>/u8|f32|counters|forms": array}: production frames, the six counters of the counting instantiation, and
    bits 16-31 of RaycaStats.node_format of the two frames (generation g on the last-vertex form: bit g)"""
    import test_gpu_general as G
    from rayca_amd import DeviceScene, abi, flatten
    engine = abi.ENGINE_FUSED if engine is None else engine
    out = {}
    for scene in sorted({s for s, _ in CASES.values()}):
        desc = flatten(G.SCENES[scene]())
        for b in BUILDERS:
            ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH) if b == "sah" else DeviceScene(desc, Config())
            if b == "sah":
                ds.finish()
            for name, (s, cfg) in CASES.items():
                if s != scene:
                    continue
                u8, f32, st0 = ds.render(cfg, W, H, engine=engine)
                st = ds.render(cfg, W, H, collect_stats=True, engine=engine)[2]
                key = f"{name}/{b}"
                out[key + "/u8"], out[key + "/f32"] = u8, f32
                out[key + "/counters"] = np.array([int(st[k]) for k in COUNTER_KEYS], np.uint64)
                out[key + "/forms"] = np.array([int(st0["node_format"]) >> 16, int(st["node_format"]) >> 16], np.uint32)
            ds.close()
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **render_cases())
    print("wrote", sys.argv[1], "RAYCA_LAST_FORM =", os.environ.get("RAYCA_LAST_FORM"))
