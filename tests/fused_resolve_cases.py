"""Cases of test_gpu_fused_resolve.py (helper module, and the program its child process runs).

The one-sample depth-1 path frame of the fused engine is one launch: k_generation's FUSED form with GEN0 && LAST (kernels.hip;
select.inc fuse_resolve, pick_kernel; api.inc frame_begin, fused_generation) writes the pixel itself -- no record, no k_resolve.
RAYCA_FUSE_RESOLVE=0 in the environment (read once per process; RAYCA_LAST_FORM=0 implies it) keeps generation + k_resolve.
Neither may change a pixel or a counter.  The scenes are test_gpu_general.py's at 61 x 35 pixels, one ragged tile column and row,
under both builders.  Which lanes end how was established with the CPU oracle on these very frames (python
tests/fused_resolve_cases.py --kinds prints the counts): the Cornell room has lit vertices whose light is visible and ones in
shadow (pixels above zero and pixels of +0.0 behind a hit), the quad-light room shows its emitter to the camera (emissive first
hits: pixels of the emission colour), the glTF box and the spheres stand in front of the sky (misses: pixels of +0.0).  In numbers,
of the 2135 camera rays: Cornell room 945 misses, 1047 lit vertices that see the light and 143 in shadow (every one a +0.0 pixel);
quad-light room 981 misses and 23 pixels of the emission colour (1, 1, 1); glTF box 1979 misses; spheres 1010.

python tests/fused_resolve_cases.py OUT.npz: the fused engine's frames, ray counters and RaycaStats of the cases, with the knobs
of the environment."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from rayca_amd import Config, SamplerStrategy   # noqa: E402

W, H = 61, 35
BUILDERS = ("reference", "sah")
FUSED_BIT = 8192   # RaycaStats.node_format bit 13: the path frame's generation kernel wrote the pixel
COUNTER_KEYS = ("rays_primary", "rays_shadow", "rays_bounce", "hits_shaded")

# name -> (scene of test_gpu_general.SCENES, Config, keyword arguments of DeviceScene.render).  These are the frames the form is
# picked for: one launch each.
CASES = {
    "cornell": ("cornell", Config(max_depth=1, seed=81), {}),
    "cornell_two_light_samples": ("cornell", Config(max_depth=1, light_samples=2, seed=82), {}),
    "cornell_gamma": ("cornell", Config(max_depth=1, gamma=2.2, seed=83), {}),
    "cornell_rgba8_only": ("cornell", Config(max_depth=1, gamma=2.2, seed=84), dict(want_f32=False)),
    "cornell_rgba32f_only": ("cornell", Config(max_depth=1, gamma=2.2, seed=85), dict(want_rgba8=False)),
    # part 2 of 3 in bands of 4 rows: bands 2, 5 and 8 of the 35 rows, the last one ragged (3 rows)
    "cornell_tiled": ("cornell", Config(max_depth=1, seed=86), dict(tile=(2, 3, 4))),
    "quad": ("room_phong", Config(max_depth=1, seed=87), {}),
    "quad_gamma_two_light_samples": ("room_phong", Config(max_depth=1, light_samples=2, gamma=2.2, seed=88), {}),
    "sky": ("box", Config(max_depth=1, seed=89), {}),
    "sky_gamma": ("box", Config(max_depth=1, gamma=2.2, seed=90), {}),
    "spheres": ("sphere_boxes", Config(max_depth=1, seed=91), {}),
}
# Frames that keep their launch sequence: name -> (scene, Config, engine name, launches of the production frame).  A fused-engine
# path frame is S (D + 1) launches (test_gpu_launch_counts.py), a wavefront one S (D (2 + L) + 1).
OFF = {
    "four_samples": ("cornell", Config(max_depth=1, samples_per_pixel=4, seed=92), "FUSED", 8),
    "depth_2": ("cornell", Config(max_depth=2, seed=93), "FUSED", 3),
    "depth_3": ("cornell", Config(max_depth=3, seed=94), "FUSED", 4),
    "no_direct_sampler": ("room_phong", Config(max_depth=1, direct_sampler=SamplerStrategy.NONE, seed=95), "FUSED", 2),
    "wavefront": ("cornell", Config(max_depth=1, seed=96), "WAVEFRONT", 4),
}


def keys():
    return [f"{name}/{b}" for name in CASES for b in BUILDERS]


def off_keys():
    return [f"{name}/{b}" for name in OFF for b in BUILDERS]


def scenes_of(builder, names=None):
    """{scene name: DeviceScene} of `names`, by default every scene the cases use (the caller closes them)"""
    import test_gpu_general as G
    from rayca_amd import DeviceScene, abi, flatten
    out = {}
    for scene in sorted({c[0] for c in CASES.values()} | {c[0] for c in OFF.values()} if names is None else names):
        desc = flatten(G.SCENES[scene]())
        out[scene] = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH) if builder == "sah" else DeviceScene(desc, Config())
        if builder == "sah":
            out[scene].finish()
    return out


def put(out, key, frame):
    u8, f32, st = frame
    if u8 is not None:
        out[key + "/u8"] = u8
    if f32 is not None:
        out[key + "/f32"] = f32
    out[key + "/counters"] = np.array([int(st[k]) for k in COUNTER_KEYS], np.uint64)
    out[key + "/stats"] = np.array([int(st["kernel_launches"]), int(st["trace_kernel_launches"]), int(st["node_format"])], np.uint32)


def render_cases(engine=None, collect_stats=False):
    """{"<case>/<builder>/u8|f32|counters|stats": array} of CASES -- stats: kernel_launches, trace_kernel_launches, node_format --
    and, for the production frames of the fused engine, of OFF under "off/<case>/<builder>/..." """
    from rayca_amd import abi
    fused = engine is None
    engine = abi.ENGINE_FUSED if fused else engine
    out = {}
    for b in BUILDERS:
        scenes = scenes_of(b)
        for name, (scene, cfg, kw) in CASES.items():
            put(out, f"{name}/{b}", scenes[scene].render(cfg, W, H, engine=engine, collect_stats=collect_stats, **kw))
        if fused and not collect_stats:
            for name, (scene, cfg, eng, _) in OFF.items():
                put(out, f"off/{name}/{b}", scenes[scene].render(cfg, W, H, engine=getattr(abi, "ENGINE_" + eng)))
        for ds in scenes.values():
            ds.close()
    return out


def oracle_kinds():
    """what the CPU oracle says about the cases' frames: pixels of +0.0 (misses, and lit vertices in shadow), pixels above it"""
    import oracle_lib
    import test_gpu_general as G
    from rayca_amd import flatten
    for name, (scene, cfg, kw) in CASES.items():
        desc = flatten(G.SCENES[scene]())
        orc = oracle_lib.OracleScene(desc, Config())
        f32 = orc.render(cfg, W, H, tile=kw.get("tile"), want_rgba8=False)[1]
        rgb = f32[..., :3].reshape(-1, 3)
        zero = int((rgb == 0.0).all(axis=1).sum())
        top = rgb.max(axis=1)
        vals, counts = np.unique(rgb[top > 0], axis=0, return_counts=True)
        print(f"{name:32s} pixels {len(rgb):5d}  all-zero {zero:5d}  above zero {int((top > 0).sum()):5d}  most frequent colour "
              f"{vals[counts.argmax()].tolist() if len(vals) else None} x {int(counts.max()) if len(vals) else 0}")
        if name in ("cornell", "sky", "spheres", "quad"):   # whole frames: the camera rays' own hits, and for the Cornell room's point light the shadow rays'
            rays = orc.camera_rays(cfg, W, H)
            t, _, _, _ = orc.trace_rays(rays)
            hit = t < 3.0e38
            line = f"{'':32s} camera rays that miss {int((~hit).sum())}, that hit {int(hit.sum())}"
            if name == "cornell":
                light = np.array([0.0, 1.9, 0.0], np.float32)
                p = rays[:, :3] + rays[:, 3:] * np.where(hit, t, 0.0)[:, None] * np.float32(0.9999)
                ts = orc.trace_rays(np.concatenate([p, light - p], axis=1)[hit])[0]
                dark = (rgb[hit] == 0.0).all(axis=1)
                line += f"; of the hits, light occluded {int((ts < 1.0).sum())} (all-zero among them {int((dark & (ts < 1.0)).sum())}), light visible and pixel above zero {int((~dark & ~(ts < 1.0)).sum())}"
            print(line)
        orc.close()


if __name__ == "__main__":
    if sys.argv[1] == "--kinds":
        oracle_kinds()
    else:
        np.savez(sys.argv[1], **render_cases())
        print("wrote", sys.argv[1], "RAYCA_FUSE_RESOLVE =", os.environ.get("RAYCA_FUSE_RESOLVE"))
