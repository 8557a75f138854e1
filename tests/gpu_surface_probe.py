"""Surface records against the query that feeds them: per-launch kernel time on the atrium, RAYCA_BUILDER_SAH after finish(),
on the camera rays of a 1920 x 1080 frame (rayca_hip_camera_rays_device, sample 0 of 1).
  closest        rayca_hip_query_device CLOSEST, unbounded: k_query_refill
  surface all    rayca_hip_surface_device, all eight outputs: k_surface, full
  surface color  rayca_hip_surface_device, color alone: k_surface stops behind get_color, as a Flat frame does
HIP-event time of each launch (RaycaStats.kernel_ms), 20 launches after 3 warm-up calls, one process: median, min and max --
the machine is shared, so the spread of each row is part of the result.  Not a test.
usage: python tests/gpu_surface_probe.py [log file, default profiles/surface_atrium.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, IntegratorStrategy, flatten, scenes, abi

W, H, REPS, WARM = 1920, 1080, 20, 3
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "surface_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
flat = Config(integrator=IntegratorStrategy.Flat)
stream = torch.cuda.Stream()
rays = ds.camera_rays(flat, W, H, stream=stream)
n = rays.shape[0]
rec = ds.query(rays, stream=stream)
stream.synchronize()
hit = float((rec[1] != -1).float().mean())
say(f"atrium, {W} x {H} camera rays = {n} records, {hit:.3f} hit; {REPS} launches after {WARM} warm-up, HIP events per launch")


def row(label, call, bytes_moved):
    ms = []
    for i in range(WARM + REPS):
        st = call()
        if i >= WARM:
            ms.append(st["kernel_ms"])
    med = float(np.median(ms))
    say(f"  {label:38s} median {med:7.4f} ms   min {min(ms):7.4f}   max {max(ms):7.4f}   {med * 1e6 / n:6.3f} ns/record"
        + (f"   {bytes_moved / med / 1e6:7.1f} GB/s of records in + out" if bytes_moved else ""))


out_q = tuple(torch.empty_like(x) for x in rec)
row("closest (k_query_refill)", lambda: ds.query(rays, out=out_q, stream=stream, want_stats=True)[-1], 0)
names = tuple(DeviceScene.SURFACE_OUTPUTS)
out_all = ds.surface(rays, *rec, stream=stream)
# records read (ray 24 B, t 4, prim 4, uv 8) and written (12 + 12 + 16 x 3 + 8 + 4 + 4); the 256-B shading record of the
# primitive and the material come on top, from the caches where neighbouring pixels share them
row("surface, all outputs (k_surface)", lambda: ds.surface(rays, *rec, want=names, out=out_all, stream=stream, want_stats=True)["stats"], n * (40 + 88))
out_c = {"color": out_all["color"]}
row("surface, color alone (k_surface)", lambda: ds.surface(None, *rec, want=("color",), out=out_c, stream=stream, want_stats=True)["stats"], n * (16 + 16))
stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
open(log_path, "w").write("\n".join(lines) + "\n")
