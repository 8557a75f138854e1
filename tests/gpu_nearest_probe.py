"""Nearest-point queries on device memory: kernel time, points per second and boxes / triangles priced per point, on the atrium
(RAYCA_BUILDER_SAH after finish()), 2**20 points of two kinds:
  near     the hit points of a 1024 x 1024 frame's camera rays, pushed 1 % of the scene's diagonal along the shading normal
  uniform  uniform in the bounds of those hit points
Per kind: CLOSEST unbounded, CLOSEST with a radius of 5 % of the diagonal, WITHIN with that radius (k_nearest, one point per
lane on the binary f32 nodes).  Beside them, in the same run, the yardstick: query(kind="closest") of as many rays -- the
frame's camera rays, and rays from the uniform points in random directions.
Medians of 10 (min / max beside them) of RaycaStats.kernel_ms after 3 warm-up calls, one process; the machine is shared, so the
spread of each row is part of the result.  The counters come from one more call with collect_stats (the counting kernel).
usage: python tests/gpu_nearest_probe.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi

SIDE, REPS, WARM = 1024, 10, 3
N = SIDE * SIDE
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
stream = torch.cuda.Stream()

cam = ds.camera_rays(Config(), SIDE, SIDE, stream=stream)
t, prim, uv = ds.query(cam, stream=stream)
s = ds.surface(cam, t, prim, uv, want=("point", "normal"), stream=stream)
stream.synchronize()
hit = prim != -1
lo, hi = s["point"][hit].min(0).values, s["point"][hit].max(0).values
diag = float(torch.linalg.norm(hi - lo))
g = torch.Generator(device="cuda").manual_seed(5)
uniform = (lo + torch.rand((N, 3), device="cuda", generator=g) * (hi - lo)).contiguous()
near = torch.where(hit[:, None], s["point"] + s["normal"] * (0.01 * diag), uniform).contiguous()
d = torch.randn((N, 3), device="cuda", generator=g)
random_rays = torch.cat([uniform, d / torch.linalg.norm(d, dim=1, keepdim=True)], 1).contiguous()
radius = 0.05 * diag
print(f"atrium: {info['triangle_count']} triangles, stack need {info['max_depth']}; {N} points per set; camera rays: {float(hit.float().mean()):.3f} hit; "
      f"diagonal {diag:.3f}, radius {radius:.3f}", flush=True)


def row(label, ms, extra=""):
    med = float(np.median(ms))
    print(f"  {label:44s} median {med:8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}   {N / med / 1e3:8.1f} M/s{extra}", flush=True)


def timed(call):
    ms = []
    for i in range(WARM + REPS):
        st = call(want_stats=True)[-1]
        if i >= WARM:
            ms.append(st["kernel_ms"])
    return ms


out = (torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"),
       torch.empty((N, 3), dtype=torch.float32, device="cuda"), torch.empty((N, 2), dtype=torch.float32, device="cuda"))
mask = torch.empty(N, dtype=torch.uint8, device="cuda")
qout = (torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty((N, 2), dtype=torch.float32, device="cuda"))
for name, pts in (("near", near), ("uniform", uniform)):
    print(f"{name}:", flush=True)
    cases = (("closest, unbounded", dict(kind="closest", out=out)), (f"closest, radius 5 % of the diagonal", dict(kind="closest", radius=radius, out=out)),
             ("within, radius 5 % of the diagonal", dict(kind="within", radius=radius, out=mask)))
    for label, kw in cases:
        ms = timed(lambda **o: ds.nearest(pts, stream=stream, **kw, **o))
        st = ds.nearest(pts, stream=stream, collect_stats=True, **kw)[-1]
        found = float((out[1] != -1).float().mean()) if kw["kind"] == "closest" else float(mask.float().mean())
        row(label, ms, f"   boxes / point {st['boxes_tested'] / N:7.1f}   triangles / point {st['triangles_tested'] / N:7.1f}   found {found:.3f}")
print("yardstick, query(kind=\"closest\") on the same scene:", flush=True)
for label, rays in (("the frame's camera rays (k_query_refill)", cam), ("rays from the uniform points, random directions", random_rays)):
    ms = timed(lambda **o: ds.query(rays, stream=stream, out=qout, **o))
    st = ds.query(rays, stream=stream, out=qout, collect_stats=True)[-1]
    row(label, ms, f"   boxes / ray   {st['boxes_tested'] / N:7.1f}   triangles / ray   {st['triangles_tested'] / N:7.1f}   found {float((qout[1] != -1).float().mean()):.3f}")
ds.close()
