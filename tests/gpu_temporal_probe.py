"""The temporal pass on a real frame: the atrium at 1920 x 1080, Pathtracer, 1 sample per pixel.  Two frames from two cameras
(the second a small step aside and a small turn, through DeviceScene.update), their G-buffers (point, normal, id = material),
and the history the first one leaves; then rayca_hip_accumulate_device for the second frame
  identity       pixel by pixel (what a standing camera costs)
  reprojection   through the first camera, with every guide (normal, point, id)
each with and without the luminance moments (+ variance).
  per call      HIP-event time of the one launch (RaycaStats.kernel_ms)
  traffic       the bytes the call has to move at least -- every input image read once, every output written once -- over that
                time, next to the HBM peak.  profiles/peaks_r03.json holds the VALU and the vector-L1 ceilings and no HBM rate,
                so the figure is the one bench.py prices its roofline with (8000 GB/s peak, 6300 GB/s achievable).  The frame
                set of a call (120 to 270 MB) is of the order of the 256-MB last-level cache, so a rate above the achievable
                HBM rate says that part of it stayed there between calls.
20 calls after 3 warm-up calls, one process: median, min and max -- the machine is shared, so the spread is part of the result.
Not a test.
usage: python tests/gpu_temporal_probe.py [log file, default profiles/temporal_atrium.log]"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, IntegratorStrategy, flatten, scenes, abi

W, H, REPS, WARM = 1920, 1080, 20, 3
HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0   # bench.py's
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "temporal_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def view(ds, cfg, stream):
    color = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    ds.render_device(cfg, W, H, 0, color.data_ptr(), stream=stream.cuda_stream)
    g = ds.gbuffer(cfg, W, H, want=("point", "normal", "material"), stream=stream)
    return color, {"point": g["point"], "normal": g["normal"], "id": g["material"]}, g["prim"], ds.camera_pose()


desc = flatten(scenes.atrium_scene())
ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
ds.finish()
stream = torch.cuda.Stream()
n = W * H
cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0)
say(f"atrium, {W} x {H} = {n} pixels, Pathtracer, 1 spp; normal_min 0.9, plane_max 0.1; {REPS} calls after {WARM} warm-up")
with torch.cuda.stream(stream):
    color_a, g_a, _, pose_a = view(ds, cfg, stream)
    first = ds.accumulate(color_a, variance=True, stream=stream)
    cam = next(x for x in desc._nodes[:desc.c.node_count] if x.camera != abi.NONE)
    t, q, turn = tuple(cam.trs.translation), tuple(cam.trs.rotation), 0.01
    cam.trs.translation[:] = (t[0] + 0.05, t[1] + 0.02, t[2] - 0.03)
    s, c = math.sin(turn / 2), math.cos(turn / 2)
    cam.trs.rotation[:] = (q[0] * c - q[2] * s, q[1] * c + q[3] * s, q[2] * c + q[0] * s, q[3] * c - q[1] * s)   # q x (0, s, 0, c)
    stream.synchronize()
    ds.update(desc)
    color_b, g_b, prim_b, pose_b = view(ds, Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0, seed=1), stream)
    stream.synchronize()
    hit = prim_b != -1
    say(f"{float(hit.float().mean()):.3f} of the second frame's pixels hit; the camera moved {math.dist(list(pose_a.origin), list(pose_b.origin)):.3f} world units and turned {turn} rad")
    # bytes per pixel a call must move: reads + writes
    base = {"identity": (16 + 16 + 4) + (16 + 4), "reprojection": (16 + 12 + 12 + 4) + (16 + 4 + 12 + 12 + 4) + (16 + 4)}
    extra = (8) + (8 + 4)   # hist_moments in; moments and variance out
    for mode in ("identity", "reprojection"):
        for moments in (False, True):
            hist = {k: first[k] for k in (("color", "length", "moments") if moments else ("color", "length"))}
            kw = dict(history=hist, moments=moments, variance=moments, stream=stream)
            if mode == "reprojection":
                kw.update(prev=g_a, prev_camera=pose_a, **g_b)
            out = None
            ms = []
            for i in range(WARM + REPS):
                r = ds.accumulate(color_b, out=out, want_stats=True, **kw)
                out = {k: v for k, v in r.items() if k != "stats"}
                if i >= WARM:
                    ms.append(r["stats"]["kernel_ms"])
            med, lo, hi = float(np.median(ms)), min(ms), max(ms)
            bpp = base[mode] + (extra if moments else 0)
            gbs = n * bpp / med / 1e6
            line = (f"  {mode:12s} {'moments + variance' if moments else 'no moments        '}   median {med:7.4f} ms   min {lo:7.4f}   max {hi:7.4f}"
                    f"   = {gbs:7.1f} GB/s of the {bpp} B/pixel the call must move ({gbs / HBM_PEAK_GBS:.2f} of the {HBM_PEAK_GBS:.0f} GB/s HBM peak, "
                    f"{gbs / HBM_ACHIEVABLE_GBS:.2f} of the achievable {HBM_ACHIEVABLE_GBS:.0f})")
            say(line)
            if mode == "reprojection" and moments:
                stream.synchronize()
                kept = (out["length"] > 1.0) & hit
                say(f"  {float(kept.sum()) / float(hit.sum()):.3f} of the hit pixels kept their history through the move")
stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
open(log_path, "w").write("\n".join(lines) + "\n")
