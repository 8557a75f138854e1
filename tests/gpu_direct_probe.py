"""Direct light at points on device memory: what DeviceScene.direct costs beside the composition it replaces, on the atrium's
G-buffer (RAYCA_BUILDER_SAH after finish()) at 1920 x 1080 under the scene's lights (one point light), light_samples 1 and 4.
On the pixels whose camera ray hits:
  direct   direct(want=("irradiance",)), hemisphere mode, bias 1e-4: k_direct_refill, then k_direct_fold
  composed the same sum from the public pieces: the samples in torch (position, fall-off, cosine: the header's formulas for a point
           light, one row per pixel x sample), query(kind="occluded", tmax=dist) on the (N x S, 6) rays, a masked torch reduction.
           The atrium has no quad light, so the second query of the general composition (closest hit + surface flags) is not run:
           this is the least the composition needs here.
All on one stream in one process; medians of REPS (min / max beside them) after WARM warm-up rounds of HIP-event time around each
whole call, the two alternating.  The machine is shared, so the spread of each row is part of the result.  Also the peak of
torch's allocator over one call of each (outputs and intermediates; the library's own scratch -- 8 B a point of mask words for
direct, nothing for query -- is not torch's and is added by hand), and the largest difference of the two results.
usage: python tests/gpu_direct_probe.py [width height]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
REPS, WARM, BIAS = 7, 2, 1e-4
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
lights = ds.lights()
assert all(int(L["kind"]) == abi.LIGHT_POINT for L in lights), "the composition below restates point lights only"
stream = torch.cuda.Stream()

with torch.cuda.stream(stream):
    g = ds.gbuffer(Config(), W, H, want=("point", "normal"), stream=stream)
    hit = g["prim"].reshape(-1) != -1
    p, n = g["point"].reshape(-1, 3)[hit].contiguous(), g["normal"].reshape(-1, 3)[hit].contiguous()
    missed = int((~hit).sum())
    del g
stream.synchronize()
N = p.shape[0]
print(f"atrium: {info['triangle_count']} triangles, {len(lights)} light(s); {W} x {H} G-buffer, {N} pixels hit ({missed} miss and are left out)", flush=True)


def composed(ls):
    """E (N, 3): one row per pixel x light x sample, as a caller without the entry point has to"""
    e = torch.zeros((N, 3), dtype=torch.float32, device=p.device)
    o = p + n * BIAS
    for L in lights:
        x1 = torch.tensor(L["position"][:3], device=p.device)
        v = x1 - p
        r2 = (v * v).sum(1)
        dist = r2.sqrt()
        omega = v / dist[:, None]
        att = [float(a) for a in L["attenuation"][:3]]
        fallof = att[0] + att[1] * dist + att[2] * r2
        le = (float(L["intensity"]) * torch.tensor(L["color"][:3], device=p.device))[None] / fallof[:, None]
        ndot = (n * omega).sum(1).clamp(0.0, 1.0)
        y = le * (ndot / r2)[:, None] * float(L["color"][3])
        rays = torch.cat([o, omega], 1).repeat_interleave(ls, 0)           # (point lights: the ls samples of a pixel are one ray, ls times)
        occ = ds.query(rays, kind="occluded", tmax=dist.repeat_interleave(ls, 0), stream=stream, context=2)
        lit = (occ == 0).reshape(N, ls) & torch.isfinite(y).all(1)[:, None] & (y != 0).any(1)[:, None]
        e = e + (y[:, None, :] * lit[:, :, None]).sum(1)
    return e


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        r = fn()
        e1.record(stream)
    stream.synchronize()
    return r, e0.elapsed_time(e1)


def peak(fn):
    stream.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.cuda.stream(stream):
        r = fn()
    stream.synchronize()
    top = torch.cuda.max_memory_allocated() - base
    del r
    return top


def row(label, ms, rays, extra=""):
    med = float(np.median(ms))
    print(f"  {label:58s} median {med:9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   {rays / med / 1e3:8.1f} Msamples/s{extra}", flush=True)


for ls in (1, 4):
    cfg = Config(light_samples=ls, max_depth=1)
    S = ls * len(lights)
    direct = lambda: ds.direct(p, n, cfg, bias=BIAS, want=("irradiance",), stream=stream, context=1)
    ms = {"direct": [], "composed": []}
    for i in range(WARM + REPS):
        for key, fn in (("direct", direct), ("composed", lambda: composed(ls))):
            r, t = timed(fn)
            if i >= WARM:
                ms[key].append(t)
            if key == "direct":
                a = r["irradiance"][:, :3]
            else:
                b = r
    st = ds.direct(p, n, cfg, bias=BIAS, want=("irradiance", "counts"), stream=stream, context=1, collect_stats=True)["stats"]
    print(f"light_samples {ls}: {S} samples a pixel, {st['rays_shadow']} of {N * S} traced", flush=True)
    row("direct (k_direct_refill + k_direct_fold)", ms["direct"], N * S,
        f"   launches {st['kernel_launches']}   kernel_ms {st['kernel_ms']:.3f} (counting run)   boxes {st['boxes_tested']}   triangles {st['triangles_tested']}")
    row("composed (torch samples + query(occluded) + torch sum)", ms["composed"], N * S)
    print(f"  direct / composed = {np.median(ms['direct']) / np.median(ms['composed']):.4f}", flush=True)
    pd, pc = peak(direct), peak(lambda: composed(ls))
    print(f"  peak bytes of torch's allocator over one call: direct {pd} (+ {8 * N} B of mask words in the context's scratch), composed {pc}; "
          f"per pixel {pd / N + 8:.1f} against {pc / N:.1f}", flush=True)
    rel = ((a.double() - b.double()).abs() / b.double().abs().clamp(min=1e-6))
    print(f"  largest relative difference of the two sums {float(rel.max()):.3e} (the composition rounds in torch's order); "
          f"mean E {[round(float(v), 5) for v in a.mean(0)]}", flush=True)
ds.close()
