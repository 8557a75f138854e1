"""The denoiser on a real frame: the atrium at 1920 x 1080, Pathtracer, 1 and 4 samples per pixel, render_denoised's chain with
all guides (albedo, normal, point, id) and 5 iterations.
  per call      HIP-event time of a whole rayca_hip_denoise_device call (RaycaStats.kernel_ms) for 0..5 iterations: the
                difference between n and n - 1 iterations is the a-trous launch of step 2^(n-1) (and the demodulation, for n = 1)
  traffic       the bytes an iteration has to move at least (read 16 colour + 12 normal + 12 point + 4 id, write 16 per pixel)
                over that launch's time
  torch         the same filter written with plain torch ops on slices of the same tensors, the baseline a user has today,
                timed with events around the 5 iterations; its result is compared with the library's
20 calls after 3 warm-up calls, one process: median, min and max -- the machine is shared, so the spread is part of the result.
Not a test.
usage: python tests/gpu_denoise_probe.py [log file, default profiles/denoise_atrium.log]"""
import dataclasses, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, IntegratorStrategy, flatten, scenes, abi

W, H, REPS, WARM, ITER = 1920, 1080, 20, 3, 5
SIGMA_COLOR, SIGMA_PLANE, NPOW = 4.0, 0.1, 7
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def stats(ms):
    return float(np.median(ms)), min(ms), max(ms)


K = (0.375, 0.25, 0.0625)


def torch_iteration(c, step, normal, point, ident, kc, kp):
    """one iteration with torch ops: per tap the overlapping slices of the image and of the image shifted by the tap"""
    h, w = c.shape[:2]
    total = torch.zeros((h, w, 3), dtype=torch.float32, device=c.device)
    wsum = torch.zeros((h, w), dtype=torch.float32, device=c.device)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            p, q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            d = c[p][..., :3] - c[q][..., :3]
            wt = (K[abs(dx)] * K[abs(dy)]) / (1.0 + (d * d).sum(-1) * kc)
            dn = (normal[p] * normal[q]).sum(-1).clamp_min(0.0)
            for _ in range(NPOW):
                dn = dn * dn
            wt = wt * dn
            pd = (normal[p] * (point[q] - point[p])).sum(-1)
            wt = wt / (1.0 + pd * pd * kp)
            wt = torch.where((ident[p] == ident[q]) & (wt > 0.0), wt, torch.zeros_like(wt))
            total[p] += wt[..., None] * c[q][..., :3]
            wsum[p] += wt
    out = c.clone()
    ok = wsum > 0.0
    out[..., :3] = torch.where(ok[..., None], total / wsum[..., None], c[..., :3])
    return out


def torch_denoise(color, albedo, normal, point, ident):
    den = albedo[..., :3].clamp_min(1e-3)
    c = color.clone()
    c[..., :3] = c[..., :3] / den
    for i in range(ITER):
        c = torch_iteration(c, 1 << i, normal, point, ident, 1.0 / (SIGMA_COLOR * SIGMA_COLOR), 1.0 / (SIGMA_PLANE * SIGMA_PLANE))
    c[..., :3] = c[..., :3] * den
    return c


ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
stream = torch.cuda.Stream()
n = W * H
say(f"atrium, {W} x {H} = {n} pixels, Pathtracer; guides albedo + normal + point + id, sigma_color {SIGMA_COLOR}, sigma_plane {SIGMA_PLANE}, "
    f"normal_power_log2 {NPOW}; {REPS} calls after {WARM} warm-up")
with torch.cuda.stream(stream):
    for spp in (1, 4):
        cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=spp, gamma=1.0)
        color = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        ds.render_device(dataclasses.replace(cfg, gamma=1.0), W, H, 0, color.data_ptr(), stream=stream.cuda_stream)
        g = ds.gbuffer(cfg, W, H, want=("color", "normal", "point", "material"), stream=stream)
        kw = dict(albedo=g["color"], normal=g["normal"], point=g["point"], id=g["material"], sigma_color=SIGMA_COLOR, sigma_plane=SIGMA_PLANE,
                  normal_power_log2=NPOW, stream=stream)
        out = torch.empty_like(color)
        stream.synchronize()
        say(f"{spp} spp: {float((g['prim'] != -1).float().mean()):.3f} of the pixels hit")
        med = {}
        for it in range(ITER + 1):
            ms, launches = [], 0
            for i in range(WARM + REPS):
                _, st = ds.denoise(color, out=out, iterations=it, want_stats=True, **kw)
                launches = st["kernel_launches"]
                if i >= WARM:
                    ms.append(st["kernel_ms"])
            med[it], lo, hi = stats(ms)
            line = f"  denoise, {it} iterations ({launches} launches)   median {med[it]:7.4f} ms   min {lo:7.4f}   max {hi:7.4f}"
            if it:
                step_ms = med[it] - med[it - 1]
                line += f"   step {1 << (it - 1):2d}{' + demodulation' if it == 1 else ''}: {step_ms:7.4f} ms"
                if it > 1:
                    line += f" = {n * 60 / step_ms / 1e6:7.1f} GB/s of the 60 B/pixel an iteration must move"
            say(line)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for i in range(WARM + REPS):
            ev0.record(stream)
            ref = torch_denoise(color, g["color"], g["normal"], g["point"], g["material"])
            ev1.record(stream)
            ev1.synchronize()
            if i >= WARM:
                ms.append(ev0.elapsed_time(ev1))
        tmed, lo, hi = stats(ms)
        say(f"  torch ops, {ITER} iterations                median {tmed:7.3f} ms   min {lo:7.3f}   max {hi:7.3f}   = {tmed / med[ITER]:.1f} x the library's {med[ITER]:.4f} ms")
        got = ds.denoise(color, iterations=ITER, **kw)
        stream.synchronize()
        both = torch.isfinite(got) & torch.isfinite(ref)
        diff = (got - ref).abs()[both]
        say(f"  library against torch: max |difference| {float(diff.max()):.3g}, {float((diff > 0).float().mean()):.4f} of the values differ "
            f"(torch sums a pixel's three products in its own order)")
stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
open(log_path, "w").write("\n".join(lines) + "\n")
