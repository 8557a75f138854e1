"""The variance-guided denoiser on a real film: the atrium at 1920 x 1080, Pathtracer, 1 sample per pixel, a film of 4 frames
(Film.add: colour, variance, length), all guides (albedo, normal, point, id), 1..5 iterations.
  per call      HIP-event time of a whole rayca_hip_denoise_variance_device call (RaycaStats.kernel_ms) for 1..5 iterations: the
                difference between n and n - 1 iterations is the k_atrous_var launch of step 2^(n-1)
  yardstick     rayca_hip_denoise_device with the same guides and iteration count, timed in the same process, the two calls
                alternating: the difference between n and n - 1 iterations is k_atrous's launch of the same step
  traffic       the bytes an iteration has to move at least (read 16 colour + 4 variance + 12 normal + 12 point + 4 id, write
                16 + 4 per pixel = 68 B; the plain filter's 60 B) over that launch's time; a tap moves 48 B against 44 B, and
                the 3 x 3 prefilter adds 9 loads of 4 B per pixel: (25 * 48 + 36) / (25 * 44) = 1.124 of the plain filter's
                cache traffic
20 calls after 3 warm-up calls, one process: median, min and max -- the machine is shared, so the spread is part of the result.
Not a test.
usage: python tests/gpu_denoise_variance_probe.py [log file, default profiles/denoise_variance_atrium.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, flatten, scenes, abi

W, H, REPS, WARM, ITER, FRAMES = 1920, 1080, 20, 3, 5, 4
SIGMA_COLOR, SIGMA_LUMINANCE, SIGMA_PLANE, NPOW, MIN_HISTORY = 4.0, 4.0, 0.1, 7, 4
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_variance_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def stats(ms):
    return float(np.median(ms)), min(ms), max(ms)


ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
stream = torch.cuda.Stream()
n = W * H
say(f"atrium, {W} x {H} = {n} pixels, Pathtracer, 1 spp, a film of {FRAMES} frames; guides albedo + normal + point + id, sigma_luminance "
    f"{SIGMA_LUMINANCE}, sigma_color {SIGMA_COLOR} (the plain filter), sigma_plane {SIGMA_PLANE}, normal_power_log2 {NPOW}; {REPS} calls after {WARM} warm-up")
with torch.cuda.stream(stream):
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0)
    film = Film(ds, W, H)
    for _ in range(FRAMES):
        film.add(cfg, stream=stream)
    albedo = ds.gbuffer(cfg, W, H, want=("color",), stream=stream)["color"]
    guides = dict(albedo=albedo, sigma_plane=SIGMA_PLANE, normal_power_log2=NPOW, stream=stream, **film.gbuffer())
    color, variance = film.color, film.variance
    out, var_out = torch.empty_like(color), torch.empty_like(variance)
    stream.synchronize()
    say(f"history length: min {float(film.length.min()):.0f}, max {float(film.length.max()):.0f}; mean variance {float(variance.mean()):.4g}")
    for name, length, min_history in (("the film of 4 frames", film.length, MIN_HISTORY),
                                      ("the same film with length 1 everywhere", torch.ones_like(film.length), MIN_HISTORY)):
        say(f"{name}: {float((length < min_history).float().mean()):.4f} of the lanes take the spatial estimate")
        med = {"var": {0: None}, "plain": {}}
        ms = {("var", it): [] for it in range(1, ITER + 1)}
        ms.update({("plain", it): [] for it in range(0, ITER + 1)})
        launches = {}
        for i in range(WARM + REPS):   # the two filters and the iteration counts alternate inside every repetition
            for it in range(0, ITER + 1):
                if it:
                    *_, st = ds.denoise_variance(color, variance, length=length, min_history=min_history, sigma_luminance=SIGMA_LUMINANCE, out=out,
                                                variance_out=var_out, iterations=it, want_stats=True, **guides)
                    launches["var", it] = st["kernel_launches"]
                    if i >= WARM:
                        ms["var", it].append(st["kernel_ms"])
                _, st = ds.denoise(color, out=out, iterations=it, sigma_color=SIGMA_COLOR, want_stats=True, **guides)
                launches["plain", it] = st["kernel_launches"]
                if i >= WARM:
                    ms["plain", it].append(st["kernel_ms"])
        for it in range(0, ITER + 1):
            med["plain"][it], lo, hi = stats(ms["plain", it])
            line = f"  plain denoise,     {it} iterations ({launches['plain', it]} launches)   median {med['plain'][it]:7.4f} ms   min {lo:7.4f}   max {hi:7.4f}"
            if it > 1:
                step_ms = med["plain"][it] - med["plain"][it - 1]
                line += f"   step {1 << (it - 1):2d}: {step_ms:7.4f} ms = {n * 60 / step_ms / 1e6:7.1f} GB/s of 60 B/pixel"
            say(line)
        for it in range(1, ITER + 1):
            med["var"][it], lo, hi = stats(ms["var", it])
            line = f"  variance-guided,   {it} iterations ({launches['var', it]} launches)   median {med['var'][it]:7.4f} ms   min {lo:7.4f}   max {hi:7.4f}"
            if it > 1:
                step_ms = med["var"][it] - med["var"][it - 1]
                plain_ms = med["plain"][it] - med["plain"][it - 1]
                line += f"   step {1 << (it - 1):2d}: {step_ms:7.4f} ms = {n * 68 / step_ms / 1e6:7.1f} GB/s of 68 B/pixel, {step_ms / plain_ms:5.3f} x k_atrous's {plain_ms:.4f} ms"
            else:
                line += f"   demodulation + initial variance + step 1 + output"
            say(line)
        say(f"  5 iterations: variance-guided {med['var'][ITER]:.4f} ms against the plain filter's {med['plain'][ITER]:.4f} ms = {med['var'][ITER] / med['plain'][ITER]:.3f} x")
stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
open(log_path, "w").write("\n".join(lines) + "\n")
