"""Guided upsampling on a real frame: the atrium, lighting traced at 1920 x 1080 and reconstructed at 3840 x 2160 with every
guide (albedo, normal, point, id = material), Pathtracer, 1 sample per pixel, max_depth 1 (one shadow ray) and max_depth 5 (four
bounces).
  upsample alone     HIP-event time of the one launch (RaycaStats.kernel_ms), and the bytes the call has to move at least -- the
                     full-size guides read once, the output written once, the low images read once -- over that time, next to
                     the HBM peak.  profiles/peaks_r03.json holds the VALU and the vector-L1 ceilings and no HBM rate, so the
                     figure is the one bench.py prices its roofline with (8000 GB/s peak, 6300 GB/s achievable).
  the parts          the two G-buffers (camera rays, closest hits, surface, at both sizes), the low-resolution frame, and the
                     whole render_upsampled, each between two events on one stream
  the yardstick      render_device of the full-size frame of the same config, in the same run: code this pass does not touch
  the error          RMSE over r, g, b (values clamped to [0, 1], pixels finite in all three frames) of the upsampled frame and
                     of the full-size one-sample frame, each against a 64-sample full-size frame of the same scene
20 calls after 3 warm-up calls, one process: median, min and max -- the machine is shared, so the spread is part of the result.
Not a test.
usage: python tests/gpu_upsample_probe.py [log file, default profiles/upsample_atrium.log]"""
import dataclasses, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, IntegratorStrategy, flatten, scenes, abi

W, H, SCALE, REPS, WARM, REF_SPP = 3840, 2160, 2, 20, 3, 64
HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0   # bench.py's
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "upsample_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def timed(stream, call):
    """median, min, max in ms of `call` between two events on `stream`"""
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def fmt(t):
    return f"median {t[0]:8.4f} ms   min {t[1]:8.4f}   max {t[2]:8.4f}"


def rmse(a, b, mask):
    d = (a[..., :3].clamp(0.0, 1.0) - b[..., :3].clamp(0.0, 1.0)).double() ** 2
    return float(d[mask].mean().sqrt())


ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
stream = torch.cuda.Stream()
w, h = W // SCALE, H // SCALE
say(f"atrium, lighting at {w} x {h}, picture at {W} x {H} (scale {SCALE}), Pathtracer, 1 spp, gamma 1; guides albedo + normal + point + id, "
    f"sigma_plane 0.1, normal_power_log2 7; {REPS} calls after {WARM} warm-up")
with torch.cuda.stream(stream):
    low, high = ds.upsample_guides(W, H, SCALE, stream=stream)
    t_guides = timed(stream, lambda: ds.upsample_guides(W, H, SCALE, stream=stream))
    t_high = timed(stream, lambda: ds.gbuffer(Config(samples_per_pixel=1), W, H, want=("color", "normal", "point", "material"), stream=stream))
    say(f"  the two G-buffers ({w} x {h} and {W} x {H})        {fmt(t_guides)}   (the full-size one alone: median {t_high[0]:.4f} ms)")
    color = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    full = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    # bytes per OUTPUT pixel the pass must move: full-size guides in, rgba32f out, the low images over scale^2 output pixels
    bpp = (16 + 12 + 12 + 4) + 16 + (16 + 16 + 12 + 12 + 4) / SCALE ** 2
    for depth in (1, 5):
        cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0, max_depth=depth)
        say(f"max_depth {depth}:")
        t_low = timed(stream, lambda: ds.render_device(cfg, w, h, 0, color.data_ptr(), stream=stream.cuda_stream))
        say(f"  render_device {w} x {h} (the low frame)           {fmt(t_low)}")
        ms = []
        for i in range(WARM + REPS):
            _, st = ds.upsample(color, SCALE, low=low, high=high, sigma_plane=0.1, out=out, stream=stream, want_stats=True)
            if i >= WARM:
                ms.append(st["kernel_ms"])
        t_up = (float(np.median(ms)), min(ms), max(ms))
        gbs = W * H * bpp / t_up[0] / 1e6
        say(f"  upsample alone (one launch, kernel_ms)             {fmt(t_up)}   = {gbs:7.1f} GB/s of the {bpp:.0f} B/pixel the call must move "
            f"({gbs / HBM_PEAK_GBS:.2f} of the {HBM_PEAK_GBS:.0f} GB/s HBM peak, {gbs / HBM_ACHIEVABLE_GBS:.2f} of the achievable {HBM_ACHIEVABLE_GBS:.0f})")
        t_all = timed(stream, lambda: ds.render_upsampled(cfg, W, H, SCALE, out=out, stream=stream))
        say(f"  render_upsampled, whole ({W} x {H})              {fmt(t_all)}")
        t_den = timed(stream, lambda: ds.render_upsampled(cfg, W, H, SCALE, denoise=True, out=out, stream=stream))
        say(f"  render_upsampled(denoise=True), whole              {fmt(t_den)}")
        t_full = timed(stream, lambda: ds.render_device(cfg, W, H, 0, full.data_ptr(), stream=stream.cuda_stream))
        say(f"  render_device {W} x {H} (the yardstick)          {fmt(t_full)}   render_upsampled / this = {t_all[0] / t_full[0]:.3f}")
        # the error side: against a 64-sample full-size frame
        ref = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        ds.render_device(dataclasses.replace(cfg, samples_per_pixel=REF_SPP, seed=977), W, H, 0, ref.data_ptr(), stream=stream.cuda_stream)
        ds.render_device(cfg, W, H, 0, full.data_ptr(), stream=stream.cuda_stream)
        up, weight = ds.render_upsampled(cfg, W, H, SCALE, weight=True, stream=stream)
        up_den = ds.render_upsampled(cfg, W, H, SCALE, denoise=True, stream=stream)
        stream.synchronize()
        ok = torch.isfinite(ref).all(-1) & torch.isfinite(full).all(-1) & torch.isfinite(up).all(-1) & torch.isfinite(up_den).all(-1)
        say(f"  RMSE against {REF_SPP} spp at {W} x {H} ({float(ok.float().mean()):.4f} of the pixels finite in every frame): full-size 1 spp {rmse(full, ref, ok):.5f}, "
            f"upsampled {rmse(up, ref, ok):.5f}, upsampled from the denoised low frame {rmse(up_den, ref, ok):.5f}")
        say(f"  fallback (weight_out == 0) at {float((weight == 0).float().mean()):.5f} of the pixels")
stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
open(log_path, "w").write("\n".join(lines) + "\n")
