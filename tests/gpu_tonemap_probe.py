"""Exposure metering and tone mapping on a real frame: the atrium's film at 1920 x 1080 (Pathtracer, 1 sample per pixel, two frames
added), 33 MB of float pixels.
  the yardstick      DeviceScene.denoise(iterations=0) on the same frame into the same output: the output stage alone, the bytes of
                     a tonemap call in and out, code this pass does not touch
  tonemap            each operator with a host scale, float output, gamma 1; and ACES with the meter's record, both outputs, gamma 2.2,
                     next to the yardstick with both outputs and gamma 2.2
  meter              the whole call (the clear, the histogram kernel, the exposure kernel), and RaycaStats.kernel_ms of the same
Every figure is the time between two events on one stream around one call, 20 rounds after 3 warm-up rounds, one process; a round
times every candidate once, in turn, so that what else the shared machine does falls on all of them alike: median, min and max.
The log ends with the two ratios the design quotes and the structure that is kept.  The A/B runs that chose that structure are in
profiles/tonemap_atrium_ab.log; the last-block-done ticket form of the meter was not built, so it is measured nowhere.  Not a test.
usage: python tests/gpu_tonemap_probe.py [log file, default profiles/tonemap_atrium.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, flatten, scenes, abi

W, H, REPS, WARM = 1920, 1080, 20, 3
HBM_ACHIEVABLE_GBS = 6300.0   # bench.py's
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tonemap_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def timed_in_turn(stream, calls):
    """{name: (median, min, max) in ms} of each call between two events on `stream`, the candidates taking turns"""
    ms = {name: [] for name in calls}
    for i in range(WARM + REPS):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if i >= WARM:
                ms[name].append(a.elapsed_time(b))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in ms.items()}


def fmt(t):
    return f"median {t[0]:8.4f} ms   min {t[1]:8.4f}   max {t[2]:8.4f}"


ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
stream = torch.cuda.Stream()
mb = W * H * 16 / 1e6
say(f"atrium film, {W} x {H}, Pathtracer, 1 spp, 2 frames added; {mb:.1f} MB of float pixels; {REPS} rounds after {WARM} warm-up, the candidates of a block in turn")
with torch.cuda.stream(stream):
    film = Film(ds, W, H)
    cfg = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0)
    film.add(cfg, stream=stream)
    film.add(cfg, stream=stream)
    color = film.color
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    hist = torch.empty((260,), dtype=torch.int32, device="cuda")
    record = torch.empty((4,), dtype=torch.float32, device="cuda")
    ds.meter(color, out=(hist, record), stream=stream)
    stream.synchronize()
    h = hist.cpu().numpy()
    say(f"  the frame: counted {h[256]}, black {h[257]}, not finite {h[258]}, {(h[:256] > 0).sum()} bins in use, the fullest holds {h[:256].max()}; "
        f"exposure record {[round(float(x), 6) for x in record.cpu()]}")

    say("float in, float out, gamma 1:")
    t = timed_in_turn(stream, {
        "stage": lambda: ds.denoise(color, iterations=0, out=out, stream=stream),
        "linear": lambda: ds.tonemap(color, "linear", scale=0.5, out=out, stream=stream),
        "reinhard": lambda: ds.tonemap(color, "reinhard", scale=0.5, white=4.0, out=out, stream=stream),
        "aces": lambda: ds.tonemap(color, "aces", scale=0.5, out=out, stream=stream),
        "meter": lambda: ds.meter(color, out=(hist, record), stream=stream),
    })
    stage = t["stage"]
    spread = (stage[2] - stage[1]) / stage[0]
    say(f"  denoise(iterations=0): the output stage alone     {fmt(stage)}   = {2 * mb / stage[0]:7.1f} GB/s of its {2 * mb:.1f} MB; run-to-run spread (max - min) / median = {spread:.3f}")
    for op in ("linear", "reinhard", "aces"):
        say(f"  tonemap {op:9s}                                 {fmt(t[op])}   / the stage = {t[op][0] / stage[0]:.3f}")
    meter = t["meter"]
    say(f"  meter, the whole call                             {fmt(meter)}   / the stage = {meter[0] / stage[0]:.3f}   = {mb / meter[0]:7.1f} GB/s of the {mb:.1f} MB it reads "
        f"({mb / meter[0] / HBM_ACHIEVABLE_GBS:.2f} of the achievable {HBM_ACHIEVABLE_GBS:.0f})")
    ms, launches = [], 0
    for i in range(WARM + REPS):
        _, _, st = ds.meter(color, out=(hist, record), stream=stream, want_stats=True)
        launches = st["kernel_launches"]
        if i >= WARM:
            ms.append(st["kernel_ms"])
    say(f"  meter: RaycaStats.kernel_ms ({launches} launches: clear, histogram, exposure)   median {np.median(ms):8.4f} ms   min {min(ms):8.4f}   max {max(ms):8.4f}")
    ratio_tonemap = max(t[op][0] for op in ("linear", "reinhard", "aces")) / stage[0]
    ratio_meter = meter[0] / stage[0]

    say("float in, float and RGBA8 out, gamma 2.2:")
    t = timed_in_turn(stream, {
        "stage": lambda: ds.denoise(color, iterations=0, gamma=2.2, out=out, rgba8=out8, stream=stream),
        "aces": lambda: ds.tonemap(color, "aces", exposure=record, gamma=2.2, out=out, rgba8=out8, stream=stream),
        "chain": lambda: (ds.meter(color, out=(hist, record), stream=stream), ds.tonemap(color, "aces", exposure=record, gamma=2.2, out=out, rgba8=out8, stream=stream)),
    })
    say(f"  denoise(iterations=0, gamma=2.2, rgba8)            {fmt(t['stage'])}")
    say(f"  tonemap aces, the meter's record                   {fmt(t['aces'])}   / the stage = {t['aces'][0] / t['stage'][0]:.3f}")
    say(f"  meter then tonemap aces, one stream, no host wait  {fmt(t['chain'])}   / the stage = {t['chain'][0] / t['stage'][0]:.3f}")
say(f"ratios against the output stage alone (float to float, gamma 1): tonemap {ratio_tonemap:.3f} (the slowest operator), meter {ratio_meter:.3f}")
say("structure kept: hipMemsetAsync of the 260 words, k_meter_hist (at most 256 blocks of 1024 lanes, one LDS copy of the bins a wave), "
    "k_exposure (one wave), three stream-ordered steps; the ticket form was not built")
stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
open(log_path, "w").write("\n".join(lines) + "\n")
