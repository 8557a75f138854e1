"""Adaptive sampling on a real film: the atrium at 1920 x 1080, Pathtracer max_depth 1, jitter 2.
  overhead      HIP-event time (RaycaStats.kernel_ms) of the three calls of one adaptive pass of B = W x H rays on a film of 8
                frames: rayca_hip_sample_plan_device (offsets and rays), rayca_hip_radiance_device along the plan's rays,
                rayca_hip_film_fold_device; the three alternate inside every repetition.  What matters is the share of plan +
                fold in the pass.  REPS calls after WARM warm-up calls, one process: median, min and max -- the machine is
                shared, so the spread is part of the result.
  error         RMS relative luminance error, sqrt(mean(((Y - Y_ref) / max(Y_ref, 0.01))^2)), against a uniform film of
                REFERENCE frames with another seed, at equal total rays: 8 uniform add(jitter=2) frames, then 24 more passes of
                W x H rays each, once uniform (add) and once adaptive (add_adaptive, the defaults).  Both curves; how many pixels
                each adaptive pass gave rays to and how unevenly the last one dealt them out; and where the adaptive film's
                error sits, by the number of samples a pixel has behind it.
Not a test.
usage: python tests/gpu_adaptive_probe.py [log file, default profiles/adaptive_atrium.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, Film, flatten, scenes, abi

W, H, REPS, WARM, JITTER, FIRST, MORE, REFERENCE = 1920, 1080, 20, 3, 2, 8, 24, 1024
log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adaptive_atrium.log")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def stats(ms):
    return float(np.median(ms)), min(ms), max(ms)


def luminance(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
stream = torch.cuda.Stream()
n = W * H
cfg = Config(max_depth=1, seed=1)
say(f"atrium, {W} x {H} = {n} pixels, Pathtracer max_depth 1, jitter {JITTER}; B = W x H rays a pass; target 0.05, lum_floor 1e-3, base_weight 0, "
    f"fresh_weight 255, min_history 4 (the defaults)")
with torch.cuda.stream(stream):
    # ---- (i) what a pass costs ------------------------------------------------------------------------------------------------------
    film = Film(ds, W, H)
    for _ in range(FIRST):
        film.add(cfg, stream=stream, jitter=JITTER)
    hist = {k: film._buffers["hist"][film._hist][k] for k in ("color", "length", "moments")}
    variance = film.variance
    offset = torch.empty((n + 1,), dtype=torch.int32, device=hist["color"].device)
    rays = torch.empty((n, 6), dtype=torch.float32, device=offset.device)
    samples = torch.empty((n, 4), dtype=torch.float32, device=offset.device)
    out = {k: torch.empty_like(v) for k, v in hist.items()}
    out["variance"] = torch.empty_like(variance)
    ms = {"plan": [], "radiance": [], "fold": []}
    launches = {}
    for i in range(WARM + REPS):
        st = {}
        st["plan"] = ds.sample_plan(hist["color"], variance, hist["length"], n, jitter=JITTER, want=("offset", "rays"), out={"offset": offset, "rays": rays},
                                    stream=stream, want_stats=True)["stats"]
        st["radiance"] = ds.radiance(rays, cfg, out=samples, stream=stream, want_stats=True)[-1]
        st["fold"] = ds.fold(samples, offset, hist, out=out, stream=stream, want_stats=True)["stats"]
        for k, s in st.items():
            launches[k] = s["kernel_launches"]
            if i >= WARM:
                ms[k].append(s["kernel_ms"])
    med = {}
    say(f"a pass on the film of {FIRST} frames, {REPS} calls after {WARM} warm-up:")
    for k in ("plan", "radiance", "fold"):
        med[k], lo, hi = stats(ms[k])
        say(f"  {k:9s} ({launches[k]:2d} launches)   median {med[k]:7.4f} ms   min {lo:7.4f}   max {hi:7.4f}")
    say(f"  plan + fold = {med['plan'] + med['fold']:.4f} ms = {100 * (med['plan'] + med['fold']) / (med['plan'] + med['fold'] + med['radiance']):.1f} % of the pass "
        f"(plan {100 * med['plan'] / (med['plan'] + med['fold'] + med['radiance']):.1f} %, fold {100 * med['fold'] / (med['plan'] + med['fold'] + med['radiance']):.1f} %)")
    # ---- (ii) the error at equal rays -----------------------------------------------------------------------------------------------
    reference = Film(ds, W, H)
    ref_cfg = Config(max_depth=1, seed=1000003)
    for _ in range(REFERENCE):
        reference.add(ref_cfg, stream=stream, jitter=JITTER)
    y_ref = luminance(reference.color.double())
    den = torch.clamp(y_ref, min=0.01)

    def error(f):
        return float(torch.sqrt((((luminance(f.color.double()) - y_ref) / den) ** 2).mean()).item())

    say(f"RMS relative luminance error against a uniform film of {REFERENCE} frames (seed {ref_cfg.seed}), after passes of W x H rays:")
    curves = {}
    for name in ("uniform", "adaptive"):
        f = Film(ds, W, H)
        for _ in range(FIRST):
            f.add(cfg, stream=stream, jitter=JITTER)
        curves[name], got_rays = [(FIRST, error(f))], []
        for k in range(MORE):
            if name == "uniform":
                f.add(cfg, stream=stream, jitter=JITTER)
            else:
                f.add_adaptive(cfg, jitter=JITTER, stream=stream)
                got_rays.append(int((torch.diff(f._buffers["plan"]["offset"].long()) > 0).sum()))
            if (k + 1) % 4 == 0:
                curves[name].append((FIRST + k + 1, error(f)))
        if name == "adaptive":
            counts = torch.diff(f._buffers["plan"]["offset"].long())
            length = f.length
            say(f"  the last plan: rays a pixel min {int(counts.min())}, median {int(counts.median())}, max {int(counts.max())}; "
                f"{int((counts > 0).sum())} of the {n} pixels got rays; history length min {float(length.min()):.0f}, max {float(length.max()):.0f}")
            # where the adaptive film's error sits, by how many samples a pixel has behind it
            sq = ((luminance(f.color.double()) - y_ref) / den) ** 2
            say(f"  pixels that got rays, pass by pass: {got_rays}")
            for lo, hi in ((0, FIRST), (FIRST, FIRST + MORE), (FIRST + MORE, 4 * (FIRST + MORE)), (4 * (FIRST + MORE), 65536), (65536, float("inf"))):
                cls = (length > lo) & (length <= hi)
                if bool(cls.any()):
                    say(f"  history length in ({lo}, {hi}]: {int(cls.sum()):8d} pixels, {float(sq[cls].sum() / sq.sum()):.4f} of the squared error, "
                        f"their own RMS relative error {float(torch.sqrt(sq[cls].mean())):.5f}, mean reference luminance {float(y_ref[cls].mean()):.4f}")
    say("  passes    uniform     adaptive    adaptive / uniform")
    for (p, u), (_, a) in zip(curves["uniform"], curves["adaptive"]):
        say(f"  {p:6d}   {u:9.5f}   {a:9.5f}   {a / u:8.3f}")
    stream.synchronize()
ds.close()
os.makedirs(os.path.dirname(log_path), exist_ok=True)
with open(log_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
