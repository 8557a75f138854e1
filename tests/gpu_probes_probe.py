"""Irradiance volumes on device memory: what a probe lookup costs and how far it is from the gather it stands in for, on the atrium's
G-buffer (RAYCA_BUILDER_SAH after finish()) at 1920 x 1080.  A grid of GRID probes around the points the camera sees is baked once
by ProbeGrid.bake (Pathtracer depth 1, BAKE_S samples a probe); then, on the pixels whose camera ray hits:
  lookup   probe_lookup(outputs=("irradiance", "mask")) with visibility (eight corner rays a pixel, k_probe_refill, then k_probe_fold)
           and without (k_probe_fold alone), normal term on in both
  gather   gather(samples=16, cosine directions, a per-pixel rotation) at depth 1 on the same points: what render_irradiance runs
           behind its G-buffer, the per-pixel measurement the lookup replaces
All on one stream in one process; medians of REPS (min / max beside them) after WARM warm-up rounds of HIP-event time around each
whole call.  The machine is shared, so the spread of each row is part of the result.  Also: the share of pixels that take the
fallback, and the relative difference of irradiance x (1 / pi) against that gather's E (cosine directions, no weights: E is the
irradiance / pi), |a - b| / max(|b|, 1e-3) per channel -- the lookup is an interpolation of a band-limited bake, the gather a
16-sample estimate: the difference is the error of both, not of the kernels.
usage: python tests/gpu_probes_probe.py [width height]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi
from rayca_amd.ambient import cosine_directions, pixel_rotations
from rayca_amd.probes import ProbeGrid

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
GRID, BAKE_S, S, REPS, WARM = (16, 8, 16), 64, 16, 7, 2
cfg = Config(max_depth=1)
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
stream = torch.cuda.Stream()

with torch.cuda.stream(stream):
    g = ds.gbuffer(Config(), W, H, want=("point", "normal"), stream=stream)
    p, n = g["point"].reshape(-1, 3).contiguous(), g["normal"].reshape(-1, 3).contiguous()
    hit = g["prim"].reshape(-1) != -1
    missed = int((~hit).sum())
    p, n = p[hit].contiguous(), n[hit].contiguous()
    N = p.shape[0]
    lo, hi = p.min(0).values.cpu().numpy(), p.max(0).values.cpu().numpy()
    diag = float(np.linalg.norm(hi - lo))
    bias = 1e-3 * diag
    table = torch.from_numpy(cosine_directions(S)).cuda()
    rot = torch.from_numpy(pixel_rotations(W, H).reshape(-1, 2)).cuda()[hit].contiguous()
    del g
stream.synchronize()
grid = ProbeGrid.around(lo, hi, GRID, margin=0.01 * diag)
print(f"atrium: {info['triangle_count']} triangles; {W} x {H} G-buffer, {N} pixels hit ({missed} miss and are left out); diagonal {diag:.3f}, "
      f"bias {bias:.5f}; grid {GRID} = {grid.count} probes, cell {[round(float(c), 4) for c in grid.cell]}", flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        r = fn()
        e1.record(stream)
    stream.synchronize()
    return r, e0.elapsed_time(e1)


def row(label, ms, rays, extra=""):
    med = float(np.median(ms))
    print(f"  {label:58s} median {med:9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   {rays / med / 1e3:8.1f} Mrays/s{extra}", flush=True)


(sh, kept), bake_ms = timed(lambda: grid.bake(ds, cfg, samples=BAKE_S, stream=stream))
print(f"  bake: {grid.count} probes x {BAKE_S} samples, depth 1: {bake_ms:.3f} ms (first call); {int((kept == 0).sum())} probes without a finite sample", flush=True)


def lookup(visibility):
    return ds.probe_lookup(p, n, grid, sh, kept=kept, visibility=visibility, bias=bias, outputs=("irradiance", "mask"), stream=stream, context=1)


def gather():
    return ds.gather(p, n, cfg, samples=S, bias=bias, dirs=table, rotations=rot, outputs=("irradiance",), stream=stream, context=2)


ms = {"vis": [], "fold": [], "gather": []}
for i in range(WARM + REPS):
    for key, fn in (("vis", lambda: lookup(True)), ("fold", lambda: lookup(False)), ("gather", gather)):
        r, t = timed(fn)
        if i >= WARM:
            ms[key].append(t)
        if key == "vis":
            with_vis = r
        elif key == "fold":
            without = r
        else:
            ref = r
st = ds.probe_lookup(p, n, grid, sh, kept=kept, bias=bias, outputs=("irradiance",), stream=stream, context=1, want_stats=True)["stats"]
row("probe_lookup, visibility + normal term (8 rays a pixel)", ms["vis"], N * 8, f"   launches {st['kernel_launches']}   kernel_ms {st['kernel_ms']:.3f}")
row("probe_lookup, normal term alone (no rays: the fold)", ms["fold"], 0)
row(f"gather, {S} samples a pixel, depth 1", ms["gather"], N * S)
print(f"  lookup with visibility / gather = {np.median(ms['vis']) / np.median(ms['gather']):.4f}; without / gather = {np.median(ms['fold']) / np.median(ms['gather']):.4f}", flush=True)
inv_pi = 0.31830987
e_ref = ref["irradiance"][:, :3].double()
for label, r in (("with visibility", with_vis), ("without visibility", without)):
    mask = r["mask"]
    fb = float(((mask >> 16) & 1).double().mean())
    occ = float(sum(((mask >> (8 + k)) & 1).double().sum() for k in range(8)) / max(float(sum(((mask >> k) & 1).double().sum() for k in range(8))), 1.0))
    e = r["irradiance"][:, :3].double() * inv_pi
    rel = (e - e_ref).abs() / e_ref.abs().clamp(min=1e-3)
    print(f"  {label}: fallback pixels {fb:.4f}; candidate rays occluded {occ:.4f}; irradiance / pi against the gather: mean relative difference {float(rel.mean()):.4f}, "
          f"max {float(rel.max()):.3f}; mean E {[round(float(v), 5) for v in e.mean(0)]} against {[round(float(v), 5) for v in e_ref.mean(0)]}", flush=True)
ds.close()
