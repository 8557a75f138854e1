"""Surface sampling on device memory: what the table and the draws cost on the atrium (RAYCA_BUILDER_SAH after finish()), beside
the composition of torch kernels a caller had to write without them.
  table    surface_cdf(): three launches (the largest area, the weights, the one-block scan)
  draws    sample_surface() with all four outputs, 2**20 and 2**24 samples, from the kept table
  torch    the same work on a (T, 3, 3) vertex tensor the caller keeps: areas (cross, norm), cumsum, rand, searchsorted, two
           more rand and the fold for the barycentrics, gathers for point and normal.  Its table is f32 sums and its draws come
           from another generator: it is a yardstick for time, not for values.
Medians of 10 (min / max beside them) after 3 warm-up calls, one process: RaycaStats.kernel_ms for the library, a pair of events
around the composition for torch; the machine is shared, so the spread of each row is part of the result and the third digit
of a sub-millisecond window is the scheduler's.  No coarse table in LDS and no wave-uniform first step were built: the rows
below are the plain binary search.
usage: python tests/gpu_sample_probe.py [log file]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi

REPS, WARM = 10, 3
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


scene = scenes.atrium_scene()
ds = DeviceScene(flatten(scene), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
stream = torch.cuda.Stream()
# the caller's copy of the triangles (the atrium's nodes carry no transform: model space is world space); slot order does not matter here
model = scene.models[0]
verts = torch.from_numpy(np.concatenate([g.positions[g.indices.astype(np.int64)].reshape(-1, 3, 3) for g in model.geometries]).astype(np.float32)).cuda()
torch.cuda.synchronize()
say(f"atrium: {info['triangle_count']} triangles; caller's vertex tensor {tuple(verts.shape)}")


def row(label, ms, n=None):
    med = float(np.median(ms))
    rate = f"   {n / med / 1e3:8.1f} M samples/s" if n else ""
    say(f"  {label:52s} median {med:8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}{rate}")


def timed_stats(call):
    ms = []
    for i in range(WARM + REPS):
        st = call()
        if i >= WARM:
            ms.append(st["kernel_ms"])
    return ms


def timed_events(call):
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            call()
            b.record(stream)
        b.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return ms


def torch_table():
    ab, ac = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    return torch.cumsum(torch.linalg.norm(torch.linalg.cross(ab, ac), dim=1), 0)


def torch_draw(cum, n, g):
    target = torch.rand(n, device="cuda", generator=g) * cum[-1]
    prim = torch.searchsorted(cum, target).clamp_(max=cum.numel() - 1)
    s, t = torch.rand(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g)
    fold = s + t > 1
    s, t = torch.where(fold, 1 - s, s), torch.where(fold, 1 - t, t)
    tri = verts[prim]
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    point = tri[:, 0] + ab * s[:, None] + ac * t[:, None]
    nrm = torch.linalg.cross(ab, ac)
    normal = nrm / torch.linalg.norm(nrm, dim=1, keepdim=True)
    uv = torch.stack([1 - s - t, s], 1)
    return prim.int(), uv, point, normal


table = torch.empty(info["triangle_count"] + 1, dtype=torch.int64, device="cuda")
say("table:")
row("surface_cdf() (3 launches)", timed_stats(lambda: ds.surface_cdf(out=table, stream=stream, want_stats=True)[1]))
row("torch: cross, norm, cumsum", timed_events(torch_table))
with torch.cuda.stream(stream):
    cum = torch_table()
gen = torch.Generator(device="cuda").manual_seed(5)
for n in (1 << 20, 1 << 24):
    say(f"{n} samples, prim + uv + point + normal:")
    out = {"prim": torch.empty(n, dtype=torch.int32, device="cuda"), "uv": torch.empty((n, 2), device="cuda"),
           "point": torch.empty((n, 3), device="cuda"), "normal": torch.empty((n, 3), device="cuda")}
    row("sample_surface() (1 launch)", timed_stats(lambda: ds.sample_surface(n, cdf=table, seed=7, out=out, stream=stream, want_stats=True)["stats"]), n)
    row("sample_surface(), prim + uv only", timed_stats(lambda: ds.sample_surface(n, cdf=table, seed=7, want=("prim", "uv"), out={k: out[k] for k in ("prim", "uv")},
                                                                             stream=stream, want_stats=True)["stats"]), n)
    row("torch: rand, searchsorted, barycentrics, gathers", timed_events(lambda: torch_draw(cum, n, gen)), n)
    del out
ds.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
