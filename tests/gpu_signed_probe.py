"""Signed distance on device memory: the fused entry against the composition of the shipped entries, on a 512 x 256 torus
(262 144 triangles, RAYCA_BUILDER_SAH after finish()) and the 128^3 points of a grid around it, three directions.
  fused        signed(grid=..., outputs=("dist2", "inside")): one launch of k_signed, the points made in registers
  composition  what a host does without it: nearest() on a point buffer (made once, outside the timed window: the composition has
               no grid source), torch builds a (N, 6) ray tensor per direction, hits(k=0, count_all) counts along each -- "both"
               alone for parity, "front" and "both" for winding -- and torch votes
  occupancy    occupancy(grid=...): the rays and the vote alone, against the same composition without nearest()
All in one process, on one stream, alternating; the comparison is against the shipped entries, never against the new code itself.
Medians of 20 (min / max beside them) after 3 warm-up rounds, HIP-event time around each whole route.  The machine is shared, so the
spread of each row is part of the result.  The outputs of the two routes are compared bit for bit, and the traversal work of one
more call each with collect_stats (the counting kernels) is printed.
usage: python tests/gpu_signed_probe.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import signed_cases as sc
from rayca_amd import Config, DeviceScene, abi, flatten
from rayca_amd.signed import grid_points, sign_directions

NU, NV, G, REPS, WARM = 512, 256, 128, 20, 3
DIMS = (G, G, G)
LO, HI = np.array([-0.95, -0.95, -0.35]), np.array([0.95, 0.95, 0.35])
ORIGIN, STEP = tuple(LO), tuple((HI - LO) / (G - 1))
N = G ** 3
GRID = (ORIGIN, STEP, DIMS)
dirs = sign_directions(3)

ds = DeviceScene(flatten(sc._scene(*sc.torus_mesh(NU, NV))), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
stream = torch.cuda.Stream()
points = torch.from_numpy(grid_points(*GRID)).cuda()
dirs_d = [torch.from_numpy(d.copy()).cuda() for d in dirs]
print(f"torus {NU} x {NV}: {info['triangle_count']} triangles, stack need {info['max_depth']}; grid {G}^3 = {N} points in {LO} .. {HI}; "
      f"{len(dirs)} directions, {N * len(dirs)} rays", flush=True)

out_f = {"dist2": torch.empty(N, dtype=torch.float32, device="cuda"), "inside": torch.empty(N, dtype=torch.uint8, device="cuda")}
occ_f = torch.empty(N, dtype=torch.uint8, device="cuda")
d2_c = torch.empty(N, dtype=torch.float32, device="cuda")
n_c = [[torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(2)] for _ in dirs]


def fused(rule, **o):
    return ds.signed(grid=GRID, dirs=3, rule=rule, outputs=("dist2", "inside"), out=out_f, stream=stream, **o)


def fused_occupancy(rule, **o):
    return ds.occupancy(grid=GRID, dirs=3, rule=rule, out=occ_f, stream=stream, **o)


def composition(rule, nearest=True, **o):
    """(inside, stats of the native calls or None)"""
    stats = []
    if nearest:
        r = ds.nearest(points, out=(d2_c, False, False, False), stream=stream, **o)
        stats.append(r[-1] if o else None)
    votes = torch.zeros(N, dtype=torch.int32, device="cuda")
    for j, d in enumerate(dirs_d):
        rays = torch.cat([points, d.expand(N, 3)], 1)                       # 24 B per point written, and read again by the kernel
        both = ds.hits(rays, 0, faces="both", count_all=True, outputs=("n",), out={"n": n_c[j][1]}, stream=stream, **o)
        stats.append(both.get("stats"))
        if rule == "winding":
            front = ds.hits(rays, 0, faces="front", count_all=True, outputs=("n",), out={"n": n_c[j][0]}, stream=stream, **o)
            stats.append(front.get("stats"))
            votes += ((both["n"] - front["n"]) > front["n"]).to(torch.int32)
        else:
            votes += both["n"] & 1
    return (2 * votes > len(dirs_d)).to(torch.uint8), stats


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        r = fn()
        e1.record(stream)
    stream.synchronize()
    return r, e0.elapsed_time(e1)


def row(label, ms, extra=""):
    med = float(np.median(ms))
    print(f"  {label:66s} median {med:8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}   {N / med / 1e3:8.1f} Mpoints/s{extra}", flush=True)
    return med


ok = True
for rule in ("parity", "winding"):
    t = {k: [] for k in ("fused", "comp", "occ", "occ_comp")}
    for i in range(WARM + REPS):
        _, a = timed(lambda: fused(rule))
        (inside_c, _), b = timed(lambda: composition(rule))
        _, c = timed(lambda: fused_occupancy(rule))
        (occ_c, _), d = timed(lambda: composition(rule, nearest=False))
        if i >= WARM:
            for k, v in zip(t, (a, b, c, d)):
                t[k].append(v)
    same = (bool((out_f["dist2"].view(torch.int32) == d2_c.view(torch.int32)).all()) and bool((out_f["inside"] == inside_c).all())
            and bool((occ_f == occ_c).all()) and bool((occ_f == out_f["inside"]).all()))
    ok = ok and same
    inside_share = float(out_f["inside"].float().mean())
    with torch.cuda.stream(stream):
        fst = fused(rule, collect_stats=True)["stats"]
        _, cst = composition(rule, collect_stats=True)
    stream.synchronize()
    launches = len(cst)
    cb, ct = sum(s["boxes_tested"] for s in cst), sum(s["triangles_tested"] for s in cst)
    print(f"{rule}: outputs of the two routes {'bit-identical' if same else 'DIFFERENT'}; {inside_share:.4f} of the grid inside "
          f"(the torus fills {2 * np.pi ** 2 * sc.TORUS_R * sc.TORUS_r ** 2 / np.prod(HI - LO):.4f} of the box)", flush=True)
    f = row(f"fused: signed(grid, outputs=('dist2', 'inside')), 1 launch", t["fused"],
            f"   boxes / point {fst['boxes_tested'] / N:7.2f}   triangles / point {fst['triangles_tested'] / N:6.2f}")
    c = row(f"composition: nearest + 3 ray builds + {launches - 1} hits + vote, {launches} native launches", t["comp"],
            f"   boxes / point {cb / N:7.2f}   triangles / point {ct / N:6.2f}")
    o = row("fused: occupancy(grid), 1 launch", t["occ"])
    oc = row(f"composition without nearest: 3 ray builds + {launches - 1} hits + vote", t["occ_comp"])
    spread = (max(t["comp"]) - min(t["comp"])) / c
    print(f"  fused / composition = {f / c:.3f} (gate: at most 1.05: {'met' if f <= 1.05 * c else 'NOT MET'}); occupancy / its composition = {o / oc:.3f}; "
          f"the composition's own spread (max - min) / median = {spread:.3f}", flush=True)
    print(f"  ray tensors the fused entry never writes or reads: {len(dirs) * N * 24 / 1e6:.1f} MB; the point buffer a grid call does not read: {N * 12 / 1e6:.1f} MB", flush=True)
ds.close()
sys.exit(0 if ok else 1)
