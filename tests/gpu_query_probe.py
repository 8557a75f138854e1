"""Ray queries on device memory against the host-array entry: kernel time and host wall time, atrium, RAYCA_BUILDER_SAH after
finish(), 2**22 rays of two kinds -- coherent (a 2048 x 2048 pinhole grid from the scene's camera) and incoherent (bounce-like:
origins = hit points of a camera grid, directions random over the hemisphere facing back, as gpu_sort_probe.py makes them).
Medians of 10 (min / max beside them) of RaycaStats.kernel_ms after 3 warm-up calls, one process; the machine is shared, so
the spread of each row is part of the result.
  trace_rays   rayca_hip_trace_rays: k_trace_rays, one ray per lane, host arrays (the baseline)
  closest      rayca_hip_query_device CLOSEST, unbounded: k_query_refill
  occluded     rayca_hip_query_device OCCLUDED, per-ray tmax = t x (0.5 or 2) by one hashed bit: about half the hits occluded
usage: python tests/gpu_query_probe.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi

N, REPS, WARM = 1 << 22, 10, 3
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()


def pinhole(w, h, eye, yfov_deg=60.0):
    """rows of a w x h pinhole grid looking down +x from `eye` (the atrium's camera stands at the -x end)"""
    py, px = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    k = np.tan(np.radians(yfov_deg) / 2)
    u = ((px.reshape(-1) + 0.5) / w * 2 - 1) * k * (w / h)
    v = (1 - (py.reshape(-1) + 0.5) / h * 2) * k
    d = np.stack([np.ones_like(u), v, u], 1).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.tile(np.asarray([eye], np.float32), (d.shape[0], 1)), d], 1).astype(np.float32)


coherent = pinhole(2048, 2048, (-14.0, 2.2, 0.3))
t, prim, _, _ = ds.trace_rays(coherent)
hit = prim != 0xFFFFFFFF
rs = np.random.RandomState(5)
o2 = (coherent[:, :3] + coherent[:, 3:] * (t[:, None] - 1e-3))[hit].astype(np.float32)
d2 = rs.normal(size=(o2.shape[0], 3)).astype(np.float32)
d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
flip = (d2 * coherent[hit, 3:]).sum(1) > 0
d2[flip] *= -1
incoherent = np.concatenate([o2, d2], 1)
incoherent = np.concatenate([incoherent, incoherent[: N - incoherent.shape[0]]], 0)[:N]   # (misses of the grid made up from the front)
print(f"atrium, {N} rays per set; coherent grid: {hit.mean():.3f} hit", flush=True)


def row(label, ms):
    print(f"  {label:34s} median {np.median(ms):8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}", flush=True)


for name, rays in (("coherent", coherent), ("incoherent", incoherent)):
    print(f"{name}:", flush=True)
    ms, wall = [], []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        t, prim, _, st = ds.trace_rays(rays)
        if i >= WARM:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(st["kernel_ms"])
    row("trace_rays kernel (k_trace_rays)", ms)
    row("trace_rays wall, numpy in / out", wall)
    hit = prim != 0xFFFFFFFF
    half = (scenes.hash_u32(7, np.arange(N)) & 1).astype(bool)
    tmax = np.where(hit, t * np.where(half, np.float32(0.5), np.float32(2.0)), np.float32(1.0)).astype(np.float32)
    rays_d, tmax_d = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda()
    out = (torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"),
           torch.empty((N, 2), dtype=torch.float32, device="cuda"))
    mask = torch.empty(N, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ms = []
    for i in range(WARM + REPS):
        *_, st = ds.query(rays_d, out=out, stream=stream, want_stats=True)
        if i >= WARM:
            ms.append(st["kernel_ms"])
    row("closest, unbounded (k_query_refill)", ms)
    same = bool((out[0].cpu().numpy().view(np.uint32) == t.view(np.uint32)).all() and (out[1].cpu().numpy().view(np.uint32) == prim).all())
    ms = []
    for i in range(WARM + REPS):
        _, st = ds.query(rays_d, tmax=tmax_d, kind="occluded", out=mask, stream=stream, want_stats=True)
        if i >= WARM:
            ms.append(st["kernel_ms"])
    row("occluded, per-ray tmax", ms)
    print(f"  (occluded: {float(mask.float().mean()):.3f} of the rays; closest equals trace_rays bit for bit: {same})", flush=True)
    wall = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        ds.query(rays_d, out=out, stream=stream)
        stream.synchronize()
        if i >= WARM:
            wall.append((time.perf_counter() - t0) * 1e3)
    row("query wall, resident tensors + sync", wall)
    *_, st = ds.query(rays_d, out=out, stream=stream, collect_stats=True)
    print(f"  lanes active, k_query_refill: node loop {st['boxes_tested'] / max(1, st['wave_box_slots']):.3f}, "
          f"leaf loop {st['triangles_tested'] / max(1, st['wave_triangle_slots']):.3f}", flush=True)
ds.close()
