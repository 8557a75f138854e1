"""Multi-hit ray queries on device memory: kernel time, rays per second and boxes / triangles priced per ray, on the atrium
(RAYCA_BUILDER_SAH after finish()), 2**20 rays of the two kinds tests/gpu_query_probe.py times:
  coherent    a 1024 x 1024 pinhole grid from the scene's camera
  incoherent  bounce-like: from the grid's hit points into random directions of the hemisphere the ray came from
Per kind: RAYCA_HITS_FRONT at k = 1, 4, 16, RAYCA_HITS_BOTH at k = 4, and count_all with k = 0 (k_hits, one ray per lane on the
binary f32 nodes).  Beside them, in the same run, the yardsticks: query(kind="closest") for k = 1, and what a caller had before
this entry for k = 4 -- four successive closest-hit queries, each restarted 10^-4 of the scene's diagonal past the previous hit
(the sum of the four kernel times; the restart arithmetic between them is not counted).  Ratios against the yardsticks at the end
of each block.  Medians of 10 (min / max beside them) of RaycaStats.kernel_ms after 3 warm-up calls, one process; the machine is
shared, so the spread of each row is part of the result.  The counters come from one more call with collect_stats.
usage: python tests/gpu_hits_probe.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi

SIDE, REPS, WARM = 1024, 10, 3
N = SIDE * SIDE
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
stream = torch.cuda.Stream()


def pinhole(w, h, eye, yfov_deg=60.0):
    """rows of a w x h pinhole grid looking down +x from `eye` (the atrium's camera stands at the -x end)"""
    py, px = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    k = np.tan(np.radians(yfov_deg) / 2)
    u = ((px.reshape(-1) + 0.5) / w * 2 - 1) * k * (w / h)
    v = (1 - (py.reshape(-1) + 0.5) / h * 2) * k
    d = np.stack([np.ones_like(u), v, u], 1).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.tile(np.asarray([eye], np.float32), (d.shape[0], 1)), d], 1).astype(np.float32)


coherent_np = pinhole(SIDE, SIDE, (-14.0, 2.2, 0.3))
coherent = torch.from_numpy(coherent_np).cuda()
t, prim, uv = ds.query(coherent, stream=stream)
stream.synchronize()
t_np, hit = t.cpu().numpy(), prim.cpu().numpy() != -1
rs = np.random.RandomState(5)
o2 = (coherent_np[:, :3] + coherent_np[:, 3:] * (t_np[:, None] - 1e-3))[hit].astype(np.float32)
d2 = rs.normal(size=(o2.shape[0], 3)).astype(np.float32)
d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
flip = (d2 * coherent_np[hit, 3:]).sum(1) > 0
d2[flip] *= -1
incoherent_np = np.concatenate([o2, d2], 1)
incoherent_np = np.concatenate([incoherent_np, incoherent_np[: N - incoherent_np.shape[0]]], 0)[:N]   # (misses of the grid made up from the front)
incoherent = torch.from_numpy(np.ascontiguousarray(incoherent_np)).cuda()
pts = (coherent_np[:, :3] + coherent_np[:, 3:] * t_np[:, None])[hit]
diag = float(np.linalg.norm(pts.max(0) - pts.min(0)))
step = 1e-4 * diag
print(f"atrium: {info['triangle_count']} triangles, stack need {info['max_depth']}; {N} rays per set; coherent grid: {hit.mean():.3f} hit; "
      f"diagonal of the hit points {diag:.3f}, restart step {step:.5f}", flush=True)


def row(label, ms, extra=""):
    med = float(np.median(ms))
    print(f"  {label:52s} median {med:8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}   {N / med / 1e3:8.1f} Mrays/s{extra}", flush=True)
    return med


def timed(call):
    ms = []
    for i in range(WARM + REPS):
        ms.append(call())
    return ms[WARM:]


def hits_call(rays, k, out, **kw):
    return lambda: ds.hits(rays, k, stream=stream, out=out, outputs=tuple(out), want_stats=True, **kw)["stats"]["kernel_ms"]


def four_closest(rays, qout):
    """what a caller had: closest hit, restart past it, four times; the sum of the four kernel times"""
    cur, total = rays, 0.0
    for _ in range(4):
        *rec, st = ds.query(cur, stream=stream, out=qout, want_stats=True)
        total += st["kernel_ms"]
        tt = torch.where(rec[1] != -1, rec[0], torch.zeros_like(rec[0]))
        cur = torch.cat([cur[:, :3] + cur[:, 3:] * (tt[:, None] + step), cur[:, 3:]], 1).contiguous()
    return total


qout = (torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty((N, 2), dtype=torch.float32, device="cuda"))
for name, rays in (("coherent", coherent), ("incoherent", incoherent)):
    print(f"{name}:", flush=True)
    med = {}
    for label, k, kw in (("FRONT, k = 1", 1, {}), ("FRONT, k = 4", 4, {}), ("FRONT, k = 16", 16, {}), ("BOTH, k = 4", 4, dict(faces="both")),
                         ("count_all, k = 0 (FRONT)", 0, dict(count_all=True))):
        out = {"n": torch.empty(N, dtype=torch.int32, device="cuda")}
        if k:
            out.update(t=torch.empty((N, k), dtype=torch.float32, device="cuda"), prim=torch.empty((N, k), dtype=torch.int32, device="cuda"),
                       uv=torch.empty((N, k, 2), dtype=torch.float32, device="cuda"), face=torch.empty((N, k), dtype=torch.uint8, device="cuda"))
        ms = timed(hits_call(rays, k, out, **kw))
        st = ds.hits(rays, k, stream=stream, out=out, outputs=tuple(out), collect_stats=True, **kw)["stats"]
        med[label] = row(label, ms, f"   boxes / ray {st['boxes_tested'] / N:7.1f}   triangles / ray {st['triangles_tested'] / N:7.1f}   hits / ray {float(out['n'].float().mean()):6.2f}")
    ms = timed(lambda: ds.query(rays, stream=stream, out=qout, want_stats=True)[-1]["kernel_ms"])
    st = ds.query(rays, stream=stream, out=qout, collect_stats=True)[-1]
    med["closest"] = row('yardstick: query(kind="closest")', ms, f"   boxes / ray {st['boxes_tested'] / N:7.1f}   triangles / ray {st['triangles_tested'] / N:7.1f}")
    med["four"] = row("yardstick: 4 x closest, restarted past the hit", timed(lambda: four_closest(rays, qout)))
    print(f"  ratios: FRONT k = 1 / closest {med['FRONT, k = 1'] / med['closest']:.2f}   FRONT k = 4 / four closest {med['FRONT, k = 4'] / med['four']:.2f}   "
          f"BOTH k = 4 / four closest {med['BOTH, k = 4'] / med['four']:.2f}   k = 16 / k = 1 {med['FRONT, k = 16'] / med['FRONT, k = 1']:.2f}   "
          f"count_all / k = 1 {med['count_all, k = 0 (FRONT)'] / med['FRONT, k = 1']:.2f}", flush=True)
ds.close()
