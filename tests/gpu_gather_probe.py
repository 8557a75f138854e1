"""Irradiance gathering on device memory: the fused entry against the composition it replaces, on the atrium's G-buffer
(RAYCA_BUILDER_SAH after finish()) at 1920 x 1080 with 16 samples per pixel and a per-pixel rotation, Pathtracer depth 1 and depth 3.
  fused    gather(outputs=("irradiance", "sh", "kept")): rays made in registers by k_enqueue_gather, the frame driver, k_gather_fold;
           the per-ray radiance lives in the context's scratch, one internal frame (2^22 rays) at a time
  route    what a host does without it: torch builds the same count x S rays (24 B each) in device memory, radiance() traces them
           (one frame of count x S "pixels"), torch reduces the count x S x 16 B to the same three outputs
Both in the same run, on the same stream, alternating; the comparison is against that existing route, never against the new code
itself.  Medians of REPS (min / max beside them) after WARM warm-up rounds: HIP-event time around each whole call (the fused call is
one native call; the route is ray construction + radiance + reduction).  The machine is shared, so the spread of each row is part of
the result.  Peak extra device memory: the drop of the device's free memory across the first call of each side (work buffers of the
library's frame context, which it keeps, and torch's caching allocator, which keeps its peak), each side on a frame context of its
own, outputs included.  E of the two sides is compared: torch's reduction has another order, so they differ in the last bits.
Both sides get the pixels whose camera ray hits: the route has no notion of an inactive point.
usage: python tests/gpu_gather_probe.py [width height]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi
from rayca_amd.ambient import cosine_directions, pixel_rotations

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
S, REPS, WARM = 16, 5, 2
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
    diag = float(torch.linalg.norm(p.max(0).values - p.min(0).values))
    bias = 1e-4 * diag
    table = torch.from_numpy(cosine_directions(S)).cuda()
    rot = torch.from_numpy(pixel_rotations(W, H).reshape(-1, 2)).cuda()[hit].contiguous()
    del g
stream.synchronize()
torch.cuda.empty_cache()
print(f"atrium: {info['triangle_count']} triangles; {W} x {H} G-buffer, {N} pixels hit ({missed} miss and are left out); {S} samples, {N * S} rays; "
      f"diagonal {diag:.3f}, bias {bias:.5f}", flush=True)


def torch_rays():
    """the specification's rays, in torch f32 (each operation a kernel of its own: nothing is fused, nothing contracted)"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sg = torch.where(nz >= 0, 1.0, -1.0).to(torch.float32)
    a = -1.0 / (sg + nz)
    b = (nx * ny) * a
    t = torch.stack([1.0 + ((sg * nx) * nx) * a, sg * b, (-sg) * nx], 1)
    bt = torch.stack([b, sg + (ny * ny) * a, -ny], 1)
    c, s = rot[:, 0:1], rot[:, 1:2]
    lx, ly, lz = table[:, 0][None], table[:, 1][None], table[:, 2][None]
    rx, ry = c * lx - s * ly, s * lx + c * ly                                 # (N, S)
    d = ((t[:, None, :] * rx[:, :, None]) + (bt[:, None, :] * ry[:, :, None])) + n[:, None, :] * lz[:, :, None]
    o = (p + n * bias)[:, None, :].expand(N, S, 3)
    return torch.cat([o, d], 2).reshape(N * S, 6), d


CONST = torch.tensor([0.2820948, 0.4886025, 0.4886025, 0.4886025, 1.0925484, 1.0925484, 0.3153916, 1.0925484, 0.5462742], dtype=torch.float32, device="cuda")


def torch_fold(L, d):
    """(irradiance (N, 4), sh (N, 9, 4), kept (N,)) by torch reductions over the sample axis"""
    L = L.reshape(N, S, 4)
    ok = torch.isfinite(L[:, :, :3]).all(2)
    c = torch.where(ok[:, :, None], L[:, :, :3], 0.0)
    x, y, z = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    basis = torch.stack([torch.ones_like(x), y, z, x, x * y, y * z, 3.0 * (z * z) - 1.0, x * z, x * x - y * y], 2) * CONST      # (N, S, 9)
    kept = ok.sum(1)
    div = kept.clamp(min=1).to(torch.float32)
    e = c.sum(1) / div[:, None]
    sh = torch.einsum("nsk,nsc->nkc", basis, c) / div[:, None, None]
    return torch.cat([e, (kept.to(torch.float32) / S)[:, None]], 1), torch.cat([sh, torch.zeros((N, 9, 1), device="cuda")], 2), kept.to(torch.int32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        r = fn()
        e1.record(stream)
    stream.synchronize()
    return r, e0.elapsed_time(e1)


def extra_memory(fn):
    """the drop of the device's free memory across fn's first call, in MB (what the library and torch's allocator keep afterwards is
    what the call needed at its peak: neither gives memory back)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    r, _ = timed(fn)
    free1 = torch.cuda.mem_get_info()[0]
    return r, (free0 - free1) / 1e6


def row(label, ms, extra=""):
    med = float(np.median(ms))
    print(f"  {label:58s} median {med:9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   {N * S / med / 1e3:8.1f} Mrays/s{extra}", flush=True)


# (each side of each Config on a frame context of its own, so that the memory a first call takes is that Config's alone)
for name, cfg, ctx_fused, ctx_route in (("Pathtracer depth 1", Config(max_depth=1), 1, 2), ("Pathtracer depth 3", Config(max_depth=3), 3, 4)):
    def fused():
        return ds.gather(p, n, cfg, samples=S, bias=bias, dirs=table, rotations=rot, outputs=("irradiance", "sh", "kept"), stream=stream, context=ctx_fused)

    def route():
        rays, d = torch_rays()
        L = ds.radiance(rays, cfg, stream=stream, context=ctx_route)
        return torch_fold(L, d)

    print(f"{name}:", flush=True)
    got, fused_mb = extra_memory(fused)
    want, route_mb = extra_memory(route)
    f_ms, r_ms = [], []
    for i in range(WARM + REPS):
        got, fm = timed(fused)
        want, rm = timed(route)
        if i >= WARM:
            f_ms.append(fm)
            r_ms.append(rm)
    st = ds.gather(p, n, cfg, samples=S, bias=bias, dirs=table, rotations=rot, outputs=("irradiance",), stream=stream, context=ctx_fused, want_stats=True)["stats"]
    e_f, e_r = got["irradiance"][:, :3].double(), want[0][:, :3].double()
    rel = float(((e_f - e_r).abs() / e_r.abs().clamp(min=1e-3)).max())
    same_kept = bool((got["kept"] == want[2]).all())
    row("fused: gather(irradiance, sh, kept), one native call", f_ms, f"   frames {st['rows_rendered']}   launches {st['kernel_launches']}   kernel_ms {st['kernel_ms']:.3f}")
    row("route: torch rays + radiance + torch reduction", r_ms)
    print(f"  peak extra device memory (first call, outputs included): fused {fused_mb:9.1f} MB, route {route_mb:9.1f} MB", flush=True)
    print(f"  E of the two sides: largest relative difference {rel:.3g} (another summation order); kept {'equal' if same_kept else 'DIFFERENT'}; "
          f"mean E {[round(float(v), 5) for v in e_f.mean(0)]}", flush=True)
    print(f"  fused median / route median = {np.median(f_ms) / np.median(r_ms):.3f}", flush=True)
    del got, want
ds.close()
