"""Ambient occlusion on device memory: the fused entry against today's route, on the atrium's G-buffer (RAYCA_BUILDER_SAH after
finish()) at 960 x 540 with 16 samples per pixel, a radius of 5 % of the scene's diagonal and a per-pixel rotation.
  fused    ambient(want=("open",)): rays made in registers inside k_ambient_refill, then k_ambient_finish
  route    what a host does without it: torch builds the same count x S rays (24 B each) in device memory, query(kind="occluded")
           traces them (k_query_refill), torch reduces the count x S bytes to the openness
Both in the same run, on the same stream; the comparison is against that existing route, never against the new code itself.
Medians of 10 (min / max beside them) after 3 warm-up calls: RaycaStats.kernel_ms of the two native calls, and HIP-event time
around the whole route (ray construction + query + reduction).  The machine is shared, so the spread of each row is part of the
result.  The counters come from one more call each with collect_stats (the counting kernels): the traversal work per ray must be
equal.  The openness images of the two routes are compared bit for bit.  Both sides get the pixels whose camera ray hits: the route
has no notion of an inactive point.
usage: python tests/gpu_ambient_probe.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi
from rayca_amd.ambient import cosine_directions, pixel_rotations

W, H, S, REPS, WARM = 960, 540, 16, 10, 3
N = W * H
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
info = ds.info()
stream = torch.cuda.Stream()

with torch.cuda.stream(stream):
    g = ds.gbuffer(Config(), W, H, want=("point", "normal"), stream=stream)
    p, n = g["point"].reshape(-1, 3).contiguous(), g["normal"].reshape(-1, 3).contiguous()
    hit = g["prim"].reshape(-1) != -1
    # the route has no notion of an inactive point -- it would trace the rays of a miss pixel from the origin, and count their boxes --
    # so both sides get the pixels that hit
    missed = int((~hit).sum())
    p, n = p[hit].contiguous(), n[hit].contiguous()
    N = p.shape[0]
    lo, hi = p.min(0).values, p.max(0).values
    diag = float(torch.linalg.norm(hi - lo))
    radius, bias = 0.05 * diag, 1e-4 * diag
    table = torch.from_numpy(cosine_directions(S)).cuda()
    rot = torch.from_numpy(pixel_rotations(W, H).reshape(-1, 2)).cuda()[hit].contiguous()
stream.synchronize()
print(f"atrium: {info['triangle_count']} triangles, stack need {info['max_depth']}; {W} x {H} G-buffer, {N} pixels hit ({missed} miss and are left out); "
      f"{S} samples, {N * S} rays; diagonal {diag:.3f}, radius {radius:.3f}, bias {bias:.5f}", flush=True)


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
    return torch.cat([o, d], 2).reshape(N * S, 6)


# the same rays from the numpy restatement of the specification (tests/ambient_literal.py): what the counters are compared on, so that
# an operation torch rounds differently shows up as a line of this log and not as a difference in traversal work
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ambient_literal as al
o_l, d_l = al.rays(p.cpu().numpy(), n.cpu().numpy(), rot.cpu().numpy(), table.cpu().numpy(), S, np.float32(bias))
literal_rays = torch.from_numpy(np.concatenate([o_l, d_l], 2).reshape(-1, 6)).cuda()
with torch.cuda.stream(stream):
    differ = int((literal_rays.view(torch.int32) != torch_rays().view(torch.int32)).any(1).sum())
stream.synchronize()
print(f"torch's rays against the numpy restatement's: {differ} of {N * S} differ in some bit", flush=True)

occ = torch.empty(N * S, dtype=torch.uint8, device="cuda")
open_out = torch.empty(N, dtype=torch.float32, device="cuda")


def fused(**o):
    return ds.ambient(p, n, samples=S, radius=radius, bias=bias, dirs=table, rotations=rot, want=("open",), out={"open": open_out}, stream=stream, **o)


mask_out = torch.empty(N, dtype=torch.int64, device="cuda")


def fused_mask(**o):
    """the trace kernel alone (and the clear of the mask words in front of it): mask_out is the only output, no fold is launched"""
    return ds.ambient(p, n, samples=S, radius=radius, bias=bias, dirs=table, rotations=rot, want=("mask",), out={"mask": mask_out}, stream=stream, **o)


def route(rays=None, **o):
    """returns (openness, stats of the query, ms of the whole route); rays: instead of torch's own"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        rays = torch_rays() if rays is None else rays
        r = ds.query(rays, kind="occluded", tmax=radius, out=occ, stream=stream, **o)
        st = r[1] if isinstance(r, tuple) else None
        active = torch.isfinite(p).all(1) & torch.isfinite(n).all(1) & (n != 0).any(1)
        hits = (occ.reshape(N, S) != 0).sum(1) * active
        opened = (S - hits).to(torch.float32) / float(S)
        e1.record(stream)
    stream.synchronize()
    return opened, st, e0.elapsed_time(e1)


def row(label, ms, extra=""):
    med = float(np.median(ms))
    print(f"  {label:52s} median {med:8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}   {N * S / med / 1e3:9.1f} Mrays/s{extra}", flush=True)


f_ms, m_ms, q_ms, r_ms = [], [], [], []
for i in range(WARM + REPS):
    st = fused(want_stats=True)["stats"]
    mst = fused_mask(want_stats=True)["stats"]
    opened, qst, whole = route(want_stats=True)
    if i >= WARM:
        f_ms.append(st["kernel_ms"])
        m_ms.append(mst["kernel_ms"])
        q_ms.append(qst["kernel_ms"])
        r_ms.append(whole)
stream.synchronize()
same = bool((open_out.view(torch.int32) == opened.view(torch.int32)).all())
fst = fused(collect_stats=True)["stats"]
opened, qst, _ = route(rays=literal_rays, collect_stats=True)
same = same and bool((open_out.view(torch.int32) == opened.view(torch.int32)).all())
rays_total = N * S
print(f"openness of the two routes: {'bit-identical' if same else 'DIFFERENT'}; mean openness {float(open_out.mean()):.4f}, {float((open_out < 1).float().mean()):.3f} of the pixels see an occluder", flush=True)
row("fused: ambient(want=('open',)), both kernels", f_ms,
    f"   boxes / ray {fst['boxes_tested'] / rays_total:7.2f}   triangles / ray {fst['triangles_tested'] / rays_total:6.2f}   launches {fst['kernel_launches']}")
row("fused: ambient(want=('mask',)), clear + trace kernel", m_ms, f"   launches {mst['kernel_launches']}")
row("route: query(kind='occluded') alone (k_query_refill)", q_ms,
    f"   boxes / ray {qst['boxes_tested'] / rays_total:7.2f}   triangles / ray {qst['triangles_tested'] / rays_total:6.2f}")
row("route: torch rays + query + torch reduction", r_ms)
print(f"traversal work: boxes {fst['boxes_tested']} against {qst['boxes_tested']}, triangles {fst['triangles_tested']} against {qst['triangles_tested']}: "
      f"{'equal' if (fst['boxes_tested'], fst['triangles_tested']) == (qst['boxes_tested'], qst['triangles_tested']) else 'NOT EQUAL'}", flush=True)
print(f"ray buffer the fused entry never writes or reads: {rays_total * 24 / 1e6:.1f} MB, and {rays_total / 1e6:.1f} MB of per-ray results; "
      f"its inputs: {N * 32 / 1e6:.1f} MB of points, normals and rotations, {S * 12} B of table", flush=True)
spread = max(q_ms) - min(q_ms)
print(f"fused median - query median = {np.median(f_ms) - np.median(q_ms):+.3f} ms, clear + trace kernel - query = {np.median(m_ms) - np.median(q_ms):+.3f} ms; "
      f"the query's own spread (max - min) {spread:.3f} ms", flush=True)
ds.close()
