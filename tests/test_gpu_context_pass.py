"""The protocol every pass on a frame context follows (ContextPass in rayca_amd/csrc/api.inc), seen from outside: a query, a
surface call, the camera-ray export and the denoiser start behind RaycaRenderOptions.wait_event and leave record_event behind
their last launch, as a frame does (tests/test_gpu_multi.py); and rayca_hip_trace_rays queues behind a frame in flight on
context 0, whose buffers it shares; a frame that has to regrow the context's buffers waits for the frame in flight on them.  The
Cornell room, 64 x 36: 2304 rays, hit records and pixels."""
import ctypes as C

import numpy as np
import pytest

from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi, flatten, lib, scenes

pytestmark = pytest.mark.gpu
W, H = 64, 36
N = W * H
FLAT = Config(integrator=IntegratorStrategy.Flat)
SURFACE = ("point", "normal", "color", "material", "flags")


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


@pytest.fixture(scope="module")
def room(gpu):
    """The scene and, made once by the synchronous form of each call, the inputs of the four passes and what they give."""
    import torch
    ds = DeviceScene(flatten(scenes.cornell_scene()), Config(), builder=abi.BUILDER_SAH)
    r = {"ds": ds, "rays": ds.camera_rays(FLAT, W, H)}
    r["t"], r["prim"], r["uv"] = ds.query(r["rays"])
    r["surface"] = ds.surface(r["rays"], r["t"], r["prim"], r["uv"], want=SURFACE)
    rng = np.random.default_rng(7)
    r["color"] = torch.from_numpy(rng.uniform(0.0, 2.0, size=(H, W, 4)).astype(np.float32)).cuda()
    r["denoised"] = ds.denoise(r["color"], iterations=2)
    torch.cuda.synchronize()
    assert int((r["prim"] != -1).sum()) > N // 2   # the room fills the frame: zeroed inputs give other results
    yield r
    ds.close()


@pytest.mark.parametrize("entry", ["query", "surface", "camera_rays", "denoise"])
def test_every_pass_waits_for_and_records_the_callers_events(room, entry):
    """The pass must not start before the event it waits for -- recorded behind a long fill on another stream and the writes of
    the pass's inputs (for the export, which has none, of its output) -- and the event it records must cover it: a copy on a
    third stream that waits for that event alone sees the finished outputs, bit for bit those of the synchronous call."""
    import torch
    ds, gpu = room["ds"], lib.load()
    s_fill, s_pass, s_copy = (torch.cuda.Stream() for _ in range(3))
    big = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    ev_filled, ev_pass = torch.cuda.Event(), torch.cuda.Event()
    ev_filled.record(s_fill)   # (torch makes an event's handle at its first record)
    ev_pass.record(s_pass)
    o = ds._opts(0, False, None, s_pass.cuda_stream, context=1)
    o.wait_event, o.record_event = ev_filled.cuda_event, ev_pass.cuda_event
    if entry == "query":
        good, want = [room["rays"]], [room["t"], room["prim"], room["uv"]]
    elif entry == "surface":
        good, want = [room[k] for k in ("rays", "t", "prim", "uv")], [room["surface"][k] for k in SURFACE]
    elif entry == "camera_rays":
        good, want = [], [room["rays"]]
    else:
        good, want = [room["color"]], [room["denoised"]]
    inputs = [torch.zeros_like(x) for x in good]
    outputs = [torch.zeros_like(x) for x in want]
    ptr = [x.data_ptr() for x in inputs]
    out = [x.data_ptr() for x in outputs]
    if entry == "query":
        q = abi.RaycaQuery()
        q.kind, q.count, q.rays, q.tmax_all = abi.QUERY_CLOSEST, N, ptr[0], float("inf")
        q.t_out, q.prim_out, q.uv_out = out
        call = lambda: gpu.rayca_hip_query_device(ds.handle, C.byref(o), C.byref(q), None)
    elif entry == "surface":
        q = abi.RaycaSurfaceQuery()
        q.count, q.rays, q.t, q.prim, q.uv = N, *ptr
        for name, p in zip(SURFACE, out):
            setattr(q, name + "_out", p)
        call = lambda: gpu.rayca_hip_surface_device(ds.handle, C.byref(o), C.byref(q), None)
    elif entry == "camera_rays":
        cfg = FLAT.to_abi()
        call = lambda: gpu.rayca_hip_camera_rays_device(ds.handle, C.byref(cfg), W, H, 0, C.byref(o), out[0])
    else:
        d = abi.RaycaDenoise()
        d.width, d.height, d.iterations, d.normal_power_log2, d.sigma_color, d.gamma = W, H, 2, 7, 4.0, 1.0
        d.color, d.rgba32f_out = ptr[0], out[0]
        call = lambda: gpu.rayca_hip_denoise_device(ds.handle, C.byref(o), C.byref(d), None)
    torch.cuda.synchronize()
    with torch.cuda.stream(s_fill):
        big.fill_(7)                  # 256 MiB of writes in front of ...
        for x, g in zip(inputs, good):
            x.copy_(g)                # ... the writes the pass has to come after
        if not inputs:
            outputs[0].fill_(9.0)
        ev_filled.record(s_fill)
    lib.check(call())
    with torch.cuda.stream(s_copy):
        s_copy.wait_event(ev_pass)
        got = [x.clone() for x in outputs]
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g), bits(w)), (entry, k)


def test_trace_rays_behind_a_frame_in_flight(room):
    """A depth-1 frame issued on a side stream on context 0, held back by a fill, and rayca_hip_trace_rays straight behind it: the
    rays come back as on an idle scene and the frame as rendered alone.  (The binary tree of this scene needs no spill area, so
    nothing is regrown under the frame: a comparison of results, not a race detector.)"""
    import torch
    ds = room["ds"]
    assert ds.info()["max_depth"] + 1 < 24   # the node stack fits the LDS part
    w, h = 256, 144
    cfg = Config(max_depth=1)
    rays = room["rays"].cpu().numpy()
    t0, prim0, uv0, st0 = ds.trace_rays(rays)
    alone = ds.render(cfg, w, h, want_f32=False)[0]
    s_fill, s_frame = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    frame = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    ev_filled = torch.cuda.Event()
    ev_filled.record(s_fill)
    torch.cuda.synchronize()
    issue = ds.prepare_device(cfg, w, h, frame.data_ptr(), 0, stream=s_frame.cuda_stream, context=0, wait_event=ev_filled.cuda_event)
    with torch.cuda.stream(s_fill):
        big.fill_(7)
        frame.fill_(9)
        ev_filled.record(s_fill)
    issue()
    t1, prim1, uv1, st1 = ds.trace_rays(rays)
    torch.cuda.synchronize()
    assert np.array_equal(t1.view(np.uint32), t0.view(np.uint32)) and np.array_equal(prim1, prim0)
    assert np.array_equal(uv1.view(np.uint32), uv0.view(np.uint32))
    assert int((prim0 != abi.NONE).sum()) > N // 2
    assert (st1["rays_primary"], st1["kernel_launches"], st1["trace_kernel_launches"]) == (N, 1, 1) and st1["kernel_ms"] > 0
    assert (st1["boxes_tested"], st1["triangles_tested"]) == (st0["boxes_tested"], st0["triangles_tested"])
    assert np.array_equal(frame.cpu().numpy(), alone)


def test_a_larger_frame_behind_a_smaller_one_held_back_on_the_same_context(room):
    """A depth-2 frame at 64 x 36 on a side stream on context 0 of a new scene, held back by a fill, and a depth-2 frame at 256 x 144 on
    a second stream and the same context straight behind it: the second has to replace the path records and both queues, which
    the first has not even started to use.  Regrowing waits for the context's earlier pass (grow_behind_pass), so both frames
    are the ones rendered alone.  A comparison of results, as above."""
    import torch
    cfg = Config(max_depth=2)
    sizes = ((W, H), (256, 144))
    alone = [room["ds"].render(cfg, w, h, want_f32=False)[0] for w, h in sizes]   # (the same scene: built the same way from the same description)
    ds = DeviceScene(flatten(scenes.cornell_scene()), Config(), builder=abi.BUILDER_SAH)   # context 0 has no buffers yet
    s_fill, s_small, s_large = (torch.cuda.Stream() for _ in range(3))
    big = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    frames = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for w, h in sizes]
    ev_filled = torch.cuda.Event()
    ev_filled.record(s_fill)
    torch.cuda.synchronize()
    issue_small = ds.prepare_device(cfg, *sizes[0], frames[0].data_ptr(), 0, stream=s_small.cuda_stream, context=0, wait_event=ev_filled.cuda_event)
    issue_large = ds.prepare_device(cfg, *sizes[1], frames[1].data_ptr(), 0, stream=s_large.cuda_stream, context=0)
    with torch.cuda.stream(s_fill):
        big.fill_(7)
        frames[0].fill_(9)
        ev_filled.record(s_fill)
    issue_small()
    issue_large()
    torch.cuda.synchronize()
    for frame, want in zip(frames, alone):
        assert np.array_equal(frame.cpu().numpy(), want)
    ds.close()
