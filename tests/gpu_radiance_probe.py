"""Radiance along caller-supplied rays against the frame that traces the same rays: atrium, 1920 x 1080, RAYCA_BUILDER_SAH after
finish(), Pathtracer max_depth=1 and the default Config (max_depth=5).  Medians of 10 (min / max beside them) of
RaycaStats.kernel_ms after 3 warm-up calls, each call on a stream of its own and waited for; the machine is shared, so the
spread of each row is part of the result.
  (a) radiance, camera rays    DeviceScene.radiance on camera_rays() of the frame: rayca_hip_radiance_device
  (b) frame, wavefront / fused render_device(engine=ENGINE_WAVEFRONT / ENGINE_FUSED) of the same Config
  (c) radiance, shuffled       the same rays in a random order (the outputs are the frame's pixels in that order)
  (d) classes                  RaycaStats.class_ms of (a), (b) wavefront and (c): "other" holds the pass that queues the rays
                               (and k_resolve)
With --tree DIR the package and its library are taken from DIR, a built checkout of another commit: where that commit has no
radiance() only (b) is measured -- the frame kernels of the commit this one is compared with, on the same machine.
usage: python tests/gpu_radiance_probe.py [--tree DIR]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
import numpy as np
import torch
from rayca_amd import Config, DeviceScene, flatten, scenes, abi

W, H, REPS, WARM = 1920, 1080, 10, 3
ds = DeviceScene(flatten(scenes.atrium_scene()), Config(), builder=abi.BUILDER_SAH)
ds.finish()
has_radiance = hasattr(ds, "radiance")
print(f"tree {ROOT}: atrium {W} x {H}, radiance() {'present' if has_radiance else 'absent: frames only'}", flush=True)
stream = torch.cuda.Stream()
frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
out = torch.empty((H * W, 4), dtype=torch.float32, device="cuda")
medians = {}


def measure(label, call):
    ms, classes = [], []
    for i in range(WARM + REPS):
        st = call()
        if i >= WARM:
            ms.append(st["kernel_ms"])
            classes.append(st["class_ms"])
    medians[label] = float(np.median(ms))
    print(f"  {label:30s} median {np.median(ms):8.3f} ms   min {min(ms):8.3f}   max {max(ms):8.3f}", flush=True)
    return np.median(np.asarray(classes), axis=0)


def show_classes(label, cls):
    print(f"    classes, {label}: " + "  ".join(f"{n} {v:.3f}" for n, v in zip(abi.KERNEL_NAMES, cls) if v > 0), flush=True)


for cfg, name in ((Config(max_depth=1), "max_depth=1"), (Config(), "default Config (max_depth=5)")):
    print(f"{name}:", flush=True)
    for _ in range(20):   # past the fused engine's node-format calibration on this scene
        ds.render_device(cfg, W, H, 0, frame.data_ptr(), stream=stream.cuda_stream, engine=abi.ENGINE_FUSED)
    torch.cuda.synchronize()
    cls_w = measure("(b) frame, wavefront", lambda: ds.render_device(cfg, W, H, 0, frame.data_ptr(), stream=stream.cuda_stream, engine=abi.ENGINE_WAVEFRONT, want_stats=True))
    measure("(b) frame, fused", lambda: ds.render_device(cfg, W, H, 0, frame.data_ptr(), stream=stream.cuda_stream, engine=abi.ENGINE_FUSED, want_stats=True))
    show_classes("frame, wavefront", cls_w)
    if not has_radiance:
        continue
    rays = ds.camera_rays(Config(samples_per_pixel=1), W, H)
    perm = torch.randperm(H * W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    shuffled = rays[perm].contiguous()
    torch.cuda.synchronize()
    cls_a = measure("(a) radiance, camera rays", lambda: ds.radiance(rays, cfg, out=out, stream=stream, want_stats=True)[1])
    same = bool(torch.equal(out.view(torch.int32), frame.view(-1, 4).view(torch.int32)))
    cls_c = measure("(c) radiance, shuffled rays", lambda: ds.radiance(shuffled, cfg, out=out, stream=stream, want_stats=True)[1])
    show_classes("radiance, camera rays", cls_a)
    show_classes("radiance, shuffled rays", cls_c)
    print(f"  (a) / (b) wavefront {medians['(a) radiance, camera rays'] / medians['(b) frame, wavefront']:.3f}   "
          f"(a) / (b) fused {medians['(a) radiance, camera rays'] / medians['(b) frame, fused']:.3f}   "
          f"(c) / (a) {medians['(c) radiance, shuffled rays'] / medians['(a) radiance, camera rays']:.3f}   "
          f"radiance on the camera rays equals the frame bit for bit: {same}", flush=True)
ds.close()
