"""What a resident draw() of the atrium costs on the host (plain script, one process, run once):

    python tests/gpu_draw_probe.py [--parent-root DIR] [--draws 20] [--out profiles/resident_draw_atrium.log]

Draws the benchmark scene (scenes.atrium_scene(), 1920x1080, primary + shadow rays) through rayca_hip_renderer_draw: once to
build, a few times to warm up (the first frames of a scene also time its node formats), then `--draws` times with the same
descriptor (REUSED) and `--draws` times along a camera orbit (UPDATED), and prints the medians of the four phase times the
library reports (rayca_hip_renderer_last_draw) and of the wall time of the whole call, RGBA8 read back to the host included.
Every call ends in the render call's stream synchronisation, so the wall clock covers the finished frame.

--parent-root DIR: a built checkout of the commit this one is compared with.  Its `SoftRenderer.draw` of the same scene at the
same size is timed in a child process (its own library, its own Python mirror) -- the code under test is not its own
yardstick -- and the ratio resident / parent is printed.  Wall-clock medians on a shared host: good for the order of magnitude
and for ratios of tens, not for percents."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
from rayca_amd import Config, Image, SoftRenderer, scenes
scene = scenes.atrium_scene()
image = Image(1920, 1080)
renderer = SoftRenderer(Config(max_depth=1))
walls = []
for _ in range(int(sys.argv[2])):
    t = time.perf_counter()
    renderer.draw(scene, image)
    walls.append((time.perf_counter() - t) * 1e3)
import rayca_amd
print(json.dumps({"walls_ms": walls, "package": rayca_amd.__file__, "resident": hasattr(renderer, "last_draw")}))
"""


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--draws", type=int, default=20)
    ap.add_argument("--parent-draws", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from rayca_amd import Config, Image, Renderer, SoftRenderer, abi, flatten, scenes

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg = Config(max_depth=1)
    W, H = 1920, 1080
    scene = scenes.atrium_scene()
    t = time.perf_counter()
    desc = flatten(scene)
    flatten_ms = (time.perf_counter() - t) * 1e3
    r = Renderer()

    def draw(want):
        t = time.perf_counter()
        _, _, _, info = r.draw(desc, cfg, W, H, want_f32=False)
        wall = (time.perf_counter() - t) * 1e3
        assert info["action"] == want, (info["action"], want)
        return wall, info

    wall, info = draw(abi.DRAW_REBUILT)
    say(f"atrium {W}x{H}, Pathtracer max_depth 1 (primary + shadow), RAYCA_BUILDER_SAH; descriptor kept for comparisons: {info['kept_bytes'] / 1e6:.1f} MB")
    say(f"first draw (REBUILT, includes the process's HIP start-up): wall {wall:.1f} ms, of which build {info['ms']['build']:.1f} ms, render {info['ms']['render']:.2f} ms")
    r.invalidate()
    wall, info = draw(abi.DRAW_REBUILT)
    say(f"second build (REBUILT after invalidate, warm process): wall {wall:.1f} ms, of which build {info['ms']['build']:.1f} ms, render {info['ms']['render']:.2f} ms")
    from rayca_amd import lib
    lib.check(lib.load().rayca_hip_scene_finish(r.scene))
    for _ in range(40):     # the scene's first frames time its node formats and camera-ray kernels
        draw(abi.DRAW_REUSED)

    cam = next(n for n in desc._nodes[:desc.c.node_count] if n.camera != abi.NONE)

    def orbit(k):
        th = math.radians(3.0 * k)
        cam.trs.translation[:] = (0.0 + 5.0 * math.sin(th), 2.2, 0.3 + 5.0 * math.cos(th))
        cam.trs.rotation[:] = (0.0, math.sin(th / 2), 0.0, math.cos(th / 2))

    rows = {}
    for name, want in (("REUSED", abi.DRAW_REUSED), ("UPDATED", abi.DRAW_UPDATED)):
        walls, phases = [], {k: [] for k in ("compare", "update", "build", "render")}
        for k in range(args.draws):
            if want == abi.DRAW_UPDATED:
                orbit(k + 1)
            wall, info = draw(want)
            walls.append(wall)
            for p in phases:
                phases[p].append(info["ms"][p])
        rows[name] = (walls, phases)
        say(f"{name:8s} x{args.draws}: median wall {med(walls):.3f} ms (min {min(walls):.3f}, max {max(walls):.3f}); "
            + ", ".join(f"{p} {med(v):.3f}" for p, v in phases.items()) + " ms")
    say(f"counters: builds {info['builds']}, updates {info['updates']}, reuses {info['reuses']}")
    r.close()

    # the whole Python draw(scene, image): flatten(scene) per call on top of the above
    soft = SoftRenderer(cfg)
    image = Image(W, H)
    soft.draw(scene, image)
    walls = []
    for _ in range(5):
        t = time.perf_counter()
        soft.draw(scene, image)
        walls.append((time.perf_counter() - t) * 1e3)
    assert soft.last_draw["action"] == abi.DRAW_REUSED
    say(f"Python SoftRenderer.draw(scene, image), REUSED x5: median wall {med(walls):.1f} ms (flatten(scene) alone: {flatten_ms:.1f} ms)")
    soft_ms = med(walls)
    soft.close()

    if args.parent_root:
        out = subprocess.run([sys.executable, "-c", PARENT_CHILD, os.path.abspath(args.parent_root), str(args.parent_draws)],
                             check=True, capture_output=True, text=True, timeout=600).stdout
        res = json.loads(out.strip().splitlines()[-1])
        assert os.path.abspath(args.parent_root) in res["package"] and not res["resident"], res
        pw = res["walls_ms"]
        say(f"parent commit SoftRenderer.draw(scene, image) x{len(pw)}: " + ", ".join(f"{w:.1f}" for w in pw) + f" ms; median {med(pw):.1f} ms (the first includes the process's HIP start-up)")
        parent_ms = med(pw)
        say(f"ratio parent / resident, whole Python draw() (flatten included): {parent_ms / soft_ms:.1f}x")
        for name in ("REUSED", "UPDATED"):
            say(f"ratio parent draw() / rayca_hip_renderer_draw {name} (the C call alone, what a C, C++ or Rust host pays besides its own flatten): {parent_ms / med(rows[name][0]):.0f}x")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
