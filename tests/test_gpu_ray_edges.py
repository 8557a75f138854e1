"""The adversarial ray families of ray_edges.py on every kernel path, bit for bit against the oracle: `prim` directly,
`t` and `uv` by their bits (assert_records of test_gpu_query.py).  test_ray_edges_cpu.py asserts that every batch holds
hits and misses in proportion, so nothing here passes on misses alone.

Ray batches run through DeviceScene.trace_rays (ordered, exhaustive) and DeviceScene.query (closest, occluded; unbounded and
with the per-ray boundary tmax = t / nextafter(t)) on RAYCA_BUILDER_REFERENCE, RAYCA_BUILDER_SAH after finish() and
RAYCA_BUILDER_SAH right after creation; the far, axis and nonfinite batches again in child processes that pin each node format;
telephoto Flat frames from 3e3 and 3e4 scene diagonals through both builders, both engines, both camera-ray kernels and (in the
child processes) every node format."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the child process of test_node_formats: the paths conftest.py gives the suite
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle_lib as ol
import ray_edges as re_
from parity_report import check_outliers
from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi, flatten
from test_gpu_parity import assert_exact
from test_gpu_query import HOW, NONE, assert_records, check_both, dev, in_slots, make_scene

pytestmark = pytest.mark.gpu
FLAT = Config(integrator=IntegratorStrategy.Flat)
_SCENES = {}      # (scene, how) -> DeviceScene, reused across families
_FAILED = set()   # families whose in-process comparison has failed, and "child" once a child process has not ended well:
                  # no (further) child process is started
CHILD_FAMILIES = ("far", "axis", "nonfinite")


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _SCENES.values():
        ds.close()
    _SCENES.clear()


def device_scene(name, how):
    if (name, how) not in _SCENES:
        _SCENES[(name, how)] = make_scene(re_.scene_desc(name), how)
    return _SCENES[(name, how)]


def boundary(t, prim):
    """tmax = t (a miss: the comparison is strict) for every other hit, the next float above t (the record) for the rest."""
    i = np.arange(t.size)
    with np.errstate(over="ignore"):   # (a miss carries FLT_MAX; its bound is 1.0)
        above = np.nextafter(t, np.float32(np.inf), dtype=np.float32)
    return np.where(prim != NONE, np.where(i % 2 == 0, t, above), np.float32(1.0)).astype(np.float32)


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("fam", re_.FAMILIES)
@pytest.mark.parametrize("name", re_.SCENES)
def test_ray_batches(gpu, name, fam, how):
    """(nonfinite: the traversal ends for any float values.  trace() and the refill kernels only move through the tree by
    node_step and test_leaf: node_step visits an inner node, pushes at most one (binary) or three (4-wide) of its children
    and continues with a child or a popped entry; test_leaf loops over a leaf's at most 64 primitives and pops.  A node is
    only ever reached from its parent, whatever the comparisons say, so it is visited at most once, the stack never holds
    more than the host sized it for from the tree's depth, and the search ends when the stack is empty.  A NaN in a
    comparison only decides WHICH children are visited.)"""
    try:
        rays = re_.family(name, fam)
        t, prim, uv = re_.oracle_records(name, fam)
        desc = re_.scene_desc(name)
        ds = device_scene(name, how)
        rec = (t, in_slots(ds, desc, prim, "edges:" + name), uv)
        what = f"{name} {fam} {how}"
        for trav, label in ((abi.TRAVERSAL_ORDERED, "ordered"), (abi.TRAVERSAL_EXHAUSTIVE, "exhaustive")):
            gt, gp, guv, _ = ds.trace_rays(rays, traversal=trav)
            assert_records((gt, gp, guv), rec, f"{what} trace_rays {label}")
        rays_d = dev(rays)
        check_both(ds, rays_d, rec, np.float32(np.inf), None, what + " unbounded")
        tmax = boundary(t, prim)
        check_both(ds, rays_d, rec, tmax, dev(tmax), what + " per-ray boundary")
    except BaseException:
        _FAILED.add(fam)
        raise


# ---- node formats: one fresh process per RAYCA_NODE_FORMAT (read once per process) -------------------------------------------
def flat_prims(order, prim):
    out = np.array(prim, np.uint32)
    hit = out != NONE
    out[hit] = order[out[hit]]
    return out


def frame_digest(f32):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(f32, np.float32).tobytes()).hexdigest()


def child(name):
    """Runs in the child: the far, axis and nonfinite batches on a finished RAYCA_BUILDER_SAH scene; prints one digest per batch
    and path.  (nonfinite under the 4-wide formats: every m, c and slack of the steering tests is finite -- trace_core.inc
    fix_axis -- so the point boxes and NaN planes of unused slots fail for these rays as for any other, and the argument in
    test_ray_batches' docstring holds.)"""
    import torch
    ds = make_scene(re_.scene_desc(name), "sah")
    order = ds.primitive_order()
    for fam in CHILD_FAMILIES:
        rays = re_.family(name, fam)
        t, prim, uv, _ = ds.trace_rays(rays)
        print("DIGEST", fam, "trace_rays", re_.digest(t, flat_prims(order, prim), uv), flush=True)
        qt, qp, quv = ds.query(dev(rays))
        torch.cuda.synchronize()
        print("DIGEST", fam, "query", re_.digest(qt.cpu().numpy(), flat_prims(order, qp.cpu().numpy().view(np.uint32)), quv.cpu().numpy()), flush=True)
    ds.close()
    if name in ("cornell", "box"):   # the telephoto frames under this node format, by both camera-ray kernels
        for R in (3e3, 3e4):
            ds = DeviceScene(telephoto_desc(name, R), Config(), builder=abi.BUILDER_SAH)
            ds.finish()
            for camera_rays in (abi.CAMERA_GENERATION, abi.CAMERA_REFILL):
                _, f32, st = ds.render(FLAT, 96, 96, camera_rays=camera_rays)
                print("FRAME", f"{R:g}", st["node_format"] & 5, frame_digest(f32), flush=True)
            ds.close()


@pytest.mark.parametrize("node_format", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["cornell", "soup1k", "box"])
def test_node_formats(gpu, name, node_format):
    stop = _FAILED & (set(CHILD_FAMILIES) | {"child"})
    if stop:
        pytest.fail(f"{sorted(stop)} failed before: no child process started")
    orc = re_.oracle_scene(name)
    want = {}
    for fam in CHILD_FAMILIES:
        t, prim, uv = re_.oracle_records(name, fam)
        want[fam] = re_.digest(t, flat_prims(orc.primitive_order(), prim), uv)
    env = dict(os.environ, RAYCA_NODE_FORMAT=str(node_format))
    try:   # a child that faults, aborts or hangs is the last one started
        p = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _FAILED.add("child")
        raise
    if p.returncode != 0:
        _FAILED.add("child")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l.split(" ", 3) for l in p.stdout.splitlines() if l.startswith("DIGEST ")]
    assert len(lines) == 2 * len(CHILD_FAMILIES), p.stdout
    for _, fam, path, got in lines:
        assert got == want[fam], f"{name} RAYCA_NODE_FORMAT={node_format} {fam} {path}: {got} != oracle {want[fam]}"
    frames = [l.split() for l in p.stdout.splitlines() if l.startswith("FRAME ")]
    assert len(frames) == (4 if name in ("cornell", "box") else 0), p.stdout
    for _, R, bits, got in frames:
        # bit 0: 4-wide nodes, bit 2: fp16 boxes (RaycaStats.node_format) -- the pinned format is the one that rendered
        assert int(bits) == (node_format & 1) | ((node_format & 2) << 1), (node_format, bits)
        o = ol.OracleScene(telephoto_desc(name, float(R)), Config())
        assert got == frame_digest(o.render(FLAT, 96, 96)[1]), f"{name} RAYCA_NODE_FORMAT={node_format} telephoto frame R={R}"
        o.close()


# ---- telephoto frames --------------------------------------------------------------------------------------------------------
def telephoto_desc(name, R):
    """The scene seen from R scene diagonals away (along +z, the camera's default view direction is -z), the field of view
    chosen so that the scene fills the frame."""
    scene = re_.build_scene(name)
    _, _, c, diag = re_.bounds(name)
    for model in scene.models:
        for node in model.nodes:
            if node.camera is not None:
                node.trs.translation = (float(c[0]), float(c[1]), float(c[2] + R * diag))
                model.cameras[node.camera].yfov_radians = 2.0 * math.atan(0.55 / R)
    return flatten(scene)


@pytest.mark.parametrize("R", [3e3, 3e4])
@pytest.mark.parametrize("name", ["cornell", "box"])
def test_telephoto_flat_frames(gpu, name, R):
    desc = telephoto_desc(name, R)
    w = h = 96
    orc = ol.OracleScene(desc, Config())
    _, of32, _ = orc.render(FLAT, w, h)
    lit = (of32[..., :3].sum(-1) > 0).mean()
    assert 0.2 <= lit <= 0.95, lit                       # the scene fills the frame, with background around it
    ref = DeviceScene(desc, Config(), builder=abi.BUILDER_REFERENCE)
    for engine in (abi.ENGINE_FUSED, abi.ENGINE_WAVEFRONT):
        _, f32, _ = ref.render(FLAT, w, h, engine=engine)
        assert_exact(f32, of32)
    ref.close()
    ds = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
    _, f32, st = ds.render(FLAT, w, h, collect_stats=True)      # (a counting frame is never a calibration frame)
    assert_exact(f32, of32)
    ds.finish()
    # Both camera-ray kernels.  (A scene only times its kernels and node formats -- the calibration cycle of
    # test_config3_soup_4096_full_size -- on frames of 65536 pixels and more (api.inc choose_generation); at 96 x 96 the
    # kernels are asked for by name here and the four node formats are pinned in the child processes of test_node_formats.)
    for camera_rays, refill in ((abi.CAMERA_GENERATION, False), (abi.CAMERA_REFILL, True)):
        _, f32, st = ds.render(FLAT, w, h, camera_rays=camera_rays)
        assert bool(st["node_format"] & 1024) == refill and not st["node_format"] & (256 | 512), st["node_format"]
        assert_exact(f32, of32)
    for engine in (abi.ENGINE_FUSED, abi.ENGINE_WAVEFRONT):
        _, f32, _ = ds.render(FLAT, w, h, engine=engine)
        assert_exact(f32, of32)
    _, f32, _ = ds.render(FLAT, w, h, traversal=abi.TRAVERSAL_EXHAUSTIVE)
    assert_exact(f32, of32)
    ds.close()
    orc.close()


@pytest.mark.parametrize("name", ["cornell", "box"])
def test_telephoto_depth2_frame(gpu, name):
    desc = telephoto_desc(name, 3e3)
    cfg = Config(max_depth=2)
    orc = ol.OracleScene(desc, cfg)
    _, of32, ost = orc.render(cfg, 96, 96)
    for builder, tag in ((abi.BUILDER_REFERENCE, "ref"), (abi.BUILDER_SAH, "sah")):
        ds = DeviceScene(desc, cfg, builder=builder)
        for engine, etag in ((abi.ENGINE_FUSED, "fused"), (abi.ENGINE_WAVEFRONT, "wavefront")):
            _, f32, st = ds.render(cfg, 96, 96, engine=engine, collect_stats=True)
            assert st["rays_shadow"] == ost["rays_shadow"] and st["rays_bounce"] == ost["rays_bounce"], (tag, etag)
            assert st["rays_shadow"] > 0 and st["rays_bounce"] > 0
            check_outliers(f"telephoto_{name}_depth2_{tag}_{etag}_96x96", f32, of32)
        ds.close()
    orc.close()


if __name__ == "__main__":
    child(sys.argv[1])
