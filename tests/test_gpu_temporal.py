"""rayca_hip_scene_camera and rayca_hip_accumulate_device (DeviceScene.camera_pose, .accumulate, Film) on the GPU.

Every comparison of the pass is bit for bit (the float words as uint32, on every output): against the literal numpy-float32
restatement (tests/temporal_literal.py -- the pass is +, -, x, /, floor, min and max only, each rounded once, so the restatement
has the kernel's bits), and between the ways of making one call (in place, another stream, another frame context, through Film)."""
import ctypes as C
import dataclasses
import math
import os

import numpy as np
import pytest

import temporal_literal as tl
from rayca_amd import Config, DeviceScene, Film, IntegratorStrategy, abi, flatten, lib, scenes
from rayca_amd import model as M
from rayca_amd import sdtf
from rayca_amd.lib import RaycaError

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
NONE = np.uint32(0xFFFFFFFF)
SIZES = [(1, 1), (1, 40), (40, 1), (3, 3), (61, 37), (65, 5), (130, 70)]   # (width, height)
POSE_A = tl.make_pose((0.2, 0.1, 2.0))
POSE_B = tl.make_pose((0.9, 0.15, 2.1), yaw=0.03, pitch=-0.02)   # shifted and slightly rotated
OUTPUTS = ("color", "length", "moments", "variance")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_desc(name):
    scene = M.Scene()
    if name == "box":
        scene.push_model(scenes.load_gltf(os.path.join(G, "box.gltf")))
        scene.push_model(M.create_default_model())
    else:
        sdtf.push_sdtf_from_path(scene, os.path.join(G, name + ".sdtf"))
    return flatten(scene)


@pytest.fixture(scope="module")
def ds(gpu):
    """the scene whose handle the synthetic calls go through (its contents are not read)"""
    s = DeviceScene(make_desc("box"), Config())
    yield s
    s.close()


def abi_pose(pose):
    p = abi.RaycaCameraPose()
    p.origin[:], p.right[:], p.up[:], p.back[:] = pose["origin"].tolist(), pose["right"].tolist(), pose["up"].tolist(), pose["back"].tolist()
    p.angle = float(pose["angle"])
    return p


_CASES = {}


def case(width, height):
    """a size's two views (A, and B with the specials aimed at A) and the history A left, made once and shared read-only"""
    key = (width, height)
    if key not in _CASES:
        seed = 300 + 131 * width + height
        a = tl.synthetic_view(POSE_A, width, height, seed)
        b = tl.synthetic_view(POSE_B, width, height, seed + 1, specials=POSE_A)
        hist = tl.first_history(a, specials=True)
        for d in (a, b, hist):
            for x in d.values():
                x.setflags(write=False)
        _CASES[key] = (a, b, hist)
    return _CASES[key]


def dev(a):
    import torch
    a = np.array(a)   # (a writable copy: the shared frames are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def dev_dict(d):
    return {k: dev(v) for k, v in d.items()}


def host(result):
    return {k: v.cpu().numpy() for k, v in result.items() if k in OUTPUTS}


def arguments(now, then, hist, which, on_device, reprojected=True, moments=True):
    """keywords of accumulate (the library's or the literal's) for a frame, the frame before it and its history"""
    put, put_dict = (dev, dev_dict) if on_device else ((lambda x: x), dict)
    kw = dict(history=put_dict({k: v for k, v in hist.items() if moments or k != "moments"}), moments=moments)
    if reprojected:
        kw.update(prev=put_dict({k: then[k] for k in ("normal",) + tuple(w for w in which if w != "normal")}),
                  prev_camera=abi_pose(POSE_A) if on_device else POSE_A, point=put(now["point"]), normal=put(now["normal"]))
        if "id" in which:
            kw["id"] = put(now["id"])
    return kw


def run(ds, color, **kw):
    import torch
    r = ds.accumulate(dev(color), **kw)
    torch.cuda.synchronize()
    return host(r)


def assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in OUTPUTS:
        if k not in want:
            continue
        g, w = got[k].reshape(want[k].shape[0], want[k].shape[1], -1), want[k].reshape(want[k].shape[0], want[k].shape[1], -1)
        bad = np.argwhere((bits(g) != bits(w)).any(-1))
        assert bad.size == 0, f"{what}: {k}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


# ---- 1, 2: against the literal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SIZES)
def test_every_size_equals_the_literal(ds, width, height):
    """widths around a wave and a block edge, single rows and columns; a NaN and an inf sample, a history length of 0, a point
    behind the previous camera, reprojections outside the image and into [-1, 0) at fixed pixels"""
    a, b, hist = case(width, height)
    which = ("normal", "point", "id")
    for reprojected in (False, True):
        got = run(ds, b["color"], variance=True, **arguments(b, a, hist, which, True, reprojected))
        want = tl.accumulate(b["color"], **arguments(b, a, hist, which, False, reprojected))
        assert_same(got, want, f"{width} x {height}, {'reprojection' if reprojected else 'identity'}")
    first = run(ds, b["color"], variance=True)
    assert_same(first, tl.accumulate(b["color"]), f"{width} x {height}, first frame")


@pytest.mark.parametrize("moments", [False, True], ids=["no_moments", "moments"])
@pytest.mark.parametrize("point", [False, True], ids=["no_point", "point"])
@pytest.mark.parametrize("ids", [False, True], ids=["no_id", "id"])
def test_every_subset_of_the_optional_inputs_equals_the_literal(ds, ids, point, moments):
    a, b, hist = case(61, 37)
    which = ("normal",) + (("point",) if point else ()) + (("id",) if ids else ())
    for max_history in (0, 4):
        for variance in ((False, True) if moments else (False,)):
            for reprojected in (False, True):
                hist_n = dict(hist, length=hist["length"] * F(5.0))   # (a history of five frames: the cap of 4 bites)
                got = run(ds, b["color"], variance=variance, max_history=max_history, **arguments(b, a, hist_n, which, True, reprojected, moments))
                want = tl.accumulate(b["color"], max_history=max_history, **arguments(b, a, hist_n, which, False, reprojected, moments))
                if not variance:
                    want.pop("variance", None)
                assert_same(got, want, f"{which}, moments {moments}, variance {variance}, max_history {max_history}, reprojected {reprojected}")
                assert ("moments" in got) == moments and ("variance" in got) == variance


# ---- 3: identity mode is a film in place ------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place_and_eight_frames_equal_the_literal(ds):
    import torch
    w, h, n = 61, 37, 8
    colors = [tl.synthetic_view(POSE_A, w, h, 800 + k)["color"] for k in range(n)]
    want = None
    film = None   # the history continued in place
    chain = None  # ... and through new tensors
    for k, c in enumerate(colors):
        want = tl.accumulate(c, history=tl.as_history(want) if want else None)
        chain = ds.accumulate(dev(c), history={x: chain[x] for x in ("color", "length", "moments")} if chain else None, variance=True)
        if film is None:
            film = ds.accumulate(dev(c), variance=True)
        else:
            hist = {x: film[x] for x in ("color", "length", "moments")}
            again = ds.accumulate(dev(c), history=hist, variance=True, out=film)
            assert all(again[x] is film[x] for x in OUTPUTS)
        torch.cuda.synchronize()
        assert_same(host(chain), want, f"frame {k}, out of place")
        assert_same(host(film), want, f"frame {k}, in place")
    # the frame itself as the colour output
    c = dev(colors[0])
    r = ds.accumulate(c, history={x: chain[x] for x in ("color", "length", "moments")}, out={"color": c})
    torch.cuda.synchronize()
    assert r["color"] is c
    assert_same(host(r), {k: v for k, v in tl.accumulate(colors[0], history=tl.as_history(want)).items() if k != "variance"}, "color_out == color")
    got = host(film)
    assert np.array_equal(got["length"], np.full((h, w), n, F))
    mean = np.mean(np.stack(colors).astype(np.float64), axis=0)
    bound = 3 * n * 2.0 ** -24 * max(float(np.abs(x).max()) for x in colors)
    err = float(np.abs(got["color"].astype(np.float64) - mean).max())
    print(f"max |film - mean| {err:.3g}, bound {bound:.3g}")
    assert err <= bound


# ---- 4: the ways of making one call -----------------------------------------------------------------------------------------
def test_strided_inputs_equal_contiguous_ones(ds):
    """an input that is not contiguous reaches the kernel as a contiguous copy: the contiguous call's bits"""
    import torch
    from strided import strided
    a, b, hist = case(65, 5)
    which = ("normal", "point", "id")
    want = run(ds, b["color"], variance=True, **arguments(b, a, hist, which, True))
    got = ds.accumulate(strided(dev(b["color"])), variance=True, **strided(arguments(b, a, hist, which, True)))
    torch.cuda.synchronize()
    assert_same(host(got), want, "strided inputs")


def test_stream_and_context_do_not_change_the_result(ds):
    import torch
    a, b, hist = case(130, 70)
    which = ("normal", "point", "id")
    want = tl.accumulate(b["color"], **arguments(b, a, hist, which, False))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        color, kw = dev(b["color"]), arguments(b, a, hist, which, True)
    side.synchronize()
    results = [ds.accumulate(color, variance=True, stream=side, context=1, **kw) for _ in range(3)]   # back to back, unwaited
    torch.cuda.synchronize()
    for r in results:
        assert_same(host(r), want, "side stream, context 1")


def test_stats_count_the_launch(ds):
    a, b, hist = case(61, 37)
    for reprojected in (False, True):
        r = ds.accumulate(dev(b["color"]), want_stats=True, **arguments(b, a, hist, ("normal", "point", "id"), True, reprojected))
        st = r["stats"]
        assert st["kernel_launches"] == 1 and st["class_launches"][abi.KERNEL_OTHER] == 1 and sum(st["class_launches"]) == 1, st
        assert st["kernel_ms"] > 0 and st["class_ms"][abi.KERNEL_OTHER] == st["kernel_ms"]


def test_guard_cells_stay_untouched(ds):
    import torch
    w, h = 61, 37
    a, b, hist = case(w, h)
    n = w * h
    sizes = {"color": 4, "length": 1, "moments": 2, "variance": 1}
    big = {k: torch.full((n * c + 128,), -7.0, dtype=torch.float32, device="cuda") for k, c in sizes.items()}
    out = {k: big[k][64:64 + n * c].view((h, w, c) if c > 1 else (h, w)) for k, c in sizes.items()}
    for reprojected in (False, True):
        for x in big.values():
            x.fill_(-7.0)
        ds.accumulate(dev(b["color"]), out=out, variance=True, **arguments(b, a, hist, ("normal", "point", "id"), True, reprojected))
        torch.cuda.synchronize()
        for k, c in sizes.items():
            assert bool((big[k][:64] == -7.0).all()) and bool((big[k][64 + n * c:] == -7.0).all()), k
        assert_same(host(out), tl.accumulate(b["color"], **arguments(b, a, hist, ("normal", "point", "id"), False, reprojected)), "guarded outputs")


# ---- 5, 6, 7: the camera pose, real scenes, the film ------------------------------------------------------------------------
_SCENES = {}
CFG = Config(integrator=IntegratorStrategy.Pathtracer, samples_per_pixel=1, gamma=1.0, seed=11)
W, H = 61, 37


def rendered(gpu, name):
    """(scene, the descriptor it was made from) -- each test that moves the camera puts it back"""
    if name not in _SCENES:
        desc = make_desc(name)
        _SCENES[name] = (DeviceScene(desc, Config(), builder=abi.BUILDER_SAH), desc)
        _SCENES[name][0].finish()
    return _SCENES[name]


def camera_node(desc):
    return next(n for n in desc._nodes[:desc.c.node_count] if n.camera != abi.NONE)


def quat_mul(a, b):
    return (a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0], -a[0] * b[2] + a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[1] - a[1] * b[0] + a[2] * b[3] + a[3] * b[2], -a[0] * b[0] - a[1] * b[1] - a[2] * b[2] + a[3] * b[3])


class moved_camera:
    """the scene's camera a small step aside and turned a little, for the time of a `with`"""

    def __init__(self, scene, desc, step=(0.04, 0.015, -0.02), turn=0.02):
        self.scene, self.desc, self.step, self.turn = scene, desc, step, turn

    def __enter__(self):
        cam = camera_node(self.desc)
        self.was = (tuple(cam.trs.translation), tuple(cam.trs.rotation))
        cam.trs.translation[:] = tuple(t + s for t, s in zip(self.was[0], self.step))
        cam.trs.rotation[:] = quat_mul(self.was[1], (0.0, math.sin(self.turn / 2), 0.0, math.cos(self.turn / 2)))
        self.scene.update(self.desc)

    def __exit__(self, *exc):
        cam = camera_node(self.desc)
        cam.trs.translation[:], cam.trs.rotation[:] = self.was
        self.scene.update(self.desc)


def frame_of(scene, cfg):
    import torch
    color = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    scene.render_device(cfg, W, H, 0, color.data_ptr())
    return color


def guides_of(scene):
    g = scene.gbuffer(CFG, W, H, want=("point", "normal", "material"))
    return {"point": g["point"], "normal": g["normal"], "id": g["material"]}, g["prim"]


@pytest.mark.parametrize("name", ["cornell_quad", "box"])
def test_camera_pose(gpu, name):
    import torch
    scene, desc = rendered(gpu, name)

    def check(s):
        pose = s.camera_pose()
        rays = s.camera_rays(CFG, W, H)
        g, prim = guides_of(s)
        torch.cuda.synchronize()
        origin = rays.cpu().numpy()[:, :3]
        assert (bits(origin) == bits(np.array(list(pose.origin), F))).all()   # every ray starts at the pose's origin, bit for bit
        assert pose.reserved0 == pose.reserved1 == pose.reserved2 == 0.0 and pose.angle > 0
        # the frame's own G-buffer points project back to their pixels
        hit = prim.cpu().numpy().view(np.uint32) != NONE
        assert hit.sum() > 100
        fx, fy, front = tl.project(tl.pose_from_abi(pose), g["point"].cpu().numpy(), W, H)
        y, x = np.mgrid[0:H, 0:W]
        ex, ey = float(np.abs(fx - x)[hit].max()), float(np.abs(fy - y)[hit].max())
        print(f"{name}: max |fx - x| {ex:.2g}, max |fy - y| {ey:.2g} over {hit.sum()} hits")
        assert front[hit].all() and ex <= 1 / 64 and ey <= 1 / 64
        return bytes(pose)

    before = check(scene)
    with moved_camera(scene, desc):
        after = check(scene)
        fresh = DeviceScene(desc, Config(), builder=abi.BUILDER_SAH)
        assert bytes(fresh.camera_pose()) == after != before   # the updated scene's pose is a fresh scene's, bit for bit
        fresh.close()
    assert bytes(scene.camera_pose()) == before
    # no camera: the error of a render call
    if name == "box":
        blind = M.Scene()
        blind.push_model(scenes.load_gltf(os.path.join(G, "box.gltf")))   # (the glTF alone has no camera)
        bs = DeviceScene(flatten(blind), Config())
        with pytest.raises(RaycaError) as e:
            bs.camera_pose()
        assert e.value.code == abi.ERR_NO_CAMERA
        bs.close()


@pytest.mark.parametrize("name", ["cornell_quad", "box"])
def test_film_through_a_camera_move_is_the_chain_and_the_literal(gpu, name):
    import torch
    scene, desc = rendered(gpu, name)
    film = Film(scene, W, H)
    # pose A by hand, then through the film
    color_a, (g_a, _), pose_a = frame_of(scene, CFG), guides_of(scene), scene.camera_pose()
    acc_a = scene.accumulate(color_a, variance=True)
    film.add(CFG)
    torch.cuda.synchronize()
    assert_same(host({k: getattr(film, k) for k in ("color", "length", "variance")}), {k: v for k, v in host(acc_a).items() if k != "moments"}, f"{name}: first frame")
    with moved_camera(scene, desc):
        film.add(CFG)
        color_b, (g_b, prim_b), pose_b = frame_of(scene, dataclasses.replace(CFG, seed=CFG.seed + 1)), guides_of(scene), scene.camera_pose()
        hist = {k: acc_a[k] for k in ("color", "length", "moments")}
        acc_b = scene.accumulate(color_b, history=hist, prev={"normal": g_a["normal"], "point": g_a["point"], "id": g_a["id"]}, prev_camera=pose_a,
                                 variance=True, **g_b)
        # the same pose as the previous camera, on the history this frame alone leaves: every hit finds itself
        own = scene.accumulate(color_b, history={k: v for k, v in scene.accumulate(color_b).items()}, prev=g_b, prev_camera=pose_b, **g_b)
        torch.cuda.synchronize()
        assert film.frames_added == 2 and bytes(pose_b) != bytes(pose_a)
        got = host({"color": film.color, "length": film.length, "variance": film.variance})
        chain = host(acc_b)
        assert_same(got, {k: v for k, v in chain.items() if k != "moments"}, f"{name}: the film against the chain")
        h = lambda d: {k: (v.cpu().numpy().view(np.uint32) if v.dtype == torch.int32 else v.cpu().numpy()) for k, v in d.items()}
        ga, gb = h(g_a), h(g_b)
        want = tl.accumulate(color_b.cpu().numpy(), history=tl.as_history(tl.accumulate(color_a.cpu().numpy())), prev=ga,
                             prev_camera=tl.pose_from_abi(pose_a), point=gb["point"], normal=gb["normal"], id=gb["id"])
        assert_same(chain, want, f"{name}: the chain against the literal")
        hit = prim_b.cpu().numpy().view(np.uint32) != NONE
        assert not gb["normal"][~hit].any()
        kept = chain["length"][hit] > 1.0
        print(f"{name}: {hit.sum()} hit pixels of {hit.size}, {kept.mean():.3f} of them kept their history through the move")
        own_len = own["length"].cpu().numpy()
        finite = np.isfinite(color_b.cpu().numpy()).all(-1)
        assert (own_len[hit & finite] > 1.5).all() and (own_len[~hit & finite] == 1.0).all()
    film.reset()


def test_film_with_a_static_camera(gpu):
    import torch
    scene, desc = rendered(gpu, "cornell_quad")
    n = 8
    cfg = dataclasses.replace(CFG, gamma=2.2)   # (the film renders with gamma 1 and keeps 2.2 for resolve)
    film = Film(scene, W, H)
    for _ in range(n):
        out = film.add(cfg)
    assert out is film.color and film.frames_added == n
    colors = [frame_of(scene, dataclasses.replace(CFG, seed=CFG.seed + k)) for k in range(n)]
    ref = frame_of(scene, dataclasses.replace(CFG, samples_per_pixel=256))
    torch.cuda.synchronize()
    colors, ref, got = [c.cpu().numpy() for c in colors], ref.cpu().numpy(), film.color.cpu().numpy()
    want = None
    for c in colors:
        want = tl.accumulate(c, history=tl.as_history(want) if want else None)
    # identity mode: the pixel-by-pixel chain's bits (a reprojection onto the same pose has weights that are not exactly 1)
    assert_same({"color": got, "length": film.length.cpu().numpy(), "variance": film.variance.cpu().numpy()}, {k: v for k, v in want.items() if k != "moments"}, "eight adds")
    assert np.isfinite(got).all()
    every = np.isfinite(np.stack(colors)).all(-1).all(0)   # (the pixels whose eight samples are all finite: the others took fewer)
    assert every.mean() > 0.99 and (film.length.cpu().numpy()[every] == n).all()
    mean = np.mean(np.stack(colors).astype(np.float64), axis=0)
    bound = 3 * n * 2.0 ** -24 * max(float(np.abs(c[every]).max()) for c in colors)
    err = float(np.abs(got.astype(np.float64) - mean)[every].max())

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))

    print(f"max |film - mean| {err:.3g}, bound {bound:.3g}; RMSE against 256 spp: one frame {rmse(colors[0]):.4f}, the film {rmse(got):.4f}")
    assert err <= bound
    assert rmse(got) < rmse(colors[0])
    # resolve: the output stage of a render call on the film's colour
    r32, r8 = film.resolve(rgba8=True)   # (gamma None: the 2.2 of the config last added)
    d32, d8 = scene.denoise(film.color, iterations=0, gamma=2.2, rgba8=True)
    e32, e8 = film.resolve(gamma=2.2, rgba8=True)
    f32 = film.resolve(denoise=True, iterations=2, gamma=1.0)
    g = film.gbuffer()
    k32 = scene.denoise(film.color, iterations=2, sigma_plane=0.1, **g)
    torch.cuda.synchronize()
    for a32, a8 in ((r32, r8), (e32, e8)):
        assert torch.equal(a32.view(torch.int32), d32.view(torch.int32)) and torch.equal(a8, d8)
    assert not torch.equal(d32, film.color) and torch.equal(f32.view(torch.int32), k32.view(torch.int32))
    # reset starts over
    film.reset()
    assert film.frames_added == 0
    with pytest.raises(ValueError):
        film.color
    film.add(cfg)
    torch.cuda.synchronize()
    assert np.array_equal(bits(film.color.cpu().numpy()), bits(colors[0]))
    assert np.array_equal(film.length.cpu().numpy(), np.isfinite(colors[0]).all(-1).astype(F))


# ---- 8: errors --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(gpu, ds):
    import torch
    w, h = 16, 8
    f = lambda *shape: torch.rand(shape, dtype=torch.float32, device="cuda")
    color, point, normal, hist_color, hist_moments, prev_normal, prev_point = f(h, w, 4), f(h, w, 3), f(h, w, 3), f(h, w, 4), f(h, w, 2), f(h, w, 3), f(h, w, 3)
    hist_length = torch.ones((h, w), dtype=torch.float32, device="cuda")
    ident = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    outs = {"color_out": torch.full((h, w, 4), -7.0, device="cuda"), "length_out": torch.full((h, w), -7.0, device="cuda"),
            "moments_out": torch.full((h, w, 2), -7.0, device="cuda"), "variance_out": torch.full((h, w), -7.0, device="cuda")}
    pose = abi_pose(POSE_A)
    p = lambda t: t.data_ptr()
    identity = dict(hist_color=p(hist_color), hist_length=p(hist_length), hist_moments=p(hist_moments))
    reprojection = dict(identity, prev_camera=C.pointer(pose), point=p(point), normal=p(normal), prev_normal=p(prev_normal), prev_point=p(prev_point),
                        id=p(ident), prev_id=p(ident))

    def call(base, scene=ds.handle, null_a=False, o_fields=None, tile_parts=0, **fields):
        a = abi.RaycaAccumulate()
        a.width, a.height, a.normal_min, a.plane_max = w, h, 0.9, 0.1
        a.color = p(color)
        for k, v in {**{k: p(v) for k, v in outs.items()}, **base, **fields}.items():
            setattr(a, k, v)
        o = abi.RaycaRenderOptions()
        o.tile.parts = tile_parts
        for k, v in (o_fields or {}).items():
            setattr(o, k, v)
        return gpu.rayca_hip_accumulate_device(scene, C.byref(o), None if null_a else C.byref(a), None)

    both = [dict(scene=None), dict(null_a=True), dict(width=0), dict(height=0), dict(width=65536, height=65536), dict(reserved=1), dict(color=None),
            dict(color_out=None), dict(length_out=None), dict(hist_color=None), dict(hist_length=None), dict(hist_moments=None),
            dict(moments_out=None), dict(color=p(color) + 4), dict(hist_color=p(hist_color) + 8), dict(color_out=p(outs["color_out"]) + 4),
            dict(length_out=p(outs["length_out"]) + 2), dict(hist_moments=p(hist_moments) + 1),
            dict(o_fields=dict(context=8)), dict(o_fields=dict(traversal=1)), dict(o_fields=dict(collect_stats=1)), dict(o_fields=dict(engine=1)),
            dict(o_fields=dict(camera_rays=1)), dict(o_fields=dict(reserved=1)), dict(tile_parts=2)]
    cases = [(identity, kw) for kw in both] + [(reprojection, kw) for kw in both]
    cases += [(identity, dict(point=p(point))), (identity, dict(normal=p(normal))), (identity, dict(id=p(ident))), (identity, dict(prev_id=p(ident)))]
    cases += [(reprojection, kw) for kw in (dict(point=None), dict(normal=None), dict(prev_normal=None), dict(id=None), dict(prev_id=None),
                                            dict(normal_min=0.0), dict(normal_min=float("nan")), dict(plane_max=0.0), dict(plane_max=-1.0),
                                            dict(plane_max=float("nan")), dict(point=p(point) + 2), dict(prev_id=p(ident) + 1))]
    for out in outs:   # the aliasing rule: no output on an image the taps read
        for src in ("hist_color", "hist_length", "hist_moments", "prev_normal", "prev_point", "prev_id"):
            cases.append((reprojection, {out: reprojection[src]}))
    for base, kw in cases:
        assert call(base, **kw) == abi.ERR_BAD_ARG, (kw, lib.last_error())
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == -7.0).all()), k   # nothing of the above wrote anything
    for base in (identity, reprojection):
        for t in outs.values():
            t.fill_(-7.0)
        assert call(base) == abi.OK
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert bool((t != -7.0).all()), k
    # the wrapper's own checks
    with pytest.raises(ValueError):
        ds.accumulate(color[:, :, :3])
    with pytest.raises(TypeError):
        ds.accumulate(color.double())
    with pytest.raises(ValueError):
        ds.accumulate(color, history={"colour": hist_color})
    with pytest.raises(RaycaError) as e:
        ds.accumulate(color, prev_camera=pose)
    assert e.value.code == abi.ERR_BAD_ARG and "point and normal" in lib.last_error()
    # an empty scene is no error: the scene is not read
    empty = M.Scene()
    empty.push_model(M.create_default_model())
    es = DeviceScene(flatten(empty), Config())
    kw = dict(history={"color": hist_color, "length": hist_length, "moments": hist_moments})
    got, want = es.accumulate(color, **kw), ds.accumulate(color, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in ("color", "length", "moments"))
    es.close()


def test_scenes_are_closed(gpu):
    for s, _ in _SCENES.values():
        s.close()
    _SCENES.clear()
