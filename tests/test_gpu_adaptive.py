"""rayca_hip_sample_plan_device and rayca_hip_film_fold_device (DeviceScene.sample_plan, .fold, Film.add_adaptive) on the GPU.

Every comparison is bit for bit: the plan's weights, offsets and ray-to-pixel map against the literal restatement
(tests/adaptive_literal.py: f32 for the weight, Python integers behind it), its rays against rows of DeviceScene.camera_rays, the
fold against that many calls of DeviceScene.accumulate, and Film.add_adaptive against Film.add and against the three calls it is
made of."""
import dataclasses

import numpy as np
import pytest

import adaptive_literal as al
from rayca_amd import Config, DeviceScene, Film, abi, flatten, scenes

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [(1, 1), (63, 3), (64, 4), (65, 9), (200, 150), (1031, 1021)]   # (width, height)
OUTPUTS = ("color", "length", "moments", "variance")
GUARD = 0x5EEDBEEF
CW, CH = 64, 48                  # the Cornell frames
PATH = Config(max_depth=2, seed=5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    a = np.array(a)   # (a writable copy: the shared films are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(x):
    a = x.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.fixture(scope="module")
def ds(gpu):
    s = DeviceScene(flatten(scenes.cornell_scene()), Config(), builder=abi.BUILDER_SAH)
    s.finish()
    yield s
    s.close()


_FILMS = {}


def film(width, height):
    """a size's synthetic film state, made once and shared read-only"""
    key = (width, height)
    if key not in _FILMS:
        f = al.synthetic_film(width, height, 7000 + 131 * width + height)
        for a in f.values():
            a.setflags(write=False)
        _FILMS[key] = f
    return _FILMS[key]


def segments(width, height):
    return -(-width // abi.PLAN_SEGMENT) * height


def run_plan(ds, f, budget, want=("weight", "offset", "pixel"), **kw):
    import torch
    r = ds.sample_plan(dev(f["color"]), dev(f["variance"]), dev(f["length"]), budget, want=want, **kw)
    torch.cuda.synchronize()
    return {k: (host(v) if k != "stats" else v) for k, v in r.items()}


def assert_plan(got, want, what):
    for k in ("weight", "offset", "pixel"):
        if k in got:
            bad = np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))
            assert got[k].shape == want[k].shape and bad.size == 0, \
                f"{what}: {k}: {bad.size} words differ, first {bad[:4].tolist()}: got {got[k].reshape(-1)[bad[:4]]} want {want[k].reshape(-1)[bad[:4]]}"


# ---- the plan against the literal -------------------------------------------------------------------------------------------------
def test_the_sizes_reach_every_level_of_the_scan():
    """a wave's 64-pixel row segment is the first level; one block scans the segment sums, PLAN_SCAN_CHUNK of them a trip"""
    counts = [segments(w, h) for w, h in SIZES]
    assert counts[0] == 1 and min(counts[1:]) > 1            # more than one first-level unit
    assert counts[3] == 2 * 9                                # two segments a row, the second one pixel wide
    assert max(counts) > 4 * abi.PLAN_SCAN_CHUNK             # the scan of the sums loops, and ends inside a chunk
    assert max(counts) % abi.PLAN_SCAN_CHUNK != 0
    assert any(1 < c < abi.PLAN_SCAN_CHUNK for c in counts)  # ... and a single partial trip


@pytest.mark.parametrize("width,height", SIZES)
def test_every_size_equals_the_literal(ds, width, height):
    f = film(width, height)
    budget = 3 * width * height + 7
    want = al.plan(**f, budget=budget)
    assert_plan(run_plan(ds, f, budget), want, f"{width} x {height}")
    assert int(want["weight"].max()) == 255 and (width * height < 100 or int(want["weight"].min()) == 0)


@pytest.mark.parametrize("budget", [0, 1, 65 * 9 - 1, 65 * 9])
@pytest.mark.parametrize("base_weight,fresh_weight", [(0, 0), (0, 255), (255, 0), (255, 255), (3, 17)])
def test_budgets_and_weight_bounds_equal_the_literal(ds, budget, base_weight, fresh_weight):
    f = film(65, 9)
    kw = dict(base_weight=base_weight, fresh_weight=fresh_weight, target=0.02, lum_floor=0.01, min_history=6)
    assert_plan(run_plan(ds, f, budget, **kw), al.plan(**f, budget=budget, **kw), f"B = {budget}, {kw}")


def test_all_zero_weights_are_the_uniform_plan(ds):
    w, h = 65, 9
    f = dict(color=np.ones((h, w, 4), F), variance=np.zeros((h, w), F), length=np.full((h, w), 9, F))
    for budget in (w * h, 2 * w * h + 5):
        got = run_plan(ds, f, budget, fresh_weight=0)
        assert not got["weight"].any()
        assert_plan(got, al.plan(**f, budget=budget, fresh_weight=0), f"uniform, B = {budget}")
    assert np.array_equal(run_plan(ds, f, w * h, fresh_weight=0)["offset"], np.arange(w * h + 1, dtype=np.uint32))


@pytest.mark.parametrize("want", [("offset",), ("weight", "offset"), ("offset", "pixel"), ("weight", "offset", "rays", "pixel")])
def test_output_subsets_write_nothing_else(ds, want):
    """every output between two guard words (so at a pointer that is 4-byte aligned only); what is not asked for is not made"""
    import torch
    w, h = 65, 9
    f, budget = film(w, h), 2 * w * h + 5
    sizes = {"weight": w * h, "offset": w * h + 1, "rays": budget * 6, "pixel": budget}
    shapes = {"weight": (h, w), "offset": (w * h + 1,), "rays": (budget, 6), "pixel": (budget,)}
    whole = {k: (torch.full((sizes[k] + 2,), GUARD, dtype=torch.int32, device="cuda") if k != "rays" else
                 torch.full((sizes[k] + 2,), -7.5, dtype=torch.float32, device="cuda")) for k in want}
    out = {k: v[1:-1].view(shapes[k]) for k, v in whole.items()}
    r = ds.sample_plan(dev(f["color"]), dev(f["variance"]), dev(f["length"]), budget, want=want, out=out)
    torch.cuda.synchronize()
    assert sorted(r) == sorted(want)
    for k, v in whole.items():
        assert r[k].data_ptr() == out[k].data_ptr()
        assert v[0].item() == v[-1].item() == (GUARD if k != "rays" else -7.5), k
    assert_plan({k: host(v) for k, v in r.items() if k != "rays"}, al.plan(**f, budget=budget), str(want))


# ---- the rays -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def peaked_film():
    """a Cornell-sized film state whose weight sits in a few pixels, so that they get more rays than there are strata"""
    rng = np.random.default_rng(7400)
    color = np.ones((CH, CW, 4), F)
    variance = np.zeros((CH, CW), F)
    hot = rng.choice(CW * CH, size=90, replace=False)
    variance.reshape(-1)[hot] = 100.0
    return dict(color=color, variance=variance, length=np.full((CH, CW), 8, F))


@pytest.fixture(scope="module")
def camera_rows(ds):
    """camera_rays of every sub-sample of an n^2-spp frame, n = 1, 2, 3: (n^2, W * H, 6) host arrays, made once"""
    import torch
    rows = {n: [ds.camera_rays(Config(samples_per_pixel=n * n), CW, CH, sample=s) for s in range(n * n)] for n in (1, 2, 3)}
    torch.cuda.synchronize()
    return {n: np.stack([host(r) for r in v]) for n, v in rows.items()}


@pytest.mark.parametrize("n,first_stratum", [(1, 0), (2, 0), (2, 3), (3, 0), (3, 14)])
@pytest.mark.parametrize("budget", [CW * CH, 2 * CW * CH + 5])
def test_every_ray_is_a_row_of_camera_rays(ds, peaked_film, camera_rows, n, first_stratum, budget):
    import torch
    f = peaked_film
    r = ds.sample_plan(dev(f["color"]), dev(f["variance"]), dev(f["length"]), budget, jitter=n, first_stratum=first_stratum, base_weight=1,
                       want=("offset", "rays", "pixel"))
    torch.cuda.synchronize()
    offset, pixel, rays = host(r["offset"]), host(r["pixel"]), host(r["rays"])
    want = al.plan(**f, budget=budget, base_weight=1)
    assert_plan(dict(offset=offset, pixel=pixel), want, f"n = {n}")
    counts = np.diff(offset.astype(np.int64))
    assert (counts >= n * n + 1).sum() >= 50 and (counts == 0).sum() + (counts == 1).sum() > 1000   # the strata wrap; most pixels get one ray or none
    strata = al.ray_strata(offset, n, first_stratum)
    assert len(set(strata.tolist())) == n * n
    expect = camera_rows[n][strata, pixel]
    bad = np.flatnonzero((bits(rays) != bits(expect)).any(-1))
    assert bad.size == 0, f"n = {n}: {bad.size} rays differ, first {bad[:4].tolist()}: {rays[bad[:2]]} vs {expect[bad[:2]]}"


# ---- the fold against the existing accumulation -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """65 x 9: n_p in 0..5 samples a pixel with a NaN and an inf among them, and the frames that hold each pixel's k-th sample (NaN
    where it has none)"""
    w, h = 65, 9
    rng = np.random.default_rng(7500)
    n = rng.integers(0, 6, size=w * h)
    offset = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    samples = rng.uniform(0.0, 3.0, size=(int(offset[-1]), 4)).astype(F)
    samples[:, 3] = 1.0
    with_list = np.flatnonzero(n >= 3)
    samples[offset[with_list[0]] + 1, 1] = np.nan       # inside a list
    samples[offset[with_list[1]], 0] = np.inf           # at the head of one
    samples[offset[with_list[2] + 1] - 1, 2] = -np.inf  # at the tail of one
    frames = []
    for k in range(int(n.max())):
        frame = np.full((w * h, 4), np.nan, F)
        has = n > k
        frame[has] = samples[offset[:-1][has] + k]
        frames.append(frame.reshape(h, w, 4))
    first = rng.uniform(0.0, 3.0, size=(h, w, 4)).astype(F)
    first[2, 3, 0] = np.nan                             # a pixel the history starts without: length 0
    first[4, 64, 1] = np.inf
    return dict(w=w, h=h, n=n, offset=offset, samples=samples, frames=frames, first=first)


def history_of(ds, ragged, frames_in, max_history):
    """a history made by accumulate itself: the first frame (two pixels of length 0), then `frames_in` more"""
    r = ds.accumulate(dev(ragged["first"]), max_history=max_history, variance=True)
    for k in range(frames_in):
        r = ds.accumulate(dev(ragged["frames"][k][::-1].copy()), history={x: r[x] for x in ("color", "length", "moments")}, max_history=max_history,
                          variance=True)
    return {x: r[x] for x in ("color", "length", "moments")}


def assert_fold(got, want, what):
    import torch
    torch.cuda.synchronize()
    got, want = {k: host(got[k]) for k in OUTPUTS}, {k: host(want[k]) for k in OUTPUTS}
    alive = got["length"] > 0
    assert (~alive).sum() <= 4
    for k in OUTPUTS:
        g, w = got[k].reshape(alive.shape + (-1,)), want[k].reshape(alive.shape + (-1,))
        if k in ("color", "variance"):   # a pixel of length 0: its colour is the validity channel's "nothing"
            g, w = g[alive], w[alive]
        bad = np.argwhere((bits(g) != bits(w)).any(-1))
        assert bad.size == 0, f"{what}: {k}: {len(bad)} pixels differ, first {bad[:4].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


@pytest.mark.parametrize("max_history", [0, 3])
@pytest.mark.parametrize("frames_in", [0, 2])
def test_a_fold_is_that_many_accumulations(ds, ragged, max_history, frames_in):
    hist = history_of(ds, ragged, frames_in, max_history)
    assert frames_in or int((host(hist["length"]) == 0).sum()) == 2   # (the first frame's NaN and inf pixels start without a history)
    want = dict(hist)
    for frame in ragged["frames"]:
        want = ds.accumulate(dev(frame), history={k: want[k] for k in ("color", "length", "moments")}, max_history=max_history, variance=True)
    got = ds.fold(dev(ragged["samples"]), dev(ragged["offset"]), hist, max_history=max_history)
    assert_fold(got, want, f"max_history {max_history}, {frames_in} frames in")
    # a pixel without samples keeps its history as it stands
    none = (ragged["n"] == 0).reshape(ragged["h"], ragged["w"])
    assert none.sum() > 20
    for k in ("color", "length", "moments"):
        assert np.array_equal(bits(host(got[k])[none]), bits(host(hist[k])[none])), k


def test_a_fold_in_place_on_another_stream_and_context(ds, ragged):
    import torch
    hist = history_of(ds, ragged, 1, 3)
    samples, offset = dev(ragged["samples"]), dev(ragged["offset"])
    want = ds.fold(samples, offset, hist, max_history=3)
    torch.cuda.synchronize()
    # the outputs are the history's own tensors
    mine = {k: v.clone() for k, v in hist.items()}
    got = ds.fold(samples, offset, mine, max_history=3, out=dict(mine))
    assert all(got[k].data_ptr() == mine[k].data_ptr() for k in mine)
    assert_fold(got, want, "in place")
    # another stream, another frame context
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = ds.fold(samples, offset, hist, max_history=3, stream=stream, context=3)
    stream.synchronize()
    assert_fold(got, want, "stream, context 3")
    # without moments: colour and length alone, the same words
    got = ds.fold(samples, offset, {k: hist[k] for k in ("color", "length")}, max_history=3, moments=False, variance=False)
    torch.cuda.synchronize()
    assert sorted(got) == ["color", "length"]
    alive = host(got["length"]) > 0
    assert np.array_equal(bits(host(got["length"])), bits(host(want["length"])))
    assert np.array_equal(bits(host(got["color"])[alive]), bits(host(want["color"])[alive]))


# ---- Film.add_adaptive ----------------------------------------------------------------------------------------------------------------
def film_state(film):
    import torch
    torch.cuda.synchronize()
    b = film._buffers["hist"][film._hist]
    return {k: host(b[k]) for k in OUTPUTS}


def two_films(ds):
    films = Film(ds, CW, CH), Film(ds, CW, CH)
    for f in films:
        for _ in range(2):
            f.add(PATH, jitter=2)
    return films


def assert_films(a, b, what):
    for k in OUTPUTS:
        bad = np.argwhere((bits(a[k]).reshape(CH, CW, -1) != bits(b[k]).reshape(CH, CW, -1)).any(-1))
        assert bad.size == 0, f"{what}: {k}: {len(bad)} pixels differ, first {bad[:4].tolist()}"


def test_with_equal_weights_an_adaptive_pass_is_a_jittered_add(ds):
    film, twin = two_films(ds)
    assert_films(film_state(film), film_state(twin), "two adds")
    film.add_adaptive(PATH, budget=CW * CH, jitter=2, target=1e30, base_weight=1, fresh_weight=0)
    twin.add(PATH, jitter=2)
    assert film.frames_added == twin.frames_added == 3
    assert_films(film_state(film), film_state(twin), "adaptive pass with equal weights against add(jitter=2)")
    assert np.array_equal(host(film._buffers["plan"]["offset"]), np.arange(CW * CH + 1, dtype=np.uint32))


def test_an_adaptive_pass_is_plan_radiance_fold(ds):
    import torch
    film, twin = two_films(ds)
    budget = 2 * CW * CH + 5
    color = film.add_adaptive(PATH, budget, jitter=2, target=0.05, min_history=2)
    assert color.data_ptr() == film.color.data_ptr() and film.frames_added == 3
    src = twin._buffers["hist"][twin._hist]
    sub = twin.frames_added % 4
    plan = ds.sample_plan(src["color"], src["variance"], src["length"], budget, jitter=2, first_stratum=sub, target=0.05, min_history=2)
    cfg = dataclasses.replace(PATH, gamma=1.0, seed=(PATH.seed + twin.frames_added) % 2 ** 32)
    samples = ds.radiance(plan["rays"], cfg, sample=sub)
    want = ds.fold(samples, plan["offset"], {k: src[k] for k in ("color", "length", "moments")})
    torch.cuda.synchronize()
    counts = np.diff(host(plan["offset"]).astype(np.int64))
    assert counts.sum() == budget and counts.max() > counts.min()      # the film's variance did deal the rays out unevenly
    assert_films(film_state(film), {k: host(want[k]) for k in OUTPUTS}, "add_adaptive against its three calls")
    assert np.array_equal(host(film._buffers["plan"]["offset"]), host(plan["offset"]))


def test_add_adaptive_leaves_the_rest_to_add(ds):
    with pytest.raises(ValueError, match=r"add\(\)"):
        Film(ds, CW, CH).add_adaptive(PATH)                       # an empty film
    plain = Film(ds, CW, CH, moments=False)
    plain.add(PATH, jitter=2)
    with pytest.raises(ValueError, match=r"add\(\)"):
        plain.add_adaptive(PATH)                                  # no moments: no variance
    film = Film(ds, CW, CH)
    film.add(PATH, jitter=2)
    film._pose = bytes(len(film._pose))                           # as after a camera move: the history's pose is another one
    with pytest.raises(ValueError, match=r"add\(\)"):
        film.add_adaptive(PATH)
    with pytest.raises(ValueError, match="jitter"):
        film.add_adaptive(PATH, jitter=9)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def test_stats_count_the_launches_under_other(ds, ragged):
    f = film(65, 9)
    for want, launches in ((("offset",), 3), (("weight", "offset"), 3), (("offset", "pixel"), 4), (("offset", "rays", "pixel"), 4)):
        stats = run_plan(ds, f, 500, want=want, want_stats=True)["stats"]
        assert stats["kernel_launches"] == launches and stats["class_launches"][abi.KERNEL_OTHER] == launches and stats["kernel_ms"] > 0, want
    assert run_plan(ds, f, 0, want=("offset", "rays", "pixel"), want_stats=True)["stats"]["kernel_launches"] == 3   # no rays: no ray kernel
    hist = history_of(ds, ragged, 0, 0)
    stats = ds.fold(dev(ragged["samples"]), dev(ragged["offset"]), hist, want_stats=True)["stats"]
    assert stats["kernel_launches"] == 1 and stats["class_launches"][abi.KERNEL_OTHER] == 1 and stats["kernel_ms"] > 0
