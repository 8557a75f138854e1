"""A film on device memory: frames of a resident scene accumulated over time (DeviceScene.accumulate), through camera moves.

`Film.add` renders one frame and folds it into the history: pixel by pixel while the camera stands still, through the
reprojection of rayca_hip_accumulate_device once it has moved (DeviceScene.update).  Everything stays in device memory and
on one stream; nothing is waited for."""
from __future__ import annotations

import dataclasses

from . import abi
from .renderer import Config, DeviceScene

GUIDES = ("point", "normal", "material")   # the G-buffer a frame leaves for the next one: surface outputs (id = the material)
METER_KEYS = ("low_permille", "high_permille", "key", "min_scale", "max_scale", "rate")   # of tonemap_kw: DeviceScene.meter's, the others are tonemap's


class Film:
    """Film(scene, width, height): the history of a width x height view of `scene` (a DeviceScene).

    max_history 0 is a running mean, else the history length is capped there (an exponential tail, which forgets what a
    moved light or material left).  normal_min and plane_max are the reprojection's thresholds (DeviceScene.accumulate);
    moments=True keeps the luminance moments, and with them `variance`.  add(config, jitter=n) traces each frame through
    another of the n x n stratified sub-pixel positions instead of the pixel centre, so that the history antialiases
    geometric edges.  A film's calls belong on one stream and one frame context: its buffers are reused from frame to
    frame, and that order is all that keeps them apart."""

    def __init__(self, scene: DeviceScene, width: int, height: int, *, max_history=0, normal_min=0.9, plane_max=0.1, moments=True):
        self.scene, self.width, self.height = scene, width, height
        self.max_history, self.normal_min, self.plane_max, self.with_moments = max_history, normal_min, plane_max, bool(moments)
        self._buffers = None
        self._meter = None     # the histogram and the two exposure records of resolve(exposure="auto"), made on first use
        self.reset()

    def reset(self) -> None:
        """Forget the history: the next add() is a first frame.  (The buffers are kept.)"""
        self.frames_added = 0
        self._pose = None      # bytes of the camera pose the history and its G-buffer belong to
        self._prev_pose = None # ... and the pose itself
        self._gamma = 1.0
        self._hist = 0         # which of the two history sets holds the film
        self._gbuf = 0         # which of the two G-buffers belongs to it
        self._exposure = None  # which of the two exposure records is the current one (None: nothing metered yet)

    def _allocate(self):
        import torch
        dev = torch.device("cuda", self.scene.device)
        h, w, n = self.height, self.width, self.height * self.width

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        def history():
            s = {"color": f32(h, w, 4), "length": f32(h, w)}
            if self.with_moments:
                s["moments"], s["variance"] = f32(h, w, 2), f32(h, w)
            return s

        def gbuffer():
            return {"point": f32(n, 3), "normal": f32(n, 3), "material": torch.empty((n,), dtype=torch.int32, device=dev)}

        self._buffers = {"frame": f32(h, w, 4), "rays": f32(n, 6), "t": f32(n), "prim": torch.empty((n,), dtype=torch.int32, device=dev),
                         "uv": f32(n, 2), "hist": (history(), history()), "gbuf": (gbuffer(), gbuffer())}

    def _gbuffer(self, which, stream, context):
        """camera rays -> closest hits -> surface, into the film's own tensors (what DeviceScene.gbuffer does into new ones)"""
        b, s = self._buffers, self.scene
        one = Config(samples_per_pixel=1)   # (the reprojection assumes points on the rays through pixel centres)
        s.camera_rays(one, self.width, self.height, stream=stream, context=context, out=b["rays"])
        s.query(b["rays"], stream=stream, context=context, out=(b["t"], b["prim"], b["uv"]))
        s.surface(b["rays"], b["t"], b["prim"], b["uv"], want=GUIDES, stream=stream, context=context, out=b["gbuf"][which])

    def _shaped(self, g):
        h, w = self.height, self.width
        return {"point": g["point"].view(h, w, 3), "normal": g["normal"].view(h, w, 3), "id": g["material"].view(h, w)}

    def add(self, config: Config, stream=None, context=0, *, jitter=None):
        """One more frame of `config`, rendered with gamma 1 and seed (config.seed + frames_added) mod 2^32, into the film.
        jitter=n (1..8): the frame's rays go through sub-sample frames_added mod n^2 of the n x n stratified sub-pixel
        positions of a frame with n^2 samples per pixel (DeviceScene.camera_rays: the reference's own positions, row-major), and
        the colour comes from DeviceScene.radiance along them, with that sub-sample index as `sample`; n^2 adds on a still camera
        are then the samples of one n^2-spp frame.  A config radiance() does not offer raises its error.  The G-buffer keeps
        coming from the rays through the pixel centres, which the reprojection assumes.  jitter=None: the frame of a render call.
        The first frame starts the history; a frame whose camera pose has the bytes of the previous one's continues it pixel by
        pixel; any other goes through the reprojection with the previous frame's G-buffer.  The two history sets and the two
        G-buffers change roles from frame to frame, so nothing is waited for.  Returns the film's colour (H, W, 4), which the
        next add() but one overwrites."""
        if self._buffers is None:
            self._allocate()
        b, s = self._buffers, self.scene
        handle = s.stream_handle(stream)
        self._gamma = config.gamma
        cfg = dataclasses.replace(config, gamma=1.0, seed=(config.seed + self.frames_added) % 2 ** 32)
        if jitter is None:
            s.render_device(cfg, self.width, self.height, 0, b["frame"].data_ptr(), stream=handle or None, context=context)
        else:
            if not isinstance(jitter, int) or isinstance(jitter, bool) or not 1 <= jitter <= 8:
                raise ValueError(f"jitter: None or an integer 1..8, not {jitter!r}")
            if "jitter_rays" not in b:
                b["jitter_rays"] = b["rays"].new_empty(b["rays"].shape)
            sub = self.frames_added % (jitter * jitter)
            s.camera_rays(Config(samples_per_pixel=jitter * jitter), self.width, self.height, sample=sub, stream=stream, context=context,
                          out=b["jitter_rays"])
            s.radiance(b["jitter_rays"], cfg, sample=sub, out=b["frame"].view(-1, 4), stream=stream, context=context)
        pose = s.camera_pose()
        pose_bytes = bytes(pose)
        src, dst = b["hist"][self._hist], b["hist"][self._hist ^ 1]
        kw = dict(max_history=self.max_history, moments=self.with_moments, variance=self.with_moments, out=dst, stream=stream, context=context)
        if self.frames_added == 0:
            self._gbuffer(self._gbuf, stream, context)
            s.accumulate(b["frame"], **kw)
        elif pose_bytes == self._pose:
            s.accumulate(b["frame"], history={k: v for k, v in src.items() if k != "variance"}, **kw)
        else:
            self._gbuffer(self._gbuf ^ 1, stream, context)
            now, then = self._shaped(b["gbuf"][self._gbuf ^ 1]), self._shaped(b["gbuf"][self._gbuf])
            s.accumulate(b["frame"], history={k: v for k, v in src.items() if k != "variance"}, prev=then, prev_camera=self._prev_pose,
                         normal_min=self.normal_min, plane_max=self.plane_max, **now, **kw)
            self._gbuf ^= 1
        self._hist ^= 1
        self._pose, self._prev_pose = pose_bytes, pose
        self.frames_added += 1
        return dst["color"]

    def add_adaptive(self, config: Config, budget=None, *, jitter=1, target=0.05, stream=None, context=0, **plan_kw):
        """One more pass of `budget` rays (default: one a pixel) that the film's own variance deals out: DeviceScene.sample_plan
        on the film's colour, variance and length, DeviceScene.radiance along the plan's rays -- gamma 1, seed (config.seed +
        frames_added) mod 2^32 and sample frames_added mod jitter^2, which is also the plan's first_stratum -- and
        DeviceScene.fold into the other history set.  `target` and `plan_kw` (lum_floor, base_weight, fresh_weight,
        min_history) are sample_plan's.  With equal weights and budget = W x H the pass is add(config, jitter=jitter), bit for
        bit.  It continues a history pixel by pixel, so the film must keep moments, hold at least one frame, and the camera must
        stand where the last frame left it: anything else is add()'s business (ValueError).  The budget is the host's: nothing
        is read back, nothing is waited for.  Returns the film's colour, as add() does."""
        n = self.width * self.height
        budget = n if budget is None else budget
        if not isinstance(jitter, int) or isinstance(jitter, bool) or not 1 <= jitter <= 8:
            raise ValueError(f"jitter: an integer 1..8, not {jitter!r}")
        stray = [k for k in plan_kw if k not in ("lum_floor", "base_weight", "fresh_weight", "min_history")]
        if stray:
            raise ValueError(f"plan_kw: {stray} are not sample_plan's weight parameters")
        if not self.with_moments:
            raise ValueError("add_adaptive: the film keeps no moments (moments=True), so it has no variance to plan with; use add()")
        if not self.frames_added:
            raise ValueError("add_adaptive: the film is empty; add() a frame first")
        b, s = self._buffers, self.scene
        if bytes(s.camera_pose()) != self._pose:
            raise ValueError("add_adaptive: the camera moved since the last frame; the reprojection is add()'s")
        import torch
        plan = b.get("plan")
        if plan is None or plan["rays"].shape[0] != budget:
            dev = b["frame"].device
            plan = b["plan"] = {"offset": torch.empty((n + 1,), dtype=torch.int32, device=dev), "rays": torch.empty((budget, 6), dtype=torch.float32, device=dev),
                                "samples": torch.empty((budget, 4), dtype=torch.float32, device=dev)}
        self._gamma = config.gamma
        cfg = dataclasses.replace(config, gamma=1.0, seed=(config.seed + self.frames_added) % 2 ** 32)
        sub = self.frames_added % (jitter * jitter)
        src, dst = b["hist"][self._hist], b["hist"][self._hist ^ 1]
        s.sample_plan(src["color"], src["variance"], src["length"], budget, jitter=jitter, first_stratum=sub, target=target, want=("offset", "rays"),
                      out={"offset": plan["offset"], "rays": plan["rays"]}, stream=stream, context=context, **plan_kw)
        s.radiance(plan["rays"], cfg, sample=sub, out=plan["samples"], stream=stream, context=context)
        s.fold(plan["samples"], plan["offset"], {k: v for k, v in src.items() if k != "variance"}, max_history=self.max_history, out=dst,
               stream=stream, context=context)
        self._hist ^= 1
        self.frames_added += 1
        return dst["color"]

    def _current(self, name):
        if not self.frames_added:
            raise ValueError("the film is empty: add() a frame first")
        return self._buffers["hist"][self._hist].get(name)

    @property
    def color(self):
        """(H, W, 4) float32, gamma 1: the accumulated frame"""
        return self._current("color")

    @property
    def length(self):
        """(H, W) float32: how many samples stand behind each pixel (0: none, its colour is not finite)"""
        return self._current("length")

    @property
    def variance(self):
        """(H, W) float32: the luminance variance over the history (None without moments)"""
        return self._current("variance")

    def gbuffer(self):
        """the G-buffer of the last frame whose camera differed from its predecessor's -- the film's view: point, normal (H, W, 3), id (H, W)"""
        if not self.frames_added:
            raise ValueError("the film is empty: add() a frame first")
        return self._shaped(self._buffers["gbuf"][self._gbuf])

    @property
    def exposure(self):
        """(4,) float32 {scale, target, L, 0}: the record of the last resolve(exposure="auto") (DeviceScene.meter), None before the
        first one and after reset()"""
        return None if self._exposure is None else self._meter["exposure"][self._exposure]

    def _resolve_tonemapped(self, op, exposure, tkw, denoise, gamma, rgba8, upsample, upsample_kw, stream, context, denoise_kw):
        if "gamma" in tkw or "rgba8" in tkw or "exposure" in tkw or "scale" in tkw:
            raise ValueError("tonemap_kw: gamma and rgba8 are resolve's own, and the scale comes from `exposure`")
        if "out" in denoise_kw or "variance_out" in denoise_kw or "out" in (upsample_kw or {}):
            raise ValueError("tonemap: the frame in front of it is an intermediate, its outputs are not the caller's (tonemap_kw['out'] is)")
        if upsample is not None or denoise:
            color = self.resolve(denoise=denoise, gamma=1.0, upsample=upsample, upsample_kw=upsample_kw, stream=stream, context=context, **denoise_kw)
            if isinstance(color, tuple):   # (upsample_kw may ask for the weight: the colour comes first)
                color = color[0]
        else:
            color = self.color
        meter_kw = {k: tkw.pop(k) for k in METER_KEYS if k in tkw}
        if exposure == "auto":
            if self._meter is None:
                import torch
                dev = torch.device("cuda", self.scene.device)
                self._meter = {"hist": torch.empty((abi.METER_WORDS,), dtype=torch.int32, device=dev),
                               "exposure": tuple(torch.empty((4,), dtype=torch.float32, device=dev) for _ in range(2))}
            prev = self.exposure
            nxt = 0 if self._exposure is None else self._exposure ^ 1
            self.scene.meter(color, prev=prev, out=(self._meter["hist"], self._meter["exposure"][nxt]), stream=stream, context=context, **meter_kw)
            self._exposure = nxt
            tkw["exposure"] = self.exposure
        else:
            if meter_kw:
                raise ValueError(f"tonemap_kw: {sorted(meter_kw)} belong to exposure='auto'")
            if isinstance(exposure, str):
                raise ValueError(f"exposure: a float, None or 'auto', not {exposure!r}")
            tkw["scale"] = 1.0 if exposure is None else float(exposure)
        return self.scene.tonemap(color, op, gamma=self._gamma if gamma is None else gamma, rgba8=rgba8, stream=stream, context=context, **tkw)

    def resolve(self, *, denoise=False, gamma=None, rgba8=False, upsample=None, upsample_kw=None, tonemap=None, exposure=None, tonemap_kw=None,
                stream=None, context=0, **denoise_kw):
        """The film through DeviceScene.denoise: its output stage alone (iterations=0: gamma and the RGBA8 quantisation of a
        render call), or with denoise=True the a-trous filter in front of it, guided by the film's G-buffer (normal, point, id;
        sigma_plane defaults to 0.1).  gamma None is the gamma of the config last added.  Returns what denoise() returns: a new
        float tensor, with rgba8 a tuple with the uint8 tensor behind it.

        denoise="variance" is the variance-guided filter instead (DeviceScene.denoise_variance): the film's colour, `variance`
        and `length` with the same G-buffer, so that the filter backs off where the film has converged.  It needs a film with
        moments=True; `denoise_kw` are denoise_variance's keywords, and it returns what that returns.

        upsample=s (1..8) gives a picture of s times the film's size, the film staying at its own: the resolved or denoised
        colour, with gamma 1, goes through DeviceScene.upsample against the G-buffers of DeviceScene.upsample_guides for the
        scene's camera as it stands (the film's current pose), and the gamma and the RGBA8 move to that call.  `upsample_kw`
        are upsample's keywords and, as `guides`, the selection of guides; it returns what upsample() returns.

        tonemap="linear", "reinhard" or "aces" puts DeviceScene.tonemap behind all of that: the resolved, denoised or upsampled
        colour leaves its pass with gamma 1, and the gamma and the RGBA8 move to the tonemap call.  `exposure` is the scale as a
        float (None: 1), or "auto": the film meters the colour it is about to map (DeviceScene.meter) and the operator reads the
        record on the device.  The film keeps two records that change roles from resolve to resolve, the previous one being the
        next call's `prev`, so that a `rate` below 1 adapts over the resolves; `exposure` (the property) is the current one,
        reset() forgets it.  `tonemap_kw` are tonemap's keywords (white, out) and, with "auto", meter's (low_permille,
        high_permille, key, min_scale, max_scale, rate); it returns what tonemap() returns."""
        if tonemap is not None:
            return self._resolve_tonemapped(tonemap, exposure, dict(tonemap_kw or {}), denoise, gamma, rgba8, upsample, upsample_kw, stream, context, denoise_kw)
        if exposure is not None or tonemap_kw:
            raise ValueError("exposure, tonemap_kw: only with tonemap")
        if upsample is not None:
            return self._resolve_upsampled(upsample, dict(upsample_kw or {}), denoise, gamma, rgba8, stream, context, denoise_kw)
        if upsample_kw:
            raise ValueError("upsample_kw: only with upsample")
        color = self.color
        kw = dict(denoise_kw)
        if isinstance(denoise, str):
            if denoise != "variance":
                raise ValueError(f"denoise: False, True or 'variance', not {denoise!r}")
            if not self.with_moments:
                raise ValueError("denoise='variance': the film keeps no moments (moments=True), so it has no variance")
            kw = {**self.gbuffer(), **kw}
            if kw.get("sigma_plane") is None:
                kw["sigma_plane"] = 0.1
            return self.scene.denoise_variance(color, self.variance, length=self.length, gamma=self._gamma if gamma is None else gamma,
                                               rgba8=rgba8, stream=stream, context=context, **kw)
        if denoise:
            kw = {**self.gbuffer(), **kw}
            if kw.get("sigma_plane") is None:
                kw["sigma_plane"] = 0.1
        else:
            kw["iterations"] = 0
        return self.scene.denoise(color, gamma=self._gamma if gamma is None else gamma, rgba8=rgba8, stream=stream, context=context, **kw)

    def _resolve_upsampled(self, scale, ukw, denoise, gamma, rgba8, stream, context, denoise_kw):
        if "gamma" in ukw or "rgba8" in ukw or "low" in ukw or "high" in ukw:
            raise ValueError("upsample_kw: gamma and rgba8 are resolve's own, and the guides come from `guides`")
        if "out" in denoise_kw or "variance_out" in denoise_kw:
            raise ValueError("upsample: the denoised film is an intermediate, its outputs are not the caller's")
        color = self.color
        if denoise:
            color = self.resolve(denoise=denoise, gamma=1.0, stream=stream, context=context, **denoise_kw)
        guides = ukw.pop("guides", ("albedo", "normal", "point", "id"))
        low, high = self.scene.upsample_guides(self.width * scale, self.height * scale, scale, guides=guides, stream=stream, context=context)
        if "point" in low and ukw.get("sigma_plane") is None:
            ukw["sigma_plane"] = 0.1
        return self.scene.upsample(color, scale, low=low, high=high, gamma=self._gamma if gamma is None else gamma, rgba8=rgba8,
                                   stream=stream, context=context, **ukw)
