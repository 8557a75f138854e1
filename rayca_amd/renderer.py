"""Mirror of rayca-soft's renderer surface on top of the C ABI: `Config` (config.rs:10-49),
`IntegratorStrategy`, `SamplerStrategy`, `SoftRenderer` with `draw(scene, image)` (scene.rs:88-154).
All compute happens in librayca_hip.so on the GPU."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import abi, lib
from .model import Image, Scene, create_default_model, flatten


class IntegratorStrategy:
    Scratcher, Raytracer, Flat, AnalyticDirect, Direct, Pathtracer = range(6)


class SamplerStrategy:
    NONE, Nee, Hemisphere, Cosine, Brdf, Mis = range(6)


@dataclass
class Config:
    """rayca_soft::Config with the reference's defaults (config.rs:10-49)."""
    bvh: bool = True
    light_samples: int = 1
    light_stratify: bool = False
    samples_per_pixel: int = 1
    russian_roulette: bool = False
    direct_sampler: int = SamplerStrategy.Nee
    indirect_sampler: int = SamplerStrategy.Cosine
    integrator: int = IntegratorStrategy.Pathtracer
    max_depth: int = 5
    gamma: float = 1.0
    seed: int = 0

    def to_abi(self) -> abi.RaycaConfig:
        c = abi.RaycaConfig()
        c.bvh, c.light_samples, c.light_stratify = int(self.bvh), self.light_samples, int(self.light_stratify)
        c.samples_per_pixel, c.russian_roulette = self.samples_per_pixel, int(self.russian_roulette)
        c.direct_sampler, c.indirect_sampler, c.integrator = self.direct_sampler, self.indirect_sampler, self.integrator
        c.max_depth, c.gamma, c.seed = self.max_depth, self.gamma, self.seed
        return c


class DeviceScene:
    """Owns a RaycaScene handle: the device-resident scene + BVH (first half of draw, scene.rs:90-99)."""

    def __init__(self, desc: abi.SceneDesc, config: Optional[Config] = None, device: int = 0,
                 builder: int = abi.BUILDER_REFERENCE, build_on_host: bool = False, _lib=None):
        self._lib = _lib or lib.load()  # _lib: an explicitly loaded build of the library (A/B experiments)
        self.desc = desc
        self.device = device
        cfg = (config or Config()).to_abi()
        opts = abi.RaycaBuildOptions()
        opts.builder, opts.device, opts.build_on_host = builder, device, int(build_on_host)
        h = C.c_void_p()
        lib.check(self._lib.rayca_hip_scene_create(desc.ptr(), C.byref(cfg), C.byref(opts), C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.rayca_hip_scene_destroy(self.handle)
            self.handle = None
            self._surface_cdf_all = None   # (sample_surface's table of all slots)

    __del__ = close

    def info(self) -> dict:
        i = abi.RaycaSceneInfo()
        lib.check(self._lib.rayca_hip_scene_info(self.handle, C.byref(i)))
        return i.as_dict()

    def finish(self) -> None:
        """Wait for the node formats scene_create left to its own thread (rayca_hip_scene_finish): only needed where the
        first frames must already be eligible for every format (format calibration tests, benchmarks)."""
        lib.check(self._lib.rayca_hip_scene_finish(self.handle))

    def update(self, desc: abi.SceneDesc) -> None:
        """rayca_hip_scene_update: the camera, lights and materials of `desc` (the whole descriptor of the edited scene)
        replace the scene's, without a rebuild.  Frames are then bit-identical to those of DeviceScene(desc).  Raises
        RaycaError with ERR_UNSUPPORTED if the edit would move geometry (recreate the scene then), ERR_BAD_ARG if a count
        or a node field other than trs differs; a refused edit changes nothing."""
        lib.check(self._lib.rayca_hip_scene_update(self.handle, desc.ptr()))
        self.desc = desc

    def primitive_order(self) -> np.ndarray:
        n = self.info()["triangle_count"] + self.info()["sphere_count"]
        out = np.zeros(n, np.uint32)
        lib.check(self._lib.rayca_hip_scene_primitive_order(self.handle, out.ctypes.data, n))
        return out

    def read_nodes(self, which: int) -> np.ndarray:
        """rayca_hip_scene_read_nodes: which = 0 the 64-B binary nodes as (N, 16) uint32, 1 the 48-B centre / half records as (N, 12)"""
        n = C.c_uint64(0)
        lib.check(self._lib.rayca_hip_scene_read_nodes(self.handle, which, None, 0, C.byref(n)))
        out = np.zeros(n.value // 4, np.uint32)
        lib.check(self._lib.rayca_hip_scene_read_nodes(self.handle, which, out.ctypes.data, n.value, None))
        return out.reshape(-1, 16 if which == 0 else 12)

    @staticmethod
    def _opts(traversal, collect_stats, tile, stream, engine=abi.ENGINE_AUTO, context=0, camera_rays=abi.CAMERA_AUTO):
        o = abi.RaycaRenderOptions()
        o.traversal, o.collect_stats = traversal, int(collect_stats)
        o.engine, o.context, o.camera_rays = engine, context, camera_rays
        if tile is not None:
            o.tile.part, o.tile.parts, o.tile.band_rows = tile
        o.stream = stream
        return o

    def tile_rows(self, tile, height) -> int:
        t = abi.RaycaTile()
        t.part, t.parts, t.band_rows = tile
        return self._lib.rayca_hip_tile_rows(C.byref(t), height)

    def render(self, config: Config, width: int, height: int, *, traversal=abi.TRAVERSAL_ORDERED,
               collect_stats=False, tile=None, want_rgba8=True, want_f32=True, engine=abi.ENGINE_AUTO, context=0,
               camera_rays=abi.CAMERA_AUTO):
        """rayca_hip_render: host outputs. Returns (rgba8 | None, rgba32f | None, stats dict)."""
        rows = height if tile is None else self.tile_rows(tile, height)
        u8 = np.zeros((rows, width, 4), np.uint8) if want_rgba8 else None
        f32 = np.zeros((rows, width, 4), np.float32) if want_f32 else None
        st = abi.RaycaStats()
        cfg = config.to_abi()
        o = self._opts(traversal, collect_stats, tile, None, engine, context, camera_rays)
        lib.check(self._lib.rayca_hip_render(self.handle, C.byref(cfg), width, height, C.byref(o),
                                             u8.ctypes.data if u8 is not None else None,
                                             f32.ctypes.data if f32 is not None else None, C.byref(st)))
        return u8, f32, st.as_dict()

    def render_device(self, config: Config, width: int, height: int, d_rgba8: int, d_f32: int = 0, *,
                      traversal=abi.TRAVERSAL_ORDERED, collect_stats=False, tile=None, stream=None,
                      want_stats=False, engine=abi.ENGINE_AUTO, context=0, camera_rays=abi.CAMERA_AUTO):
        """rayca_hip_render_device: outputs stay in device memory (pointers as ints)."""
        st = abi.RaycaStats()
        cfg = config.to_abi()
        o = self._opts(traversal, collect_stats, tile, stream, engine, context, camera_rays)
        lib.check(self._lib.rayca_hip_render_device(self.handle, C.byref(cfg), width, height, C.byref(o),
                                                    d_rgba8 or None, d_f32 or None,
                                                    C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def prepare_device(self, config: Config, width: int, height: int, d_rgba8: int, d_f32: int = 0, *,
                       traversal=abi.TRAVERSAL_ORDERED, tile=None, stream=None, engine=abi.ENGINE_AUTO, context=0,
                       camera_rays=abi.CAMERA_AUTO, wait_event=None, record_event=None):
        """rayca_hip_render_device with every argument marshalled once: returns a zero-argument callable that issues the
        frame (asynchronously, no statistics).  A frame loop that renders the same frame into the same buffer again and
        again -- bench.py's ranks, a viewer -- pays the ctypes marshalling once instead of per frame (~10 us of the
        ~50 us a rank's share of a 1080p frame costs on the host)."""
        cfg = config.to_abi()
        o = self._opts(traversal, False, tile, stream, engine, context, camera_rays)
        # hipEvent_t handles (ints): the frame's stream waits for the one before its first kernel and records the other
        # behind its last -- wait + render + record in ONE native call (RaycaRenderOptions.wait_event / record_event)
        o.wait_event, o.record_event = wait_event, record_event
        fn, handle, check = self._lib.rayca_hip_render_device, self.handle, lib.check
        args = (handle, C.byref(cfg), width, height, C.byref(o), d_rgba8 or None, d_f32 or None, None)

        def issue(_keep=(cfg, o)):
            rc = fn(*args)
            if rc:
                check(rc)
        return issue

    def trace_rays(self, rays: np.ndarray, *, traversal=abi.TRAVERSAL_ORDERED, collect_stats=False):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        t = np.zeros(n, np.float32)
        prim = np.zeros(n, np.uint32)
        uv = np.zeros((n, 2), np.float32)
        st = abi.RaycaStats()
        o = self._opts(traversal, collect_stats, None, None)
        lib.check(self._lib.rayca_hip_trace_rays(self.handle, C.byref(o), n, rays.ctypes.data, t.ctypes.data,
                                                 prim.ctypes.data, uv.ctypes.data, C.byref(st)))
        return t, prim, uv, st.as_dict()

    def query(self, rays, *, tmax=None, kind="closest", stream=None, context=0, out=None, want_stats=False,
              traversal=abi.TRAVERSAL_ORDERED, collect_stats=False):
        """rayca_hip_query_device: closest hits or occlusion for rays that live in device memory, asynchronously.

        rays: torch tensor (N, 6) float32 on this scene's device (origin xyz, direction xyz).  tmax: None (unbounded), a
        float for every ray, or an (N,) float32 tensor; a hit counts iff t < tmax.  kind "closest" returns (t, prim, uv):
        float32 (N,) with FLT_MAX on a miss, int32 (N,) holding the u32 primitive slot (abi.NONE, i.e. -1, on a miss) and
        float32 (N, 2); kind "occluded" returns a uint8 (N,) mask.  `out`: the tensor(s) to write instead of new ones (for
        "closest" a 3-tuple whose entries may be None).  The kernel is launched on `stream` (a torch.cuda.Stream or a raw
        handle), by default torch's current stream of the device; nothing is copied except an input that is not contiguous,
        and nothing is waited for unless statistics are asked for (`want_stats` / `collect_stats`: the stats dict is appended
        to the result)."""
        if kind not in ("closest", "occluded"):
            raise ValueError(f"kind must be 'closest' or 'occluded', not {kind!r}")
        occluded = kind == "occluded"
        call = _DeviceCall(self, stream)
        torch = call.torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError(f"rays: a torch tensor on {call.dev} is expected, not {type(rays).__name__}")
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError(f"rays: shape {tuple(rays.shape)}, expected (N, 6)")
        n = rays.shape[0]
        if n > 0xFFFFFFFF:
            raise ValueError("rays: more than 2**32 - 1 rays")
        q = abi.RaycaQuery()
        q.kind, q.count, q.rays = (abi.QUERY_OCCLUDED if occluded else abi.QUERY_CLOSEST), n, call.input(rays, "rays", torch.float32, (n, 6)).data_ptr()
        if tmax is None:
            q.tmax_all = float("inf")
        elif isinstance(tmax, torch.Tensor):
            q.tmax = call.input(tmax, "tmax", torch.float32, (n,)).data_ptr()
        else:
            q.tmax_all = float(tmax)
        if occluded:
            result = call.output(out, "out", torch.uint8, (n,))
            q.occluded_out = result.data_ptr()
        else:
            o_t, o_prim, o_uv = out if out is not None else (None, None, None)
            result = (call.output(o_t, "out[0] (t)", torch.float32, (n,)), call.output(o_prim, "out[1] (prim)", torch.int32, (n,)),
                      call.output(o_uv, "out[2] (uv)", torch.float32, (n, 2)))
            q.t_out, q.prim_out, q.uv_out = (x.data_ptr() for x in result)
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_query_device, q, context=context, want_stats=want_stats or collect_stats,
                             traversal=traversal, collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is None:
            return result
        return (result, stats) if occluded else (*result, stats)

    def nearest(self, points, *, radius=None, kind="closest", stream=None, context=0, out=None, want_stats=False,
                traversal=abi.TRAVERSAL_ORDERED, collect_stats=False):
        """rayca_hip_nearest_device: the nearest surface point to points that live in device memory, asynchronously.

        points: torch tensor (N, 3) float32 on this scene's device.  radius: None (unbounded), a float for every point, or an
        (N,) float32 tensor; a surface point counts iff its SQUARED distance is below radius * radius.  kind "closest" returns
        (dist2, prim, point, uv): float32 (N,) squared distances with FLT_MAX on a miss, int32 (N,) holding the u32 primitive
        slot (abi.NONE, i.e. -1, on a miss), float32 (N, 3) nearest points and float32 (N, 2) in the convention of hit records
        -- prim and uv go to surface() as they are; kind "within" returns a uint8 (N,) mask.  `out`: the tensor(s) to write
        instead of new ones (for "closest" a 4-tuple: None makes a new tensor, False leaves that output out; not all four).
        Scenes with spheres are refused (ERR_UNSUPPORTED).  Stream handling and statistics as query()."""
        if kind not in ("closest", "within"):
            raise ValueError(f"kind must be 'closest' or 'within', not {kind!r}")
        within = kind == "within"
        call = _DeviceCall(self, stream)
        torch = call.torch
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor on {call.dev} is expected, not {type(points).__name__}")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: shape {tuple(points.shape)}, expected (N, 3)")
        n = points.shape[0]
        if n > 0xFFFFFFFF:
            raise ValueError("points: more than 2**32 - 1 points")
        q = abi.RaycaNearest()
        q.kind, q.count = (abi.NEAREST_WITHIN if within else abi.NEAREST_CLOSEST), n
        if within:
            result = call.output(out, "out", torch.uint8, (n,))
            q.within_out = result.data_ptr()
        else:
            o_d, o_prim, o_point, o_uv = out if out is not None else (None, None, None, None)
            result = (call.output(o_d, "out[0] (dist2)", torch.float32, (n,), optional=o_d is False),
                      call.output(o_prim, "out[1] (prim)", torch.int32, (n,), optional=o_prim is False),
                      call.output(o_point, "out[2] (point)", torch.float32, (n, 3), optional=o_point is False),
                      call.output(o_uv, "out[3] (uv)", torch.float32, (n, 2), optional=o_uv is False))
            if all(x is None for x in result):
                raise ValueError("out: at least one of the four outputs must be asked for")
            q.dist2_out, q.prim_out, q.point_out, q.uv_out = (_ptr(x) for x in result)
        q.points = call.input(points, "points", torch.float32, (n, 3)).data_ptr()
        if radius is None:
            q.radius_all = float("inf")
        elif isinstance(radius, torch.Tensor):
            q.radius = call.input(radius, "radius", torch.float32, (n,)).data_ptr()
        else:
            q.radius_all = float(radius)
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_nearest_device, q, context=context, want_stats=want_stats or collect_stats,
                             traversal=traversal, collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is None:
            return result
        return (result, stats) if within else (*result, stats)

    # ---- surface sampling: area-weighted points on the triangles (rayca_hip_surface_cdf_device, rayca_hip_surface_sample_device) ----
    SAMPLE_OUTPUTS = {"prim": ("int32", 0), "uv": ("float32", 2), "point": ("float32", 3), "normal": ("float32", 3)}

    def _slots(self) -> int:
        """the number of primitive slots (fixed for the handle)"""
        if "_slot_count" not in self.__dict__:
            i = self.info()
            self._slot_count = i["triangle_count"] + i["sphere_count"]
        return self._slot_count

    def surface_cdf(self, include=None, *, stream=None, context=0, out=None, want_stats=False):
        """rayca_hip_surface_cdf_device: the cumulative area table sample_surface() draws from, in device memory, asynchronously.

        include: None (every slot) or a (T,) uint8 / bool torch tensor on this scene's device, T the number of primitive slots;
        a slot whose byte is 0 gets area 0 and is never drawn.  Returns an int64 (T + 1,) tensor: 0, then the running sums of the
        slots' integer weights (the largest area weighs just under 2**32, every sum stays below 2**57); its last entry is 0 iff
        nothing can be drawn.  The table depends on the handle's geometry alone, which never changes.  `out`: the tensor to
        write instead of a new one.  Scenes with spheres are refused (ERR_UNSUPPORTED).  Stream handling as query();
        `want_stats` waits and returns (table, stats)."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        slots = self._slots()
        a = abi.RaycaSurfaceCdf()
        table = call.output(out, "out", torch.int64, (slots + 1,))
        a.cdf_out = table.data_ptr()
        if include is not None:
            if isinstance(include, torch.Tensor) and include.dtype == torch.bool:
                include = include.view(torch.uint8)   # (one byte an element, 0 / 1)
            a.include = call.input(include, "include", torch.uint8, (slots,)).data_ptr()
        stats = call.run(self._lib.rayca_hip_surface_cdf_device, a, context=context, want_stats=want_stats)
        return table if stats is None else (table, stats)

    def sample_surface(self, n, *, cdf=None, seed=0, sample=0, first_index=0, want=("prim", "uv", "point", "normal"), out=None,
                       stream=None, context=0, want_stats=False):
        """rayca_hip_surface_sample_device: `n` area-weighted random points on the scene's triangles, in device memory,
        asynchronously.

        cdf: a table from surface_cdf() (or any int64 (T + 1,) tensor of non-decreasing sums that starts at 0); None uses the
        table of all slots, which is made on first use -- that one call waits for it -- and kept on the handle.  Sample j draws
        from the stream of (seed, first_index + j, sample), as radiance() names a ray's: it does not depend on n, and chunks with
        the first_index of their first sample give what one call gives.  Returns a dict with one tensor per name in `want`: prim
        (n,) int32 holding the u32 primitive slot (abi.NONE, i.e. -1, when the table's total is 0), uv (n, 2) float32 in the
        convention of hit records -- prim and uv go to surface() as they are, rays=None -- point (n, 3) float32 and normal
        (n, 3) float32, the unit geometric normal in winding order; zeros on a miss.  `out`: a dict of tensors to write instead
        of new ones.  Scenes with spheres are refused (ERR_UNSUPPORTED).  Stream handling as query(); `want_stats` waits and
        adds "stats"."""
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 0xFFFFFFFF:
            raise ValueError(f"n: an int in 0 .. 2**32 - 1 is expected, not {n!r}")
        want = tuple(want)
        unknown = [w for w in want if w not in self.SAMPLE_OUTPUTS]
        if unknown or not want or len(set(want)) != len(want):
            raise ValueError(f"want: a non-empty selection without repeats of {tuple(self.SAMPLE_OUTPUTS)}, not {want!r}")
        for name, v in (("seed", seed), ("sample", sample), ("first_index", first_index)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError(f"{name}: an int in 0 .. 2**32 - 1 is expected, not {v!r}")
        call = _DeviceCall(self, stream)
        torch = call.torch
        slots = self._slots()
        a = abi.RaycaSurfaceSample()
        a.count, a.seed, a.sample, a.first_index = n, seed, sample, first_index
        out = dict(out) if out is not None else {}
        stray = [k for k in out if k not in want]
        if stray:
            raise ValueError(f"out: {stray} not in want")
        result = {}
        for name in want:
            dtype, width = self.SAMPLE_OUTPUTS[name]
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), (n, width) if width else (n,))
            setattr(a, name + "_out", result[name].data_ptr() or None)
        if cdf is None:
            if self.__dict__.get("_surface_cdf_all") is None:   # (made once: the call waits, so every later stream may read it)
                self._surface_cdf_all = self.surface_cdf(stream=stream, context=context, want_stats=True)[0]
            cdf = self._surface_cdf_all
        a.cdf = call.input(cdf, "cdf", torch.int64, (slots + 1,)).data_ptr()
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_surface_sample_device, a, context=context, want_stats=want_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is not None:
            result["stats"] = stats
        return result

    # ---- multi-hit queries: the first k hits along a ray, in order (rayca_hip_hits_device) ----
    HITS_OUTPUTS = {"t": ("float32", 0), "prim": ("int32", 0), "uv": ("float32", 2), "face": ("uint8", 0), "n": ("int32", None)}

    def hits(self, rays, k, *, tmax=None, faces="front", count_all=False, outputs=("t", "prim", "uv", "face", "n"), stream=None, context=0,
             out=None, want_stats=False, traversal=abi.TRAVERSAL_ORDERED, collect_stats=False):
        """rayca_hip_hits_device: the first k hits along rays that live in device memory, in order, asynchronously.

        rays: torch tensor (N, 6) float32 on this scene's device.  k: 0 .. abi.HITS_MAX hits per ray (0 only with count_all and
        "n" alone).  tmax: None (unbounded), a float for every ray, or an (N,) float32 tensor; a hit counts iff t < tmax.
        faces: "front" (back faces culled, as closest hits) or "both" (a hit on the back of a triangle has face 1).  Returns a
        dict with one tensor per name in `outputs`: t (N, k) float32 with FLT_MAX in unused entries, prim (N, k) int32 holding the
        u32 slot (abi.NONE, i.e. -1, unused), uv (N, k, 2) float32, face (N, k) uint8 and n (N,) int32: min(hits, k), or the number
        of all hits in front of tmax with count_all.  Hits are ordered by (t, the reference's primitive order); entry 0 with
        "front" is query(kind="closest")'s record; t, prim and uv of an entry go to surface() as they are.  `out`: a dict of
        tensors to write instead of new ones.  Stream handling and statistics as query(): `want_stats` / `collect_stats` wait and
        add "stats"."""
        if faces not in ("front", "both"):
            raise ValueError(f"faces must be 'front' or 'both', not {faces!r}")
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= abi.HITS_MAX:
            raise ValueError(f"k: an int in 0 .. {abi.HITS_MAX} is expected, not {k!r}")
        outputs = tuple(outputs)
        unknown = [w for w in outputs if w not in self.HITS_OUTPUTS]
        if unknown or not outputs or len(set(outputs)) != len(outputs):
            raise ValueError(f"outputs: a non-empty selection without repeats of {tuple(self.HITS_OUTPUTS)}, not {outputs!r}")
        if k == 0 and (not count_all or outputs != ("n",)):
            raise ValueError("k == 0 counts crossings: it needs count_all=True and outputs=('n',)")
        call = _DeviceCall(self, stream)
        torch = call.torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError(f"rays: a torch tensor on {call.dev} is expected, not {type(rays).__name__}")
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError(f"rays: shape {tuple(rays.shape)}, expected (N, 6)")
        n = rays.shape[0]
        if n > 0xFFFFFFFF:
            raise ValueError("rays: more than 2**32 - 1 rays")
        q = abi.RaycaHits()
        q.count, q.k, q.faces, q.count_all = n, k, (abi.HITS_BOTH if faces == "both" else abi.HITS_FRONT), 1 if count_all else 0
        out = dict(out) if out is not None else {}
        stray = [w for w in out if w not in outputs]
        if stray:
            raise ValueError(f"out: {stray} not in outputs")
        result = {}
        for name in outputs:
            dtype, width = self.HITS_OUTPUTS[name]
            shape = (n,) if width is None else ((n, k, width) if width else (n, k))
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), shape)
            setattr(q, name + "_out", result[name].data_ptr() or None)
        q.rays = call.input(rays, "rays", torch.float32, (n, 6)).data_ptr()
        if tmax is None:
            q.tmax_all = float("inf")
        elif isinstance(tmax, torch.Tensor):
            q.tmax = call.input(tmax, "tmax", torch.float32, (n,)).data_ptr()
        else:
            q.tmax_all = float(tmax)
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_hits_device, q, context=context, want_stats=want_stats or collect_stats,
                             traversal=traversal, collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is not None:
            result["stats"] = stats
        return result

    # ---- signed distance and occupancy: the nearest point plus a vote of crossing-count rays (rayca_hip_signed_device) ----
    SIGNED_OUTPUTS = {"dist2": ("float32", ()), "prim": ("int32", ()), "point": ("float32", (3,)), "uv": ("float32", (2,)),
                      "inside": ("uint8", ()), "votes": ("uint8", ()), "cross": ("int32", None)}
    SIGNED_RULES = {"parity": abi.SIGNED_PARITY, "winding": abi.SIGNED_WINDING}

    def signed(self, points=None, *, grid=None, radius=None, dirs=3, rule="parity",
               outputs=("dist2", "prim", "point", "uv", "inside", "votes", "cross"), stream=None, context=0, out=None, want_stats=False,
               traversal=abi.TRAVERSAL_ORDERED, collect_stats=False):
        """rayca_hip_signed_device: the nearest surface point of points in device memory and the side of the surface they lie
        on, in one launch, asynchronously.

        points: torch tensor (N, 3) float32 on this scene's device -- or grid=(origin, step, dims): the N = nx * ny * nz points
        origin + index * step of a regular grid, x running fastest, made inside the kernel (signed.grid_points restates them).
        radius: as for nearest(); it bounds the distance part only.  dirs: 1, 3 or 5 -- that many of signed.sign_directions() --
        or an (n, 3) array of directions without a zero component.  rule: "parity" (an odd number of crossings is inside) or
        "winding" (more exits than entries is inside: the union of overlapping closed meshes).  Returns a dict with one tensor
        per name in `outputs`: dist2, prim, point, uv as nearest() returns them; inside (N,) uint8, the majority of the
        directions' votes; votes (N,) uint8, bit j the vote of direction j; cross (N, n, 2) int32, the (front, back) crossing
        counts of each direction.  At least one of inside, votes, cross must be asked for; without a distance output the
        nearest search is left out.  The sign is meaningful for closed, consistently wound meshes.  `out`: a dict of tensors
        to write instead of new ones.  Stream handling and statistics as query(): `want_stats` / `collect_stats` wait and add
        "stats".  Scenes with spheres are refused (ERR_UNSUPPORTED)."""
        from .signed import checked_directions, checked_grid
        if rule not in self.SIGNED_RULES:
            raise ValueError(f"rule must be 'parity' or 'winding', not {rule!r}")
        outputs = tuple(outputs)
        unknown = [w for w in outputs if w not in self.SIGNED_OUTPUTS]
        if unknown or not outputs or len(set(outputs)) != len(outputs):
            raise ValueError(f"outputs: a non-empty selection without repeats of {tuple(self.SIGNED_OUTPUTS)}, not {outputs!r}")
        if not {"inside", "votes", "cross"} & set(outputs):
            raise ValueError("outputs: one of 'inside', 'votes', 'cross' must be asked for (the distance outputs alone are nearest())")
        if (points is None) == (grid is None):
            raise ValueError("either points or grid=(origin, step, dims) is expected")
        d = checked_directions(dirs)
        call = _DeviceCall(self, stream)
        torch = call.torch
        q = abi.RaycaSigned()
        if grid is not None:
            origin, step, dims, n = checked_grid(grid)
            q.source = abi.SIGNED_GRID
            for a in range(3):
                q.grid_origin[a], q.grid_step[a], q.grid_dims[a] = float(origin[a]), float(step[a]), dims[a]
        else:
            if not isinstance(points, torch.Tensor):
                raise TypeError(f"points: a torch tensor on {call.dev} is expected, not {type(points).__name__}")
            if points.dim() != 2 or points.shape[1] != 3:
                raise ValueError(f"points: shape {tuple(points.shape)}, expected (N, 3)")
            n = points.shape[0]
            if n > 0xFFFFFFFF:
                raise ValueError("points: more than 2**32 - 1 points")
            q.source = abi.SIGNED_POINTS
        q.count, q.rule, q.n_dirs = n, self.SIGNED_RULES[rule], d.shape[0]
        for j in range(d.shape[0]):
            for a in range(3):
                q.dirs[j][a] = float(d[j, a])
        out = dict(out) if out is not None else {}
        stray = [w for w in out if w not in outputs]
        if stray:
            raise ValueError(f"out: {stray} not in outputs")
        result = {}
        for name in outputs:
            dtype, tail = self.SIGNED_OUTPUTS[name]
            shape = (n, d.shape[0], 2) if tail is None else (n, *tail)
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), shape)
            setattr(q, name + "_out", result[name].data_ptr() or None)
        if grid is None:
            q.points = call.input(points, "points", torch.float32, (n, 3)).data_ptr()
        if radius is None:
            q.radius_all = float("inf")
        elif isinstance(radius, torch.Tensor):
            q.radius = call.input(radius, "radius", torch.float32, (n,)).data_ptr()
        else:
            q.radius_all = float(radius)
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_signed_device, q, context=context, want_stats=want_stats or collect_stats,
                             traversal=traversal, collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is not None:
            result["stats"] = stats
        return result

    def signed_distance(self, points=None, *, grid=None, **kw):
        """The signed distance to the surface, float32 (N,): sqrt(dist2) of signed(), negated where `inside`.  The square root is
        torch's, on the stream of the call; the kernel's own contract stays free of it.  A point without a surface point within
        `radius` has the square root of FLT_MAX.  Keywords as signed() without `outputs` and `out`."""
        call = _DeviceCall(self, kw.get("stream"))
        r = self.signed(points, grid=grid, outputs=("dist2", "inside"), **kw)
        torch = call.torch
        # (a raw handle is wrapped; without a stream the call has waited, and torch's current stream will do)
        stream = call.stream if hasattr(call.stream, "cuda_stream") else (torch.cuda.ExternalStream(call.handle, device=call.dev) if call.handle else None)
        with torch.cuda.stream(stream):
            d = torch.sqrt(r["dist2"])
            return torch.where(r["inside"] != 0, -d, d)

    def occupancy(self, points=None, *, grid=None, **kw):
        """The inside mask of signed(), uint8 (N,).  No distance output is asked for, so the nearest search is not run.  Keywords
        as signed() without `outputs`; `out`: the tensor to write."""
        if "out" in kw:
            kw["out"] = {"inside": kw["out"]} if kw["out"] is not None else None
        return self.signed(points, grid=grid, outputs=("inside",), **kw)["inside"]

    # ---- surface queries: what is at a hit (rayca_hip_surface_device), and the rays of a frame (rayca_hip_camera_rays_device) ----
    SURFACE_OUTPUTS ={"point": ("float32", 3), "normal": ("float32", 3), "color": ("float32", 4), "diffuse": ("float32", 4),
                       "specular": ("float32", 4), "rough": ("float32", 2), "material": ("int32", 0), "flags": ("int32", 0)}

    def stream_handle(self, stream=None) -> int:
        """The raw handle of `stream` (a torch.cuda.Stream, a raw handle, or None: torch's current stream of the scene's device)
        as the device calls take it; 0 is the legacy default stream, which is synchronised here (see _DeviceCall)."""
        return _DeviceCall(self, stream).handle

    def camera_rays(self, config: Config, width: int, height: int, *, sample=0, tile=None, stream=None, context=0, out=None):
        """rayca_hip_camera_rays_device: the camera rays of sub-sample `sample` of a width x height frame of `config` (only its
        samples_per_pixel matters), as a (rows * width, 6) float32 tensor on the scene's device -- origin xyz, direction xyz,
        what query() reads; rows = tile_rows(tile, height), the whole frame without a tile.  Stream handling as query()."""
        call = _DeviceCall(self, stream)
        rows = height if tile is None else self.tile_rows(tile, height)
        out = call.output(out, "out", call.torch.float32, (rows * width, 6))
        cfg = config.to_abi()
        o = call.options(context, tile=tile)
        lib.check(self._lib.rayca_hip_camera_rays_device(self.handle, C.byref(cfg), width, height, sample, C.byref(o), out.data_ptr() or None))
        return out

    def surface(self, rays, t, prim, uv, *, want=("point", "normal", "color", "diffuse", "specular", "rough", "material", "flags"),
                stream=None, context=0, out=None, want_stats=False):
        """rayca_hip_surface_device: the surface at hit records, asynchronously, everything in device memory.

        t (N,) float32, prim (N,) int32 holding the u32 slot, uv (N, 2) float32: records as query(kind="closest") returns
        them; rays (N, 6) float32 the rays they belong to (may be None unless "point" or "normal" is wanted).  Returns a dict
        with one tensor per name in `want`: point / normal (N, 3), color / diffuse / specular (N, 4), rough (N, 2: roughness,
        shininess) float32; material / flags (N,) int32 holding the u32 bits (material abi.NONE, i.e. -1, without a material
        and on a miss; flags: abi.SURFACE_*).  A record whose prim is not a slot of the scene is a miss: zeros.  `out`: a dict
        of tensors to write instead of new ones.  Stream handling as query(); `want_stats` waits and adds "stats"."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        want = tuple(want)
        unknown = [w for w in want if w not in self.SURFACE_OUTPUTS]
        if unknown or not want or len(set(want)) != len(want):
            raise ValueError(f"want: a non-empty selection without repeats of {tuple(self.SURFACE_OUTPUTS)}, not {want!r}")
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"t: a torch tensor on {call.dev} is expected, not {type(t).__name__}")
        if t.dim() != 1:
            raise ValueError(f"t: shape {tuple(t.shape)}, expected (N,)")
        n = t.shape[0]
        if n > 0xFFFFFFFF:
            raise ValueError("t: more than 2**32 - 1 records")
        need_rays = "point" in want or "normal" in want
        if rays is None and need_rays:
            raise ValueError("rays: needed for 'point' and 'normal'")
        q = abi.RaycaSurfaceQuery()
        q.count = n
        q.t = call.input(t, "t", torch.float32, (n,)).data_ptr()
        q.prim = call.input(prim, "prim", torch.int32, (n,)).data_ptr()
        q.uv = call.input(uv, "uv", torch.float32, (n, 2)).data_ptr()
        if rays is not None:
            q.rays = call.input(rays, "rays", torch.float32, (n, 6)).data_ptr()
        out = dict(out) if out is not None else {}
        stray = [k for k in out if k not in want]
        if stray:
            raise ValueError(f"out: {stray} not in want")
        result = {}
        for name in want:
            dtype, width = self.SURFACE_OUTPUTS[name]
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), (n, width) if width else (n,))
            setattr(q, name + "_out", result[name].data_ptr() or None)
        # (an empty batch has no device pointers; the native call checks everything else and launches nothing)
        stats = call.run(self._lib.rayca_hip_surface_device, q, context=context, want_stats=want_stats)
        if stats is not None:
            result["stats"] = stats
        return result

    def gbuffer(self, config: Config, width: int, height: int, *, sample=0,
                want=("point", "normal", "color", "diffuse", "specular", "rough", "material", "flags"), stream=None, context=0):
        """The surface under every pixel of a frame: camera_rays -> query(closest) -> surface on one stream, nothing waited for
        in between.  Returns surface()'s dict plus "t" and "prim", every tensor shaped (height, width, ...)."""
        rays = self.camera_rays(config, width, height, sample=sample, stream=stream, context=context)
        t, prim, uv = self.query(rays, stream=stream, context=context)
        g = self.surface(rays, t, prim, uv, want=want, stream=stream, context=context)
        g["t"], g["prim"] = t, prim
        return {k: v.reshape(height, width, *v.shape[1:]) for k, v in g.items()}

    # ---- ambient occlusion: hemisphere visibility at points (rayca_hip_ambient_device) ----
    AMBIENT_OUTPUTS = {"mask": ("int64", 0), "hits": ("int32", 0), "open": ("float32", 0), "bent": ("float32", 3)}

    def _ambient_table(self, call, n):
        """cosine_directions(n) on the scene's device, made once per n"""
        cache = self.__dict__.setdefault("_ambient_tables", {})
        if n not in cache:
            from .ambient import cosine_directions
            cache[n] = call.torch.from_numpy(cosine_directions(n)).to(call.dev)
        return cache[n]

    def ambient(self, points, normals, *, samples=16, radius=None, bias=0.0, dirs=None, dir_first=0, rotations=None,
                want=("open",), stream=None, context=0, out=None, want_stats=False, collect_stats=False):
        """rayca_hip_ambient_device: how open the scene is at points in device memory -- `samples` occlusion rays over the
        hemisphere of each normal, made inside the traversal kernel, one record per point -- asynchronously.

        points, normals: torch tensors (N, 3) float32 on this scene's device, as surface() / gbuffer() return them (a zero normal,
        surface()'s miss, or a value that is not finite marks an inactive point: open 1).  samples: 1..64.  radius: None
        (unbounded), a float for every point, or an (N,) float32 tensor; a ray is occluded iff it hits at t < radius.  bias: the
        origin is point + normal * bias.  dirs: (M, 3) float32 local directions, z along the normal (None: cosine_directions(samples),
        kept on the device); sample j takes dirs[dir_first + j].  rotations: (N, 2) float32 (cos, sin) that turn the table about
        the normal per point (pixel_rotations), or None.  Returns a dict with one tensor per name in `want`: "mask" (N,) int64
        holding the u64 whose bit j says sample j is occluded, "hits" (N,) int32, "open" (N,) float32 = (samples - hits) /
        samples, "bent" (N, 3) float32, the unnormalised sum of the unoccluded directions.  `out`: a dict of tensors to write
        instead of new ones.  Stream handling as query(); `want_stats` / `collect_stats` wait and add "stats"."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        want = tuple(want)
        unknown = [w for w in want if w not in self.AMBIENT_OUTPUTS]
        if unknown or not want or len(set(want)) != len(want):
            raise ValueError(f"want: a non-empty selection without repeats of {tuple(self.AMBIENT_OUTPUTS)}, not {want!r}")
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor on {call.dev} is expected, not {type(points).__name__}")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: shape {tuple(points.shape)}, expected (N, 3)")
        n = points.shape[0]
        if not 1 <= samples <= 64:
            raise ValueError(f"samples: {samples}, expected 1..64")
        if n * samples >= 1 << 32:
            raise ValueError("points: the number of points x samples must stay below 2**32")
        if dirs is None:
            dirs, dir_first = self._ambient_table(call, samples), 0
        if not isinstance(dirs, torch.Tensor):
            raise TypeError(f"dirs: a torch tensor on {call.dev} is expected, not {type(dirs).__name__}")
        if dirs.dim() != 2 or dirs.shape[1] != 3:
            raise ValueError(f"dirs: shape {tuple(dirs.shape)}, expected (M, 3)")
        m = dirs.shape[0]
        if dir_first < 0 or dir_first + samples > m:
            raise ValueError(f"dir_first: {dir_first} + samples {samples} exceeds the {m} directions of dirs")
        out = dict(out) if out is not None else {}
        stray = [k for k in out if k not in want]
        if stray:
            raise ValueError(f"out: {stray} not in want")
        a = abi.RaycaAmbient()
        a.count, a.samples, a.dir_count, a.dir_first, a.bias = n, samples, m, dir_first, float(bias)
        result = {}
        for name in want:
            dtype, width = self.AMBIENT_OUTPUTS[name]
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), (n, width) if width else (n,))
            setattr(a, name + "_out", result[name].data_ptr() or None)
        a.points = call.input(points, "points", torch.float32, (n, 3)).data_ptr()
        a.normals = call.input(normals, "normals", torch.float32, (n, 3)).data_ptr()
        a.dirs = call.input(dirs, "dirs", torch.float32, (m, 3)).data_ptr()
        if rotations is not None:
            a.rotations = call.input(rotations, "rotations", torch.float32, (n, 2)).data_ptr()
        if radius is None:
            a.radius_all = float("inf")
        elif isinstance(radius, torch.Tensor):
            a.radius = call.input(radius, "radius", torch.float32, (n,)).data_ptr()
        else:
            a.radius_all = float(radius)
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_ambient_device, a, context=context, want_stats=want_stats or collect_stats,
                             collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is not None:
            result["stats"] = stats
        return result

    def render_ambient(self, config: Config, width: int, height: int, *, samples=16, radius=None, bias=1e-3, rotate=True,
                       stream=None, context=0):
        """An ambient-occlusion image without a render call: gbuffer() -> ambient() on one stream, nothing waited for in between.
        Returns the (height, width) float32 openness, 1 where nothing is occluded; a pixel whose camera ray misses is exactly 1
        (its normal is zero: an inactive point).  bias, in world units, lifts the origins off the surface; `rotate` turns the
        direction table per pixel (pixel_rotations)."""
        call = _DeviceCall(self, stream)
        g = self.gbuffer(config, width, height, want=("point", "normal"), stream=stream, context=context)
        rotations = None
        if rotate:
            from .ambient import pixel_rotations
            rotations = call.torch.from_numpy(pixel_rotations(width, height).reshape(-1, 2)).to(call.dev)
        a = self.ambient(g["point"].reshape(-1, 3), g["normal"].reshape(-1, 3), samples=samples, radius=radius, bias=bias, rotations=rotations,
                         stream=stream, context=context)
        return a["open"].reshape(height, width)

    # ---- radiance along the caller's rays (rayca_hip_radiance_device) ----
    def radiance(self, rays, config: Config, *, sample=0, first_index=0, rgba8=False, out=None, stream=None, context=0,
                 want_stats=False, collect_stats=False):
        """rayca_hip_radiance_device: the light that arrives along rays in device memory, asynchronously.

        rays: torch tensor (N, 6) float32 on this scene's device (origin xyz, direction xyz), any rays: another camera model,
        probe directions, a frame's own camera_rays().  Row i of the result is the pixel of a one-sample frame of `config` whose
        camera ray is rays[i] and whose pixel index is first_index + i: the integrator's value, alpha 1, through `config.gamma`;
        the path draws from the random stream of (config.seed, first_index + i, sample).  Several samples are several calls with
        different `sample`; consecutive chunks of a ray set, each with the first_index of its first ray, give what one call
        gives.  Flat, and the Pathtracer configs the generation kernels render, are offered (else RaycaError ERR_UNSUPPORTED
        naming the field); config.samples_per_pixel is not read.  Returns the (N, 4) float32 tensor (`out`: the tensor to
        write), with rgba8=True (or the tensor to write) also the (N, 4) uint8 one, and the stats dict behind them when
        `want_stats` / `collect_stats` ask for it (the call then waits).  Stream handling as query()."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError(f"rays: a torch tensor on {call.dev} is expected, not {type(rays).__name__}")
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError(f"rays: shape {tuple(rays.shape)}, expected (N, 6)")
        n = rays.shape[0]
        if first_index < 0 or first_index + n > 1 << 32:
            raise ValueError("first_index + the number of rays exceeds 2**32")
        out = call.output(out, "out", torch.float32, (n, 4))
        out8 = call.output(rgba8, "rgba8", torch.uint8, (n, 4), optional=True)
        r = abi.RaycaRadiance()
        r.count, r.sample, r.first_index = n, sample, first_index
        r.rays = call.input(rays, "rays", torch.float32, (n, 6)).data_ptr() or None
        r.rgba32f_out, r.rgba8_out = out.data_ptr() or None, _ptr(out8) or None
        cfg = config.to_abi()
        fn = self._lib.rayca_hip_radiance_device
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(lambda handle, o, args, st: fn(handle, C.byref(cfg), o, args, st), r, context=context,
                             want_stats=want_stats or collect_stats, collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        return _asked_for(out, out8, stats)

    # ---- irradiance at points: radiance over a hemisphere of rays, folded (rayca_hip_gather_device) ----
    GATHER_OUTPUTS = {"irradiance": ("float32", lambda n, s: (n, 4)), "sh": ("float32", lambda n, s: (n, 9, 4)),
                      "kept": ("int32", lambda n, s: (n,)), "samples": ("float32", lambda n, s: (n, s, 4))}

    def gather(self, points, normals, config: Config, *, samples, dirs=None, weights=None, rotations=None, dir_first=0, bias=0.0,
               sample=0, first_index=0, chunk_points=0, outputs=("irradiance",), stream=None, context=0, out=None, want_stats=False,
               collect_stats=False):
        """rayca_hip_gather_device: the light that arrives at points in device memory -- `samples` rays over the hemisphere of each
        normal, ambient()'s rays made on the device, the radiance() of `config` along each, folded per point in a fixed order --
        asynchronously.

        points, normals, dirs, dir_first, rotations, bias: as for ambient() (a zero normal or a value that is not finite marks an
        inactive point: zeros); `samples` (1..64) has no default, bias is 0 unless given.  weights: (M,) float32, one per direction of dirs, multiplied into the samples (None: none).
        config: a Config radiance() serves, with gamma 1.  Ray j of point i is "pixel" first_index + i * samples + j of a
        radiance() call with the same `sample`.  chunk_points: at most this many points per internal frame (0: the library's
        choice); the results do not depend on it.  Returns a dict with one tensor per name in `outputs`: "irradiance" (N, 4) float32
        (the mean r, g, b of the samples that are finite, and the fraction that are), "sh" (N, 9, 4) float32 (the mean of
        sample x Y_k(direction), k = 0..8, in r, g, b), "kept" (N,) int32 (the number of finite samples), "samples" (N, samples, 4)
        float32 (the radiance itself).  With cosine_directions and no weights, irradiance is the irradiance / pi.  `out`: a dict of
        tensors to write instead of new ones.  Stream handling as query(); `want_stats` / `collect_stats` wait and add "stats"."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        outputs = tuple(outputs)
        unknown = [w for w in outputs if w not in self.GATHER_OUTPUTS]
        if unknown or not outputs or len(set(outputs)) != len(outputs):
            raise ValueError(f"outputs: a non-empty selection without repeats of {tuple(self.GATHER_OUTPUTS)}, not {outputs!r}")
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor on {call.dev} is expected, not {type(points).__name__}")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: shape {tuple(points.shape)}, expected (N, 3)")
        n = points.shape[0]
        if not 1 <= samples <= 64:
            raise ValueError(f"samples: {samples}, expected 1..64")
        if n * samples > 1 << 31 or first_index < 0 or first_index + n * samples > 1 << 32:
            raise ValueError("points: points x samples must stay within 2**31, and first_index + points x samples within 2**32")
        if dirs is None:
            dirs, dir_first = self._ambient_table(call, samples), 0
        if not isinstance(dirs, torch.Tensor):
            raise TypeError(f"dirs: a torch tensor on {call.dev} is expected, not {type(dirs).__name__}")
        if dirs.dim() != 2 or dirs.shape[1] != 3:
            raise ValueError(f"dirs: shape {tuple(dirs.shape)}, expected (M, 3)")
        m = dirs.shape[0]
        if dir_first < 0 or dir_first + samples > m:
            raise ValueError(f"dir_first: {dir_first} + samples {samples} exceeds the {m} directions of dirs")
        if chunk_points < 0:
            raise ValueError(f"chunk_points: {chunk_points}, expected 0 or a positive number of points")
        out = dict(out) if out is not None else {}
        stray = [k for k in out if k not in outputs]
        if stray:
            raise ValueError(f"out: {stray} not in outputs")
        g = abi.RaycaGather()
        g.count, g.samples, g.dir_count, g.dir_first, g.bias = n, samples, m, dir_first, float(bias)
        g.sample, g.first_index, g.chunk_points = sample, first_index, min(chunk_points, 0xFFFFFFFF)
        result = {}
        for name in outputs:
            dtype, shape = self.GATHER_OUTPUTS[name]
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), shape(n, samples))
            setattr(g, name + "_out", result[name].data_ptr() or None)
        g.points = call.input(points, "points", torch.float32, (n, 3)).data_ptr()
        g.normals = call.input(normals, "normals", torch.float32, (n, 3)).data_ptr()
        g.dirs = call.input(dirs, "dirs", torch.float32, (m, 3)).data_ptr()
        if weights is not None:
            g.weights = call.input(weights, "weights", torch.float32, (m,)).data_ptr()
        if rotations is not None:
            g.rotations = call.input(rotations, "rotations", torch.float32, (n, 2)).data_ptr()
        cfg = config.to_abi()
        fn = self._lib.rayca_hip_gather_device
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(lambda handle, o, args, st: fn(handle, C.byref(cfg), o, args, st), g, context=context,
                             want_stats=want_stats or collect_stats, collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is not None:
            result["stats"] = stats
        return result

    def render_irradiance(self, config: Config, width: int, height: int, *, samples, bias, rotate=True, sample=0,
                          outputs=("irradiance",), stream=None, context=0):
        """The light that arrives at the surface under every pixel, without a render call: gbuffer() -> gather() on one stream,
        nothing waited for in between.  Returns gather()'s dict with every tensor shaped (height, width, ...); a pixel whose
        camera ray misses is all zeros (its normal is zero: an inactive point).  bias, in world units, lifts the origins off the
        surface; `rotate` turns the direction table per pixel (pixel_rotations).  `samples` and `bias` have no defaults: both
        decide what the picture means."""
        call = _DeviceCall(self, stream)
        g = self.gbuffer(config, width, height, want=("point", "normal"), stream=stream, context=context)
        rotations = None
        if rotate:
            from .ambient import pixel_rotations
            rotations = call.torch.from_numpy(pixel_rotations(width, height).reshape(-1, 2)).to(call.dev)
        r = self.gather(g["point"].reshape(-1, 3), g["normal"].reshape(-1, 3), config, samples=samples, bias=bias, rotations=rotations,
                        sample=sample, outputs=outputs, stream=stream, context=context)
        return {k: v.reshape(height, width, *v.shape[1:]) for k, v in r.items()}

    # ---- irradiance volumes: the light at points from a grid of SH9 probes (rayca_hip_probe_lookup_device) ----
    PROBE_OUTPUTS = {"irradiance": ("float32", lambda n: (n, 4)), "sh": ("float32", lambda n: (n, 9, 4)), "mask": ("int32", lambda n: (n,)),
                     "radiance": ("float32", lambda n: (n, 4))}

    def probe_lookup(self, points, normals, grid, sh, *, kept=None, visibility=True, normal_term=True, bias=0.0, albedo=None, base=None,
                     outputs=("irradiance",), stream=None, context=0, out=None, want_stats=False, collect_stats=False):
        """rayca_hip_probe_lookup_device: the diffuse light at points in device memory from a grid of SH9 probes -- the eight probes
        of each point's cell blended by trilinear weight, the normal term and one short occlusion ray per probe -- asynchronously.

        points, normals: as for ambient() (a zero normal or a value that is not finite marks an inactive point: zeros).  grid: a
        probes.ProbeGrid (origin, cell, dims).  sh: (M, 9, 4) float32, M = the grid's probe count: gather()'s "sh" at the probes'
        centres (ProbeGrid.bake).  kept: (M,) int32, gather()'s "kept", or None; a probe with kept 0 is left out.  visibility: trace
        the corner rays (from point + normal * bias to each probe's centre); normal_term: weigh probes in front of the surface
        higher.  albedo, base: (N, 4) float32; "radiance" = albedo * irradiance / pi + base needs albedo.  Returns a dict with one
        tensor per name in `outputs`: "irradiance" (N, 4) float32 (r, g, b, the weight sum), "sh" (N, 9, 4) float32 (the blended
        coefficients), "mask" (N,) int32 (bits 0..7 the candidate corners, 8..15 the occluded ones, bit 16 the fallback), "radiance"
        (N, 4) float32.  `out`: a dict of tensors to write instead of new ones.  Stream handling as query(); `want_stats` /
        `collect_stats` wait and add "stats"."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        outputs = tuple(outputs)
        unknown = [w for w in outputs if w not in self.PROBE_OUTPUTS]
        if unknown or not outputs or len(set(outputs)) != len(outputs):
            raise ValueError(f"outputs: a non-empty selection without repeats of {tuple(self.PROBE_OUTPUTS)}, not {outputs!r}")
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor on {call.dev} is expected, not {type(points).__name__}")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: shape {tuple(points.shape)}, expected (N, 3)")
        n = points.shape[0]
        if n * 8 >= 1 << 32:
            raise ValueError("points: the number of points x 8 must stay below 2**32")
        dims = tuple(int(d) for d in grid.dims)
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > 1 << 24:
            raise ValueError(f"grid.dims: {dims}, expected three counts >= 1 with a product of at most 2**24")
        m = dims[0] * dims[1] * dims[2]
        if "radiance" in outputs and albedo is None:
            raise ValueError('outputs: "radiance" needs albedo')
        out = dict(out) if out is not None else {}
        stray = [k for k in out if k not in outputs]
        if stray:
            raise ValueError(f"out: {stray} not in outputs")
        a = abi.RaycaProbeLookup()
        a.count, a.bias = n, float(bias)
        a.flags = (abi.PROBE_VISIBILITY if visibility else 0) | (abi.PROBE_NORMAL_TERM if normal_term else 0)
        for k in range(3):
            a.origin[k], a.cell[k], a.dims[k] = float(grid.origin[k]), float(grid.cell[k]), dims[k]
        result = {}
        for name in outputs:
            dtype, shape = self.PROBE_OUTPUTS[name]
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), shape(n))
            setattr(a, name + "_out", result[name].data_ptr() or None)
        a.points = call.input(points, "points", torch.float32, (n, 3)).data_ptr()
        a.normals = call.input(normals, "normals", torch.float32, (n, 3)).data_ptr()
        a.sh = call.input(sh, "sh", torch.float32, (m, 9, 4)).data_ptr()
        if kept is not None:
            a.kept = call.input(kept, "kept", torch.int32, (m,)).data_ptr()
        if albedo is not None:
            a.albedo = call.input(albedo, "albedo", torch.float32, (n, 4)).data_ptr()
        if base is not None:
            a.base = call.input(base, "base", torch.float32, (n, 4)).data_ptr()
        stats = None
        if n:   # (an empty batch has no device pointers to hand over; the native call would launch nothing either)
            stats = call.run(self._lib.rayca_hip_probe_lookup_device, a, context=context, want_stats=want_stats or collect_stats,
                             collect_stats=collect_stats)
        elif context >= 8:
            raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
        elif want_stats or collect_stats:
            stats = abi.RaycaStats().as_dict()
        if stats is not None:
            result["stats"] = stats
        return result

    def render_probe_lit(self, width: int, height: int, grid, sh, *, config: Optional[Config] = None, kept=None, visibility=True,
                         normal_term=True, bias=1e-3, albedo="color", base=None, stream=None, context=0):
        """A frame lit by a probe grid, without a render call: gbuffer() -> probe_lookup() on one stream, nothing waited for in
        between.  Returns the (height, width, 4) float32 radiance: the surface's `albedo` output ("color" or "diffuse") x the
        blended irradiance / pi, plus `base` (an (height, width, 4) direct-light frame) when given; a pixel whose camera ray misses
        is base's pixel, or (0, 0, 0, 1).  config: the camera rays' Config (None: Config()).  bias, in world units, lifts the
        origins of the corner rays off the surface."""
        if albedo not in ("color", "diffuse"):
            raise ValueError(f'albedo: {albedo!r}, expected "color" or "diffuse"')
        g = self.gbuffer(config if config is not None else Config(), width, height, want=("point", "normal", albedo), stream=stream, context=context)
        r = self.probe_lookup(g["point"].reshape(-1, 3), g["normal"].reshape(-1, 3), grid, sh, kept=kept, visibility=visibility,
                              normal_term=normal_term, bias=bias, albedo=g[albedo].reshape(-1, 4),
                              base=base.reshape(-1, 4) if base is not None else None, outputs=("radiance",), stream=stream, context=context)
        return r["radiance"].reshape(height, width, 4)

    # ---- direct light at points: the NEE sum of a path vertex without the BRDF (rayca_hip_direct_device) ----
    DIRECT_OUTPUTS = {"irradiance": ("float32", lambda n: (n, 4)), "sh": ("float32", lambda n: (n, 9, 4)), "mask": ("int64", lambda n: (n,)),
                      "counts": ("int32", lambda n: (n,))}

    def lights(self) -> np.ndarray:
        """rayca_hip_scene_read_lights: the scene's light records as the kernels read them (after update(): the updated ones), a
        structured array with the fields of abi.RaycaLightRecord: kind, material, intensity, area, color, attenuation, position
        (the translation of the light node's LOCAL transform), ab, ac, normal."""
        n = C.c_uint32(0)
        lib.check(self._lib.rayca_hip_scene_read_lights(self.handle, None, 0, C.byref(n)))
        out = (abi.RaycaLightRecord * max(n.value, 1))()
        if n.value:
            lib.check(self._lib.rayca_hip_scene_read_lights(self.handle, out, n.value, None))
        return np.ctypeslib.as_array(out)[:n.value].copy()

    def torch_stream(self, stream=None):
        """the torch stream object a device call with this `stream` argument runs on (for torch work queued behind it)"""
        return _DeviceCall(self, stream).torch_stream()

    def direct(self, points, normals, config: Config, *, light_first=0, light_count=None, sample=0, first_index=0, bias=0.0,
               want=("irradiance",), out=None, stream=None, context=0, want_stats=False, collect_stats=False):
        """rayca_hip_direct_device: the light that arrives at points in device memory straight from the scene's point and quad
        lights -- the next-event-estimation sum of a path vertex with the BRDF taken out -- asynchronously.

        points: (N, 3) float32.  normals: (N, 3) float32 -- hemisphere mode: the cosine-weighted irradiance E at a surface point
        (a Lambert surface radiates albedo * E / pi), rays from point + normal * bias (bias = 1e-4 reproduces a path vertex), a
        zero normal or a value that is not finite marks an inactive point -- or None -- sphere mode: the incident radiance times
        solid angle, no cosine, bias must be 0, and "sh" is available: its SH9 projection, in the units of gather()'s "sh" under
        sphere_directions with weights of 4 pi, so the two add.  config: its light_samples, light_stratify and seed are read.
        Lights light_first .. light_first + light_count (None: to the scene's last).  Point i draws a quad light's points from
        the stream of "pixel" first_index + i of a radiance() call with the same `sample`.
        Returns a dict with one tensor per name in `want`: "irradiance" (N, 4) float32 (r, g, b, the lit fraction of the samples),
        "sh" (N, 9, 4) float32, "mask" (N, C) int64 (one word per chunk of lights, C = 1 unless the range needs more than 64
        samples; bit j of a word = sample j of that chunk was traced and lit), "counts"
        (N,) int32 (lit samples in the low 16 bits, dropped ones -- a component that is not finite -- in the high 16).
        One native call serves at most 64 samples (lights x light_samples).  A longer range is cut into chunks of whole lights;
        irradiance, sh and counts are summed on the device, chunk by chunk, and "mask" holds one word per chunk.  Across chunk
        borders that sum is not the single fold in sample order: equal to rounding, not to the bit.  `out`: a dict of tensors to
        write instead of new ones.  Stream handling as query(); `want_stats` / `collect_stats` wait and add "stats" (summed)."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        want = tuple(want)
        unknown = [w for w in want if w not in self.DIRECT_OUTPUTS]
        if unknown or not want or len(set(want)) != len(want):
            raise ValueError(f"want: a non-empty selection without repeats of {tuple(self.DIRECT_OUTPUTS)}, not {want!r}")
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor on {call.dev} is expected, not {type(points).__name__}")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: shape {tuple(points.shape)}, expected (N, 3)")
        n = points.shape[0]
        if "sh" in want and normals is not None:
            raise ValueError('want: "sh" is a sphere-mode output (normals=None)')
        if first_index < 0 or first_index + n > 1 << 32:
            raise ValueError("first_index + points must stay within 2**32")
        ls = int(config.light_samples)
        if not 1 <= ls <= 64:
            raise ValueError(f"config.light_samples: {ls}, expected 1..64")
        total = self.info()["light_count"]
        if light_count is None:
            light_count = total - light_first
        if light_first < 0 or light_count < 1 or light_first + light_count > total:
            raise ValueError(f"lights {light_first} .. {light_first + light_count}: the scene has {total}")
        per = 64 // ls
        chunks = [(a, min(per, light_first + light_count - a)) for a in range(light_first, light_first + light_count, per)]
        out = dict(out) if out is not None else {}
        stray = [k for k in out if k not in want]
        if stray:
            raise ValueError(f"out: {stray} not in want")
        result = {}
        for name in want:
            dtype, shape = self.DIRECT_OUTPUTS[name]
            shp = (n, len(chunks)) if name == "mask" else shape(n)
            result[name] = call.output(out.get(name), f"out[{name!r}]", getattr(torch, dtype), shp)
        p = call.input(points, "points", torch.float32, (n, 3))
        nrm = call.input(normals, "normals", torch.float32, (n, 3)) if normals is not None else None
        cfg = config.to_abi()
        fn = self._lib.rayca_hip_direct_device
        stats = None
        if n == 0:
            if context >= 8:
                raise lib.RaycaError(abi.ERR_BAD_ARG, "context out of range")
            if want_stats or collect_stats:
                stats = abi.RaycaStats().as_dict()
        for c, (first, cnt) in enumerate(chunks if n else ()):
            d = abi.RaycaDirect()
            d.count, d.light_first, d.light_count, d.sample, d.first_index, d.bias = n, first, cnt, sample, first_index, float(bias)
            d.points, d.normals = p.data_ptr(), nrm.data_ptr() if nrm is not None else None
            part = {}
            for name in want:
                if name == "mask":
                    part[name] = result[name][:, 0] if len(chunks) == 1 else torch.empty((n,), dtype=torch.int64, device=call.dev)
                elif c == 0:
                    part[name] = result[name]
                else:
                    part[name] = torch.empty_like(result[name])
                setattr(d, name + "_out", part[name].data_ptr() or None)
            st = call.run(lambda handle, o, args, s_: fn(handle, C.byref(cfg), o, args, s_), d, context=context,
                          want_stats=want_stats or collect_stats, collect_stats=collect_stats)
            if st is not None:
                if stats is None:
                    stats = st
                else:
                    for k, v in st.items():
                        if isinstance(v, (int, float)) and k != "node_format":
                            stats[k] += v
                        elif isinstance(v, list):
                            stats[k] = [a + b for a, b in zip(stats[k], v)]
            if len(chunks) > 1:
                with torch.cuda.stream(call.torch_stream()):
                    for name in want:
                        if name == "mask":
                            result[name][:, c] = part[name]
                        elif c > 0 and name == "irradiance":   # (the lit fractions are re-weighted by their sample counts below)
                            result[name][:, :3] += part[name][:, :3]
                            result[name][:, 3] += part[name][:, 3] * float(cnt * ls)
                        elif c > 0:
                            result[name] += part[name]
                        elif name == "irradiance":
                            result[name][:, 3] *= float(cnt * ls)
                    for x in part.values():
                        x.record_stream(call.torch_stream())
        if n and len(chunks) > 1 and "irradiance" in want:
            with torch.cuda.stream(call.torch_stream()):
                result["irradiance"][:, 3] /= float(light_count * ls)
        if stats is not None:
            result["stats"] = stats
        return result

    # ---- the denoiser: an edge-avoiding a-trous filter on a frame and its G-buffer (rayca_hip_denoise_device) ----
    def denoise(self, color, *, albedo=None, normal=None, point=None, id=None, iterations=5, sigma_color=4.0, sigma_plane=None,
                normal_power_log2=7, gamma=1.0, out=None, rgba8=False, stream=None, context=0, want_stats=False):
        """rayca_hip_denoise_device: the edge-avoiding a-trous filter, asynchronously, everything in device memory.

        color (H, W, 4) float32: a frame rendered with gamma 1 (render_device's float output).  Guides, each optional, as
        gbuffer() returns them: albedo (H, W, 4) float32 (the colour is divided by max(albedo, 1e-3) in front of the filter and
        multiplied with it behind), normal and point (H, W, 3) float32 (point needs normal and a sigma_plane > 0, in world
        units), id (H, W) int32 (a tap counts only where the ids are equal: material, prim, ...).  iterations 0..8, iteration i
        with step 2**i; 0 runs the output stage alone.  sigma_color <= 0 switches the colour term off; the normal weight is
        max(0, n_p . n_q) squared normal_power_log2 times.  `gamma` is applied to the result as a render call applies
        Config.gamma.  `out`: the (H, W, 4) float32 tensor to write (may be `color` itself), else a new one; rgba8=True adds an
        (H, W, 4) uint8 tensor (or pass the tensor to write).  Stream handling as query().  Returns the float tensor, or a
        tuple with the uint8 tensor and the stats dict (`want_stats` waits) behind it when asked for.

        The defaults are starting values: nobody has tuned them on rendered frames."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        if point is not None and sigma_plane is None:
            raise ValueError("sigma_plane: needed with point")
        d = abi.RaycaDenoise()
        d.width, d.height, d.iterations, d.normal_power_log2 = w, h, iterations, normal_power_log2
        d.sigma_color, d.sigma_plane, d.gamma = sigma_color, (sigma_plane if sigma_plane is not None else 0.0), gamma
        out = call.output(out, "out", torch.float32, (h, w, 4))
        out8 = call.output(rgba8, "rgba8", torch.uint8, (h, w, 4), optional=True)
        d.color = call.input(color, "color", torch.float32, (h, w, 4)).data_ptr()
        call.guides(d, h, w, albedo=albedo, normal=normal, point=point, id=id)
        d.rgba32f_out, d.rgba8_out = out.data_ptr(), _ptr(out8)
        stats = call.run(self._lib.rayca_hip_denoise_device, d, context=context, want_stats=want_stats)
        return _asked_for(out, out8, stats)

    DENOISE_GUIDES = {"albedo": "color", "normal": "normal", "point": "point", "id": "material"}   # guide -> surface output

    def _guide_selection(self, guides):
        guides = tuple(guides)
        unknown = [g for g in guides if g not in self.DENOISE_GUIDES]
        if unknown or len(set(guides)) != len(guides):
            raise ValueError(f"guides: a selection without repeats of {tuple(self.DENOISE_GUIDES)}, not {guides!r}")
        return guides

    def _render_linear(self, config, width, height, stream, context):
        """render_device with gamma forced to 1 into a new (height, width, 4) float32 tensor, nothing waited for"""
        import dataclasses
        call = _DeviceCall(self, stream)
        color = call.output(None, "color", call.torch.float32, (height, width, 4))
        self.render_device(dataclasses.replace(config, gamma=1.0), width, height, 0, color.data_ptr(), stream=call.handle or None, context=context)
        return color

    def render_denoised(self, config: Config, width: int, height: int, *, guides=("albedo", "normal", "point", "id"), stream=None,
                        context=0, **denoise_kw):
        """A frame, its G-buffer and the filter on one stream, nothing waited for in between: render_device with gamma forced
        to 1 into a tensor, gbuffer() for the guides asked for (albedo = the surface's color, id = its material), then
        denoise(..., gamma=config.gamma) in place.  Returns what denoise() returns; `denoise_kw` are its keywords (with the
        "point" guide sigma_plane defaults to 0.1 world units -- a starting value like the others)."""
        guides = self._guide_selection(guides)
        if "gamma" in denoise_kw or "out" in denoise_kw:
            raise ValueError("gamma comes from config, and the frame is filtered in place")
        color = self._render_linear(config, width, height, stream, context)
        kw = dict(denoise_kw)
        if guides:
            g = self.gbuffer(config, width, height, want=tuple(self.DENOISE_GUIDES[k] for k in guides), stream=stream, context=context)
            kw.update({k: g[self.DENOISE_GUIDES[k]] for k in guides})
        if "point" in guides and kw.get("sigma_plane") is None:
            kw["sigma_plane"] = 0.1
        return self.denoise(color, gamma=config.gamma, out=color, stream=stream, context=context, **kw)

    # ---- the variance-guided filter: the stage behind accumulate() (rayca_hip_denoise_variance_device) ----
    def denoise_variance(self, color, variance, *, length=None, min_history=4, sigma_luminance=4.0, variance_floor=1e-10, variance_out=False,
                         albedo=None, normal=None, point=None, id=None, iterations=5, sigma_plane=None, normal_power_log2=7, gamma=1.0,
                         out=None, rgba8=False, stream=None, context=0, want_stats=False):
        """rayca_hip_denoise_variance_device: the variance-guided a-trous filter, asynchronously, everything in device memory.

        color (H, W, 4) float32 and variance (H, W) float32: a film and its luminance variance as accumulate(variance=True)
        returns them; length (H, W) float32 its history length -- with it the variance becomes that of the film's mean, so the
        filter backs off as the film converges, and a pixel whose length is below min_history takes a spatial variance estimate
        from its 7 x 7 neighbourhood (min_history 0: never; without `length` min_history is not used).  The luminance weight of a
        tap is 1 / (1 + d^2 / (sigma_luminance^2 * variance + variance_floor)), the variance being prefiltered 3 x 3; the variance
        is filtered along with the colour.  Guides, iterations (1..8 here), sigma_plane, normal_power_log2, gamma, out, rgba8 and
        the stream handling are denoise()'s.  variance_out=True adds the filtered variance as an (H, W) float32 tensor (or pass
        the tensor to write, which may be `variance` itself); it is in the units the filter ran in, demodulated where there is
        an albedo.  Returns the float tensor, or a tuple with the uint8 tensor, the variance and the stats dict (`want_stats`
        waits) behind it, each when asked for.

        The defaults are untuned starting values: nobody has tuned them on rendered frames."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        if point is not None and sigma_plane is None:
            raise ValueError("sigma_plane: needed with point")
        d = abi.RaycaDenoiseVariance()
        d.width, d.height, d.iterations, d.normal_power_log2 = w, h, iterations, normal_power_log2
        d.min_history = min_history if length is not None else 0
        d.sigma_luminance, d.sigma_plane, d.variance_floor, d.gamma = sigma_luminance, (sigma_plane if sigma_plane is not None else 0.0), variance_floor, gamma
        out = call.output(out, "out", torch.float32, (h, w, 4))
        out8 = call.output(rgba8, "rgba8", torch.uint8, (h, w, 4), optional=True)
        var_out = call.output(variance_out, "variance_out", torch.float32, (h, w), optional=True)
        d.color = call.input(color, "color", torch.float32, (h, w, 4)).data_ptr()
        d.variance = call.input(variance, "variance", torch.float32, (h, w)).data_ptr()
        if length is not None:
            d.length = call.input(length, "length", torch.float32, (h, w)).data_ptr()
        call.guides(d, h, w, albedo=albedo, normal=normal, point=point, id=id)
        d.rgba32f_out, d.rgba8_out, d.variance_out = out.data_ptr(), _ptr(out8), _ptr(var_out)
        stats = call.run(self._lib.rayca_hip_denoise_variance_device, d, context=context, want_stats=want_stats)
        return _asked_for(out, out8, var_out, stats)

    # ---- guided upsampling: a low-resolution frame onto a full-size G-buffer (rayca_hip_upsample_device) ----
    # guide -> (dtype, channels, the keys of a gbuffer() dict it is taken from, the first one present)
    UPSAMPLE_GUIDES = {"albedo": ("float32", 4, ("albedo", "color")), "normal": ("float32", 3, ("normal",)),
                       "point": ("float32", 3, ("point",)), "id": ("int32", 0, ("id", "material"))}

    def upsample(self, color, scale, *, low=None, high=None, sigma_plane=None, normal_power_log2=7, gamma=1.0, out=None, rgba8=False,
                 weight=False, stream=None, context=0, want_stats=False):
        """rayca_hip_upsample_device: a joint bilateral upsample, asynchronously, everything in device memory.

        color (h, w, 4) float32: a frame rendered with gamma 1 at 1 / scale of the output's size (scale 1..8); the output is
        (h * scale, w * scale, 4).  `low` and `high`: dicts as gbuffer() returns them for the low and the full-size view of one
        camera (of a one-sample config).  The keys used are "albedo" (or "color"), "normal", "point" and "id" (or "material");
        a guide is used where both dicts hold it, and a guide in one dict alone is an error.  With the albedo the taps are
        divided by max(albedo, 1e-3) at low resolution and the result is multiplied with the full-size one, so textures come
        from the full-size surface data; normal, point (needs normal and a sigma_plane > 0, in world units) and id weigh the
        four taps of the bilinear footprint as denoise() weighs its taps.  A pixel none of whose taps agrees with its surface
        falls back to plain bilinear; weight=True adds the guided weight sum as an (H, W) float32 tensor, 0 at those pixels
        (or pass the tensor to write).  `gamma`, `out`, `rgba8`, the stream handling and the return convention are
        denoise()'s; no output may be an input.  Returns the float tensor, or a tuple with the uint8 tensor, the weight and the
        stats dict (`want_stats` waits) behind it, each when asked for."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        _scale_ok(scale)
        big_h, big_w = h * scale, w * scale
        low, high = dict(low or {}), dict(high or {})
        u = abi.RaycaUpsample()
        u.width, u.height, u.scale, u.normal_power_log2 = big_w, big_h, scale, normal_power_log2
        u.sigma_plane, u.gamma = (sigma_plane if sigma_plane is not None else 0.0), gamma
        out = call.output(out, "out", torch.float32, (big_h, big_w, 4))
        out8 = call.output(rgba8, "rgba8", torch.uint8, (big_h, big_w, 4), optional=True)
        weight_out = call.output(weight, "weight", torch.float32, (big_h, big_w), optional=True)
        u.color = call.input(color, "color", torch.float32, (h, w, 4)).data_ptr()
        for guide, (dtype, channels, keys) in self.UPSAMPLE_GUIDES.items():
            found = [next((d[k] for k in keys if d.get(k) is not None), None) for d in (low, high)]
            if (found[0] is None) != (found[1] is None):
                raise ValueError(f"{guide}: in `low` and in `high`, or in neither")
            if found[0] is None:
                continue
            if guide == "point" and sigma_plane is None:
                raise ValueError("sigma_plane: needed with point")
            for x, where, field, (gh, gw) in ((found[0], "low", guide + "_low", (h, w)), (found[1], "high", guide, (big_h, big_w))):
                shape = (gh, gw, channels) if channels else (gh, gw)
                setattr(u, field, call.input(x, f"{where}[{guide!r}]", getattr(torch, dtype), shape).data_ptr())
        u.rgba32f_out, u.rgba8_out, u.weight_out = out.data_ptr(), _ptr(out8), _ptr(weight_out)
        stats = call.run(self._lib.rayca_hip_upsample_device, u, context=context, want_stats=want_stats)
        return _asked_for(out, out8, weight_out, stats)

    def upsample_guides(self, width: int, height: int, scale: int, *, guides=("albedo", "normal", "point", "id"), stream=None, context=0):
        """The two G-buffers upsample() takes, (low, high): gbuffer() of a one-sample config at width / scale x height / scale and
        at width x height for the guides asked for (albedo = the surface's color, id = its material), on one stream."""
        guides = self._guide_selection(guides)
        _scale_ok(scale, width, height)
        if not guides:
            return {}, {}
        one = Config(samples_per_pixel=1)   # (points on the rays through pixel centres)
        want = tuple(self.DENOISE_GUIDES[k] for k in guides)
        return tuple({k: g[self.DENOISE_GUIDES[k]] for k in guides}
                     for g in (self.gbuffer(one, width // scale, height // scale, want=want, stream=stream, context=context),
                               self.gbuffer(one, width, height, want=want, stream=stream, context=context)))

    def render_upsampled(self, config: Config, width: int, height: int, scale: int = 2, *, guides=("albedo", "normal", "point", "id"),
                         denoise=False, stream=None, context=0, **upsample_kw):
        """A width x height picture whose lighting is traced at width / scale x height / scale, on one stream, nothing waited
        for in between: render_device of the low view with gamma forced to 1, upsample_guides() for the guides asked for,
        with `denoise` (True, or a dict of denoise()'s keywords) the a-trous filter on the low frame with its low guides and
        gamma 1, then upsample(..., gamma=config.gamma).  Returns what upsample() returns; `upsample_kw` are its keywords (with
        the "point" guide sigma_plane defaults to 0.1 world units -- a starting value like the denoiser's)."""
        if "gamma" in upsample_kw or "low" in upsample_kw or "high" in upsample_kw:
            raise ValueError("gamma comes from config, and the guides from `guides`")
        _scale_ok(scale, width, height)
        color = self._render_linear(config, width // scale, height // scale, stream, context)
        low, high = self.upsample_guides(width, height, scale, guides=guides, stream=stream, context=context)
        kw = dict(upsample_kw)
        if "point" in low and kw.get("sigma_plane") is None:
            kw["sigma_plane"] = 0.1
        if denoise:
            dkw = dict(denoise) if isinstance(denoise, dict) else {}
            if "gamma" in dkw or "out" in dkw or "rgba8" in dkw:
                raise ValueError("denoise: the low frame is filtered in place with gamma 1; gamma and the RGBA8 belong to the upsample")
            if "point" in low and dkw.get("sigma_plane") is None:
                dkw["sigma_plane"] = kw["sigma_plane"]
            self.denoise(color, gamma=1.0, out=color, stream=stream, context=context, **low, **dkw)
        return self.upsample(color, scale, low=low, high=high, gamma=config.gamma, stream=stream, context=context, **kw)

    # ---- exposure metering and tone mapping: a linear frame to a displayable one (rayca_hip_meter_device, rayca_hip_tonemap_device) ----
    def meter(self, color, *, low_permille=10, high_permille=990, key=0.18, min_scale=2.0 ** -10, max_scale=2.0 ** 10, rate=1.0, prev=None,
              out=None, stream=None, context=0, want_stats=False):
        """rayca_hip_meter_device: how bright a frame is, asynchronously, everything in device memory.

        color (H, W, 4) float32, gamma 1.  Returns (hist, exposure): hist (260,) int32 -- 256 luminance bins (8 an octave over
        2^-16 .. 2^16), then the counts of the counted, the black and the non-finite pixels, then 0 -- and exposure (4,)
        float32 {scale, target, L, 0}: L the metered luminance (the mean, in the bins' logarithm, of the counted pixels between
        the low_permille and the high_permille quantile), target = key / L clamped to [min_scale, max_scale], and scale the step
        from prev[0] towards the target by `rate` (0 < rate <= 1: the caller's adaptation factor, for instance
        1 - exp(-dt * speed)); without a usable `prev` (None, or a record whose scale is not positive and finite) the scale is
        the target.  `prev`: a (4,) float32 tensor as this call returns one.  `out`: (hist, exposure) tensors to write instead
        of new ones; exposure may be `prev` itself.  tonemap(exposure=) reads the record where it lies.  Stream handling as
        query(); with `want_stats` (which waits) the stats dict comes third."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        hist, exposure = out if out is not None else (None, None)
        hist = call.output(hist, "out[0]", torch.int32, (abi.METER_WORDS,))
        exposure = call.output(exposure, "out[1]", torch.float32, (4,))
        m = abi.RaycaMeter()
        m.width, m.height, m.low_permille, m.high_permille = w, h, low_permille, high_permille
        m.key, m.min_scale, m.max_scale, m.rate = key, min_scale, max_scale, rate
        m.color, m.hist_out, m.exposure_out = call.input(color, "color", torch.float32, (h, w, 4)).data_ptr(), hist.data_ptr(), exposure.data_ptr()
        if prev is not None:   # (not copied: it may be the record this call writes)
            m.exposure_prev = call.output(prev, "prev", torch.float32, (4,)).data_ptr()
        stats = call.run(self._lib.rayca_hip_meter_device, m, context=context, want_stats=want_stats)
        return (hist, exposure) + ((stats,) if stats is not None else ())

    def tonemap(self, color, op="aces", *, exposure=None, scale=1.0, white=0.0, gamma=1.0, rgba8=False, out=None, stream=None, context=0,
                want_stats=False):
        """rayca_hip_tonemap_device: exposure, a display operator and the output stage, asynchronously, everything in device
        memory.

        color (H, W, 4) float32, gamma 1.  op: "linear" (the scale alone), "reinhard" (extended Reinhard on the luminance;
        `white` > 0 is the luminance that maps to 1, 0 none) or "aces" (the rational fit, per channel), or its abi.TONEMAP_
        value.  The scale is word 0 of `exposure`, a (4,) float32 tensor as meter() returns it -- read on the device, nothing
        waited for -- or else the float `scale`.  `gamma`, `out` (may be `color` itself), `rgba8`, the stream handling and the
        return convention are denoise()'s; out=False with rgba8 writes and returns the uint8 picture alone."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        if isinstance(op, str):
            if op not in abi.TONEMAP_NAMES:
                raise ValueError(f"op: one of {abi.TONEMAP_NAMES}, not {op!r}")
            op = abi.TONEMAP_NAMES.index(op)
        t = abi.RaycaTonemap()
        t.width, t.height, t.op, t.scale, t.white, t.gamma = w, h, op, scale, white, gamma
        out = call.output(out, "out", torch.float32, (h, w, 4)) if out is not False else None
        out8 = call.output(rgba8, "rgba8", torch.uint8, (h, w, 4), optional=True)
        t.color = call.input(color, "color", torch.float32, (h, w, 4)).data_ptr()
        if exposure is not None:   # (not copied: read where meter() wrote it)
            t.exposure = call.output(exposure, "exposure", torch.float32, (4,)).data_ptr()
        t.rgba32f_out, t.rgba8_out = _ptr(out), _ptr(out8)
        stats = call.run(self._lib.rayca_hip_tonemap_device, t, context=context, want_stats=want_stats)
        return _asked_for(out, out8, stats)

    # ---- temporal accumulation: a frame into a history, with reprojection (rayca_hip_scene_camera, rayca_hip_accumulate_device) ----
    def camera_pose(self) -> abi.RaycaCameraPose:
        """rayca_hip_scene_camera: the camera the scene's frames use, as accumulate() takes it for `prev_camera` (origin, tan of
        half the vertical field of view, and the rows right / up / back of the inverse of the camera's rotation and scale).
        Host only; after update() the new camera."""
        pose = abi.RaycaCameraPose()
        lib.check(self._lib.rayca_hip_scene_camera(self.handle, C.byref(pose)))
        return pose

    def accumulate(self, color, *, history=None, prev=None, prev_camera=None, point=None, normal=None, id=None, max_history=0,
                   normal_min=0.9, plane_max=0.1, moments=None, variance=False, out=None, stream=None, context=0, want_stats=False):
        """rayca_hip_accumulate_device: one frame into a history, asynchronously, everything in device memory.

        color (H, W, 4) float32: a frame rendered with gamma 1.  history: None (the first frame) or a dict as this call
        returns one -- "color" (H, W, 4), "length" (H, W) float32, optionally "moments" (H, W, 2).  Without `prev_camera` the
        history is taken pixel by pixel (the camera did not move).  With it (a camera_pose() of the frame the history belongs
        to) every pixel looks its history up where its surface point was seen then: point and normal (H, W, 3) float32 and
        optionally id (H, W) int32 are this frame's G-buffer as gbuffer() returns it (of a one-sample config: points on the rays
        through pixel centres), `prev` a dict with the other frame's "normal" and optionally "point" and "id" (id with id or not
        at all).  A tap of the bilinear footprint counts only where the ids are equal, the normals' dot product is at least
        normal_min and, with prev["point"], the tap lies within plane_max world units of this pixel's tangent plane.
        max_history 0 is a running mean, else the length is capped there.  moments (default: whenever the history allows it)
        adds "moments" (mean and mean square of the luminance), variance=True "variance" (H, W).  `out`: a dict of tensors to
        write instead of new ones; without prev_camera they may be the history's own (a film in place), and out["color"] may
        always be `color`.  Stream handling as query().  Returns a dict: color, length, [moments], [variance], [stats]."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        history, prev, out = dict(history or {}), dict(prev or {}), dict(out or {})
        for name, d, known in (("history", history, ("color", "length", "moments")), ("prev", prev, ("normal", "point", "id")),
                               ("out", out, ("color", "length", "moments", "variance"))):
            stray = [k for k in d if k not in known]
            if stray:
                raise ValueError(f"{name}: {stray} not in {known}")
        if moments is None:
            moments = variance or not history or "moments" in history
        if variance and not moments:
            raise ValueError("variance: needs moments")
        shapes = {"color": (torch.float32, (h, w, 4)), "length": (torch.float32, (h, w)), "moments": (torch.float32, (h, w, 2)),
                  "variance": (torch.float32, (h, w)), "point": (torch.float32, (h, w, 3)), "normal": (torch.float32, (h, w, 3)),
                  "id": (torch.int32, (h, w))}
        a = abi.RaycaAccumulate()
        a.width, a.height, a.max_history, a.normal_min, a.plane_max = w, h, max_history, normal_min, plane_max
        result = {}
        for name in ("color", "length") + (("moments",) if moments else ()) + (("variance",) if variance else ()):
            result[name] = call.output(out.get(name), f"out[{name!r}]", *shapes[name])
            setattr(a, name + "_out", result[name].data_ptr())
        a.color = call.input(color, "color", *shapes["color"]).data_ptr()
        for name, x in (("point", point), ("normal", normal), ("id", id)):
            if x is not None:
                setattr(a, name, call.input(x, name, *shapes[name]).data_ptr())
        for name, x in history.items():
            setattr(a, "hist_" + name, call.input(x, f"history[{name!r}]", *shapes[name]).data_ptr())
        for name, x in prev.items():
            setattr(a, "prev_" + name, call.input(x, f"prev[{name!r}]", *shapes[name]).data_ptr())
        if prev_camera is not None:
            if not isinstance(prev_camera, abi.RaycaCameraPose):
                raise TypeError(f"prev_camera: a camera_pose() is expected, not {type(prev_camera).__name__}")
            a.prev_camera = C.pointer(prev_camera)
        stats = call.run(self._lib.rayca_hip_accumulate_device, a, context=context, want_stats=want_stats)
        if stats is not None:
            result["stats"] = stats
        return result

    # ---- adaptive sampling: a film's variance decides where the next rays go (rayca_hip_sample_plan_device, rayca_hip_film_fold_device) ----
    def sample_plan(self, color, variance, length, budget, *, jitter=1, first_stratum=0, target=0.05, lum_floor=1e-3, base_weight=0,
                    fresh_weight=255, min_history=4, want=("offset", "rays", "pixel"), out=None, stream=None, context=0, want_stats=False):
        """rayca_hip_sample_plan_device: where the next `budget` rays of a film go, asynchronously, everything in device memory.

        color (H, W, 4), variance (H, W), length (H, W) float32: a film's colour, luminance variance and history length
        (accumulate(), Film).  Every pixel gets an integer weight 0..255: base_weight plus one step for every `target`^2 of the
        relative variance of its mean (variance / length over the squared luminance, the luminance at least lum_floor), and at
        least fresh_weight where the history is shorter than min_history.  The budget is dealt out in proportion to the
        weights, exactly: pixel p gets offset[p + 1] - offset[p] rays, which sum to `budget`.  Returns a dict of the outputs in
        `want`: "weight" (H, W) int32, "offset" (H * W + 1,) int32, "rays" (budget, 6) float32 -- ray j of pixel p goes through
        stratum (first_stratum + j - offset[p]) mod jitter^2 of the jitter x jitter sub-pixel positions, and is the row p of
        camera_rays() for that sample of a jitter^2-spp frame -- and "pixel" (budget,) int32, the pixel of every ray; "offset"
        is always made.  `out`: a dict of tensors to write instead of new ones.  The budget is the host's, so radiance() takes
        the rays without a readback.  Stream handling as query(); with `want_stats` (which waits) the stats dict is "stats"."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        h, w = call.image(color)
        known = ("weight", "offset", "rays", "pixel")
        out = dict(out or {})
        stray = [k for k in tuple(want) + tuple(out) if k not in known]
        if stray:
            raise ValueError(f"want / out: {stray} not in {known}")
        if not isinstance(budget, int) or isinstance(budget, bool) or not 0 <= budget <= 1 << 31:
            raise ValueError(f"budget: an integer 0..2**31, not {budget!r}")
        shapes = {"weight": (torch.int32, (h, w)), "offset": (torch.int32, (h * w + 1,)), "rays": (torch.float32, (budget, 6)),
                  "pixel": (torch.int32, (budget,))}
        a = abi.RaycaSamplePlan()
        a.width, a.height, a.budget, a.jitter, a.first_stratum = w, h, budget, jitter, first_stratum
        a.base_weight, a.fresh_weight, a.min_history, a.target, a.lum_floor = base_weight, fresh_weight, min_history, target, lum_floor
        result = {}
        for name in known:
            if name == "offset" or name in want or name in out:
                result[name] = call.output(out.get(name), f"out[{name!r}]", *shapes[name])
                setattr(a, name + "_out", result[name].data_ptr() or None)   # (an empty tensor has no pointer: budget 0 makes no rays)
        a.color = call.input(color, "color", torch.float32, (h, w, 4)).data_ptr()
        a.variance = call.input(variance, "variance", torch.float32, (h, w)).data_ptr()
        a.length = call.input(length, "length", torch.float32, (h, w)).data_ptr()
        stats = call.run(self._lib.rayca_hip_sample_plan_device, a, context=context, want_stats=want_stats)
        if stats is not None:
            result["stats"] = stats
        return result

    def fold(self, samples, offset, history, *, max_history=0, moments=True, variance=True, out=None, stream=None, context=0, want_stats=False):
        """rayca_hip_film_fold_device: the samples of a plan's rays into a history, asynchronously, everything in device memory.

        samples (B, 4) float32: what radiance() returned for sample_plan()'s rays, with gamma 1; offset (H * W + 1,) int32: that
        plan's offsets; history: a dict as accumulate() returns one -- "color" (H, W, 4), "length" (H, W) and, for moments,
        "moments" (H, W, 2).  Pixel p's samples offset[p] .. offset[p + 1] - 1 enter its history one after the other, each as
        accumulate() without prev_camera would blend a frame that held it; a pixel without samples keeps its history.
        max_history, moments, variance and `out` as accumulate(): the outputs may be the history's own tensors.  Stream handling
        as query().  Returns a dict: color, length, [moments], [variance], [stats]."""
        call = _DeviceCall(self, stream)
        torch = call.torch
        history, out = dict(history or {}), dict(out or {})
        for name, d, known in (("history", history, ("color", "length", "moments")), ("out", out, ("color", "length", "moments", "variance"))):
            stray = [k for k in d if k not in known]
            if stray:
                raise ValueError(f"{name}: {stray} not in {known}")
        if "color" not in history or "length" not in history:
            raise ValueError("history: color and length are required (a fold continues a history; accumulate() starts one)")
        h, w = call.image(history["color"], "history['color']")
        if variance and not moments:
            raise ValueError("variance: needs moments")
        if moments and "moments" not in history:
            raise ValueError("moments: the history has none")
        if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[1] != 4:
            raise ValueError("samples: a (B, 4) float32 tensor is expected")
        shapes = {"color": (torch.float32, (h, w, 4)), "length": (torch.float32, (h, w)), "moments": (torch.float32, (h, w, 2)),
                  "variance": (torch.float32, (h, w))}
        a = abi.RaycaFilmFold()
        a.width, a.height, a.max_history = w, h, max_history
        result = {}
        for name in ("color", "length") + (("moments",) if moments else ()) + (("variance",) if variance else ()):
            result[name] = call.output(out.get(name), f"out[{name!r}]", *shapes[name])
            setattr(a, name + "_out", result[name].data_ptr())
        # (an empty sample list has no pointer; no offset then leads into it, and the call still wants one that is not NULL)
        a.samples = call.input(samples, "samples", torch.float32, (samples.shape[0], 4)).data_ptr() or result["color"].data_ptr()
        a.offset = call.input(offset, "offset", torch.int32, (h * w + 1,)).data_ptr()
        for name, x in history.items():
            if name != "moments" or moments:
                setattr(a, "hist_" + name, call.input(x, f"history[{name!r}]", *shapes[name]).data_ptr())
        stats = call.run(self._lib.rayca_hip_film_fold_device, a, context=context, want_stats=want_stats)
        if stats is not None:
            result["stats"] = stats
        return result


class _DeviceCall:
    """One call of a device entry point on torch tensors: the device and stream handling that query(), surface(), camera_rays()
    and the post passes share, and the tensors the call has to keep alive.  `stream`: a torch.cuda.Stream, a raw handle, or
    None for torch's current stream of the scene's device.

    The ordering rule: resolve every output() before the input() that may share its tensor (out=color, a film in place) --
    an input that is not contiguous is replaced by a copy, and the output must still be the caller's tensor."""

    def __init__(self, scene, stream):
        import torch
        self.torch, self.scene = torch, scene
        self.dev = torch.device("cuda", scene.device)
        self.stream = torch.cuda.current_stream(self.dev) if stream is None else stream
        self.handle = self.stream.cuda_stream if hasattr(self.stream, "cuda_stream") else int(self.stream)
        if not self.handle:
            # the legacy default stream: the library runs a call without a stream on the context's own (non-blocking) stream
            # and waits for it, so what torch still has queued for the inputs must have finished first
            torch.cuda.default_stream(self.dev).synchronize()
        self.temporaries = []

    def checked(self, x, name, dtype, shape):
        if not isinstance(x, self.torch.Tensor):
            raise TypeError(f"{name}: a torch tensor on {self.dev} is expected, not {type(x).__name__}")
        if x.device != self.dev:
            raise ValueError(f"{name}: on {x.device}, the scene is on {self.dev}")
        if x.dtype != dtype:
            raise TypeError(f"{name}: dtype {x.dtype}, expected {dtype}")
        if tuple(x.shape) != shape:
            raise ValueError(f"{name}: shape {tuple(x.shape)}, expected {shape}")
        return x

    def image(self, color, name="color"):
        """(H, W) of an (H, W, 4) tensor; input() checks the rest of it"""
        if not isinstance(color, self.torch.Tensor):
            raise TypeError(f"{name}: a torch tensor on {self.dev} is expected, not {type(color).__name__}")
        if color.dim() != 3 or color.shape[2] != 4:
            raise ValueError(f"{name}: shape {tuple(color.shape)}, expected (H, W, 4)")
        return color.shape[0], color.shape[1]

    def input(self, x, name, dtype, shape):
        x = self.checked(x, name, dtype, shape)
        if not x.is_contiguous():
            x = x.contiguous()
            self.temporaries.append(x)
        return x

    def output(self, x, name, dtype, shape, optional=False):
        """The tensor to write: `x` itself (checked, contiguous), or a new one for None / True; with `optional`, None / False
        mean that the output is not asked for."""
        if optional and (x is None or x is False):
            return None
        if x is None or x is True:
            return self.torch.empty(shape, dtype=dtype, device=self.dev)
        if not self.checked(x, name, dtype, shape).is_contiguous():
            raise ValueError(f"{name}: must be contiguous (an output, or an input that is read in place)")
        return x

    def guides(self, args, h, w, **guides):
        """the guides that are given, into the fields of `args` that carry their names"""
        f32, i32 = self.torch.float32, self.torch.int32
        shapes = {"albedo": (f32, (h, w, 4)), "normal": (f32, (h, w, 3)), "point": (f32, (h, w, 3)), "id": (i32, (h, w))}
        for name, x in guides.items():
            if x is not None:
                setattr(args, name, self.input(x, name, *shapes[name]).data_ptr())

    def options(self, context, traversal=0, collect_stats=False, tile=None):
        return self.scene._opts(traversal, collect_stats, tile, self.handle or None, context=context)

    def torch_stream(self):
        """the call's stream as a torch stream object: for torch work that is to run behind the call"""
        return self.stream if hasattr(self.stream, "cuda_stream") else self.torch.cuda.ExternalStream(self.handle, device=self.dev)

    def run(self, fn, args, *, context, want_stats=False, **options):
        """fn(scene, options, args, stats) through lib.check; returns the stats dict (the call has waited) or None"""
        st = abi.RaycaStats() if want_stats else None
        o = self.options(context, **options)
        lib.check(fn(self.scene.handle, C.byref(o), C.byref(args), C.byref(st) if st is not None else None))
        # (a contiguous copy made here is read by a kernel on the stream: the allocator must know)
        for x in self.temporaries:
            x.record_stream(self.stream if hasattr(self.stream, "cuda_stream") else self.torch.cuda.ExternalStream(self.handle, device=self.dev))
        return st.as_dict() if st is not None else None


def _ptr(x):
    return x.data_ptr() if x is not None else None


def _asked_for(*parts):
    """The return convention of the post passes: what was asked for in the order given -- the float tensor, then the optional
    tensors and the stats dict -- as a tuple, or alone where it is the only thing."""
    result = tuple(x for x in parts if x is not None)
    return result[0] if len(result) == 1 else result


def _scale_ok(scale, width=0, height=0):
    if not isinstance(scale, int) or isinstance(scale, bool) or not 1 <= scale <= 8 or width % scale or height % scale:
        raise ValueError(f"scale: an integer 1..8 that divides width and height, not {scale!r} for {width} x {height}")


def _multi_args(scenes, config, band_rows, gather, traversal, collect_stats, engine, context):
    handles = (C.c_void_p * len(scenes))(*[s.handle for s in scenes])
    o = abi.RaycaMultiOptions()
    o.traversal, o.collect_stats, o.band_rows, o.gather, o.engine, o.context = traversal, int(collect_stats), band_rows, gather, engine, context
    return handles, o, config.to_abi()


def render_multi(scenes, config: Config, width: int, height: int, *, band_rows=8, gather=abi.GATHER_RCCL, traversal=abi.TRAVERSAL_ORDERED,
                 collect_stats=False, engine=abi.ENGINE_AUTO, want_stats=False, context=0):
    """rayca_hip_render_multi: one frame on len(scenes) devices of this process, scenes[i] = the DeviceScene that renders
    part i (created on its own device); returns (rgba8 (H, W, 4), [stats per device] | None)."""
    l = scenes[0]._lib
    handles, o, cfg = _multi_args(scenes, config, band_rows, gather, traversal, collect_stats, engine, context)
    u8 = np.zeros((height, width, 4), np.uint8)
    st = (abi.RaycaStats * len(scenes))() if (want_stats or collect_stats) else None
    lib.check(l.rayca_hip_render_multi(handles, len(scenes), C.byref(cfg), width, height, C.byref(o), u8.ctypes.data, st))
    return u8, ([x.as_dict() for x in st] if st is not None else None)


class MultiFrames:
    """Frames in flight through the several-devices entry (rayca_hip_render_multi_issue / _wait): `issue(context, out)`
    queues a whole frame -- every part's kernels, the one exchange, de-interleave, copy into `out` -- on frame context
    `context` of every scene and returns; `wait(context)` blocks until that frame has landed.  A host that walks the
    contexts in turn keeps that many frames in flight on every device (what a C or Rust host of the library does)."""

    def __init__(self, scenes, config: Config, width: int, height: int, *, band_rows=8, gather=abi.GATHER_RCCL,
                 traversal=abi.TRAVERSAL_ORDERED, engine=abi.ENGINE_AUTO):
        self.scenes, self.width, self.height = list(scenes), width, height
        self._l = scenes[0]._lib
        self._args = {}
        self._mk = lambda ctx: _multi_args(self.scenes, config, band_rows, gather, traversal, False, engine, ctx)

    def issue(self, context: int, out, on_device=None) -> None:
        """out: a (H, W, 4) uint8 numpy array (kept alive by the caller until wait), or a pointer (int): device memory of
        scenes[0]'s device unless on_device=False (then host memory, e.g. a page-locked torch tensor's data_ptr)."""
        if context not in self._args:
            self._args[context] = self._mk(context)
        handles, o, cfg = self._args[context]
        if on_device is None:
            on_device = isinstance(out, int)
        o.output_on_device = int(bool(on_device))
        ptr = out if isinstance(out, int) else out.ctypes.data
        lib.check(self._l.rayca_hip_render_multi_issue(handles, len(self.scenes), C.byref(cfg), self.width, self.height, C.byref(o), ptr))

    def wait(self, context: int) -> None:
        handles = self._args[context][0] if context in self._args else (C.c_void_p * len(self.scenes))(*[s.handle for s in self.scenes])
        lib.check(self._l.rayca_hip_render_multi_wait(handles, len(self.scenes), context))


class Renderer:
    """Owns a RaycaRenderer handle: the resident draw().  `draw(desc, ...)` compares `desc` with the descriptor of the previous
    call inside the library and renders the resident scene as it is (abi.DRAW_REUSED), updates its camera, lights and
    materials in place (DRAW_UPDATED) or rebuilds it (DRAW_REBUILT); the frame is the one a new DeviceScene(desc, config,
    builder=...) renders, bit for bit."""

    def __init__(self, device: int = 0, builder: int = abi.BUILDER_SAH, build_on_host: bool = False, _lib=None):
        self._lib = _lib or lib.load()
        opts = abi.RaycaBuildOptions()
        opts.builder, opts.device, opts.build_on_host = builder, device, int(build_on_host)
        h = C.c_void_p()
        lib.check(self._lib.rayca_hip_renderer_create(C.byref(opts), C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.rayca_hip_renderer_destroy(self.handle)
            self.handle = None

    __del__ = close

    def draw(self, desc: abi.SceneDesc, config: Config, width: int, height: int, *, traversal=abi.TRAVERSAL_ORDERED,
             collect_stats=False, tile=None, want_rgba8=True, want_f32=True, engine=abi.ENGINE_AUTO, context=0,
             camera_rays=abi.CAMERA_AUTO):
        """rayca_hip_renderer_draw: host outputs, the render options of DeviceScene.render.  Returns (rgba8 | None,
        rgba32f | None, stats dict, info dict as `last_draw`)."""
        rows = height
        if tile is not None:
            t = abi.RaycaTile()
            t.part, t.parts, t.band_rows = tile
            rows = self._lib.rayca_hip_tile_rows(C.byref(t), height)
        u8 = np.zeros((rows, width, 4), np.uint8) if want_rgba8 else None
        f32 = np.zeros((rows, width, 4), np.float32) if want_f32 else None
        st = abi.RaycaStats()
        cfg = config.to_abi()
        o = DeviceScene._opts(traversal, collect_stats, tile, None, engine, context, camera_rays)
        action = C.c_uint32(abi.NONE)
        lib.check(self._lib.rayca_hip_renderer_draw(self.handle, desc.ptr(), C.byref(cfg), width, height, C.byref(o),
                                                    u8.ctypes.data if u8 is not None else None,
                                                    f32.ctypes.data if f32 is not None else None, C.byref(st), C.byref(action)))
        return u8, f32, st.as_dict(), self.last_draw()

    def last_draw(self) -> dict:
        """rayca_hip_renderer_last_draw: {"action": abi.DRAW_* (None before the first draw), "ms": {compare, update, build,
        render} of that draw (host wall time), "builds" / "updates" / "reuses": totals, "kept_bytes"}."""
        action = C.c_uint32(abi.NONE)
        ms = (C.c_float * abi.DRAW_MS_COUNT)()
        n = (C.c_uint64 * abi.DRAW_N_COUNT)()
        lib.check(self._lib.rayca_hip_renderer_last_draw(self.handle, C.byref(action), ms, n))
        return {"action": None if action.value == abi.NONE else action.value,
                "ms": {"compare": ms[abi.DRAW_MS_COMPARE], "update": ms[abi.DRAW_MS_UPDATE], "build": ms[abi.DRAW_MS_BUILD],
                       "render": ms[abi.DRAW_MS_RENDER]},
                "builds": n[abi.DRAW_N_BUILDS], "updates": n[abi.DRAW_N_UPDATES], "reuses": n[abi.DRAW_N_REUSES],
                "kept_bytes": n[abi.DRAW_N_KEPT_BYTES]}

    @property
    def scene(self) -> Optional[C.c_void_p]:
        """The resident RaycaScene handle (None before the first draw).  The renderer owns it: the next rebuilding draw
        destroys it."""
        h = C.c_void_p()
        lib.check(self._lib.rayca_hip_renderer_scene(self.handle, C.byref(h)))
        return h if h.value else None

    def invalidate(self) -> None:
        """The next draw rebuilds, whatever it is handed."""
        lib.check(self._lib.rayca_hip_renderer_invalidate(self.handle))


class SoftRenderer:
    """Drop-in for rayca_soft::SoftRenderer (scene.rs:11-14): `draw(scene, image)` renders `scene`
    with camera_draw_infos[0] into `image` (RGBA8).  The reference rebuilds the BVH on every draw; this one keeps the
    scene of the last draw resident (a `Renderer`, made at the first draw) and rebuilds only when the scene's geometry,
    textures or graph changed -- `last_draw` says what the call did.  Same pixels either way."""

    def __init__(self, config: Optional[Config] = None, device: int = 0, builder: int = abi.BUILDER_SAH):
        self.config = config or Config()
        self.device = device
        self.builder = builder
        self.last_stats = None
        self.last_draw = None
        self._renderer = None

    @staticmethod
    def new_with_config(config: Config) -> "SoftRenderer":
        return SoftRenderer(config)

    @staticmethod
    def create_default_model():
        return create_default_model()

    def draw(self, scene: Scene, image: Image) -> None:
        if image.color_type != abi.COLOR_RGBA8:
            raise ValueError("draw() writes RGBA8 images (scene.rs:117)")
        if self._renderer is None:
            self._renderer = Renderer(self.device, self.builder)
        u8, _, self.last_stats, self.last_draw = self._renderer.draw(flatten(scene), self.config, image.width, image.height, want_f32=False)
        image.data[...] = u8

    def close(self) -> None:
        if getattr(self, "_renderer", None) is not None:
            self._renderer.close()
            self._renderer = None

    __del__ = close
