"""What the four device passes other than a frame take of RaycaRenderOptions, without a GPU: stream, context and the two events
always; beyond them a query takes traversal and collect_stats, the camera-ray export the tile, a surface call and the denoiser
nothing.  Every other field is refused while it is not zero, and so is a context above 7 -- all of it before the scene handle is
looked at (any non-NULL value will do for it) and before any HIP call."""
import ctypes as C

import pytest

from rayca_amd import abi
from rayca_amd.lib import last_error

GROUPS = {"traversal": ("traversal",), "collect_stats": ("collect_stats",),
          "tile": ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved"),
          "engine": ("engine",), "camera_rays": ("camera_rays",), "reserved": ("reserved",)}
ACCEPTS = {"query": ("traversal", "collect_stats"), "camera_rays": ("tile",), "surface": (), "denoise": ()}


def options(**kw):
    o = abi.RaycaRenderOptions()
    for name, v in kw.items():
        target, _, leaf = name.rpartition(".")
        setattr(getattr(o, target) if target else o, leaf, v)
    return o


@pytest.fixture(scope="module")
def calls(product_lib):
    """entry -> call(options, **changes of its own arguments), each with arguments that pass every check in front of the options'"""
    dummy = C.create_string_buffer(64)
    scene, ptr = C.cast(dummy, C.c_void_p), C.addressof(dummy)   # (ptr stands for a device pointer: nothing is launched)
    cfg = abi.RaycaConfig()
    product_lib.rayca_hip_config_default(C.byref(cfg))

    def query(o, kind=abi.QUERY_CLOSEST):
        q = abi.RaycaQuery()
        q.kind, q.count, q.rays, q.t_out, q.occluded_out, q.tmax_all = kind, 4, ptr, ptr, ptr, float("inf")
        return product_lib.rayca_hip_query_device(scene, C.byref(o), C.byref(q), None)

    def surface(o):
        q = abi.RaycaSurfaceQuery()
        q.count, q.t, q.prim, q.uv, q.color_out = 4, ptr, ptr, ptr, ptr
        return product_lib.rayca_hip_surface_device(scene, C.byref(o), C.byref(q), None)

    def camera_rays(o):
        return product_lib.rayca_hip_camera_rays_device(scene, C.byref(cfg), 8, 8, 0, C.byref(o), ptr)

    def denoise(o):
        d = abi.RaycaDenoise()
        d.width, d.height, d.iterations, d.normal_power_log2, d.sigma_color, d.gamma = 8, 8, 2, 7, 4.0, 1.0
        d.color, d.rgba32f_out = ptr, ptr
        return product_lib.rayca_hip_denoise_device(scene, C.byref(o), C.byref(d), None)

    return {"query": query, "surface": surface, "camera_rays": camera_rays, "denoise": denoise, "_keep": (dummy, cfg)}


@pytest.mark.parametrize("entry", ["query", "surface", "camera_rays", "denoise"])
def test_a_field_the_pass_does_not_take_must_be_zero(calls, entry):
    call = calls[entry]
    refused = [f for group, fields in GROUPS.items() if group not in ACCEPTS[entry] for f in fields]
    assert len(refused) == 9 - sum(len(GROUPS[g]) for g in ACCEPTS[entry])
    for field in refused:
        for value in (1, 0xFFFFFFFF):
            assert call(options(**{field: value})) == abi.ERR_BAD_ARG, (field, value)
            assert "must be zero" in last_error() and field.partition(".")[0] in last_error(), (field, value, last_error())
    assert call(options(context=8)) == abi.ERR_BAD_ARG and "context" in last_error()
    assert call(options(context=0xFFFFFFFF)) == abi.ERR_BAD_ARG and "context" in last_error()
    # the fields every pass takes do not shield one that it does not
    assert call(options(context=7, stream=1, wait_event=1, record_event=1, engine=1)) == abi.ERR_BAD_ARG and "must be zero" in last_error()


def test_a_query_takes_traversal_and_collect_stats(calls):
    """An exhaustive occlusion query is refused as unsupported, behind the options' check and in front of the scene: the check let
    traversal and collect_stats through.  (The camera-ray export's tile leads into the scene: tests/test_gpu_surface.py.)"""
    query = calls["query"]
    for stats in (0, 1):
        o = options(traversal=abi.TRAVERSAL_EXHAUSTIVE, collect_stats=stats)
        assert query(o, kind=abi.QUERY_OCCLUDED) == abi.ERR_UNSUPPORTED, stats
    assert query(options(traversal=abi.TRAVERSAL_EXHAUSTIVE + 1)) == abi.ERR_BAD_ARG and "unknown traversal" in last_error()
