"""What the post passes check alike (post.inc: frame_tiles, check_alignment, pass_options last), through the C ABI in front of
any GPU work: one table over the entry points, one good call each, and the same eight refusals asked of every one.  Any
non-NULL value will do for the scene handle, as in tests/test_upsample_cpu.py: no check reads through it."""
import ctypes as C

import pytest

from rayca_amd import abi
from rayca_amd.lib import last_error

_BUFFER = C.create_string_buffer(1024)
_BASE = (C.addressof(_BUFFER) + 15) // 16 * 16


def ptr(i):
    """distinct 16-byte aligned addresses that stand for device pointers (nothing is launched)"""
    return _BASE + 16 * i


# entry point -> (argument struct, the fields of a call that passes every check, a pointer read 16 bytes at a time, one read 4 bytes
# at a time -- given or not in the good call)
ENTRIES = {
    "rayca_hip_denoise_device": (abi.RaycaDenoise, dict(iterations=1, normal_power_log2=7, sigma_color=4.0, gamma=1.0, color=ptr(0), rgba32f_out=ptr(1)),
                                 "color", "rgba8_out"),
    "rayca_hip_accumulate_device": (abi.RaycaAccumulate, dict(color=ptr(0), color_out=ptr(1), length_out=ptr(2)), "color_out", "length_out"),
    "rayca_hip_denoise_variance_device": (abi.RaycaDenoiseVariance, dict(iterations=1, normal_power_log2=7, sigma_luminance=4.0, variance_floor=1e-10,
                                                                         gamma=1.0, color=ptr(0), variance=ptr(2), rgba32f_out=ptr(1)),
                                          "rgba32f_out", "variance"),
    "rayca_hip_upsample_device": (abi.RaycaUpsample, dict(scale=2, normal_power_log2=7, gamma=1.0, color=ptr(0), rgba32f_out=ptr(1)), "color", "weight_out"),
    "rayca_hip_meter_device": (abi.RaycaMeter, dict(low_permille=10, high_permille=990, key=0.18, min_scale=2.0 ** -10, max_scale=2.0 ** 10, rate=1.0,
                                                    color=ptr(0), hist_out=ptr(1), exposure_out=ptr(2)), "exposure_out", "hist_out"),
    "rayca_hip_tonemap_device": (abi.RaycaTonemap, dict(op=abi.TONEMAP_NAMES.index("aces"), scale=1.0, gamma=1.0, color=ptr(0), rgba32f_out=ptr(1)),
                                 "color", "rgba8_out"),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_post_pass_checks_its_frame_pointers_and_options_alike(product_lib, entry):
    struct, good, by16, by4 = ENTRIES[entry]
    scene = C.cast(_BUFFER, C.c_void_p)

    def call(context=0, **fields):
        a = struct()
        a.width, a.height = 16, 8
        for k, v in {**good, **fields}.items():
            setattr(a, k, v)
        o = abi.RaycaRenderOptions()
        o.context = context
        return getattr(product_lib, entry)(scene, C.byref(o), C.byref(a), None)

    # the frame's size: empty, more than 2^32 - 1 pixels
    assert call(width=0) == abi.ERR_BAD_ARG, last_error()
    assert call(height=0) == abi.ERR_BAD_ARG, last_error()
    assert call(width=1 << 16, height=1 << 16) == abi.ERR_BAD_ARG, last_error()
    # 2^24 tiles of 64 x 4 pixels: one launch cannot cover the frame -- whatever the options hold, which come last
    assert call(width=2, height=1 << 26) == abi.ERR_UNSUPPORTED and "tiles" in last_error(), last_error()
    assert call(context=8, width=2, height=1 << 26) == abi.ERR_UNSUPPORTED and "tiles" in last_error(), last_error()
    # a call that is refused for its context alone has passed every check of its own
    assert call(context=8) == abi.ERR_BAD_ARG and "context out of range" in last_error(), last_error()
    # alignment: 16 bytes where a pixel is read and written at once, 4 bytes an element elsewhere
    assert call(**{by16: ptr(4) + 4}) == abi.ERR_BAD_ARG and "alignment" in last_error(), last_error()
    assert call(**{by4: ptr(5) + 2}) == abi.ERR_BAD_ARG and "alignment" in last_error(), last_error()
