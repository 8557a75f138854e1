"""rayca_hip_radiance_device without a GPU: the layout of RaycaRadiance against the header, the symbol, and everything the entry
refuses from its structs alone -- checked through the C ABI in front of any GPU work, with a dummy non-NULL scene handle that
the entry must not look at (as tests/test_tonemap_cpu.py does for the post passes)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from rayca_amd import abi
from rayca_amd.lib import last_error
from rayca_amd.renderer import Config, IntegratorStrategy, SamplerStrategy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["count", "sample", "first_index", "reserved", "rays", "rgba32f_out", "rgba8_out"]


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaRadiance %zu\\n", sizeof(RaycaRadiance));']
    for field in FIELDS:
        lines.append(f'printf("{field} %zu\\n", offsetof(RaycaRadiance, {field}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        want = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert [n for n, _ in abi.RaycaRadiance._fields_] == FIELDS
    assert C.sizeof(abi.RaycaRadiance) == int(want["RaycaRadiance"]) == 4 * 4 + 3 * 8
    for field in FIELDS:
        assert getattr(abi.RaycaRadiance, field).offset == int(want[field]), field
    # the header's field order, read from its text, and the shim's
    header = open(os.path.join(ROOT, "include", "rayca_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"struct RaycaRadiance \{(.*?)\};", header, flags=re.S).group(1), flags=re.S)
    assert [re.search(r"(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()] == FIELDS
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaRadiance \{(.*?)\n\}", shim, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\S+ ?\S*),", rbody) == [("count", "u32"), ("sample", "u32"), ("first_index", "u32"), ("reserved", "u32"),
                                                          ("rays", "*const c_void"), ("rgba32f_out", "*mut c_void"), ("rgba8_out", "*mut c_void")]
    assert re.search(r"pub fn rayca_hip_radiance_device\(scene: \*mut RaycaScene, cfg: \*const RaycaConfig, opts: \*const RaycaRenderOptions, "
                     r"radiance: \*const RaycaRadiance, stats_out: \*mut RaycaStats\) -> i32;", shim)


def test_the_symbol_is_a_product_symbol(product_lib):
    assert "rayca_hip_radiance_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_radiance_device.restype is C.c_int32
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # (no layout changed: the version stays)


@pytest.fixture(scope="module")
def call(product_lib):
    """call(options fields, cfg=dict of Config fields or raw RaycaConfig fields, **changes of RaycaRadiance): the arguments pass
    every check unless changed.  ptr(i) stand for device pointers (nothing is launched): distinct 16-byte aligned addresses."""
    dummy = C.create_string_buffer(1024)
    scene, base = C.cast(dummy, C.c_void_p), (C.addressof(dummy) + 15) // 16 * 16

    def ptr(i):
        return base + 16 * i

    def radiance(o_fields=None, cfg=None, stats=None, **fields):
        o = abi.RaycaRenderOptions()
        for name, v in (o_fields or {}).items():
            target, _, leaf = name.rpartition(".")
            setattr(getattr(o, target) if target else o, leaf, v)
        c = Config().to_abi()
        for k, v in (cfg or {}).items():
            setattr(c, k, v)
        r = abi.RaycaRadiance()
        r.count, r.sample, r.first_index, r.rays, r.rgba32f_out, r.rgba8_out = 100, 0, 0, ptr(0), ptr(8), ptr(40)
        for k, v in fields.items():
            setattr(r, k, v)
        return product_lib.rayca_hip_radiance_device(scene, C.byref(c), C.byref(o), C.byref(r), C.byref(stats) if stats is not None else None)

    radiance.ptr, radiance.scene, radiance.keep = ptr, scene, dummy
    return radiance


def test_null_arguments(product_lib, call):
    fn, o, c, r = product_lib.rayca_hip_radiance_device, abi.RaycaRenderOptions(), Config().to_abi(), abi.RaycaRadiance()
    assert fn(None, C.byref(c), C.byref(o), C.byref(r), None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert fn(call.scene, None, C.byref(o), C.byref(r), None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert fn(call.scene, C.byref(c), C.byref(o), None, None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert call(rays=None) == abi.ERR_BAD_ARG and "rays" in last_error()


def test_every_struct_level_refusal_names_its_field(call):
    ptr = call.ptr
    cases = [(dict(first_index=0xFFFFFFFF, count=2), "first_index"), (dict(first_index=1 << 31, count=(1 << 31) + 1), "first_index"),
             (dict(reserved=1), "reserved"), (dict(rgba32f_out=None, rgba8_out=None), "no output"),
             (dict(rgba32f_out=ptr(8) + 4), "rgba32f_out"), (dict(rgba32f_out=ptr(8) + 8), "rgba32f_out"), (dict(rgba32f_out=ptr(8) + 1, rgba8_out=None), "rgba32f_out"),
             (dict(cfg=dict(integrator=6)), "integrator"), (dict(cfg=dict(integrator=0xFFFFFFFF)), "integrator"),
             (dict(cfg=dict(direct_sampler=6)), "direct_sampler"), (dict(cfg=dict(indirect_sampler=6)), "indirect_sampler"),
             (dict(cfg=dict(light_samples=0)), "light_samples")]
    for fields, word in cases:
        assert call(**fields) == abi.ERR_BAD_ARG, fields
        assert word in last_error(), (fields, last_error())
    # the options: what does not apply to the call, and the context
    for field in ("tile.part", "tile.parts", "tile.band_rows", "tile.reserved", "engine", "camera_rays", "reserved"):
        assert call({field: 1}) == abi.ERR_BAD_ARG, field
        assert "must be zero" in last_error() and field.partition(".")[0] in last_error(), (field, last_error())
    assert call(dict(traversal=2)) == abi.ERR_BAD_ARG and "traversal" in last_error()
    assert call(dict(context=8)) == abi.ERR_BAD_ARG and "context out of range" in last_error()


def test_the_options_are_checked_last_among_the_struct_checks(call):
    """A call that is refused for context 8 -- and for nothing else -- has passed every check of the two structs: the ends of the
    ranges, each output alone, every Config the entry offers.  And a struct-level fault wins over a bad context."""
    ptr, last = call.ptr, dict(context=8)
    valid = [dict(), dict(rgba8_out=None), dict(rgba32f_out=None), dict(rgba8_out=ptr(40) + 1), dict(first_index=0xFFFFFFFF, count=1),
             dict(first_index=(1 << 32) - 100), dict(first_index=1 << 31, count=1 << 31), dict(sample=0xFFFFFFFF), dict(count=0), dict(count=1),
             dict(cfg=dict(integrator=IntegratorStrategy.Flat)), dict(cfg=dict(max_depth=0)), dict(cfg=dict(samples_per_pixel=0)),
             dict(cfg=dict(bvh=0)), dict(cfg=dict(direct_sampler=SamplerStrategy.NONE, indirect_sampler=SamplerStrategy.Hemisphere)),
             dict(cfg=dict(max_depth=1, light_samples=4, light_stratify=1)), dict(cfg=dict(gamma=2.2, seed=0xFFFFFFFF))]
    for fields in valid:
        assert call(last, **fields) == abi.ERR_BAD_ARG and "context out of range" in last_error(), (fields, last_error())
    assert call(dict(context=8, stream=1, wait_event=1, record_event=1, collect_stats=1)) == abi.ERR_BAD_ARG and "context out of range" in last_error()
    for fields, word in ((dict(reserved=1), "reserved"), (dict(rgba32f_out=ptr(8) + 4), "rgba32f_out"), (dict(cfg=dict(light_samples=0)), "light_samples"),
                         (dict(cfg=dict(integrator=9)), "integrator")):
        assert call(last, **fields) == abi.ERR_BAD_ARG and word in last_error() and "context" not in last_error(), (fields, last_error())


def test_an_empty_batch_is_ok_and_touches_nothing(call):
    assert call(count=0) == abi.OK
    assert call(count=0, first_index=0xFFFFFFFF, cfg=dict(integrator=IntegratorStrategy.Flat)) == abi.OK
    st = abi.RaycaStats()
    st.rays_primary, st.kernel_launches = 7, 7
    assert call(count=0, stats=st) == abi.OK and st.rays_primary == 0 and st.kernel_launches == 0
    assert bytes(call.keep) == bytes(1024)   # the dummy handle's bytes: not written


def test_configs_off_the_generation_kernels_are_unsupported_without_a_scene(call):
    """(They need no scene to be judged, so they are judged in front of it -- behind the BAD_ARG checks -- and name their field.)"""
    cases = [(dict(integrator=IntegratorStrategy.Raytracer), "integrator"), (dict(russian_roulette=1), "russian_roulette"),
             (dict(direct_sampler=SamplerStrategy.Mis), "direct_sampler"), (dict(max_depth=3, light_samples=2), "light_samples"),
             (dict(indirect_sampler=SamplerStrategy.Brdf), "indirect_sampler")]
    for cfg, word in cases:
        assert call(cfg=cfg) == abi.ERR_UNSUPPORTED, cfg
        assert "RaycaConfig." + word in last_error(), (cfg, last_error())
    assert call(dict(traversal=abi.TRAVERSAL_EXHAUSTIVE)) == abi.ERR_UNSUPPORTED and "traversal" in last_error()
