"""rayca_hip_surface_device and rayca_hip_camera_rays_device without a GPU: the symbols, the layout of RaycaSurfaceQuery in
all three descriptions of the ABI (the header, the ctypes mirror, the Rust shim), and the argument errors that need no scene."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rayca_hip_surface_device", "rayca_hip_camera_rays_device")


def test_library_exports_both_entries(product_lib):
    for name in ENTRIES:
        assert name in abi.PRODUCT_SYMBOLS
        assert getattr(product_lib, name) is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # (no layout changed: the version stays)


def test_surface_struct_layout_matches_header():
    """The rule of test_abi.py: a C program prints sizeof / offsetof from the header, ctypes must agree."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaSurfaceQuery %zu\\n", sizeof(RaycaSurfaceQuery));']
    for name, _ in abi.RaycaSurfaceQuery._fields_:
        lines.append(f'printf("RaycaSurfaceQuery.{name} %zu\\n", offsetof(RaycaSurfaceQuery, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaSurfaceQuery) == int(want["RaycaSurfaceQuery"]) == 8 + 12 * 8
    for name, _ in abi.RaycaSurfaceQuery._fields_:
        assert getattr(abi.RaycaSurfaceQuery, name).offset == int(want[f"RaycaSurfaceQuery.{name}"]), name
    assert [n for n, _ in abi.RaycaSurfaceQuery._fields_] == ["count", "reserved", "rays", "t", "prim", "uv", "point_out", "normal_out", "color_out",
                                                             "diffuse_out", "specular_out", "rough_out", "material_out", "flags_out"]


def test_shim_struct_lists_the_headers_fields_and_both_signatures():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaSurfaceQuery \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)$", decl).groups()
            assert ptr or ctype == "uint32_t", decl
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else "u32"))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaSurfaceQuery \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaSurfaceQuery._fields_] == [n for n, _ in c_fields]
    assert re.search(r"pub fn rayca_hip_surface_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, query: \*const RaycaSurfaceQuery, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)
    assert re.search(r"pub fn rayca_hip_camera_rays_device\(scene: \*mut RaycaScene, cfg: \*const RaycaConfig, width: u32, height: u32, sample: u32, "
                     r"opts: \*const RaycaRenderOptions, d_rays_out: \*mut c_void\) -> i32;", shim)
    for name in ENTRIES:   # and the header declares them
        assert re.search(r"int32_t " + name + r"\(", header)


def test_surface_argument_errors_that_need_no_scene(product_lib):
    """Every one of these is decided before the scene handle is looked at: any non-NULL value will do for it."""
    f = product_lib.rayca_hip_surface_device
    dummy = C.create_string_buffer(64)
    scene = C.cast(dummy, C.c_void_p)
    ptr = C.addressof(dummy)   # (stands for a device pointer: nothing is launched)

    def query(**kw):
        q = abi.RaycaSurfaceQuery()
        q.count, q.t, q.prim, q.uv, q.color_out = 4, ptr, ptr, ptr, ptr
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def opts(**kw):
        o = abi.RaycaRenderOptions()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert f(None, None, C.byref(query()), None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert f(scene, None, None, None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert f(scene, None, C.byref(query(reserved=1)), None) == abi.ERR_BAD_ARG and "reserved" in last_error()
    for name in ("t", "prim", "uv"):
        assert f(scene, None, C.byref(query(**{name: None})), None) == abi.ERR_BAD_ARG and "null hit records" in last_error(), name
    assert f(scene, None, C.byref(query(color_out=None)), None) == abi.ERR_BAD_ARG and "no output" in last_error()
    for name in ("point_out", "normal_out"):
        assert f(scene, None, C.byref(query(**{name: ptr})), None) == abi.ERR_BAD_ARG and "rays" in last_error(), name
    assert f(scene, C.byref(opts(context=8)), C.byref(query()), None) == abi.ERR_BAD_ARG and "context" in last_error()
    for name in ("traversal", "collect_stats", "engine", "camera_rays", "reserved"):
        assert f(scene, C.byref(opts(**{name: 1})), C.byref(query()), None) == abi.ERR_BAD_ARG and "must be zero" in last_error(), name
    o = opts()
    o.tile.parts = 2
    assert f(scene, C.byref(o), C.byref(query()), None) == abi.ERR_BAD_ARG and "tile" in last_error()


def test_camera_rays_argument_errors_that_need_no_scene(product_lib):
    f = product_lib.rayca_hip_camera_rays_device
    dummy = C.create_string_buffer(64)
    scene = C.cast(dummy, C.c_void_p)
    ptr = C.addressof(dummy)
    cfg = abi.RaycaConfig()
    product_lib.rayca_hip_config_default(C.byref(cfg))
    cfg.samples_per_pixel = 4
    assert f(None, C.byref(cfg), 8, 8, 0, None, ptr) == abi.ERR_BAD_ARG and "null" in last_error()
    assert f(scene, None, 8, 8, 0, None, ptr) == abi.ERR_BAD_ARG and "null" in last_error()
    assert f(scene, C.byref(cfg), 0, 8, 0, None, ptr) == abi.ERR_BAD_ARG and "empty image" in last_error()
    assert f(scene, C.byref(cfg), 8, 0, 0, None, ptr) == abi.ERR_BAD_ARG and "empty image" in last_error()
    assert f(scene, C.byref(cfg), 8, 8, 4, None, ptr) == abi.ERR_BAD_ARG and "samples_per_pixel" in last_error()
    o = abi.RaycaRenderOptions()
    o.context = 8
    assert f(scene, C.byref(cfg), 8, 8, 0, C.byref(o), ptr) == abi.ERR_BAD_ARG and "context" in last_error()
    for name in ("traversal", "collect_stats", "engine", "camera_rays"):
        o = abi.RaycaRenderOptions()
        setattr(o, name, 1)
        assert f(scene, C.byref(cfg), 8, 8, 0, C.byref(o), ptr) == abi.ERR_BAD_ARG and "must be zero" in last_error(), name
