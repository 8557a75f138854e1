"""rayca_hip_query_device without a GPU: the symbol, the layout of RaycaQuery in all three descriptions of the ABI (the header,
the ctypes mirror, the Rust shim), and the argument errors that need no scene."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_query_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_query_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2


def test_query_struct_layout_matches_header():
    """The rule of test_abi.py: a C program prints sizeof / offsetof from the header, ctypes must agree."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaQuery %zu\\n", sizeof(RaycaQuery));',
             'printf("kinds %d\\n", RAYCA_QUERY_CLOSEST * 10 + RAYCA_QUERY_OCCLUDED);']
    for name, _ in abi.RaycaQuery._fields_:
        lines.append(f'printf("RaycaQuery.{name} %zu\\n", offsetof(RaycaQuery, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert C.sizeof(abi.RaycaQuery) == int(want["RaycaQuery"]) == 64
    for name, _ in abi.RaycaQuery._fields_:
        assert getattr(abi.RaycaQuery, name).offset == int(want[f"RaycaQuery.{name}"]), name
    assert int(want["kinds"]) == abi.QUERY_CLOSEST * 10 + abi.QUERY_OCCLUDED == 1


def test_shim_struct_lists_the_headers_fields():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayca_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "rayca_shim.rs")).read()
    body = re.search(r"struct RaycaQuery \{(.*?)\};", header, flags=re.S).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            const, ctype, ptr, name = re.match(r"(const )?(\w+)\s*(\*)?\s*(\w+)$", decl).groups()
            scalar = {"uint32_t": "u32", "float": "f32"}.get(ctype)
            c_fields.append((name, f"*{'const' if const else 'mut'} c_void" if ptr else scalar))
    rbody = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RaycaQuery \{(.*?)\n\}", shim, flags=re.S).group(1)
    r_fields = [tuple(x.strip() for x in re.match(r"\s*pub (\w+): (.+),$", l).groups()) for l in rbody.splitlines() if l.strip()]
    assert r_fields == c_fields
    assert [n for n, _ in abi.RaycaQuery._fields_] == [n for n, _ in c_fields]
    assert re.search(r"pub fn rayca_hip_query_device\(scene: \*mut RaycaScene, opts: \*const RaycaRenderOptions, query: \*const RaycaQuery, "
                     r"stats_out: \*mut RaycaStats\) -> i32;", shim)


def test_null_arguments_are_refused_with_a_message(product_lib):
    q = abi.RaycaQuery()
    rc = product_lib.rayca_hip_query_device(None, None, C.byref(q), None)
    assert rc == abi.ERR_BAD_ARG and "null" in last_error()
    # (a scene handle is only looked at behind the query pointer's check: any non-NULL value will do here)
    dummy = C.create_string_buffer(64)
    rc = product_lib.rayca_hip_query_device(C.cast(dummy, C.c_void_p), None, None, None)
    assert rc == abi.ERR_BAD_ARG and "null" in last_error()
