"""rayca_hip_scene_update without a GPU: the entry point is exported and bound, refuses a null handle before it touches a
device, and the C++ mirror's DeviceScene::update compiles against include/rayca.hpp."""
import ctypes as C
import os
import subprocess

from rayca_amd import abi, flatten, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_symbol_is_exported_and_bound(product_lib):
    assert "rayca_hip_scene_update" in abi.PRODUCT_SYMBOLS
    fn = product_lib.rayca_hip_scene_update
    assert fn.restype is C.c_int32
    assert fn.argtypes == [C.c_void_p, C.POINTER(abi.RaycaSceneDesc)]


def test_update_of_a_null_scene_is_a_bad_argument(product_lib):
    from rayca_amd.lib import last_error
    d = flatten(scenes.cornell_scene())
    assert product_lib.rayca_hip_scene_update(None, d.ptr()) == abi.ERR_BAD_ARG
    assert "null" in last_error()
    assert product_lib.rayca_hip_scene_update(None, None) == abi.ERR_BAD_ARG


def test_device_scene_update_python_mirror_exists():
    from rayca_amd import DeviceScene
    assert callable(getattr(DeviceScene, "update", None))


def test_cpp_device_scene_update_compiles(product_lib, tmp_path):
    """compile only: DeviceScene::update(const FlatScene&) and the C entry it calls, against the header the mirrors ship"""
    src = tmp_path / "update.cpp"
    src.write_text(
        '#include "rayca.hpp"\n'
        "void frame(rayca::DeviceScene& resident, const rayca::Scene& edited) {\n"
        "  const rayca::FlatScene flat(edited);\n"
        "  resident.update(flat);\n"
        "}\n"
        "int32_t (*entry)(RaycaScene*, const RaycaSceneDesc*) = &rayca_hip_scene_update;\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "update.o")], check=True)
