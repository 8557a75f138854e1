"""rayca_hip_denoise_device without a GPU: the symbol, the layout of RaycaDenoise against the header, the argument errors that
need no scene, and the properties of the filter as specified, on the literal restatement (tests/denoise_literal.py) that the GPU
tests compare the kernels with bit for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_literal as dl
from rayca_amd import abi
from rayca_amd.lib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["width", "height", "iterations", "normal_power_log2", "sigma_color", "sigma_plane", "gamma", "reserved", "color", "albedo",
          "normal", "point", "id", "rgba32f_out", "rgba8_out"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_entry(product_lib):
    assert "rayca_hip_denoise_device" in abi.PRODUCT_SYMBOLS
    assert product_lib.rayca_hip_denoise_device is not None
    assert product_lib.rayca_hip_version() == abi.ABI_VERSION == 2   # (no layout changed: the version stays)


def test_denoise_struct_layout_matches_header():
    """The rule of test_abi.py: a C program prints sizeof / offsetof from the header, ctypes must agree."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/rayca_hip.h"', "int main(void){",
             'printf("RaycaDenoise %zu\\n", sizeof(RaycaDenoise));']
    for name in FIELDS:
        lines.append(f'printf("RaycaDenoise.{name} %zu\\n", offsetof(RaycaDenoise, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = dict(l.split() for l in out.strip().splitlines())
    assert [n for n, _ in abi.RaycaDenoise._fields_] == FIELDS
    assert C.sizeof(abi.RaycaDenoise) == int(want["RaycaDenoise"]) == 8 * 4 + 7 * 8
    for name in FIELDS:
        assert getattr(abi.RaycaDenoise, name).offset == int(want[f"RaycaDenoise.{name}"]), name


def test_argument_errors_that_need_no_scene(product_lib):
    """Every one of these is decided before the scene handle is looked at: any non-NULL value will do for it."""
    f = product_lib.rayca_hip_denoise_device
    dummy = C.create_string_buffer(64)
    scene = C.cast(dummy, C.c_void_p)
    ptr = C.addressof(dummy)   # (stands for a device pointer: nothing is launched)

    def args(**kw):
        d = abi.RaycaDenoise()
        d.width, d.height, d.iterations, d.normal_power_log2, d.sigma_color, d.sigma_plane, d.gamma = 8, 8, 2, 7, 4.0, 0.5, 1.0
        d.color, d.rgba32f_out = ptr, ptr
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def opts(**kw):
        o = abi.RaycaRenderOptions()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad(d, o=None, word=None):
        rc = f(scene, C.byref(o) if o is not None else None, C.byref(d), None)
        return rc == abi.ERR_BAD_ARG and (word is None or word in last_error())

    assert f(None, None, C.byref(args()), None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert f(scene, None, None, None) == abi.ERR_BAD_ARG and "null" in last_error()
    assert bad(args(color=None), word="color")
    assert bad(args(rgba32f_out=None), word="no output")
    assert bad(args(width=0), word="empty image") and bad(args(height=0), word="empty image")
    assert bad(args(width=65536, height=65536), word="2^32")
    assert bad(args(iterations=9), word="iterations")
    assert bad(args(normal_power_log2=11), word="normal_power_log2")
    assert bad(args(point=ptr), word="point needs normal")
    for sigma in (0.0, -1.0, float("nan")):
        assert bad(args(point=ptr, normal=ptr, sigma_plane=sigma), word="sigma_plane"), sigma
    for gamma in (0.0, -2.2, float("nan")):
        assert bad(args(gamma=gamma), word="gamma"), gamma
    assert bad(args(reserved=1), word="reserved")
    assert bad(args(), opts(context=8), word="context")
    for name in ("traversal", "collect_stats", "engine", "camera_rays", "reserved"):
        assert bad(args(), opts(**{name: 1}), word="must be zero"), name
    o = opts()
    o.tile.parts = 2
    assert bad(args(), o, word="tile")


# ---- the filter as specified: properties of the literal ---------------------------------------------------------------------
W, H, SEED = 64, 48, 20240


@pytest.fixture(scope="module")
def frame():
    s = dl.synthetic(W, H, SEED)
    for a in s.values():
        a.setflags(write=False)
    return s


def guides_of(s, which):
    g = {k: s[k] for k in which}
    if "point" in g:
        g["sigma_plane"] = 0.5
    return g


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


@pytest.mark.parametrize("which", [("albedo", "normal", "point", "id"), ()], ids=["all_guides", "no_guides"])
def test_error_falls_with_the_first_iteration_and_never_rises(frame, which):
    errs = [rmse(frame["color"], frame["clean"])]
    for n in range(1, 6):
        out, _ = dl.denoise(frame["color"], iterations=n, **guides_of(frame, which))
        errs.append(rmse(out, frame["clean"]))
    print(which, " ".join(f"{e:.4f}" for e in errs))
    assert errs[1] < errs[0]
    assert all(errs[n + 1] <= errs[n] for n in range(1, 5)), errs


def test_nothing_crosses_an_id_boundary(frame):
    g = guides_of(frame, ("albedo", "normal", "point", "id"))
    out, out8 = dl.denoise(frame["color"], iterations=5, **g)
    side = frame["id"] == 7
    assert 0.2 < side.mean() < 0.8
    rng = np.random.default_rng(5)
    color2, g2 = frame["color"].copy(), {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    color2[side] = rng.uniform(0.0, 50.0, size=color2[side].shape).astype(np.float32)
    for k in ("albedo", "normal", "point"):
        g2[k][side] = rng.uniform(-3.0, 3.0, size=g2[k][side].shape).astype(np.float32)
    out2, out8_2 = dl.denoise(color2, iterations=5, **g2)
    assert np.array_equal(bits(out[~side]), bits(out2[~side])) and np.array_equal(out8[~side], out8_2[~side])
    assert not np.array_equal(bits(out[side]), bits(out2[side]))


@pytest.mark.parametrize("which", [("albedo", "normal", "point", "id"), ()], ids=["all_guides", "no_guides"])
def test_a_nan_pixel_stays_the_only_nan(frame, which):
    color = frame["color"].copy()
    color[20, 31, 1] = np.nan
    out, _ = dl.denoise(color, iterations=5, **guides_of(frame, which))
    nan = np.isnan(out)
    assert nan[20, 31, 1] and nan.sum() == 1
    if "albedo" not in which:   # (the trip through color / den * den may move a finite channel's last bit)
        assert np.array_equal(bits(out[20, 31]), bits(color[20, 31]))   # the pixel passes through, its finite channels too


def test_no_iterations_and_no_gamma_return_the_input_bits(frame):
    out, out8 = dl.denoise(frame["color"], iterations=0, **guides_of(frame, ("albedo", "normal", "point", "id")))
    assert np.array_equal(bits(out), bits(frame["color"]))
    assert np.array_equal(out8, dl.quantize(frame["color"]))
