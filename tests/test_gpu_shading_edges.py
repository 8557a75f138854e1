"""The shading arithmetic of the kernels -- surf_brdf, ggx_d / ggx_g1 / ggx_f, the Phong lobe and nee_prepare in trace_core.inc,
surf_radiance and light_intensity in general.inc -- at grazing angles, low roughness and degenerate light terms, against float64.

Every frame of shading_cases.py is one BRDF evaluation per pixel and light.  The device's own camera rays, closest hits and
surface records (held word for word to the oracle by test_gpu_surface_oracle.py) are the float32 inputs; from them
shading_literal.pixel() computes the pixel in float64 with the conditioning bound a float32 evaluation has to lie in.

  A (GGX, PBR x point light), F (n.wo above 1)      every kept pixel inside the float64 bound: here the kernels' closed forms and
                                                    the oracle's libm spelling differ, and the oracle cannot judge (its own share
                                                    outside the bound is recorded)
  B (Phong), C (light terms), D (Whitted)           every kept pixel inside the bound, and no pixel beyond 1e-4 of the oracle
  all, E (quad lights from behind and edge-on) too  the NaN set, the infinities with their signs and the sign of every pixel equal
                                                    the oracle's; the engines agree bit for bit; a radiance query along the frame's
                                                    camera rays is the frame; rays_shadow and hits_shaded equal the oracle's

on both builders.  What is measured goes to shading_edges.json in the directory parity_report.py writes its counts to and,
summarised, to shading_edges.log beside it (committed as profiles/shading_edges.log)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import shading_cases as sc
import shading_literal as sl
import parity_report
from parity_report import check_outliers
from rayca_amd import Config, DeviceScene, IntegratorStrategy, abi

pytestmark = pytest.mark.gpu
BUILDERS = {"reference": abi.BUILDER_REFERENCE, "sah": abi.BUILDER_SAH}
ENGINES = {"fused": abi.ENGINE_FUSED, "wavefront": abi.ENGINE_WAVEFRONT, "general": abi.ENGINE_GENERAL}
_OUT = os.path.dirname(parity_report._OUT)     # the run's output directory: the parity counts' file lies there
_ORACLE = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class DeviceBackend:
    """camera rays, closest hits and surface records of a DeviceScene, as numpy arrays"""

    def __init__(self, ds):
        self.ds = ds

    def surface_records(self, config, width, height):
        import torch
        self.rays = self.ds.camera_rays(config, width, height)
        t, prim, uv = self.ds.query(self.rays)
        s = self.ds.surface(self.rays, t, prim, uv)
        torch.cuda.synchronize()
        return self.rays.cpu().numpy(), prim.cpu().numpy().view(np.uint32), {k: v.cpu().numpy() for k, v in s.items()}


def oracle_frame(case):
    """the oracle's frame (N, 3), its statistics and its share of kept pixels outside the float64 bound: once per case, read-only"""
    key = repr(case)
    if key not in _ORACLE:
        be = sc.OracleBackend(case.desc)
        _, f32, st = be.render(case.config, case.width, case.height)
        frame = f32.reshape(-1, 4)[:, :3].copy()
        outside = None
        if case.family != "E":
            j = sl.judge(frame, sc.expected(case, sc.records(case, be)))
            outside = (len(j["outside"]), j["kept"])
        be.close()
        _ORACLE[key] = (frame, st, outside)
    return _ORACLE[key]


def same_special_values_and_signs(got, want):
    with np.errstate(invalid="ignore"):
        return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(np.sign(got)[~np.isnan(got)], np.sign(want)[~np.isnan(want)]))


def record(family, builder, rows):
    os.makedirs(_OUT, exist_ok=True)
    path = os.path.join(_OUT, "shading_edges.json")
    try:
        with open(path) as f:
            report = json.load(f)
    except (OSError, ValueError):
        report = {}
    report[f"{family}/{builder}"] = rows
    with open(path, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    with open(os.path.join(_OUT, "shading_edges.log"), "w") as f:
        f.write("\n".join(summary(report)) + "\n")


def summary(report):
    """the lines of profiles/shading_edges.log from the record of a run's shading_edges.json"""
    lines = ["Shading at grazing angles and low roughness: the device's frames of tests/shading_cases.py against the float64 literal and its",
             "conditioning bound (tests/shading_literal.py: DELTA0 = %g x 2^-24, DELTA_R = %g x DELTA0, EPS = %g), MI355X." % (sl.DELTA0 * 2 ** 24, sl.DELTA_R / sl.DELTA0, sl.EPS),
             "worst: the largest distance of a kept pixel from the float64 value, in half envelopes (1 = on the bound).  from float64: the largest",
             "relative distance of a kept pixel from the float64 value, the device's and the oracle's.  from the oracle: the device's largest",
             "distance from the oracle's pixel by the parity tests' rule (absolute below 1, relative above).", "",
             "family/builder  engine     frames  kept pixels  dropped share  worst  outside  device from float64  oracle from float64  device from the oracle  oracle outside the bound"]
    for key in sorted(report):
        for engine in sorted({r["engine"] for r in report[key]}):
            rs = [r for r in report[key] if r["engine"] == engine]
            kept, dropped = sum(r["kept"] for r in rs), sum(r["wide"] + r["undecided"] for r in rs)
            o_out, o_kept = sum(r["oracle_outside"] for r in rs), sum(r["oracle_kept"] for r in rs)
            lines.append(f"{key:15s} {engine:10s} {len(rs):6d} {kept:12d} {dropped / max(kept + dropped, 1):14.4f} {max(r['worst'] for r in rs):6.3f} "
                         f"{sum(r['outside'] for r in rs):8d} {max(r['device_from_float64'] for r in rs):20.3g} {max(r['oracle_from_float64'] for r in rs):20.3g} "
                         f"{max(r['device_from_oracle'] for r in rs):23.3g}  {o_out} of {o_kept} ({o_out / max(o_kept, 1):.2%})")
    if "A/sah" in report:
        lines += ["", "Family A frame by frame (fused engine, SAH builder):",
                  "frame            kept  dropped  worst  device from float64  oracle from float64  device from the oracle  oracle outside the bound"]
        for r in report["A/sah"]:
            if r["engine"] == "fused":
                lines.append(f"{r['case']:14s} {r['kept']:6d} {r['wide'] + r['undecided']:8d} {r['worst']:6.3f} {r['device_from_float64']:20.3g} {r['oracle_from_float64']:20.3g} "
                             f"{r['device_from_oracle']:23.3g}  {r['oracle_outside']}")
    acc = sl.term_accuracy()
    lines += ["", "The GGX terms alone, largest relative error against float64 over cosines 1e-4 .. 1 - 6e-8 and roughness 1 .. 1e-3, numpy float32:",
              f"closed forms (the kernels' spelling):  D {acc['d_closed']:.3g}  G1 {acc['g1_closed']:.3g}  x^5 {acc['x5_closed']:.3g}",
              f"libm compositions (the reference's):   D {acc['d_libm']:.3g}  G1 {acc['g1_libm']:.3g}  x^5 {acc['x5_libm']:.3g}"]
    return lines


def engines_of(case):
    if case.config.integrator == IntegratorStrategy.Raytracer:
        return ["general"]     # the generation kernels hand a Raytracer to the stack machine
    return list(ENGINES)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F"])
def test_family(gpu, name, builder):
    import torch
    rows, failures = [], []
    for case in sc.FAMILIES[name]():
        ds = DeviceScene(case.desc, Config(), builder=BUILDERS[builder])
        if BUILDERS[builder] == abi.BUILDER_SAH:
            ds.finish()
        o_frame, o_st, o_outside = oracle_frame(case)
        want = None
        be = DeviceBackend(ds)
        if name != "E":
            want = sc.expected(case, sc.records(case, be))
        frames = {}
        for engine in engines_of(case):
            _, f32, st = ds.render(case.config, case.width, case.height, engine=ENGINES[engine], collect_stats=True)
            assert (f32[..., 3] == 1.0).all()
            frames[engine] = f32.reshape(-1, 4)[:, :3].copy()
            for k in ("rays_shadow", "hits_shaded"):
                if st[k] != o_st[k]:
                    failures.append(f"{case!r} {engine}: {k} {st[k]}, the oracle's {o_st[k]}")
        if case.config.integrator == IntegratorStrategy.Pathtracer:
            rays = be.rays if name != "E" else ds.camera_rays(case.config, case.width, case.height)
            out, st = ds.radiance(rays, case.config, collect_stats=True)
            torch.cuda.synchronize()
            frames["radiance"] = out.cpu().numpy()[:, :3].copy()
            if st["rays_shadow"] != o_st["rays_shadow"]:
                failures.append(f"{case!r} radiance: rays_shadow {st['rays_shadow']}, the oracle's {o_st['rays_shadow']}")
        ds.close()
        first = next(iter(frames))
        for engine, frame in frames.items():
            if not np.array_equal(bits(frame), bits(frames[first])):
                failures.append(f"{case!r}: {engine} and {first} differ in {int((bits(frame) != bits(frames[first])).any(1).sum())} pixels")
            if not same_special_values_and_signs(frame, o_frame):
                failures.append(f"{case!r} {engine}: NaN {int(np.isnan(frame).any(1).sum())} / {int(np.isnan(o_frame).any(1).sum())}, inf "
                                f"{int(np.isinf(frame).any(1).sum())} / {int(np.isinf(o_frame).any(1).sum())}, negative "
                                f"{int((frame < 0).any(1).sum())} / {int((o_frame < 0).any(1).sum())} pixels (device / oracle): the sets differ")
            if want is None:
                continue
            j = sl.judge(frame, want)
            kept = (want["status"] == sl.KEPT)[:, None] & (want["value"] != 0.0)
            with np.errstate(all="ignore"):
                from_f64 = [float(np.max(np.where(kept, np.abs(f - want["value"]) / np.abs(want["value"]), 0.0), initial=0.0)) for f in (frame, o_frame)]
                finite = np.isfinite(o_frame) & np.isfinite(frame)
                from_oracle = float(np.max(np.where(finite, np.abs(frame - o_frame) / np.maximum(1.0, np.abs(o_frame)), 0.0), initial=0.0))
            rows.append(dict(case=case.name, engine=engine, kept=j["kept"], wide=j["wide"], undecided=j["undecided"], special=j["special"],
                             miss=j["miss"], worst=j["worst"], outside=len(j["outside"]), special_differs=len(j["special_differs"]),
                             oracle_outside=o_outside[0], oracle_kept=o_outside[1], device_from_float64=from_f64[0], oracle_from_float64=from_f64[1],
                             device_from_oracle=from_oracle))
            print(f"{case!r:28s} {engine:9s} kept {j['kept']:5d} dropped {j['wide'] + j['undecided']:4d} special {j['special']:4d} worst {j['worst']:.3f} "
                  f"outside {len(j['outside'])}; the oracle outside at {o_outside[0]}")
            if len(j["outside"]) or len(j["special_differs"]):
                i = (list(j["outside"]) + list(j["special_differs"]))[0]
                failures.append(f"{case!r} {engine}: {len(j['outside'])} kept pixels outside the float64 bound, {len(j['special_differs'])} special pixels differ; "
                                f"pixel {i}: device {frame[i]} literal {want['value'][i]} in [{want['lo'][i]}, {want['hi'][i]}] oracle {o_frame[i]}")
            if name in "BCD":
                # (an infinity has no distance from an infinity: the sets were compared above, the finite pixels are compared here)
                finite = np.isfinite(o_frame)
                try:
                    check_outliers(f"shading_edges_{name}_{case.name}_{builder}_{engine}", np.where(finite, frame, 0.0), np.where(finite, o_frame, 0.0))
                except AssertionError as e:
                    failures.append(f"{case!r} {engine}: {e}")
    if rows:
        record(name, builder, rows)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:20])
