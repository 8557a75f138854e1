"""The shading goniometer without a GPU: the float64 literal (shading_literal.py) pinned to the oracle where the two spell the same
thing, the float32 restatement of the kernels' closed forms inside the literal's conditioning bound at every kept point, the
families of shading_cases.py reaching the structures they are named for, and the power of the bound: seven wrong spellings of
the arithmetic, each leaving it somewhere.

The oracle's share of family A's pixels outside the bound is printed and not asserted: the oracle keeps the reference's libm
spelling of the GGX terms, tan(acos c)^2 and powf, whose float32 composition the bound does not cover at grazing angles.  That
number is why family A is held to float64 and not to the oracle."""
import numpy as np
import pytest

import shading_cases as sc
import shading_literal as sl

_DATA = {}


def family(name):
    """per case of a family: (case, records from the oracle's rays / hits / HitInfo, the literal's pixels with their bound, the
    oracle's frame (N, 3), the oracle's statistics); made once, read-only"""
    if name not in _DATA:
        rows = []
        for case in sc.FAMILIES[name]():
            be = sc.OracleBackend(case.desc)
            rec = sc.records(case, be)
            _, f32, st = be.render(case.config, case.width, case.height)
            be.close()
            want = sc.expected(case, rec) if case.family != "E" else None
            rows.append((case, rec, want, f32.reshape(-1, 4)[:, :3].copy(), st))
        _DATA[name] = rows
    return _DATA[name]


def violations(j):
    return len(j["outside"]) + len(j["special_differs"])


def cosines(case, rec):
    """float64 n.wi, n.wo, n.h and r.wi of the case's first light at every record"""
    p, n, wo = (np.asarray(rec[k], np.float64) for k in ("point", "normal", "view"))
    wi = sl.normalize(np.asarray(case.lights[0]["position"], np.float64) - p)
    return sl.dot(n, wi), sl.dot(n, wo), sl.dot(n, sl.normalize(wi + wo)), sl.dot(sl.normalize(sl.reflect(-wo, n)), wi)


@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_literal_agrees_with_the_oracle_where_both_spell_the_same(name):
    """Phong, the light terms and the Whitted radiance have no closed form anywhere: the oracle's float32 frame has to lie inside
    the float64 bound at every kept pixel and show the literal's NaNs and infinities exactly."""
    worst = 0.0
    for case, rec, want, frame, _ in family(name):
        j = sl.judge(frame, want)
        worst = max(worst, j["worst"])
        i = (list(j["outside"]) + list(j["special_differs"]) + [0])[0]
        assert violations(j) == 0, f"{case!r}: {len(j['outside'])} pixels outside, {len(j['special_differs'])} special pixels differ; pixel {i}: " \
                                   f"oracle {frame[i]} literal {want['value'][i]} in [{want['lo'][i]}, {want['hi'][i]}] kind {rec['kind'][i]}"
    print(f"family {name}: the oracle's worst pixel at {worst:.3f} of its half envelope")


@pytest.mark.parametrize("name", ["A", "B", "C", "F"])
def test_closed_form_f32_lies_inside_the_bound(name):
    """what settles DELTA0, DELTA_R and EPS: the header's arithmetic in numpy float32, powf as the host has it and one float32
    step to either side"""
    worst = 0.0
    for case, rec, want, _, _ in family(name):
        for ulps in (0, 1, -1):
            j = sl.judge(sl.closed_form_f32(rec, case.lights, sc.visible(case, rec), pow_ulps=ulps), want)
            worst = max(worst, j["worst"])
            assert violations(j) == 0, f"{case!r} (powf {ulps:+d} ulp): outside at {j['outside'][:5]}, special pixels differ at {j['special_differs'][:5]}"
    print(f"family {name}: closed_form_f32's worst pixel at {worst:.3f} of its half envelope")
    assert worst <= 1.0


def test_the_constants_are_the_smallest_of_their_ladders():
    """one halving step down in any of the three and closed_form_f32 leaves the bound somewhere"""
    saved = sl.DELTA0, sl.DELTA_R, sl.EPS
    try:
        for d0, dr, eps in ((saved[0] / 2, saved[1] / 2, saved[2]), (saved[0], 2.0 * saved[0], saved[2]), (saved[0], saved[1], saved[2] / 2)):
            sl.DELTA0, sl.DELTA_R, sl.EPS = d0, dr, eps
            n = 0
            for name in "AB":
                for case, rec, _, _, _ in family(name):
                    n += violations(sl.judge(sl.closed_form_f32(rec, case.lights, sc.visible(case, rec)), sc.expected(case, rec)))
            print(f"DELTA0 {d0 * 2 ** 24:g} x 2^-24, DELTA_R {dr / d0:g} x DELTA0, EPS {eps:g}: {n} pixels outside")
            assert n > 0
    finally:
        sl.DELTA0, sl.DELTA_R, sl.EPS = saved


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "F"])
def test_kept_share_and_displayable_share(name):
    """at most 30 % of a family's hit pixels with a finite value are dropped (too wide a bound, or on the edge of a special case);
    at least half of the compared oracle values lie in [0.1, 100] (the project's tolerance is absolute below 1)"""
    kept = dropped = in_range = values = 0
    for case, rec, want, frame, _ in family(name):
        st = want["status"]
        kept += int((st == sl.KEPT).sum())
        dropped += int(((st == sl.TOO_WIDE) | (st == sl.UNDECIDED)).sum())
        v = np.abs(frame[st == sl.KEPT])
        in_range += int(((v >= 0.1) & (v <= 100.0)).sum())
        values += v.size
        print(f"{case!r:28s} kept {int((st == sl.KEPT).sum()):5d} wide {int((st == sl.TOO_WIDE).sum()):4d} undecided {int((st == sl.UNDECIDED).sum()):4d} "
              f"special {int((st == sl.SPECIAL).sum()):4d} miss {int((st == sl.MISS).sum()):4d}")
    print(f"family {name}: kept {kept / (kept + dropped):.4f}, in [0.1, 100] {in_range / max(values, 1):.3f}")
    assert kept / (kept + dropped) >= 0.70
    assert in_range / values >= 0.5


def test_family_a_reaches_the_peak_of_d_and_grazing_cosines():
    peak = grazing_i = grazing_o = low_rough_peak = 0
    for case, rec, want, _, _ in family("A"):
        ci, co, ch, _ = cosines(case, rec)
        hit = rec["hit"]
        peak += int((hit & (ch > 1.0 - 1e-6)).sum())
        low_rough_peak += int((hit & (ch > 1.0 - 1e-6) & (rec["roughness"] <= 0.02) & (want["status"] == sl.KEPT)).sum())
        grazing_i += int((hit & (ci > 0.0) & (ci < 1e-3)).sum())
        grazing_o += int((hit & (co > 0.0) & (co < 1e-3)).sum())
    print(f"n.h > 1 - 1e-6: {peak} pixels ({low_rough_peak} kept at roughness <= 0.02); n.wi < 1e-3: {grazing_i}; n.wo < 1e-3: {grazing_o}")
    assert peak > 0 and grazing_i > 100 and grazing_o > 100


def test_family_b_reaches_nan_and_the_negative_lobe():
    nan = negative = 0
    for case, rec, want, frame, _ in family("B"):
        r_wi = cosines(case, rec)[3]
        nan_here = np.isnan(frame).any(1)
        assert (rec["shininess"][nan_here] == 2.5).all() and (r_wi[nan_here] < 0.0).all()
        nan += int(nan_here.sum())
        neg = (frame < 0.0).any(1)
        assert np.isin(rec["shininess"][neg], (1.0, 3.0)).all() and (r_wi[neg] < 0.0).all()     # the odd powers of a negative base
        negative += int((neg & (rec["shininess"] == 3.0)).sum())
    print(f"NaN pixels (shininess 2.5, r.wi < 0): {nan}; negative pixels of shininess 3: {negative}")
    assert nan > 100 and negative > 100


def test_family_c_reaches_infinity_and_the_skipped_sample():
    rows = {case.name: (case, rec, want, frame, st) for case, rec, want, frame, st in family("C")}
    for dist in ("0.001", "1", "1000"):
        frame = rows[f"att000-dist{dist}"][3]
        assert (np.isinf(frame) | np.isnan(frame)).all(1).sum() == frame.shape[0]
    case, rec, want, frame, st = rows["intensity0"]
    assert (frame == 0.0).all() and st["rays_shadow"] == st["hits_shaded"] == rec["hit"].sum() > 0     # the sample that is not traced still counts
    assert (rows["below"][3] == 0.0).all()
    near = rows["att001-dist0.001"][1]
    d = np.linalg.norm(np.asarray(near["point"], np.float64) - np.array(rows["att001-dist0.001"][0].lights[0]["position"]), axis=1)
    assert d.min() < 0.05 and d.max() > 0.5


def test_family_e_reaches_negative_pixels_and_gamma_of_a_negative_mean():
    rows = {case.name: frame for case, _, _, frame, _ in family("E")}
    counts = {k: (int((v < 0.0).any(1).sum()), int(np.isnan(v).any(1).sum())) for k, v in rows.items()}
    print(counts)
    assert counts["behind"][0] > counts["front"][0] > 0     # d_omega below zero, beyond the negative Phong lobe both have
    assert counts["edge-on"][0] > 0
    # gamma: powf(negative, 1 / 2.2) is NaN: every negative pixel of the linear frame
    for k in ("behind", "edge-on"):
        assert counts[k + "-gamma2.2"][0] == 0 and counts[k + "-gamma2.2"][1] == counts[k][0] + counts[k][1]


def test_family_f_has_a_cosine_above_one():
    (case, rec, want, frame, _), = family("F")
    co = cosines(case, rec)[1]
    assert co[sc.F_PIXEL] > 1.0 and np.isnan(frame[sc.F_PIXEL]).all()     # in float64 from the float32 vectors, and G1's NaN in the oracle
    assert want["status"][sc.F_PIXEL] == sl.SPECIAL and np.isnan(want["value"][sc.F_PIXEL]).all()
    assert int(np.isnan(frame).any(1).sum()) == int((want["status"] == sl.SPECIAL).sum()) == 1


def test_terms_at_their_special_arguments():
    """D at a clamped cosine of exactly 0 (no frame reaches it: with both n.wi and n.wo above 0, n.h is; surf_pdf does) and G1 above 1,
    term by term: the special value, exactly."""
    a = np.array(sc.ROUGHNESSES, sl.F)
    for c in (0.0, -0.25, -0.0):
        assert (sl.ggx_d32(a, np.full(a.shape, c, sl.F)) == 0.0).all() and (sl.ggx_d(a.astype(np.float64), np.full(a.shape, c)) == 0.0).all()
    above = np.full(a.shape, 1.0 + 2.0 ** -23, sl.F)
    assert np.isnan(sl.ggx_g132(a, above)).all() and np.isnan(sl.ggx_g1(a.astype(np.float64), above.astype(np.float64))).all()
    assert (sl.ggx_d32(a, np.ones_like(a))[a > 0] > 0).all() and sl.ggx_d32(a, np.ones_like(a))[a == 0] == 0.0     # a = 0: 0 / 0 guarded
    # between the special arguments the closed forms follow the formulas to the roundings their operations allow (the header's
    # "within 4e-7"), which the libm spelling evaluated in float32 does not
    acc = sl.term_accuracy()
    print({k: f"{v:.3g}" for k, v in acc.items()})
    assert acc["d_closed"] <= 13 * sl.U and acc["g1_closed"] <= 8 * sl.U and acc["x5_closed"] <= 4 * sl.U
    assert max(acc["d_closed"], acc["g1_closed"], acc["x5_closed"]) <= 4e-7


@pytest.mark.parametrize("mutant", sl.MUTANTS)
def test_the_bound_catches_a_wrong_spelling(mutant):
    """each mutant of closed_form_f32 leaves the bound -- a kept pixel outside its envelope, or a special pixel with another
    special value -- in at least one family"""
    caught = {}
    for name in "ABCF":
        n = 0
        for case, rec, want, _, _ in family(name):
            n += violations(sl.judge(sl.closed_form_f32(rec, case.lights, sc.visible(case, rec), mutant=mutant), want))
        caught[name] = n
    if mutant == "d_without_guard":
        # no NEE frame evaluates D at a clamped cosine of 0 (see test_terms_at_their_special_arguments): caught at the term
        a = np.array(sc.ROUGHNESSES, sl.F)
        caught["terms"] = int((sl.ggx_d32(a, np.zeros_like(a), mutant=mutant) != sl.ggx_d(a.astype(np.float64), np.zeros(a.shape))).sum())
    print(f"{mutant}: pixels that leave the bound, by family: {caught}")
    assert sum(caught.values()) > 0


def test_oracle_share_of_family_a_outside_the_bound():
    """recorded, not asserted: where the oracle's libm spelling of the GGX terms leaves the float64 bound"""
    total = out = 0
    for case, rec, want, frame, _ in family("A"):
        j = sl.judge(frame, want)
        total += j["kept"]
        out += len(j["outside"])
        print(f"{case!r:20s} oracle outside the bound at {len(j['outside']):4d} of {j['kept']} kept pixels, worst {j['worst']:.3g} half envelopes")
    print(f"family A: the oracle leaves the bound at {out} of {total} kept pixels ({out / total:.4%})")
