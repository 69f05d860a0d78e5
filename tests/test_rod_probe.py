"""The contact law's and the kinematic step's references, cases and budgets (tests/rod_probe_ref.py) on the CPU: the
scalar transcription of the literal law is the NumPy twin's function, no element of any crafted rod sits where the
float run and the 50-digit run disagree about the surface_tol cut (the exclusion cap is zero), the branch quantities
really are spread over their regimes — the rod's two end elements included —, every budget is computed from the
reference side and has teeth, and the kinematic step's operation sequence meets its derived budgets in NumPy, with and
without single-rounding fmas.  tests/test_gpu_rod_probe.py holds the device to the same cases and budgets.

TEETH.  Each mutation of the transcription in rod_probe_ref.MUTATIONS — a swapped coefficient pair, swapped or
halved end weights, the rolling direction negated, 1/3 -> 1/2, 2 t_axial -> t_axial, the rest radius, a ramp that
saturates at three thresholds, the damping's sign, a static cap from the kinetic coefficient, one radius along a
tapered rod, the torque's arm pointing up — run in floats must leave the budget of at least one case.
"""
import json

import numpy as np
import pytest

from tests import rod_probe_ref as R

CASES = R.contact_cases()
KIN = R.kin_cases()


def record(**kw):
    print("rod-probe-record: " + json.dumps(kw))


def test_cases_are_single_launches_of_at_most_16_waves():
    for case in CASES.values():
        assert 1 <= len(case.rods) <= R.MAX_WAVES
        for form in case.forms:
            assert case.n + 1 <= R.WAVE * R.FORM_EPL[form]
    assert {c.n for c in CASES.values() if R.ZUP1 in c.forms} >= {2, 5, 63}
    assert {c.n for c in CASES.values() if R.ZUP2 in c.forms} >= {5, 64, 101, 126}
    assert {c.n for c in CASES.values() if set(c.forms) & {R.ZUP_TAPER1, R.ZUP_TAPER2}} >= {5, 63, 101}
    for case in KIN.values():
        assert 1 <= case.waves <= R.MAX_WAVES
    for case in CASES.values():             # the tapered rods fall 10:1, every radius inside the envs' range
        for rod in case.rods:
            radius = rod.r0s / np.sqrt(rod.len)
            assert 0.9e-3 <= radius.min() and radius.max() <= 1.3e-2
            if rod.taper:
                assert abs(rod.r0s[0] / rod.r0s[-1] - 10.0) < 1e-9


@pytest.mark.parametrize("name", list(CASES))
def test_the_transcription_is_the_numpy_twins_function(name):
    """In Python floats, to 1e-12 of the rod's largest force component (nodal forces in and out) and of its largest
    torque component: the scalar transcription and the project's pinned second transcription are the same law.
    (Against the contact force alone the bound is not one two roundings of the law can meet: k (dist - radius) is a
    difference of two numbers near 6e-3 times 100, so its last bit is 2e-16, and a rod that barely touches returns
    4e-5 — generic/n5 has one where the twin's matrix product and a left-to-right dot differ by 5e-12 of that.)"""
    for rod in CASES[name].rods:
        fc, dt, _ = R.float_law(rod)
        tf, tt = R.twin_law(rod)
        f_scale = max(np.abs(tf).max(), np.abs(rod.F).max())
        t_scale = max(np.abs(tt).max(), np.abs(rod.tq).max())
        assert f_scale > 0 and np.abs(fc - tf).max() <= 1e-12 * f_scale
        assert np.abs(dt - tt).max() <= 1e-12 * t_scale


@pytest.mark.parametrize("name", list(CASES))
def test_no_element_is_excused(name):
    """The exclusion cap is zero because the law is continuous everywhere but at the surface_tol cut, and no element
    is nearer to the cut than surface_tol x 1e-6: the float run and the 50-digit run take the same side everywhere."""
    case = CASES[name]
    for rod, (_, _, ref) in zip(case.rods, R.contact_reference(name)):
        _, _, flt = R.float_law(rod)
        for a, b in zip(ref, flt):
            assert a.off == b.off
            assert abs(float(a.gap) / R.SURFACE_TOL - 1.0) >= 0.99e-6
            assert abs(float(a.gap) - b.gap) < 1e-15


def test_every_regime_is_reached_in_one_wave_and_at_both_ends():
    seen = {}
    for name in CASES:
        launch = {}
        for _, _, info in R.contact_reference(name):
            reg = R.regimes(info)
            for key, labels in reg.items():
                seen.setdefault(("first", key), set()).add(labels[0])
                seen.setdefault(("last", key), set()).add(labels[-1])
                launch.setdefault(key, set()).update(labels)
                if len(info) >= 63:           # one rod, one wave: its elements sit in different branches
                    assert len(set(labels)) >= 2, (name, key, set(labels))
        if CASES[name].n >= 63:               # and one launch holds every regime of every branch quantity
            for key, want in R.ALL_REGIMES.items():
                assert launch[key] >= want, (name, key, launch[key])
    for key, want in R.ALL_REGIMES.items():
        assert seen["first", key] >= want, ("first element", key, seen["first", key])
        assert seen["last", key] >= want, ("last element", key, seen["last", key])
    # exact zeros of both signs are among the inputs, and the exact multiples of slip_velocity_tol
    assert {0.0, 1.0, 1.3, 1.7, 2.0} <= set(abs(s) for s in R.SLIPS)
    signs = {np.signbit(rod.w[e, 0]) for c in CASES.values() for rod in c.rods for e in range(rod.n)
             if not rod.w[e].any()}
    assert signs == {True, False}


def test_exact_zeros_of_both_signs_and_the_exact_zero_gap_are_reached():
    """The rods at rest (rod_probe_ref.make_zero_rod): the axial speed, the rolling slip, the push and the no-slip
    force are exact zeros in the 50-digit run and in floats, the push of both signs; the middle element's gap as fp64
    forms it is exactly 0, the threshold of the penetration term, where the 50-digit gap is a fraction of an ulp to
    either side."""
    push_signs, gap_sides = set(), set()
    for rod, (_, _, ref) in zip(CASES[R.ZERO_CASE].rods, R.contact_reference(R.ZERO_CASE)):
        _, _, flt = R.float_law(rod)
        assert flt[rod.n // 2].gap == 0.0
        gap_sides.add(ref[rod.n // 2].gap > 0)
        for a, b in zip(ref, flt):
            assert a.vam == 0 and a.srm == 0 and a.push == 0 and a.noslip == 0 and a.along < 0
            assert b.vam == 0.0 and b.srm == 0.0 and b.push == 0.0 and b.noslip == 0.0
            push_signs.add(bool(np.signbit(b.push)))
        labels = R.regimes(ref)
        assert set(labels["push"]) == set(labels["no-slip"]) == set(labels["axial speed"]) == {"zero"}
    assert push_signs == {True, False} and gap_sides == {True, False}
    assert {bool(np.signbit(rod.v[0, 0])) for rod in CASES[R.ZERO_CASE].rods} == {True, False}


@pytest.mark.parametrize("name", list(CASES))
def test_budgets_come_from_the_reference_side(name):
    for quantity, b in R.contact_budget(name).items():
        record(case=name, quantity=quantity, unit="2^-52 x scale", **{k: round(v, 3) for k, v in b.items()})
        assert np.isfinite(b["baseline"]) and b["baseline"] == max(b["float"], b["twin"])
        assert b["budget"] == max(8.0, 4.0 * b["baseline"]) and b["literal_budget"] == max(8.0, 2.0 * b["baseline"])
        assert b["baseline"] < 1.0e3              # a case this ill-conditioned would hold nothing


def _worst_over_budget(name, mut):
    case, budget = CASES[name], R.contact_budget(name)
    worst = 0.0
    for rod, ref in zip(case.rods, R.contact_reference(name)):
        fc, dt, _ = R.float_law(rod, mut=(mut,))
        ef, et = R.contact_errors(ref, fc, R._mp_rows(dt))
        worst = max(worst, ef.max() / budget["force"]["budget"], et.max() / budget["torque"]["budget"])
    return worst


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_leaves_a_budget(mut):
    caught = {name: _worst_over_budget(name, mut) for name in CASES}
    hit = [n for n, w in caught.items() if w > 1.0]
    record(mutation=mut, cases_over_budget=len(hit), worst=float(max(caught.values())))
    assert hit, f"{mut}: inside every budget (worst {max(caught.values()):.3g} of 1)"


def test_the_unmutated_transcription_is_inside_every_budget():
    for name in CASES:
        assert _worst_over_budget(name, None) <= 1.0


# ---- the kinematic step ------------------------------------------------------------------------------------------
def test_kinematic_cases_reach_their_tiers():
    trips = {name: set(np.unique(R.kin_trips(case))) for name, case in KIN.items()}
    assert trips["in_range"] == {0} and trips["axis_aligned_and_zero"] == {0}
    assert trips["edge"] == {0, 1}
    assert trips["quartered"] == set(range(1, 10))
    assert trips["mixed"] == {12}
    assert trips["two_slots"] == {0, 3, 9, 1, 6}
    k = R.kin_trips(KIN["two_slots"]).reshape(-1, R.WAVE, 2)
    assert np.all(k[:, :, 0] != k[:, :, 1])                 # the two slots of a lane in different regimes
    a = np.linalg.norm(KIN["quartered"].w * KIN["quartered"].h, axis=1)
    assert 9.9 < a.max() < 10.0
    t = np.sum((KIN["in_range"].w * KIN["in_range"].h) ** 2, axis=1)
    assert t.max() < 1e-3 and t.max() > 0.999e-3 and np.sqrt(t.min()) < 1e-11


def test_kinematic_transcriptions_meet_the_derived_budgets():
    """Both roundings of the operation sequence, per trip count; the fall-back rule applies only where the exactly
    rounded-fma transcription itself misses the derived bound, and the record names those k."""
    budgets = R.kin_budgets()
    record(block="kinematic_n", unit="ulp (2^-52) absolute",
           by_trips={k: {n: (round(v, 3) if isinstance(v, float) else v) for n, v in d.items()}
                     for k, d in sorted(budgets.items())})
    for k, d in budgets.items():
        assert d["derived"] == (3.0 if k == 0 else 2.0 * (k + 3))
        assert d["fma"] <= d["budget"] and d["plain"] <= d["budget"], (k, d)
        if d["note"] == "derived":
            assert d["budget"] == d["derived"]
        else:
            assert d["fma"] > d["derived"] and d["budget"] == d["fma"] + 2.0
    for name, case in KIN.items():
        with np.errstate(all="ignore"):
            ex, _ = R.kin_errors(name, *R.t_kinematic(case))
        assert ex.max() <= 1.0, (name, ex.max())


def test_kinematic_budget_has_teeth():
    """A cosc with 1/24 written as 1/25, or a transposed R, leaves the in-range budget by orders of magnitude."""
    case = KIN["in_range"]
    x, Q = R.t_kinematic(case)
    flipped = R.KinCase(case.name, case.epl, case.h, case.x, case.v, case.Q, -case.w, case.hx, case.hq)
    _, Qt = R.t_kinematic(flipped)
    _, eq = R.kin_errors("in_range", x, Qt)
    assert eq.max() > 1e6
    _, eq = R.kin_errors("in_range", x, Q * (1 + 4 * R.ULP))
    assert eq.max() > 3.0


@pytest.mark.parametrize("name", ["held"])
def test_held_slots_stay_in_place(name):
    """hq = 0 leaves all nine entries of Q, hx = 0 the position, bit for bit, for any finite w and v — in a blown-up
    wave too (the operation sequence: R = I exactly, and 1 b + 0 b' + 0 b'' = b for b != 0)."""
    case = KIN[name]
    with np.errstate(all="ignore"):
        x, Q = R.t_kinematic(case)
    held_q, held_x = case.hq == 0.0, case.hx == 0.0
    assert held_q.sum() > 90 and held_x.sum() > 60 and 12 in R.kin_trips(case)[~held_q]
    assert np.array_equal(Q[held_q].view(np.uint64), case.Q[held_q].view(np.uint64))
    assert np.array_equal(x[held_x].view(np.uint64), case.x[held_x].view(np.uint64))
    assert not np.array_equal(Q[~held_q], case.Q[~held_q])


def test_the_record_covers_every_case_and_shows_the_device_inside_its_budget():
    """profiles/rod_probe_error.json is a copy of the GPU test's lines for THESE cases: its baselines are the ones
    computed here, every (case, form) and every kinematic case is there, and the device's maxima are inside."""
    from pathlib import Path

    rec = json.loads((Path(__file__).resolve().parents[1] / "profiles" / "rod_probe_error.json").read_text())
    assert {b["case"] for b in rec["contact_baselines"]["cases"]} == set(CASES)
    for b in rec["contact_baselines"]["cases"]:
        for q in ("force", "torque"):
            assert b[q]["baseline"] == pytest.approx(R.contact_budget(b["case"])[q]["baseline"], rel=1e-3, abs=1e-3), b
    value = [r for r in rec["records"] if "form" in r and "device_force" in r]
    assert {(r["case"], r["form"]) for r in value} == {(n, R.FORM_NAMES[f]) for n, c in CASES.items() for f in c.forms}
    for r in value:
        assert r["device_force"] <= r["force_budget"] and r["device_torque"] <= r["torque_budget"], (r["case"], r["form"])
    kin = [r for r in rec["records"] if r.get("block") == "kinematic_n" and "device_by_trips" in r]
    assert {r["case"] for r in kin} == set(KIN)
    for r in kin:
        assert r["device_position"] <= 1.0
        for k, v in r["device_by_trips"].items():
            assert v <= r["budget_by_trips"][k] == pytest.approx(R.kin_budgets()[int(k)]["budget"]), (r["case"], k)
