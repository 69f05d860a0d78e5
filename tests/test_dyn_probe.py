"""The references, cases and budgets of tests/dyn_probe_ref.py, checked on the CPU (no GPU needed): the literal law L
against the NumPy twin, the planar substep P against L inside the bounds softrod_planar.hpp states, budgets that are
finite and excuse nothing, the tiers the cases reach, and the teeth: fifteen single mutations of L or P, each of which
leaves the budget of at least one case when the mutated float run stands in for the device.
"""
import json

import numpy as np
import pytest

from tests import dyn_probe_ref as D
from tests import math_primitives_ref as M

CASES = D.dyn_cases()
PLANAR = D.planar_cases()
SMALL = [n for n, c in CASES.items() if c.n <= 5]
SMALL_PLANAR = [n for n, c in PLANAR.items() if c.n <= 5]


_masks = D.case_masks


@pytest.mark.parametrize("name", list(CASES))
def test_literal_law_in_floats_is_the_numpy_twin(name):
    """1e-12 of the rod's largest internal force / torque component (through dt / m and dt / J), kappa and t relative."""
    case = CASES[name]
    for mask in _masks(case):
        feat = D.mask_features(mask) & ~D.PLANE_ZUP & ~D.CONTACT      # (the lifted rods' contact adds nothing: below)
        for rod in case.rods:
            a, b = D.literal_law(rod, D.FLOAT, features=feat), D.twin(rod, feat)
            m = rod.mat
            fs = max(float(np.abs(b.f_int).max()), 1e-300) * m.dt / float(np.min(m.mass))
            ts = max(float(np.abs(b.t_int).max()), 1e-300) * m.dt * float(np.max(m.invJ0)) * 2.0
            assert np.abs(np.array(a.v) - b.v).max() <= 1e-12 * (fs + np.abs(b.v).max())
            assert np.abs(np.array(a.w) - b.w).max() <= 1e-12 * (ts + np.abs(b.w).max())
            assert np.abs(np.array(a.t) - b.t).max() <= 1e-12
            assert np.abs(np.array(a.kap) - b.kap).max() <= 1e-12 * max(float(np.abs(b.kap).max()), 1.0)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.lifted])
def test_contact_adds_exactly_nothing_to_the_lifted_rods(name):
    """The compiled arm mask runs the contact operator; rod_probe_ref.contact_law says its force and torque on these
    states (1 m above the plane) are exact zeros, so the literal law without contact is their reference."""
    for rod in CASES[name].rods:
        assert D.contact_is_zero(rod)


def test_planar_substep_against_the_literal_law_within_the_headers_bounds():
    """softrod_planar.hpp: kappa = s2 D / D^ times 1 + acos_shift / 3 to O(1e-10 D^2), the eps_sin factor to 1e-16.  At 50
    digits, per vertex: the couple's relative difference <= 1e-10 D^2 + 1e-16; everything else identical."""
    worst, worst_d, other, small = 0.0, 0.0, 0.0, 0.0
    for name in SMALL_PLANAR:
        for rod in PLANAR[name].rods:
            couples, rest = D.planar_gap(rod)
            other = max(other, float(rest))
            for rel, Dk, _ in couples:
                if Dk == 0:
                    continue
                bound = 1e-10 * float(Dk) ** 2 + 1e-16
                if float(rel) / bound > worst:
                    worst, worst_d = float(rel) / bound, float(Dk)
                if abs(float(Dk)) <= 1e-5:
                    small = max(small, float(rel))
                assert float(rel) <= bound, f"{name}: D = {float(Dk)}: {float(rel)} of {bound}"
    print("dyn-probe-record: " + json.dumps({"check": "P against L at 50 digits", "couple_over_bound": round(worst, 4),
                                             "at_D": worst_d, "couple_rel_nearly_straight": small,
                                             "everything_else_rel": other}))
    assert other <= 1e-40


@pytest.mark.parametrize("name", list(CASES))
def test_every_budget_is_finite_and_no_output_is_excused(name):
    case = CASES[name]
    for mask in _masks(case):
        budget = D.dyn_budget(name, mask)
        compared = total = 0
        for rod, (ref, scales) in zip(case.rods, D.dyn_reference(name, mask)):
            errs = D.dyn_errors(rod, ref, scales, D.literal_law(rod, D.FLOAT, features=D.mask_features(mask)))
            for k, n_out in zip(D.OUTPUTS, (rod.n + 1, rod.n, rod.n, rod.n - 1)):
                total += n_out
                compared += int(np.sum(np.isfinite(errs[k])))
                assert len(errs[k]) == n_out
            assert all(np.all(np.isfinite(s)) and np.all(s > 0) for s in scales)
        assert compared == total                      # the share left out of any comparison is 0
        for k in D.OUTPUTS:
            assert np.isfinite(budget[k]["budget"]) and 8.0 <= budget[k]["budget"] < 1.0e4, (k, budget[k])


@pytest.mark.parametrize("name", list(PLANAR))
def test_every_planar_budget_is_finite(name):
    budget = D.planar_budget(name)
    for rod, (ref, scales) in zip(PLANAR[name].rods, D.planar_reference(name)):
        assert all(np.all(np.isfinite(s)) and np.all(s > 0) for s in scales)
        errs = D.planar_errors(ref, scales, D.planar_law(rod, D.FLOAT))
        assert [len(errs[k]) for k in D.PLANAR_OUTPUTS] == [rod.n + 1, rod.n, rod.n, rod.n]
    for k in D.PLANAR_OUTPUTS:
        assert np.isfinite(budget[k]["budget"]) and 8.0 <= budget[k]["budget"] < 1.0e3, (k, budget[k])


def test_every_tier_is_reached():
    """Counted from the 50-digit run: every tier of theta_over_sin (6, 12, 20 terms, half angle) and every tier of
    exp_pair (|x| < 1e-3, < 0.04, beyond) are hit by a joint / an element, every wave tier is taken by a rod, a `hot` rod stays in the
    first tiers and a `one_theta` / `one_stretch` rod is dragged out of them by its one joint / element."""
    joints, elems, wave_theta, wave_exp = set(), set(), set(), set()
    for name in SMALL + [n for n in CASES if "n63" in n and not CASES[n].lifted]:
        case = CASES[name]
        for rod, (ref, _) in zip(case.rods, D.dyn_reference(name, _masks(case)[0])):
            wt, we, j, e = D.tiers(rod, ref)
            joints |= j
            elems |= e
            wave_theta.add(wt)
            wave_exp.add(we)
            if rod.kind in ("hot", "hot_zeros"):
                assert (wt, we) == (0, 0)
            if name.startswith("from-"):
                continue
            if rod.kind == "one_theta":
                assert wt == 3 and we == 0 and (rod.n == 2 or min(j) == 0)
            if rod.kind == "one_stretch":
                assert we == 2 and wt == 0 and min(e) == 0
    assert joints == {0, 1, 2, 3} and wave_theta == {0, 1, 2, 3}, (joints, wave_theta)
    assert elems == {0, 1, 2} and wave_exp == {0, 1, 2}, (elems, wave_exp)
    halvings = {c.halvings for c in PLANAR.values()}
    assert 0 in halvings and max(halvings) >= 1


def _factor(errs, budget):
    return max(float(errs[k].max()) / budget[k]["budget"] for k in errs if len(errs[k]))


def test_teeth_every_mutation_leaves_a_budget():
    """Each single mutation of L (or P), run in floats in the device's place, misses the budget of at least one case."""
    factors = {}
    for mut in D.MUTATIONS:
        best, where = 0.0, None
        if mut not in D.PLANAR_ONLY:
            for name in SMALL:
                case = CASES[name]
                if case.lifted or name.startswith("from-"):
                    continue
                mask = "damper+rest_kappa"
                budget = D.dyn_budget(name, mask)
                for rod, (ref, scales) in zip(case.rods, D.dyn_reference(name, mask)):
                    run = D.literal_law(rod, D.FLOAT, mut=(mut,), features=D.mask_features(mask))
                    f = _factor(D.dyn_errors(rod, ref, scales, run), budget)
                    if f > best:
                        best, where = f, name
        if mut in D.PLANAR_ONLY or best <= 1.0:
            for name in SMALL_PLANAR:
                budget = D.planar_budget(name)
                for rod, (ref, scales) in zip(PLANAR[name].rods, D.planar_reference(name)):
                    f = _factor(D.planar_errors(ref, scales, D.planar_law(rod, D.FLOAT, mut=(mut,))), budget)
                    if f > best:
                        best, where = f, name
        factors[mut] = (best, where)
    print("dyn-probe-record: " + json.dumps({"check": "teeth", "unit": "mutated float run / budget, best case",
                                             "factors": {k: [float(f"{v[0]:.4g}"), v[1]] for k, v in factors.items()}}))
    missed = [k for k, v in factors.items() if not v[0] > 1.0]
    assert not missed, f"no case sees {missed}"
    assert len(factors) >= 12


def test_unmutated_float_runs_sit_inside_their_budgets():
    """(the teeth's control: the same loop without a mutation stays inside, at a quarter of the budget or less)"""
    for name in SMALL:
        case = CASES[name]
        for mask in _masks(case):
            budget = D.dyn_budget(name, mask)
            for rod, (ref, scales) in zip(case.rods, D.dyn_reference(name, mask)):
                run = D.literal_law(rod, D.FLOAT, features=D.mask_features(mask))
                assert _factor(D.dyn_errors(rod, ref, scales, run), budget) <= 0.25 + 1e-12


def test_the_argument_checks_are_named():
    """The GPU test drives these lists; every refusal the two entry points document has an entry."""
    dyn, planar = dict(D.BAD_DYNAMIC), dict(D.BAD_PLANAR)
    assert len(dyn) == len(D.BAD_DYNAMIC) and len(planar) == len(D.BAD_PLANAR)
    for needed in ("unknown form", "no rods", "too many rods", "one element", "65 nodes in 64 lanes",
                   "129 nodes in 128 slots", "no x"):
        assert needed in dyn
    for needed in ("epl 3", "no rods", "too many rods", "one element", "65 nodes in 64 lanes", "129 nodes in 128 slots",
                   "no c"):
        assert needed in planar
    assert len(D.params(CASES["epl1/n5/walk"].mat)) == D.N_PARAMS
    assert D.material_table(CASES["taper/n5/walk"].mat, 1).shape == (D.MAT_ROWS, 64)
    assert M.THETA_EDGES == (2.5e-3, 0.04, 0.15) and M.EXP_EDGES[0] == 1.0e-3
