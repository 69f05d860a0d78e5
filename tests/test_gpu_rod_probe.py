"""The FAST contact law and the 3-D kinematic step alone on the device, against 50 digits.

variants/libsoftrod_rod_probe.so (csrc/probe/softrod_rod_probe.hip, `make probe`) runs plane_contact_n in its FAST
instantiations (z-up and general plane, one and two slots per lane, tapered) and its literal one, and kinematic_n<1> /
<2>, one rod per wave on plain arrays.  The crafted rods, the references, the budgets and the reasons for them are
tests/rod_probe_ref.py's; tests/test_rod_probe.py shows on the CPU that the budgets come from the reference side, that
no element needs to be excused and that thirteen mutations of the law leave them.  Every case is one launch of at most
16 waves.

Each value test prints a line `rod-probe-record: {...}` with the device's maximum, the baseline and the budget;
profiles/rod_probe_error.json is a copy of those lines.
"""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import rod_probe_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CASES = R.contact_cases()
KIN = R.kin_cases()
SENTINEL = -12345.0
TAIL = 64


def layout(case, epl, behind="clean", seed=5):
    """The case's rods as the probe's arrays (rods, 64 epl, components).  behind: what the slots behind each rod hold
    in x, v (past node n), Q, w (past element n - 1): 'clean' zeros, 'poison' NaN / +-inf / 1e300, or 'continued', a
    finite continuation of the rod."""
    W, n, rods = R.WAVE * epl, case.n, case.rods
    rng = np.random.default_rng(seed)
    a = {k: np.zeros((len(rods), W, c)) for k, c in (("x", 3), ("v", 3), ("Q", 9), ("w", 3), ("t", 3), ("F", 3),
                                                    ("tq", 3), ("len", 1), ("mass", 1), ("r0s", 1))}
    a["len"][:] = 1.0
    a["r0s"][:] = 1.0
    for r, rod in enumerate(rods):
        for k in ("x", "v", "F"):
            a[k][r, :n + 1] = getattr(rod, k)
        for k in ("Q", "w", "t", "tq"):
            a[k][r, :n] = getattr(rod, k)
        a["len"][r, :n, 0], a["r0s"][r, :n, 0], a["mass"][r, :n + 1, 0] = rod.len, rod.r0s, rod.mass
        nodes, elems = W - (n + 1), W - n
        if behind == "poison":
            bad = np.array([np.nan, np.inf, -np.inf, 1.0e300, -1.0e300])
            a["x"][r, n + 1:] = rng.choice(bad, (nodes, 3))
            a["v"][r, n + 1:] = rng.choice(bad, (nodes, 3))
            a["Q"][r, n:] = rng.choice(bad, (elems, 9))
            a["w"][r, n:] = rng.choice(bad, (elems, 3))
        elif behind == "continued":
            step = rod.x[n] - rod.x[n - 1]
            a["x"][r, n + 1:] = rod.x[n] + np.arange(1, nodes + 1)[:, None] * step
            a["v"][r, n + 1:] = rng.normal(size=(nodes, 3)) * 1e-3
            a["Q"][r, n:] = np.stack([R._random_rotation(rng).ravel() for _ in range(elems)])
            a["w"][r, n:] = rng.normal(size=(elems, 3))
    return a


class Probe:
    def __init__(self):
        import torch      # first: the probe must bind to the HIP runtime torch has loaded (gym_softrobot_amd/_capi.py)

        self.torch = torch
        path = ROOT / "variants" / "libsoftrod_rod_probe.so"
        if not path.exists():
            subprocess.run(["make", "-C", str(ROOT / "gym_softrobot_amd" / "csrc"), "probe"], check=True)
        self.lib = C.CDLL(str(path))
        self.lib.softrod_rod_probe_contact.restype = C.c_int
        self.lib.softrod_rod_probe_contact.argtypes = [C.c_int] * 3 + [C.c_void_p] * 14
        self.lib.softrod_rod_probe_kinematic.restype = C.c_int
        self.lib.softrod_rod_probe_kinematic.argtypes = [C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 9
        self.lib.softrod_rod_probe_forms.restype = C.c_int
        self.cache = {}

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda")

    def out(self, n):
        return self.torch.full((n + TAIL,), SENTINEL, dtype=self.torch.float64, device="cuda")

    @staticmethod
    def params(par):
        return (C.c_double * 17)(par.k, par.nu, par.slip_tol, par.surface_tol, *par.kin_mu, *par.stat_mu, *par.origin,
                                 *par.normal, par.r0s_uniform)

    def contact(self, case, form, behind="clean"):
        """One launch -> (fc (rods, n + 1, 3), tq_out (rods, n, 3)); nothing else may have been written."""
        epl, n, rods = R.FORM_EPL[form], case.n, len(case.rods)
        W = R.WAVE * epl
        a = layout(case, epl, behind)
        t = {k: self.dev(v) for k, v in a.items()}
        fc, tq = self.out(rods * W * 3), self.out(rods * W * 3)
        rc = self.lib.softrod_rod_probe_contact(
            form, rods, n, C.cast(self.params(case.par), C.c_void_p), *(t[k].data_ptr() for k in
                                                                         ("x", "v", "Q", "w", "t", "len", "F", "tq", "mass", "r0s")),
            fc.data_ptr(), tq.data_ptr(), self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"softrod_rod_probe_contact({form}) returned {rc}"
        self.torch.cuda.synchronize()
        fc, tq = fc.cpu().numpy(), tq.cpu().numpy()
        assert np.all(fc[-TAIL:] == SENTINEL) and np.all(tq[-TAIL:] == SENTINEL), "the probe wrote behind its output"
        fc, tq = fc[:-TAIL].reshape(rods, W, 3), tq[:-TAIL].reshape(rods, W, 3)
        assert np.all(fc[:, n + 1:] == SENTINEL) and np.all(tq[:, n:] == SENTINEL), "a lane behind the rod stored"
        return fc[:, :n + 1].copy(), tq[:, :n].copy()

    def run(self, name, form):
        if (name, form) not in self.cache:
            self.cache[name, form] = self.contact(CASES[name], form)
        return self.cache[name, form]

    def kinematic(self, case):
        n = len(case.hx)
        t = [self.dev(a) for a in (case.x, case.v, case.Q, case.w, case.hx, case.hq)]
        x, Q = self.out(3 * n), self.out(9 * n)
        rc = self.lib.softrod_rod_probe_kinematic(case.epl, case.waves, case.h, *(v.data_ptr() for v in t),
                                                  x.data_ptr(), Q.data_ptr(),
                                                  self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"softrod_rod_probe_kinematic returned {rc}"
        self.torch.cuda.synchronize()
        x, Q = x.cpu().numpy(), Q.cpu().numpy()
        assert np.all(x[-TAIL:] == SENTINEL) and np.all(Q[-TAIL:] == SENTINEL), "the probe wrote behind its output"
        return x[:-TAIL].reshape(n, 3).copy(), Q[:-TAIL].reshape(n, 9).copy()

    def run_kin(self, name):
        if name not in self.cache:
            self.cache[name] = self.kinematic(KIN[name])
        return self.cache[name]


@pytest.fixture(scope="module")
def probe(hip_lib):
    return Probe()


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def record(**kw):
    print("rod-probe-record: " + json.dumps(kw))


def device_errors(name, fc, tq):
    """(force errors (rods, n + 1), torque errors (rods, n)) of one launch's outputs, in budget units."""
    case = CASES[name]
    ef, et = [], []
    for rod, ref, f, t in zip(case.rods, R.contact_reference(name), fc, tq):
        a, b = R.contact_errors(ref, f, R.added_torque(rod.tq, t))
        ef.append(a)
        et.append(b)
    return np.array(ef), np.array(et)


CONTACT = [(n, f) for n, c in CASES.items() for f in c.forms]
CONTACT_IDS = [f"{n}-{R.FORM_NAMES[f]}" for n, f in CONTACT]


@pytest.mark.parametrize("name,form", CONTACT, ids=CONTACT_IDS)
def test_contact_law_meets_its_budget(probe, name, form):
    """Every element of every rod: none is excused.  The FAST forms at 4 x the case's baseline, the literal
    instantiation at 2 x (floor 8), in units of 2^-52 x the reference side's scale."""
    b = R.contact_budget(name)
    key = "literal_budget" if form == R.LITERAL1 else "budget"
    fb, tb = b["force"][key], b["torque"][key]
    fc, tq = probe.run(name, form)
    ef, et = device_errors(name, fc, tq)
    rf, nf = np.unravel_index(np.argmax(ef), ef.shape)
    rt, nt = np.unravel_index(np.argmax(et), et.shape)
    record(case=name, form=R.FORM_NAMES[form], unit="2^-52 x scale", device_force=round(float(ef.max()), 3),
           device_torque=round(float(et.max()), 3), worst_node=[int(rf), int(nf)], worst_element=[int(rt), int(nt)],
           force_baseline=round(b["force"]["baseline"], 3), force_budget=round(fb, 3),
           torque_baseline=round(b["torque"]["baseline"], 3), torque_budget=round(tb, 3))
    assert ef.max() <= fb, f"force: {ef.max():.3f} of {fb:.3f} at rod {rf} node {nf}"
    assert et.max() <= tb, f"torque: {et.max():.3f} of {tb:.3f} at rod {rt} element {nt}"


def _agree(name, form_a, form_b, probe):
    """The two forms' outputs differ by no more than the sum of their budgets (force and torque each against its own);
    -> the larger difference as a fraction of what is allowed."""
    b = R.contact_budget(name)
    (fa, ta), (fb, tb) = probe.run(name, form_a), probe.run(name, form_b)
    worst = 0.0
    for r, ref in enumerate(R.contact_reference(name)):
        node, elem = R.contact_scales(ref)
        worst = max(worst, float((np.abs(fa[r] - fb[r]).max(axis=1) / node).max() / R.ULP) / (2.0 * b["force"]["budget"]),
                    float((np.abs(ta[r] - tb[r]).max(axis=1) / elem).max() / R.ULP) / (2.0 * b["torque"]["budget"]))
    assert worst <= 1.0, f"{worst:.3f} of the sum of the two budgets"
    return worst


EZ = [(n, a, b) for n, c in CASES.items() if c.par.normal == R.E_Z
      for a, b in ((R.ZUP1, R.PLANE1), (R.ZUP2, R.PLANE2)) if a in c.forms and b in c.forms]


@pytest.mark.parametrize("name,zup,plane", EZ, ids=[f"{n}-epl{R.FORM_EPL[a]}" for n, a, _ in EZ])
def test_z_up_and_general_plane_forms_agree_on_e_z(probe, name, zup, plane):
    worst = _agree(name, zup, plane, probe)
    record(case=name, check="z-up against general plane", epl=R.FORM_EPL[zup], difference_over_allowed=round(worst, 5))


@pytest.mark.parametrize("name,one,two", [("ez/n5", R.ZUP1, R.ZUP2), ("ez/n5", R.PLANE1, R.PLANE2),
                                          ("taper/n5", R.ZUP_TAPER1, R.ZUP_TAPER2),
                                          ("generic/n5", R.PLANE1, R.PLANE2)])
def test_one_and_two_slots_per_lane_agree(probe, name, one, two):
    worst = _agree(name, one, two, probe)
    record(case=name, check="EPL 1 against EPL 2", form=R.FORM_NAMES[one], difference_over_allowed=round(worst, 5))


BEHIND = [("ez/n5", R.ZUP1), ("ez/n5", R.ZUP2), ("ez/n63", R.ZUP1), ("ez/n101", R.ZUP2), ("ez/n126", R.ZUP2),
          ("taper/n5", R.ZUP_TAPER1), ("taper/n63", R.ZUP_TAPER2), ("generic/n5", R.PLANE1), ("generic/n126", R.PLANE2)]


@pytest.mark.parametrize("name,form", BEHIND, ids=[f"{n}-{R.FORM_NAMES[f]}" for n, f in BEHIND])
def test_slots_behind_the_rod_change_no_valid_output(probe, name, form):
    """NaN, +-inf and 1e300 in x, v, Q, w behind the rod, or a finite continuation of the rod there: every valid
    output compares equal to the clean run's (the FM law turns its masks into zero factors; sanitize_unused_slots and
    the mass fields' zeros are what keeps those factors zero).  A zero may change its sign."""
    clean = probe.run(name, form)
    for behind in ("poison", "continued"):
        got = probe.contact(CASES[name], form, behind)
        for c, g in zip(clean, got):
            assert np.all(np.isfinite(g)), behind
            assert np.array_equal(c, g), f"{behind}: {int(np.sum(c != g))} values differ"


@pytest.mark.parametrize("name,form", CONTACT, ids=CONTACT_IDS)
def test_a_second_contact_launch_repeats_the_first(probe, name, form):
    for a, b in zip(probe.run(name, form), probe.contact(CASES[name], form)):
        assert np.array_equal(bits(a), bits(b))


# ---- the kinematic step ------------------------------------------------------------------------------------------
VALUE_KIN = ["in_range", "edge", "axis_aligned_and_zero", "quartered", "mixed", "two_slots", "held"]


@pytest.mark.parametrize("name", VALUE_KIN)
def test_kinematic_step_meets_its_budgets(probe, name):
    """Q in absolute ulps per trip count (3 in range, 2 (k + 3) after k quarterings; a mixed wave at the budget of
    the tier it takes; rod_probe_ref.kin_budgets() for the fall-back rule), positions to 1 ulp of the result."""
    case = KIN[name]
    x, Q = probe.run_kin(name)
    ex, eq = R.kin_errors(name, x, Q)
    k, budget = R.kin_trips(case), R.kin_q_budget(case)
    with np.errstate(all="ignore"):
        _, tq = R.kin_errors(name, *R.t_kinematic(case))
    record(block="kinematic_n", case=name, epl=case.epl, unit="ulp (2^-52) absolute; position: of the result",
           device_position=round(float(ex.max()), 3),
           device_by_trips={int(kk): round(float(eq[k == kk].max()), 3) for kk in np.unique(k)},
           transcription_by_trips={int(kk): round(float(tq[k == kk].max()), 3) for kk in np.unique(k)},
           budget_by_trips={int(kk): float(budget[k == kk].max()) for kk in np.unique(k)})
    assert ex.max() <= 1.0, f"position: {ex.max():.3f} ulp"
    over = eq > budget
    assert not over.any(), f"{int(over.sum())} slots over budget, worst {float((eq / budget).max()):.3f} of 1"


@pytest.mark.parametrize("name", ["held"])
def test_held_slots_stay_in_place_bit_for_bit(probe, name):
    """hq = 0: all nine entries of Q; hx = 0: the position — for any w and v, in the blown-up wave too."""
    case = KIN[name]
    x, Q = probe.run_kin(name)
    held_q, held_x = case.hq == 0.0, case.hx == 0.0
    assert np.array_equal(bits(Q[held_q]), bits(case.Q[held_q]))
    assert np.array_equal(bits(x[held_x]), bits(case.x[held_x]))
    assert not np.array_equal(Q[~held_q], case.Q[~held_q]) and not np.array_equal(x[~held_x], case.x[~held_x])


def test_held_identity_directors_and_zero_positions_keep_their_value(probe):
    """The same with exact zeros in what is held (the identity director, a node at the origin): equal as numbers (the
    sum 1 b + 0 b' + 0 b'' may turn a negative zero into a positive one)."""
    src = KIN["held"]
    Q = src.Q.copy()
    x = src.x.copy()
    held_q, held_x = src.hq == 0.0, src.hx == 0.0
    Q[held_q] = np.eye(3).ravel() * np.where(np.arange(held_q.sum()) % 2 == 0, 1.0, -1.0)[:, None]
    x[held_x] = 0.0
    case = R.KinCase("held/zeros", src.epl, src.h, x, src.v, Q, src.w, src.hx, src.hq)
    xo, Qo = probe.kinematic(case)
    assert np.array_equal(Qo[held_q], Q[held_q]) and np.array_equal(xo[held_x], x[held_x])


@pytest.mark.parametrize("name", VALUE_KIN)
def test_one_step_keeps_the_directors_orthogonal(probe, name):
    """max |Q Q^T - I| (largest entry, 2^-52) after the step is no larger than the input's own defect plus the slot's
    budget.  This check found the one defect: without sinc_cosc's ON_CIRCLE correction the defect grew by 25.2 and
    37.6 at k = 9 where 24 is allowed, with every entry inside its budget — the doubling steps grow the pair's
    distance from the unit circle (softrod_fast.hpp)."""
    case = KIN[name]
    _, Q = probe.run_kin(name)
    before, after = R.orthogonality_defect(case.Q), R.orthogonality_defect(Q)
    budget = R.kin_q_budget(case)
    k = R.kin_trips(case)
    worst = float(((after - before) / budget).max())
    record(block="kinematic_n", case=name, check="orthogonality defect", input=round(float(before.max()), 3),
           output=round(float(after.max()), 3), growth_over_budget=round(worst, 3),
           growth_by_trips={int(kk): round(float((after - before)[k == kk].max()), 3) for kk in np.unique(k)},
           budget_by_trips={int(kk): float(budget[k == kk].max()) for kk in np.unique(k)})
    assert np.all(after <= before + budget), f"worst growth {worst:.3f} of the budget"


@pytest.mark.parametrize("name", VALUE_KIN)
def test_a_second_kinematic_launch_repeats_the_first(probe, name):
    for a, b in zip(probe.run_kin(name), probe.kinematic(KIN[name])):
        assert np.array_equal(bits(a), bits(b))


def test_bad_arguments_are_refused(probe):
    lib, torch = probe.lib, probe.torch
    assert lib.softrod_rod_probe_forms() == R.N_FORMS == len(R.FORM_NAMES)
    t = torch.zeros(64 * 2 * 9 + TAIL, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    par = C.cast(Probe.params(CASES["ez/n5"].par), C.c_void_p)
    tilted = C.cast(Probe.params(CASES["tilted/n5"].par), C.c_void_p)
    ok = [p] * 12
    assert lib.softrod_rod_probe_contact(R.N_FORMS, 1, 5, par, *ok, None) == -1
    assert lib.softrod_rod_probe_contact(-1, 1, 5, par, *ok, None) == -1
    assert lib.softrod_rod_probe_contact(R.ZUP1, 0, 5, par, *ok, None) == -1
    assert lib.softrod_rod_probe_contact(R.ZUP1, 1, 0, par, *ok, None) == -1
    assert lib.softrod_rod_probe_contact(R.ZUP1, 1, 64, par, *ok, None) == -1          # 65 nodes in 64 lanes
    assert lib.softrod_rod_probe_contact(R.ZUP2, 1, 128, par, *ok, None) == -1
    assert lib.softrod_rod_probe_contact(R.ZUP1, 1, 5, tilted, *ok, None) == -1        # a z-up form, another normal
    assert lib.softrod_rod_probe_contact(R.ZUP1, 1, 5, None, *ok, None) == -1
    for missing in (0, 5, 10, 11):
        args = list(ok)
        args[missing] = None
        assert lib.softrod_rod_probe_contact(R.ZUP1, 1, 5, par, *args, None) == -1
    args = list(ok)
    args[9] = None                                                                     # r0s: the tapered forms only
    assert lib.softrod_rod_probe_contact(R.ZUP_TAPER1, 1, 5, par, *args, None) == -1
    assert lib.softrod_rod_probe_kinematic(3, 1, 1e-4, *[p] * 8, None) == -1
    assert lib.softrod_rod_probe_kinematic(1, 0, 1e-4, *[p] * 8, None) == -1
    assert lib.softrod_rod_probe_kinematic(1, 1, 1e-4, None, *[p] * 7, None) == -1
    torch.cuda.synchronize()


def test_the_shipped_library_does_not_know_the_probe():
    """Neither probe is a source of libsoftrod_hip.so: the library's source hash is taken over csrc/*.hpp,
    softrod_capi.hip and include/softrod.h."""
    from gym_softrobot_amd import _capi

    csrc = ROOT / "gym_softrobot_amd" / "csrc"
    assert (csrc / "probe" / "softrod_rod_probe.hip").exists()
    assert not list(csrc.glob("*probe*.hpp")) and not list(csrc.glob("*probe*.hip"))
    assert _capi.library_source_hash() == _capi.source_hash()
