"""One force evaluation and rate update of the FAST step kernels alone on the device, against 50 digits.

variants/libsoftrod_dyn_probe.so (csrc/probe/softrod_dyn_probe.hip, `make probe`) runs one dynamic_n call in six
instantiations the step table ships (<kRuntimeFeatures> and <kArmSingleZup>, one and two slots per lane, tapered) and one
planar_dynamic_n<1> / <2>, one rod per wave on plain arrays, with ConstN / PlanarC from the shipped build_const /
planar_build_const.  The crafted rods, the references L and P, the budgets and the reasons for them are
tests/dyn_probe_ref.py's; tests/test_dyn_probe.py shows on the CPU that the budgets come from the reference side, that no
output is excused, that P is L inside the header's bounds and that fifteen mutations leave the budgets.  Every case is one
launch of at most 16 waves.

Each value test prints a line `dyn-probe-record: {...}` with the device's maximum, the baseline and the budget;
profiles/dyn_probe_error.json is a copy of those lines.
"""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import dyn_probe_ref as D

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CASES = D.dyn_cases()
PLANAR = D.planar_cases()
SENTINEL = -12345.0
TAIL = 64
DYN_IN = ("x", "v", "Q", "w", "rk")
PLANAR_IN = ("x", "v", "c", "s", "wz", "dl", "d", "dv")


class Probe:
    def __init__(self):
        import torch      # first: the probe must bind to the HIP runtime torch has loaded (gym_softrobot_amd/_capi.py)

        self.torch = torch
        path = ROOT / "variants" / "libsoftrod_dyn_probe.so"
        if not path.exists():
            subprocess.run(["make", "-C", str(ROOT / "gym_softrobot_amd" / "csrc"), "probe"], check=True)
        self.lib = C.CDLL(str(path))
        self.lib.softrod_dyn_probe_dynamic.restype = C.c_int
        self.lib.softrod_dyn_probe_dynamic.argtypes = [C.c_int] * 3 + [C.c_void_p] * 12
        self.lib.softrod_dyn_probe_planar.restype = C.c_int
        self.lib.softrod_dyn_probe_planar.argtypes = [C.c_int] * 3 + [C.c_void_p] * 9 + [C.c_double] + [C.c_void_p] * 5
        self.lib.softrod_dyn_probe_forms.restype = C.c_int
        self.lib.softrod_dyn_probe_params.restype = C.c_int
        self.cache = {}

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda")

    def out(self, n):
        return self.torch.full((n + TAIL,), SENTINEL, dtype=self.torch.float64, device="cuda")

    @staticmethod
    def params(mat, features=None):
        m = mat if features is None else D.with_features(mat, features)
        return (C.c_double * D.N_PARAMS)(*D.params(m))

    def _collect(self, outs, rods, W, valid):
        """outs: {name: (tensor, components)} -> {name: (rods, valid[name], components)}; sentinels behind the arrays and
        behind every rod must be intact."""
        self.torch.cuda.synchronize()
        res = {}
        for k, (t, c) in outs.items():
            a = t.cpu().numpy()
            assert np.all(a[-TAIL:] == SENTINEL), f"the probe wrote behind {k}"
            a = a[:-TAIL].reshape(rods, W, c)
            assert np.all(a[:, valid[k]:] == SENTINEL), f"{k}: a slot behind the rod was stored"
            res[k] = a[:, :valid[k]].copy()
        return res

    def dynamic(self, case, form, mask, behind="clean"):
        """One launch -> {v (rods, n + 1, 3), w, t (rods, n, 3), kap (rods, n - 1, 3)}."""
        epl, n, rods = D.FORM_EPL[form], case.n, len(case.rods)
        W = D.WAVE * epl
        a = D.dyn_layout(case, epl, behind)
        t = {k: self.dev(v) for k, v in a.items()}
        mat = self.dev(D.material_table(case.mat, epl)) if D.FORM_TAPER[form] else None
        outs = {k: (self.out(rods * W * 3), 3) for k in D.OUTPUTS}
        rc = self.lib.softrod_dyn_probe_dynamic(
            form, rods, n, C.cast(self.params(case.mat, D.mask_features(mask)), C.c_void_p),
            *(t[k].data_ptr() for k in DYN_IN), mat.data_ptr() if mat is not None else None,
            *(outs[k][0].data_ptr() for k in D.OUTPUTS), self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"softrod_dyn_probe_dynamic({form}) returned {rc}"
        return self._collect(outs, rods, W, {"v": n + 1, "w": n, "t": n, "kap": n - 1})

    def run(self, name, form, mask):
        key = (name, form, mask)
        if key not in self.cache:
            self.cache[key] = self.dynamic(CASES[name], form, mask)
        return self.cache[key]

    def planar(self, case, behind="clean"):
        """One launch -> {v (rods, n + 1, 2), wz (rods, n, 1), t, dv (rods, n, 2)}."""
        n, rods = case.n, len(case.rods)
        W = D.WAVE * case.epl
        a = D.planar_layout(case, behind)
        t = {k: self.dev(v) for k, v in a.items()}
        outs = {k: (self.out(rods * W * c), c) for k, c in zip(D.PLANAR_OUTPUTS, (2, 1, 2, 2))}
        rc = self.lib.softrod_dyn_probe_planar(
            case.epl, rods, n, C.cast(self.params(case.mat), C.c_void_p), *(t[k].data_ptr() for k in PLANAR_IN),
            case.s2, *(outs[k][0].data_ptr() for k in D.PLANAR_OUTPUTS), self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"softrod_dyn_probe_planar({case.epl}) returned {rc}"
        return self._collect(outs, rods, W, {"v": n + 1, "wz": n, "t": n, "dv": n})

    def run_planar(self, name):
        if name not in self.cache:
            self.cache[name] = self.planar(PLANAR[name])
        return self.cache[name]


@pytest.fixture(scope="module")
def probe(hip_lib):
    return Probe()


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def record(**kw):
    print("dyn-probe-record: " + json.dumps(kw))


def device_errors(name, mask, got):
    """{output: (rods, slots)} errors of one launch, in budget units."""
    case = CASES[name]
    errs = {k: [] for k in D.OUTPUTS}
    for r, (rod, (ref, scales)) in enumerate(zip(case.rods, D.dyn_reference(name, mask))):
        for k, e in D.dyn_errors(rod, ref, scales, {k: got[k][r] for k in D.OUTPUTS}).items():
            errs[k].append(e)
    return {k: np.array(v) for k, v in errs.items()}


def planar_device_errors(name, got):
    errs = {k: [] for k in D.PLANAR_OUTPUTS}
    for r, (ref, scales) in enumerate(D.planar_reference(name)):
        for k, e in D.planar_errors(ref, scales, {k: got[k][r] for k in D.PLANAR_OUTPUTS}).items():
            errs[k].append(e)
    return {k: np.array(v) for k, v in errs.items()}


def _held(errs, budget, what):
    for k, e in errs.items():
        if e.size:
            r, s = np.unravel_index(np.argmax(e), e.shape)
            assert e.max() <= budget[k]["budget"], f"{what}: {k}: {e.max():.3f} of {budget[k]['budget']:.3f} at rod {r} slot {s}"


def _summary(errs, budget):
    return {k: {"device": round(float(e.max()), 3) if e.size else 0.0, "baseline": round(budget[k]["baseline"], 3),
                "budget": round(budget[k]["budget"], 3)} for k, e in errs.items()}


DYN = [(n, f, m) for n, c in CASES.items() for f, m in D.case_forms(c)]
DYN_IDS = [f"{n}-{D.FORM_NAMES[f]}-{m}" for n, f, m in DYN]


@pytest.mark.parametrize("name,form,mask", DYN, ids=DYN_IDS)
def test_dynamic_n_meets_its_budget(probe, name, form, mask):
    """Every node, element and vertex of every rod: none is excused.  4 x the case's baseline (floor 8) in units of 2^-52 x
    the reference side's scale, for v, w, t and kap each."""
    budget = D.dyn_budget(name, mask)
    errs = device_errors(name, mask, probe.run(name, form, mask))
    record(block="dynamic_n", case=name, form=D.FORM_NAMES[form], mask=mask, unit="2^-52 x scale", **_summary(errs, budget))
    _held(errs, budget, f"{name} {D.FORM_NAMES[form]} {mask}")


def _distance(name, mask, a, b):
    """Largest difference of two launches' outputs, in units of the budget."""
    case, budget = CASES[name], D.dyn_budget(name, mask)
    worst = 0.0
    for r, (rod, (ref, scales)) in enumerate(zip(case.rods, D.dyn_reference(name, mask))):
        for k, s in zip(D.OUTPUTS, scales):
            if len(s):
                d = np.abs(a[k][r] - b[k][r]).max(axis=-1) / (D.ULP * s)
                worst = max(worst, float(d.max()) / budget[k]["budget"])
    return worst


PAIRS = [(n, m, fa, fb) for n, c in CASES.items() for m in D.case_masks(c)
         for fa, fb in ((D.RT1, D.RT2), (D.ARM1, D.ARM2)) if {(fa, m), (fb, m)} <= set(D.case_forms(c))]


@pytest.mark.parametrize("name,mask,one,two", PAIRS, ids=[f"{n}-{m}-{D.FORM_NAMES[a]}" for n, m, a, _ in PAIRS])
def test_one_and_two_slots_per_lane(probe, name, mask, one, two):
    budget = D.dyn_budget(name, mask)
    a, b = probe.run(name, one, mask), probe.run(name, two, mask)
    record(case=name, mask=mask, check="EPL 1 against EPL 2", form=D.FORM_NAMES[one],
           difference_over_budget=round(_distance(name, mask, a, b), 5))
    _held(device_errors(name, mask, a), budget, "one slot")
    _held(device_errors(name, mask, b), budget, "two slots")


LIFTED = [(n, [f for f, _ in D.case_forms(c)]) for n, c in CASES.items() if c.lifted]


@pytest.mark.parametrize("name,forms", LIFTED, ids=[n for n, _ in LIFTED])
def test_run_time_and_compiled_arm_mask_on_the_lifted_rod(probe, name, forms):
    """<kRuntimeFeatures> with the arm benchmark's mask at run time against <kArmSingleZup>: the contact operator runs
    in both and adds nothing 1 m above the plane."""
    budget = D.dyn_budget(name, "arm")
    rt, arm = forms[-1], forms[0]
    a, b = probe.run(name, rt, "arm"), probe.run(name, arm, "arm")
    record(case=name, check="run-time against compiled arm mask", forms=[D.FORM_NAMES[rt], D.FORM_NAMES[arm]],
           difference_over_budget=round(_distance(name, "arm", a, b), 5))
    _held(device_errors(name, "arm", a), budget, "run-time mask")
    _held(device_errors(name, "arm", b), budget, "compiled mask")


@pytest.mark.parametrize("name", list(PLANAR))
def test_planar_dynamic_n_meets_its_budget(probe, name):
    """Against P at 50 digits: v, wz, t, dv of every node and element.  A case outside exp_one's polynomial range gets
    exp_one's recorded error at its trip count on top (profiles/math_primitives_error.json)."""
    budget = D.planar_budget(name)
    errs = planar_device_errors(name, probe.run_planar(name))
    record(block="planar_dynamic_n", case=name, epl=PLANAR[name].epl, exp_one_halvings=PLANAR[name].halvings,
           unit="2^-52 x scale", **_summary(errs, budget))
    _held(errs, budget, name)


@pytest.mark.parametrize("pname", D.FROM_PLANAR)
def test_the_same_planar_state_through_both_substeps(probe, pname):
    """planar_dynamic_n against P, dynamic_n<kRuntimeFeatures> (SoftPendulum's mask less its BC) against L, on the same
    state: both inside their budgets; their distance is recorded (node 0's pinned v_y apart)."""
    name, case = "from-" + pname, CASES["from-" + pname]
    form = D.RT1 if case.epl == 1 else D.RT2
    three, two = probe.run(name, form, "pendulum"), probe.run_planar(pname)
    _held(device_errors(name, "pendulum", three), D.dyn_budget(name, "pendulum"), "3-D")
    _held(planar_device_errors(pname, two), D.planar_budget(pname), "planar")
    s2, worst = PLANAR[pname].s2, 0.0
    for r, (_, scales) in enumerate(D.planar_reference(pname)):
        dv = np.abs(three["v"][r][:, :2] - two["v"][r]) / (D.ULP * scales[0][:, None])
        dv[0, 1] = 0.0
        dw = np.abs(s2 * three["w"][r][:, 1] - two["wz"][r][:, 0]) / (D.ULP * scales[1])
        dt = np.abs(three["t"][r][:, :2] - two["t"][r]) / D.ULP
        worst = max(worst, float(dv.max()), float(dw.max()), float(dt.max()))
        assert np.all(three["v"][r][:, 2] == 0.0) and np.all(three["w"][r][:, [0, 2]] == 0.0)      # exact zeros stay
    record(case=pname, check="planar_dynamic_n against dynamic_n on the same state", unit="2^-52 x P's scale",
           distance=round(worst, 3))


BEHIND = [("epl1/n2/walk", D.RT1, "damper+rest_kappa"), ("epl1/n5/walk", D.RT1, "damper+gravity"),
          ("epl1/n5/walk", D.RT2, "damper"), ("epl1/n63/walk", D.RT1, "damper+rest_kappa"),
          ("epl2/n101/walk", D.RT2, "damper+rest_kappa"), ("epl2/n126/walk", D.RT2, "damper"),
          ("epl2/n127/walk", D.RT2, "damper+rest_kappa"), ("taper/n5/walk", D.RT_TAPER1, "damper+rest_kappa"),
          ("taper/n63/hot", D.RT_TAPER1, "damper"), ("epl1/n5/walk/lifted", D.ARM1, "arm"),
          ("epl1/n63/dragged/lifted", D.ARM1, "arm"), ("epl2/n127/hot/lifted", D.ARM2, "arm"),
          ("taper/n63/walk/lifted", D.ARM_TAPER1, "arm")]


@pytest.mark.parametrize("name,form,mask", BEHIND, ids=[f"{n}-{D.FORM_NAMES[f]}-{m}" for n, f, m in BEHIND])
def test_slots_behind_the_rod_change_no_valid_output(probe, name, form, mask):
    """NaN, +-inf and +-1e300 in x, v (past node n) and Q, w, rk (past element n - 1), or a finite continuation of the rod
    there (rk from vertex slot n - 1): every valid output has the clean run's bits (sanitize_unused_slots and the zero stiffnesses behind the rod
    are what keeps them out), and no slot behind the rod is stored (Probe._collect)."""
    clean = probe.run(name, form, mask)
    for behind in ("poison", "continued"):
        got = probe.dynamic(CASES[name], form, mask, behind)
        for k in D.OUTPUTS:
            assert np.all(np.isfinite(got[k])), f"{behind}: {k} is not finite"
            assert np.array_equal(bits(clean[k]), bits(got[k])), f"{behind}: {int(np.sum(clean[k] != got[k]))} {k} differ"


PLANAR_BEHIND = ["planar1/n2/walk/s2+", "planar1/n5/walk/s2-", "planar1/n63/walk/s2+", "planar2/n64/walk/s2-",
                 "planar2/n127/hot/s2+"]


@pytest.mark.parametrize("name", PLANAR_BEHIND)
def test_slots_behind_the_planar_rod_change_no_valid_output(probe, name):
    """The same for planar_dynamic_n behind planar_sanitize_unused, the shipped kernel's own way into the loop
    (planar_from_lane calls it): NaN, +-inf, +-1e300 or a finite continuation in x, v past node n, in c, s, wz, d, dv past
    element n - 1 and in dl past vertex n - 2 leave every valid output's bits alone.  Before that helper existed a NaN or inf
    in (c, s) of the slot behind the last element came out as a NaN velocity of the tip node."""
    clean = probe.run_planar(name)
    for behind in ("poison", "continued"):
        got = probe.planar(PLANAR[name], behind)
        for k in D.PLANAR_OUTPUTS:
            assert np.all(np.isfinite(got[k])), f"{behind}: {k} is not finite"
            assert np.array_equal(bits(clean[k]), bits(got[k])), f"{behind}: {int(np.sum(clean[k] != got[k]))} {k} differ"


@pytest.mark.parametrize("n_elem", [5, 63, 70])
def test_garbage_behind_the_rod_changes_no_softpendulum_step(hip_lib, n_elem):
    """The whole step kernel, which forms d and dv behind the rod itself (planar_from_lane): NaN, +-inf, +-1e300 written
    through softrod_state_view into the slots behind the rod (position, velocity past node n; director, omega past element
    n - 1) change no output of two env.steps and no valid slot of the state.  5 and 63 elements at one slot per lane (63
    fills the wave: only the element slot is behind the rod), 70 at two."""
    import torch

    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    n_envs = 4
    theta = np.linspace(-0.4, 0.5, n_envs)
    pair = [HipRodBackend(_capi.softpendulum_config(n_envs, n_elems=n_elem)) for _ in range(2)]
    rng = np.random.default_rng(11)
    bad = np.array([np.nan, np.inf, -np.inf, 1.0e300, -1.0e300])
    states = []
    for be in pair:
        be.reset(theta)
        states.append(be.state())            # (both handles: views switch the planar certificates off)
    dirty = states[1]
    for row, first in (("position", n_elem + 1), ("velocity", n_elem + 1), ("director", n_elem), ("omega", n_elem)):
        t = dirty[row]
        fill = rng.choice(bad, tuple(t[:, :, first:].shape))
        t[:, :, first:] = torch.from_numpy(fill).to(t.device)
    actions = rng.uniform(-22.0, 22.0, (2, n_envs)).astype(np.float32)
    for a in actions:
        outs = []
        for be in pair:
            be.step(a)
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy().tobytes() for x in (be.obs, be.reward, be.terminated, be.truncated)])
        assert outs[0] == outs[1]
    for row, valid in (("position", n_elem + 1), ("velocity", n_elem + 1), ("director", n_elem), ("omega", n_elem),
                       ("tangents", n_elem)):
        a, b = (st[row][:, :, :valid].cpu().numpy() for st in states)
        assert np.all(np.isfinite(a)) and np.array_equal(bits(a), bits(b)), row
    for be in pair:
        be.close()


@pytest.mark.parametrize("name,form,mask", BEHIND, ids=[f"{n}-{D.FORM_NAMES[f]}-{m}" for n, f, m in BEHIND])
def test_a_second_launch_repeats_the_first(probe, name, form, mask):
    first, again = probe.run(name, form, mask), probe.dynamic(CASES[name], form, mask)
    for k in D.OUTPUTS:
        assert np.array_equal(bits(first[k]), bits(again[k]))


@pytest.mark.parametrize("name", PLANAR_BEHIND + ["planar1/n5/damped"])
def test_a_second_planar_launch_repeats_the_first(probe, name):
    first, again = probe.run_planar(name), probe.planar(PLANAR[name])
    for k in D.PLANAR_OUTPUTS:
        assert np.array_equal(bits(first[k]), bits(again[k]))


def test_bad_arguments_are_refused_and_store_nothing(probe):
    lib, torch = probe.lib, probe.torch
    assert lib.softrod_dyn_probe_forms() == D.N_FORMS == len(D.FORM_NAMES)
    assert lib.softrod_dyn_probe_params() == D.N_PARAMS
    t = torch.full((1025 * 128 * 9 + TAIL,), SENTINEL, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    par = C.cast(Probe.params(CASES["epl1/n5/walk"].mat), C.c_void_p)
    good = dict(form=D.RT1, n_rods=1, n_elem=5, par=par, x=p, v=p, Q=p, w=p, rk=p, mat=p, v_out=p, w_out=p, t_out=p,
                kap_out=p)
    for what, change in D.BAD_DYNAMIC:
        a = {**good, **change}
        assert lib.softrod_dyn_probe_dynamic(*a.values(), None) == -1, what
    tilted = D.with_features(CASES["epl1/n5/walk"].mat, D.ARM_SINGLE)
    tilted.contact = D.R._par(D.R.TILTED, D.R.MU_OCTOPUS)
    a = {**good, "form": D.ARM1, "par": C.cast(Probe.params(tilted), C.c_void_p)}
    assert lib.softrod_dyn_probe_dynamic(*a.values(), None) == -1, "a z-up form with another normal"
    good = dict(epl=1, n_rods=1, n_elem=5, par=par, x=p, v=p, c=p, s=p, wz=p, dl=p, d=p, dv=p, s2=1.0, v_out=p, wz_out=p,
                t_out=p, dv_out=p)
    for what, change in D.BAD_PLANAR:
        a = {**good, **change}
        assert lib.softrod_dyn_probe_planar(*a.values(), None) == -1, what
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all()), "a refused call stored something"


def test_the_shipped_library_does_not_know_the_probe():
    """The probe is no source of libsoftrod_hip.so: the library's source hash is taken over csrc/*.hpp,
    softrod_capi.hip and include/softrod.h."""
    from gym_softrobot_amd import _capi

    csrc = ROOT / "gym_softrobot_amd" / "csrc"
    assert (csrc / "probe" / "softrod_dyn_probe.hip").exists()
    assert not list(csrc.glob("*probe*.hpp")) and not list(csrc.glob("*probe*.hip"))
    assert _capi.library_source_hash() == _capi.source_hash()
