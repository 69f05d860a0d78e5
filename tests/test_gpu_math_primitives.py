"""The SOFTROD_MATH_FAST device primitives, one at a time, against mpmath at 50 digits.

variants/libsoftrod_math_probe.so (csrc/probe/softrod_math_probe.hip, `make probe`) runs each primitive element-wise
on plain arrays in blocks of 64 threads: a wave is 64 consecutive inputs.  The cases, references, budgets and the
reasons for them are tests/math_primitives_ref.py's; tests/test_math_primitives.py holds the same budgets on NumPy
transcriptions and shows that they have teeth.  Every case is one launch of at most 4096 values.

Each test prints a line `math-primitive-record: {...}` with the measured maximum (device and transcription side by
side, per trip count where a case has several); profiles/math_primitives_error.json is a copy of those lines.
"""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import math_primitives_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CASES = R.cases()
FORM_NAMES = {R.FAST_RCP: "fast_rcp", R.FAST_RSQRT: "fast_rsqrt", R.SEED_RCP: "rcp_seed", R.SEED_RSQ: "rsq_seed",
              R.SINC_LEAN: "sinc_cosc<true>", R.SINC_PLAIN: "sinc_cosc<false>", R.SERIES6: "series<6>",
              R.SERIES12: "series<12>", R.SERIES20: "series<20>", R.THETA: "theta_over_sin<false>",
              R.THETA_BATCHED: "theta_over_sin<true>", R.EPS_SIN: "eps_sin_factor", R.EXP_PAIR: "exp_pair",
              R.EXP_WIDE: "exp_wide_pair", R.EXP_ONE: "exp_one<1>", R.PLANAR: "planar_kinematic_n<1>"}
SENTINEL = -12345.0


class Probe:
    def __init__(self):
        import torch      # first: the probe must bind to the HIP runtime torch has loaded (gym_softrobot_amd/_capi.py)

        self.torch = torch
        path = ROOT / "variants" / "libsoftrod_math_probe.so"
        if not path.exists():
            subprocess.run(["make", "-C", str(ROOT / "gym_softrobot_amd" / "csrc"), "probe"], check=True)
        self.lib = C.CDLL(str(path))
        self.lib.softrod_math_probe.restype = C.c_int
        self.lib.softrod_math_probe.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
        self.lib.softrod_math_probe_forms.restype = C.c_int
        self.cache = {}

    def launch(self, which, a, b=None, valid=None):
        """One launch -> (out0, out1) as NumPy arrays; the 64 entries behind the n-th must come back untouched."""
        torch = self.torch
        n = len(a)
        dev = torch.device("cuda", 0)
        ta = torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        tb = None if b is None else torch.from_numpy(np.ascontiguousarray(b, np.float64)).to(dev)
        tv = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).to(dev)
        o0 = torch.full((n + R.WAVE,), SENTINEL, dtype=torch.float64, device=dev)
        o1 = torch.full((n + R.WAVE,), SENTINEL, dtype=torch.float64, device=dev)
        rc = self.lib.softrod_math_probe(which, ta.data_ptr(), None if tb is None else tb.data_ptr(),
                                         None if tv is None else tv.data_ptr(), o0.data_ptr(), o1.data_ptr(), n,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"softrod_math_probe({which}) returned {rc}"
        torch.cuda.synchronize()
        o0, o1 = o0.cpu().numpy(), o1.cpu().numpy()
        assert np.all(o0[n:] == SENTINEL) and np.all(o1[n:] == SENTINEL), "the probe wrote behind its output"
        return o0[:n], o1[:n]

    def run(self, name, which):
        """A case through one form, once per module."""
        if (name, which) not in self.cache:
            case = CASES[name]
            self.cache[name, which] = self.launch(which, case.a, case.b, case.valid)
        return self.cache[name, which]


@pytest.fixture(scope="module")
def probe(hip_lib):
    return Probe()


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def record(**kw):
    print("math-primitive-record: " + json.dumps(kw))


def n_outputs(case):
    return len(R.transcribe(case)) if case.assert_values else 2


def per_tier_max(case, err):
    """{tier: max over its waves' checked lanes} for a case whose waves take several trip counts."""
    e = np.where(case.check, err, 0.0).reshape(-1, R.WAVE).max(axis=1)
    return {int(t): float(e[case.tiers == t].max()) for t in np.unique(case.tiers)}


VALUE = [(n, f) for n, c in CASES.items() if c.assert_values for f in c.forms]


@pytest.mark.parametrize("name,which", VALUE, ids=[f"{n}-{FORM_NAMES[f]}" for n, f in VALUE])
def test_device_meets_the_budget(probe, name, which):
    case = CASES[name]
    got = probe.run(name, which)[:n_outputs(case)]
    trans = R.transcribe(case)
    rec = {"case": name, "form": FORM_NAMES[which], "unit": "ulp (2^-52)" + (" absolute" if case.absolute else "")}
    if name == "eps_sin_factor":
        dev, tr = R.eps_sin_excess(case, got[0]), R.eps_sin_excess(case, trans[0])
        raw = R.errors(case, got)[0]
        record(**rec, device=float(dev.max()), transcription=float(tr.max()), device_plain_error=float(raw.max()),
               note="error beyond 2^-22 |ref - 1|; budget 1")
        assert dev.max() <= 1.0
        return
    e_dev, e_tr = R.errors(case, got), R.errors(case, trans)
    if name == "theta_over_sin/near_one":
        d, t = e_dev[0][case.check], e_tr[0][case.check]
        record(**rec, y="1 - 10^-j, j = 1 .. 12", device=[round(float(v), 3) for v in d],
               transcription=[round(float(v), 3) for v in t])
        g = got[0][case.check]
        assert np.all(np.isfinite(g)) and np.all(g > 0.0)
        assert np.all(d <= 100.0 * t), (d, t)
        return
    dev = max(float(e[case.check].max()) for e in e_dev)
    tr = max(float(e[case.check].max()) for e in e_tr)
    rec.update(device=dev, transcription=tr, budget=float(case.budget.max()))
    if case.tiers is not None and len(np.unique(case.tiers)) > 1:
        rec["device_by_trips"] = {k: round(max(per_tier_max(case, e)[k] for e in e_dev), 3)
                                  for k in per_tier_max(case, e_dev[0])}
        rec["transcription_by_trips"] = {k: round(max(per_tier_max(case, e)[k] for e in e_tr), 3)
                                         for k in per_tier_max(case, e_tr[0])}
    if case.bias_budget is not None:
        rec.update(device_edge_bias=R.edge_bias(case, got), transcription_edge_bias=R.edge_bias(case, trans),
                   edge_bias_budget=case.bias_budget)
    record(**rec)
    for e in e_dev:
        over = (e > case.budget) & case.check
        assert not over.any(), (f"{int(over.sum())} values over budget, worst {dev:.3f} ulp at input "
                                f"{case.a[np.argmax(np.where(case.check, e / case.budget, 0.0))]!r}")
    if case.bias_budget is not None:
        assert max(abs(b) for b in rec["device_edge_bias"]) <= case.bias_budget


@pytest.mark.parametrize("name,fn", [("fast_rcp", R.t_fast_rcp), ("fast_rsqrt", R.t_fast_rsqrt)])
def test_refinement_is_the_documented_sequence_on_the_hardware_seed(probe, name, fn):
    """fast_rcp / fast_rsqrt from the device's own seed, in exactly rounded fmas: the same bits as the device."""
    case = CASES[name]
    seed = probe.run(name, case.extra["seed"])[0]
    got = probe.run(name, case.forms[0])[0]
    want = fn(case.a, seed=seed)
    differ = int(np.sum(bits(got) != bits(want)))
    record(case=name, form="refinement of the hardware seed", differing_bit_patterns=differ, of=len(got))
    assert differ == 0


# every polynomial tier and both loops; not the half-angle tier and eps_sin_factor, whose inner 1/sqrt starts from a
# hardware seed the host does not have
BIT_FOR_BIT = ["series6", "series12", "series20", "theta_over_sin/tier1", "theta_over_sin/tier2", "theta_over_sin/tier3",
               "sinc_cosc/in_range", "sinc_cosc/quartered", "exp_pair/tier1", "exp_pair/tier2", "exp_pair/beyond",
               "exp_wide_pair", "exp_one/in_range", "exp_one/halved", "planar_rotation/in_range",
               "planar_rotation/quartered"]


@pytest.mark.parametrize("name", BIT_FOR_BIT)
def test_device_is_the_transcription_in_single_rounding_fmas_bit_for_bit(probe, name):
    """The budgets bound what an error may be; this pins what the operation sequence IS.  The transcription run with
    exactly rounded fmas (rationals) is the device's sequence operation by operation, so the two agree in every bit,
    and a coefficient, a term or an order of operations that changes — below any budget or not — shows.  On the
    case's first 24 waves (its edge values and the top of its tier are there; rationals are slow)."""
    case = CASES[name]
    n = min(len(case.a), 24 * R.WAVE)
    head = R.Case(name, case.forms, case.a[:n], b=None if case.b is None else case.b[:n])
    with R.single_rounding():
        want = R.transcribe(head)
    got = probe.run(name, case.forms[0])
    for k, (g, w) in enumerate(zip(got, want)):
        differ = bits(g[:n]) != bits(w)
        assert not differ.any(), (f"output {k}: {int(differ.sum())} of {n} differ, first at input "
                                  f"{case.a[np.argmax(differ)]!r}: device {g[np.argmax(differ)]!r}, "
                                  f"transcription {w[np.argmax(differ)]!r}")


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if len(c.forms) == 2])
def test_variants_are_bit_identical(probe, name):
    """sinc_cosc<true> == sinc_cosc<false> (horner: "same operation, same rounding") and theta_over_sin<true> ==
    theta_over_sin<false> (the range tests batched or not), on every wave — the non-finite ones included."""
    case = CASES[name]
    first, second = (probe.run(name, f) for f in case.forms)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b)), f"{int(np.sum(bits(a) != bits(b)))} values differ"


ALL = [(n, f) for n, c in CASES.items() for f in c.forms]


@pytest.mark.parametrize("name,which", ALL, ids=[f"{n}-{FORM_NAMES[f]}" for n, f in ALL])
def test_a_second_launch_repeats_the_first(probe, name, which):
    case = CASES[name]
    first = probe.run(name, which)
    second = probe.launch(which, case.a, case.b, case.valid)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b))


def test_non_finite_and_huge_angles_return(probe):
    """t >= 4.3e6 (past the sixteen quarterings), inf and NaN are ordinary data: the launch returns.  Nothing is
    asserted about the values of those waves."""
    case = CASES["sinc_cosc/non_finite"]
    for which in case.forms:
        sc, cc = probe.run(case.name, which)
        assert sc.shape == cc.shape == case.a.shape


POISON = (np.nan, 1.0e300, 0.99)


def _with_invalid_lanes(rng, benign, fill):
    """A copy of `benign` with three lanes of every wave marked invalid and holding `fill` (None: left benign)."""
    v = benign.copy()
    valid = np.ones(len(v), np.uint8)
    for w in range(len(v) // R.WAVE):
        for j, lane in enumerate(rng.choice(R.WAVE, 3, replace=False)):
            valid[w * R.WAVE + lane] = 0
            if fill is not None:
                v[w * R.WAVE + lane] = fill[j]
    return v, valid


@pytest.mark.parametrize("which", [R.THETA, R.THETA_BATCHED, R.EXP_PAIR], ids=lambda f: FORM_NAMES[f])
def test_invalid_lanes_do_not_choose_the_tier(probe, which):
    """NaN, 1e300 and 0.99 in lanes with valid = 0: the valid lanes' outputs are the bits of a run where those lanes
    hold an in-range value."""
    name = "theta_over_sin/tier1" if which != R.EXP_PAIR else "exp_pair/tier1"
    case = CASES[name]
    a, b = case.a[:8 * R.WAVE], None if case.b is None else case.b[:8 * R.WAVE]
    clean_a, valid = _with_invalid_lanes(np.random.default_rng(11), a, None)
    dirty_a, valid2 = _with_invalid_lanes(np.random.default_rng(11), a, POISON)
    assert np.array_equal(valid, valid2) and not np.array_equal(bits(clean_a), bits(dirty_a))
    keep = valid.astype(bool)
    clean = probe.launch(which, clean_a, b, valid)
    dirty = probe.launch(which, dirty_a, b, valid)
    for c, d in zip(clean, dirty):
        assert np.array_equal(bits(c[keep]), bits(d[keep]))
    if which == R.EXP_PAIR:     # the second argument too
        dirty_b, _ = _with_invalid_lanes(np.random.default_rng(11), b, POISON[::-1])
        dirty = probe.launch(which, dirty_a, dirty_b, valid)
        for c, d in zip(clean, dirty):
            assert np.array_equal(bits(c[keep]), bits(d[keep]))
    # the valid lanes are still inside their tier's budget
    ref = R.reference(name)
    for out, r in zip(clean, ref):
        e = R.err_ulps(out, r[:len(out)])
        assert e[keep].max() <= 2.0


def test_unknown_forms_and_missing_arrays_are_refused(probe):
    lib = probe.lib
    assert lib.softrod_math_probe_forms() == R.N_FORMS == len(FORM_NAMES)
    t = probe.torch.zeros(64, dtype=probe.torch.float64, device="cuda")
    assert lib.softrod_math_probe(R.N_FORMS, t.data_ptr(), None, None, t.data_ptr(), None, 64, None) == -1
    assert lib.softrod_math_probe(-1, t.data_ptr(), None, None, t.data_ptr(), None, 64, None) == -1
    assert lib.softrod_math_probe(R.FAST_RCP, None, None, None, t.data_ptr(), None, 64, None) == -1
    assert lib.softrod_math_probe(R.FAST_RCP, t.data_ptr(), None, None, None, None, 64, None) == -1
    assert lib.softrod_math_probe(R.FAST_RCP, t.data_ptr(), None, None, t.data_ptr(), None, 0, None) == 0
    probe.torch.cuda.synchronize()


def test_the_shipped_library_does_not_know_the_probe():
    """The probe is no source of libsoftrod_hip.so: the library's source hash is taken over csrc/*.hpp,
    softrod_capi.hip and include/softrod.h, none of which this suite added or changed."""
    from gym_softrobot_amd import _capi

    csrc = ROOT / "gym_softrobot_amd" / "csrc"
    assert (csrc / "probe" / "softrod_math_probe.hip").exists()
    assert not list(csrc.glob("*probe*.hpp")) and not list(csrc.glob("*probe*.hip"))
    assert _capi.library_source_hash() == _capi.source_hash()
