"""rod_clearance() without a GPU (softrod_rod_clearance, VecRodEnvBase.rod_clearance): the symbol in header, library
source and bindings with the ABI still 17; the argument refusals, which need no device; the known answers of the
yardstick (tests/rod_clearance_ref.py) and its own float64 error against long double on the shared case matrix;
rod_clearance_self_gap; the shells through a stub backend."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi, diagnostics

try:
    from tests import rod_clearance_ref as ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import rod_clearance_ref as ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"
EINVAL = -1
DECLARATION = "int softrod_rod_clearance(softrod_handle* h, int self_gap, double* out, void* stream);"


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


class StubBackend:
    """A backend with a rod_clearance of the device's shapes (zeros): what VecRodEnvBase hands on."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}
        self.self_gaps = []

    def rod_clearance(self, self_gap=None):
        import torch

        self.self_gaps.append(self_gap)
        rods = _capi.config_rods_per_env(self.cfg)
        buf = torch.zeros((self.n_envs, rods, rods + 1, 6), dtype=torch.float64)
        return diagnostics.rod_clearance_views(buf, int(self.cfg.env_kind) in _capi.TARGET_ENVS)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


# ---- 1. the interface --------------------------------------------------------------------------------------------------
def test_symbol_header_and_table(hip_lib):
    header = (ROOT / "include" / "softrod.h").read_text()
    assert DECLARATION in header
    for words in ("[n_envs][rods_per_env][rods_per_env + 1][6]", "THE SEGMENT-SEGMENT RULE", "Ericson", "REST\n * radius",
                  "relative to node 0 of rod a BEFORE any product", "the lowest i wins, then the lowest j",
                  "NaN, NaN, -1, -1, NaN, NaN", "+inf, +inf, -1, -1, 0, 0", "deliberately NOT a body"):
        assert words in header, words
    source = (CSRC / "softrod_capi.hip").read_text()
    assert DECLARATION[:-1] + " {" in source
    assert source.count("case SOFTROD_ENV_REACH:") == 1             # the target switch exists once, for render and clearance
    assert source.count("env_target(h)") == 2
    kernels = (CSRC / "softrod_kernels.hpp").read_text()
    assert kernels.index('#include "softrod_joint_readout.hpp"') < kernels.index('#include "softrod_clearance.hpp"')
    kernel = (CSRC / "softrod_clearance.hpp").read_text()
    assert "#pragma clang fp contract(off)" in kernel and "atomic" not in kernel.replace("No atomics", "")
    assert "float" not in re.sub(r"//.*", "", kernel).replace("<float.h>", "")     # float64 everywhere
    assert "softrod_rod_clearance" in _capi.EXPORTED_SYMBOLS and hasattr(hip_lib, "softrod_rod_clearance")
    assert hip_lib.softrod_rod_clearance.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert _capi.ABI_VERSION == 17 and hip_lib.softrod_abi_version() == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)
    assert gsa.RodClearance is diagnostics.RodClearance


def test_null_arguments_are_refused_before_any_device_is_needed(hip_lib):
    out = (C.c_double * 12)()
    assert hip_lib.softrod_rod_clearance(None, 2, out, None) == EINVAL
    assert hip_lib.softrod_last_error(None) == b"rod clearance: null handle"
    assert hip_lib.softrod_rod_clearance(None, 2, None, None) == EINVAL
    assert hip_lib.softrod_last_error(None).startswith(b"rod clearance:")
    source = re.sub(r'"\s*\n\s*"', "", (CSRC / "softrod_capi.hip").read_text())
    assert set(re.findall(r'"(rod clearance: [^"]*)"', source)) >= set(_capi.ROD_CLEARANCE_ARGUMENT_ERRORS)
    body = source[source.index(DECLARATION[:-1] + " {"):]
    assert body.index("null output buffer") < body.index("self_gap must be") < body.index("SR_ON_DEVICE(h)")


# ---- 2. the yardstick's known answers ---------------------------------------------------------------------------------
L, N_EL, R = 0.2, 10, 0.004
RADII = np.full(N_EL, R)


def test_parallel_rods_and_the_tie_rule():
    D = 0.03
    x = ref.parallel_rods(N_EL, L, D)
    out = ref.clearance(x, RADII, 2)
    got_d = (x[1, 0, 1] - x[0, 0, 1])                                # D as the coordinates hold it
    # every pair (i, i) is exactly D apart, and so are (i, i +- 1) at their shared ends: the lowest i, then the lowest j
    assert out[0, 1].tolist() == [got_d - R - R, got_d, 0.0, 0.0, 0.0, 0.0]
    assert abs(got_d - D) < 1e-15
    # two exactly equal candidates further along win only when the first is taken away
    r2 = RADII.copy()
    r2[0] = 0.5 * R                                                  # pairs with element 0 of either rod are now wider
    out2 = ref.clearance(x, r2, 2)
    assert out2[0, 1][:4].tolist() == [got_d - R - R, got_d, 1.0, 1.0]
    assert out2[0, 1][4] == 0.0 and out2[0, 1][5] == 0.0


def test_mirrored_records():
    x = ref.skew_rods(N_EL, L, 0.005)
    out = ref.clearance(x, np.linspace(0.006, 0.003, N_EL), 2)
    assert np.array_equal(out[1, 0], out[0, 1][[0, 1, 3, 2, 5, 4]])
    assert out[0, 1][2] != out[0, 1][3] or out[0, 1][4] != out[0, 1][5]       # an asymmetric record: the swap shows


def test_skew_perpendicular_rods():
    h = 0.005
    x = ref.skew_rods(N_EL, L, h)
    rec = ref.clearance(x, RADII, 2)[0, 1]
    # rod 1 passes over x = 0.4375 L of rod 0: element 4 at s = 0.375; its own y = 0 is 0.40625 L along: element 4, t = 0.0625
    assert rec[1] == pytest.approx(h, abs=1e-15) and rec[0] == pytest.approx(h - 2 * R, abs=1e-15) and rec[0] < 0
    assert rec[2:4].tolist() == [4.0, 4.0]
    assert rec[4] == pytest.approx(0.375, abs=1e-12) and rec[5] == pytest.approx(0.0625, abs=1e-12)
    crossing = ref.clearance(ref.skew_rods(N_EL, L, 0.0), RADII, 2)[0, 1]
    assert crossing[1] <= ref.BAND_CROSSING * L * 1e-3 and crossing[0] == pytest.approx(-2 * R, abs=1e-12)


def test_target_beyond_the_tip_and_beside_the_middle():
    x = ref.straight(N_EL, L, ref.FAR, (1, 0, 0))[None]
    beyond = ref.FAR + np.array([L + 0.03, 0.04, 0.0])
    rec = ref.clearance(x, RADII, 2, beyond)[0, 1]
    assert rec[2:].tolist() == [N_EL - 1.0, -1.0, 1.0, 0.0]           # the end clamp
    assert rec[1] == pytest.approx(0.05, abs=1e-15) and rec[0] == pytest.approx(0.05 - R, abs=1e-15)
    beside = ref.FAR + np.array([0.45 * L, 0.0, -0.02])
    rec = ref.clearance(x, RADII, 2, beside)[0, 1]
    assert rec[2] == 4.0 and rec[4] == pytest.approx(0.5, abs=1e-12) and rec[1] == pytest.approx(0.02, abs=1e-15)
    before = ref.FAR + np.array([-0.03, 0.0, 0.04])
    assert ref.clearance(x, RADII, 2, before)[0, 1][2:].tolist() == [0.0, -1.0, 0.0, 0.0]
    assert np.array_equal(ref.clearance(x, RADII, 2, None)[0, 1], ref.NO_PAIR)


def test_a_zero_length_element_is_a_point():
    x = ref.parallel_rods(N_EL, L, 0.03)
    x[1, 4] = x[1, 3]                                                 # element 3 of rod 1 has no length
    x[1, 3:5, 1] -= 0.02                                              # ... and is the nearest thing to rod 0
    x[1, 3:5, 0] += 0.25 * L / N_EL
    rec = ref.clearance(x, RADII, 2)[0, 1]
    assert rec[2:4].tolist() == [3.0, 2.0]                            # elements 2 and 4 end on the same point; (3, 2) is first
    assert rec[1] == pytest.approx(0.01, abs=1e-15)
    d, s, t = ref.segments(x[0, 3] - x[0, 0], x[0, 4] - x[0, 3], x[1, 3] - x[0, 0], x[1, 4] - x[1, 3])
    assert (float(d), float(s), float(t)) == (pytest.approx(0.01, abs=1e-15), pytest.approx(0.25, abs=1e-12), 0.0)
    both = ref.segments(np.zeros(3), np.zeros(3), np.array([0.0, 3.0, 4.0]), np.zeros(3))
    assert [float(v) for v in both] == [5.0, 0.0, 0.0]


def test_a_straight_rods_self_record_at_the_default_gap():
    for n, radii in ((10, np.full(10, 0.004)), (20, np.full(20, 0.012)), (40, np.linspace(0.012, 0.002, 40))):
        ell = L / n
        g = _capi.rod_clearance_self_gap(ell, radii)
        x = ref.straight(n, L, ref.FAR, (0.6, 0.0, 0.8))[None]
        rec = ref.clearance(x, radii, g)[0, 0]
        i = int(rec[2])
        assert rec[3] == i + g and rec[4:].tolist() == [1.0, 0.0]     # the end of element i to the start of element i + g
        assert rec[0] == pytest.approx((g - 1) * ell - radii[i] - radii[i + g], abs=1e-15)
        assert rec[0] >= -1e-15                                       # the default: no overlap by construction
        gaps = (g - 1) * ell - radii[:n - g] - radii[g:]
        assert rec[0] == pytest.approx(gaps.min(), abs=1e-15)         # (which of a uniform rod's equal pairs: rounding's)
        if g > 2:                                                     # ... and the first such separation
            assert ((g - 2) * ell - radii[:n - g + 1] - radii[g - 1:]).min() < 0
        # no pair that far apart: the no-pair record
        assert np.array_equal(ref.clearance(x[:, :g + 1], radii[:g], g)[0, 0], ref.NO_PAIR)


def test_the_nan_rule():
    x = np.concatenate([ref.parallel_rods(N_EL, L, 0.03), ref.straight(N_EL, L, ref.FAR + [0, -0.05, 0.01], (1, 0, 0))[None]])
    target = ref.FAR + np.array([0.1, 0.01, 0.0])
    clean = ref.clearance(x, RADII, 2, target)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[1, N_EL, 2] = bad                                           # the LAST node of rod 1
        out = ref.clearance(y, RADII, 2, target)
        for b in range(4):
            assert np.array_equal(out[1, b], ref.NON_FINITE, equal_nan=True)
        for a in (0, 2):
            assert np.array_equal(out[a, 1], ref.NON_FINITE, equal_nan=True)
            for b in (0, 2, 3):
                assert np.array_equal(out[a, b], clean[a, b])
    out = ref.clearance(x, RADII, 2, target * np.array([1.0, np.nan, 1.0]))
    assert np.array_equal(out[:, :3], clean[:, :3])
    for a in range(3):
        assert np.array_equal(out[a, 3], ref.NON_FINITE, equal_nan=True)


def test_the_yardsticks_own_error_is_a_tenth_of_the_band():
    """float64 against long double on the shared case matrix: gap and distance of every record."""
    assert np.finfo(np.longdouble).eps < 1e-18
    for name, x, radii, g, target, length in ref.case_matrix():
        lo = ref.clearance(x, radii, g, target)
        hi = ref.clearance(x, radii, g, target, dtype=np.longdouble)
        fin = np.isfinite(lo[..., 0])
        assert np.array_equal(fin, np.isfinite(hi[..., 0].astype(np.float64))), name
        assert fin.any(), name
        crossing = lo[..., 1] < 1e-3 * length
        # the cases' premise: a winning distance is >= 1e-3 L, or it is the exact crossing (the one case built for it)
        assert not (crossing & fin).any() or (name == "crossing" and (lo[..., 1][crossing & fin] < 1e-12 * length).all()), name
        band = np.where(crossing, ref.BAND_CROSSING, ref.BAND) * length
        err = np.abs((hi[..., :2][fin] - lo[..., :2][fin]).astype(np.float64)).max(axis=-1)
        print(f"{name}: max |float64 - long double| = {err.max() / length:.2e} L")
        assert (err <= 0.1 * band[fin]).all(), (name, err.max())
        crossed = ((0, 1),) if name == "crossing" else ()
        assert ref.compare(lo, lo, x, length, name, target, crossed) <= 1.0   # its own (i, s), (j, t) reproduce its distance


def test_self_gap_values():
    f = _capi.rod_clearance_self_gap
    assert f(0.02, 0.004) == 2 and f(0.02, 0.01) == 2 and f(0.02, 0.0101) == 3 and f(0.01, 0.012) == 4
    assert f(0.2 / 126, np.linspace(0.012, 0.002, 126)) == 1 + 16 and f(1.0, [0.1, 0.6, 0.2]) == 3
    assert isinstance(f(0.02, np.float64(0.004)), int)
    cfg = _capi.octo_flat_config(2)
    assert f(cfg.base_length / cfg.n_elem, cfg.base_radius) >= 2


# ---- 3. the shells ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,n,rods,target", [("SoftPendulum-v0", 3, 1, False), ("OctoArmTwo-v0", 2, 2, True),
                                                  ("OctoFlat-v0", 2, 8, True), ("OctoArmSingle-v0", 2, 1, True),
                                                  ("OctoArmPush-v1", 2, 1, False)])
def test_shapes_and_numpy_output(env_id, n, rods, target):
    fields = ("gap", "distance", "element", "point", "target_gap", "target_distance", "target_element", "target_point")
    for kw, kind in (({}, None), (dict(numpy_output=True), np.ndarray)):
        env = _vec(env_id, n, StubBackend, **kw)
        out = env.rod_clearance(self_gap=3)
        assert env.backend.self_gaps == [3]
        assert type(out) is gsa.RodClearance and out._fields == fields
        assert tuple(out.gap.shape) == tuple(out.distance.shape) == (n, rods, rods)
        assert tuple(out.element.shape) == tuple(out.point.shape) == (n, rods, rods, 2)
        for t in out[4:]:
            assert (t is None) if not target else tuple(t.shape) == (n, rods)
        assert kind is None or all(isinstance(t, kind) for t in out if t is not None)


def test_views_share_the_one_buffer():
    buf = np.arange(2 * 3 * 4 * 6, dtype=np.float64).reshape(2, 3, 4, 6)
    v = diagnostics.rod_clearance_views(buf)
    for t in v:
        assert t.base is not None and np.shares_memory(t, buf)
    assert v.gap[1, 2, 0] == buf[1, 2, 0, 0] and v.distance[1, 2, 0] == buf[1, 2, 0, 1]
    assert v.element[1, 2, 0].tolist() == buf[1, 2, 0, 2:4].tolist() and v.point[1, 2, 0].tolist() == buf[1, 2, 0, 4:6].tolist()
    assert (v.target_gap[1, 2], v.target_distance[1, 2], v.target_element[1, 2], v.target_point[1, 2]) == \
        (buf[1, 2, 3, 0], buf[1, 2, 3, 1], buf[1, 2, 3, 2], buf[1, 2, 3, 4])
    assert diagnostics.rod_clearance_views(buf, has_target=False)[4:] == (None,) * 4


def test_single_env_shell_drops_the_env_axis():
    from gym_softrobot_amd.envs.octo_flat import FlatEnv
    from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

    for cls, rods, target in ((SoftPendulumEnv, 1, False), (FlatEnv, 8, True)):
        probe = cls(backend=_Probe())
        out = cls(backend=StubBackend(probe._vec.cfg)).rod_clearance()
        assert isinstance(out.gap, np.ndarray) and out.gap.shape == (rods, rods) and out.point.shape == (rods, rods, 2)
        assert (out.target_gap is None) if not target else out.target_gap.shape == (rods,)


def test_oracle_backend_has_no_rod_clearance(oracle_built):
    env = _vec("SoftPendulum-v0", 2, OracleBackend)
    with pytest.raises(NotImplementedError, match="rod clearance needs the HIP backend, not OracleBackend"):
        env.rod_clearance()
