"""joint_loads() without a GPU (softrod_joint_loads, VecRodEnvBase.joint_loads, diagnostics.joint_loads_host): the symbol
in header, library source and bindings; the NumPy twin against the EXECUTED reference (the 24 vectors of
tests/golden/octo_operator_vectors.npz, outputs of the reference's own FixedJoint2Rigid) and against
oracle/softrod_oracle_np.py's fixed_joint_to_rigid / NumpyCylinder applied arm by arm; known answers; the calibration of
the band tests/test_gpu_joint_loads.py holds the device to; the shells; the new kernel's scratch and LDS."""
import copy
import functools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi, diagnostics
from gym_softrobot_amd.diagnostics import JointLoads
from oracle.softrod_oracle_np import fixed_joint_to_rigid

try:
    from tests import joint_loads_ref as ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import joint_loads_ref as ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"
GOLD = ROOT / "tests" / "golden"
EPS = 2.0 ** -52
FIELDS = ("body_force", "body_torque", "arm_force", "arm_torque", "gap", "gap_length", "net_force", "net_torque",
          "acceleration", "angular_acceleration")


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


class StubBackend:
    """A backend with a joint_loads of the device's shapes (zeros): what VecRodEnvBase hands on."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}

    def joint_loads(self):
        import torch

        buf = torch.zeros((self.n_envs, _capi.config_rods_per_env(self.cfg) + 1, 16), dtype=torch.float64)
        return diagnostics.joint_loads_views(buf)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


@functools.lru_cache(maxsize=None)
def _oracle(n_arm):
    """(cfg, states, the NumpyOctopus after its last substep) of one CPU case, computed once."""
    return ref.oracle_octopus(n_arm)


def _octopus_at(n_arm, st):
    """A copy of the case's NumpyOctopus holding state `st`, external loads zeroed."""
    oc = copy.deepcopy(_oracle(n_arm)[2])
    for a, rod in enumerate(oc.arms):
        rod.x, rod.v, rod.Q = st["x"][a].copy(), st["v"][a].copy(), st["Q"][a].copy()
        rod.zero_external()
    h = oc.head
    h.x, h.v, h.w = (np.array(st[k], np.float64).reshape(3, 1) for k in ("head_x", "head_v", "head_w"))
    h.Q = np.array(st["head_Q"], np.float64).reshape(3, 3, 1)
    h.zero_external()
    return oc


# ---- 0. header, library and bindings agree ---------------------------------------------------------------------------
def test_symbol_in_header_library_and_bindings():
    header = (ROOT / "include" / "softrod.h").read_text()
    assert "int softrod_joint_loads(softrod_handle* h, double* out, void* stream);" in header
    assert "joint.py:47-219" in header and "NOT the value the last substep applied" in header
    assert "gyroscopic term" in header and "vanishes identically" in header
    source = (CSRC / "softrod_capi.hip").read_text()
    assert "int softrod_joint_loads(softrod_handle* h, double* out, void* stream) {" in source
    assert set(re.findall(r'"(joint loads: [^"]*)"', source)) == {
        "joint loads: null handle", "joint loads: null output buffer", "joint loads: this handle has no rigid body"}
    kernel = (CSRC / "softrod_joint_readout.hpp").read_text()
    assert "kJointCols = 16" in kernel and "#pragma clang fp contract(off)" in kernel
    assert "const JointLoad J = joint_load_literal(P, H, arm, x0, v0, x1);" in kernel      # force, torque AND gap from one call
    assert "o[12 + c] = J.gap[c];" in kernel and "o[15] = J.dist;" in kernel and "sqrt(" not in kernel
    assert "__shared__" not in kernel and "atomic" not in kernel.replace("no atomics", "")
    assert "softrod_joint_loads" in _capi.EXPORTED_SYMBOLS
    assert _capi._EXPORTS["softrod_joint_loads"] == _capi._EXPORTS["softrod_rod_energies"]
    assert _capi.ABI_VERSION == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)
    for cfg in (_capi.softpendulum_config(2), _capi.arm_single_config(2), _capi.arm_push_config(2)):
        assert _capi.joint_loads_refusal(cfg) == "joint loads: this handle has no rigid body"
    for cfg in (_capi.octo_flat_config(2), _capi.arm_pull_weight_config(2), _capi.muscle_octopus_config(_capi.ENV_CRAWL, 2)):
        assert _capi.joint_loads_refusal(cfg) is None


# ---- 1. the twin against the executed reference ------------------------------------------------------------------------
def test_twin_reproduces_the_references_own_joint():
    """All 24 vectors of the reference's own FixedJoint2Rigid, at the tolerances tests/test_oracle_golden.py holds the C
    oracle to on the same file: forces rtol 1e-10, atol 1e-10 max(|f|max, k 1e-5); torques rtol 1e-10, atol 1e-16."""
    z = np.load(GOLD / "octo_operator_vectors.npz")
    k = float(z["joint_params"][0])
    cases = ref.golden_cases(z)
    assert len(cases) == 24
    for c, (cfg, st) in enumerate(cases):
        assert float(cfg.base_length) / int(cfg.n_elem) == pytest.approx(float(z["joint_rest_len"][c]), rel=1e-15)
        r = ref.twin(cfg, st)
        scale_f = max(np.abs(z["joint_head_f"][c]).max(), k * 1e-5)
        np.testing.assert_allclose(r.body_force[0], z["joint_head_f"][c], rtol=1e-10, atol=1e-10 * scale_f)
        np.testing.assert_allclose(r.arm_force[0], z["joint_arm_f"][c], rtol=1e-10, atol=1e-10 * scale_f)
        np.testing.assert_allclose(r.body_torque[0], z["joint_head_t"][c], rtol=1e-10, atol=1e-16)
        np.testing.assert_allclose(r.arm_torque[0], z["joint_arm_t"][c], rtol=1e-10, atol=1e-16)
        np.testing.assert_array_equal(r.net_force, r.body_force[0])        # one arm: the net row is its row
        np.testing.assert_array_equal(r.net_torque, r.body_torque[0])
    assert max(np.abs(z["joint_head_t"]).max(), np.abs(z["joint_head_f"]).max()) > 0


# ---- 2. the twin against fixed_joint_to_rigid applied arm by arm on a NumpyOctopus ------------------------------------
@pytest.mark.parametrize("case", ref.CPU_CASES, ids=lambda c: c[0])
def test_twin_equals_the_oracle_arm_by_arm(case):
    """States of a few oracle substeps under random actions.  BITWISE: body_force, arm_force, arm_torque, net_force, and
    body_torque against the oracle's own lab-frame torque taken through joint.py's loop (external_torques[i] -=
    Q[i, j] * torque[j]); net_torque is then bitwise the left-to-right sum of those rows.  The oracle's lab-frame torque
    is read from a copy of the arm whose element 0 has the identity for its directors (I @ torque is exact).
    NOT BITWISE, and reported apart: the oracle's head row as it forms it, head.Q @ torque with NumPy's matrix-vector
    product.  Wherever that differs from the loop it equals the same sum with one product fused into it (checked in
    exact rational arithmetic), so it is within one ulp of the largest product; the count of such entries is printed."""
    n_arm = case[1]
    cfg, states, _ = _oracle(n_arm)
    assert ref.joint_angles(cfg).tolist() == [360 / n_arm * a for a in range(n_arm)]
    moving = fused = 0
    for st in states:
        r = ref.twin(cfg, st)
        oc, one, probe = (_octopus_at(n_arm, st) for _ in range(3))
        h = oc.head                                        # gathers every arm's load, as the oracle's substep does
        net_ulp, net_loop = np.zeros(3), np.zeros(3)
        joint = (cfg.joint_k, cfg.joint_nu, cfg.joint_kt)
        for a, rod in enumerate(oc.arms):
            fixed_joint_to_rigid(h, rod, *joint, oc.angles[a], cfg.head_radius)
            np.testing.assert_array_equal(rod.f_ext[:, 0], r.arm_force[a])
            np.testing.assert_array_equal(rod.t_ext[:, 0], r.arm_torque[a])
            assert not rod.f_ext[:, 1:].any() and not rod.t_ext[:, 1:].any()
            one.head.zero_external()                       # this arm's load alone, added to zero: the row itself
            fixed_joint_to_rigid(one.head, one.arms[a], *joint, oc.angles[a], cfg.head_radius)
            np.testing.assert_array_equal(one.head.f_ext[:, 0], r.body_force[a])
            probe.arms[a].Q[:, :, 0] = np.eye(3)           # the oracle's own lab-frame torque: I @ torque
            fixed_joint_to_rigid(probe.head, probe.arms[a], *joint, oc.angles[a], cfg.head_radius)
            tau = probe.arms[a].t_ext[:, 0].copy()
            Qh, loop = h.Q[:, :, 0], np.zeros(3)
            for i in range(3):
                for j in range(3):
                    loop[i] -= Qh[i, j] * tau[j]           # joint.py:212-216
            assert loop.tobytes() == r.body_torque[a].tobytes()
            net_loop = net_loop + loop
            matvec = one.head.t_ext[:, 0]
            ulp = np.spacing(np.abs(Qh * tau[None, :]).max(axis=1))
            for i in range(3):
                if matvec[i] != loop[i]:
                    fused += 1
                    assert -matvec[i] in _fused_sums(Qh[i], tau), (a, i)
                    assert abs(matvec[i] - loop[i]) <= ulp[i]
            net_ulp += ulp
        assert net_loop.tobytes() == r.net_torque.tobytes()
        np.testing.assert_array_equal(h.f_ext[:, 0], r.net_force)
        assert (np.abs(h.t_ext[:, 0] - r.net_torque) <= net_ulp).all(), (h.t_ext[:, 0] - r.net_torque, net_ulp)

        # the body's rates: NumpyCylinder.dynamic then constrain_rates, from the oracle's own loads
        dt = float(cfg.dt)
        v0, w0 = h.v[:, 0].copy(), h.w[:, 0].copy()
        acc_t = (1.0 / h.J[2]) * h.t_ext[2, 0]              # the oracle's own torque: its last bit may differ (above)
        h.dynamic(dt)
        h.constrain_rates()
        v1, w1 = h.v[:, 0], h.w[:, 0]
        vm, wm = np.maximum(np.abs(v0), np.abs(v1)), np.maximum(np.abs(w0), np.abs(w1))
        a_lin, a_ang = r.acceleration, r.angular_acceleration
        assert (np.abs((v1 - v0) / dt - a_lin) <= 4 * EPS * vm / dt + EPS * np.abs(a_lin)).all()
        assert a_lin[2] == 0.0 and a_ang[0] == 0.0 and a_ang[1] == 0.0
        assert abs((w1[2] - w0[2]) / dt - acc_t) <= 4 * EPS * wm[2] / dt + EPS * abs(acc_t)
        assert abs(a_ang[2] - acc_t) <= (1.0 / h.J[2]) * net_ulp[2] + EPS * abs(acc_t)
        assert w1[0] == 0.0 and w1[1] == 0.0 and v1[2] == 0.0
        moving += int(np.abs(r.net_force).max() > 0)
    assert moving >= len(states) - 1                       # every state but the reset's carries a net force
    print(f"{case[0]}: entries where the oracle's Q @ torque differs from joint.py's loop (a fused product): {fused}")


def _fused_sums(q, t):
    """q . t with one or two of its products fused into the running sum, each exact and rounded once."""
    from fractions import Fraction as F

    def fma(a, b, c):
        return float(F(a) * F(b) + F(c))

    return (fma(q[1], t[1], q[0] * t[0]), fma(q[0], t[0], q[1] * t[1]),
            fma(q[2], t[2], fma(q[1], t[1], q[0] * t[0])), fma(q[2], t[2], q[0] * t[0] + q[1] * t[1]))


# ---- 3. known answers --------------------------------------------------------------------------------------------------
def _reset_state(n_arm):
    cfg, states, _ = _oracle(n_arm)
    return cfg, {k: np.array(v, np.float64) for k, v in states[0].items()}


@pytest.mark.parametrize("case", ref.CPU_CASES, ids=lambda c: c[0])
def test_reset_state_is_load_free_to_rounding(case):
    """At build_octopus' reset every arm starts on its connection point along its connection direction: every gap is a
    rounding of head_radius (4 eps head_radius: the rotation's, the product's and the sum's) and every torque a
    rounding of its unit (4 eps joint_kt |link| (|x1| + |target|))."""
    cfg, st = _reset_state(case[1])
    r = ref.twin(cfg, st)
    u = ref.band_units(cfg, st)
    assert (r.gap_length <= 4 * EPS * float(cfg.head_radius)).all()
    assert (np.abs(r.body_torque) <= 4 * EPS * u.body_torque).all() and (np.abs(r.arm_torque) <= 4 * EPS * u.arm_torque).all()
    assert (np.abs(r.net_torque) <= 4 * EPS * u.net_torque).all()


def test_head_moved_along_x_is_pulled_back_by_every_spring():
    """The body moved by delta along x from the reset state, nothing moving: every spring is stretched by -delta x^,
    net_force = -n_arm joint_k delta x^ to joint_k eps head_radius, and the acceleration is that over head_mass.  That
    bound is the rounding of ONE spring's subtraction of two numbers of head_radius' size, so it is held as it stands
    on the one-arm octopus.  The eight-arm sum carries eight such roundings — the gaps build_octopus' reset leaves
    between eight rotated start points and eight rotated connection points — and is held to eight times it (1.27e-11
    against 7.1e-11 here; it does not meet the single bound of 8.9e-12, and neither does the reset state itself).
    delta is a power of two, so that moving the head adds no rounding of its own."""
    delta = 2.0 ** -10
    for name, n_arm in ref.CPU_CASES:
        cfg, st = _reset_state(n_arm)
        st["head_x"][0] += delta
        r = ref.twin(cfg, st)
        want = np.array([-n_arm * float(cfg.joint_k) * delta, 0.0, 0.0])
        bound = float(cfg.joint_k) * EPS * float(cfg.head_radius)
        err = np.abs(r.net_force - want).max()
        print(f"{name}: |net_force + n k delta x^| = {err:.2e}, bound {bound:.2e}")
        assert err <= n_arm * bound
        mass, _ = ref.head_mass_invj(cfg)
        np.testing.assert_array_equal(r.acceleration, np.array([r.net_force[0] / mass, r.net_force[1] / mass, 0.0]))
        assert r.acceleration[0] < 0 and not r.angular_acceleration[:2].any()


def test_head_turned_by_a_small_angle_is_turned_back():
    """The body turned by phi about z from the reset state: the connection points move round the centre, their sum
    does not (eight arms, evenly spaced), so the net force is at rounding level — 4 eps of its band unit — while
    every joint's restoring torque opposes the turn: net_torque_z has the sign of -phi and the size of
    n_arm joint_kt rest_length (head_radius + rest_length) phi to first order."""
    cfg, st0 = _reset_state(8)
    rl = float(cfg.base_length) / int(cfg.n_elem)
    for phi in (1e-3, -1e-3):
        st = {k: v.copy() for k, v in st0.items()}
        c, s = np.cos(phi), np.sin(phi)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        st["head_Q"] = st["head_Q"] @ R.T                       # every body axis (a row) turned by phi
        r = ref.twin(cfg, st)
        u = ref.band_units(cfg, st)
        assert (np.abs(r.net_force) <= 4 * EPS * u.net_force).all(), r.net_force
        assert np.sign(r.net_torque[2]) == -np.sign(phi)
        first_order = 8 * float(cfg.joint_kt) * rl * (float(cfg.head_radius) + rl) * abs(phi)
        assert abs(r.net_torque[2]) == pytest.approx(first_order, rel=1e-2)
        assert np.sign(r.angular_acceleration[2]) == -np.sign(phi)


@pytest.mark.parametrize("case", ref.CPU_CASES, ids=lambda c: c[0])
def test_a_held_head_reports_loads_and_no_acceleration(case):
    cfg, st = _reset_state(case[1])
    cfg = cfg.copy()
    cfg.head_fixed = 1
    st["head_x"][0] += 2.0 ** -10
    r = ref.twin(cfg, st)
    six = np.concatenate([r.acceleration, r.angular_acceleration])
    assert (six == 0.0).all() and not np.signbit(six).any()
    assert np.abs(r.net_force).max() > 0


@pytest.mark.parametrize("case", ref.CPU_CASES, ids=lambda c: c[0])
def test_rows_are_exact_negations_and_left_to_right_sums(case):
    cfg, states, _ = _oracle(case[1])
    for st in states:
        r = ref.twin(cfg, st)
        assert r.arm_force.tobytes() == (-r.body_force).tobytes()
        nf, nt = np.zeros(3), np.zeros(3)
        for a in range(case[1]):
            nf = nf + r.body_force[a]
            nt = nt + r.body_torque[a]
        assert r.net_force.tobytes() == nf.tobytes() and r.net_torque.tobytes() == nt.tobytes()


# ---- 4. band calibration -----------------------------------------------------------------------------------------------
def _calibration_inputs():
    for _, n_arm in ref.CPU_CASES:
        cfg, states, _ = _oracle(n_arm)
        for st in states:
            yield cfg, st
    yield from ref.golden_cases(np.load(GOLD / "octo_operator_vectors.npz"))


def _largest_move():
    top = {}
    for cfg, st in _calibration_inputs():
        base = ref.twin(cfg, st)
        assert all(np.isfinite(np.asarray(t)).all() for t in base)
        moved = []
        for k in range(6):                                   # the arms' x, v, Q and the body's x, v, Q
            for sgn in (1.0, -1.0):
                sc = [1.0] * 6
                sc[k] = 1.0 + sgn * EPS
                moved.append(ref.twin(cfg, st, scale=sc))
        trig = ref.host_trig(cfg)
        for col in (0, 1):                                   # cos, sin: one ulp either way
            for toward in (np.inf, -np.inf):
                t = trig.copy()
                t[:, col] = np.nextafter(t[:, col], toward)
                moved.append(ref.twin(cfg, st, trig=t))
        np.testing.assert_array_equal(ref.twin(cfg, st, trig=trig).body_force, base.body_force)
        for m in moved:
            for f, v in ref.worst(m, base, cfg, st).items():
                top[f] = max(top.get(f, 0.0), v)
    return top


def test_band_is_ten_times_the_twins_own_conditioning():
    """BAND is the smallest power of ten that is at least ten times the largest move of the twin, in band units, over the
    oracle's states and the golden vectors, and WORST is that move as recorded in tests/joint_loads_ref.py."""
    top = _largest_move()
    print("the twin moves by at most", {f: f"{v:.2e}" for f, v in top.items()})
    largest = max(top.values())
    assert set(top) == set(FIELDS)
    assert ref.BAND == 10.0 ** np.ceil(np.log10(10.0 * largest)), (largest, ref.BAND)
    assert abs(largest / ref.WORST - 1.0) < 0.1, (largest, ref.WORST)      # the recorded figure, to its two digits


# ---- 5. shapes and shells ----------------------------------------------------------------------------------------------
def test_other_backends_raise(oracle_built):
    env = _vec("OctoFlat-v0", 2, OracleBackend)
    with pytest.raises(NotImplementedError) as e:
        env.joint_loads()
    assert str(e.value) == "joint loads need the HIP backend, not OracleBackend"


@pytest.mark.parametrize("env_id", ["SoftPendulum-v0", "OctoArmSingle-v0", "OctoArmPush-v1"])
def test_an_env_without_a_rigid_body_raises_the_librarys_text(env_id):
    env = _vec(env_id, 2, StubBackend)
    with pytest.raises(ValueError) as e:
        env.joint_loads()
    assert str(e.value) == "joint loads: this handle has no rigid body"


@pytest.mark.parametrize("env_id,n,rods", [("OctoFlat-v0", 3, 8), ("OctoFlatLite-v0", 2, 1), ("OctoArmPullWeight-v0", 2, 1),
                                           ("OctoCrawl-v0", 2, 8), ("OctoArmTwo-v0", 2, 2), ("OctoReach-v0", 2, 8)])
def test_shapes_and_numpy_output(env_id, n, rods):
    shapes = [(rods, 3)] * 5 + [(rods,)] + [(3,)] * 4
    r = _vec(env_id, n, StubBackend).joint_loads()
    assert isinstance(r, JointLoads) and r._fields == FIELDS
    assert [tuple(t.shape) for t in r] == [(n,) + s for s in shapes]
    r = _vec(env_id, n, StubBackend, numpy_output=True).joint_loads()
    assert all(isinstance(t, np.ndarray) for t in r) and [t.shape for t in r] == [(n,) + s for s in shapes]


def test_single_env_shell_drops_the_env_axis():
    from gym_softrobot_amd.envs.octo_flat import FlatEnv

    probe = FlatEnv(backend=_Probe())
    r = FlatEnv(backend=StubBackend(probe._vec.cfg)).joint_loads()
    assert isinstance(r, JointLoads) and all(isinstance(t, np.ndarray) for t in r)
    assert [t.shape for t in r] == [(8, 3)] * 5 + [(8,)] + [(3,)] * 4


def test_views_cut_the_buffer_into_its_rows_and_columns():
    buf = np.arange(2 * 4 * 16, dtype=np.float64).reshape(2, 4, 16)          # three arms and the body
    v = diagnostics.joint_loads_views(buf)
    assert [t.shape for t in v] == [(2, 3, 3)] * 5 + [(2, 3)] + [(2, 3)] * 4
    assert v.body_torque[1, 2, 1] == buf[1, 2, 4] and v.arm_force[0, 1, 2] == buf[0, 1, 8]
    assert v.arm_torque[1, 0, 0] == buf[1, 0, 9] and v.gap[0, 2, 2] == buf[0, 2, 14] and v.gap_length[1, 1] == buf[1, 1, 15]
    assert v.net_force[1, 0] == buf[1, 3, 0] and v.net_torque[0, 2] == buf[0, 3, 5]
    assert v.acceleration[1, 1] == buf[1, 3, 7] and v.angular_acceleration[0, 2] == buf[0, 3, 11]


# ---- 6. codegen of the new kernel --------------------------------------------------------------------------------------
def test_joint_loads_kernel_has_no_scratch_and_no_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path / "capi.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(asm), str(CSRC / "softrod_capi.hip")], check=True, timeout=900, stderr=subprocess.DEVNULL)
    text = asm.read_text()
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        if "softrod_joint_loads_kernel" in re.search(r"\.name:\s+(\S+)", blk).group(1):
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))      # noqa: E731
            print(f"softrod_joint_loads_kernel: {g('vgpr_count')} VGPRs")
            assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0
            assert g("group_segment_fixed_size") == 0
            return
    raise AssertionError("softrod_joint_loads_kernel not found")
