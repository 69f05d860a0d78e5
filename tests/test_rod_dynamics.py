"""rod_dynamics() without a GPU (softrod_rod_dynamics, VecRodEnvBase.rod_dynamics): the symbol in header, library source
and bindings; the Python copy of the refusals against the library's wording; the shells through a stub backend; the
calibration of the band tests/test_gpu_rod_dynamics.py holds the device to, on the C oracle's states of the same seeds;
known answers of the yardstick (tests/rod_dynamics_ref.py) and its dependence on what it claims to contain."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi, diagnostics

try:
    from tests import ground_reaction_ref as gr
    from tests import muscle_loads_ref as ml
    from tests import rod_dynamics_ref as ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import ground_reaction_ref as gr
    import muscle_loads_ref as ml
    import rod_dynamics_ref as ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


class RecordingOracle(OracleBackend):
    """The oracle backend, keeping the layers it is handed where the HIP backend keeps them."""

    def set_muscle_layers(self, ratio_position, strength):
        rp, st = np.ascontiguousarray(ratio_position, np.float64), np.ascontiguousarray(strength, np.float64)
        self._tables = {"muscle_layers": rp.tobytes() + st.tobytes()}
        super().set_muscle_layers(ratio_position, strength)


class StubBackend:
    """A backend with a rod_dynamics of the device's shapes (zeros): what VecRodEnvBase hands on."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}

    def rod_dynamics(self):
        import torch

        buf = torch.zeros((self.n_envs, _capi.config_rods_per_env(self.cfg), 18, int(self.cfg.n_elem) + 1), dtype=torch.float64)
        return diagnostics.rod_dynamics_views(buf)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    kw = {k: v for k, v in kw.items() if k != "math_mode" or not issubclass(backend_cls, OracleBackend)}
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


# ---- 1. the interface --------------------------------------------------------------------------------------------------
def test_symbol_header_and_table():
    header = (ROOT / "include" / "softrod.h").read_text()
    assert "int softrod_rod_dynamics(softrod_handle* h, double* out, void* stream);" in header
    assert "[n_envs][rods_per_env][18][n_elem + 1]" in header and "NOT the value the last substep applied" in header
    source = (CSRC / "softrod_capi.hip").read_text()
    assert "int softrod_rod_dynamics(softrod_handle* h, double* out, void* stream) {" in source
    kernel = (CSRC / "softrod_dynamics_readout.hpp").read_text()
    assert "kDynamicsRows = 18" in kernel and "#pragma clang fp contract(off)" in kernel
    assert "rod_literal_joint(P, S, R.N, R.env, R.arm, lane, X, jf, jt);" in kernel
    assert "rod_literal_contact(P, S, env, lane, X, F, T, fc, dt);" in kernel
    literal = (CSRC / "softrod_literal.hpp").read_text()                       # ... which call the two laws themselves
    assert "const JointLoad J = joint_load_literal(P, H, arm, x0, v0, x1);" in literal
    assert "plane_contact_n<1, false, false>(CP, Pc, lane, CK, X.L, X.xn, X.vn, X.len, F1, tq, fc1);" in literal
    assert "__shared__" not in kernel and "atomic" not in kernel.replace("no atomics", "")
    assert "softrod_rod_dynamics" in _capi.EXPORTED_SYMBOLS
    assert _capi._EXPORTS["softrod_rod_dynamics"] == _capi._EXPORTS["softrod_rod_energies"]
    assert _capi.ABI_VERSION == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)


def test_every_refusal_has_its_copy_on_the_other_side():
    source = re.sub(r'"\s*\n\s*"', "", (CSRC / "softrod_capi.hip").read_text())
    py = (ROOT / "gym_softrobot_amd" / "_capi.py").read_text()
    lib, copy = (set(re.findall(r'"(rod dynamics: [^"]*)"', t)) for t in (source, py))
    assert lib == copy and len(lib) == 5
    assert set(_capi.ROD_DYNAMICS_ARGUMENT_ERRORS) == {"rod dynamics: null handle", "rod dynamics: null output buffer"}
    assert _capi.rod_dynamics_refusal(_capi.arm_push_config(2), muscles_set=False) == \
        "rod dynamics: softrod_set_muscle_layers has not been called"
    assert _capi.rod_dynamics_refusal(_capi.arm_push_config(2)) is None


REFUSED = [("SoftArmTracking-v0", {}, "not with spline muscle torques"),
           ("OctoArmSingle-v0", dict(n_elems=100), "rods of up to 63 elements only"),
           ("OctoArmPush-v1", dict(n_elems=64), "rods of up to 63 elements only"),
           ("SoftPendulum-v0", dict(n_elems=64), "rods of up to 63 elements only")]


@pytest.mark.parametrize("env_id,kw,part", REFUSED, ids=[r[0] + "".join(f"-{v}" for v in r[1].values()) for r in REFUSED])
def test_python_refusals_use_the_librarys_wording(env_id, kw, part):
    env = _vec(env_id, 2, StubBackend, **kw)
    why = _capi.rod_dynamics_refusal(env.cfg)
    assert why.startswith("rod dynamics: ") and part in why
    source = (CSRC / "softrod_capi.hip").read_text()
    assert f'"{why}"' in re.sub(r'"\s*\n\s*"', "", source)          # the library's string literal, word for word
    with pytest.raises(NotImplementedError) as e:
        env.rod_dynamics()
    assert str(e.value) == why


@pytest.mark.parametrize("env_id,n,rods,ne", [("SoftPendulum-v0", 3, 1, 50), ("OctoArmTwo-v0", 2, 2, 20), ("OctoFlat-v0", 2, 8, 10)])
def test_shapes_and_numpy_output(env_id, n, rods, ne):
    env = _vec(env_id, n, StubBackend)
    assert _capi.rod_dynamics_refusal(env.cfg) is None
    for out, kind in ((env.rod_dynamics(), None), (_vec(env_id, n, StubBackend, numpy_output=True).rod_dynamics(), np.ndarray)):
        assert type(out).__name__ == "RodDynamics" and out._fields == ref.FIELDS
        for f, t in zip(ref.FIELDS, out):
            assert tuple(t.shape) == (n, rods, 3, ne + 1 if f in ref.NODAL else ne), f
            assert kind is None or isinstance(t, kind)


def test_single_env_shell_drops_the_env_axis():
    from gym_softrobot_amd.envs.octo_flat import FlatEnv
    from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

    for cls, rods, ne in ((SoftPendulumEnv, 1, 50), (FlatEnv, 8, 10)):
        probe = cls(backend=_Probe())
        out = cls(backend=StubBackend(probe._vec.cfg)).rod_dynamics()
        for f, t in zip(ref.FIELDS, out):
            assert isinstance(t, np.ndarray) and t.shape == (rods, 3, ne + 1 if f in ref.NODAL else ne), f


def test_oracle_backend_has_no_rod_dynamics(oracle_built):
    env = _vec("SoftPendulum-v0", 2, OracleBackend)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        env.rod_dynamics()


# ---- 2. the oracle backend's states of the case matrix ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _states(case_id):
    """[(label, [one state per env])] of one case on the oracle backend, at the instants of the GPU test: after
    reset(seed=0) and 2 steps of the case's actions; the muscle cases also at time 0 with the seeded activations
    written; the static cases with their rates scaled; arm-random with each env's drawn rows in its config."""
    case = next(c for c in ref.NO_CONTACT + ref.CONTACT + ref.MUSCLE if c[0] == case_id)
    _, env_id, n, _ = case
    env = _vec(env_id, n, RecordingOracle, **ref.make_kwargs(case))
    env.reset(seed=ref.SEED)
    out = []
    if case in ref.MUSCLE:
        ml.write_activations(env, ml.seeded_activations(env))
        out.append(("time 0", ref.env_states(env)))
        assert all(s["time"] == 0.0 for s in out[0][1])
    for a in ref.actions(env, case):
        env.step(a)
    cfgs = None
    if case == ref.RANDOM:
        tables = ref.draw_tables(env.cfg, n)
        cfgs = [ref.cfg_with_tables(env.cfg, i, tables) for i in range(n)]
    states = ref.env_states(env, cfgs)
    if case in ref.STATIC:
        states = [gr.slowed(s) for s in states]
    assert all(s["time"] != 0.0 for s in states)
    out.append(("stepped", states))
    env.close()
    return out


ALL = ref.NO_CONTACT + ref.CONTACT + ref.MUSCLE
CPU = [c for c in ALL if "libm" not in c[0]]         # the oracle backend has one arithmetic: the -libm cases repeat their twins


@pytest.mark.parametrize("case", CPU, ids=lambda c: c[0])
def test_band_is_ten_times_the_yardsticks_own_conditioning(oracle_built, case):
    """Scaling x, v, Q, w or the body's state by 1 +- 2^-52, one at a time, moves the yardstick by at most WORST units
    on what is compared, on every state of the matrix; BAND is the smallest power of ten at least ten times WORST, and
    at most ground_reaction_ref.RTOL."""
    top = {}
    left = touch = 0
    for label, states in _states(case[0]):
        for st in states:
            base = ref.evaluate(st)
            assert all(np.isfinite(t).all() for t in base)
            sens, touching = ref.sensitive(st)
            left, touch = left + int(sens.sum()), touch + int(touching.sum())
            for which in ("x", "v", "Q", "w", "head"):
                if which == "head" and "head_x" not in st:
                    continue
                for sgn in (1.0, -1.0):
                    moved = ref.evaluate(ref.scaled(st, which, 1.0 + sgn * ref.EPS))
                    for f, v in ref.worst(moved, base, st, sens).items():
                        top[f] = max(top.get(f, 0.0), v)
    print(f"{case[0]}: the yardstick moves by at most", {f: f"{v:.1e}" for f, v in top.items()},
          "left out", left, "of", touch, "in contact")
    assert max(top.values()) <= ref.WORST, top
    assert 10.0 * ref.WORST <= ref.BAND < 100.0 * ref.WORST
    assert ref.BAND == 10.0 ** round(np.log10(ref.BAND)) and ref.BAND <= gr.RTOL
    if ref.has_contact(states[0]["cfg"]):
        assert touch > 0 and left <= gr.CAP * touch, (left, touch)
    else:
        assert left == 0


# ---- 3. known answers of the yardstick --------------------------------------------------------------------------------
def _straight_state(cfg, point_force=0.0):
    n = int(cfg.n_elem)
    x = np.zeros((1, 3, n + 1))
    x[0, 0] = float(cfg.base_length) * np.arange(n + 1) / n
    Q = np.zeros((1, 3, 3, n))
    Q[0, 0, 1], Q[0, 1, 2], Q[0, 2, 0] = 1.0, 1.0, 1.0           # d1 = e_y, d2 = e_z, d3 = e_x: the tangent
    return dict(x=x, v=np.zeros((1, 3, n + 1)), Q=Q, w=np.zeros((1, 3, n)), rest_kappa=np.zeros((1, 3, n - 1)), time=0.0,
                cfg=cfg, radius=None, point_force=point_force)


def test_a_straight_rod_at_rest_falls_freely():
    """acceleration == gravity at every node and zero angular acceleration: within the band on SoftPendulum's own
    config (the node positions k / 50 are rounded, so neighbouring elements differ by an ulp of strain), and exactly on
    positions that are exact in fp64."""
    cfg = _capi.softpendulum_config(1)
    g = np.asarray(list(cfg.gravity), float)[:, None]
    st = _straight_state(cfg)
    r = ref.evaluate(st)
    u = ref.band_units(st, r)
    assert (np.abs(r.acceleration[0] - g) <= ref.BAND * u.acceleration[0]).all()
    assert (np.abs(r.angular_acceleration[0]) <= ref.BAND * u.angular_acceleration[0]).all()
    cfg.base_length, cfg.n_elem = 2.0, 8                          # eight elements of 0.25
    r = ref.evaluate(_straight_state(cfg))
    assert np.abs(r.internal_force).max() == 0.0 and np.abs(r.internal_torque).max() == 0.0
    assert np.abs(r.angular_acceleration).max() == 0.0
    assert np.abs(r.acceleration[0] - g).max() <= 4 * np.finfo(float).eps * np.abs(g).max()      # g m / m


def test_internal_forces_cancel_and_momentum_balances(oracle_built):
    """sum_nodes internal_force == 0 and sum_nodes mass * acceleration == sum_nodes external_force, within the band (a
    sum of n + 1 entries, each good to a band unit), on every stepped case."""
    for case in CPU:
        for label, states in _states(case[0]):
            for st in states:
                r = ref.evaluate(st)
                u = ref.band_units(st, r)
                n1 = r.internal_force.shape[-1]
                s = np.abs(r.internal_force.sum(axis=-1))
                assert (s <= ref.BAND * n1 * u.internal_force.max(axis=-1)).all(), (case[0], label)
                m = ref.nodal_mass(st)[:, None, :]
                lhs, rhs = (m * r.acceleration).sum(axis=-1), r.external_force.sum(axis=-1)
                unit = np.maximum(u.internal_force.max(axis=-1), u.external_force[..., 0])
                assert (np.abs(lhs - rhs) <= ref.BAND * n1 * unit).all(), (case[0], label)


@pytest.mark.parametrize("case_id,without,fields", [
    ("flat-4", "joint", ("external_force", "external_torque")),
    ("flat-static", "joint", ("external_force", "external_torque")),
    ("arm-fast", "contact", ("external_force", "external_torque", "acceleration", "angular_acceleration")),
    ("crawl", "joint", ("external_force", "external_torque")),
    ("push", "muscles", ("external_force", "external_torque", "acceleration", "angular_acceleration")),
    ("reach", "muscles", ("external_force", "external_torque")),
    ("pendulum-3", "point", ("external_force", "acceleration")),
])
def test_the_yardstick_contains_what_it_claims(oracle_built, case_id, without, fields):
    """Removing the joint, the contact, the muscles or the point force moves the expected values by far more than the
    band."""
    moved = {f: 0.0 for f in fields}
    for label, states in _states(case_id):
        for st in states:
            full, less = ref.evaluate(st), ref.evaluate(st, without=without)
            none = np.zeros(st["x"].shape[:1] + (int(st["cfg"].n_elem),), bool)
            fig = ref.worst(less, full, st, none)
            for f in fields:
                moved[f] = max(moved[f], fig[f])
    print(f"{case_id}: without {without} the yardstick moves by", {f: f"{v:.1e}" for f, v in moved.items()}, "units")
    for f, v in moved.items():
        assert v > 1e3 * ref.BAND, (f, v)


def test_the_point_force_is_the_float32_action_and_none_at_time_zero(oracle_built):
    (_, states), = _states("pendulum-3")
    prev = ref.actions(_vec("SoftPendulum-v0", 4, StubBackend, n_elems=3), ref.NO_CONTACT[0])[-1]
    for e, st in enumerate(states):
        assert st["point_force"] == float(np.float32(prev[e].ravel()[0])) != 0.0
        assert ref.evaluate(st).external_force[0, 0, 0] == st["point_force"]
        fresh = dict(st, time=0.0, point_force=0.0)
        assert ref.evaluate(fresh).external_force[0, 0, 0] == 0.0
