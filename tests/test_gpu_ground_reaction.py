"""softrod_ground_reaction on the MI355X: every rod of every env against oracle/softrod_oracle_np.py evaluated on the
device's own read-back state (tests/ground_reaction_ref.py: the band, the rule for leaving an element out, the cap,
the cases), per-env contact and material, known answers that need no oracle, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi

try:
    from tests import ground_reaction_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import ground_reaction_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1          # SOFTROD_EINVAL
ROD_KEYS = ("x", "v", "Q", "w", "rest_kappa")


def _stepped(env_id, n, **kw):
    env = gsa.make_vec(env_id, n, **kw)
    env.reset(seed=ref.SEED)
    for a in ref.actions(env):
        env.step(a)
    return env


def _states(env):
    """Per env: the read-back state in the oracle's shapes."""
    if env.cfg.env_kind == _capi.ENV_OCTO_FLAT:
        s = env.backend.octo_state_numpy()
        return [{k: s[k][i] for k in ROD_KEYS + ("head_x", "head_v", "head_Q", "head_w")} for i in range(env.num_envs)]
    s = env.backend.state_numpy()
    return [{k: s[k][i] for k in ROD_KEYS} for i in range(env.num_envs)]


def _reaction(env):
    force, torque = env.ground_reaction()
    return force.cpu().numpy().copy(), torque.cpu().numpy().copy()


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_every_rod_matches_the_oracle_on_the_devices_state(hip_lib, case):
    _, env_id, n, kw = case
    env = _stepped(env_id, n, **kw)
    octo = env.cfg.env_kind == _capi.ENV_OCTO_FLAT
    got = _reaction(env)
    rods_per_env = int(env.cfg.n_arm) if octo else 1
    assert got[0].shape == (n, rods_per_env, 3, int(env.cfg.n_elem) + 1)
    assert got[1].shape == (n, rods_per_env, 3, int(env.cfg.n_elem))
    rods, left, touch = ref.check_case([env.cfg] * n, _states(env), got, octo, kw.get("radius_profile"))
    assert rods == n * rods_per_env                   # every arm of every env was checked
    assert np.abs(got[0]).max() > 0 and np.abs(got[1]).max() > 0
    _assert_waves(env, case[0])
    env.close()


def _assert_waves(env, case_id):
    """The wave shape a case claims: the state rows of an env are 64 lanes per wave wide."""
    if case_id in ref.WAVES:
        assert env.backend.state()["position"].shape[2] == 64 * ref.WAVES[case_id]


@pytest.mark.parametrize("case", ref.STATIC_CASES, ids=lambda c: c[0])
def test_static_friction_reads_the_internal_loads_and_the_joint(hip_lib, case):
    """The stepped, bent states with every rate scaled below the slip tolerance (ref.STATIC_CASES): the kinetic terms
    vanish and the static ones answer to f_int + f_ext and t_int + t_ext, the joint's force and torque included
    (tests/test_ground_reaction.py shows on the CPU that the expected values move when any of them is removed)."""
    _, env_id, n, kw = case
    env = _stepped(env_id, n, **kw)
    octo = env.cfg.env_kind == _capi.ENV_OCTO_FLAT
    st = env.backend.state()
    st["velocity"] *= ref.RATE_SCALE
    st["omega"] *= ref.RATE_SCALE
    if octo:
        st["head"][3:6] *= ref.RATE_SCALE
        st["head"][15:18] *= ref.RATE_SCALE
    states = _states(env)
    for s in states:
        assert 0 < np.abs(s["v"]).max() < 0.1 * env.cfg.slip_velocity_tol
    got = _reaction(env)
    rods, left, touch = ref.check_case([env.cfg] * n, states, got, octo, kw.get("radius_profile"))
    assert rods == n * (int(env.cfg.n_arm) if octo else 1)
    assert np.abs(got[1]).max() > 0                   # static rolling friction's torque
    _assert_waves(env, case[0])
    env.close()


def _draw_contact(n, seed):
    rng = np.random.default_rng(seed)
    return dict(contact_k=100.0 * 2.0 ** rng.uniform(-1, 1, n), contact_nu=10.0 * 2.0 ** rng.uniform(-1, 1, n),
                friction_multiplier=2.0 ** rng.uniform(-2, 2, n), friction_symmetry=rng.random(n) < 0.5)


def _draw_material(env, n, seed):
    rng = np.random.default_rng(seed)
    c = env.cfg
    return dict(youngs_modulus=c.youngs_modulus * 2.0 ** rng.uniform(-1, 1, n), density=c.density * 2.0 ** rng.uniform(-1, 1, n),
                damping_constant=c.damping_constant * 2.0 ** rng.uniform(-1, 1, n))


@pytest.mark.parametrize("env_id,n,material", [("OctoArmSingle-v0", 8, True), ("OctoFlat-v0", 5, False)])
def test_per_env_tables_are_honoured(hip_lib, env_id, n, material):
    """Random contact (and material) rows on all envs but the first, the middle and the last: each env matches the
    oracle built with ITS values, and the envs left at the config's values are byte-identical to a handle without
    tables."""
    mask = np.ones(n, bool)
    mask[[0, n // 2, n - 1]] = False
    uni = _stepped(env_id, n)
    rnd = gsa.make_vec(env_id, n)
    rnd.set_contact(mask, **_draw_contact(n, 5))
    if material:
        rnd.set_material(mask, **_draw_material(rnd, n, 6))
    rnd.reset(seed=ref.SEED)
    for a in ref.actions(rnd):
        rnd.step(a)
    assert rnd.backend.kernel_tier().endswith("env contact")
    got_u, got_r = _reaction(uni), _reaction(rnd)
    for g_u, g_r in zip(got_u, got_r):
        assert g_u[~mask].tobytes() == g_r[~mask].tobytes()
        assert not np.array_equal(g_u[mask], g_r[mask])
    octo = rnd.cfg.env_kind == _capi.ENV_OCTO_FLAT
    cfgs = [ref.cfg_env(rnd, i) for i in range(n)]
    assert any(cfgs[i].contact_k != rnd.cfg.contact_k for i in range(n))
    rods, _, _ = ref.check_case(cfgs, _states(rnd), got_r, octo)
    assert rods == n * (int(rnd.cfg.n_arm) if octo else 1)
    uni.close()
    rnd.close()


@pytest.mark.parametrize("env_id,n", [("OctoArmSingle-v0", 3), ("OctoFlat-v0", 5)])
def test_arms_above_the_plane_feel_nothing(hip_lib, env_id, n):
    env = _stepped(env_id, n)
    c = env.cfg
    st = env.backend.state()
    st["position"][2] += 10.0 * (c.base_radius + c.surface_tol) + 1.0       # far more than radius + surface_tol
    force, torque = _reaction(env)
    assert not force.any() and not torque.any()                               # exact zeros
    env.close()


@pytest.mark.parametrize("math_mode", [_capi.MATH_LIBM, _capi.MATH_FAST], ids=["libm", "fast"])
def test_straight_arm_at_rest_pressed_into_the_plane(hip_lib, math_mode):
    """A straight OctoArmSingle arm at rest (the reset state: v = omega = 0), every node 1e-4 below touching: per
    element F_z = k * penetration + the plane's response to the element's weight, written out here; no damping, no
    kinetic friction (nothing moves), no rolling friction (nothing pushes sideways)."""
    n = 3
    env = gsa.make_vec("OctoArmSingle-v0", n, math_mode=math_mode)
    env.reset(seed=0)
    c = env.cfg
    ne = int(c.n_elem)
    assert tuple(c.plane_normal) == (0.0, 0.0, 1.0)
    z = c.plane_origin[2] + c.base_radius - 1e-4
    st = env.backend.state()
    st["position"][2, :, : ne + 1] = z
    x = env.backend.state_numpy()["x"][0]
    assert np.array_equal(x[2], np.full(ne + 1, z))
    # what the law sees, in NumPy: element lengths and radii (volume preserving), nodal weights, their element sums
    d = x[:, 1:] - x[:, :-1]
    length = np.sqrt((d * d).sum(axis=0)) + c.eps_length
    rest_len = c.base_length / ne
    radius = np.sqrt(np.pi * c.base_radius ** 2 * rest_len / length / np.pi)
    pen = np.minimum((z - c.plane_origin[2]) - radius, 0.0)
    np.testing.assert_allclose(pen, -1e-4, rtol=1e-6)
    m_node = np.full(ne + 1, c.density * np.pi * c.base_radius ** 2 * rest_len)
    m_node[[0, -1]] *= 0.5
    w_node = c.gravity[2] * m_node                                            # < 0
    w_elem = 0.5 * (w_node[:-1] + w_node[1:])
    w_elem[0] += 0.5 * w_node[0]
    w_elem[-1] += 0.5 * w_node[-1]
    fz_elem = -c.contact_k * pen + -w_elem
    fz_node = np.zeros(ne + 1)
    fz_node[:-1] += 0.5 * fz_elem
    fz_node[1:] += 0.5 * fz_elem
    force, torque = _reaction(env)
    for i in range(n):
        np.testing.assert_allclose(force[i, 0, 2], fz_node, rtol=0, atol=ref.RTOL * np.abs(fz_node).max())
        assert np.abs(force[i, 0, 1]).max() == 0.0 and np.abs(torque[i, 0]).max() <= ref.RTOL * np.abs(fz_node).max() * c.base_radius
        # along the arm: static friction never exceeds the push it opposes, here the stretch force E A e of the
        # eps_length pre-strain (plus the rounding of the reset's node positions) at the two end elements
        push = c.youngs_modulus * np.pi * c.base_radius ** 2 * (c.eps_length / rest_len + 1e-12)
        assert np.abs(force[i, 0, 0]).max() <= push
    env.close()


@pytest.mark.parametrize("env_id,n", [("OctoArmSingle-v0", 5), ("OctoFlat-v0", 5)])
def test_reading_twice_is_identical_and_moves_nothing(hip_lib, env_id, n):
    a_env, b_env = _stepped(env_id, n), _stepped(env_id, n)
    first = _reaction(a_env)
    second = _reaction(a_env)
    for u, v in zip(first, second):
        assert u.tobytes() == v.tobytes()
    f, t = a_env.ground_reaction()
    assert f.data_ptr() == a_env.ground_reaction()[0].data_ptr()               # one buffer, overwritten
    assert t.shape[-1] == f.shape[-1] - 1
    keys = ["position", "velocity", "director", "omega", "time", "kappa", "rest_kappa"] + (
        ["head"] if a_env.cfg.env_kind == _capi.ENV_OCTO_FLAT else [])
    sa, sb = a_env.backend.state(), b_env.backend.state()
    for k in keys:
        assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), k
    act = ref.actions(a_env, 1, 9)[0]
    for u, v in zip(a_env.step(act)[:4], b_env.step(act)[:4]):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    for k in keys:
        assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), k
    a_env.close()
    b_env.close()


def test_numpy_output_and_the_single_env(hip_lib):
    env = gsa.make_vec("OctoArmSingle-v0", 2, numpy_output=True)
    env.reset(seed=0)
    force, torque = env.ground_reaction()
    assert isinstance(force, np.ndarray) and force.shape == (2, 1, 3, 51) and torque.shape == (2, 1, 3, 50)
    env.close()
    one = gsa.make("OctoFlat-v0")
    one.reset(seed=0)
    force, torque = one.ground_reaction()
    assert isinstance(force, np.ndarray) and force.shape == (8, 3, 11) and torque.shape == (8, 3, 10)
    one.close()


REFUSED = [("SoftPendulum-v0", {}), ("OctoArmPush-v1", {}), ("OctoCrawl-v0", {}), ("OctoArmSingle-v0", dict(n_elems=100))]


@pytest.mark.parametrize("env_id,kw", REFUSED, ids=[r[0] + ("-100" if r[1] else "") for r in REFUSED])
def test_out_of_scope_handles_are_refused(hip_lib, env_id, kw):
    env = gsa.make_vec(env_id, 2, **kw)
    be = env.backend
    out = torch.zeros(2 * 8 * 6 * 128, dtype=torch.float64, device=be.device)
    assert hip_lib.softrod_ground_reaction(be._h, C.c_void_p(out.data_ptr()), be._stream()) == EINVAL
    why = hip_lib.softrod_last_error(be._h).decode()
    assert why.startswith("ground reaction: ")
    assert why == _capi.ground_reaction_refusal(env.cfg)
    with pytest.raises(NotImplementedError) as e:
        env.ground_reaction()
    assert str(e.value) == why
    torch.cuda.synchronize()
    assert not out.any()                                                      # nothing was launched
    env.close()
