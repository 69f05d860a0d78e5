"""Per-env rod material on the MI355X (set_material / softrod_set_env_material): the config's own values give
byte-identical rollouts, randomised envs match the CPU oracle built with each env's own config, untouched envs are
bit-identical to a uniform batch, energies, auto-resets, masked updates, snapshots, captured graphs and the
refusals of out-of-scope handles."""
import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import rod_energies_host, rod_material_host

pytestmark = pytest.mark.gpu

RTOL = 1e-5
EINVAL = -1          # SOFTROD_EINVAL
ENVS = ["SoftPendulum-v0", "SoftPendulum3D-v0", "OctoArmSingle-v0"]
MODES = [(0, "libm"), (1, "fast")]
KEYS = ("youngs_modulus", "shear_modulus", "density", "damping_constant")


def _acts(env_id, T, n, seed):
    rng = np.random.default_rng(seed)
    if env_id == "SoftPendulum-v0":
        return rng.uniform(-22, 22, (T, n, 1)).astype(np.float32)
    if env_id == "SoftPendulum3D-v0":
        return rng.uniform(-1, 1, (T, n, 2)).astype(np.float32)
    return rng.uniform(-6, 6, (T, n, 7)).astype(np.float32)


def _outputs(env, a):
    obs, rew, term, trunc, _ = env.step(a)
    return [x.cpu().numpy().copy() for x in (obs, rew, term, trunc)]


def _state(env):
    st = env.backend.state()
    return {k: st[k].cpu().numpy().copy() for k in ("position", "velocity", "director", "omega", "time", "control")}


def _draw(n, seed):
    """E, rho, nu per env across x0.5 .. x2 of the config's (G = E / 3)."""
    rng = np.random.default_rng(seed)
    return {k: 2.0 ** rng.uniform(-1, 1, n) for k in ("youngs_modulus", "density", "damping_constant")}


def _randomise(env, f, mask=None):
    c = env.cfg
    env.set_material(mask, youngs_modulus=c.youngs_modulus * f["youngs_modulus"], density=c.density * f["density"],
                     damping_constant=c.damping_constant * f["damping_constant"])


def _cfg_i(env, i):
    c = env.cfg.copy()
    c.n_envs = 1
    m = env.material()
    for k in KEYS:
        setattr(c, k, float(m[k][i]))
    return c


@pytest.mark.parametrize("math_mode,mode_id", MODES, ids=[m[1] for m in MODES])
@pytest.mark.parametrize("env_id", ENVS)
def test_config_values_are_byte_identical(hip_lib, env_id, math_mode, mode_id):
    n, T = 13, 3
    a_env = gsa.make_vec(env_id, n, math_mode=math_mode)
    b_env = gsa.make_vec(env_id, n, math_mode=math_mode)
    b_env.set_material(**{k: getattr(b_env.cfg, k) for k in KEYS})
    assert b_env.backend.kernel_tier().endswith(",env material")
    assert not a_env.backend.kernel_tier().endswith(",env material")
    a_env.reset(seed=5)
    b_env.reset(seed=5)
    for a in _acts(env_id, T, n, 1):
        for x, y in zip(_outputs(a_env, a), _outputs(b_env, a)):
            assert x.tobytes() == y.tobytes()
    sa, sb = _state(a_env), _state(b_env)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    np.testing.assert_array_equal(a_env.rod_energies().cpu().numpy(), b_env.rod_energies().cpu().numpy())
    a_env.close()
    b_env.close()


def _oracles(env, env_id, oracle_c):
    from gym_softrobot_amd.envs.soft_pendulum_3d import initial_tilt
    from gym_softrobot_amd.seeding import initial_angle, np_random

    rods = []
    for i in range(env.num_envs):
        r = oracle_c.OracleRod(_cfg_i(env, i))
        if env_id == "SoftPendulum-v0":
            r.reset_pendulum(initial_angle(np_random(i)[0]))
        elif env_id == "SoftPendulum3D-v0":
            r.reset_pendulum3d(initial_tilt(np_random(i)[0]))
        else:
            r.reset_arm()
        rods.append(r)
    return rods


def _ostep(env_id, r, a):
    if env_id == "SoftPendulum-v0":
        return r.env_step(a[0])
    if env_id == "SoftPendulum3D-v0":
        return r.env_step3d(a)[:4]
    return r.env_step_arm(a)


@pytest.mark.parametrize("math_mode,mode_id", MODES, ids=[m[1] for m in MODES])
@pytest.mark.parametrize("env_id,n,T", [("SoftPendulum-v0", 256, 3), ("SoftPendulum3D-v0", 64, 3),
                                        ("OctoArmSingle-v0", 64, 2)])
def test_randomised_batch_matches_the_oracle_per_env(hip_lib, oracle_built, env_id, n, T, math_mode, mode_id):
    env = gsa.make_vec(env_id, n, math_mode=math_mode)
    _randomise(env, _draw(n, 11))
    env.reset(seed=0)                                   # env i draws from seed i
    rods = _oracles(env, env_id, oracle_built)
    perturbed = []
    if env_id == "SoftPendulum-v0":       # a few envs out of the plane: the 3-D fallback with the env's own row
        st = env.backend.state()
        for i in (3, 100, n - 1):
            v = rods[i].get("v")
            v[2, 10:30] = 0.3
            rods[i].set("v", v)
            st["velocity"][2, i, 10:30] = 0.3
            perturbed.append(i)
    for a in _acts(env_id, T, n, 2):
        obs, rew, term, trunc = _outputs(env, a)
        for i, r in enumerate(rods):
            o, rw, te, tr = _ostep(env_id, r, a[i])
            np.testing.assert_allclose(obs[i], o, rtol=RTOL, atol=1e-7)
            np.testing.assert_allclose(rew[i], rw, rtol=RTOL, atol=1e-9)
            assert bool(term[i]) == te and bool(trunc[i]) == tr
    sn = env.backend.state_numpy()
    for i, r in enumerate(rods):
        for name in ("x", "Q"):
            ref = r.get(name)
            assert np.max(np.abs(sn[name][i] - ref)) <= RTOL * np.max(np.abs(ref)), (i, name)
        assert sn["time"][i] == r.time
    for i in perturbed:
        assert np.abs(sn["x"][i][2]).max() > 1e-4
    env.close()


@pytest.mark.parametrize("env_id", ENVS)
@pytest.mark.parametrize("n", [7, 64])
def test_untouched_envs_are_bit_identical_to_a_uniform_batch(hip_lib, env_id, n):
    T = 3
    uni = gsa.make_vec(env_id, n)
    rnd = gsa.make_vec(env_id, n)
    f = _draw(n, 3)
    mask = np.ones(n, bool)
    mask[[0, n // 2, n - 1]] = False                                  # first, middle and last env keep the config
    _randomise(rnd, f, mask)
    uni.reset(seed=9)
    rnd.reset(seed=9)
    for a in _acts(env_id, T, n, 4):
        for x, y in zip(_outputs(uni, a), _outputs(rnd, a)):
            assert x[~mask].tobytes() == y[~mask].tobytes()
            if x.dtype.kind == "f":
                assert not np.array_equal(x[mask], y[mask])
    su, sr = _state(uni), _state(rnd)
    for k in ("position", "velocity", "director", "omega"):
        assert su[k][:, ~mask].tobytes() == sr[k][:, ~mask].tobytes(), k
    uni.close()
    rnd.close()


@pytest.mark.parametrize("math_mode,mode_id", MODES, ids=[m[1] for m in MODES])
@pytest.mark.parametrize("env_id", ENVS)
def test_energies_use_each_envs_material(hip_lib, env_id, math_mode, mode_id):
    n = 9
    env = gsa.make_vec(env_id, n, math_mode=math_mode)
    _randomise(env, _draw(n, 21))
    env.reset(seed=2)
    for a in _acts(env_id, 2, n, 5):
        env.step(a)
    E = env.rod_energies().cpu().numpy()[:, 0]
    st = env.backend.state_numpy()
    bc = env.backend.state()["bc_targets"].cpu().numpy()
    rk = bool(env.cfg.features & _capi.FEAT_REST_KAPPA_ACTION)
    for i in range(n):
        ci = _cfg_i(env, i)
        kw = {}
        if env.cfg.features & (_capi.FEAT_PENDULUM_BC | _capi.FEAT_FIXED_BC | _capi.FEAT_MOVING_BASE_BC):
            kw = dict(fixed_pos=bc[:3, i], fixed_dir=bc[3:, i].reshape(3, 3), base_xy=st["control"][i, :2])
        want = rod_energies_host(st["x"][i], st["v"][i], st["Q"][i], st["w"][i], float(st["time"][i]), ci,
                                 rod_material_host(ci), st["rest_kappa"][i] if rk else None, **kw)
        np.testing.assert_allclose(E[i], want, rtol=1e-9, atol=max(1e-20, 1e-12 * np.abs(want).max()))
    env.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_device_autoreset_equals_host_autoreset(hip_lib, env_id):
    n, T = 8, 6
    outs = []
    for mode in ("host", "device"):
        kw = dict(final_time=0.08) if env_id != "OctoArmSingle-v0" else dict(final_time=0.02)
        env = gsa.make_vec(env_id, n, autoreset=mode, **kw)
        _randomise(env, _draw(n, 8))
        env.reset(seed=4)
        seq = []
        for a in _acts(env_id, T, n, 6):
            seq.append(_outputs(env, a))
        outs.append(seq)
        env.close()
    assert any(s[3].any() for s in outs[0]), "no episode ended: the auto-reset was not exercised"
    for x, y in zip(*outs):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("env_id", ENVS)
def test_masked_update_between_steps_changes_only_those_envs_from_the_next_step(hip_lib, env_id):
    n = 6
    a_env, b_env = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    for e in (a_env, b_env):
        _randomise(e, _draw(n, 1))
        e.reset(seed=0)
    acts = _acts(env_id, 3, n, 7)
    for e in (a_env, b_env):
        e.step(acts[0])
    mask = np.array([0, 1, 0, 0, 1, 0], bool)
    b_env.set_material(mask, density=b_env.material()["density"] * 1.5)
    assert _state(a_env)["position"].tobytes() == _state(b_env)["position"].tobytes()   # nothing moved yet
    for a in acts[1:]:
        xa, xb = _outputs(a_env, a), _outputs(b_env, a)
        assert xa[0][~mask].tobytes() == xb[0][~mask].tobytes()
        assert not np.array_equal(xa[0][mask], xb[0][mask])
    a_env.close()
    b_env.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_snapshot_restore_reproduces_the_rollout(hip_lib, env_id):
    n = 5
    env = gsa.make_vec(env_id, n)
    _randomise(env, _draw(n, 13))
    env.reset(seed=1)
    acts = _acts(env_id, 4, n, 8)
    env.step(acts[0])
    sd = env.state_dict()
    assert "env_material" in sd["backend"]
    want_mat = env.material()
    first = [_outputs(env, a) for a in acts[1:]]
    env.set_material(density=123.0)                          # the restore must bring back the snapshot's material
    env.load_state_dict(sd)
    for k in KEYS:
        np.testing.assert_array_equal(env.material()[k], want_mat[k])
    again = [_outputs(env, a) for a in acts[1:]]
    for x, y in zip(first, again):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    # a snapshot without the key means the config's values
    del sd["backend"]["env_material"]
    env.load_state_dict(sd)
    for k in KEYS:
        np.testing.assert_array_equal(env.material()[k], getattr(env.cfg, k))
    env.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_captured_graph_matches_eager_and_sees_in_place_updates(hip_lib, env_id):
    n = 16
    eager, graphed = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    W = torch.randn(eager.obs_dim, eager.action_dim, device="cuda", dtype=torch.float32) * 0.1

    def policy(obs):
        return torch.tanh(obs @ W)

    f = _draw(n, 17)
    for e in (eager, graphed):
        _randomise(e, f)
        e.reset(seed=3)
    replay = graphed.capture_policy_step(policy)
    for t in range(4):
        if t == 2:                                           # in-place update between replays, on the env's stream
            for e in (eager, graphed):
                e.set_material(np.arange(n) % 3 == 0, youngs_modulus=e.material()["youngs_modulus"] * 0.7)
        obs_e, rew_e, te, tr, _ = eager.step(policy(eager.backend.obs))
        obs_g, rew_g, tg, trg = replay()
        assert obs_e.cpu().numpy().tobytes() == obs_g.cpu().numpy().tobytes()
        assert rew_e.cpu().numpy().tobytes() == rew_g.cpu().numpy().tobytes()
    eager.close()
    graphed.close()


REFUSED = [("OctoFlat-v0", {}), ("SoftArmTracking-v0", {}), ("OctoArmPush-v1", {}), ("OctoCrawl-v0", {}),
           ("OctoArmSingle-v0", dict(n_elems=100)), ("SoftPendulum3D-v0", dict(n_elems=100))]


@pytest.mark.parametrize("env_id,kw", REFUSED, ids=[r[0] + ("-n100" if r[1] else "") for r in REFUSED])
def test_out_of_scope_handles_refuse_at_the_c_abi(hip_lib, env_id, kw):
    env = gsa.make_vec(env_id, 2, **kw)
    be = env.backend
    m = np.tile(_capi.env_material_defaults(be.cfg), (2, 1))
    rc = hip_lib.softrod_set_env_material(be._h, m.ctypes.data, None, be._stream())
    assert rc == EINVAL
    assert b"per-env material" in hip_lib.softrod_last_error(be._h)
    assert not be.kernel_tier().endswith(",env material")
    with pytest.raises(NotImplementedError):
        env.set_material(density=900.0)
    env.close()


def test_tapered_arm_and_bad_values_refuse_at_the_c_abi(hip_lib):
    edge = np.linspace(0.012, 0.001, 51)
    env = gsa.make_vec("OctoArmSingle-v0", 2, radius_profile=(edge[:-1] + edge[1:]) / 2)
    be = env.backend
    m = np.tile(_capi.env_material_defaults(be.cfg), (2, 1))
    assert hip_lib.softrod_set_env_material(be._h, m.ctypes.data, None, be._stream()) == EINVAL
    env.close()
    env = gsa.make_vec("SoftPendulum-v0", 2)
    be = env.backend
    for bad in ((0, np.nan), (1, -1.0), (2, 0.0), (3, -1e-9), (0, np.inf)):
        m = np.tile(_capi.env_material_defaults(be.cfg), (2, 1))
        m[1, bad[0]] = bad[1]
        assert hip_lib.softrod_set_env_material(be._h, m.ctypes.data, None, be._stream()) == EINVAL
        mask = np.array([1, 0], np.uint8)                    # the bad row masked out: accepted
        assert hip_lib.softrod_set_env_material(be._h, m.ctypes.data, mask.ctypes.data, be._stream()) == 0
    env.close()
