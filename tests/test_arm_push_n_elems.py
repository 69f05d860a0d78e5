"""OctoArmPush with `n_elems` (2..126) on the host side: the config, the env classes and the oracle backend.  The
default of 40 must give the config it gave before the keyword existed; ArmPullWeight stays at 40 (its rigid-body kernel
lays the arm out on a 32-slot pitch).  The device path is tests/test_gpu_arm_push_n_elems.py."""
import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.envs.arm_push import ArmPullWeightEnv, ArmPushEnv, VecArmPullWeightEnv, VecArmPushEnv


@pytest.mark.parametrize("mode", ["discrete", "continuous"])
def test_default_config_is_byte_identical(mode):
    a = _capi.arm_push_config(4, mode=mode)
    b = _capi.arm_push_config(4, mode=mode, n_elems=40)
    assert bytes(a) == bytes(b)
    assert int(a.n_elem) == 40


def test_hundred_elements_config():
    cfg = _capi.arm_push_config(4, mode="continuous", n_elems=100)
    assert int(cfg.n_elem) == 100
    assert _capi.config_obs_dim(cfg) == 2 * 101 + 2 == 204
    ref = _capi.arm_push_config(4, mode="continuous")
    ref.n_elem = 100
    assert bytes(cfg) == bytes(ref)          # n_elem is the only field the keyword moves


@pytest.mark.parametrize("n", [0, 1, 127, 200, -40])
def test_out_of_range_n_elems_raise(n):
    with pytest.raises(ValueError, match="n_elems"):
        _capi.arm_push_config(1, n_elems=n)


@pytest.mark.parametrize("make", [
    lambda: VecArmPullWeightEnv(2, n_elems=100),
    lambda: VecArmPullWeightEnv(2, n_elems=20),
    lambda: gsa.make_vec("OctoArmPullWeight-v0", 2, n_elems=64),
    lambda: ArmPullWeightEnv(n_elems=100),
], ids=["vec-100", "vec-20", "make_vec-64", "single-100"])
def test_pull_weight_refuses_other_lengths(make):
    with pytest.raises(ValueError, match="n_elems must be 40"):
        make()


def test_n_elems_is_keyword_only_on_the_vec_env():
    import inspect

    p = inspect.signature(VecArmPushEnv.__init__).parameters["n_elems"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 40
    p = inspect.signature(ArmPushEnv.__init__).parameters["n_elems"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 40


@pytest.mark.parametrize("mode", ["discrete", "continuous"])
def test_oracle_backend_vec_env_at_100_elements(oracle_built, mode):
    """The env wiring at 100 elements (radii, muscle layers, observation width) through the oracle backend, against
    oracle rods built by hand from the same tables."""
    from tests.oracle_backend import OracleBackend

    N, n = 3, 100
    env = gsa.make_vec("OctoArmPush-v0", N, mode=mode, n_elems=n,
                       backend=OracleBackend(_capi.arm_push_config(N, mode=mode, n_elems=n)), numpy_output=True)
    assert env.n_elem == n and env.obs_dim == 204 and env.single_observation_space.shape == (204,)
    obs, _ = env.reset(seed=0)
    assert obs.shape == (N, 204)
    cfg1 = _capi.arm_push_config(1, mode=mode, n_elems=n)
    radii = _capi.arm_push_radii(n)
    rods = []
    for _ in range(N):
        r = oracle_built.OracleRod(cfg1)
        r.set_radius_profile(radii)
        r.set_muscle_layers(*_capi.es_muscle_layers(radii, 0.012))
        np.testing.assert_array_equal(r.reset_push(), obs[0])
        rods.append(r)
    rng = np.random.default_rng(0)
    for t in range(2):
        if mode == "discrete":
            a = np.array([0, 1, 0], np.float32).reshape(N, 1)
        else:
            a = rng.uniform(0.0, 1.0, (N, 2)).astype(np.float32)
            a[:, 1] *= 0.5
        obs, rew, term, trunc, _ = env.step(a)
        for i, r in enumerate(rods):
            o, rw, te, tr = r.env_step_push(a[i])
            np.testing.assert_array_equal(obs[i], o)
            assert rew[i] == rw and bool(term[i]) == te and bool(trunc[i]) == tr
    assert np.isfinite(obs).all() and np.abs(obs[:, :n + 1] - np.linspace(0, 0.2, n + 1)).max() > 1e-6
    env.close()


def test_single_env_observation_follows_n_elems(oracle_built):
    from tests.oracle_backend import OracleBackend

    env = ArmPushEnv(mode="continuous", n_elems=64,
                     backend=OracleBackend(_capi.arm_push_config(1, mode="continuous", n_elems=64)))
    assert env.n_elem == 64 and env.observation_space.shape == (2 * 65 + 2,)
    obs, _ = env.reset()
    assert obs.shape == (132,)
    obs, *_ = env.step(np.array([0.5, 0.3], np.float32))
    assert obs.shape == (132,) and np.isfinite(obs).all()
    env.close()
