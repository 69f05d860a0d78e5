"""The N = 1 drop-in classes behave as they did before they shared one shell (envs/base.py `SingleRodEnv`).

CPU only, on the oracle-backed test double with the substep count lowered (host logic does not depend on it).  Every
literal here and in tests/single_env_table.py was recorded from a run of the parent commit — the one in which each of
the ten classes still had its own reset / step / get_state / render / close — and the tests passed there unchanged:
they pin that behaviour for the shell."""
import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd.envs import base

from .oracle_backend import OracleBackend
from .single_env_table import COUNTERS, NAMES, TABLE, assert_obs, check_api, sample_action


def _make(name, n_substeps=2, **kw):
    cfg = TABLE[name]["config"]()
    cfg.n_substeps = n_substeps            # keep the CPU suite quick, as tests/test_host_logic.py does
    return gsa.make(TABLE[name]["id"], backend=OracleBackend(cfg), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_api_table_counters_and_second_reset(oracle_built, name):
    case = TABLE[name]
    env = _make(name)
    assert isinstance(env, base.GymEnv) and env.unwrapped is env
    action, _ = check_api(env, name, seed=3)
    rng = env.np_random
    ob, info = env.reset()                                         # no seed: the counters restart, the stream goes on
    assert_obs(ob, case["obs"], "second reset")
    assert info == {} and env.np_random is rng
    assert (env._vec._rngs[0] is env.np_random) == case["shares_rng"]
    for k in COUNTERS:
        if k in case["counters"]:
            typ = case["counters"][k][0]
            assert type(getattr(env, k)) is typ and getattr(env, k) == 0
    if case["prev_action"] is not None:                            # reset leaves _prev_action alone
        assert (env._prev_action is action) if case["prev_action"] == "caller" else (env._prev_action == 0.25).all()
    env.close()


# the instance attributes each class sets (render.py and callers read them), beside _vec and the Gymnasium base's own
ATTRS = {
    "SoftPendulumEnv": "action_space config_generate_video counter final_time n_action n_elems n_seg observation_space recording_fps render_mode reward_range step_skip time time_step total_steps",
    "SoftPendulum3DEnv": "action_space base_limit base_step counter final_time n_action n_elems observation_space recording_fps render_mode step_skip time time_step total_steps",
    "ArmSingleEnv": "_target action_space control_penalty_coeff counter final_time kappa_range kappa_rate_range n_action n_elems n_seg observation_space policy_mode recording_fps render_mode reward_range step_skip time time_step total_steps",
    "FlatEnv": "_observation_size action_space counter final_time n_action n_arm n_elems n_seg observation_space policy_mode recording_fps render_mode reward_range step_skip time time_step total_steps",
    "SoftArmTrackingEnv": "RL_update_interval action_space base_length max_episode_final_time mode n_elem num_steps_per_update number_of_control_points number_of_observation_segments observation_space radius render_mode sim_dt target_location target_v_scale tick time_tracker torque_scale youngs_modulus",
    "ArmPushEnv": "_observation_size _prev_action action_space config_early_termination config_generate_video final_time mode n_elem observation_space recording_fps render_mode step_skip time time_step total_steps",
    "ArmPullWeightEnv": "_observation_size _prev_action action_space config_early_termination config_generate_video final_time mode n_elem observation_space recording_fps render_mode step_skip time time_step total_steps",
    "CrawlEnv": "_observation_size _prev_action action_space config_random_final_time counter final_time n_action n_agent n_arm n_elems n_seg observation_space recording_fps render_mode reward_range step_skip time time_step total_steps",
    "ArmTwoEnv": "_observation_size _prev_action action_space control_location counter final_time n_action n_arm n_elems n_seg n_sucker observation_space recording_fps render_mode reward_range step_skip sucker_location time time_step total_steps",
    "ReachEnv": "_observation_size _prev_action action_space counter final_time n_action n_arm n_elems n_muscle n_seg observation_space recording_fps render_mode reward_range step_skip time time_step total_steps",
}


@pytest.mark.parametrize("name", NAMES)
def test_instance_attributes_and_mirrored_timing(oracle_built, name):
    env = _make(name)
    assert " ".join(sorted(k for k in vars(env) if k not in ("_vec", "_np_random", "_np_random_seed"))) == ATTRS[name]
    for k in ("final_time", "time_step", "total_steps", "recording_fps", "step_skip"):
        assert hasattr(env, k) == (name != "SoftArmTrackingEnv")
        if hasattr(env, k):
            assert type(getattr(env, k)) is type(getattr(env._vec, k)) and getattr(env, k) == getattr(env._vec, k)
    env.close()


def test_capabilities_by_class():
    got = {name: (hasattr(getattr(gsa, name), "set_material"), hasattr(getattr(gsa, name), "set_contact")) for name in NAMES}
    assert got == {
        "SoftPendulumEnv": (True, False), "SoftPendulum3DEnv": (True, False), "ArmSingleEnv": (True, True),
        "FlatEnv": (False, True), "SoftArmTrackingEnv": (False, False), "ArmPushEnv": (False, False),
        "ArmPullWeightEnv": (False, False), "CrawlEnv": (False, False), "ArmTwoEnv": (False, False),
        "ReachEnv": (False, False)}
    assert {name for name in NAMES if hasattr(getattr(gsa, name), "summary")} == {"ArmSingleEnv", "FlatEnv"}
    assert gsa.ArmPushEnv.parity_label == gsa.CrawlEnv.parity_label and "parity-unpinned" in gsa.ReachEnv.parity_label


@pytest.mark.parametrize("name, first, second", [
    ("FlatEnv", [0.6284737507154365, 0.8552157598941496], [1.7019116978095954, 1.3732430540965517]),
    ("ReachEnv", [0.02141229178590609, 0.059202626649024925, 0.20031861630159922],
     [0.14554050901609195, 0.023532160560099796, 0.10828173505911845]),
])
def test_second_reset_without_a_seed_continues_the_stream(oracle_built, name, first, second):
    env = _make(name)
    env.reset(seed=3)
    assert env._target.dtype == np.float64 and env._target.tolist() == first
    env.reset()
    assert env._target.tolist() == second
    # the draws are env.np_random's own: the stream of seed 3, two resets on
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(3)))
    rng.random(len(first)), rng.random(len(first))
    assert env.np_random.random() == rng.random()
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_bad_render_mode(oracle_built, name):
    with pytest.raises(ValueError, match="^Unsupported render mode: ascii$"):
        _make(name, render_mode="ascii")


def test_action_validation_errors(oracle_built):
    env = _make("ArmPushEnv")
    env.reset(seed=0)
    with pytest.raises(NotImplementedError, match="^Action must be 1 or 0$"):          # arm_push_env.py:267
        env.step(2)
    assert env.time == 0.0 and (env._prev_action == 0).all()                            # nothing was booked
    env.close()
    env = _make("SoftPendulum3DEnv")
    env.reset(seed=0)
    with pytest.raises(ValueError) as exc:                                               # soft_pendulum_3d.py:116-117
        env.step(np.array([2.0, 0.0], np.float32))
    assert str(exc.value) == "Action array([2., 0.], dtype=float32) is outside Box(-1.0, 1.0, (2,), float32)"
    assert env.counter == 0
    env.close()
    with pytest.raises(TypeError) as exc:                                                # arm_push_env.py:518
        gsa.ArmPullWeightEnv(time_step=1e-5)
    assert str(exc.value) == "__init__() got multiple values for keyword argument 'time_step'"


def test_softpendulum_prints_its_nan_line_on_termination(oracle_built, capsys):
    env = _make("SoftPendulumEnv")
    env.reset(seed=0)
    capsys.readouterr()
    _, _, terminated, _, _ = env.step(np.array([np.nan], np.float32))
    assert terminated is True
    assert capsys.readouterr().out == " Nan detected in, exiting simulation now. self.time=np.float64(0.04000000000000063)\n"
    env.close()


SUMMARY = {
    "ArmSingleEnv": "\n        self.final_time=10.0\n        self.time_step=7e-05\n        self.total_steps=142857\n        self.step_skip=714\n        simulation time per action: 1.0/self.step_skip=0.0014005602240896359\n        max number of action per episode: 200.07983193277312\n\n        self.n_elems=50\n        self.action_space=Box(-22.0, 22.0, (7,), float32)\n        self.observation_space=Box(-inf, inf, (25,), float32)\n        self.reward_range=10.0\n        \n",
    "FlatEnv": "\n        self.final_time=5.0\n        self.time_step=7e-05\n        self.total_steps=71428\n        self.step_skip=2857\n        simulation time per action: 1.0/self.step_skip=0.00035001750087504374\n        max number of action per episode: 25.001050052502624\n\n        self.n_elems=10\n        self.action_space=Box(-22.0, 22.0, (24,), float32)\n        self.observation_space=Dict('individual': Box(-inf, inf, (8, 56), float32), 'shared': Box(-inf, inf, (13,), float32))\n        self.reward_range=100.0\n        \n",
}


@pytest.mark.parametrize("name", sorted(SUMMARY))
def test_summary_prints_what_it_printed(oracle_built, capsys, name):
    env = _make(name)
    capsys.readouterr()
    env.summary()
    assert capsys.readouterr().out == SUMMARY[name]
    env.close()


def test_sample_action_is_in_every_declared_space(oracle_built):
    for name in NAMES:
        env = _make(name)
        a = sample_action(env)
        assert name == "FlatEnv" or env.action_space.contains(a), name
        env.close()
