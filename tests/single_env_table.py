"""What the ten public single-env classes (the N = 1 drop-ins of gym_softrobot_amd.envs) hand back, as a table
shared by tests/test_single_env_shell.py (CPU, oracle-backed test double) and tests/test_gpu_env_api.py (HIP backend).

Every literal was RECORDED from a run of the commit before the single-env classes were given one shell
(`SingleRodEnv`), when each class still carried its own reset / step / get_state: the table pins that behaviour, it
does not describe the new code.  Per class:

  id          the registered id `make` builds the class from (its registered kwargs are the defaults used here)
  config      the softrod_config of that id for one env (the test double is built from it)
  signature   str(inspect.signature(cls))
  obs         (dtype, shape) of the observation of reset / step / get_state, or {key: (dtype, shape)} for a dict
  info        {key: type} of step's info
  counters    the host counters after two steps: {attribute: (type, value)}
  prev_action None (no such attribute), "caller" (the caller's own object) or the shape it is reshaped to
  shares_rng  reset hands env.np_random to the one-env batch (classes whose build draws nothing do not)
  material, contact, summary   the class has set_material / set_contact / summary()
"""
import inspect

import numpy as np

from gym_softrobot_amd import _capi

F32, F64 = "float32", "float64"
_TIMED = {"time": np.float64, "TimeLimit.truncated": bool}
_KW = "*, device: 'int' = 0, math_mode: 'int' = 1, backend=None"


def _mocto(kind):
    return lambda: _capi.muscle_octopus_config(kind, 1)


TABLE = {
    "SoftPendulumEnv": dict(
        id="SoftPendulum-v0", config=lambda: _capi.softpendulum_config(1),
        signature="(final_time=5.0, time_step=0.0001, recording_fps=25, n_elems=50, config_generate_video=False, "
                  f"render_mode: 'Optional[str]' = None, {_KW})",
        obs=(F32, (4,)), info=_TIMED, counters={"time": (np.float64, 0.07999999999999935), "counter": (int, 2)},
        prev_action=None, shares_rng=True, material=True, contact=False, summary=False),
    "SoftPendulum3DEnv": dict(
        id="SoftPendulum3D-v0", config=lambda: _capi.softpendulum3d_config(1),
        signature="(final_time: 'float' = 5.0, time_step: 'float' = 0.0001, recording_fps: 'int' = 25, n_elems: 'int' = 50, "
                  f"config_generate_video: 'bool' = False, render_mode: 'Optional[str]' = None, {_KW})",
        obs=(F32, (9,)), info={"time": np.float64, "tilt": float},
        counters={"time": (np.float64, 0.07999999999999935), "counter": (int, 2)},
        prev_action=None, shares_rng=True, material=True, contact=False, summary=False),
    "ArmSingleEnv": dict(
        id="OctoArmSingle-v0", config=lambda: _capi.arm_single_config(1),
        signature="(final_time=10.0, time_step=7e-05, recording_fps=20, n_elems=50, n_action=7, control_penalty_coeff=0.001, "
                  f"config_generate_video=False, policy_mode='centralized', render_mode: 'Optional[str]' = None, {_KW})",
        obs=(F32, (25,)), info=_TIMED, counters={"time": (np.float64, 0.09995999999999342), "counter": (int, 2)},
        prev_action=None, shares_rng=False, material=True, contact=True, summary=True),
    "FlatEnv": dict(
        id="OctoFlat-v0", config=lambda: _capi.octo_flat_config(1),
        signature="(final_time=5.0, time_step=7e-05, recording_fps=5, n_elems=10, n_arm=8, n_action=3, config_generate_video=False, "
                  f"config_save_head_data=False, policy_mode='centralized', render_mode: 'Optional[str]' = None, {_KW})",
        obs={"individual": (F32, (8, 56)), "shared": (F32, (13,))}, info=_TIMED,
        counters={"time": (np.float64, 0.3999800000000456), "counter": (int, 2)},
        prev_action=None, shares_rng=True, material=False, contact=True, summary=True),
    "SoftArmTrackingEnv": dict(
        id="SoftArmTracking-v0", config=lambda: _capi.soft_arm_config(1),
        signature=f"(game_mode: 'int' = 1, render_mode: 'Optional[str]' = None, {_KW})",
        obs=(F64, (14,)), info={"ctime": np.float64},
        counters={"tick": (int, 100), "time_tracker": (np.float64, 0.019999999999999934)},
        prev_action=None, shares_rng=True, material=False, contact=False, summary=False),
    "ArmPushEnv": dict(
        id="OctoArmPush-v0", config=lambda: _capi.arm_push_config(1),
        signature="(final_time: 'float' = 2.5, time_step: 'float' = 5e-05, recording_fps: 'int' = 40, mode: 'str' = 'discrete', "
                  "config_generate_video: 'bool' = False, config_early_termination: 'bool' = False, "
                  f"render_mode: 'Optional[str]' = None, {_KW}, n_elems: 'int' = 40)",
        obs=(F32, (84,)), info=_TIMED, counters={"time": (np.float64, 0.04999999999999857)},
        prev_action="caller", shares_rng=False, material=False, contact=False, summary=False),
    "ArmPullWeightEnv": dict(
        id="OctoArmPullWeight-v0", config=lambda: _capi.arm_pull_weight_config(1, mode="continuous"),
        signature="(**kwargs)",
        obs=(F32, (84,)), info=_TIMED, counters={"time": (np.float64, 0.04999999999999653)},
        prev_action="caller", shares_rng=False, material=False, contact=False, summary=False),
    "CrawlEnv": dict(
        id="OctoCrawl-v0", config=_mocto(_capi.ENV_CRAWL),
        signature="(final_time=10.0, time_step=5e-05, recording_fps=25, n_elems=20, config_random_final_time=False, "
                  "render_mode: 'Optional[str]' = None, **kw)",
        obs=(F32, (1048,)), info=_TIMED, counters={"time": (np.float64, 0.07999999999999527), "counter": (int, 2)},
        prev_action=(8, 3), shares_rng=True, material=False, contact=False, summary=False),
    "ArmTwoEnv": dict(
        id="OctoArmTwo-v0", config=_mocto(_capi.ENV_ARM_TWO),
        signature="(final_time=5.0, time_step=5e-05, recording_fps=25, n_elems=20, render_mode: 'Optional[str]' = None, **kw)",
        obs=(F32, (104,)), info=_TIMED, counters={"time": (np.float64, 0.07999999999999527), "counter": (int, 2)},
        prev_action=(2, 9), shares_rng=True, material=False, contact=False, summary=False),
    "ReachEnv": dict(
        id="OctoReach-v0", config=_mocto(_capi.ENV_REACH),
        signature="(final_time=5.0, time_step=5e-05, recording_fps=25, n_elems=20, render_mode: 'Optional[str]' = None, **kw)",
        obs=(F32, (1512,)), info=_TIMED, counters={"time": (np.float64, 0.07999999999999527), "counter": (int, 2)},
        prev_action=(8, 60), shares_rng=True, material=False, contact=False, summary=False),
}
NAMES = list(TABLE)
# host counters any of the classes keeps: a class has exactly those its `counters` entry names
COUNTERS = ("time", "counter", "tick", "time_tracker")


def sample_action(env):
    """An action every class accepts: 1 for Discrete(2), else 0.25 in every entry (FlatEnv's step takes all
    n_arm * n_action values whatever its declared space)."""
    sp = env.action_space
    if not hasattr(sp, "low"):
        return 1
    n = env.n_arm * env.n_action if type(env).__name__ == "FlatEnv" else sp.shape[0]
    return np.full(n, 0.25, sp.dtype)


def assert_obs(ob, want, what):
    if isinstance(want, dict):
        assert type(ob) is dict and list(ob) == list(want), what
        for k, w in want.items():
            assert_obs(ob[k], w, f"{what}[{k}]")
        return
    assert type(ob) is np.ndarray and (str(ob.dtype), ob.shape) == want, (what, type(ob), ob.dtype, ob.shape)
    assert ob.flags.owndata, what                      # the caller's own copy, never a view of the batch's buffer


def check_api(env, name, seed):
    """reset(seed), two steps, get_state on a freshly built `env` of class `name`, against TABLE[name].  Returns the
    action stepped with and the second step's result."""
    case = TABLE[name]
    assert type(env).__name__ == name and str(inspect.signature(type(env))) == case["signature"]
    ob, info = env.reset(seed=seed)
    assert_obs(ob, case["obs"], "reset")
    assert type(info) is dict and info == {}
    assert (env._vec._rngs[0] is env.np_random) == case["shares_rng"]
    action = sample_action(env)
    for _ in range(2):
        out = env.step(action)
    ob, reward, terminated, truncated, info = out
    assert_obs(ob, case["obs"], "step")
    assert (type(reward), type(terminated), type(truncated)) == (float, bool, bool)
    assert type(info) is dict and {k: type(v) for k, v in info.items()} == case["info"]
    assert list(info) == list(case["info"])
    assert_obs(env.get_state(), case["obs"], "get_state")
    assert {k for k in COUNTERS if hasattr(env, k)} == set(case["counters"])
    for k, (typ, value) in case["counters"].items():
        assert type(getattr(env, k)) is typ and getattr(env, k) == value, (k, getattr(env, k))
    first = next(iter(info))                   # "time" / "ctime": the float64 host clock itself
    assert info[first] is getattr(env, "time" if "time" in case["counters"] else "time_tracker")
    pa = case["prev_action"]
    if pa is None:
        assert not hasattr(env, "_prev_action")
    elif pa == "caller":
        assert env._prev_action is action
    else:
        assert type(env._prev_action) is np.ndarray and env._prev_action.dtype == np.float32
        assert env._prev_action.shape == pa and (env._prev_action == 0.25).all()
    assert (hasattr(env, "set_material"), hasattr(env, "set_contact"), hasattr(env, "summary")) == \
        (case["material"], case["contact"], case["summary"])
    return action, out
