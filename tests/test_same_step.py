"""autoreset="same_step" without a GPU: the two C-ABI entry points are declared and listed, the ABI version stands, the
mode is accepted / refused where it should be, and — against a small recording stand-in backend — the top-up cadence is
halved, the info keys have their shapes, and fork() / state_dict() / ShardedVecEnv refuse the mode."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from tests.oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
KW = dict(final_time=5e-4, time_step=1e-4, recording_fps=5000, n_elems=6)     # episodes of three env.steps


def test_entry_points_are_declared_and_listed_without_an_abi_bump():
    header = (ROOT / "include" / "softrod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("softrod_autoreset_same_step", "softrod_final_view"):
        assert re.search(rf"\bint {name}\s*\(softrod_handle\* h,", code), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert name in header.split("Device-side auto-reset")[1].split("*/")[0], f"{name}: not in the auto-reset block"
    assert _capi.ABI_VERSION == 17 and "#define SOFTROD_ABI_VERSION 17" in header


def test_the_library_exports_them_and_refuses_a_null_handle(hip_lib):
    assert hip_lib.softrod_autoreset_same_step(None, 1) == -1
    p = [_capi.C.c_void_p() for _ in range(3)]
    assert hip_lib.softrod_final_view(None, *(_capi.C.byref(x) for x in p)) == -1


def test_unknown_modes_are_still_refused_and_the_message_names_the_new_one():
    cfg = _capi.softpendulum_config(2, **KW)
    with pytest.raises(ValueError, match="same_step"):
        gsa.VecSoftPendulumEnv(2, backend=OracleBackend(cfg), autoreset="bogus", **KW)


def test_a_backend_without_the_entry_point_refuses_before_anything_is_staged():
    be = OracleBackend(_capi.softpendulum_config(2, **KW))
    with pytest.raises(NotImplementedError, match="same-step auto-reset needs the HIP backend, not OracleBackend"):
        gsa.VecSoftPendulumEnv(2, backend=be, autoreset="same_step", **KW)
    assert getattr(be, "queue_depth", 0) == 0          # autoreset_enable was not reached


def test_soft_arm_tracking_game_mode_2_refuses():
    for mode in ("device", "same_step"):
        with pytest.raises(NotImplementedError, match="game_mode 2"):
            gsa.VecSoftArmTrackingEnv(1, game_mode=2, backend=OracleBackend(_capi.soft_arm_config(1)), autoreset=mode)


class StubBackend:
    """Records what VecRodEnvBase asks of a backend in the device auto-reset modes; CPU tensors of the right shapes.
    Every env `finishes` on every third step."""

    def __init__(self, cfg, aux_dim=0):
        self.cfg = cfg.copy()
        self.n_envs = n = int(cfg.n_envs)
        self.device = torch.device("cpu")
        self.obs_dim = _capi.config_obs_dim(cfg)
        self.calls = []
        self.obs = torch.zeros((n, self.obs_dim), dtype=torch.float32)
        self.reward = torch.zeros(n, dtype=torch.float64)
        self.terminated = torch.zeros(n, dtype=torch.uint8)
        self.truncated = torch.zeros(n, dtype=torch.uint8)
        self.aux = torch.zeros((n, aux_dim), dtype=torch.float64) if aux_dim else None
        self.time = torch.zeros(n, dtype=torch.float64)
        self.consumed = np.zeros(n, np.int32)
        self.steps = 0

    def autoreset_enable(self, depth):
        self.calls.append(("autoreset_enable", depth))
        self.queue_depth = depth

    def autoreset_same_step(self, on=True):
        assert self.calls and self.calls[-1][0] == "autoreset_enable"
        self.calls.append(("autoreset_same_step", on))
        n = self.n_envs
        self.final_obs = torch.zeros((n, self.obs_dim), dtype=torch.float32)
        self.final_time = torch.zeros(n, dtype=torch.float64)
        self.final_aux = torch.zeros(n, dtype=torch.float64)

    def reset(self, theta0, mask=None):
        self.calls.append(("reset",))

    reset_straight = lambda self, *a, **k: self.calls.append(("reset",))      # noqa: E731

    def queue_push(self, theta0, counts):
        self.calls.append(("queue_push", np.asarray(counts).copy()))

    queue_push_straight = lambda self, s, d, n, counts: self.calls.append(("queue_push", np.asarray(counts).copy()))  # noqa: E731

    def queue_status(self):
        return self.consumed.copy(), 0

    def queue_advance(self, by):
        pass

    def observe(self, prev_action=None):
        return self.obs

    def state(self):
        return {"time": self.time}

    def step(self, a):
        self.steps += 1
        self.calls.append(("step",))
        done = self.steps % 3 == 0
        self.truncated[:] = int(done)
        if done:
            self.consumed += 1
        return self.obs, self.reward, self.terminated, self.truncated

    def step_packed(self, a, out=None):
        from gym_softrobot_amd.distributed import packed_width

        self.step(a)
        return torch.zeros((self.n_envs, packed_width(self.obs_dim)), dtype=torch.float32)

    def close(self):
        pass


def _stub_env(mode, n=4, **extra):
    cfg = _capi.softpendulum_config(n, **KW)
    return gsa.VecSoftPendulumEnv(n, backend=StubBackend(cfg), autoreset=mode, **KW, **extra)


def test_top_up_cadence_is_halved_in_same_step_mode_only():
    dev, same = _stub_env("device"), _stub_env("same_step")
    assert dev.device_autoreset and same.device_autoreset and same.same_step and not dev.same_step
    assert [c[0] for c in same.backend.calls[:2]] == ["autoreset_enable", "autoreset_same_step"]
    assert all(c[0] != "autoreset_same_step" for c in dev.backend.calls)
    assert dev.queue_depth == same.queue_depth == 32
    assert dev.top_up_every == 30 and same.top_up_every == 15
    for depth, every_dev, every_same in ((3, 1, 1), (4, 2, 1), (5, 3, 1), (6, 4, 2), (16, 14, 7)):
        dev.queue_depth = same.queue_depth = depth
        assert (dev.top_up_every, same.top_up_every) == (every_dev, every_same), depth
        # an env may use one record per step: fewer than 2 * top_up_every steps lie between a reading of the counters
        # and the end of the next top-up, and depth - 1 records are certainly staged at the reading
        assert 2 * same.top_up_every - 1 <= depth - 1


def test_the_queue_is_topped_up_at_the_halved_deadline():
    env = _stub_env("same_step")
    env.queue_depth = 8                                  # top_up_every 3
    env.reset(seed=0)
    be = env.backend
    first = len(be.calls)
    a = np.zeros(4, np.float32)
    for _ in range(9):
        env.step(a)
    kinds = [c[0] for c in be.calls[first:]]
    steps_before_push = [kinds[:i].count("step") for i, k in enumerate(kinds) if k == "queue_push"]
    assert steps_before_push == [3, 6, 9]                # (envs finish on steps 3, 6, 9: a record each to restage)


@pytest.mark.parametrize("numpy_output", [False, True])
def test_info_keys_and_shapes(numpy_output):
    n = 4
    env = _stub_env("same_step", n=n, numpy_output=numpy_output)
    env.reset(seed=0)
    a = np.zeros(n, np.float32)
    for k in range(1, 4):
        obs, rew, term, trunc, info = env.step(a)
        assert set(info) == {"time", "TimeLimit.truncated", "final_obs", "_final_obs", "final_info"}
        assert set(info["final_info"]) == {"time"}
        assert tuple(info["final_obs"].shape) == (n, env.obs_dim) and tuple(obs.shape) == (n, env.obs_dim)
        assert tuple(info["_final_obs"].shape) == (n,) and tuple(info["final_info"]["time"].shape) == (n,)
        kind = np.ndarray if numpy_output else torch.Tensor
        for v in (info["final_obs"], info["_final_obs"], info["final_info"]["time"], info["time"]):
            assert isinstance(v, kind)
        fo, flag, ft = (np.asarray(v) for v in (info["final_obs"], info["_final_obs"], info["final_info"]["time"]))
        assert fo.dtype == np.float32 and flag.dtype == np.bool_ and ft.dtype == np.float64
        assert flag.tolist() == [k == 3] * n and np.asarray(trunc).tolist() == [k == 3] * n
    packed, pinfo = env.step_packed(a)
    assert set(pinfo) == {"final_obs"} and tuple(pinfo["final_obs"].shape) == (n, env.obs_dim)
    # the NEXT_STEP device mode keeps its two keys, and its packed info stays empty
    dev = _stub_env("device", n=n, numpy_output=numpy_output)
    dev.reset(seed=0)
    assert set(dev.step(a)[4]) == {"time", "TimeLimit.truncated"}
    assert dev.step_packed(a)[1] == {}


def test_soft_pendulum_3d_carries_the_tilt_beside_the_final_observation():
    n = 3
    kw = dict(final_time=6e-4, time_step=1e-4, recording_fps=5000, n_elems=6)
    cfg = _capi.softpendulum3d_config(n, **kw)
    env = gsa.VecSoftPendulum3DEnv(n, backend=StubBackend(cfg, aux_dim=1), autoreset="same_step", **kw)
    env.reset(seed=0)
    info = env.step(np.zeros((n, 2), np.float32))[4]
    assert tuple(info["tilt"].shape) == (n,) and set(info["final_info"]) == {"time", "tilt"}
    assert tuple(info["final_info"]["tilt"].shape) == (n,) and info["final_info"]["tilt"].dtype == torch.float64


def test_fork_state_dict_and_the_sharded_env_refuse_the_mode():
    from gym_softrobot_amd.distributed import ShardedVecEnv

    env = _stub_env("same_step")
    with pytest.raises(NotImplementedError, match="autoreset='same_step'"):
        env.fork(0, [1, 2])
    with pytest.raises(NotImplementedError, match="autoreset='same_step'"):
        env.state_dict()
    with pytest.raises(NotImplementedError, match="same_step"):
        ShardedVecEnv(env, env.num_envs)
    dev = _stub_env("device")
    with pytest.raises(NotImplementedError, match="autoreset='device'"):
        dev.fork(0, [1, 2])
    ShardedVecEnv(dev, dev.num_envs, gather=False)       # the NEXT_STEP device mode is still taken
