"""Observation and reward normalisation on the GPU (csrc/softrod_normalize.hpp, softrod_normalize_*): the kernels
against their NumPy twin (tests/normalize_ref.py) on synthetic rows at the sizes that cross the tile (64 columns) and
partial (16 rows) edges, in all three modes; through the env under the four reset modes; frozen statistics; the state
round trip; inside a captured graph; off; the refusals that need a handle.  Every comparison with the twin is BITWISE:
float64 arrays as uint64, float32 arrays as uint32."""
import ctypes as C

import numpy as np
import pytest

from tests.normalize_ref import ARRAYS, MANUAL, NEXT_STEP, SAME_STEP, NormalizeRef

pytestmark = pytest.mark.gpu

STATS = ("obs_mean", "obs_var", "obs_count", "obs_inv_std", "ret_mean", "ret_var", "ret_count", "ret_inv_std")


@pytest.fixture(scope="module")
def torch_gpu(hip_lib):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def backends(torch_gpu):
    """One OctoArmPush handle per (n_elems, batch size), shared by the modes (the pass never looks at the rods):
    obs_dim = 2 * (n_elems + 1) + 2."""
    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    made = {}

    def get(n_elems, n):
        if (n_elems, n) not in made:
            made[n_elems, n] = HipRodBackend(_capi.arm_push_config(n, n_elems=n_elems), 0)
        return made[n_elems, n]

    yield get
    for be in made.values():
        be.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(t):
    return t.cpu().numpy().copy() if hasattr(t, "cpu") else np.array(t)


def _snapshot(torch, be):
    torch.cuda.synchronize()
    return {k: _host(be.normalize[k]) for k in (*ARRAYS, "norm_final_obs")}


def _assert_equals_twin(torch, be, ref, where):
    got = _snapshot(torch, be)
    for name in (*ARRAYS, "norm_final_obs"):
        want = getattr(ref, name)
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (where, name)
        assert np.array_equal(_bits(got[name]), _bits(want)), f"{where}: {name} differs from the twin"
    return got


PLAN = ("random", "random", "random", "all", "random", "random", "none", "bad", "random", "frozen", "random", "random")


def _sequence(torch, be, mode, seed, ref=None):
    """12 calls of seeded rows on handle `be`: flags with probability 0.3, one call with every flag, one with none, one
    with a NaN row and an inf element, one with update = 0; in the manual mode a masked reset after every third call.
    With `ref` every resident array is compared with the twin after every call.  Returns the snapshots."""
    n, d = be.n_envs, be.obs_dim
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=be.device)      # noqa: E731
    be.normalize_enable(True, True, gamma=0.97, clip_obs=2.5, clip_reward=1.5, epsilon=1e-6, mode=mode, in_step=False)
    rng = np.random.default_rng(seed)
    scale, shift = 10.0 ** rng.uniform(-2, 2, d), rng.uniform(-5, 5, d)
    rows = lambda: (rng.standard_normal((n, d)) * scale + shift).astype(np.float32)     # noqa: E731
    shots = []
    first = rows()
    be.normalize_reset(dev(first))
    if ref is not None:
        ref.reset(first)
        shots.append(_assert_equals_twin(torch, be, ref, "first reset"))
    for c, kind in enumerate(PLAN):
        obs, reward = rows(), rng.standard_normal(n) * 3.0 + 1.0
        if kind in ("all", "none"):
            te, tr = np.full(n, kind == "all"), np.zeros(n, bool)
        else:
            te, tr = rng.random(n) < 0.3, rng.random(n) < 0.3
        if kind == "bad":
            obs[0, :] = np.nan
            obs[n - 1, d // 2] = np.inf if n > 1 else obs[n - 1, d // 2]
            if n > 2:
                obs[1, d - 1] = -np.inf
        final = rows() if mode == SAME_STEP else None
        update = kind != "frozen"
        if kind == "all" and mode == MANUAL:            # every env open, so that every env finishes on this call
            be.normalize_reset(dev(obs), None, False)
            if ref is not None:
                ref.reset(obs, None, False)
        be.normalize_step(dev(obs), dev(reward), dev(te.astype(np.uint8)), dev(tr.astype(np.uint8)),
                          None if final is None else dev(final), mode, update)
        if ref is not None:
            ref.step(obs, reward, te, tr, final, mode, update)
            shots.append(_assert_equals_twin(torch, be, ref, f"call {c} ({kind})"))
        else:
            shots.append(_snapshot(torch, be))
        if mode == MANUAL and c % 3 == 2:
            mask, again = rng.random(n) < 0.5, rows()
            be.normalize_reset(dev(again), mask)
            if ref is not None:
                ref.reset(again, mask)
                shots.append(_assert_equals_twin(torch, be, ref, f"masked reset after call {c}"))
            else:
                shots.append(_snapshot(torch, be))
    be.normalize_enable(False, False)
    assert be.normalize is None
    return shots


@pytest.mark.parametrize("mode", [MANUAL, NEXT_STEP, SAME_STEP])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1025])
@pytest.mark.parametrize("n_elems", [2, 30, 31, 63])
def test_kernels_equal_the_twin(torch_gpu, backends, n_elems, n, mode):
    """obs_dim 8, 64, 66, 130: a sub-tile, one full tile, a tile plus two columns, three tiles with a ragged end;
    N = 1, 15, 16, 17, 1025: fewer rows than partials, exactly 16, one over, a ragged tail."""
    be = backends(n_elems, n)
    assert be.obs_dim == 2 * (n_elems + 1) + 2
    ref = NormalizeRef(n, be.obs_dim, gamma=0.97, clip_obs=2.5, clip_reward=1.5, epsilon=1e-6)
    shots = _sequence(torch_gpu, be, mode, 1000 * n + 10 * n_elems + mode, ref)
    assert ref.obs_count[0] > n and ref.ret_count[0] > 1.0 and np.isfinite(ref.obs_mean).all() and np.isfinite(ref.obs_var).all()
    assert any(np.isnan(s["norm_obs"]).any() for s in shots)            # the NaN row came out as NaN


def test_two_runs_are_bitwise_equal(torch_gpu, backends):
    for mode in (MANUAL, NEXT_STEP, SAME_STEP):
        a = _sequence(torch_gpu, backends(63, 1025), mode, 7)
        b = _sequence(torch_gpu, backends(63, 1025), mode, 7)
        assert len(a) == len(b) >= len(PLAN)
        for i, (x, y) in enumerate(zip(a, b)):
            for k in x:
                assert np.array_equal(_bits(x[k]), _bits(y[k])), (mode, i, k)


def test_obs_only_and_reward_only(torch_gpu, backends):
    """With one half off its arrays stay as enable left them; the latch moves either way."""
    torch = torch_gpu
    be = backends(31, 17)
    n, d = be.n_envs, be.obs_dim
    rng = np.random.default_rng(5)
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=be.device)      # noqa: E731
    for obs_on, reward_on in ((True, False), (False, True)):
        be.normalize_enable(obs_on, reward_on, mode=NEXT_STEP, in_step=False)
        ref = NormalizeRef(n, d, obs_on, reward_on)
        for c in range(4):
            obs, reward = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal(n)
            te = rng.random(n) < 0.4
            be.normalize_step(dev(obs), dev(reward), dev(te.astype(np.uint8)), dev(np.zeros(n, np.uint8)), None, NEXT_STEP, True)
            ref.step(obs, reward, te, np.zeros(n, bool), None, NEXT_STEP, True)
            _assert_equals_twin(torch, be, ref, f"obs {obs_on} reward {reward_on} call {c}")
        assert (ref.obs_count[0] > 1.0) == obs_on and (ref.ret_count[0] > 1.0) == reward_on
    be.normalize_enable(False, False)


# ---- through the env ------------------------------------------------------------------------------------------------
def _env_run(torch, autoreset, calls=12, n=65, seed=0, stats=True):
    """SoftPendulum-v0, 10 elements, final_time 0.1: an episode lasts three calls.  Every returned observation and
    reward is compared with the twin fed with infos["raw_*"]; returns the per-call records."""
    import gym_softrobot_amd as gsa

    mode = SAME_STEP if autoreset == "same_step" else NEXT_STEP if autoreset else MANUAL
    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset=autoreset, final_time=0.1, n_elems=10)
    env.set_normalization(gamma=0.9)
    if stats:
        env.record_episode_statistics(8)
    ref = NormalizeRef(n, env.obs_dim, gamma=0.9)
    obs, info = env.reset(seed=seed)
    ref.reset(_host(info["raw_obs"]))
    assert _same(_host(obs), ref.norm_obs), "reset observation"
    rng = np.random.default_rng(11)
    records, raw_rewards = [], []
    for c in range(calls):
        a = rng.uniform(-5.0, 5.0, (n, 1)).astype(np.float32)
        ret_count = float(env.backend.normalize["ret_count"].cpu()[0])
        latched = _host(env.backend.normalize["latch"]).astype(bool)
        o, r, te, tr, info = env.step(a)
        o, r, te, tr = _host(o), _host(r), _host(te), _host(tr)
        raw_o, raw_r = _host(info["raw_obs"]), _host(info["raw_reward"])
        assert o.dtype == np.float32 and o.shape == raw_o.shape and r.dtype == np.float64 and r.shape == raw_r.shape
        final = _host(info["raw_final_obs"]) if mode == SAME_STEP else None
        fin = ref.step(raw_o, raw_r, te, tr, final, mode)
        assert _same(o, ref.norm_obs), f"call {c}: observation"
        assert _same(r, ref.norm_reward), f"call {c}: reward"
        got = _assert_equals_twin(torch, env.backend, ref, f"call {c}")
        if mode == SAME_STEP:
            assert np.array_equal(_host(info["_final_obs"]), fin)
            assert _same(_host(info["final_obs"])[fin], ref.norm_final_obs[fin]), f"call {c}: final_obs"
            if fin.any():       # normalised, not raw
                assert not np.array_equal(_bits(_host(info["final_obs"])[fin]), _bits(final[fin]))
        else:
            assert "raw_final_obs" not in info
        # the reward is counted for the envs that were not latched, and for no other
        assert float(got["ret_count"][0]) - ret_count == pytest.approx(float((~latched).sum()), abs=1e-6)
        if mode == NEXT_STEP and latched.any():     # a reset call: zero reward, no flag, not in the return statistics
            assert not raw_r[latched].any() and not (te | tr)[latched].any()
        raw_rewards.append(raw_r)
        if stats:
            ended = _host(info["_episode"])
            for e in np.nonzero(ended)[0]:          # episode statistics keep reading the RAW reward
                assert _host(info["episode"]["r"])[e] == (raw_rewards[c - 2][e] + raw_rewards[c - 1][e]) + raw_rewards[c][e]
                assert _host(info["episode"]["l"])[e] == 3
        records.append(dict(raw_obs=raw_o, raw_reward=raw_r, te=te, tr=tr, obs=o, reward=r, latched=latched))
        done = te | tr
        if mode == MANUAL and done.any():
            o2, i2 = env.reset(mask=done)
            ref.reset(_host(i2["raw_obs"]), done)
            assert _same(_host(o2), ref.norm_obs), f"call {c}: masked reset"
            _assert_equals_twin(torch, env.backend, ref, f"masked reset after call {c}")
    finished = env.episode_statistics().count if stats else None
    env.close()
    return records, finished


@pytest.mark.parametrize("autoreset", [False, True, "device", "same_step"])
def test_through_the_env(torch_gpu, autoreset):
    records, finished = _env_run(torch_gpu, autoreset)
    n = 65
    assert finished == (3 if autoreset in (True, "device") else 4) * n          # at least three episodes per env
    if autoreset in (True, "device"):
        resets = [c for c, rec in enumerate(records) if rec["latched"].any()]
        assert resets == [3, 7, 11] and all(records[c]["latched"].all() for c in resets)


def test_host_and_device_next_step_agree(torch_gpu):
    """autoreset=True runs the pass from the env layer on the composed rows, "device" from the backend behind the step:
    with one seed the normalised outputs are bitwise equal wherever the raw outputs up to that call are."""
    host, _ = _env_run(torch_gpu, True, stats=False)
    device, _ = _env_run(torch_gpu, "device", stats=False)
    equal_so_far, checked = True, 0
    for c, (x, y) in enumerate(zip(host, device)):
        equal_so_far = equal_so_far and all(np.array_equal(_bits(x[k]), _bits(y[k])) for k in ("raw_obs", "raw_reward", "te", "tr"))
        if not equal_so_far:
            break
        assert np.array_equal(_bits(x["obs"]), _bits(y["obs"])) and np.array_equal(_bits(x["reward"]), _bits(y["reward"])), c
        checked += 1
    assert checked >= 5, f"the raw outputs of the two modes part at call {checked}: nothing compared past a reset call"


def test_wide_rows_through_octoflat(torch_gpu):
    """OctoFlat-v0 at n_elems = 3 (its three knots need three elements): obs_dim 181, three tiles with a ragged end."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n = 16
    env = gsa.make_vec("OctoFlat-v0", n, device=0, autoreset="same_step", n_elems=3, final_time=3e-4, time_step=7e-5,
                       recording_fps=7000)
    assert env.obs_dim == 181
    env.set_normalization()
    ref = NormalizeRef(n, env.obs_dim)
    obs, info = env.reset(seed=1)
    ref.reset(_host(info["raw_obs"]))
    assert _same(_host(obs), ref.norm_obs)
    rng = np.random.default_rng(2)
    ends = 0
    for c in range(6):
        o, r, te, tr, info = env.step(rng.uniform(-22.0, 22.0, (n, env.action_dim)).astype(np.float32))
        fin = ref.step(_host(info["raw_obs"]), _host(info["raw_reward"]), _host(te), _host(tr), _host(info["raw_final_obs"]), SAME_STEP)
        assert _same(_host(o), ref.norm_obs) and _same(_host(r), ref.norm_reward), c
        assert _same(_host(info["final_obs"])[fin], ref.norm_final_obs[fin]), c
        ends += int(fin.sum())
    assert ends >= n
    env.close()


def test_frozen_statistics(torch_gpu):
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n = 17
    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="device", final_time=0.1, n_elems=10)
    env.set_normalization()
    ref = NormalizeRef(n, env.obs_dim)
    _, info = env.reset(seed=4)
    ref.reset(_host(info["raw_obs"]))
    a = np.full((n, 1), 2.0, np.float32)
    for _ in range(2):
        _, _, te, tr, info = env.step(a)
        ref.step(_host(info["raw_obs"]), _host(info["raw_reward"]), _host(te), _host(tr), None, NEXT_STEP)
    before = _assert_equals_twin(torch, env.backend, ref, "before freezing")
    env.normalization_training = False
    outs = []
    for c in range(4):              # crosses an episode end and a reset call
        o, r, te, tr, info = env.step(a)
        ref.step(_host(info["raw_obs"]), _host(info["raw_reward"]), _host(te), _host(tr), None, NEXT_STEP, update=False)
        after = _assert_equals_twin(torch, env.backend, ref, f"frozen call {c}")
        for k in (*STATS, "ret", "latch"):
            assert np.array_equal(_bits(after[k]), _bits(before[k])), k
        assert _same(_host(o), ref.norm_obs) and _same(_host(r), ref.norm_reward)
        outs.append(_host(o))
    assert not np.array_equal(outs[0], outs[1])         # the outputs still follow the rows
    env.normalization_training = True
    env.step(a)
    torch.cuda.synchronize()
    assert float(env.backend.normalize["obs_count"].cpu()[0]) > float(before["obs_count"][0])
    env.close()


def test_state_round_trip_into_a_second_env(torch_gpu):
    import gym_softrobot_amd as gsa

    n = 9
    kw = dict(device=0, n_elems=10)
    first, second = gsa.make_vec("SoftPendulum-v0", n, **kw), gsa.make_vec("SoftPendulum-v0", n, **kw)
    first.set_normalization(gamma=0.95)
    first.reset(seed=6)
    second.reset(seed=6)
    rng = np.random.default_rng(7)
    acts = rng.uniform(-5.0, 5.0, (4, n, 1)).astype(np.float32)
    for a in acts[:2]:
        first.step(a)
        second.step(a)              # the same rods, no normalisation yet
    state = first.normalization_state()
    assert type(state).__name__ == "NormalizationState" and state.obs_mean.shape == (first.obs_dim,)
    assert state.obs_mean.dtype == np.float64 and isinstance(state.ret_var, float) and state.ret_count > 1.0
    second.set_normalization(gamma=0.95)
    second.load_normalization_state(state)
    back = second.normalization_state()
    for x, y in zip(state, back):
        assert np.array_equal(_bits(np.asarray(x)), _bits(np.asarray(y)))
    assert _same(_host(first.backend.normalize["obs_inv_std"]), _host(second.backend.normalize["obs_inv_std"]))
    assert _same(_host(first.backend.normalize["ret_inv_std"]), _host(second.backend.normalize["ret_inv_std"]))
    first.normalization_training = second.normalization_training = False
    for a in acts[2:]:
        x, y = first.step(a), second.step(a)
        assert _same(_host(x[0]), _host(y[0])) and _same(_host(x[1]), _host(y[1]))
        assert not np.array_equal(_host(x[0]), _host(x[4]["raw_obs"]))
    first.close()
    second.close()


def test_graph_replays_equal_the_eager_loop(torch_gpu):
    """capture_policy_step with normalisation on: the policy reads the normalised observation and the pass is part of
    the captured line.  10 replays leave the policy inputs, normalization_info and the statistics of 10 eager steps of
    a second env built with the same seed, bit for bit."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n, steps = 65, 10

    def policy(obs):
        return (obs[:, :1] * 0.5).clamp(-1.0, 1.0)

    def run(graphed):
        env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", final_time=0.1, n_elems=10)
        env.set_normalization()
        obs, _ = env.reset(seed=3)
        replay = env.capture_policy_step(policy) if graphed else None
        rows = []
        for _ in range(steps):
            if graphed:
                obs, reward = replay()[:2]
            else:
                obs, reward = env.step(policy(obs))[:2]
            info = env.normalization_info
            assert info["obs"].data_ptr() == obs.data_ptr() and info["reward"].data_ptr() == reward.data_ptr()
            rows.append({k: _host(v) for k, v in info.items()})
        st = _snapshot(torch, env.backend)
        env.close()
        return st, rows

    (a, ra), (b, rb) = run(False), run(True)
    assert a["obs_count"][0] > steps * n
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{k} differs between the eager loop and the graph"
    for t, (x, y) in enumerate(zip(ra, rb)):
        assert set(x) == {"obs", "raw_obs", "final_obs", "raw_final_obs", "reward", "raw_reward"}
        for k in x:
            assert np.array_equal(_bits(x[k]), _bits(y[k])), f"step {t + 1}: {k}"
    assert not np.array_equal(ra[-1]["obs"], ra[-1]["raw_obs"])


def test_off_restores_the_plain_outputs(torch_gpu):
    import gym_softrobot_amd as gsa

    n = 4
    kw = dict(device=0, final_time=0.1, autoreset="same_step")
    plain, env = gsa.make_vec("SoftPendulum-v0", n, **kw), gsa.make_vec("SoftPendulum-v0", n, **kw)
    assert plain.backend.normalize is None
    env.set_normalization()
    plain.reset(seed=2)
    _, info = env.reset(seed=2)
    assert "raw_obs" in info
    rng = np.random.default_rng(3)
    acts = rng.uniform(-5.0, 5.0, (6, n, 1)).astype(np.float32)
    for a in acts[:3]:
        x, y = plain.step(a), env.step(a)
        assert {"raw_obs", "raw_reward", "raw_final_obs"} <= set(y[4]) and not {"raw_obs", "raw_reward", "raw_final_obs"} & set(x[4])
        assert _same(_host(x[0]), _host(y[4]["raw_obs"])) and _same(_host(x[1]), _host(y[4]["raw_reward"]))
        assert not np.array_equal(_host(x[0]), _host(y[0]))
    with pytest.raises(NotImplementedError, match="normalisation"):
        env.step_packed(np.zeros((n, 1), np.float32))
    env.set_normalization(obs=False, reward=False)
    assert env.backend.normalize is None
    for a in acts[3:]:
        x, y = plain.step(a), env.step(a)
        assert not {"raw_obs", "raw_reward", "raw_final_obs"} & set(y[4])
        for name, u, v in zip(("obs", "reward", "terminated", "truncated"), x, y):
            assert np.array_equal(_host(u).view(np.uint8), _host(v).view(np.uint8)), name
        assert _same(_host(x[4]["final_obs"]), _host(y[4]["final_obs"]))
    assert "raw_obs" not in env.reset(seed=5)[1]
    plain.close()
    env.close()


def test_refusals_that_need_a_handle(torch_gpu, hip_lib, backends):
    from gym_softrobot_amd import _capi

    torch = torch_gpu
    be = backends(2, 15)
    n, d = be.n_envs, be.obs_dim
    o = torch.zeros((n, d), dtype=torch.float32, device=be.device)
    r = torch.zeros(n, dtype=torch.float64, device=be.device)
    f = torch.zeros(n, dtype=torch.uint8, device=be.device)
    view = _capi.SoftrodNormalizeView()
    off = b"normalize: the feature is off (softrod_normalize_enable)"
    err = lambda: hip_lib.softrod_last_error(be._h)     # noqa: E731
    assert hip_lib.softrod_normalize_enable(be._h, 0, 0, 0.99, 10.0, 10.0, 1e-8) == 0        # off stays off
    assert hip_lib.softrod_normalize_step(be._h, o.data_ptr(), r.data_ptr(), f.data_ptr(), f.data_ptr(), None, 0, 1, None) == -1 and err() == off
    assert hip_lib.softrod_normalize_reset(be._h, o.data_ptr(), None, 1, None) == -1 and err() == off
    assert hip_lib.softrod_normalize_view(be._h, C.byref(view)) == -1 and err() == off and not view.obs_mean
    host = np.zeros(d)
    assert hip_lib.softrod_normalize_load(be._h, *([host.ctypes.data] * 6), None) == -1 and err() == off
    assert hip_lib.softrod_normalize_enable(be._h, 1, 1, 1.01, 10.0, 10.0, 1e-8) == -1
    assert err() == b"normalize: gamma 1.01 is outside [0, 1]"
    be.normalize_enable(True, True, in_step=False)
    assert hip_lib.softrod_normalize_view(be._h, C.byref(view)) == 0
    assert (view.n_envs, view.obs_dim, view.obs_on, view.reward_on) == (n, d, 1, 1)
    assert (view.gamma, view.clip_obs, view.clip_reward, view.epsilon) == (0.99, 10.0, 10.0, 1e-8)
    before = _snapshot(torch, be)
    assert hip_lib.softrod_normalize_step(be._h, o.data_ptr(), r.data_ptr(), f.data_ptr(), f.data_ptr(), o.data_ptr(), 1, 1, None) == -1
    assert err() == b"normalize: final_obs needs mode 2"
    assert hip_lib.softrod_normalize_step(be._h, o.data_ptr(), r.data_ptr(), f.data_ptr(), f.data_ptr(), None, 3, 1, None) == -1
    assert err() == b"normalize: mode 3 is outside 0 .. 2"
    assert hip_lib.softrod_normalize_step(be._h, o.data_ptr(), None, f.data_ptr(), f.data_ptr(), None, 0, 1, None) == -1
    assert hip_lib.softrod_normalize_enable(be._h, 1, 1, 0.5, -2.0, 10.0, 1e-8) == -1 and err() == b"normalize: clip_obs -2 is not positive"
    after = _snapshot(torch, be)
    for k in before:                                    # a refused call changes nothing
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    assert after["obs_count"].tolist() == [1e-4] * d and after["obs_var"].tolist() == [1.0] * d and not after["ret"].any()
    be.normalize_enable(False, False)
    assert hip_lib.softrod_normalize_view(be._h, C.byref(view)) == -1
