"""Episode statistics on the GPU (csrc/softrod_episode_stats.hpp, softrod_episode_stats_*): the kernel against its NumPy
twin (tests/episode_stats_ref.py) on synthetic rewards and flags at the sizes that cross the wave (64), chunk (1024) and
ring edges; the masked clear; the statistics through the env under all four reset modes; inside a captured graph; off;
the C entry points' refusals.  Every comparison is BITWISE: a return is a sequence of float64 adds in call order."""
import ctypes as C

import numpy as np
import pytest

from tests.episode_stats_ref import ARRAYS, MANUAL, NEXT_STEP, SAME_STEP, EpisodeStatsRef

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(hip_lib):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def backends(torch_gpu):
    """One SoftPendulum-v0 handle per batch size, shared by the cases (the statistics never look at the rods)."""
    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    made = {}

    def get(n):
        if n not in made:
            made[n] = HipRodBackend(_capi.softpendulum_config(n, n_elems=10), 0)
        return made[n]

    yield get
    for be in made.values():
        be.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_equals_twin(torch, be, ref, where):
    torch.cuda.synchronize()
    st = be.episode_stats
    for name in ARRAYS:
        got, want = st[name].cpu().numpy(), getattr(ref, name)
        assert got.dtype == want.dtype and got.shape == want.shape, (where, name)
        assert np.array_equal(_bits(got), _bits(want)), f"{where}: {name} differs from the twin"
    assert int(st["count"].cpu()[0]) == ref.count, f"{where}: count"


CASES = [(n, 4) for n in (1, 64, 65, 1024, 1025, 2049)] + [(65, 1), (65, 100)]


@pytest.mark.parametrize("mode", [MANUAL, NEXT_STEP, SAME_STEP])
@pytest.mark.parametrize("n,ring", CASES)
def test_kernel_equals_the_twin(torch_gpu, backends, n, ring, mode):
    """20 calls with seeded normal rewards and each flag set with probability 0.3, an all-flags call (at N = 2049, K = 4
    the F > K case: 2049 finished envs, in the manual mode after a full clear) and a no-flag call in their middle; one
    call without an end time.  In the manual mode a random half of the envs is cleared after every third call, as a
    caller that resets finished envs by hand would.  After each call every resident array and count equal the twin's."""
    torch = torch_gpu
    be = backends(n)
    be.episode_stats_enable(ring, mode)
    ref = EpisodeStatsRef(n, ring)
    _assert_equals_twin(torch, be, ref, "enabled")          # everything zero
    rng = np.random.default_rng(1000 * n + 10 * ring + mode)
    plan = ["random"] * 10 + ["all", "none"] + ["random"] * 10
    for c, kind in enumerate(plan):
        reward = rng.standard_normal(n)
        if kind == "random":
            te, tr = rng.random(n) < 0.3, rng.random(n) < 0.3
        else:
            te = np.full(n, kind == "all")
            tr = np.zeros(n, bool)
        t = None if c == 5 else rng.random(n)
        if kind == "all" and mode == MANUAL:
            be.episode_stats_reset(None)
            ref.reset(None)
        dev = [torch.as_tensor(v, device=be.device) for v in (reward, te.astype(np.uint8), tr.astype(np.uint8))]
        be.episode_stats_update(*dev, None if t is None else torch.as_tensor(t, device=be.device), mode)
        before = ref.count
        ref.update(reward, te, tr, t, mode)
        if kind == "all" and mode != NEXT_STEP:
            assert ref.count - before == n                   # F = N: more than the ring holds wherever N > K
        _assert_equals_twin(torch, be, ref, f"call {c}")
        if mode == MANUAL and c % 3 == 2:
            mask = rng.random(n) < 0.5
            be.episode_stats_reset(mask)
            ref.reset(mask)
            _assert_equals_twin(torch, be, ref, f"clear after call {c}")
    assert ref.count > 0
    be.episode_stats_enable(0)
    assert be.episode_stats is None


def test_masked_clear(torch_gpu, backends):
    torch = torch_gpu
    n, ring = 65, 4
    be = backends(n)
    be.episode_stats_enable(ring, MANUAL)
    ref = EpisodeStatsRef(n, ring)
    rng = np.random.default_rng(7)
    for _ in range(3):
        reward, te = rng.standard_normal(n), (rng.random(n) < 0.3).astype(np.uint8)
        tr, t = np.zeros(n, np.uint8), rng.random(n)
        be.episode_stats_update(*(torch.as_tensor(v, device=be.device) for v in (reward, te, tr, t)), MANUAL)
        ref.update(reward, te, tr, t, MANUAL)
    _assert_equals_twin(torch, be, ref, "before the clear")
    assert ref.latch.any() and (ref.acc_length > 0).any() and ref.ep_mask.any() and ref.count > 0
    before = {k: be.episode_stats[k].cpu().numpy().copy() for k in (*ARRAYS, "count")}
    mask = np.arange(n) % 3 == 0
    mask[64] = True                     # the env behind the first wave
    be.episode_stats_reset(torch.as_tensor(mask, device=be.device))
    torch.cuda.synchronize()
    after = {k: be.episode_stats[k].cpu().numpy() for k in (*ARRAYS, "count")}
    for k in ("acc_return", "acc_length", "latch", "ep_r", "ep_l", "ep_t", "ep_mask"):
        assert not after[k][mask].any(), k                                           # cleared envs are zeroed
        assert np.array_equal(_bits(after[k][~mask]), _bits(before[k][~mask])), k    # the others are untouched
    for k in ("finished", "ring_r", "ring_l", "ring_t", "ring_env", "count"):
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
    ref.reset(mask)
    _assert_equals_twin(torch, be, ref, "after the clear")
    be.episode_stats_reset(None)        # NULL: every env
    ref.reset(None)
    _assert_equals_twin(torch, be, ref, "after the full clear")
    be.episode_stats_enable(0)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("autoreset", [False, True, "device", "same_step"])
def test_through_the_env(torch_gpu, autoreset, shifted):
    """N = 5, final_time = 0.1, zero actions: an episode lasts three calls.  8 calls.  infos["episode"] / ["_episode"]
    equal the twin fed with what the call returned; every finished episode has l == 3 and r = the sum of its three
    returned rewards; in the NEXT_STEP modes the reset call is counted in no episode; `shifted`: after
    reset(mask=[True, False, False, False, False]) following the first call env 0's episodes end one call later."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n, calls = 5, 8
    mode = SAME_STEP if autoreset == "same_step" else NEXT_STEP if autoreset else MANUAL
    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset=autoreset, final_time=0.1)
    env.record_episode_statistics(4)
    env.reset(seed=0)
    ref = EpisodeStatsRef(n, 4)
    zeros = torch.zeros(n, 1)
    rewards, ends, episodes = [], [[] for _ in range(n)], []
    for c in range(calls):
        o, r, te, tr, info = env.step(zeros)
        assert info["episode"]["r"].dtype == torch.float64 and info["episode"]["l"].dtype == torch.int32
        assert info["episode"]["t"].dtype == torch.float64 and info["_episode"].dtype == torch.bool
        r, te, tr = r.cpu().numpy().copy(), te.cpu().numpy().copy(), tr.cpu().numpy().copy()
        clock = info["final_info"]["time"] if mode == SAME_STEP else info["time"]
        clock = clock.cpu().numpy() if hasattr(clock, "cpu") else np.asarray(clock)
        ref.update(r, te, tr, clock, mode)
        ep = {k: v.cpu().numpy() for k, v in info["episode"].items()}
        got_mask = info["_episode"].cpu().numpy()
        for k, want in (("r", ref.ep_r), ("l", ref.ep_l), ("t", ref.ep_t)):
            assert np.array_equal(_bits(ep[k]), _bits(want)), f"call {c + 1}: episode.{k}"
        assert np.array_equal(got_mask, ref.ep_mask.astype(bool)), f"call {c + 1}: _episode"
        assert np.array_equal(got_mask, (te | tr) if mode == SAME_STEP else got_mask & (te | tr))
        same = env.episode_info
        assert same["episode"]["r"].data_ptr() == info["episode"]["r"].data_ptr()
        rewards.append(r)
        if mode == NEXT_STEP and c > 0:
            was = [c - 1 in ends[e] for e in range(n)]       # the reset call: reward 0, no flag, no episode
            assert not r[was].any() and not (te | tr)[was].any() and not got_mask[was].any()
        for e in np.nonzero(got_mask)[0]:
            ends[e].append(c)
            assert ep["l"][e] == 3, f"call {c + 1}, env {e}: length {ep['l'][e]}"
            assert ep["r"][e] == (rewards[c - 2][e] + rewards[c - 1][e]) + rewards[c][e]
            assert ep["t"][e] > 0.0
            episodes.append((ep["r"][e], ep["l"][e], ep["t"][e], e))
        done = te | tr
        if mode == MANUAL and done.any():
            env.reset(mask=done)
            ref.reset(done)
        if shifted and c == 0:
            first = np.array([True, False, False, False, False])
            env.reset(mask=first)
            ref.reset(first)
    period = 4 if mode == NEXT_STEP else 3
    assert ends[1] == [2, 2 + period] and all(ends[e] == ends[1] for e in range(2, n))
    assert ends[0] == ([c + 1 for c in ends[1]] if shifted else ends[1])
    _assert_equals_twin(torch, env.backend, ref, "after the run")
    stats = env.episode_statistics()
    assert stats.count == 2 * n == len(episodes) and stats.finished.tolist() == [2] * n
    for got, want, last in zip(stats[1:5], ref.recent(), zip(*episodes[-4:])):
        assert np.array_equal(_bits(got), _bits(want)) and got.tolist() == list(last)
    env.record_episode_statistics(0)
    assert "episode" not in env.step(zeros)[4]
    env.close()


def test_graph_replays_equal_the_eager_loop(torch_gpu):
    """capture_policy_step with statistics on: the update is one more kernel of the captured line.  7 replays leave the
    arrays, the ring and count of 7 eager steps of a second env built with the same seed, bit for bit."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n, steps = 65, 7

    def policy(obs):
        return (obs[:, :1] * 0.5).clamp(-1.0, 1.0)

    def run(graphed):
        env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", final_time=0.1)
        obs, _ = env.reset(seed=3)
        env.record_episode_statistics(100)
        replay = env.capture_policy_step(policy) if graphed else None
        rows = []
        for _ in range(steps):
            obs = replay()[0] if graphed else env.step(policy(obs))[0]
            info = env.episode_info
            rows.append((info["episode"]["r"].cpu().numpy().copy(), info["_episode"].cpu().numpy().copy()))
        torch.cuda.synchronize()
        st = {k: env.backend.episode_stats[k].cpu().numpy().copy() for k in (*ARRAYS, "count")}
        stats = env.episode_statistics()
        env.close()
        return st, rows, stats

    (a, ra, sa), (b, rb, sb) = run(False), run(True)
    assert int(a["count"][0]) == 2 * n            # two episode ends per env in 7 three-call episodes: the ring has wrapped
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{k} differs between the eager loop and the graph"
    for t, ((r1, m1), (r2, m2)) in enumerate(zip(ra, rb)):
        assert np.array_equal(_bits(r1), _bits(r2)) and np.array_equal(m1, m2), f"step {t + 1}"
    assert sa.count == sb.count and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(sa[1:], sb[1:]))
    assert sa.returns.shape == (100,) and sa.envs.tolist() == list(range(30, 65)) + list(range(65))


def test_off_changes_nothing(torch_gpu):
    """An env that never switched them on has no "episode" key; the step outputs of an env with statistics on are
    bitwise those of one without; step_packed with statistics on raises."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n = 4
    kw = dict(device=0, final_time=0.1)
    off, on = gsa.make_vec("SoftPendulum-v0", n, **kw), gsa.make_vec("SoftPendulum-v0", n, **kw)
    assert off.backend.episode_stats is None
    on.record_episode_statistics()
    assert on.backend.episode_stats["ring_r"].shape == (100,)
    off.reset(seed=2)
    on.reset(seed=2)
    rng = np.random.default_rng(3)
    for t in range(4):
        a = rng.uniform(-5.0, 5.0, (n, 1)).astype(np.float32)
        x, y = off.step(a), on.step(a)
        assert "episode" not in x[4] and "_episode" not in x[4] and "episode" in y[4]
        for name, u, v in zip(("obs", "reward", "terminated", "truncated"), x, y):
            assert np.array_equal(u.cpu().numpy().view(np.uint8), v.cpu().numpy().view(np.uint8)), f"step {t + 1}: {name}"
        assert np.array_equal(np.asarray(x[4]["time"]), np.asarray(y[4]["time"]))
    with pytest.raises(NotImplementedError, match="episode statistics"):
        on.step_packed(np.zeros((n, 1), np.float32))
    off.step_packed(np.zeros((n, 1), np.float32))
    with pytest.raises(ValueError):
        on.record_episode_statistics(-2)
    assert on.backend.episode_stats is not None          # a refused call changes nothing
    off.close()
    on.close()


def test_c_abi_refusals(torch_gpu, hip_lib):
    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    torch = torch_gpu
    n = 3
    be = HipRodBackend(_capi.softpendulum_config(n, n_elems=10), 0)
    r = torch.ones(n, dtype=torch.float64, device=be.device)
    f = torch.ones(n, dtype=torch.uint8, device=be.device)
    view = _capi.SoftrodEpisodeStatsView()
    off = b"episode stats: the feature is off (softrod_episode_stats_enable)"
    # an off handle
    assert hip_lib.softrod_episode_stats_update(be._h, r.data_ptr(), f.data_ptr(), f.data_ptr(), None, 0, None) == -1
    assert hip_lib.softrod_last_error(be._h) == off
    assert hip_lib.softrod_episode_stats_reset(be._h, None, None) == -1 and hip_lib.softrod_last_error(be._h) == off
    assert hip_lib.softrod_episode_stats_view(be._h, C.byref(view)) == -1 and hip_lib.softrod_last_error(be._h) == off
    assert not view.acc_return and view.ring == 0
    assert hip_lib.softrod_episode_stats_enable(be._h, -1) == -1
    assert hip_lib.softrod_last_error(be._h) == b"episode stats: ring -1 is negative"
    assert hip_lib.softrod_episode_stats_enable(be._h, 0) == 0          # off stays off
    assert hip_lib.softrod_episode_stats_enable(None, 4) == -1
    assert hip_lib.softrod_last_error(None) == b"episode stats: null handle"
    be.episode_stats_enable(4)
    assert hip_lib.softrod_episode_stats_view(be._h, C.byref(view)) == 0 and view.n_envs == n and view.ring == 4
    assert view.count and view.ring_env and view.ep_mask
    # a bad mode, null pointers: refused, nothing changes
    for mode in (-1, 3):
        assert hip_lib.softrod_episode_stats_update(be._h, r.data_ptr(), f.data_ptr(), f.data_ptr(), None, mode, None) == -1
        assert hip_lib.softrod_last_error(be._h) == f"episode stats: mode {mode} is outside 0 .. 2".encode()
    for args in ((None, f.data_ptr(), f.data_ptr()), (r.data_ptr(), None, f.data_ptr()), (r.data_ptr(), f.data_ptr(), None)):
        assert hip_lib.softrod_episode_stats_update(be._h, *args, None, 0, None) == -1
        assert hip_lib.softrod_last_error(be._h) == b"episode stats: null reward, terminated or truncated"
    assert hip_lib.softrod_episode_stats_view(be._h, None) == -1
    assert hip_lib.softrod_last_error(be._h) == b"episode stats: null argument"
    assert hip_lib.softrod_episode_stats_enable(be._h, -5) == -1
    torch.cuda.synchronize()
    assert be.episode_stats is not None and int(be.episode_stats["count"].cpu()[0]) == 0
    assert not any(bool(be.episode_stats[k].cpu().any()) for k in ARRAYS)
    # an accepted call works, with a NULL end time
    be.episode_stats_update(r, f, f, None, SAME_STEP)
    torch.cuda.synchronize()
    assert int(be.episode_stats["count"].cpu()[0]) == n and be.episode_stats["ring_env"].cpu().tolist() == [0, 1, 2, 0]
    be.episode_stats_enable(0)
    assert hip_lib.softrod_episode_stats_view(be._h, C.byref(view)) == -1
    be.close()
