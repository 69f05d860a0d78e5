"""set_reset_shapes() on the GPU: while a pool of start shapes is set, every reset of an env — reset(), the host-driven
auto-reset, autoreset="device" and "same_step" — leaves the env exactly as reset followed by set_rod_shape(pool[idx]).

The yardstick is the code as it stood: a twin batch with autoreset=False and NO pool, driven by hand
(tests/reset_shapes_ref.py: step; where terminated | truncated, reset(mask=done) and set_rod_shape(done, pool[idx]) with
idx from the NumPy index function and a host-side count of each env's resets).  Both sides run the same kernels'
arithmetic on the same draws of each env's stream, so everything is compared BITWISE."""
import numpy as np
import pytest

try:
    from tests import reset_shapes_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import reset_shapes_ref as ref

pytestmark = pytest.mark.gpu

SHORT = dict(time_step=1e-4, recording_fps=5000)
ARM = dict(final_time=3e-4, time_step=7e-5, recording_fps=7000)
SEED, K = ref.KNOWN_SEED, ref.KNOWN_K
PENDULUM = dict(final_time=5e-4, n_elems=20, **SHORT)


@pytest.fixture(scope="module")
def torch_gpu(hip_lib):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch


def _actions(env_id, rng, n, dim):
    if env_id.startswith("SoftPendulum3D"):
        return rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    if env_id.startswith("SoftPendulum") or env_id.startswith("OctoArmSingle"):
        return rng.uniform(-5.0, 5.0, (n, dim)).astype(np.float32)
    if env_id.startswith("OctoFlat"):
        return rng.uniform(-20.0, 20.0, (n, dim)).astype(np.float32)
    a = rng.uniform(0.0, 1.0, (n, dim)).astype(np.float32)           # the muscle envs: activations
    return a * 0.6 if env_id == "OctoReach-v0" else a


def _bits_equal(u, v):
    """Same shape, dtype and bits (a NaN equals the same NaN)."""
    import torch

    if u.shape != v.shape or u.dtype != v.dtype:
        return False
    return bool((u.contiguous().view(-1).view(torch.uint8) == v.contiguous().view(-1).view(torch.uint8)).all())


def _rods(env):
    from gym_softrobot_amd import _capi

    return _capi.config_rods_per_env(env.cfg)


def _pair(gsa, torch, env_id, kw, n, mode, planar=False):
    """The batch under test with a pool, and its hand-driven twin."""
    env = gsa.make_vec(env_id, n, device=0, autoreset=mode, **kw)
    twin_env = gsa.make_vec(env_id, n, device=0, autoreset=False, **kw)
    fields = ref.pool(env.cfg, _rods(env), K, planar=planar)
    env.set_reset_shapes(**fields, seed=SEED)
    return env, ref.Twin(torch, twin_env, fields, SEED)


def _assert_rows(env, twin, where):
    np.testing.assert_array_equal(env.reset_shape_index.cpu().numpy(), twin.index, err_msg=f"{where}: reset_shape_index")
    np.testing.assert_array_equal(env.reset_shape_episode.cpu().numpy(), twin.episode, err_msg=f"{where}: reset_shape_episode")


def _assert_state_equal(torch, env, twin):
    sa, sb = env.backend.state(), twin.env.backend.state()
    torch.cuda.synchronize()
    for k in env.backend._snapshot_keys():
        assert np.array_equal(sa[k].cpu().numpy(), sb[k].cpu().numpy(), equal_nan=True), f"state {k!r} differs"


CASES = [
    ("SoftPendulum-v0", PENDULUM, 6, True, True),
    ("SoftPendulum-v0", dict(final_time=7e-4, n_elems=100, **SHORT), 6, False, True),
    ("SoftPendulum3D-v0", dict(final_time=6e-4, n_elems=20, **SHORT), 6, False, False),
    ("OctoArmSingle-v0", dict(n_elems=20, **ARM), 6, False, False),
    ("OctoFlat-v0", dict(**ARM), 6, False, True),
    ("OctoArmPush-v1", dict(final_time=0.06, n_elems=100), 6, False, False),
    ("OctoArmTwo-v0", dict(final_time=0.07), 2, False, False),
    ("OctoReach-v0", dict(final_time=0.07), 2, False, False),
]
IDS = ["pendulum-planar-pool", "pendulum-2-per-lane", "pendulum3d", "arm", "octo", "push-2-per-lane", "arm-two", "reach"]
MODE_CASES = [pytest.param(*c, mode, id=f"{i}-{'host' if mode is True else mode}")
              for c, i in zip(CASES, IDS) for mode in ("device", "same_step", True) if mode is not True or c[4]]
MAX_STEPS = 48


@pytest.mark.parametrize("env_id,kw,n,planar,host_too,mode", MODE_CASES)
def test_shaped_resets_equal_the_hand_driven_twin(torch_gpu, env_id, kw, n, planar, host_too, mode):
    """Bit for bit, every step, until every env has restarted at least twice, with episode ends staggered inside the
    batch by a manual masked reset of the first half after the first step (which is also the manual reset of the device
    modes).  seed 1, K = 3: by the known answers every env changes entry and all three entries occur within three
    episodes of a batch of six."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    env, twin = _pair(gsa, torch, env_id, kw, n, mode, planar)
    o1, _ = env.reset(seed=3)
    o2 = twin.reset(seed=3)
    assert _bits_equal(o1, o2), "reset: obs"
    _assert_rows(env, twin, "reset")
    assert twin.index.tolist() == [ref.KNOWN[e][0] for e in range(n)]
    rng = np.random.default_rng(0)
    restarts = np.zeros(n, int)
    seen = [twin.index.copy()]
    same = mode == "same_step"
    for t in range(MAX_STEPS):
        a = _actions(env_id, rng, n, env.action_dim)
        o, r, te, tr, info = env.step(a)
        if same:
            o2, r2, te2, tr2, done, final, clock, tinfo = twin.step_same(a)
            restarted = done.cpu().numpy()
        else:
            o2, r2, te2, tr2, restarted = twin.step_next(a)
        assert _bits_equal(o, o2), f"step {t}: obs"
        assert _bits_equal(r, r2) and torch.equal(te, te2) and torch.equal(tr, tr2), f"step {t}: reward / flags"
        _assert_rows(env, twin, f"step {t}")
        if same:
            assert torch.equal(info["_final_obs"], done), f"step {t}: _final_obs"
            assert _bits_equal(info["final_obs"][done], final[done]), f"step {t}: final_obs"
            d = restarted
            np.testing.assert_array_equal(info["final_info"]["time"].cpu().numpy()[d], clock[d], err_msg=f"step {t}: final_info.time")
            np.testing.assert_array_equal(info["time"].cpu().numpy(), np.where(d, 0.0, clock), err_msg=f"step {t}: time")
            if env_id == "SoftPendulum3D-v0":      # aux follows the shaped obs; the finished step's value stays beside final_obs
                assert torch.equal(info["final_info"]["tilt"][done], tinfo["tilt"][done]), t
                assert torch.equal(info["tilt"][~done], tinfo["tilt"][~done]), t
                assert torch.equal(info["tilt"][done].float(), o[done][:, 8]), t
        restarts += restarted
        seen.append(twin.index.copy())
        if t == 0:
            m = np.zeros(n, bool)
            m[: n // 2] = True
            assert _bits_equal(env.reset(mask=m)[0], twin.reset(mask=m)), "masked reset: obs"
            _assert_rows(env, twin, "masked reset")
            restarts += m
            seen.append(twin.index.copy())
        if restarts.min() >= 2 and not restarted.any():      # (not on a restarting call: NEXT_STEP's twin steps and discards)
            break
    assert restarts.min() >= 2, f"every env was meant to restart at least twice: {restarts}"
    seen = np.array(seen)
    assert (seen != seen[0]).any(), "the indices seen were meant to change: the test would pass without a pool otherwise"
    assert len(set(seen.reshape(-1).tolist())) >= 2
    if n >= 6:
        assert set(seen.reshape(-1).tolist()) == {0, 1, 2}
    _assert_state_equal(torch, env, twin)
    if mode is not True:
        cons, underflow = env.backend.queue_status()
        assert underflow == 0 and cons.min() >= 1
    env.close()
    twin.env.close()


def test_the_pool_changes_the_start(torch_gpu):
    """Not vacuous: with the pool the restarted envs' observations differ from a batch without one."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n = 4
    plain = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **PENDULUM)
    shaped = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **PENDULUM)
    shaped.set_reset_shapes(**ref.pool(shaped.cfg, 1, K), seed=SEED)
    with pytest.raises(Exception, match="no pool"):
        plain.reset_shape_index
    o1, _ = plain.reset(seed=3)
    o2, _ = shaped.reset(seed=3)
    assert torch.equal(o1[:, 0], o2[:, 0]) and bool((o1[:, 3] != o2[:, 3]).all())      # the base stays, the angle moves
    a = np.zeros((n, 1), np.float32)
    for _ in range(8):
        o1, _, _, tr1, _ = plain.step(a)
        o2, _, _, tr2, _ = shaped.step(a)
        assert torch.equal(tr1, tr2)
        if bool(tr1.all()):
            break
    assert bool(tr1.all()) and bool((o1[:, 3] != o2[:, 3]).all())       # the starts of the second episodes
    plain.close()
    shaped.close()


@pytest.mark.parametrize("mode", ["device", "same_step"])
def test_packed_rows_carry_the_shaped_observation(torch_gpu, mode):
    import gym_softrobot_amd as gsa
    from gym_softrobot_amd.distributed import unpack_outputs

    torch = torch_gpu
    n = 6
    for env_id, kw in (("SoftPendulum-v0", PENDULUM),
                       ("SoftPendulum3D-v0", dict(final_time=6e-4, n_elems=20, **SHORT))):      # odd obs_dim: a padded row
        dense = gsa.make_vec(env_id, n, device=0, autoreset=mode, **kw)
        packd = gsa.make_vec(env_id, n, device=0, autoreset=mode, **kw)
        for e in (dense, packd):
            e.set_reset_shapes(**ref.pool(e.cfg, 1, K), seed=SEED)
            e.reset(seed=3)
        rng = np.random.default_rng(0)
        ends = 0
        for t in range(16):
            a = _actions(env_id, rng, n, dense.action_dim)
            o, r, te, tr, info = dense.step(a)
            packed, _ = packd.step_packed(a)
            po, pr, pte, ptr = unpack_outputs(packed, dense.obs_dim)[:4]
            assert torch.equal(o, po) and torch.equal(r, pr), (env_id, t)
            assert torch.equal(te, pte.view(torch.bool)) and torch.equal(tr, ptr.view(torch.bool)), (env_id, t)
            assert torch.equal(dense.reset_shape_index, packd.reset_shape_index), (env_id, t)
            assert torch.equal(dense.reset_shape_episode, packd.reset_shape_episode), (env_id, t)
            ends += int((te | tr).sum())
        assert ends >= 2 * n and int(dense.reset_shape_episode.min()) >= 3
        sa, sb = dense.backend.state(), packd.backend.state()
        for k in dense.backend._snapshot_keys():
            assert np.array_equal(sa[k].cpu().numpy(), sb[k].cpu().numpy(), equal_nan=True), f"state {k!r} differs"
        dense.close()
        packd.close()


def test_a_dry_queue_is_neither_shaped_nor_counted(torch_gpu):
    """final_time below one env.step: every step ends every episode.  With the top-ups paused the envs starve after
    queue_depth records: they stay finished, are neither shaped nor counted, and are shaped once a record arrives."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    kw = dict(final_time=5e-5, time_step=1e-4, recording_fps=10000, n_elems=10)
    n = 3
    a = np.zeros(n, np.float32)
    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **kw)
    env.set_reset_shapes(**ref.pool(env.cfg, 1, K), seed=SEED)
    env.queue_depth = 4
    env.top_up_paused = True
    env.reset(seed=0)

    def want(j):
        return [ref.index(SEED, e, j, K) for e in range(n)]

    assert env.reset_shape_index.tolist() == want(0) and env.reset_shape_episode.tolist() == [1] * n
    for t in range(7):
        o, r, te, tr, info = env.step(a)
        assert bool(tr.all()), t
        fed = min(t + 1, 4)                      # four records were staged: from the fifth step on the envs stay finished
        assert env.reset_shape_episode.tolist() == [1 + fed] * n, t
        assert env.reset_shape_index.tolist() == want(fed), t
        if t >= 4:
            assert torch.equal(o, info["final_obs"]) and bool((info["time"] > 0).all()), t
        else:
            assert not torch.equal(o, info["final_obs"]) and bool((info["time"] == 0).all()), t
    cons, underflow = env.backend.queue_status()
    assert cons.tolist() == [4] * n and underflow == 3 * n
    # one record each arrives (staged by hand: the env's own top-up reports the shortage instead)
    counts = np.ones(n, np.int32)
    draws = [[env._draw_reset(i)] for i in range(n)]
    env._queue_from_draws(draws, counts)
    env._produced += counts
    o, r, te, tr, info = env.step(a)
    assert env.reset_shape_episode.tolist() == [6] * n and env.reset_shape_index.tolist() == want(5)
    assert not torch.equal(o, info["final_obs"]) and bool((info["time"] == 0).all())
    o, r, te, tr, info = env.step(a)             # dry again
    assert env.reset_shape_episode.tolist() == [6] * n and torch.equal(o, info["final_obs"])
    env.close()


def test_policy_step_as_one_graph_equals_the_eager_loop(torch_gpu):
    """capture_policy_step in same-step mode with a pool: the shaping pass is three more kernels of the captured
    straight line.  Bitwise against the eager loop, the index row included; 5-step episodes, 14 steps."""
    import sys
    from pathlib import Path

    import gym_softrobot_amd as gsa

    torch = torch_gpu
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench

    n, steps = 8, 14
    kw = dict(autoreset="same_step", final_time=0.19)

    def run(graphed):
        env = gsa.make_vec("SoftPendulum-v0", n, device=0, **kw)
        env.set_reset_shapes(**ref.pool(env.cfg, 1, K), seed=SEED)
        obs, _ = env.reset(seed=5)
        policy = bench.make_policy(torch, env.backend.device, env.obs_dim, env.action_dim, 22.0)
        replay = env.capture_policy_step(policy) if graphed else None
        rec = []
        for _ in range(steps):
            out = replay() if graphed else env.step(policy(obs))[:4]
            obs = out[0]
            be = env.backend
            rec.append(tuple(x.detach().cpu().clone() for x in (*out, be.final_obs, be.final_time, be.reset_shape_index,
                                                                be.reset_shape_episode)))
        torch.cuda.synchronize()
        cons, underflow = env.backend.queue_status()
        env.close()
        return rec, cons, underflow

    (a, ca, ua), (b, cb, ub) = run(False), run(True)
    assert ua == ub == 0 and ca.tolist() == cb.tolist() and ca.min() >= 2
    names = ("obs", "reward", "terminated", "truncated", "final_obs", "final_time", "reset_shape_index", "reset_shape_episode")
    for t, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(names, x, y):
            assert np.array_equal(u.numpy(), v.numpy(), equal_nan=True), f"step {t + 1}: {name} differs"
    assert a[-1][7].tolist() == [1 + int(c) for c in ca]                # one shaped start per consumed record, and reset's
    assert len({tuple(x[6].tolist()) for x in a}) >= 2                   # the entries moved


def test_a_new_pool_takes_effect_at_the_next_reset_and_clearing_returns_to_straight_starts(torch_gpu):
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n = 6
    env, twin = _pair(gsa, torch, "SoftPendulum-v0", PENDULUM, n, "same_step")
    env.reset(seed=3)
    twin.reset(seed=3)
    rng = np.random.default_rng(4)

    def run(steps, where):
        ends = 0
        for t in range(steps):
            a = _actions("SoftPendulum-v0", rng, n, 1)
            o, r, te, tr, info = env.step(a)
            o2, r2, te2, tr2, done = twin.step_same(a)[:5]
            assert _bits_equal(o, o2) and _bits_equal(r, r2) and torch.equal(tr, tr2), f"{where}, step {t}"
            ends += int(done.sum())
        return ends

    assert run(2, "first pool") == 0                                    # mid-episode
    before = {k: v.cpu().clone() for k, v in env.backend.state().items() if hasattr(v, "cpu")}
    other = {k: -0.5 * v[::-1] for k, v in ref.pool(env.cfg, 1, 2).items()}          # K = 2, other shapes
    env.set_reset_shapes(**other, seed=9)
    after = env.backend.state()
    for k, v in before.items():
        assert np.array_equal(v.numpy(), after[k].cpu().numpy(), equal_nan=True), f"set_reset_shapes moved state {k!r}"
    assert env.reset_shape_index.tolist() == [-1] * n and env.reset_shape_episode.tolist() == [0] * n
    twin.fields = {k: np.ascontiguousarray(v) for k, v in other.items()}
    twin.count, twin.seed = 2, 9
    twin.episode[:] = 0
    twin.index[:] = -1
    assert run(9, "second pool") >= n
    _assert_rows(env, twin, "second pool")
    assert set(twin.index.tolist()) <= {0, 1} and (twin.index >= 0).all()
    env.set_reset_shapes()                                              # cleared: straight starts, nothing launched
    with pytest.raises(Exception, match="no pool"):
        env.reset_shape_index
    twin.fields, twin.count = {}, 0
    assert run(8, "no pool") >= n
    _assert_state_equal(torch, env, twin)
    env.close()
    twin.env.close()


def test_fork_and_snapshot_carry_the_rows(torch_gpu):
    import gym_softrobot_amd as gsa

    n = 4
    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset=False, n_elems=20)
    env.set_reset_shapes(**ref.pool(env.cfg, 1, K), seed=SEED)
    env.reset(seed=1)
    env.reset(mask=np.array([True, False, False, False]))
    idx = [ref.KNOWN[0][1]] + [ref.KNOWN[e][0] for e in range(1, n)]
    assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == [2, 1, 1, 1]
    assert env.reset_shape_index.dtype == torch_gpu.int32 and env.reset_shape_index.is_cuda
    env.fork(0, [2], copy_rng=True)
    idx[2] = idx[0]
    assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == [2, 1, 2, 1]
    env.reset(mask=np.array([False, False, False, True]))               # env 3: its second start
    idx[3] = ref.KNOWN[3][1]
    env.fork(0, [1], copy_rng=False)                                    # the index travels, the ordinal stays dst's own
    assert idx[1] != idx[0]
    idx[1] = idx[0]
    assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == [2, 1, 2, 2]
    sd = env.state_dict()
    assert sd["backend"]["reset_shape_index"].tolist() == idx and sd["backend"]["reset_shape_episode"].tolist() == [2, 1, 2, 2]
    env.reset()
    assert env.reset_shape_episode.tolist() == [3, 2, 3, 3] and env.reset_shape_index.tolist() != idx
    env.load_state_dict(sd)
    assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == [2, 1, 2, 2]
    env.close()


def test_a_seed_reproduces_the_starts(torch_gpu):
    import gym_softrobot_amd as gsa

    n = 6

    def run(pool_seed):
        env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="device", **PENDULUM)
        env.set_reset_shapes(**ref.pool(env.cfg, 1, K), seed=pool_seed)
        env.reset(seed=3)
        rows = [env.reset_shape_index.tolist()]
        rng = np.random.default_rng(0)
        for _ in range(16):
            env.step(_actions("SoftPendulum-v0", rng, n, 1))
            rows.append(env.reset_shape_index.tolist())
        episodes = env.reset_shape_episode.tolist()
        env.close()
        return rows, episodes

    (a, ea), (b, eb), (c, ec) = run(SEED), run(SEED), run(SEED + 1)
    assert a == b and ea == eb == ec and min(ea) >= 3
    assert a != c
    assert a[-1] == [ref.index(SEED, e, ea[e] - 1, K) for e in range(n)]
    assert c[-1] == [ref.index(SEED + 1, e, ec[e] - 1, K) for e in range(n)]
