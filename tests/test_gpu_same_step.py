"""autoreset="same_step" on the GPU (Gymnasium's AutoresetMode.SAME_STEP on the staged reset queue,
csrc/softrod_autoreset.hpp): the call that ends an env's episode returns that step's reward and flags, the NEW episode's
first observation, and the terminal observation in infos["final_obs"].

The yardstick is the code as it stood: a twin batch with autoreset=False driven by hand — step, and where
terminated | truncated, keep the observation as the final one, reset(mask=done), take the reset observation.  That is
the composition VecRodEnvBase.step uses for the host-driven mode.  Both sides run the same kernels' arithmetic on the
same draws of each env's stream, so everything is compared BITWISE."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHORT = dict(time_step=1e-4, recording_fps=5000)
ARM = dict(final_time=3e-4, time_step=7e-5, recording_fps=7000)


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


def _twin_step(torch, twin, a):
    """One step of the hand-driven twin -> (obs, reward, terminated, truncated, done, final obs, clock before the reset,
    the step's own info)."""
    o, r, te, tr, info = twin.step(a)
    done = te | tr
    final = o.clone()                      # (reset's observe() rewrites the buffer `o` is a view of)
    clock = np.array(info["time"], np.float64)
    if bool(done.any()):
        robs, _ = twin.reset(mask=done.cpu().numpy())
        o = torch.where(done[:, None], robs, final)
    else:
        o = final
    return o, r.clone(), te.clone(), tr.clone(), done, final, clock, info


def _bits_equal(u, v):
    """Same shape, dtype and bits (a NaN equals the same NaN)."""
    import torch

    if u.shape != v.shape or u.dtype != v.dtype:
        return False
    return bool((u.contiguous().view(-1).view(torch.uint8) == v.contiguous().view(-1).view(torch.uint8)).all())


def _assert_step_equal(torch, t, same_out, twin_out):
    o, r, te, tr, info = same_out
    o2, r2, te2, tr2, done, final, clock, _ = twin_out
    assert _bits_equal(o, o2), f"step {t}: obs"
    assert _bits_equal(r, r2) and torch.equal(te, te2) and torch.equal(tr, tr2), f"step {t}: reward / flags"
    assert info["_final_obs"].dtype == torch.bool and torch.equal(info["_final_obs"], done), f"step {t}: _final_obs"
    assert info["final_obs"].shape == o.shape and info["final_obs"].dtype == torch.float32
    assert _bits_equal(info["final_obs"][done], final[done]), f"step {t}: final_obs"
    ft = info["final_info"]["time"]
    assert ft.dtype == torch.float64 and ft.shape == (o.shape[0],)
    d = done.cpu().numpy()
    np.testing.assert_array_equal(ft.cpu().numpy()[d], clock[d], err_msg=f"step {t}: final_info.time")
    # the resident clock: 0 for a restarted env, the twin's otherwise
    np.testing.assert_array_equal(info["time"].cpu().numpy(), np.where(d, 0.0, clock), err_msg=f"step {t}: time")


@pytest.mark.parametrize("env_id,kw,n,T", [
    ("SoftPendulum-v0", dict(final_time=5e-4, n_elems=20, **SHORT), 6, 36),
    ("SoftPendulum-v0", dict(final_time=7e-4, n_elems=100, **SHORT), 6, 36),
    ("SoftPendulum3D-v0", dict(final_time=6e-4, n_elems=20, **SHORT), 6, 36),
    ("OctoArmSingle-v0", dict(n_elems=20, **ARM), 6, 36),
    ("OctoArmSingle-v0", dict(n_elems=100, **ARM), 6, 36),
    ("OctoFlat-v0", dict(**ARM), 6, 36),
    ("OctoArmPush-v1", dict(final_time=0.06), 3, 12),
    ("OctoArmPush-v1", dict(final_time=0.06, n_elems=100), 6, 12),
    ("OctoArmPullWeight-v0", dict(final_time=0.03), 6, 8),
    ("OctoCrawl-v0", dict(final_time=0.07), 2, 8),
    ("OctoArmTwo-v0", dict(final_time=0.07), 2, 8),
    ("OctoReach-v0", dict(final_time=0.07), 2, 8),
], ids=["pendulum", "pendulum-2-per-lane", "pendulum3d", "arm", "arm-two-windows", "octo", "push", "push-2-per-lane",
        "pull-weight", "crawl", "arm-two", "reach"])
def test_same_step_equals_the_hand_driven_twin(torch_gpu, env_id, kw, n, T):
    """Equivalence, bit for bit, over stretches in which every env restarts at least twice — the short shapes run past
    queue_depth steps, so the queue is topped up on the way — with episode ends staggered inside the batch by a manual
    masked reset of the first half after the first step."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    same = gsa.make_vec(env_id, n, device=0, autoreset="same_step", **kw)
    twin = gsa.make_vec(env_id, n, device=0, autoreset=False, **kw)
    assert same.same_step and same.device_autoreset
    o1, _ = same.reset(seed=3)
    o2, _ = twin.reset(seed=3)
    assert torch.equal(o1, o2)
    rng = np.random.default_rng(0)
    ends = np.zeros(n, int)
    for t in range(T):
        a = _actions(env_id, rng, n, same.action_dim)
        out = same.step(a)
        ref = _twin_step(torch, twin, a)
        _assert_step_equal(torch, t, out, ref)
        if env_id == "SoftPendulum3D-v0":          # aux follows obs; the finished step's value goes beside final_obs
            done = ref[4]
            tilt_final = ref[7]["tilt"]
            assert torch.equal(out[4]["final_info"]["tilt"][done], tilt_final[done]), t
            assert torch.equal(out[4]["tilt"][~done], tilt_final[~done]), t
            assert torch.equal(out[4]["tilt"][done].float(), out[0][done][:, 8]), t
        ends += ref[4].cpu().numpy()
        if t == 0:
            m = np.zeros(n, bool)
            m[: n // 2] = True
            assert torch.equal(same.reset(mask=m)[0], twin.reset(mask=m)[0])
    assert ends.min() >= 2, f"every env was meant to restart at least twice: {ends}"
    sa, sb = same.backend.state(), twin.backend.state()
    torch.cuda.synchronize()
    for k in same.backend._snapshot_keys():
        assert np.array_equal(sa[k].cpu().numpy(), sb[k].cpu().numpy(), equal_nan=True), f"state {k!r} differs"
    cons, underflow = same.backend.queue_status()
    assert underflow == 0 and cons.min() >= 2
    if T > same.queue_depth:
        assert int((same._produced - same.queue_depth).min()) > 0, "the queue was meant to be topped up on the way"
    same.close()
    twin.close()


def test_nan_termination_restarts_within_the_call(torch_gpu):
    """A poisoned env reports terminated with the step's own reward and comes back with a finite reset observation in the
    same call; its neighbours are bit-identical to an unpoisoned run."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n, bad = 4, 2
    kw = dict(n_elems=20)
    same = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **kw)
    clean = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **kw)
    twin = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset=False, **kw)
    for e in (same, clean, twin):
        e.reset(seed=3)
    rng = np.random.default_rng(1)
    for t in range(4):
        a = _actions("SoftPendulum-v0", rng, n, 1)
        if t == 2:
            for e in (same, twin):
                e.backend.state()["velocity"][0, bad, 3] = float("nan")
        out = same.step(a)
        oc, rc, tec, trc, _ = clean.step(a)
        ref = _twin_step(torch, twin, a)
        _assert_step_equal(torch, t, out, ref)
        o, r, te, tr, info = out
        others = torch.arange(n, device=o.device) != bad
        assert torch.equal(o[others], oc[others]) and torch.equal(r[others], rc[others]), t
        assert not bool(te[others].any()) and not bool(tr[others].any())
        if t == 2:
            assert bool(te[bad]) and bool(info["_final_obs"][bad]) and float(r[bad]) != 0.0
            assert bool(torch.isfinite(o).all())
            assert float(info["time"][bad]) == 0.0 and float(info["final_info"]["time"][bad]) > 0.0
        else:
            assert not bool(te.any())
    assert same.backend.queue_status()[0].tolist() == [1 if i == bad else 0 for i in range(n)]
    for e in (same, clean, twin):
        e.close()


def test_packed_rows_carry_the_same_step(torch_gpu):
    import gym_softrobot_amd as gsa
    from gym_softrobot_amd.distributed import unpack_outputs

    torch = torch_gpu
    n = 6
    for env_id, kw in (("SoftPendulum-v0", dict(final_time=5e-4, n_elems=20, **SHORT)),
                       ("SoftPendulum3D-v0", dict(final_time=6e-4, n_elems=20, **SHORT)),      # odd obs_dim: a padded row
                       ("OctoFlat-v0", dict(**ARM))):
        dense = gsa.make_vec(env_id, n, device=0, autoreset="same_step", **kw)
        packd = gsa.make_vec(env_id, n, device=0, autoreset="same_step", **kw)
        dense.reset(seed=3)
        packd.reset(seed=3)
        rng = np.random.default_rng(0)
        ends = 0
        for t in range(9):
            a = _actions(env_id, rng, n, dense.action_dim)
            o, r, te, tr, info = dense.step(a)
            packed, pinfo = packd.step_packed(a)
            po, pr, pte, ptr = unpack_outputs(packed, dense.obs_dim)[:4]
            assert torch.equal(o, po) and torch.equal(r, pr), (env_id, t)
            assert torch.equal(te, pte.view(torch.bool)) and torch.equal(tr, ptr.view(torch.bool)), (env_id, t)
            assert set(pinfo) == {"final_obs"} and torch.equal(pinfo["final_obs"], info["final_obs"]), (env_id, t)
            ends += int((te | tr).sum())
        assert ends >= 2 * n
        dense.close()
        packd.close()


def test_an_episode_end_on_every_step(torch_gpu):
    """final_time below one env.step: every env uses one staged record per step.  Left alone, the halved top_up_every
    keeps the queue ahead; with the top-ups paused the shortage is reported, and until then the starved envs stay
    finished with obs == final_obs."""
    import gym_softrobot_amd as gsa
    from gym_softrobot_amd._capi import SoftrodError

    torch = torch_gpu
    kw = dict(final_time=5e-5, time_step=1e-4, recording_fps=10000, n_elems=10)
    n = 3
    a = np.zeros(n, np.float32)
    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **kw)
    assert env.top_up_every == (env.queue_depth - 2) // 2
    env.reset(seed=0)
    steps = 4 * env.queue_depth
    for _ in range(steps):
        o, r, te, tr, info = env.step(a)
    assert bool(tr.all()) and bool(info["_final_obs"].all())
    assert bool((o[:, :2] == 0).all()) and not torch.equal(o, info["final_obs"])      # a fresh episode's observation
    cons, underflow = env.backend.queue_status()
    assert underflow == 0 and cons.tolist() == [steps] * n
    env.close()

    env = gsa.make_vec("SoftPendulum-v0", n, device=0, autoreset="same_step", **kw)
    env.queue_depth = 4
    env.top_up_paused = True
    env.reset(seed=0)
    for t in range(7):
        o, r, te, tr, info = env.step(a)
        assert bool(tr.all()), t
        if t >= 4:                       # four records were staged: from the fifth step on the envs stay finished
            assert torch.equal(o, info["final_obs"]), t
            assert bool((info["time"] > 0).all()), t
        else:
            assert bool((info["time"] == 0).all()), t
    cons, underflow = env.backend.queue_status()
    assert cons.tolist() == [4] * n and underflow == 3 * n
    with pytest.raises(SoftrodError, match="no staged record"):
        env._top_up()
    env.close()


def test_policy_step_as_one_graph_equals_the_eager_loop(torch_gpu):
    """capture_policy_step in same-step mode: the pass behind the step is one more kernel of the captured straight
    line.  Bitwise against the eager loop, backend.final_obs / final_time included; 5-step episodes, 14 steps."""
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
        obs, _ = env.reset(seed=5)
        policy = bench.make_policy(torch, env.backend.device, env.obs_dim, env.action_dim, 22.0)
        replay = env.capture_policy_step(policy) if graphed else None
        rec = []
        for _ in range(steps):
            out = replay() if graphed else env.step(policy(obs))[:4]
            obs = out[0]
            be = env.backend
            rec.append(tuple(x.detach().cpu().clone() for x in (*out, be.final_obs, be.final_time)))
        torch.cuda.synchronize()
        cons, underflow = env.backend.queue_status()
        env.close()
        return rec, cons, underflow

    (a, ca, ua), (b, cb, ub) = run(False), run(True)
    assert ua == ub == 0 and ca.tolist() == cb.tolist() and ca.min() >= 2
    for t, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("obs", "reward", "terminated", "truncated", "final_obs", "final_time"), x, y):
            assert np.array_equal(u.numpy(), v.numpy(), equal_nan=True), f"step {t + 1}: {name} differs"


def test_early_termination_keeps_the_finished_steps_time_limit_flag(torch_gpu):
    """config_early_termination: `truncated` carries the Hamiltonian cut-off too, and infos["TimeLimit.truncated"] comes
    from the env_aux row the epilogue writes; the reset behind the step leaves that row alone."""
    import gym_softrobot_amd as gsa

    torch = torch_gpu
    n = 8
    kw = dict(final_time=0.06, config_early_termination=True)
    same = gsa.make_vec("OctoArmPush-v1", n, device=0, autoreset="same_step", **kw)
    twin = gsa.make_vec("OctoArmPush-v1", n, device=0, autoreset=False, **kw)
    same.reset(seed=1)
    twin.reset(seed=1)
    rng = np.random.default_rng(2)
    saw_tl = saw_cut = False
    for t in range(9):
        a = _actions("OctoArmPush-v1", rng, n, 2)
        a[: n // 4, 1] = 0.0                    # a quarter of the envs never activate the muscle: the cut-off ends them
        out = same.step(a)
        ref = _twin_step(torch, twin, a)
        _assert_step_equal(torch, t, out, ref)
        tl = np.asarray(ref[7]["TimeLimit.truncated"])
        np.testing.assert_array_equal(out[4]["TimeLimit.truncated"].cpu().numpy(), tl, err_msg=f"step {t}")
        saw_tl |= bool(tl.any())
        saw_cut |= bool((ref[3].cpu().numpy() & ~tl).any())
    assert saw_tl and saw_cut
    same.close()
    twin.close()


def test_c_abi_refusals(torch_gpu, hip_lib):
    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    be = HipRodBackend(_capi.softpendulum_config(2, n_elems=10), 0)
    ptrs = [C.c_void_p() for _ in range(3)]
    refs = [C.byref(p) for p in ptrs]
    assert hip_lib.softrod_autoreset_same_step(be._h, 1) == -1
    assert hip_lib.softrod_last_error(be._h) == b"call softrod_autoreset_enable first"
    assert hip_lib.softrod_final_view(be._h, *refs) == -1
    be.autoreset_enable(4)
    assert hip_lib.softrod_final_view(be._h, *refs) == -1            # same-step is still off
    assert b"softrod_autoreset_same_step" in hip_lib.softrod_last_error(be._h)
    assert not any(p.value for p in ptrs)
    be.autoreset_same_step(True)
    assert hip_lib.softrod_final_view(be._h, *refs) == 0 and all(p.value for p in ptrs)
    assert be.final_obs.shape == (2, 4) and be.final_time.shape == (2,) and be.final_aux.shape == (2,)
    assert float(be.final_obs.abs().sum()) == 0.0                    # zero-filled until an episode ends
    first = [p.value for p in ptrs]
    be.autoreset_same_step(False)                                    # back to NEXT_STEP
    assert hip_lib.softrod_final_view(be._h, *refs) == -1
    be.autoreset_same_step(True)                                     # the buffers are the handle's: same pointers
    assert hip_lib.softrod_final_view(be._h, *refs) == 0 and [p.value for p in ptrs] == first
    be.close()
