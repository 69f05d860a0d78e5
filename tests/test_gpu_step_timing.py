"""softrod_set_timing's records ride on the step's own dispatches (launch_stamped, softrod_capi.hip): the start event on
the first kernel of an env.step, the stop event on the last, no event record in front of or behind the kernels.

Held here: timing changes no byte of what a step computes (5, 50 and 63 elements: padding-heavy, the flagship, the
lane-filling rod); one entry per env.step, each positive, their sum within the wall time of the synchronised window that
held them; a step of SEVERAL kernels — the windowed 100-element arm: its substeps on the two-window kernel, then reward and
observation by the handle's plain kernel — still yields one entry per env.step (launch_step counts one per call and
softrod_step calls it once), and that entry spans both kernels; re-arming starts again at entry 0."""
import time

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa

pytestmark = pytest.mark.gpu

N_ENVS, STEPS = 8, 3
STATE_ROWS = ("position", "velocity", "director", "omega", "tangents", "time")


def _pendulum_run(n_elems, timed):
    """STEPS env.steps of N_ENVS SoftPendulum-v0 envs -> (bytes of every output and state row, entries, wall ms)."""
    env = gsa.make_vec("SoftPendulum-v0", N_ENVS, device=0, n_elems=n_elems)
    env.reset(seed=0)
    acts = np.random.default_rng(3).uniform(-22, 22, (STEPS, N_ENVS)).astype(np.float32)
    env.backend.set_timing(STEPS if timed else 0)
    got = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(STEPS):
        res = env.step(acts[t])
        got.append([r.clone() for r in res[:4]])
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    entries = env.backend.kernel_times_ms() if timed else np.zeros(0, np.float32)
    st = env.backend.state()
    blob = [r.cpu().numpy().tobytes() for step in got for r in step] + [st[name].cpu().numpy().tobytes() for name in STATE_ROWS]
    env.close()
    return blob, entries, wall_ms


@pytest.fixture(scope="module")
def runs():
    return {ne: {timed: _pendulum_run(ne, timed) for timed in (True, False)} for ne in (5, 50, 63)}


@pytest.mark.parametrize("n_elems", [5, 50, 63])
def test_timing_changes_no_byte(runs, n_elems):
    timed, plain = runs[n_elems][True][0], runs[n_elems][False][0]
    names = [f"step {t + 1} {o}" for t in range(STEPS) for o in ("obs", "reward", "terminated", "truncated")] + list(STATE_ROWS)
    assert len(timed) == len(plain) == len(names)
    for name, a, b in zip(names, timed, plain):
        assert a == b, f"n_elems {n_elems}: {name} differs between a timed and an untimed run"


@pytest.mark.parametrize("n_elems", [5, 50, 63])
def test_one_positive_entry_per_step_within_the_wall_time(runs, n_elems):
    _, entries, wall_ms = runs[n_elems][True]
    print(f"n_elems {n_elems}: entries {entries.tolist()} ms, wall {wall_ms:.3f} ms")
    assert len(entries) == STEPS
    assert (entries > 0).all()
    assert float(entries.sum()) <= wall_ms
    assert len(runs[n_elems][False][1]) == 0


def test_one_pair_brackets_every_kernel_of_a_step(runs):
    single = runs[50][True][1]
    env = gsa.make_vec("OctoArmSingle-v0", 4, device=0, n_elems=100)
    assert "window" in env.backend.kernel_tier()        # two kernels per env.step: the windows' substeps, then the epilogue
    env.reset(seed=0)
    acts = np.random.default_rng(5).uniform(-1, 1, (STEPS, 4, env.backend.action_dim)).astype(np.float32)
    env.backend.set_timing(STEPS)
    for t in range(STEPS):
        env.step(acts[t])
    entries = env.backend.kernel_times_ms()
    env.close()
    print(f"arm-100 entries {entries.tolist()} ms, SoftPendulum entries {single.tolist()} ms")
    assert len(entries) == STEPS                         # one launch_step per softrod_step, one entry per launch_step
    assert (entries >= float(single.max())).all()


def test_rearmed_timing_starts_at_entry_zero():
    env = gsa.make_vec("SoftPendulum-v0", N_ENVS, device=0)
    env.reset(seed=0)
    acts = np.zeros(N_ENVS, np.float32)
    be = env.backend
    be.set_timing(4)
    for _ in range(3):
        env.step(acts)
    assert len(be.kernel_times_ms()) == 3
    be.set_timing(0)
    env.step(acts)
    assert len(be.kernel_times_ms()) == 0
    be.set_timing(2)
    assert len(be.kernel_times_ms()) == 0
    for _ in range(3):                                   # the third is past the ring: untimed
        env.step(acts)
    entries = be.kernel_times_ms()
    env.close()
    assert len(entries) == 2 and (entries > 0).all()
