"""copy_envs() / fork() on the MI355X (softrod_copy_envs): a fork equals the host path snapshot() -> permute rows ->
restore() to the bit, a copy and its source continue bitwise equal, the per-env tables travel, the read-outs agree,
every refusal leaves the state alone, fork() moves the host bookkeeping, and the planner example runs.

N = 6 envs at the registered defaults; the pairs are (0 -> 1), (0 -> 2), (3 -> 5): one source twice, env 4 untouched,
and on OctoFlat (four envs per workgroup) copies inside a workgroup and across two."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.registration import registered

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
N = 6
SRC, DST = [0, 0, 3], [1, 2, 5]
UNTOUCHED = [0, 3, 4]
# every registered id, the two-slot muscle arm (lane_stride 128) and ArmPush's env_aux
CASES = [(i, {}) for i in registered()] + [("OctoArmPush-v1", {"n_elems": 100}),
                                           ("OctoArmPush-v1", {"config_early_termination": True})]
CASE_IDS = [i + "".join(f",{k}={v}" for k, v in kw.items()) for i, kw in CASES]
ENV_AXIS0 = ("time", "env_memory", "prev_action", "prev_kappa", "env_material", "env_contact")   # [n_envs, ...]; the rest [comps, n_envs, ...]
PER_ARM = ("sucker_ratio", "sucker_index")      # [4][n_envs * per]: per = n_arm on the muscle octopus, else 1

_envs = {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in _envs.values():
        env.close()
    _envs.clear()


def _env(case):
    """One env per case for the whole module (every test starts from reset(seed=0))."""
    key = CASE_IDS[CASES.index(case)]
    if key not in _envs:
        _envs[key] = gsa.make_vec(case[0], N, **case[1])
    return _envs[key]


def _per(env):
    return int(env.cfg.n_arm) if env.backend.is_mocto else 1


def _by_env(key, t, per):
    """`t` with the env axis first (a view where the layout allows, for in-place edits of a snapshot)."""
    if key in PER_ARM:
        t = t.reshape(t.shape[0], -1, per)
    if key in ENV_AXIS0:
        return t
    return t.transpose(0, 1) if torch.is_tensor(t) else np.swapaxes(t, 0, 1)


def _state(env):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in env.backend.state().items() if torch.is_tensor(v)}


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _assert_rows_equal(env, st, a_envs, b_envs, what):
    """Env b's part of every state array is env a's, bitwise."""
    for k, v in st.items():
        rows = _by_env(k, v, _per(env))
        for a, b in zip(a_envs, b_envs):
            assert _same(rows[a], rows[b]), f"{what}: {k} of env {b} differs from env {a}"


def _assert_states_equal(env, got, want, envs, what):
    assert got.keys() == want.keys()
    for k in got:
        g, w = _by_env(k, got[k], _per(env)), _by_env(k, want[k], _per(env))
        for e in envs:
            assert _same(g[e], w[e]), f"{what}: {k} of env {e}"


def _actions(env, rng, t=None):
    if getattr(env, "mode", None) == 0:                       # OctoArmPush-v0: the index 0 / 1
        if t is not None:                                     # the warm-up: no two envs of a pair act alike
            return ((np.arange(N) >> t) & 1).astype(np.float32).reshape(N, env.action_dim)
        return rng.integers(0, 2, (N, env.action_dim)).astype(np.float32)
    lo, hi = env.action_low, env.action_high
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return (mid + 0.3 * half * rng.uniform(-1, 1, (N, env.action_dim))).astype(np.float32)


def _paired(a):
    a = a.copy()
    a[DST] = a[SRC]
    return a


def _step(env, a):
    out = env.step(a)[:4]
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in out]


def _warm(env, seed=0):
    """reset(seed=0) and two steps with distinct random actions per env."""
    rng = np.random.default_rng(seed)
    env.reset(seed=0)
    for t in range(2):
        _step(env, _actions(env, rng, t))
    return rng


def _assert_pairs_differ(env, st):
    """Before a copy every copy-to-be differs from its source somewhere: the equalities asserted later are not trivial."""
    for a, b in zip(SRC, DST):
        assert any(not _same(_by_env(k, v, _per(env))[a], _by_env(k, v, _per(env))[b]) for k, v in st.items()), (a, b)


def _permuted(env, snap):
    """The snapshot with rows DST overwritten by rows SRC on the host."""
    snap = {k: v.clone() for k, v in snap.items()}
    for k, v in snap.items():
        if k != "config_fingerprint":
            rows = _by_env(k, v, _per(env))
            rows[DST] = rows[SRC].clone()
    return snap


def _assert_continuation(env, rng, steps=3):
    for t in range(steps):
        out = _step(env, _paired(_actions(env, rng)))
        for name, x in zip(("obs", "reward", "terminated", "truncated"), out):
            assert _same(x[DST], x[SRC]), f"step {t}: {name} of the copies differs from their sources'"
    _assert_rows_equal(env, _state(env), SRC, DST, f"after {steps} steps")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_control_step_does_not_depend_on_batch_position(hip_lib, case):
    """Holds without copy_envs: rows copied on the host step like their sources.  What tests 2 and 3 lean on."""
    env = _env(case)
    rng = _warm(env)
    env.backend.restore(_permuted(env, env.backend.snapshot()))
    _assert_rows_equal(env, _state(env), SRC, DST, "after restore")
    out = _step(env, _paired(_actions(env, rng)))
    for name, x in zip(("obs", "reward", "terminated", "truncated"), out):
        assert _same(x[DST], x[SRC]), name
    _assert_rows_equal(env, _state(env), SRC, DST, "after one step")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_copy_equals_the_host_path(hip_lib, case):
    env = _env(case)
    _warm(env)
    before, snap = _state(env), env.backend.snapshot()
    _assert_pairs_differ(env, before)
    env.backend.copy_envs(SRC, DST)
    got = _state(env)
    _assert_states_equal(env, got, before, UNTOUCHED, "sources and env 4 after copy_envs")
    _assert_rows_equal(env, got, SRC, DST, "after copy_envs")
    env.backend.restore(_permuted(env, snap))
    want = _state(env)
    for k in want:
        assert _same(got[k], want[k]), f"{k}: copy_envs differs from snapshot -> permute -> restore"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_copies_continue_bitwise(hip_lib, case):
    env = _env(case)
    rng = _warm(env)
    _assert_pairs_differ(env, _state(env))
    env.backend.copy_envs(SRC, DST)
    _assert_continuation(env, rng)


def _set_rows(env, table):
    f = 1.0 + 0.1 * np.arange(N)
    if table == "material":
        env.set_material(youngs_modulus=env.cfg.youngs_modulus * f, density=env.cfg.density / f,
                         damping_constant=env.cfg.damping_constant * (2.0 - 0.1 * np.arange(N)))
    else:
        env.set_contact(contact_k=env.cfg.contact_k * f, contact_nu=env.cfg.contact_nu / f,
                        kinetic_mu=np.outer(f, np.array(list(env.cfg.kinetic_mu))))


@pytest.mark.parametrize("env_id,table", [("SoftPendulum-v0", "material"), ("SoftPendulum3D-v0", "material"),
                                          ("OctoArmSingle-v0", "material"), ("OctoArmSingle-v0", "contact"),
                                          ("OctoFlat-v0", "contact")])
def test_per_env_tables_travel(hip_lib, env_id, table):
    env = gsa.make_vec(env_id, N)
    try:
        read = getattr(env, table)
        rng = _warm(env)
        defaults = read()
        env.fork(SRC, DST)                                    # before the first set_*: no table exists yet
        for k, v in read().items():
            assert _same(v, defaults[k]), k
        _assert_continuation(env, rng, steps=1)
        _set_rows(env, table)
        mine = read()
        assert all(any(not _same(v[[a]], v[[b]]) for v in mine.values()) for a, b in zip(SRC, DST))
        _step(env, _actions(env, rng))
        env.fork(SRC, DST)
        for k, v in read().items():
            assert _same(v[DST], mine[k][SRC]) and _same(v[UNTOUCHED], mine[k][UNTOUCHED]), k
        carried = env.backend.snapshot()["env_" + table].numpy()
        assert _same(carried[DST], carried[SRC]) and not _same(carried[[1]], carried[[4]])
        _assert_continuation(env, rng)
        # a later masked set_* uploads the whole table from the library's host copy: the copied rows stay
        if table == "material":
            env.set_material(np.arange(N) == 4, density=2.0 * env.cfg.density)
        else:
            env.set_contact(np.arange(N) == 4, contact_k=2.0 * env.cfg.contact_k)
        _assert_continuation(env, rng, steps=1)
    finally:
        env.close()


@pytest.mark.parametrize("env_id,readout", [("OctoArmPush-v1", "rod_strains"), ("OctoFlat-v0", "rod_energies"),
                                            ("OctoArmSingle-v0", "rod_dynamics")])
def test_readouts_of_a_copy_equal_its_source(hip_lib, env_id, readout):
    env = _env((env_id, {}))
    _warm(env)
    before = getattr(env, readout)()
    before = [t.cpu().numpy().copy() for t in (before if isinstance(before, tuple) else (before,))]
    assert not all(_same(t[DST], t[SRC]) for t in before)     # the envs differ before the fork
    env.fork(SRC, DST)
    after = getattr(env, readout)()
    torch.cuda.synchronize()
    for t in (after if isinstance(after, tuple) else (after,)):
        t = t.cpu().numpy()
        assert _same(t[DST], t[SRC])


REFUSED = [
    ([0] * (N + 1), list(range(N + 1)), f"copy envs: count {N + 1} is outside 0 .. n_envs = {N}"),
    ([0], [N], f"copy envs: env index {N} (pair 0) is outside 0 .. {N - 1}"),
    ([0, N], [1, 2], f"copy envs: env index {N} (pair 1) is outside 0 .. {N - 1}"),
    ([-1], [1], f"copy envs: env index -1 (pair 0) is outside 0 .. {N - 1}"),
    ([0, 3], [1, 1], "copy envs: env 1 appears twice in dst"),
    ([0, 1], [1, 2], "copy envs: env 1 is the dst of one pair and the src of another"),
    ([0, 1], [1, 0], "copy envs: env 0 is the dst of one pair and the src of another"),
]


@pytest.mark.parametrize("env_id", ["SoftPendulum-v0", "OctoCrawl-v0"])
def test_refusals_change_nothing(hip_lib, env_id):
    env = _env((env_id, {}))
    _warm(env)
    be = env.backend
    before = _state(env)
    for src, dst, text in REFUSED:
        for call in (be.copy_envs, env.fork):
            with pytest.raises(_capi.SoftrodError) as err:
                call(src, dst)
            assert str(err.value).endswith(text), (src, dst, str(err.value))
    # what the Python layer cannot express: the raw call
    raw, stream = be._lib.softrod_copy_envs, be._stream()
    one = np.zeros(1, np.int32)
    for args, text in (((None, one.ctypes.data, 1), b"copy envs: null src or dst"),
                       ((one.ctypes.data, None, 1), b"copy envs: null src or dst"),
                       ((one.ctypes.data, one.ctypes.data, -1), b"copy envs: count -1 is outside 0 .. n_envs = 6")):
        assert raw(be._h, *args, stream) == -1
        assert be._lib.softrod_last_error(be._h) == text
    assert raw(None, one.ctypes.data, one.ctypes.data, 1, stream) == -1
    assert be._lib.softrod_last_error(None) == b"copy envs: null handle"
    steps = env._steps.copy()
    # accepted no-ops
    be.copy_envs([], [])
    env.fork([], [])
    be.copy_envs([2], [2])
    env.fork([2, 4], [2, 4])
    assert raw(be._h, None, None, 0, stream) == 0
    _assert_states_equal(env, _state(env), before, range(N), "after refused calls and no-ops")
    assert (env._steps == steps).all()


def test_device_autoreset_refuses_at_both_levels(hip_lib):
    env = gsa.make_vec("SoftPendulum-v0", N, autoreset="device")
    try:
        env.reset(seed=0)
        before = _state(env)
        with pytest.raises(NotImplementedError, match="autoreset='device'"):
            env.fork(0, [1])
        with pytest.raises(_capi.SoftrodError, match="copy envs: not on a handle with device-side auto-reset"):
            env.backend.copy_envs(0, [1])
        _assert_states_equal(env, _state(env), before, range(N), "after the refusals")
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["SoftPendulum-v0", "OctoFlat-v0", "OctoReach-v0"])
def test_fork_moves_the_host_bookkeeping(hip_lib, env_id):
    env = _env((env_id, {}))
    rng = _warm(env)
    env.reset(mask=np.arange(N) == 3)                          # env 3 is two steps behind the others
    _step(env, _actions(env, rng))
    env._needs_reset[0] = True                                 # as a host auto-reset would flag it
    steps = env._steps.copy()
    targets = None if getattr(env, "targets", None) is None else env.targets.copy()
    assert steps.tolist() == [3, 3, 3, 1, 3, 3]
    env.fork(SRC, DST)
    assert env._steps.tolist() == [3, 3, 3, 1, 3, 1]
    assert env._needs_reset.tolist() == [True, True, True, False, False, False]
    if targets is not None:
        assert _same(env.targets[DST], targets[SRC]) and _same(env.targets[UNTOUCHED], targets[UNTOUCHED])
    # copy_rng=True: the copies draw their source's next reset
    mask = np.zeros(N, bool)
    mask[SRC + DST] = True
    obs = env.reset(mask=mask)[0].cpu().numpy().copy()
    assert _same(obs[DST], obs[SRC])
    _assert_rows_equal(env, _state(env), SRC, DST, "after the masked reset")
    if targets is not None:
        assert _same(env.targets[DST], env.targets[SRC])
    assert not env._needs_reset[mask].any()


def test_fork_without_copy_rng_keeps_the_streams_apart(hip_lib):
    env = _env(("SoftPendulum-v0", {}))
    _warm(env)
    env.fork(SRC, DST, copy_rng=False)
    mask = np.zeros(N, bool)
    mask[SRC + DST] = True
    obs = env.reset(mask=mask)[0].cpu().numpy().copy()        # SoftPendulum draws its initial angle
    for s, d in zip(SRC, DST):
        assert not _same(obs[d], obs[s])


def test_example_runs(hip_lib):
    """examples/soft_pendulum_cem.py at a tiny size, in a fresh child process under its own time limit."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, str(ROOT / "examples" / "soft_pendulum_cem.py"),
           "--num-envs", "8", "--horizon", "2", "--iters", "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "return of the controlled trajectory over 1 planning steps" in r.stdout
