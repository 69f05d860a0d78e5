"""The state bank on the MI355X (softrod_bank_create / _save / _load): a save and a load equal the host path
snapshot() -> pick rows -> restore() to the bit, a loaded env continues bitwise as the env it was saved from did, the
bank changes nothing it is not asked to, the per-env tables, the reset-shape rows and the host bookkeeping travel,
every refusal leaves the batch and the bank alone, the single env returns to a saved state, and the example runs.

N = 6 envs, K = 4 slots at the registered defaults, after a warm-up of two random steps.  Envs 1 and 4 are saved into
slots 3 and 0; slots 3, 0, 3 are loaded into envs 0, 2, 5: slot index and env index differ on every pair, one slot
feeds two envs, envs 1, 3 and 4 stay untouched — a wrong component stride on the bank's side (K where the batch has
N) lands in another slot or env and shows.  Everything is compared bitwise."""
import copy
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from tests import reset_shapes_ref as shapes_ref
from tests.test_gpu_copy_envs import CASE_IDS, CASES, ENV_AXIS0, PER_ARM, N, _actions, _same, _set_rows, _state, _step, _warm

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
K = 4
SAVE_ENVS, SAVE_SLOTS = [1, 4], [3, 0]
LOAD_SLOTS, LOAD_ENVS = [3, 0, 3], [0, 2, 5]
LOADED_FROM = [1, 4, 1]                       # the env each loaded env is a copy of
UNTOUCHED = [1, 3, 4]
AXIS0 = ENV_AXIS0 + ("reset_shape_index", "reset_shape_episode")

_envs = {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in _envs.values():
        env.close()
    _envs.clear()


def _env(case):
    """One env with a bank per case for the whole module (every test starts from reset(seed=0))."""
    key = CASE_IDS[CASES.index(case)]
    if key not in _envs:
        _envs[key] = gsa.make_vec(case[0], N, **case[1])
        _envs[key].create_state_bank(K)
    return _envs[key]


def _snap(env):
    """backend.snapshot() as NumPy arrays with the env axis first."""
    per = int(env.cfg.n_arm) if env.backend.is_mocto else 1
    out = {}
    for k, v in env.backend.snapshot().items():
        if k == "config_fingerprint":
            continue
        a = v.numpy().copy()
        if k in PER_ARM:
            a = a.reshape(a.shape[0], -1, per)
        out[k] = a if k in AXIS0 else np.swapaxes(a, 0, 1)
    return out


def _assert_rows(got, got_envs, want, want_envs, what):
    assert got.keys() == want.keys()
    for k in got:
        for g, w in zip(got_envs, want_envs):
            assert _same(got[k][g], want[k][w]), f"{what}: {k} of env {g}"


def _save_step_load(env):
    """The flow of tests 1 and 2: warm up, save, three recorded steps, load."""
    rng = _warm(env)
    first = _snap(env)
    assert any(not _same(v[SAVE_ENVS[0]], v[SAVE_ENVS[1]]) for v in first.values())      # the two slots will differ
    env.save_states(SAVE_ENVS, SAVE_SLOTS)
    acts, outs = [], []
    for _ in range(3):
        acts.append(_actions(env, rng))
        outs.append(_step(env, acts[-1]))
    before_load = _snap(env)
    env.load_states(LOAD_SLOTS, LOAD_ENVS)
    return rng, first, acts, outs, before_load


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_save_and_load_equal_the_host_path(hip_lib, case):
    env = _env(case)
    _, first, _, _, before_load = _save_step_load(env)
    got = _snap(env)
    _assert_rows(got, LOAD_ENVS, first, LOADED_FROM, "loaded envs against their sources at the save")
    _assert_rows(got, UNTOUCHED, before_load, UNTOUCHED, "the other envs against the snapshot before the load")
    assert any(not _same(got[k][0], before_load[k][0]) for k in got)         # the load did change env 0
    assert env.state_bank_slots == K and env.state_bank_filled.tolist() == [True, False, False, True]
    # a slot holds at least what the snapshot carries of the rod itself
    assert env.state_bank_bytes >= sum(got[k][0].nbytes for k in ("position", "velocity", "director", "omega", "time"))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_loaded_envs_continue_bitwise(hip_lib, case):
    env = _env(case)
    rng, _, acts, outs, _ = _save_step_load(env)
    for t in range(3):
        a = _actions(env, rng)
        a[LOAD_ENVS] = acts[t][LOADED_FROM]                   # what their sources received after the save
        out = _step(env, a)
        for name, x, was in zip(("obs", "reward", "terminated", "truncated"), out, outs[t]):
            assert _same(x[LOAD_ENVS], was[LOADED_FROM]), f"step {t}: {name} of the loaded envs differs from their sources'"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_bank_is_inert(hip_lib, case):
    """Two fresh batches (what survives a reset, such as the previous action, is then the same in both), one with a bank."""
    env, twin = gsa.make_vec(case[0], N, **case[1]), gsa.make_vec(case[0], N, **case[1])
    try:
        env.create_state_bank(K)
        assert twin.state_bank_slots == 0

        def both(what, call):
            a, b = call(env), call(twin)
            torch.cuda.synchronize()
            for x, y in zip(a, b):
                assert _same(x.cpu().numpy(), y.cpu().numpy()), what

        rng = np.random.default_rng(0)
        both("reset", lambda e: e.reset(seed=0)[:1])
        for t in range(2):
            a = _actions(env, rng, t)
            both(f"warm-up step {t}", lambda e: e.step(a)[:4])
        env.save_states(SAVE_ENVS, SAVE_SLOTS)
        saved = _snap(env)
        both("reset after the save", lambda e: e.reset()[:1])
        for t in range(2):
            a = _actions(env, rng)
            both(f"step {t} after the save", lambda e: e.step(a)[:4])
        _assert_rows(_snap(env), range(N), _snap(twin), range(N), "the batch with a bank against the one without")
        env.load_states(SAVE_SLOTS, [0, 2])
        _assert_rows(_snap(env), [0, 2], saved, SAVE_ENVS, "a load after a reset and two steps")
    finally:
        env.close()
        twin.close()


@pytest.mark.parametrize("env_id,table", [("SoftPendulum-v0", "material"), ("SoftPendulum3D-v0", "material"),
                                          ("OctoArmSingle-v0", "material"), ("OctoArmSingle-v0", "contact"),
                                          ("OctoFlat-v0", "contact")])
def test_per_env_tables_travel(hip_lib, env_id, table):
    env = gsa.make_vec(env_id, N)
    try:
        read = getattr(env, table)

        def assert_step_alike(a_env, b_env, what):
            a = _actions(env, rng)
            a[b_env] = a[a_env]
            for name, x in zip(("obs", "reward", "terminated", "truncated"), _step(env, a)):
                assert _same(x[[a_env]], x[[b_env]]), f"{what}: {name}"

        rng = _warm(env)
        env.create_state_bank(K)
        defaults = read()
        env.save_states([1], [2])                             # before the first set_*: no table exists yet
        _set_rows(env, table)                                 # the table is created after the bank and after a save
        mine = read()
        _step(env, _actions(env, rng))
        env.save_states(SAVE_ENVS, SAVE_SLOTS)
        env.load_states(LOAD_SLOTS, LOAD_ENVS)
        for k, v in read().items():
            assert _same(v[LOAD_ENVS], mine[k][LOADED_FROM]) and _same(v[UNTOUCHED], mine[k][UNTOUCHED]), k
        carried = env.backend.snapshot()["env_" + table].numpy()
        assert _same(carried[LOAD_ENVS], carried[LOADED_FROM]) and not _same(carried[[1]], carried[[4]])
        assert_step_alike(1, 0, "env 0, loaded from env 1's slot")        # the device rows travelled too
        # a later masked set_* uploads the whole table from the library's host copy: the loaded rows stay
        env.load_states([3], [5])
        env.load_states([3], [0])
        if table == "material":
            env.set_material(np.arange(N) == 4, density=2.0 * env.cfg.density)
        else:
            env.set_contact(np.arange(N) == 4, contact_k=2.0 * env.cfg.contact_k)
        assert_step_alike(0, 5, "after a masked set")
        # the slot saved before the table existed loads the uniform row: its env as it would be now, left alone
        env.load_states([2, 2], [3, 0])
        now = read()
        for k, v in now.items():
            assert _same(v[[3]], defaults[k][[3]]) and _same(v[[0]], defaults[k][[0]]), k
            assert _same(v[[1, 2, 5]], mine[k][[1, 4, 1]]), k
        # ... in the library too: env 0 keeps the loaded row, env 3 is given the config's values by hand
        (env.set_material if table == "material" else env.set_contact)(np.arange(N) == 3, **defaults)
        assert_step_alike(3, 0, "the uniform row")
    finally:
        env.close()


def test_reset_shape_rows_travel(hip_lib):
    env = gsa.make_vec("SoftPendulum-v0", N, n_elems=20)
    late = gsa.make_vec("SoftPendulum-v0", N, n_elems=20)
    try:
        known, pool = shapes_ref.KNOWN, shapes_ref.pool(env.cfg, 1, shapes_ref.KNOWN_K)
        env.set_reset_shapes(**pool, seed=shapes_ref.KNOWN_SEED)
        env.create_state_bank(K)
        env.reset(seed=1)
        env.reset(mask=np.arange(N) == 0)                     # env 0: its second start
        idx, ep = [known[0][1]] + [known[e][0] for e in range(1, N)], [2, 1, 1, 1, 1, 1]
        assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == ep
        env.save_states([0], [1])
        env.load_states([1], [2], copy_rng=True)              # the index and the ordinal travel
        idx[2], ep[2] = idx[0], 2
        assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == ep
        assert idx[1] != idx[0]
        env.load_states([1], [1], copy_rng=False)             # the index travels, the ordinal stays the env's own
        idx[1] = idx[0]
        assert env.reset_shape_index.tolist() == idx and env.reset_shape_episode.tolist() == ep
        # a new pool restarts every env's sequence of starts, and every slot's
        env.set_reset_shapes(**pool, seed=9)
        env.reset(mask=np.arange(N) == 4)
        assert env.reset_shape_episode.tolist() == [0, 0, 0, 0, 1, 0] and int(env.reset_shape_index[4]) >= 0
        env.load_states([1], [4])
        assert env.reset_shape_index.tolist() == [-1] * N and env.reset_shape_episode.tolist() == [0] * N
        # the first pool of a handle set after the bank and after a save: the rows' twins are made then
        late.create_state_bank(K)
        late.reset(seed=1)
        late.save_states([0], [1])
        late.set_reset_shapes(**pool, seed=shapes_ref.KNOWN_SEED)
        late.reset(mask=np.arange(N) < 2)
        assert late.reset_shape_episode.tolist() == [1, 1, 0, 0, 0, 0]
        late.load_states([1], [1])
        assert late.reset_shape_index.tolist() == [known[0][0], -1, -1, -1, -1, -1]
        assert late.reset_shape_episode.tolist() == [1, 0, 0, 0, 0, 0]
    finally:
        env.close()
        late.close()


def _host(x):
    return x.cpu().numpy().copy() if torch.is_tensor(x) else np.array(x)


@pytest.mark.parametrize("env_id", ["SoftPendulum-v0", "OctoFlat-v0", "OctoReach-v0"])
def test_host_bookkeeping_travels(hip_lib, env_id):
    env = gsa.make_vec(env_id, N, autoreset=True)
    try:
        rng = _warm(env)
        env.create_state_bank(K)
        env.reset(mask=np.arange(N) == 3)                      # env 3 is two steps behind the others
        _step(env, _actions(env, rng))
        assert env._steps.tolist() == [3, 3, 3, 1, 3, 3] and not env._needs_reset.any()
        has_targets = getattr(env, "targets", None) is not None
        targets = env.targets.copy() if has_targets else None
        env._needs_reset[0] = True                             # as the host auto-reset flags a finished env
        env.save_states([3, 0], [1, 2])
        streams = [copy.deepcopy(g.bit_generator.state) for g in env._rngs]
        a = _actions(env, rng)
        obs, _, _, _, infos = env.step(a)                      # env 0 restarts here, from its stream as it was saved
        obs0, time3 = _host(obs)[0], _host(infos["time"])[3]
        targets0 = env.targets[0].copy() if has_targets else None
        assert env._steps.tolist() == [0, 4, 4, 2, 4, 4] and not env._needs_reset.any()
        env.load_states([1, 2], [5, 4])
        assert env._steps.tolist() == [0, 4, 4, 2, 3, 1]
        assert env._needs_reset.tolist() == [False, False, False, False, True, False]
        if has_targets:
            assert _same(env.targets[[5, 4]], targets[[3, 0]]) and _same(env.targets[[1, 2, 3]], targets[[1, 2, 3]])
        assert env._rngs[5].bit_generator.state == streams[3] and env._rngs[4].bit_generator.state == streams[0]
        a[5] = a[3]
        obs, reward, term, trunc, infos = env.step(a)
        # env 5 is env 3 as saved: the same step again; env 4 carried env 0's pending reset, which fires with the same draws
        assert _host(infos["time"])[5] == time3 and env._steps.tolist() == [1, 5, 5, 3, 0, 2]
        assert _same(_host(obs)[4], obs0) and float(_host(reward)[4]) == 0.0 and not _host(term)[4] and not _host(trunc)[4]
        if has_targets:
            assert _same(env.targets[4], targets0)
        assert not env._needs_reset.any()
        # copy_rng=False: the env keeps its own stream, and its next reset draws from it
        own = copy.deepcopy(env._rngs[2].bit_generator.state)
        env.load_states([2], [2], copy_rng=False)
        assert env._rngs[2].bit_generator.state == own and own != streams[0]
        assert env._needs_reset[2] and env._steps[2] == 3
        obs = env.step(a)[0]
        assert env._steps[2] == 0 and env._rngs[2].bit_generator.state != own
        assert not (_same(_host(obs)[2], obs0) and (not has_targets or _same(env.targets[2], targets0)))
    finally:
        env.close()


def _refused(n, k):
    save = [([n], [0], f"bank save: env index {n} (pair 0) is outside 0 .. {n - 1}"),
            ([0, -1], [0, 1], f"bank save: env index -1 (pair 1) is outside 0 .. {n - 1}"),
            ([0], [k], f"bank save: slot index {k} (pair 0) is outside 0 .. {k - 1}"),
            ([0, 1], [1, -2], f"bank save: slot index -2 (pair 1) is outside 0 .. {k - 1}"),
            ([0, 1], [1, 1], "bank save: slot 1 appears twice"),
            ([0] * (k + 1), list(range(k)) + [0], f"bank save: count {k + 1} is outside 0 .. slots = {k}")]
    load = [([2], [n], f"bank load: env index {n} (pair 0) is outside 0 .. {n - 1}"),
            ([k], [0], f"bank load: slot index {k} (pair 0) is outside 0 .. {k - 1}"),
            ([2, 2], [1, 1], "bank load: env 1 appears twice"),
            ([2, 0], [1, 3], "bank load: slot 0 holds no state"),
            ([2] * (n + 1), list(range(n + 1)), f"bank load: count {n + 1} is outside 0 .. n_envs = {n}")]
    return save, load


@pytest.mark.parametrize("env_id", ["SoftPendulum-v0", "OctoCrawl-v0"])
def test_refusals_change_nothing(hip_lib, env_id):
    env = gsa.make_vec(env_id, N)
    try:
        _warm(env)
        be = env.backend
        before = _snap(env)
        for call, args in ((env.save_states, ([0], [1])), (be.bank_save, ([0], [1])),
                           (env.load_states, ([1], [0])), (be.bank_load, ([1], [0]))):
            with pytest.raises(_capi.SoftrodError, match=r"the handle has no state bank \(softrod_bank_create\)"):
                call(*args)
        for bad in (0, -3):
            with pytest.raises(_capi.SoftrodError, match=f"bank create: slots {bad} is not positive"):
                env.create_state_bank(bad)
        assert env.state_bank_slots == 0
        env.create_state_bank(K)
        for call in (env.create_state_bank, be.bank_create):
            with pytest.raises(_capi.SoftrodError, match=f"bank create: the handle already has a state bank of {K} slots"):
                call(2)
        env.save_states([1], [2])
        filled = [False, False, True, False]
        assert env.state_bank_slots == K and env.state_bank_filled.tolist() == filled
        steps = env._steps.copy()
        save, load = _refused(N, K)
        for cases, calls in ((save, (be.bank_save, env.save_states)), (load, (be.bank_load, env.load_states))):
            for a, b, text in cases:
                for call in calls:
                    with pytest.raises(_capi.SoftrodError) as err:
                        call(a, b)
                    assert str(err.value).endswith(text), (a, b, str(err.value))
                    _assert_rows(_snap(env), range(N), before, range(N), text)
                    assert env.state_bank_filled.tolist() == filled, text
        # what the Python layer cannot express: the raw calls
        one, stream = np.zeros(1, np.int32), be._stream()
        for raw, what in ((be._lib.softrod_bank_save, b"bank save: "), (be._lib.softrod_bank_load, b"bank load: ")):
            for args, text in (((None, one.ctypes.data, 1), b"null envs or slots"),
                               ((one.ctypes.data, None, 1), b"null envs or slots"),
                               ((one.ctypes.data, one.ctypes.data, -1), b"count -1 is outside 0 .. ")):
                assert raw(be._h, *args, stream) == -1
                assert be._lib.softrod_last_error(be._h).startswith(what + text)
            assert raw(be._h, None, None, 0, stream) == 0                      # an empty call is a no-op
        env.save_states([], [])
        env.load_states([], [])
        _assert_rows(_snap(env), range(N), before, range(N), "after refused calls and no-ops")
        assert env.state_bank_filled.tolist() == filled and (env._steps == steps).all()
        # the slot saved at the start still loads what it held
        env.load_states([2], [0])
        _assert_rows(_snap(env), [0], before, [1], "slot 2 after the refusals")
    finally:
        env.close()


def test_device_autoreset_refuses_at_both_levels(hip_lib):
    env = gsa.make_vec("SoftPendulum-v0", N, autoreset="device")
    try:
        env.reset(seed=0)
        before = _state(env)
        for call, args in ((env.create_state_bank, (K,)), (env.save_states, ([0], [1])), (env.load_states, ([1], [0]))):
            with pytest.raises(NotImplementedError, match="autoreset='device'"):
                call(*args)
        with pytest.raises(_capi.SoftrodError, match="bank create: not on a handle with device-side auto-reset"):
            env.backend.bank_create(K)
        assert env.backend.bank_info()[0] == 0
        after = _state(env)
        assert before.keys() == after.keys() and all(_same(before[k], after[k]) for k in before)
    finally:
        env.close()


def test_single_env_returns_to_a_saved_state(hip_lib):
    env = gsa.make("SoftPendulum-v0")
    try:
        env.reset(seed=0)
        rng = np.random.default_rng(1)
        env.step(rng.uniform(-1, 1, env.action_space.shape).astype(np.float32))
        env.create_state_bank(2)
        env.save_state(0)
        actions = [rng.uniform(-1, 1, env.action_space.shape).astype(np.float32) for _ in range(3)]
        first = [env.step(a) for a in actions]
        assert env.counter == 4
        env.load_state(0)
        assert env.counter == 1
        again = [env.step(a) for a in actions]
        for (o1, r1, t1, u1, i1), (o2, r2, t2, u2, i2) in zip(first, again):
            assert _same(o1, o2) and r1 == r2 and t1 == t2 and u1 == u2 and i1 == i2
        assert not _same(first[0][0], first[2][0])
        with pytest.raises(_capi.SoftrodError, match="bank load: slot 1 holds no state"):
            env.load_state(1)
    finally:
        env.close()


@pytest.mark.parametrize("env_id,readout", [("OctoArmPush-v1", "rod_strains"), ("OctoFlat-v0", "rod_energies")])
def test_readouts_of_a_loaded_env_equal_its_source_at_the_save(hip_lib, env_id, readout):
    env = _env((env_id, {}))
    rng = _warm(env)

    def read():
        out = getattr(env, readout)()
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (out if isinstance(out, tuple) else (out,))]

    at_save = read()
    env.save_states(SAVE_ENVS, SAVE_SLOTS)
    for _ in range(2):
        _step(env, _actions(env, rng))
    assert not all(_same(t[LOAD_ENVS], s[LOADED_FROM]) for t, s in zip(read(), at_save))
    env.load_states(LOAD_SLOTS, LOAD_ENVS)
    for t, s in zip(read(), at_save):
        assert _same(t[LOAD_ENVS], s[LOADED_FROM])


def test_example_runs(hip_lib):
    """examples/soft_pendulum_restarts.py at a tiny size, in a fresh child process under its own time limit."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, str(ROOT / "examples" / "soft_pendulum_restarts.py"),
           "--num-envs", "8", "--slots", "4", "--rounds", "2"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "archive after 2 rounds" in r.stdout
