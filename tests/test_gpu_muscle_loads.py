"""softrod_muscle_loads on the MI355X: every element of every rod of every COOMM muscle env against the NumPy twin
(diagnostics.muscle_loads_host) evaluated on the state read back from the same handle, inside the band of
tests/muscle_loads_ref.py (tests/test_muscle_loads.py calibrates it without a GPU and holds the twin to the oracle's
transcription of the law); padding, repeatability, refusals, read-only, consistency with softrod_rod_strains of the same
handle, and the single-env shell."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import MuscleLoads

try:
    from tests import muscle_loads_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import muscle_loads_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1          # SOFTROD_EINVAL


def _make(case):
    _, env_id, n, kw = case
    return gsa.make_vec(env_id, n, **kw)


def _check(env, tag):
    """Every element of all six fields inside the band.  -> the device's fields, the rods' states."""
    got = MuscleLoads(*(t.cpu().numpy() for t in env.muscle_loads()))
    states = ref.rod_states(env)
    rods = _capi.config_rods_per_env(env.cfg)
    n, ne = env.num_envs, int(env.cfg.n_elem)
    assert got.layer_force.shape == (n, rods, 4, ne) and got.layer_length.shape == (n, rods, 4, ne)
    assert got.internal_force.shape == (n, rods, 3, ne) and got.internal_couple.shape == (n, rods, 3, ne - 1)
    assert got.external_force.shape == (n, rods, 3, ne + 1) and got.external_couple.shape == (n, rods, 3, ne)
    top = {}
    for i, d in enumerate(states):
        e, a = divmod(i, rods)
        dev = MuscleLoads(*(t[e, a] for t in got))
        assert all(np.isfinite(t).all() for t in dev)
        for f, v in ref.worst(dev, ref.twin(d), d).items():
            top[f] = max(top.get(f, 0.0), v)
    print(f"{tag}: worst |device - twin| in band units", {f: f"{v:.1e}" for f, v in top.items()})
    for f, v in top.items():
        assert v <= ref.BAND, (tag, f, v)
    return got, states


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_muscle_loads_equal_the_host_twin(hip_lib, case):
    """Three instants per case: right after reset(seed=0) with seeded per-element activations written into the resident
    rows (time 0: the state as it stands), after 2 steps of seeded actions (the mid-substep configuration), and after a
    masked reset of every other env (both in one launch)."""
    _, env_id, n, kw = case
    env = _make(case)
    env.reset(seed=ref.SEED)
    ref.write_activations(env, ref.seeded_activations(env))
    got, states = _check(env, case[0] + " reset")
    assert all(d["time"] == 0.0 for d in states)
    assert np.abs(got.layer_force).max() > 0
    for a in ref.actions(env, env_id):
        env.step(a)
    got, states = _check(env, case[0] + " stepped")
    assert all(d["time"] != 0.0 for d in states)
    assert np.abs(got.layer_force).max() > 0                                 # a layer is driven
    nm = int(env.cfg.n_muscles)
    assert (got.layer_length[:, :, :nm] > 0).all() and not got.layer_length[:, :, nm:].any()
    if _capi.config_rods_per_env(env.cfg) > 1:
        assert not np.array_equal(got.layer_length[:, 0], got.layer_length[:, 1])      # arms are read at their own stride
        assert not np.array_equal(got.external_force[:, 0], got.external_force[:, 1])
    mask = np.arange(n) % 2 == 0
    env.reset(seed=ref.SEED + 7, mask=mask)
    _, states = _check(env, case[0] + " masked reset")
    rods = _capi.config_rods_per_env(env.cfg)
    assert [d["time"] == 0.0 for d in states] == [bool(mask[i // rods]) for i in range(n * rods)]
    env.close()


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in ("push-3", "push-64", "crawl", "pull")],
                         ids=lambda c: c[0])
def test_padding_is_written_as_zero_and_calls_repeat(hip_lib, case):
    """The raw C-ABI call into a buffer pre-filled with NaN: no NaN is left; every column past a row's range and every
    row of a layer >= n_muscles is exactly +0.0; a second call without a step in between gives the same bytes."""
    _, env_id, n, kw = case
    env = _make(case)
    env.reset(seed=ref.SEED)
    for a in ref.actions(env, env_id, 1):
        env.step(a)
    be = env.backend
    rods, ne, nm = _capi.config_rods_per_env(env.cfg), int(env.cfg.n_elem), int(env.cfg.n_muscles)
    bufs = []
    for _ in range(2):
        out = torch.full((n, rods, 20, ne + 1), float("nan"), dtype=torch.float64, device=be.device)
        torch.cuda.synchronize()
        assert hip_lib.softrod_muscle_loads(be._h, C.c_void_p(out.data_ptr()), be._stream()) == 0
        torch.cuda.synchronize()
        bufs.append(out.cpu().numpy())
    b = bufs[0]
    assert not np.isnan(b).any()

    def plus_zero(a, what):
        assert (a == 0.0).all() and not np.signbit(a).any(), what

    for row in range(20):
        if not 14 <= row <= 16:                                      # every row but the nodal one ends at n_elem
            plus_zero(b[:, :, row, ne:], row)
    for row in (11, 12, 13):                                         # the Voronoi rows end at n_elem - 1
        plus_zero(b[:, :, row, ne - 1:], row)
    assert nm < 4
    for m in range(nm, 4):
        plus_zero(b[:, :, m], m)
        plus_zero(b[:, :, 4 + m], 4 + m)
    assert bufs[0].tobytes() == bufs[1].tobytes()
    views = env.muscle_loads()
    assert views.layer_force.data_ptr() == env.muscle_loads().layer_force.data_ptr()       # one buffer, overwritten
    np.testing.assert_array_equal(views.internal_couple.cpu().numpy(), b[:, :, 11:14, :-2])
    env.close()


def test_refusals(hip_lib):
    from gym_softrobot_amd.backend import HipRodBackend

    env = gsa.make_vec("SoftPendulum-v0", 2)
    be = env.backend
    out = torch.zeros((2, 1, 20, int(env.cfg.n_elem) + 1), dtype=torch.float64, device=be.device)
    assert hip_lib.softrod_muscle_loads(be._h, C.c_void_p(out.data_ptr()), be._stream()) == EINVAL
    assert hip_lib.softrod_last_error(be._h).decode() == "muscle loads: this handle has no COOMM muscles"
    assert _capi.muscle_loads_refusal(env.cfg) == "muscle loads: this handle has no COOMM muscles"
    with pytest.raises(ValueError) as e:
        env.muscle_loads()
    assert str(e.value) == "muscle loads: this handle has no COOMM muscles"
    assert hip_lib.softrod_muscle_loads(be._h, None, be._stream()) == EINVAL
    assert hip_lib.softrod_last_error(be._h).decode() == "muscle loads: null output buffer"
    assert hip_lib.softrod_muscle_loads(None, None, None) == EINVAL
    assert hip_lib.softrod_last_error(None).decode() == "muscle loads: null handle"
    env.close()
    bare = HipRodBackend(_capi.arm_push_config(2, mode="continuous"))          # no softrod_set_muscle_layers yet
    out = torch.zeros((2, 1, 20, 41), dtype=torch.float64, device=bare.device)
    assert hip_lib.softrod_muscle_loads(bare._h, C.c_void_p(out.data_ptr()), bare._stream()) == EINVAL
    assert hip_lib.softrod_last_error(bare._h).decode() == "muscle loads: softrod_set_muscle_layers has not been called"
    assert _capi.muscle_loads_refusal(bare.cfg) is None
    bare.close()


@pytest.mark.parametrize("env_id,n", [("OctoArmPush-v1", 4), ("OctoCrawl-v0", 2)])
def test_read_out_does_not_touch_the_state(hip_lib, env_id, n):
    """Two handles of the same seed, one reading muscle_loads() between steps: observations, rewards and the rod
    snapshot are bit-identical after 2 steps."""
    a_env, b_env = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    a_env.reset(seed=5)
    b_env.reset(seed=5)
    a_env.muscle_loads()
    for act in ref.actions(a_env, env_id):
        oa, ra = a_env.step(act)[:2]
        a_env.muscle_loads()
        ob, rb = b_env.step(act)[:2]
        assert oa.cpu().numpy().tobytes() == ob.cpu().numpy().tobytes()
        assert ra.cpu().numpy().tobytes() == rb.cpu().numpy().tobytes()
    sa, sb = a_env.backend.rod_snapshot(list(range(n))), b_env.backend.rod_snapshot(list(range(n)))
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    a_env.close()
    b_env.close()


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in ("push", "push-126", "crawl")], ids=lambda c: c[0])
def test_layer_rows_follow_rod_strains_of_the_same_handle(hip_lib, case):
    """nu_m = sigma + (0, 0, 1) + kappa_e x x_m and F_m of every layer rebuilt on the host from rod_strains()' sigma,
    kappa and dilatation of the same handle equal rows 0-7 within the band: the two kernels read one instant."""
    _, env_id, n, kw = case
    env = _make(case)
    env.reset(seed=ref.SEED)
    for a in ref.actions(env, env_id):
        env.step(a)
    s = [t.cpu().numpy() for t in env.rod_strains()]
    got = MuscleLoads(*(t.cpu().numpy() for t in env.muscle_loads()))
    cfg, rods = env.cfg, _capi.config_rods_per_env(env.cfg)
    assert int(cfg.muscle_position_current_radius) == 1 and int(cfg.muscle_tm_length_law) == 0
    top = {"layer_force": 0.0, "layer_length": 0.0}
    for i, d in enumerate(ref.rod_states(env)):
        e, a = divmod(i, rods)
        sigma, kappa, dil = s[0][e, a], s[1][e, a], s[2][e, a]
        ratio, strength = d["layers"]
        shear = sigma.copy()
        shear[2] += 1.0
        kappa_e = np.zeros_like(sigma)
        kappa_e[:, :-1] += 0.5 * kappa
        kappa_e[:, 1:] += 0.5 * kappa
        rad = d["radius"] * np.sqrt(1.0 / dil)                              # r0 sqrt(l_rest / l)
        A = ref.strength_sum(d)
        for m in range(int(cfg.n_muscles)):
            nu = shear + np.cross(kappa_e, rad * ratio[m], axis=0)
            norm = np.sqrt((nu * nu).sum(0))
            length = 1.0 / np.sqrt(norm) if int(cfg.muscle_kind[m]) == _capi.MUSCLE_TRANSVERSE else norm
            fl = np.zeros_like(length)
            for p in range(int(cfg.muscle_fl_degree), -1, -1):
                fl = fl * length + float(cfg.muscle_fl_coef[p])
            F = d["activation"][m] * strength[m] * np.maximum(fl, 0.0)
            top["layer_length"] = max(top["layer_length"], float(np.abs(got.layer_length[e, a, m] - length).max()))
            top["layer_force"] = max(top["layer_force"], float((np.abs(got.layer_force[e, a, m] - F) / A).max()))
    print(f"{case[0]}: worst |muscle_loads - rebuilt from rod_strains| in band units", {k: f"{v:.1e}" for k, v in top.items()})
    assert np.abs(got.layer_force).max() > 0
    for k, v in top.items():
        assert v <= ref.BAND, (k, v)
    env.close()


def test_single_env_shell(hip_lib):
    from gym_softrobot_amd.envs.arm_push import ArmPushEnv

    env = ArmPushEnv()
    env.reset(seed=0)
    env.step(0)
    r = env.muscle_loads()
    ne = int(env._vec.cfg.n_elem)
    assert isinstance(r, MuscleLoads) and all(isinstance(t, np.ndarray) for t in r)
    assert [t.shape for t in r] == [(1, 4, ne), (1, 4, ne), (1, 3, ne), (1, 3, ne - 1), (1, 3, ne + 1), (1, 3, ne)]
    env.close()
