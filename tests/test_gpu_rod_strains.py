"""softrod_rod_strains on the MI355X: every element of every rod of every env kind against the NumPy twin
(diagnostics.rod_strains_host) evaluated on the state read back from the same handle, inside the bands of
tests/rod_strains_ref.py (tests/test_rod_strains.py calibrates them without a GPU); the energy identity against
softrod_rod_energies of the same handle; padding, read-only, repeatability and the single-env shell."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import RodStrains

try:
    from tests import rod_strains_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import rod_strains_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1          # SOFTROD_EINVAL


def _make(case):
    _, env_id, n, kw = case
    env = gsa.make_vec(env_id, n, **ref.make_kwargs(kw))
    if kw.get("material"):
        ref.randomise_material(env)
    return env


def _check(env, tag):
    """Every element of all six fields inside the band; the energy identity at rtol 1e-12.  -> the device's fields."""
    got = RodStrains(*(t.cpu().numpy() for t in env.rod_strains()))
    E = env.rod_energies().cpu().numpy()
    states = ref.rod_states(env)
    rods = _capi.config_rods_per_env(env.cfg)
    n, ne = env.num_envs, int(env.cfg.n_elem)
    assert got.sigma.shape == (n, rods, 3, ne) and got.kappa.shape == (n, rods, 3, ne - 1)
    assert got.dilatation.shape == (n, rods, ne) and got.voronoi_dilatation.shape == (n, rods, ne - 1)
    assert got.internal_force.shape == (n, rods, 3, ne) and got.internal_couple.shape == (n, rods, 3, ne - 1)
    top = {}
    for i, d in enumerate(states):
        e, a = divmod(i, rods)
        dev = RodStrains(*(t[e, a] for t in got))
        assert all(np.isfinite(t).all() for t in dev)
        for f, v in ref.worst(dev, ref.twin(d), d).items():
            top[f] = max(top.get(f, 0.0), v)
        bend, shear = ref.energies_from_strains(dev, d)
        np.testing.assert_allclose([bend, shear], E[e, a, 2:], rtol=1e-12, atol=0, err_msg=f"{tag} rod {i}")
    print(f"{tag}: worst |device - twin| in band units", {f: f"{v:.1e}" for f, v in top.items()})
    for f, v in top.items():
        assert v <= ref.BAND, (tag, f, v)
    return got, states


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_strains_equal_the_host_twin(hip_lib, case):
    """Three instants per case: right after reset(seed=0) (time 0: the state as it stands), after 2 steps of seeded
    actions (the mid-substep configuration), and after a masked reset of every other env (both in one launch)."""
    _, env_id, n, kw = case
    env = _make(case)
    env.reset(seed=ref.SEED)
    _, states = _check(env, case[0] + " reset")
    assert all(d["time"] == 0.0 for d in states)
    for a in ref.actions(env, env_id):
        env.step(a)
    got, states = _check(env, case[0] + " stepped")
    assert all(d["time"] != 0.0 for d in states)
    assert np.abs(got.sigma).max() > 0 and (got.dilatation > 0).all()
    if _capi.config_rods_per_env(env.cfg) > 1:
        assert not np.array_equal(got.sigma[:, 0], got.sigma[:, 1])          # arms are read at their own stride
    mask = np.arange(n) % 2 == 0
    env.reset(seed=ref.SEED + 7, mask=mask)
    _, states = _check(env, case[0] + " masked reset")
    rods = _capi.config_rods_per_env(env.cfg)
    assert [d["time"] == 0.0 for d in states] == [bool(mask[i // rods]) for i in range(n * rods)]
    env.close()


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in ("pendulum-3", "pendulum-64", "flat", "push-126")],
                         ids=lambda c: c[0])
def test_padding_is_written_as_zero_and_calls_repeat(hip_lib, case):
    """The raw C-ABI call into a buffer pre-filled with NaN: no NaN is left, the last column of every Voronoi row is
    exactly 0.0; a second call without a step in between gives the same bytes."""
    _, env_id, n, kw = case
    env = _make(case)
    env.reset(seed=ref.SEED)
    for a in ref.actions(env, env_id, 1):
        env.step(a)
    be = env.backend
    rods, ne = _capi.config_rods_per_env(env.cfg), int(env.cfg.n_elem)
    bufs = []
    for _ in range(2):
        out = torch.full((n, rods, 14, ne), float("nan"), dtype=torch.float64, device=be.device)
        torch.cuda.synchronize()
        assert hip_lib.softrod_rod_strains(be._h, C.c_void_p(out.data_ptr()), be._stream()) == 0
        torch.cuda.synchronize()
        bufs.append(out.cpu().numpy())
    assert not np.isnan(bufs[0]).any()
    for row in (3, 4, 5, 7, 11, 12, 13):
        last = bufs[0][:, :, row, -1]
        assert (last == 0.0).all() and not np.signbit(last).any(), row
    assert bufs[0].tobytes() == bufs[1].tobytes()
    views = env.rod_strains()
    assert views.sigma.data_ptr() == env.rod_strains().sigma.data_ptr()       # one buffer, overwritten
    np.testing.assert_array_equal(views.kappa.cpu().numpy(), bufs[0][:, :, 3:6, :-1])
    env.close()


def test_null_arguments_are_refused(hip_lib):
    env = gsa.make_vec("SoftPendulum-v0", 2)
    be = env.backend
    assert hip_lib.softrod_rod_strains(be._h, None, be._stream()) == EINVAL
    assert hip_lib.softrod_last_error(be._h).decode() == "rod strains: null output buffer"
    assert hip_lib.softrod_rod_strains(None, None, None) == EINVAL
    assert hip_lib.softrod_last_error(None).decode() == "rod strains: null handle"
    env.close()


@pytest.mark.parametrize("env_id,n", [("SoftPendulum-v0", 4), ("OctoFlat-v0", 2), ("OctoArmPush-v1", 4)])
def test_read_out_does_not_touch_the_state(hip_lib, env_id, n):
    """Two handles of the same seed, one reading rod_strains() between steps: observations, rewards and the rod
    snapshot are bit-identical after 2 steps."""
    a_env, b_env = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    a_env.reset(seed=5)
    b_env.reset(seed=5)
    a_env.rod_strains()
    for act in ref.actions(a_env, env_id):
        oa, ra = a_env.step(act)[:2]
        a_env.rod_strains()
        ob, rb = b_env.step(act)[:2]
        assert oa.cpu().numpy().tobytes() == ob.cpu().numpy().tobytes()
        assert ra.cpu().numpy().tobytes() == rb.cpu().numpy().tobytes()
    sa, sb = a_env.backend.rod_snapshot(list(range(n))), b_env.backend.rod_snapshot(list(range(n)))
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    a_env.close()
    b_env.close()


def test_single_env_shell(hip_lib):
    from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

    env = SoftPendulumEnv()
    env.reset(seed=0)
    r = env.rod_strains()
    ne = int(env._vec.cfg.n_elem)
    assert isinstance(r, RodStrains) and all(isinstance(t, np.ndarray) for t in r)
    assert [t.shape for t in r] == [(1, 3, ne), (1, 3, ne - 1), (1, ne), (1, ne - 1), (1, 3, ne), (1, 3, ne - 1)]
    env.close()
