"""OctoArmPush-v0 / -v1 with `n_elems` of 64..126 on the MI355X: the two-slot-per-lane ArmPush instantiations
(softrod_step_fast_kernel<SOFTROD_FEATURES_ARM_PUSH, SOFTROD_ENV_ARM_PUSH, 2, TAPER>, one wave per rod) against the
CPU oracle's env_step_push, which is generic in n_elem.  PARITY UNPINNED underneath like every muscle env (the COOMM
law is restated): what is held is HIP == this repo's oracle at rtol 1e-5.

THE REGIME.  Measured on the oracle: the discrete scripts of test_gpu_muscles.py keep the arm at max |v| 0.4-9.4 at 64
and 100 elements; at 126, scripts 2 and 4 drive it to |v| ~ 300 with the tip at x ~ -0.95 in the oracle itself, and
continuous actions with transverse activations up to 1.0 do the same at 100 and 126 elements.  The scripts below stay
inside: discrete mode at 64 and 100 only, continuous activations in [0, 0.5] (max |v| <= 2.8 at every length)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-5
CUTOFF = 1e-7
DISCRETE = [[0, 0, 1, 1], [0, 1, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1], [0, 1, 1, 0]]
LOCATIONS = [0.0, 1.0, 0.999, 0.5, 0.0125, 0.3]          # the clip at both ends of the index range


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch


def _continuous(rng, N, t):
    a = rng.uniform(0.0, 1.0, (N, 2)).astype(np.float32)
    a[:, 1] *= 0.5
    a[0, 0] = LOCATIONS[t % len(LOCATIONS)]
    return a


def _oracle_rods(oracle_c, n_rods, n, mode):
    from gym_softrobot_amd import _capi

    cfg1 = _capi.arm_push_config(1, mode=mode, n_elems=n)
    radii = _capi.arm_push_radii(n)
    layers = _capi.es_muscle_layers(radii, 0.012)
    rods = []
    for _ in range(n_rods):
        r = oracle_c.OracleRod(cfg1)
        r.set_radius_profile(radii)
        r.set_muscle_layers(*layers)
        r.reset_push()
        rods.append(r)
    return cfg1, radii, rods


@pytest.mark.parametrize("n,mode", [(64, "discrete"), (64, "continuous"), (100, "discrete"), (100, "continuous"),
                                    (126, "continuous")])
def test_long_arm_matches_oracle(torch_gpu, hip_lib, oracle_built, n, mode):
    """Six env.steps of 500 substeps on 4 envs: obs, reward, flags, time, then x v w Q of every env and the sucker
    index the actions moved."""
    import gym_softrobot_amd as gsa
    from tests.oracle_backend import OracleBackend

    N = 4
    env = gsa.make_vec("OctoArmPush-v0", N, mode=mode, n_elems=n)
    assert "ArmPush,epl=2,taper" in env.backend.kernel_tier()
    assert env.obs_dim == 2 * (n + 1) + 2
    ref = gsa.make_vec("OctoArmPush-v0", N, mode=mode, n_elems=n,
                       backend=OracleBackend(gsa._capi.arm_push_config(N, mode=mode, n_elems=n)), numpy_output=True)
    o, _ = env.reset(seed=0)
    o2, _ = ref.reset(seed=0)
    np.testing.assert_array_equal(o.cpu().numpy(), o2)
    rng = np.random.default_rng(3)
    for t in range(6):
        a = np.array(DISCRETE[t], np.float32).reshape(N, 1) if mode == "discrete" else _continuous(rng, N, t)
        o, r, te, tr, info = env.step(a)
        o2, r2, te2, tr2, info2 = ref.step(a)
        torch_gpu.cuda.synchronize()
        np.testing.assert_allclose(o.cpu().numpy(), o2, rtol=RTOL, atol=2e-7, err_msg=f"obs step {t}")
        np.testing.assert_allclose(r.cpu().numpy(), r2, rtol=RTOL, atol=1e-9, err_msg=f"reward step {t}")
        np.testing.assert_array_equal(te.cpu().numpy(), te2)
        np.testing.assert_array_equal(tr.cpu().numpy(), tr2)
        np.testing.assert_array_equal(np.asarray(info["time"]), np.asarray(info2["time"]))
    assert not te.cpu().numpy().any() and max(np.abs(q.get("v")).max() for q in ref.backend.rods) < 10.0
    st = env.backend.state_numpy()
    for i, q in enumerate(ref.backend.rods):
        for name in ("x", "v", "w", "Q"):
            np.testing.assert_allclose(st[name][i], q.get(name), rtol=RTOL, atol=1e-9, err_msg=f"{name} env {i}")
    idx = env.backend.state()["sucker_index"][0].cpu().numpy()
    np.testing.assert_array_equal(idx, [int(q.get("sucker_index")[0]) for q in ref.backend.rods])
    assert np.abs(st["x"][:, 0, -1] - 0.2).max() > 5e-3          # the arm really extended / moved
    env.close()
    ref.close()


def test_long_arm_every_env_of_a_thousand(torch_gpu, hip_lib, oracle_built):
    """configs[2]'s arm with muscles: 1024 OctoArmPush-v1 envs x 100 elements, one env.step under the bench's own
    actions, every env against the oracle's ArmPush env (host threads over independent oracle rods)."""
    import gym_softrobot_amd as gsa

    N, n = 1024, 100
    env = gsa.make_vec("OctoArmPush-v1", N, n_elems=n)
    env.reset(seed=0)
    _, _, rods = _oracle_rods(oracle_built, N, n, "continuous")
    acts = np.random.default_rng(1).uniform(0.0, 1.0, (N, 2)).astype(np.float32)
    o, r_, te, tr, _ = env.step(acts)
    with ThreadPoolExecutor(max_workers=8) as pool:          # ctypes drops the GIL inside the oracle
        ref = list(pool.map(lambda i: rods[i].env_step_push(acts[i]), range(N)))
    torch_gpu.cuda.synchronize()
    o2 = np.stack([x[0] for x in ref])
    r2 = np.array([x[1] for x in ref])
    np.testing.assert_allclose(o.cpu().numpy(), o2, rtol=RTOL, atol=2e-7)
    np.testing.assert_allclose(r_.cpu().numpy(), r2, rtol=RTOL, atol=1e-9)
    np.testing.assert_array_equal(te.cpu().numpy(), np.array([x[2] for x in ref]))
    np.testing.assert_array_equal(tr.cpu().numpy(), np.array([x[3] for x in ref]))
    env.close()


def test_long_arm_energies_and_early_termination(torch_gpu, hip_lib):
    """rod_energies() of the two-slot tapered arm equals the host twin evaluated on the device's own state (the
    material table is 128 slots wide there), at reset and after a step.  With config_early_termination, rods put at
    rest through the state view end their episode (H < 1e-7: terminated = truncated, reward -10); moving rods do not."""
    import gym_softrobot_amd as gsa
    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.diagnostics import rod_energies_host, rod_material_host

    N, n = 4, 100
    cfg1 = _capi.arm_push_config(1, mode="continuous", n_elems=n)
    mat = rod_material_host(cfg1, _capi.arm_push_radii(n))

    def host_energies(env):
        s = env.backend.state_numpy()
        return np.stack([rod_energies_host(s["x"][i], s["v"][i], s["Q"][i], s["w"][i], float(s["time"][i]), cfg1, mat)
                         for i in range(N)])

    env = gsa.make_vec("OctoArmPush-v1", N, n_elems=n, config_early_termination=True)
    assert "ArmPush,epl=2,taper" in env.backend.kernel_tier()
    env.reset()
    np.testing.assert_allclose(env.rod_energies().cpu().numpy()[:, 0], host_energies(env), rtol=1e-8, atol=1e-20)
    st = env.backend.state()
    rest = {k: st[k].clone() for k in ("position", "director")}
    a = np.array([[0.3, 0.4], [0.8, 0.5], [0.1, 0.2], [0.6, 0.45]], np.float32)
    _, rew, term, trunc, _ = env.step(a)
    E = env.rod_energies().cpu().numpy()[:, 0]
    want = host_energies(env)
    np.testing.assert_allclose(E, want, rtol=1e-8, atol=1e-20)
    assert (want.sum(axis=1) > 100 * CUTOFF).all()
    assert not term.cpu().numpy().any() and (rew.cpu().numpy() == -10.0).all()
    # envs 0 and 2 back to the straight rest state, their muscles off; envs 1 and 3 keep moving
    for k in ("position", "director"):
        st[k][:, [0, 2]] = rest[k][:, [0, 2]]
    for k in ("velocity", "omega"):
        st[k][:, [0, 2]] = 0.0
    a[[0, 2], 1] = 0.0
    _, rew, term, trunc, info = env.step(a)
    H = host_energies(env).sum(axis=1)
    np.testing.assert_allclose(env.rod_energies().cpu().numpy()[:, 0], host_energies(env), rtol=1e-8, atol=1e-20)
    np.testing.assert_array_equal(term.cpu().numpy().astype(bool), H < CUTOFF)
    np.testing.assert_array_equal(term.cpu().numpy().astype(bool), [True, False, True, False])
    np.testing.assert_array_equal(trunc.cpu().numpy().astype(bool), [True, False, True, False])
    assert (rew.cpu().numpy() == -10.0).all()
    assert not np.asarray(info["TimeLimit.truncated"]).any()
    env.close()


@pytest.mark.parametrize("early_termination", [False, True], ids=["plain", "early-termination"])
def test_long_arm_device_autoreset_matches_host_autoreset(torch_gpu, hip_lib, early_termination):
    import gym_softrobot_amd as gsa

    N, n = 16, 100
    kw = dict(n_elems=n, final_time=0.06, config_early_termination=early_termination)
    host = gsa.make_vec("OctoArmPush-v1", N, autoreset=True, **kw)
    dev = gsa.make_vec("OctoArmPush-v1", N, autoreset="device", **kw)
    host.reset(seed=1)
    dev.reset(seed=1)
    rng = np.random.default_rng(2)
    saw_tl = False
    for k in range(12):
        a = _continuous(rng, N, k)
        a[: N // 4, 1] = 0.0
        oh, rh, th, trh, ih = host.step(a)
        od, rd, td, trd, idd = dev.step(a)
        np.testing.assert_array_equal(rh.cpu().numpy(), rd.cpu().numpy())
        np.testing.assert_array_equal(th.cpu().numpy(), td.cpu().numpy())
        np.testing.assert_array_equal(trh.cpu().numpy(), trd.cpu().numpy())
        np.testing.assert_array_equal(oh.cpu().numpy(), od.cpu().numpy())
        tl_h = np.asarray(ih["TimeLimit.truncated"])
        tl_d = idd["TimeLimit.truncated"]
        tl_d = tl_d.cpu().numpy() if hasattr(tl_d, "cpu") else np.asarray(tl_d)
        np.testing.assert_array_equal(tl_d, tl_h)
        saw_tl |= bool(tl_h.any())
        assert not np.isnan(oh.cpu().numpy()).any()
    assert saw_tl
    host.close()
    dev.close()


def test_long_arm_refuses_libm(torch_gpu, hip_lib):
    import gym_softrobot_amd as gsa
    from gym_softrobot_amd import _capi

    with pytest.raises(_capi.SoftrodError, match="SOFTROD_MATH_FAST"):
        gsa.make_vec("OctoArmPush-v1", 2, n_elems=100, math_mode=_capi.MATH_LIBM)


def test_default_length_keeps_its_kernel(torch_gpu, hip_lib):
    import gym_softrobot_amd as gsa

    env = gsa.make_vec("OctoArmPush-v1", 2)
    assert env.n_elem == 40 and "ArmPush,epl=1,taper" in env.backend.kernel_tier()
    env.close()
