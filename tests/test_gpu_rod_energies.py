"""softrod_rod_energies on the MI355X: closed forms written into the device state, the host twin
(diagnostics.rod_energies_host) on every registered env after a reset and after a few steps, and energy
conservation of an undamped free rod stepped by the HIP kernel."""
import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import rod_energies_host, rod_material_host

pytestmark = pytest.mark.gpu

_BC = _capi.FEAT_PENDULUM_BC | _capi.FEAT_FIXED_BC | _capi.FEAT_MOVING_BASE_BC


def host_energies(be):
    """(N, R, 4) from the backend's state, through the host twin."""
    cfg = be.cfg
    prof = be._tables.get("radius_profile")
    mat = rod_material_host(cfg, None if prof is None else np.frombuffer(prof, np.float64))
    rk = bool(cfg.features & _capi.FEAT_REST_KAPPA_ACTION)
    n = be.n_envs
    if be.is_octo or be.is_mocto:
        st = be.octo_state_numpy()
        R = int(cfg.n_arm)
        out = np.empty((n, R, 4))
        for e in range(n):
            for a in range(R):
                out[e, a] = rod_energies_host(st["x"][e, a], st["v"][e, a], st["Q"][e, a], st["w"][e, a],
                                              float(st["time"][e]), cfg, mat, st["rest_kappa"][e, a] if rk else None)
        return out
    st = be.state_numpy()
    bc = be.state()["bc_targets"].cpu().numpy()
    out = np.empty((n, 1, 4))
    for e in range(n):
        kw = {}
        if cfg.features & _BC:
            kw = dict(fixed_pos=bc[:3, e], fixed_dir=bc[3:, e].reshape(3, 3), base_xy=st["control"][e, :2])
        out[e, 0] = rod_energies_host(st["x"][e], st["v"][e], st["Q"][e], st["w"][e], float(st["time"][e]), cfg, mat,
                                      st["rest_kappa"][e] if rk else None, **kw)
    return out


def _close(dev, host, rel):
    # absolute floor: 1e-12 of the batch's largest energy, and 1e-20 J for the rounding-level residues of a rod
    # at rest (its shear energy of eps_length alone is ~1e-26 J)
    np.testing.assert_allclose(dev, host, rtol=rel, atol=max(1e-20, 1e-12 * np.abs(host).max()))


CASES = [("SoftPendulum-v0", {}), ("SoftPendulum3D-v0", {}), ("OctoArmSingle-v0", {}),
         ("OctoArmSingle-v0", dict(n_elems=100)), ("OctoArmSingle-v0", dict(radius_profile="taper")),
         ("SoftArmTracking-v0", {}), ("OctoFlat-v0", {}), ("OctoFlatLite-v0", {}), ("OctoArmPush-v0", {}),
         ("OctoArmPush-v1", {}), ("OctoArmPullWeight-v0", {}), ("OctoCrawl-v0", {}), ("OctoArmTwo-v0", {}),
         ("OctoReach-v0", {})]


@pytest.mark.parametrize("env_id,kw", CASES, ids=[c[0] + ("-" + "-".join(map(str, c[1].values())) if c[1] else "")
                                                   for c in CASES])
def test_energies_equal_the_host_twin_on_every_env(env_id, kw):
    kw = dict(kw)
    if kw.get("radius_profile") == "taper":
        edge = np.linspace(0.012, 0.001, 51)
        kw["radius_profile"] = (edge[:-1] + edge[1:]) / 2
    n = 6
    env = gsa.make_vec(env_id, n, **kw)
    env.reset(seed=3)
    E0 = env.rod_energies().cpu().numpy()
    assert E0.shape == (n, _capi.config_rods_per_env(env.cfg), 4)
    _close(E0, host_energies(env.backend), 1e-9)                       # right after a reset: the state itself
    rng = np.random.default_rng(0)
    for _ in range(3):
        if getattr(env, "mode", None) == 0 and env_id.startswith("OctoArmPush"):
            a = rng.integers(0, 2, (n, 1)).astype(np.float32)
        else:
            lo, hi = env.action_space.low, env.action_space.high
            a = rng.uniform(np.maximum(lo, -1.0), np.minimum(hi, 1.0)).astype(np.float32)
        env.step(a)
    E = env.rod_energies().cpu().numpy()
    H = host_energies(env.backend)
    assert np.isfinite(E).all() and (E[..., 0] > 0).any()
    _close(E, H, 1e-9)
    env.close()


def _free_backend(n_elem=20, dt=5e-5, n_envs=2):
    from gym_softrobot_amd.backend import HipRodBackend

    cfg = _capi.softpendulum_config(n_envs)
    cfg.n_elem, cfg.dt, cfg.features, cfg.damping_constant = n_elem, dt, 0, 0.0
    cfg.env_kind = _capi.ENV_NONE
    be = HipRodBackend(cfg)
    z = np.zeros((n_envs, 3))
    be.reset_straight(z, np.tile([1.0, 0, 0], (n_envs, 1)), np.tile([0, 0, 1.0], (n_envs, 1)))
    return be


def test_closed_forms_in_the_device_state():
    be = _free_backend()
    n, N = int(be.cfg.n_elem), be.n_envs
    mat = rod_material_host(be.cfg)
    st = be.state()
    u = torch.tensor([0.3, -0.2, 0.7], dtype=torch.float64, device=be.device)
    st["velocity"][:, 0, : n + 1] = u[:, None]                        # env 0: rigid translation
    st["omega"][2, 1, :n] = 3.0                                      # env 1: spin about d3
    st["position"][:, 1, : n + 1] *= 1.001                           # and a uniform stretch
    st["time"].zero_()
    torch.cuda.synchronize()
    E = be.rod_energies().cpu().numpy()
    M = float(be.cfg.density) * np.pi * float(be.cfg.base_radius) ** 2 * float(be.cfg.base_length)
    rl = mat["rest_length"]
    assert E[0, 0, 0] == pytest.approx(0.5 * M * float(u @ u), rel=1e-12)
    e = (rl * 1.001 + 1e-14) / rl
    assert E[1, 0, 1] == pytest.approx(0.5 * mat["J"][2, 0] * 9.0 * n / e, rel=1e-12)
    EA = float(be.cfg.youngs_modulus) * np.pi * float(be.cfg.base_radius) ** 2
    assert E[1, 0, 3] == pytest.approx(0.5 * EA * (e - 1.0) ** 2 * float(be.cfg.base_length), rel=1e-9)
    assert abs(E[0, 0, 1]) < 1e-30 and E[0, 0, 2] < 1e-20 and E[1, 0, 0] < 1e-30
    be.close()


def _put_rod(st, env, x, Q, n):
    dev = st["position"].device
    st["position"][:, env, : n + 1] = torch.from_numpy(x).to(dev)
    st["director"][:, env, :n] = torch.from_numpy(Q.reshape(9, n)).to(dev)


def test_closed_forms_arc_taper_and_the_mid_substep_path():
    be = _free_backend(n_envs=3)
    n, cfg = int(be.cfg.n_elem), be.cfg
    mat = rod_material_host(cfg)
    rl, dt = mat["rest_length"], float(cfg.dt)
    st = be.state()
    # env 0: a circular arc turning phi about d1 per element (acos_shift, eps_sin), at a reset (time 0)
    phi = 0.05
    Q = np.empty((3, 3, n))
    x = np.zeros((3, n + 1))
    for k in range(n):
        d1, d3 = np.array([1.0, 0.0, 0.0]), np.array([0.0, np.cos(k * phi), np.sin(k * phi)])
        Q[:, :, k] = np.stack([d1, np.cross(d3, d1), d3])
        x[:, k + 1] = x[:, k] + rl * d3
    _put_rod(st, 0, x, Q, n)
    # env 1: straight, spun about d3 at a rate growing along the rod, AFTER a step (time != 0): the mid-substep
    # directors R(dt/2 w)^T Q are twisted by c dt/2 per element -> a closed-form kappa_3
    c = 0.02 / dt
    st["omega"][2, 1, :n] = torch.arange(n, dtype=torch.float64, device=be.device) * c
    # env 2: a rigid translation after a step: the back half step moves the rod rigidly, nothing but 1/2 M u^2
    u = torch.tensor([0.3, -0.2, 0.7], dtype=torch.float64, device=be.device)
    st["velocity"][:, 2, : n + 1] = u[:, None]
    st["time"][:] = torch.tensor([0.0, 0.25, 0.25], dtype=torch.float64, device=be.device)
    torch.cuda.synchronize()
    E = be.rod_energies().cpu().numpy()[:, 0]
    theta = np.arccos(np.cos(phi) - float(cfg.acos_shift))
    kap = np.sin(phi) * theta / np.sin(theta + float(cfg.eps_sin)) / rl
    B = rod_material_host(cfg)["bend"]
    assert E[0, 2] == pytest.approx(0.5 * B[0, 0] * kap * kap * rl * (n - 1), rel=1e-9)
    tw = c * 0.5 * dt
    theta = np.arccos(np.cos(tw) - float(cfg.acos_shift))
    kap3 = np.sin(tw) * theta / np.sin(theta + float(cfg.eps_sin)) / rl
    assert E[1, 2] == pytest.approx(0.5 * B[2, 0] * kap3 * kap3 * rl * (n - 1), rel=1e-9)
    e = (rl + 1e-14) / rl
    w2 = (np.arange(n) * c) ** 2
    assert E[1, 1] == pytest.approx(0.5 * mat["J"][2, 0] * w2.sum() / e, rel=1e-12)
    M = float(cfg.density) * np.pi * float(cfg.base_radius) ** 2 * float(cfg.base_length)
    assert E[2, 0] == pytest.approx(0.5 * M * float(u @ u), rel=1e-12)
    assert E[2, 1] == 0.0 and E[2, 2] < 1e-20 and E[2, 3] < 1e-20
    be.close()

    # a tapered rod: the sums run over the per-slot material table
    from gym_softrobot_amd.backend import HipRodBackend

    radius = np.linspace(0.012, 0.001, n)
    tb = HipRodBackend(cfg.copy())
    tb.set_radius_profile(radius)
    tb.reset_straight(np.zeros((3, 3)), np.tile([1.0, 0, 0], (3, 1)), np.tile([0, 0, 1.0], (3, 1)))
    ts = tb.state()
    ts["velocity"][1, 0, : n + 1] = 0.5
    ts["omega"][0, 0, :n] = 2.0
    torch.cuda.synchronize()
    E = tb.rod_energies().cpu().numpy()[0, 0]
    Mt = float(cfg.density) * np.pi * (radius ** 2).sum() * rl
    J1 = (np.pi * radius ** 2) ** 2 / (4 * np.pi) * float(cfg.density) * rl
    assert E[0] == pytest.approx(0.5 * Mt * 0.25, rel=1e-12)
    assert E[1] == pytest.approx(0.5 * 4.0 * J1.sum() / e, rel=1e-12)
    tb.close()


def test_undamped_free_rod_conserves_H_on_the_gpu():
    be = _free_backend(n_envs=1)
    n = int(be.cfg.n_elem)
    s = np.linspace(0, 1, n + 1)
    v = np.zeros((3, n + 1))
    v[1] = 0.05 * np.sin(np.pi * s)
    v[2] = 0.03 * np.cos(2 * np.pi * s)
    v[0] = 0.01 * (s - 0.5)
    be.state()["velocity"][:, 0, : n + 1] = torch.from_numpy(v).to(be.device)
    be.substeps(None, 1)
    h0 = be.rod_energies().sum().item()
    hs = []
    for _ in range(40):
        be.substeps(None, 250)
        hs.append(be.rod_energies().sum().item())
    _close(be.rod_energies().cpu().numpy(), host_energies(be), 1e-9)
    hs = np.array(hs)
    assert h0 > 0
    assert np.abs(hs / h0 - 1).max() < 1e-3                         # (tests/test_rod_energies.py: the same bound)
    assert abs(hs[-10:].mean() / hs[:10].mean() - 1) < 3e-4
    be.close()


def test_arm_push_energies_against_the_oracle():
    """OctoArmPush-v1 on the device against the CPU oracle's state, through the host twin, inside the 1e-5 band of
    the other OctoArmPush parity tests."""
    from oracle import oracle_c

    oracle_c.build()
    n = 4
    env = gsa.make_vec("OctoArmPush-v1", n)
    env.reset()
    acts = np.random.default_rng(4).uniform(0.0, 1.0, (3, n, 2)).astype(np.float32)
    cfg1 = _capi.arm_push_config(1, mode="continuous")
    radii = _capi.arm_push_radii(40)
    mat = rod_material_host(cfg1, radii)
    orcs = []
    for i in range(n):
        o = oracle_c.OracleRod(cfg1)
        o.set_radius_profile(radii)
        o.set_muscle_layers(*_capi.es_muscle_layers(radii, 0.012))
        o.reset_push()
        orcs.append(o)
    for a in acts:
        env.step(a)
        for i, o in enumerate(orcs):
            o.env_step_push(a[i])
    E = env.rod_energies().cpu().numpy()[:, 0]
    want = np.stack([rod_energies_host(o.get("x"), o.get("v"), o.get("Q"), o.get("w"), float(o.time), cfg1, mat)
                     for o in orcs])
    assert (want.sum(axis=1) > 1e-6).all()
    np.testing.assert_allclose(E, want, rtol=1e-5, atol=1e-5 * want.max())
    env.close()
