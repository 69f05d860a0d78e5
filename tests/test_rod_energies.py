"""CPU checks of the rod energies (diagnostics.rod_energies_host, the host twin of softrod_rod_energies) and of the
early-termination switch's host side.  The energy FORMS are our recollection of pyelastica 1.0.0 (not on disk);
these tests hold the twin to closed-form answers and to energy conservation of an undamped rod, not to PyElastica."""
import ctypes as C

import numpy as np
import pytest

from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import rod_energies_host, rod_material_host


def _free_cfg(n_elem=20, dt=1e-4):
    cfg = _capi.softpendulum_config(1)
    cfg.n_elem, cfg.dt, cfg.features, cfg.damping_constant = n_elem, dt, 0, 0.0
    return cfg


def _straight(n, rl, direction=(1.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    d3 = np.asarray(direction, float)
    d1 = np.asarray(normal, float)
    d2 = np.cross(d3, d1)
    x = np.outer(d3, np.arange(n + 1) * rl)
    Q = np.repeat(np.stack([d1, d2, d3])[:, :, None], n, axis=2)
    return x, Q


def test_rigid_translation_is_half_m_u2():
    cfg = _free_cfg()
    n, mat = int(cfg.n_elem), rod_material_host(cfg)
    x, Q = _straight(n, mat["rest_length"])
    u = np.array([0.3, -0.2, 0.7])
    v = np.repeat(u[:, None], n + 1, axis=1)
    E = rod_energies_host(x, v, Q, np.zeros((3, n)), 0.0, cfg, mat)
    M = float(cfg.density) * np.pi * float(cfg.base_radius) ** 2 * float(cfg.base_length)
    assert E[0] == pytest.approx(0.5 * M * (u @ u), rel=1e-12)
    assert abs(E[1]) == 0.0 and abs(E[2]) == 0.0 and E[3] < 1e-20


def test_rigid_spin_about_d3():
    cfg = _free_cfg()
    n, mat = int(cfg.n_elem), rod_material_host(cfg)
    x, Q = _straight(n, mat["rest_length"])
    om = 3.0
    w = np.zeros((3, n))
    w[2] = om
    E = rod_energies_host(x, np.zeros((3, n + 1)), Q, w, 0.0, cfg, mat)
    e = (mat["rest_length"] + 1e-14) / mat["rest_length"]
    assert E[1] == pytest.approx(0.5 * mat["J"][2, 0] * om * om * n / e, rel=1e-12)


def test_uniform_stretch_is_half_EA_eps2_L():
    cfg = _free_cfg()
    n, mat = int(cfg.n_elem), rod_material_host(cfg)
    rl = mat["rest_length"]
    eps = 1e-3
    x, Q = _straight(n, rl * (1 + eps))
    E = rod_energies_host(x, np.zeros((3, n + 1)), Q, np.zeros((3, n)), 0.0, cfg, mat)
    l = rl * (1 + eps)
    eps_p = (l + 1e-14) / rl - 1.0                      # eps_length in the dilatation
    EA = float(cfg.youngs_modulus) * np.pi * float(cfg.base_radius) ** 2
    assert E[3] == pytest.approx(0.5 * EA * eps_p ** 2 * float(cfg.base_length), rel=1e-9)
    assert E[2] < 1e-25


def test_circular_arc_bending_closed_form():
    cfg = _free_cfg()
    n, mat = int(cfg.n_elem), rod_material_host(cfg)
    rl = mat["rest_length"]
    phi = 0.05                                          # turn between consecutive elements, about d1
    Q = np.empty((3, 3, n))
    x = np.zeros((3, n + 1))
    for k in range(n):
        a = k * phi
        d1 = np.array([1.0, 0.0, 0.0])
        d3 = np.array([0.0, np.cos(a), np.sin(a)])
        Q[:, :, k] = np.stack([d1, np.cross(d3, d1), d3])
        x[:, k + 1] = x[:, k] + rl * d3
    E = rod_energies_host(x, np.zeros((3, n + 1)), Q, np.zeros((3, n)), 0.0, cfg, mat)
    theta = np.arccos(np.cos(phi) - float(cfg.acos_shift))
    kap = np.sin(phi) * theta / np.sin(theta + float(cfg.eps_sin)) / rl
    B1 = float(cfg.youngs_modulus) * (np.pi * float(cfg.base_radius) ** 2) ** 2 / (4 * np.pi)
    assert E[2] == pytest.approx(0.5 * B1 * kap * kap * rl * (n - 1), rel=1e-9)


def test_material_matches_the_oracle_uniform_and_tapered(oracle_built):
    cfg = _free_cfg()
    n = int(cfg.n_elem)
    radius = np.linspace(0.012, 0.003, n)
    for prof in (None, radius):
        rod = oracle_built.OracleRod(cfg)
        if prof is not None:
            rod.set_radius_profile(prof)
        rod.reset_straight([0, 0, 0], [1, 0, 0], [0, 0, 1])
        mat = rod_material_host(cfg, prof)
        for k in ("mass", "J", "shear", "bend"):
            np.testing.assert_allclose(mat[k], rod.get(k), rtol=1e-13, err_msg=k)


def test_tapered_rod_sums_over_its_table():
    cfg = _free_cfg()
    n = int(cfg.n_elem)
    radius = np.linspace(0.012, 0.001, n)
    mat = rod_material_host(cfg, radius)
    x, Q = _straight(n, mat["rest_length"])
    u = np.array([0.0, 0.5, 0.0])
    v = np.repeat(u[:, None], n + 1, axis=1)
    w = np.zeros((3, n))
    w[0] = 2.0
    E = rod_energies_host(x, v, Q, w, 0.0, cfg, mat)
    M = float(cfg.density) * np.pi * (radius ** 2).sum() * mat["rest_length"]
    assert E[0] == pytest.approx(0.5 * M * 0.25, rel=1e-12)
    J1 = (np.pi * radius ** 2) ** 2 / (4 * np.pi) * float(cfg.density) * mat["rest_length"]
    e = (mat["rest_length"] + 1e-14) / mat["rest_length"]
    assert E[1] == pytest.approx(0.5 * 4.0 * J1.sum() / e, rel=1e-12)


def test_undamped_free_rod_conserves_H_at_the_reference_instant(oracle_built):
    """The reference instant mixes the mid-substep strains with the end-of-step rates, so its H is not the
    integrator's conserved quantity: on this run it wanders by up to 4.0e-4 (the end-of-step state's H by 6e-5,
    tests/test_oracle_physics.py holds that at 2e-4).  The bound says bounded, no secular drift."""
    cfg = _free_cfg(n_elem=20, dt=5e-5)
    rod = oracle_built.OracleRod(cfg)
    rod.reset_straight([0, 0, 0], [1, 0, 0], [0, 0, 1])
    n = int(cfg.n_elem)
    s = np.linspace(0, 1, n + 1)
    v = np.zeros((3, n + 1))
    v[1] = 0.05 * np.sin(np.pi * s)
    v[2] = 0.03 * np.cos(2 * np.pi * s)
    v[0] = 0.01 * (s - 0.5)
    rod.set("v", v)
    mat = rod_material_host(cfg)

    def H():
        return rod_energies_host(rod.get("x"), rod.get("v"), rod.get("Q"), rod.get("w"), 1.0, cfg, mat).sum()

    rod.substeps(0.0, 1)
    h0 = H()
    hs = []
    for _ in range(40):
        rod.substeps(0.0, 250)
        hs.append(H())
    hs = np.array(hs)
    assert h0 > 0
    assert np.abs(hs / h0 - 1).max() < 1e-3
    assert abs(hs[-10:].mean() / hs[:10].mean() - 1) < 3e-4


def test_config_field_replaces_reserved2():
    names = [f[0] for f in _capi.SoftrodConfig._fields_]
    assert "early_termination" in names and "reserved2" not in names
    i = names.index("early_termination")
    assert names[i - 1] == "sucker_index" and names[i + 1] == "sucker_reduction_ratio"
    assert _capi.arm_push_config(2).early_termination == 0
    assert _capi.arm_push_config(2, early_termination=True).early_termination == 1
    assert _capi.arm_pull_weight_config(2, early_termination=True).early_termination == 1
    assert _capi.ABI_VERSION == 17


def test_create_refuses_bad_early_termination_without_a_gpu(hip_lib):
    h = C.c_void_p()
    cfg = _capi.softpendulum_config(4)
    cfg.early_termination = 1                       # not an ArmPush env
    assert hip_lib.softrod_create(C.byref(cfg), 0, C.byref(h)) == -1
    assert b"early_termination" in hip_lib.softrod_last_error(None)
    cfg = _capi.arm_push_config(4)
    cfg.early_termination = 2
    assert hip_lib.softrod_create(C.byref(cfg), 0, C.byref(h)) == -1
    assert b"early_termination" in hip_lib.softrod_last_error(None)


def test_oracle_backend_refuses_early_termination_by_name():
    from gym_softrobot_amd.envs.arm_push import VecArmPushEnv
    from tests.oracle_backend import OracleBackend

    cfg = _capi.arm_push_config(2, early_termination=True)
    with pytest.raises(NotImplementedError, match="OracleBackend"):
        VecArmPushEnv(2, config_early_termination=True, backend=OracleBackend(cfg))
