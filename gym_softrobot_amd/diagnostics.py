"""Diagnostic taps: the data the reference's callbacks collect, taken
from the resident state after each env.step instead of from inside PyElastica's stepper.

`RodCallBack` (gym_softrobot/utils/custom_elastica/callback_func.py:23-41) fires when
`current_step % step_skip == 0`, i.e. once per env.step, and appends copies of the rod's
time, radius, dilatation, voronoi_dilatation, position, director, velocity, omega, sigma and
kappa to `callback_params` (soft_pendulum.py:117-126 wires it to `rod_parameters_dict`).
`RodRecorder.record()` appends the same fields for the chosen envs of a batch.

WHICH INSTANT.  `system.sigma / kappa / dilatation / voronoi_dilatation / radius` are PyElastica's
cached arrays: they were last written by the force evaluation of the final substep, i.e. at the
MID-substep configuration (after the first kinematic half step and constrain_values), not at the
end-of-step state that `position_collection` etc. hold.  The kernels keep the
state, not those caches, so the mid-substep configuration is rebuilt here exactly: the closing
half step of PositionVerlet is x_end = x_mid + (dt/2) v_end, Q_end = R((dt/2) omega_end) Q_mid with
the END rates (nothing touches v, omega after the rate update), hence
    x_mid = x_end - (dt/2) v_end,   Q_mid = R((dt/2) omega_end)^T Q_end,
followed by the boundary condition's constrain_values (which the reference applied at that
instant: build.py:71-74, soft_pendulum_3d/build.py:31-34), and the strains are evaluated there with
the formulas of the step kernels.  The tangents this yields are the row the kernel itself caches at
the force evaluation (softrod_state_view.tangents) to rounding — tests/test_gpu_parity.py checks
that.  Rendering itself (matplotlib / POV-Ray) stays out of scope; this is what its inputs would be.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, List, NamedTuple, Sequence

import numpy as np


def half_step_rotation(omega: np.ndarray, h: float, eps_rot_axis: float = 1e-14) -> np.ndarray:
    """R (3, 3, n) of the kinematic update Q <- R Q for the step h (PyElastica _get_rotation_matrix:
    axis = omega / (|omega| + eps), angle = h |omega|; the TRANSPOSED Rodrigues matrix)."""
    th = np.sqrt((omega * omega).sum(axis=0))
    a = omega / (th + eps_rot_axis)
    ang = th * h
    up, usq = np.sin(ang), 1.0 - np.cos(ang)
    R = np.empty((3, 3, omega.shape[1]))
    R[0, 0] = 1.0 - usq * (a[1] * a[1] + a[2] * a[2])
    R[1, 1] = 1.0 - usq * (a[0] * a[0] + a[2] * a[2])
    R[2, 2] = 1.0 - usq * (a[0] * a[0] + a[1] * a[1])
    R[0, 1] = up * a[2] + usq * a[0] * a[1]
    R[1, 0] = -up * a[2] + usq * a[0] * a[1]
    R[0, 2] = -up * a[1] + usq * a[0] * a[2]
    R[2, 0] = up * a[1] + usq * a[0] * a[2]
    R[1, 2] = up * a[0] + usq * a[1] * a[2]
    R[2, 1] = -up * a[0] + usq * a[1] * a[2]
    return R


def mid_substep_configuration(x, v, Q, w, dt: float, eps_rot_axis: float = 1e-14):
    """(x_mid, Q_mid): the configuration at which the LAST substep evaluated its forces (module
    docstring), before the boundary condition's constrain_values."""
    R = half_step_rotation(w, 0.5 * dt, eps_rot_axis)
    return x - 0.5 * dt * v, np.einsum("jik,jlk->ilk", R, Q)       # R^T Q


def constrain_values_host(features: int, x, Q, fixed_pos, fixed_dir, base_xy=None):
    """The boundary condition's constrain_values on node 0 / element 0, in place (what the kernels'
    constrain_values_n does; build.py:71-74, soft_pendulum_3d/build.py:31-34, OneEndFixedBC)."""
    from . import _capi

    if features & _capi.FEAT_PENDULUM_BC:
        x[1, 0], x[2, 0] = fixed_pos[1], fixed_pos[2]
        Q[0, :, 0], Q[2, :, 0] = fixed_dir[0], fixed_dir[2]       # row 1 untouched
    if features & _capi.FEAT_FIXED_BC:
        x[:, 0] = fixed_pos
        Q[:, :, 0] = fixed_dir
    if features & _capi.FEAT_MOVING_BASE_BC:
        x[0, 0], x[1, 0], x[2, 0] = base_xy[0], base_xy[1], fixed_pos[2]
        Q[:, :, 0] = fixed_dir


def rod_strains(x: np.ndarray, Q: np.ndarray, rest_length: float, base_radius,
                acos_shift: float = 1e-10, eps_sin: float = 1e-14) -> Dict[str, np.ndarray]:
    """x (3, n+1), Q (3, 3, n) -> lengths, dilatation, voronoi_dilatation, radius, sigma, kappa.
    base_radius: the rest radius, a scalar or one per element (a tapered rod)."""
    d = x[:, 1:] - x[:, :-1]
    lengths = np.sqrt((d * d).sum(axis=0)) + 1e-14
    tangents = d / lengths
    dilatation = lengths / rest_length
    vor = 0.5 * (lengths[1:] + lengths[:-1])
    voronoi_dilatation = vor / rest_length            # uniform rod: rest Voronoi length = rest length
    radius = base_radius * np.sqrt(rest_length / lengths)      # volume-preserving
    sigma = dilatation * np.einsum("ijk,jk->ik", Q, tangents)
    sigma[2] -= 1.0
    # kappa = -log(Q_{k+1} Q_k^T) / D  (_inv_rotate)
    R = np.einsum("ijk,ljk->ilk", Q[:, :, 1:], Q[:, :, :-1])
    vec = np.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    trace = R[0, 0] + R[1, 1] + R[2, 2]
    theta = np.arccos(np.clip(0.5 * trace - 0.5 - acos_shift, -1.0, 1.0))
    kappa = vec * (-0.5 * theta / np.sin(theta + eps_sin)) / rest_length
    return {"lengths": lengths, "dilatation": dilatation, "voronoi_dilatation": voronoi_dilatation,
            "radius": radius, "sigma": sigma, "kappa": kappa, "tangents": tangents}


def rod_material_host(cfg, radius=None) -> Dict[str, np.ndarray]:
    """What CosseratRod.straight_rod derives for the energies, as the kernels hold it (RodParams for a uniform rod,
    the softrod_set_radius_profile table for a tapered one): nodal masses (n+1,) with half masses at the ends,
    J (3, n) and the shear diagonal (3, n) per element, the bend diagonal (3, n-1) on the Voronoi vertices
    (rest-length-weighted average of the two elements), the rest lengths.  radius: per-element radii or None."""
    n = int(cfg.n_elem)
    rl = float(cfg.base_length) / n
    r = np.full(n, float(cfg.base_radius)) if radius is None else np.asarray(radius, np.float64).reshape(n)
    A = np.pi * r * r
    I1 = A * A / (4.0 * np.pi)
    I = np.stack([I1, I1, 2.0 * I1])
    J = I * (float(cfg.density) * rl)
    shear = np.stack([float(cfg.alpha_c) * float(cfg.shear_modulus) * A] * 2 + [float(cfg.youngs_modulus) * A])
    B = np.stack([float(cfg.youngs_modulus) * I[0], float(cfg.youngs_modulus) * I[1], float(cfg.shear_modulus) * I[2]])
    bend = (B[:, 1:] * rl + B[:, :-1] * rl) / (rl + rl)
    half = 0.5 * float(cfg.density) * (np.pi * r * r * rl)
    mass = np.zeros(n + 1)
    mass[:-1] += half
    mass[1:] += half
    return {"mass": mass, "J": J, "shear": shear, "bend": bend, "rest_length": rl, "rest_voronoi": 0.5 * (rl + rl)}


def rod_energies_host(x, v, Q, w, time: float, cfg, material, rest_kappa=None, fixed_pos=None, fixed_dir=None,
                      base_xy=None) -> np.ndarray:
    """NumPy twin of softrod_rod_energies for one rod: [translational, rotational, bending, shear].

    The instant is PyElastica's (module docstring): the strains of the mid-substep configuration
    (mid_substep_configuration, then constrain_values_host), the end-of-step rates; time == 0 (a reset) uses
    the state as it stands.  The forms are our recollection of pyelastica 1.0.0's compute_*_energy (not on
    disk): 1/2 sum m|v|^2, 1/2 sum w.(J w)/e, 1/2 sum dk.B dk D^ with dk = kappa - rest_kappa, 1/2 sum s.S s l^.
    material: rod_material_host(...); rest_kappa (3, n-1) or None (zero)."""
    x, Q = np.array(x, np.float64), np.array(Q, np.float64)
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    if time != 0.0:
        x, Q = mid_substep_configuration(x, v, Q, w, float(cfg.dt), float(cfg.eps_rot_axis))
        if fixed_pos is not None:
            constrain_values_host(int(cfg.features), x, Q, fixed_pos, fixed_dir, base_xy)
    rl = material["rest_length"]
    s = rod_strains(x, Q, rl, 1.0, float(cfg.acos_shift), float(cfg.eps_sin))
    dk = s["kappa"] if rest_kappa is None else s["kappa"] - rest_kappa
    trans = 0.5 * (material["mass"] * (v * v).sum(0)).sum()
    rot = 0.5 * ((material["J"] * w * w).sum(0) / s["dilatation"]).sum()
    bend = 0.5 * ((material["bend"] * dk * dk).sum(0) * material["rest_voronoi"]).sum()
    shear = 0.5 * ((material["shear"] * s["sigma"] * s["sigma"]).sum(0) * rl).sum()
    return np.array([trans, rot, bend, shear])


class RodStrains(NamedTuple):
    """What softrod_rod_strains / rod_strains() return (include/softrod.h): sigma (.., 3, n_elem), kappa
    (.., 3, n_elem - 1; not reduced by the rest curvature), dilatation (.., n_elem), voronoi_dilatation
    (.., n_elem - 1), internal_force S sigma (.., 3, n_elem), internal_couple B (kappa - rest_kappa) (.., 3, n_elem - 1)."""
    sigma: object
    kappa: object
    dilatation: object
    voronoi_dilatation: object
    internal_force: object
    internal_couple: object


def rod_strains_views(buf) -> RodStrains:
    """The six fields as views of softrod_rod_strains' buffer (.., 14, n_elem): the Voronoi rows without their
    last (zero) column."""
    return RodStrains(buf[..., 0:3, :], buf[..., 3:6, :-1], buf[..., 6, :], buf[..., 7, :-1], buf[..., 8:11, :],
                      buf[..., 11:14, :-1])


def rod_strains_host(x, v, Q, w, time: float, cfg, material, rest_kappa=None, fixed_pos=None, fixed_dir=None,
                     base_xy=None) -> RodStrains:
    """NumPy twin of softrod_rod_strains for one rod, at rod_energies_host's instant: the strains of the mid-substep
    configuration (mid_substep_configuration, then constrain_values_host); time == 0 (a reset) uses the state as
    it stands.  internal_force = S sigma and internal_couple = B (kappa - rest_kappa) are the passive elastic loads
    (no muscle layers), so that 1/2 sum sigma . n l^ and 1/2 sum (kappa - rest_kappa) . m D^ are rod_energies_host's
    shear and bending entries.  material: rod_material_host(...); rest_kappa (3, n-1) or None (zero)."""
    x, Q = np.array(x, np.float64), np.array(Q, np.float64)
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    if time != 0.0:
        x, Q = mid_substep_configuration(x, v, Q, w, float(cfg.dt), float(cfg.eps_rot_axis))
        if fixed_pos is not None:
            constrain_values_host(int(cfg.features), x, Q, fixed_pos, fixed_dir, base_xy)
    s = rod_strains(x, Q, material["rest_length"], 1.0, float(cfg.acos_shift), float(cfg.eps_sin))
    dk = s["kappa"] if rest_kappa is None else s["kappa"] - rest_kappa
    return RodStrains(s["sigma"], s["kappa"], s["dilatation"], s["voronoi_dilatation"], material["shear"] * s["sigma"],
                      material["bend"] * dk)


class MuscleLoads(NamedTuple):
    """What softrod_muscle_loads / muscle_loads() return (include/softrod.h; PARITY UNPINNED like the muscle law
    itself): layer_force (.., 4, n_elem) and layer_length (.., 4, n_elem) of the COOMM layers (zero rows for a layer
    the config does not have), the muscle internal_force (.., 3, n_elem) and internal_couple (.., 3, n_elem - 1) in
    the material frame, and the equivalent external_force (.., 3, n_elem + 1) on the nodes and external_couple
    (.., 3, n_elem) on the elements that ApplyMuscles adds to the rod."""
    layer_force: object
    layer_length: object
    internal_force: object
    internal_couple: object
    external_force: object
    external_couple: object


def muscle_loads_views(buf) -> MuscleLoads:
    """The six fields as views of softrod_muscle_loads' buffer (.., 20, n_elem + 1): every row without its zero
    columns."""
    return MuscleLoads(buf[..., 0:4, :-1], buf[..., 4:8, :-1], buf[..., 8:11, :-1], buf[..., 11:14, :-2],
                       buf[..., 14:17, :], buf[..., 17:20, :-1])


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _difference(a):
    """(3, k) -> (3, k + 1): a padded with a zero column at both ends, differenced."""
    out = np.zeros((3, a.shape[1] + 1))
    out[:, :-1] += a
    out[:, 1:] -= a
    return out


def muscle_loads_host(x, v, Q, w, time: float, cfg, material, layers, activation, radius=None, fixed_pos=None,
                      fixed_dir=None, base_xy=None) -> MuscleLoads:
    """NumPy twin of softrod_muscle_loads for one rod, at rod_strains_host's instant: the mid-substep configuration
    (mid_substep_configuration, then constrain_values_host); time == 0 (a reset) uses the state as it stands.  The law
    is the one csrc/softrod_muscle.hpp restates (Chang et al. 2023, section 2(c); PARITY UNPINNED), with the config's
    muscle_kind, muscle_tm_length_law, muscle_equiv_load_form, muscle_position_current_radius, muscle_fl_degree /
    muscle_fl_coef and n_muscles.  layers: (ratio_position (m, 3, n), strength (m, n)) as _capi.es_muscle_layers
    returns them; activation (>= m, n): the resident activation rows of this rod; radius: the per-element rest radii
    of a tapered rod, or None for cfg.base_radius; material: rod_material_host(...)."""
    x, Q = np.array(x, np.float64), np.array(Q, np.float64)
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    if time != 0.0:
        x, Q = mid_substep_configuration(x, v, Q, w, float(cfg.dt), float(cfg.eps_rot_axis))
        if fixed_pos is not None:
            constrain_values_host(int(cfg.features), x, Q, fixed_pos, fixed_dir, base_xy)
    n = Q.shape[2]
    rl, rv = material["rest_length"], material["rest_voronoi"]
    rest_radius = np.full(n, float(cfg.base_radius)) if radius is None else np.asarray(radius, np.float64).reshape(n)
    s = rod_strains(x, Q, rl, rest_radius, float(cfg.acos_shift), float(cfg.eps_sin))
    e, kappa = s["dilatation"], s["kappa"]
    qt = np.einsum("ijk,jk->ik", Q, s["tangents"])
    shear = e * qt                                               # sigma + (0, 0, 1)
    kappa_e = np.zeros((3, n))                                   # Voronoi -> elements, half weights at both ends
    kappa_e[:, :-1] += 0.5 * kappa
    kappa_e[:, 1:] += 0.5 * kappa
    rad = s["radius"] if int(cfg.muscle_position_current_radius) else rest_radius
    ratio, strength = np.asarray(layers[0], np.float64), np.asarray(layers[1], np.float64)
    activation = np.asarray(activation, np.float64)
    degree = int(cfg.muscle_fl_degree)
    layer_force, layer_length = np.zeros((4, n)), np.zeros((4, n))
    f, c = np.zeros((3, n)), np.zeros((3, n))
    for m in range(int(cfg.n_muscles)):
        pos = rad * ratio[m]
        nu = shear + _cross(kappa_e, pos)
        norm = np.sqrt((nu * nu).sum(axis=0))
        length = norm
        if int(cfg.muscle_kind[m]) == 1 and int(cfg.muscle_tm_length_law) == 0:       # a transverse layer: radial fibres
            length = 1.0 / np.sqrt(norm)
        fl = np.zeros(n)
        for p in range(degree, -1, -1):                          # Horner, as the kernels
            fl = fl * length + float(cfg.muscle_fl_coef[p])
        F = activation[m] * strength[m] * np.where(fl < 0.0, 0.0, fl)
        g = F * (nu / norm)
        layer_force[m], layer_length[m] = F, length
        f += g
        c += _cross(pos, g)
    cv = 0.5 * (c[:, :-1] + c[:, 1:])
    QT = np.transpose(Q, (1, 0, 2))
    if int(cfg.muscle_equiv_load_form) == 0:    # F = D^h(Q^T f); tau = D^h(c_v) + A^h(kappa x c_v D^) + (e Q t) x f l^
        ef = 1.0
        ext_force = _difference(np.einsum("ijk,jk->ik", QT, f))
        arm = shear
    else:                                       # PyElastica's internal-load form: Q^T f / e, c_v / eps^3, (Q t) x f l^
        ef = 1.0 / s["voronoi_dilatation"] ** 3
        ext_force = _difference(np.einsum("ijk,jk->ik", QT, f) / e)
        arm = qt
    h3 = _cross(kappa, cv) * rv * ef
    trapezoid = np.zeros((3, n))
    trapezoid[:, :-1] += 0.5 * h3
    trapezoid[:, 1:] += 0.5 * h3
    ext_couple = _difference(cv * ef) + trapezoid + _cross(arm, f) * rl
    return MuscleLoads(layer_force, layer_length, f, cv, ext_force, ext_couple)


class JointLoads(NamedTuple):
    """What softrod_joint_loads / joint_loads() return (include/softrod.h): per arm the load FixedJoint2Rigid exchanges
    with the rigid body — body_force (.., rods, 3) = contact_force, added to the body (lab frame); body_torque
    (.., rods, 3), added to the body (body frame); arm_force (.., rods, 3) = -contact_force, added to the arm's node 0;
    arm_torque (.., rods, 3), added to the arm's element 0 (its material frame); gap (.., rods, 3) =
    end_distance_vector and gap_length (.., rods) = end_distance — and for the body net_force, net_torque (.., 3), the
    per-arm rows summed in arm order, with the linear acceleration (.., 3) and the body-frame angular_acceleration
    (.., 3) they give it under its constraints."""
    body_force: object
    body_torque: object
    arm_force: object
    arm_torque: object
    gap: object
    gap_length: object
    net_force: object
    net_torque: object
    acceleration: object
    angular_acceleration: object


def joint_loads_views(buf) -> JointLoads:
    """The ten fields as views of softrod_joint_loads' buffer (.., rods + 1, 16): rows 0 .. rods - 1 the joints, the last
    row the body."""
    arms, body = buf[..., :-1, :], buf[..., -1, :]
    return JointLoads(arms[..., 0:3], arms[..., 3:6], arms[..., 6:9], arms[..., 9:12], arms[..., 12:15], arms[..., 15],
                      body[..., 0:3], body[..., 3:6], body[..., 6:9], body[..., 9:12])


class RodDynamics(NamedTuple):
    """What softrod_rod_dynamics / rod_dynamics() return (include/softrod.h): the two sides of every rod's equation of
    motion from ONE evaluation at the resident state — internal_force (.., rods, 3, n_elem + 1) on the nodes (lab
    frame) and internal_torque (.., rods, 3, n_elem) on the elements (material frame), CosseratRod's
    _compute_internal_forces / _torques; external_force (.., 3, n_elem + 1) and external_torque (.., 3, n_elem),
    everything synchronize adds: the joint, gravity, the point force, the tip force, the muscle layers' equivalent
    loads and the plane contact; acceleration (.., 3, n_elem + 1) = (internal_force + external_force) / mass and
    angular_acceleration (.., 3, n_elem) = J^-1 (internal_torque + external_torque) e, update_accelerations'."""
    internal_force: object
    internal_torque: object
    external_force: object
    external_torque: object
    acceleration: object
    angular_acceleration: object


def rod_dynamics_views(buf) -> RodDynamics:
    """The six fields as views of softrod_rod_dynamics' buffer (.., rods, 18, n_elem + 1): three rows each, the
    per-element fields without the last column."""
    return RodDynamics(buf[..., 0:3, :], buf[..., 3:6, :-1], buf[..., 6:9, :], buf[..., 9:12, :-1],
                       buf[..., 12:15, :], buf[..., 15:18, :-1])


class RodClearance(NamedTuple):
    """What softrod_rod_clearance / rod_clearance() return (include/softrod.h): for every row rod a and column rod b of
    an env, gap (.., rods, rods) = the least (centre-line distance - r_i - r_j) over the element pairs (negative when
    the capsules interpenetrate; a == b: over the pairs with j - i >= self_gap), distance (.., rods, rods) = that
    pair's centre-line distance, element (.., rods, rods, 2) = (i, j) as exact float64 and point (.., rods, rods, 2) =
    (s, t), the closest points' parameters along the two elements; [b][a] is [a][b] with i <-> j, s <-> t.  For the
    env's target: target_distance (.., rods) from the target to the nearest point of rod a's centre line, target_gap
    = target_distance - r_i, target_element i and target_point s; all four None for an env kind without a target.
    No pair: +inf, +inf, -1, -1, 0, 0.  A non-finite rod: NaN, NaN, -1, -1, NaN, NaN in its rows and columns."""
    gap: object
    distance: object
    element: object
    point: object
    target_gap: object
    target_distance: object
    target_element: object
    target_point: object


def rod_clearance_views(buf, has_target: bool = True) -> RodClearance:
    """The eight fields as views of softrod_rod_clearance's buffer (.., rods, rods + 1, 6): the last column holds the
    target's records (None fields with has_target false)."""
    rods, tgt = buf[..., :-1, :], buf[..., -1, :]
    target = (tgt[..., 0], tgt[..., 1], tgt[..., 2], tgt[..., 4]) if has_target else (None,) * 4
    return RodClearance(rods[..., 0], rods[..., 1], rods[..., 2:4], rods[..., 4:6], *target)


class EpisodeStatistics(NamedTuple):
    """What episode_statistics() returns (softrod_episode_stats_*, include/softrod.h), NumPy values: count = episodes
    finished by the whole batch since record_episode_statistics(); returns (m,) float64, lengths (m,) int32, times (m,)
    float64 — the simulated end time, the env clock — and envs (m,) int32, the env each episode ran in: the last
    m = min(count, buffer_length) finished episodes in chronological order, oldest first (within one step the finished
    envs in ascending env index); finished (N,) int32, the episodes ended per env."""
    count: int
    returns: np.ndarray
    lengths: np.ndarray
    times: np.ndarray
    envs: np.ndarray
    finished: np.ndarray


def episode_ring_order(count: int, ring: int) -> np.ndarray:
    """The ring's slots in chronological order, oldest first: finished episode number c (0-based) sits in slot
    c % ring, so the last min(count, ring) episodes are numbers max(0, count - ring) .. count - 1."""
    count, ring = int(count), int(ring)
    return np.arange(max(0, count - ring), count, dtype=np.int64) % ring


class NormalizationState(NamedTuple):
    """What normalization_state() returns and load_normalization_state() takes (softrod_normalize_*,
    include/softrod.h), NumPy values: the running statistics of set_normalization() — Gymnasium's RunningMeanStd per
    observation column, obs_mean / obs_var / obs_count (obs_dim,) float64, and for the discounted return, ret_mean /
    ret_var / ret_count float64 scalars.  What a checkpointed policy carries with its weights."""
    obs_mean: np.ndarray
    obs_var: np.ndarray
    obs_count: np.ndarray
    ret_mean: float
    ret_var: float
    ret_count: float


def _z_rotation(vector, theta):
    """joint.py:7-17."""
    theta = theta / 180.0 * np.pi
    R = np.array([[np.cos(theta), -np.sin(theta), 0.0], [np.sin(theta), np.cos(theta), 0.0], [0.0, 0.0, 1.0]])
    return np.dot(R, vector.T).T


def joint_angles(cfg) -> np.ndarray:
    """(n_arm,) degrees: the `angle` of every arm's FixedJoint2Rigid as softrod_create takes it from the config —
    joint_angle0 + a * joint_angle_step, or 360 / n_arm * a for a config that leaves head_length at zero."""
    na = int(cfg.n_arm)
    if float(cfg.head_length) > 0.0:
        return np.array([float(cfg.joint_angle0) + float(cfg.joint_angle_step) * a for a in range(na)])
    return np.array([0.0 + 360 / float(na) * a for a in range(na)])


def joint_loads_host(x, v, Q, head_x, head_v, head_Q, head_w, cfg, trig=None) -> JointLoads:
    """NumPy twin of softrod_joint_loads for one env, written from the reference — FixedJoint2Rigid.apply_forces /
    apply_torques (utils/custom_elastica/joint.py:47-219) arm by arm in arm order, then the rigid body's
    update_accelerations and BodyBoundaryCondition.compute_constrain_rates as oracle/softrod_oracle_np.py transcribes
    them (fixed_joint_to_rigid, NumpyCylinder.dynamic, constrain_rates) — at the state as it stands.  x (rods, 3, >= 2)
    and v (rods, 3, >= 1): the arms' nodes (node 0 and node 1 are read); Q (rods, 3, 3, >= 1): their directors (element
    0 is read); head_x, head_v, head_w (3,), head_Q (3, 3): the body.  cfg: joint_k / joint_nu / joint_kt, head_radius,
    head_density, head_length, head_fixed, the joint angles (joint_angles) and the arms' rest length.  trig: in place
    of the cosine and sine of each arm's angle, (rods, 2) — the band calibration of tests/joint_loads_ref.py."""
    x, v, Q = (np.asarray(a, np.float64) for a in (x, v, Q))
    head_x, head_v, head_w = (np.asarray(a, np.float64).reshape(3) for a in (head_x, head_v, head_w))
    head_Q = np.asarray(head_Q, np.float64).reshape(3, 3)
    rods = x.shape[0]
    k, nu, kt, radius = float(cfg.joint_k), float(cfg.joint_nu), float(cfg.joint_kt), float(cfg.head_radius)
    rest_length = float(cfg.base_length) / int(cfg.n_elem)
    angles = joint_angles(cfg)
    out = JointLoads(*(np.zeros((rods, 3)) for _ in range(5)), np.zeros(rods), *(np.zeros(3) for _ in range(4)))
    for a in range(rods):
        # apply_forces, :47-123
        rigid_rod_pos = head_x.copy()
        rigid_rod_pos[2] = 0.0
        binormal = head_Q[1]
        if trig is None:
            connection_dir = -_z_rotation(binormal, angles[a])
        else:
            c, s = trig[a]
            connection_dir = -np.dot(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), binormal.T).T
        rigid_rod_pos += connection_dir * radius
        end_distance_vector = x[a, :, 0] - rigid_rod_pos
        end_distance = np.sqrt(np.dot(end_distance_vector, end_distance_vector))
        if end_distance <= np.finfo(np.float64).eps * 1e4:
            normalized = np.array([0.0, 0.0, 0.0])
        else:
            normalized = end_distance_vector / end_distance
        elastic_force = k * end_distance_vector
        relative_velocity = v[a, :, 0] - head_v
        damping_force = -nu * (np.dot(relative_velocity, normalized) * normalized)
        contact_force = elastic_force + damping_force
        # apply_torques, :125-219
        link_direction = x[a, :, 1] - x[a, :, 0]
        tgt_destination = rigid_rod_pos + rest_length * connection_dir
        forcedirection = -kt * (x[a, :, 1] - tgt_destination)
        torque = np.cross(link_direction, forcedirection)
        for i in range(3):
            for j in range(3):
                out.body_torque[a, i] -= head_Q[i, j] * torque[j]
                out.arm_torque[a, i] += Q[a, i, j, 0] * torque[j]
        out.body_force[a] = contact_force
        out.arm_force[a] = -contact_force
        out.gap[a] = end_distance_vector
        out.gap_length[a] = end_distance
        out.net_force[:] += out.body_force[a]          # external_forces[..., index_one] += contact_force, arm after arm
        out.net_torque[:] += out.body_torque[a]
    if not int(cfg.head_fixed):
        # Cylinder: mass and diagonal inertia as PyElastica allocates them; update_accelerations; constrain_rates
        length = float(cfg.head_length) if float(cfg.head_length) > 0.0 else 2.0 * float(cfg.base_radius)
        area = np.pi * radius * radius
        mass = np.pi * radius * radius * length * float(cfg.head_density)
        i1 = area * area / (4.0 * np.pi)
        J = np.array([i1, i1, 2.0 * i1]) * float(cfg.head_density) * length
        jw = J * head_w
        gyro = np.array([jw[1] * head_w[2] - jw[2] * head_w[1], jw[2] * head_w[0] - jw[0] * head_w[2],
                         jw[0] * head_w[1] - jw[1] * head_w[0]])
        out.acceleration[:] = out.net_force / mass
        out.angular_acceleration[:] = (1.0 / J) * (gyro + out.net_torque)
        out.acceleration[2] = 0.0                      # compute_constrain_rates holds v_z, omega_x, omega_y
        out.angular_acceleration[:2] = 0.0
    return out


class RodRecorder:
    """Collects RodCallBack's fields for `env_indices` of a batch; one dict of lists per env,
    keyed like the reference's `rod_parameters_dict`."""

    FIELDS = ("time", "radius", "dilatation", "voronoi_dilatation", "position", "director", "velocity",
              "omega", "sigma", "kappa")

    def __init__(self, backend, env_indices: Sequence[int] = (0,)):
        self.backend = backend
        self.env_indices = [int(i) for i in env_indices]
        cfg = backend.cfg
        self.rest_length = float(cfg.base_length) / int(cfg.n_elem)
        self.base_radius = float(cfg.base_radius)
        prof = getattr(backend, "_tables", {}).get("radius_profile")
        if prof is not None:                                    # tapered rod: per-element rest radii
            self.base_radius = np.frombuffer(prof, np.float64).copy()
        self.acos_shift = float(cfg.acos_shift)
        self.eps_sin = float(cfg.eps_sin)
        self.eps_rot_axis = float(cfg.eps_rot_axis)
        self.dt = float(cfg.dt)
        self.features = int(cfg.features)
        self.params: List[Dict[str, list]] = [defaultdict(list) for _ in self.env_indices]
        self.last_mid_tangents: List[np.ndarray] = []           # of the latest record(): test access

    def _bc(self):
        """fixed_position (k, 3), fixed_directors (k, 3, 3), moving-base position (k, 2) of the recorded envs."""
        st = self.backend.state()
        idx = self.env_indices
        bc = st["bc_targets"][:, idx].cpu().numpy()             # (12, k)
        ctrl = st["control"][:2, idx].cpu().numpy()             # (2, k)
        return bc[:3].T, bc[3:].T.reshape(len(idx), 3, 3), ctrl.T

    def record(self) -> None:
        snap = self.backend.rod_snapshot(self.env_indices)
        fpos, fdir, base = self._bc()
        self.last_mid_tangents = []
        for k, p in enumerate(self.params):
            x, Q = snap["x"][k], snap["Q"][k]
            xm, Qm = mid_substep_configuration(x, snap["v"][k], Q, snap["w"][k], self.dt, self.eps_rot_axis)
            constrain_values_host(self.features, xm, Qm, fpos[k], fdir[k], base[k])
            s = rod_strains(xm, Qm, self.rest_length, self.base_radius, self.acos_shift, self.eps_sin)
            self.last_mid_tangents.append(s["tangents"])
            p["time"].append(float(snap["time"][k]))
            p["radius"].append(s["radius"])
            p["dilatation"].append(s["dilatation"])
            p["voronoi_dilatation"].append(s["voronoi_dilatation"])
            p["position"].append(x.copy())
            p["director"].append(Q.copy())
            p["velocity"].append(snap["v"][k].copy())
            p["omega"].append(snap["w"][k].copy())
            p["sigma"].append(s["sigma"])
            p["kappa"].append(s["kappa"])


class OctoRecorder:
    """FlatEnv's taps (octopus/flat_env.py:188-206): one RodCallBack dict per arm
    (`rod_parameters_dict_list`, when config_generate_video) and the head's
    RigidCylinderCallBack dict (`head_dict`: time, step, position, velocity —
    callback_func.py:4-20 — when config_save_head_data), for ONE env of the batch, sampled
    once per env.step like the reference's `current_step % step_skip == 0`."""

    def __init__(self, backend, env_index: int = 0, rods: bool = True, head: bool = True):
        self.backend = backend
        self.env_index = int(env_index)
        cfg = backend.cfg
        self.n_arm = int(cfg.n_arm)
        self.rest_length = float(cfg.base_length) / int(cfg.n_elem)
        self.base_radius = float(cfg.base_radius)
        self.acos_shift = float(cfg.acos_shift)
        self.eps_sin = float(cfg.eps_sin)
        self.n_substeps = int(cfg.n_substeps)
        self.eps_rot_axis = float(cfg.eps_rot_axis)
        self.dt = float(cfg.dt)
        self.rod_parameters_dict_list = [defaultdict(list) for _ in range(self.n_arm)] if rods else None
        self.head_dict = defaultdict(list) if head else None
        self._steps = 0

    def record(self) -> None:
        st = self.backend.octo_state_numpy()
        e = self.env_index
        self._steps += 1
        t = float(st["time"][e])
        if self.rod_parameters_dict_list is not None:
            for a, p in enumerate(self.rod_parameters_dict_list):
                x, Q = st["x"][e, a], st["Q"][e, a]
                # the arms carry no boundary condition of their own (the joints hold them): the
                # mid-substep configuration is the plain back half step
                xm, Qm = mid_substep_configuration(x, st["v"][e, a], Q, st["w"][e, a], self.dt, self.eps_rot_axis)
                s = rod_strains(xm, Qm, self.rest_length, self.base_radius, self.acos_shift, self.eps_sin)
                p["time"].append(t)
                p["radius"].append(s["radius"])
                p["dilatation"].append(s["dilatation"])
                p["voronoi_dilatation"].append(s["voronoi_dilatation"])
                p["position"].append(x.copy())
                p["director"].append(Q.copy())
                p["velocity"].append(st["v"][e, a].copy())
                p["omega"].append(st["w"][e, a].copy())
                p["sigma"].append(s["sigma"])
                p["kappa"].append(s["kappa"])
        if self.head_dict is not None:
            self.head_dict["time"].append(t)
            self.head_dict["step"].append(self._steps * self.n_substeps)
            self.head_dict["position"].append(st["head_x"][e].reshape(3, 1).copy())
            self.head_dict["velocity"].append(st["head_v"][e].reshape(3, 1).copy())
