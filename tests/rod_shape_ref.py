"""Shared by tests/test_rod_shape.py (CPU) and tests/test_gpu_rod_shape.py: the NumPy float64 yardstick of
set_rod_shape() (softrod_set_rod_shape, include/softrod.h), the bands, and the random fields of the GPU cases.

THE DEFINITION, one rod at a time, as a sequential product from the base pose (x_0, Q_0; Q's rows are the directors):
    Q_{k+1} = exp([-kappa_k D^]x) Q_k        kappa in the material frame, not reduced by rest curvature
    x_{k+1} = x_k + l^ Q_k^T (sigma_k + e3)
with the exact rotation exp([v]x) = I + sin(th)/th [v]x + (1 - cos(th))/th^2 [v]x^2, th = |v|.  The device forms the
same products as a doubling scan, so its rounding differs from this loop's.

THE BANDS.  The sequential product and the doubling scan in float64 against an 80-bit evaluation, for 2, 5, 63, 64 and
126 elements, |kappa D^| <= 0.3, |sigma| <= 0.05, stayed within 1.3e-15 on director entries, 4.3e-16 L on positions and
1.4e-15 on orthonormality.  The device band is about 100 times that spread — room for a device libm sin / cos a few
ulp off and for FMA contraction, eight orders below any convention error:
    BAND_Q   2e-13      director entries, orthonormality, tangent entries (|x_{k+1} - x_k| >= 0.9 l^ keeps them there)
    BAND_X   2e-13 L    positions
    BAND_KAPPA 1e-9 max|kappa|   rod_strains().kappa against the input: slot_kappa's acos_shift scales kappa by
                        1 + 1e-10 / 3 (measured 3.4e-11 relative)
tests/test_rod_shape.py holds the yardstick's own float64 error against long double to a tenth of the bands."""
import numpy as np

from gym_softrobot_amd import diagnostics

BAND_Q = 2e-13
BAND_X = 2e-13          # times the rod's length
BAND_KAPPA = 1e-9       # times max |kappa|
SIZES = (2, 5, 63, 64, 126)
MAX_ANGLE = 0.3         # |kappa D^| of the random fields
MAX_SIGMA = 0.05


def rotation(v, dtype=np.float64):
    """exp([v]x) for one 3-vector: Rodrigues, with the series below |v|^2 = 1e-6."""
    v = np.asarray(v, dtype)
    t = v @ v
    if t < 1e-6:
        a = 1 - t / 6 + t * t / 120
        b = dtype(0.5) - t / 24 + t * t / 720
    else:
        th = np.sqrt(t)
        a = np.sin(th) / th
        b = (1 - np.cos(th)) / t
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype)
    return np.eye(3, dtype=dtype) + a * K + b * (K @ K)


def build(x0, Q0, kappa, sigma, rest_length, rest_voronoi=None, dtype=np.float64, n=None):
    """One rod from its base pose: x0 (3,), Q0 (3, 3), kappa (3, n - 1) or None, sigma (3, n) or None (`n` is needed
    only when both are None) -> x (3, n + 1), Q (3, 3, n)."""
    if n is None:
        n = sigma.shape[1] if sigma is not None else kappa.shape[1] + 1
    kappa = np.zeros((3, n - 1), dtype) if kappa is None else np.asarray(kappa, dtype)
    sigma = np.zeros((3, n), dtype) if sigma is None else np.asarray(sigma, dtype)
    rl = dtype(rest_length)
    rv = rl if rest_voronoi is None else dtype(rest_voronoi)
    e3 = np.array([0, 0, 1], dtype)
    x = np.empty((3, n + 1), dtype)
    Q = np.empty((3, 3, n), dtype)
    x[:, 0] = np.asarray(x0, dtype)
    Q[:, :, 0] = np.asarray(Q0, dtype)
    for k in range(n):
        x[:, k + 1] = x[:, k] + rl * (Q[:, :, k].T @ (sigma[:, k] + e3))
        if k + 1 < n:
            Q[:, :, k + 1] = rotation(-kappa[:, k] * rv, dtype) @ Q[:, :, k]
    return x, Q


def derived(x, Q, cfg, rest_length=None):
    """What reset derives from a shape: (tangents (3, n), kappa (3, n - 1)) with reset's eps_length and slot_kappa's
    law (diagnostics.rod_strains: the twin the strain read-out is held to)."""
    n = Q.shape[2]
    rl = float(cfg.base_length) / n if rest_length is None else rest_length
    s = diagnostics.rod_strains(np.asarray(x, np.float64), np.asarray(Q, np.float64), rl, 1.0,
                                float(cfg.acos_shift), float(cfg.eps_sin))
    return s["tangents"], s["kappa"]


def center_of_mass_xy(x, mass):
    """compute_position_center_of_mass()[:2] of one rod: nodal masses (n + 1,) with half masses at the ends."""
    return (mass * x[:2]).sum(axis=1) / mass.sum()


def random_fields(rng, n_envs, rods, n, rest_voronoi, angle=MAX_ANGLE, stretch=MAX_SIGMA, rates=True):
    """kappa, sigma, velocity, omega of the GPU cases: uniform in +-angle / D^ and +-stretch per component / sqrt(3), so
    that |kappa D^| <= angle and |sigma| <= stretch hold for the vectors."""
    s3 = np.sqrt(3.0)
    kappa = rng.uniform(-angle / s3, angle / s3, (n_envs, rods, 3, n - 1)) / rest_voronoi
    sigma = rng.uniform(-stretch / s3, stretch / s3, (n_envs, rods, 3, n))
    velocity = rng.uniform(-0.1, 0.1, (n_envs, rods, 3, n + 1)) if rates else None
    omega = rng.uniform(-1.0, 1.0, (n_envs, rods, 3, n)) if rates else None
    return kappa, sigma, velocity, omega


def orthonormality(Q):
    """max |Q_k Q_k^T - I| over the elements of Q (3, 3, n)."""
    G = np.einsum("ijk,ljk->ilk", Q, Q) - np.eye(3)[:, :, None]
    return float(np.abs(G).max())


# ---- parity after the call: the oracle started from the same configuration ---------------------------------------------
# (id, env id, kwargs, env.steps asserted, per-vertex angle |kappa D^| of the smooth shape, planar?, the bend's director,
# the factor on rod_strains_ref.actions' actions).  Amplitudes and actions were chosen on the CPU: the oracle against its
# FMA build (libsoftrod_oracle_fma.so), started from the same shape, stays within a tenth of the parity band (1e-6
# relative, every observation, reward and state field) over the asserted horizon — measured 4e-14 (pendulum), 2e-10
# (pendulum3d), 3e-11 (arm), 4e-10 (push-100), 9e-12 (flat); no angle is below 0.02.  The plane-contact envs are
# rounding-sensitive where friction sticks and slips: OctoArmSingle from a curled start holds 3e-11 only with no action
# (1e-5 .. 1e-2 with |a| <= 0.3), OctoFlat only when driven as tests/test_gpu_octo.py drives it, |a| <= 22 (2e-3 with
# |a| <= 1, and with none).
PARITY_CASES = [
    ("pendulum-fast", "SoftPendulum-v0", dict(math_mode=1), 2, 0.03, True, 1, 1.0),
    ("pendulum-libm", "SoftPendulum-v0", dict(math_mode=0), 2, 0.03, True, 1, 1.0),
    ("pendulum-out-of-plane", "SoftPendulum-v0", dict(math_mode=1), 2, 0.03, False, 1, 1.0),
    ("pendulum3d", "SoftPendulum3D-v0", {}, 2, 0.03, False, 1, 1.0),
    ("arm", "OctoArmSingle-v0", {}, 2, 0.03, True, 0, 0.0),
    ("push-100", "OctoArmPush-v1", dict(n_elems=100), 2, 0.025, True, 0, 1.0),
    ("flat", "OctoFlat-v0", {}, 1, 0.025, True, 0, 22.0),
]
PARITY_RTOL = 1e-5          # tests/test_gpu_parity.py's RTOL
OBS_TOL = dict(rtol=2e-7, atol=1e-9)        # tests/test_gpu_reference_fixtures.py's: float32 observations, one ulp


def smooth_fields(n_envs, rods, n, rest_voronoi, angle, planar, seed=0, stretch=0.002, axis=1):
    """A smooth curl per rod: kappa D^ = +-angle * sin(pi (m s + phase)) about director `axis` — d2 for the pendulum,
    whose d2 is the plane's normal; d1 for the ground-plane envs, whose d1 is e_z — with sigma_3 = stretch cos(pi s) and a
    shear of 0.4 stretch along the other in-plane director; unless `planar`, also 0.6 of the bend about the other
    director, a twist of 0.4 of it and the same shear out of the plane."""
    rng = np.random.default_rng(seed)
    sv = (np.arange(n - 1) + 1.0) / n
    se = (np.arange(n) + 0.5) / n
    kappa = np.zeros((n_envs, rods, 3, n - 1))
    sigma = np.zeros((n_envs, rods, 3, n))
    for e in range(n_envs):
        for a in range(rods):
            m, ph, sign = rng.uniform(0.5, 1.5), rng.uniform(0, 1), rng.choice([-1.0, 1.0])
            kappa[e, a, axis] = sign * angle * np.sin(np.pi * (m * sv + ph))
            sigma[e, a, 1 - axis] = 0.4 * stretch * np.sin(2 * np.pi * se)
            sigma[e, a, 2] = stretch * np.cos(np.pi * se)
            if not planar:
                kappa[e, a, 1 - axis] = 0.6 * angle * np.cos(np.pi * (m * sv + ph))
                kappa[e, a, 2] = 0.4 * angle * np.sin(2 * np.pi * sv)
                sigma[e, a, axis] = 0.4 * stretch * np.sin(np.pi * se)
    return kappa / rest_voronoi, sigma


def oracle_rods(backend, env):
    """The rods of env `env` of a tests/oracle_backend.py backend: one OracleRod, or OctoFlat's arm views."""
    r = backend.rods[env]
    return [r.arm(a) for a in range(r.n_arm)] if hasattr(r, "arm") else [r]


def apply_to_oracle(backend, mask, kappa, sigma):
    """What set_rod_shape does, on the oracle: every rod of the masked envs rebuilt by the yardstick from its own base
    pose ("x", "Q"), rates cleared, the strain caches re-evaluated as CosseratRod.__init__ evaluates them, and
    OctoArmSingle's prev_kappa_state / prev_com_state taken from the new shape (arm_single_env.py:173-174)."""
    cfg = backend.cfg
    for e in np.nonzero(mask)[0]:
        for a, rod in enumerate(oracle_rods(backend, e)):
            x, Q = rod.get("x"), rod.get("Q")
            n = Q.shape[2]
            rl = float(cfg.base_length) / n
            x, Q = build(x[:, 0], Q[:, :, 0], kappa[e, a], sigma[e, a], rl)
            rod.set("x", x)
            rod.set("Q", Q)
            rod.set("v", np.zeros_like(x))
            rod.set("w", np.zeros((3, n)))
            rod._lib.oracle_refresh_strains(rod._h)
            if getattr(backend, "isarm", False):
                rod.set("prev_kappa", rod.get("kappa")[0])
                rod.set("prev_com", center_of_mass_xy(x, rod.get("mass")))


def oracle_observe(backend, env):
    """The oracle's get_state on env `env` as it stands (None for OctoFlat, whose oracle observes only inside a step).
    OctoArmSingle: the step's own get_state with no substep run, zero action (prev_action and rest_kappa are zero
    after a reset of a fresh env), which moves prev_kappa_state / prev_com_state as the device's observe does."""
    r = backend.rods[env]
    if backend.isocto:
        return None
    if backend.isarm:
        r.set_run_substeps(0)
        o = r.env_step_arm(np.zeros(7, np.float32))[0]
        r.set_run_substeps(-1)
        return o
    if backend.ispush:
        return r.observe_push()
    if backend.is3d:
        o = r.observe3d()
        o[6:8] = 0.0            # the env owns _prev_action, cleared by reset
        return o
    r.set_prev_action(0.0)
    return r.observe()
