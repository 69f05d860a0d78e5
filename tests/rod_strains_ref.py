"""Shared by tests/test_rod_strains.py (CPU) and tests/test_gpu_rod_strains.py: the case matrix of rod_strains(), the
actions, the bands, and the yardstick — diagnostics.rod_strains_host evaluated rod by rod on a state read back from a
backend (the device's own, or the oracle backend's for the CPU calibration of the bands).

THE BANDS (absolute, fp64, positions O(1), element length >= 1/126, a few ulp per libm call):
  sigma, dilatation               1e-12  (dimensionless; the cancellation in x_{i+1} - x_i is eps |x| / l ~ 3e-14)
  kappa * D^, voronoi_dilatation  1e-12  (the angle per Voronoi region: independent of n_elems)
  internal force                  1e-12 * S per component          internal couple   1e-12 * B / D^ per component
No element is left out of any comparison."""
import numpy as np

from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import RodStrains, rod_material_host, rod_strains_host

BAND = 1e-12
SEED = 0
BC = _capi.FEAT_PENDULUM_BC | _capi.FEAT_FIXED_BC | _capi.FEAT_MOVING_BASE_BC
KEYS = ("youngs_modulus", "shear_modulus", "density", "damping_constant")

# (id, env id, envs, kwargs).  "material": a random set_material table; "taper": a radius profile.
CASES = [
    ("pendulum-3", "SoftPendulum-v0", 4, dict(n_elems=3)),
    ("pendulum-63", "SoftPendulum-v0", 4, dict(n_elems=63)),
    ("pendulum-63-libm", "SoftPendulum-v0", 4, dict(n_elems=63, math_mode=_capi.MATH_LIBM)),
    ("pendulum-64", "SoftPendulum-v0", 4, dict(n_elems=64)),
    ("pendulum3d", "SoftPendulum3D-v0", 4, {}),
    ("arm", "OctoArmSingle-v0", 4, {}),
    ("arm-taper", "OctoArmSingle-v0", 4, dict(radius_profile="taper")),
    ("arm-100", "OctoArmSingle-v0", 4, dict(n_elems=100)),
    ("arm-material", "OctoArmSingle-v0", 4, dict(material=True)),
    ("flat", "OctoFlat-v0", 2, {}),
    ("flat-lite", "OctoFlatLite-v0", 2, {}),
    ("soft-arm", "SoftArmTracking-v0", 4, {}),
    ("push", "OctoArmPush-v1", 4, {}),
    ("push-100", "OctoArmPush-v1", 4, dict(n_elems=100)),
    ("push-126", "OctoArmPush-v1", 4, dict(n_elems=126)),
    ("pull", "OctoArmPullWeight-v0", 2, {}),
    ("crawl", "OctoCrawl-v0", 2, {}),
    ("arm-two", "OctoArmTwo-v0", 2, {}),
]


def make_kwargs(kw):
    """The env's keyword arguments of a case (the "material" flag is not one)."""
    kw = {k: v for k, v in kw.items() if k != "material"}
    if kw.get("radius_profile") == "taper":
        edge = np.linspace(0.012, 0.001, 51)
        kw["radius_profile"] = (edge[:-1] + edge[1:]) / 2
    return kw


def randomise_material(env, seed=21):
    """E, rho, nu per env across x0.5 .. x2 of the config's."""
    rng = np.random.default_rng(seed)
    c, n = env.cfg, env.num_envs
    f = {k: 2.0 ** rng.uniform(-1, 1, n) for k in ("youngs_modulus", "density", "damping_constant")}
    env.set_material(None, youngs_modulus=c.youngs_modulus * f["youngs_modulus"], density=c.density * f["density"],
                     damping_constant=c.damping_constant * f["damping_constant"])


def actions(env, env_id, steps=2, seed=1):
    rng = np.random.default_rng(seed)
    n = env.num_envs
    out = []
    for _ in range(steps):
        if getattr(env, "mode", None) == 0 and env_id.startswith("OctoArmPush"):
            out.append(rng.integers(0, 2, (n, 1)).astype(np.float32))
        else:
            lo, hi = env.action_space.low, env.action_space.high
            out.append(rng.uniform(np.maximum(lo, -1.0), np.minimum(hi, 1.0)).astype(np.float32))
    return out


def _radius(be):
    prof = getattr(be, "_tables", {}).get("radius_profile")
    if prof is not None:
        return np.frombuffer(prof, np.float64).copy()
    r = getattr(be, "_radius", None)
    return None if r is None else np.asarray(r, np.float64)


def rod_states(env):
    """One dict per rod of the batch, in buffer order (env major): x, v, Q, w, time, rest_kappa (or None), the
    boundary condition's targets (or None), the env's config with its own material, the material.  Works on the
    HIP backend (state_numpy / octo_state_numpy, material()) and on tests/oracle_backend.py's."""
    be, cfg = env.backend, env.cfg
    n, rods = be.n_envs, _capi.config_rods_per_env(cfg)
    rk = bool(cfg.features & _capi.FEAT_REST_KAPPA_ACTION)
    radius = _radius(be)
    table = env.material() if getattr(be, "_env_material", None) is not None else None
    out = []
    hip = hasattr(be, "state_numpy")
    arms = rods > 1 or int(cfg.env_kind) == _capi.ENV_OCTO_FLAT or int(cfg.env_kind) in _capi.MUSCLE_OCTOPUS_ENVS
    if hip:
        st = be.octo_state_numpy() if arms else be.state_numpy()
        bc = None if arms else be.state()["bc_targets"].cpu().numpy()
    for e in range(n):
        ci = cfg
        if table is not None:
            ci = cfg.copy()
            for k in KEYS:
                setattr(ci, k, float(table[k][e]))
        mat = rod_material_host(ci, radius)
        for a in range(rods):
            if hip and arms:
                d = {k: st[k][e, a] for k in ("x", "v", "Q", "w")}
                d["rest_kappa"] = st["rest_kappa"][e, a] if rk else None
                d["time"] = float(st["time"][e])
            elif hip:
                d = {k: st[k][e] for k in ("x", "v", "Q", "w")}
                d["rest_kappa"] = st["rest_kappa"][e] if rk else None
                d["time"] = float(st["time"][e])
                if cfg.features & BC:
                    d["bc"] = dict(fixed_pos=bc[:3, e], fixed_dir=bc[3:, e].reshape(3, 3), base_xy=st["control"][e, :2])
            else:
                r = be.rods[e]
                src = r.arm(a) if hasattr(r, "arm") else r
                d = {k: src.get(k) for k in ("x", "v", "Q", "w")}
                d["rest_kappa"] = src.get("rest_kappa") if rk else None
                d["time"] = float(r.time)
                if cfg.features & BC:
                    ctrl = be.state()["control"].numpy()
                    d["bc"] = dict(fixed_pos=src.get("fixed_pos"), fixed_dir=src.get("fixed_dir"), base_xy=ctrl[:2, e])
            d.update(cfg=ci, material=mat)
            out.append(d)
    return out


def twin(d, scale=None):
    """rod_strains_host on one rod_states() entry; `scale`: factors for x, v, Q, w (the band calibration)."""
    sx, sv, sq, sw = scale or (1.0, 1.0, 1.0, 1.0)
    return rod_strains_host(d["x"] * sx, d["v"] * sv, d["Q"] * sq, d["w"] * sw, d["time"], d["cfg"], d["material"],
                            d["rest_kappa"], **d.get("bc", {}))


def band_units(d):
    """What the band 1e-12 multiplies, per field: 1 for the strains (kappa is compared as kappa * D^), the row's
    stiffness for the loads (S per component; B / D^ per component, the couple being compared as it is)."""
    m = d["material"]
    return RodStrains(1.0, 1.0 / m["rest_voronoi"], 1.0, 1.0, m["shear"], m["bend"] / m["rest_voronoi"])


def worst(got: RodStrains, want: RodStrains, d):
    """max over all elements of |got - want| in band units, per field (every element counts)."""
    return {f: float(np.max(np.abs(np.asarray(g) - w) / u)) for f, g, w, u in zip(RodStrains._fields, got, want, band_units(d))}


def energies_from_strains(s: RodStrains, d):
    """(bending, shear) of diagnostics.rod_energies_host's forms from a RodStrains: 1/2 sum (kappa - rest_kappa) . m D^
    and 1/2 sum sigma . n l^."""
    m = d["material"]
    dk = np.asarray(s.kappa) if d["rest_kappa"] is None else np.asarray(s.kappa) - d["rest_kappa"]
    bend = 0.5 * ((dk * np.asarray(s.internal_couple)).sum(0) * m["rest_voronoi"]).sum()
    shear = 0.5 * ((np.asarray(s.sigma) * np.asarray(s.internal_force)).sum(0) * m["rest_length"]).sum()
    return bend, shear
