"""Shared by tests/test_muscle_loads.py (CPU) and tests/test_gpu_muscle_loads.py: the case matrix of muscle_loads(), the
activations written for the instant of a reset, the band units, and the yardstick — diagnostics.muscle_loads_host
evaluated rod by rod on a state read back from a backend (the device's own, or the oracle backend's for the CPU
calibration of the band).

THE BAND UNITS (absolute, fp64), with A = sum_m |strength_m| per element, floored by 1e-3 of its maximum over the rod
so that the thin tip of a tapered arm does not divide by nearly nothing, r the element's rest radius, l^ the rest length:
  layer force       A              layer length      1
  internal force    A              internal couple   A r        (on a Voronoi vertex: the mean of its two elements)
  external force    A  (A / e under muscle_form 1; on a node: the mean of its two elements, the end element at an end)
  external couple   A (r + l^)
No element is left out of any comparison.

BAND is calibrated by tests/test_muscle_loads.py::test_band_is_ten_times_the_twins_own_conditioning and by nothing else:
the smallest power of ten such that, on every case, scaling x, v, Q or w by 1 +- 2^-52 moves the twin by less than a
tenth of it.  The worst movement seen over the matrix is WORST = 1.8e-14 (the layer length of push-126, where the
curvature error of a 126-element arm enters nu_m through kappa x x_m; every other case stays below 9e-15), so 1e-13
does not hold and 1e-12 does."""
import numpy as np

from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import MuscleLoads, muscle_loads_host

try:
    from tests import rod_strains_ref as rs
except ImportError:                                  # imported with tests/ itself on the path
    import rod_strains_ref as rs

BAND = 1e-12
WORST = 1.8e-14          # the calibration's largest printed figure, in band units
SEED = rs.SEED
actions = rs.actions

# (id, env id, envs, kwargs)
CASES = [
    ("push-3", "OctoArmPush-v1", 4, dict(n_elems=3)),          # the smallest rod with two Voronoi vertices
    ("push", "OctoArmPush-v1", 4, {}),                         # 40 elements, tapered
    ("push-63", "OctoArmPush-v1", 4, dict(n_elems=63)),        # the last one-slot size
    ("push-64", "OctoArmPush-v1", 4, dict(n_elems=64)),        # the first two-slot size
    ("push-126", "OctoArmPush-v1", 4, dict(n_elems=126)),
    ("push-v0", "OctoArmPush-v0", 4, {}),                      # discrete: the transverse layer only
    ("pull", "OctoArmPullWeight-v0", 2, {}),
    ("crawl", "OctoCrawl-v0", 2, {}),                          # 8 arms on 4 waves
    ("arm-two", "OctoArmTwo-v0", 2, {}),
    ("reach", "OctoReach-v0", 2, {}),
]


def layers_of(env):
    """(ratio_position (m, 3, n), strength (m, n)) of the handle, from the backend's record of softrod_set_muscle_layers."""
    cfg = env.cfg
    m, n = int(cfg.n_muscles), int(cfg.n_elem)
    raw = np.frombuffer(env.backend._tables["muscle_layers"], np.float64)
    return raw[: m * 3 * n].reshape(m, 3, n).copy(), raw[m * 3 * n:].reshape(m, n).copy()


def _arm_sources(be, e, rods):
    r = be.rods[e]
    return [r.arm(a) if hasattr(r, "arm") else r for a in range(rods)]


def seeded_activations(env, seed=3):
    """(n_envs, rods, 4, n_elem) in [0, 1]: per-element activations for every layer the config has, zero rows above."""
    cfg = env.cfg
    rng = np.random.default_rng(seed)
    act = rng.uniform(0.0, 1.0, (env.num_envs, _capi.config_rods_per_env(cfg), _capi.MAX_MUSCLES, int(cfg.n_elem)))
    act[:, :, int(cfg.n_muscles):] = 0.0
    return act


def write_activations(env, act):
    """Put `act` (seeded_activations' shape) into the resident activation rows: state()["muscle_activation"] on the HIP
    backend, the rods' own rows on the oracle backend."""
    be, cfg = env.backend, env.cfg
    rods, ne = _capi.config_rods_per_env(cfg), int(cfg.n_elem)
    if hasattr(be, "state_numpy"):
        import torch

        st = be.state()
        seg = int(st["arm_stride"])
        rows = st["muscle_activation"]
        for a in range(rods):
            rows[:, :, a * seg: a * seg + ne] = torch.as_tensor(act[:, a].transpose(1, 0, 2), device=rows.device)
        torch.cuda.synchronize(be.device)
    else:
        for e in range(be.n_envs):
            for a, src in enumerate(_arm_sources(be, e, rods)):
                src.set("muscle_activation", act[e, a])


def read_activations(env):
    """(n_envs, rods, 4, n_elem): the resident activation rows."""
    be, cfg = env.backend, env.cfg
    rods, ne = _capi.config_rods_per_env(cfg), int(cfg.n_elem)
    if hasattr(be, "state_numpy"):
        st = be.state()
        seg = int(st["arm_stride"])
        rows = st["muscle_activation"].cpu().numpy()                    # (4, n_envs, lane_stride)
        return np.stack([rows[:, :, a * seg: a * seg + ne].transpose(1, 0, 2) for a in range(rods)], axis=1)
    return np.stack([np.stack([src.get("muscle_activation") for src in _arm_sources(be, e, rods)])
                     for e in range(be.n_envs)])


def rod_states(env):
    """rod_strains_ref.rod_states, each rod with its activation rows (4, n_elem), the handle's layers and its
    per-element rest radii."""
    states = rs.rod_states(env)
    act = read_activations(env)
    layers = layers_of(env)
    radius = rs._radius(env.backend)
    rods = _capi.config_rods_per_env(env.cfg)
    for i, d in enumerate(states):
        e, a = divmod(i, rods)
        d.update(activation=act[e, a], layers=layers, radius=radius)
    return states


def twin(d, scale=None, cfg=None, activation=None):
    """muscle_loads_host on one rod_states() entry; `scale`: factors for x, v, Q, w (the band calibration); `cfg`,
    `activation`: in place of the entry's own."""
    sx, sv, sq, sw = scale or (1.0, 1.0, 1.0, 1.0)
    return muscle_loads_host(d["x"] * sx, d["v"] * sv, d["Q"] * sq, d["w"] * sw, d["time"], cfg or d["cfg"], d["material"],
                             d["layers"], d["activation"] if activation is None else activation, d["radius"],
                             **d.get("bc", {}))


def strength_sum(d):
    """A: sum_m |strength_m| per element, floored by 1e-3 of its maximum over the rod."""
    A = np.abs(d["layers"][1]).sum(axis=0)
    return np.maximum(A, 1e-3 * A.max())


def band_units(d, cfg=None):
    """What BAND multiplies, per field (module docstring)."""
    cfg = cfg or d["cfg"]
    n = int(cfg.n_elem)
    rl = d["material"]["rest_length"]
    A = strength_sum(d)
    r = np.full(n, float(cfg.base_radius)) if d["radius"] is None else np.asarray(d["radius"], np.float64)
    ends = np.concatenate([A[:1], A, A[-1:]])
    A_node = 0.5 * (ends[:-1] + ends[1:])
    if int(cfg.muscle_equiv_load_form) == 1:
        dx = d["x"][:, 1:] - d["x"][:, :-1]
        e = np.sqrt((dx * dx).sum(axis=0)) / rl
        ends = np.concatenate([(A / e)[:1], A / e, (A / e)[-1:]])
        A_node = 0.5 * (ends[:-1] + ends[1:])
    Ar = A * r
    return MuscleLoads(A, 1.0, A, 0.5 * (Ar[:-1] + Ar[1:]), A_node, A * (r + rl))


def worst(got: MuscleLoads, want: MuscleLoads, d, cfg=None):
    """max over all elements of |got - want| in band units, per field (every element counts)."""
    return {f: float(np.max(np.abs(np.asarray(g) - w) / u))
            for f, g, w, u in zip(MuscleLoads._fields, got, want, band_units(d, cfg))}
