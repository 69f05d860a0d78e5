"""Helpers of the set_reset_shapes tests: the index function restated in NumPy, pool builders, and the hand-driven twin.

The twin is the code as it stood before set_reset_shapes: a batch with autoreset=False and NO pool.  It steps, and where
an env's episode ends it runs reset(mask=done) followed by set_rod_shape(done, kappa=pool_kappa[idx], ...), with idx
from the NumPy index function and a host-side count of each env's resets.  Both sides run the same kernels' arithmetic
on the same draws of each env's stream, so everything is compared bitwise."""
import numpy as np

FIELDS = ("kappa", "sigma", "velocity", "omega")
MASK64 = (1 << 64) - 1

# softrod_reset_shape_index's known answers (include/softrod.h): seed 1, K 3, rows e = 0..5, columns j = 0..2
KNOWN_SEED, KNOWN_K = 1, 3
KNOWN = [[2, 1, 1], [2, 2, 1], [2, 1, 1], [0, 2, 2], [2, 1, 2], [1, 2, 0]]


def _mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def index(seed, env, episode, count):
    """mix(mix(seed + 0x9E3779B97F4A7C15 * (env + 1)) + episode) % count on Python ints, mod 2^64."""
    a = _mix((int(seed) + 0x9E3779B97F4A7C15 * (int(env) + 1)) & MASK64)
    return _mix((a + int(episode)) & MASK64) % int(count)


def widths(n_elem):
    return dict(kappa=n_elem - 1, sigma=n_elem, velocity=n_elem + 1, omega=n_elem)


def pool(cfg, rods, count=KNOWN_K, planar=False, fields=FIELDS):
    """A pool of `count` distinct smooth start shapes, (count, rods, 3, width) float64 each: a total bend of about a
    radian per rod with its sign and size changing from entry to entry and from rod to rod, |sigma| <= 0.02, small rates.
    planar: kappa row 1 (about d2, the in-plane bend of SoftPendulum) only — the planar tier keeps stepping."""
    n = int(cfg.n_elem)
    length = float(cfg.base_length)
    w = widths(n)
    k = np.arange(count, dtype=np.float64)[:, None, None]
    r = np.arange(rods, dtype=np.float64)[None, :, None]
    amp = (1.0 - 0.35 * k) * np.where((k + r) % 2 == 0, 1.0, -1.0)            # (count, rods, 1)

    def s(width):
        return (np.arange(width, dtype=np.float64) + 0.5)[None, None, :] / width

    out = {}
    if "kappa" in fields:
        kap = np.zeros((count, rods, 3, w["kappa"]))
        kap[:, :, 1] = amp / length * (0.6 + 0.8 * s(w["kappa"]))             # integrates to amp: about a radian
        if not planar:
            kap[:, :, 0] = 0.4 * amp / length * np.sin(np.pi * s(w["kappa"]))
            kap[:, :, 2] = 0.3 * amp / length
        out["kappa"] = kap
    if planar:
        return out
    if "sigma" in fields:
        sig = np.zeros((count, rods, 3, w["sigma"]))
        sig[:, :, 0] = 0.01 * amp * s(w["sigma"])
        sig[:, :, 1] = -0.005 * amp
        sig[:, :, 2] = 0.02 * np.cos(2.0 * s(w["sigma"]) + k)
        out["sigma"] = sig
    if "velocity" in fields:
        vel = np.zeros((count, rods, 3, w["velocity"]))
        vel[:, :, 0] = 0.02 * amp * s(w["velocity"])
        vel[:, :, 1] = -0.01 * amp * s(w["velocity"]) ** 2
        out["velocity"] = vel
    if "omega" in fields:
        omg = np.zeros((count, rods, 3, w["omega"]))
        omg[:, :, 2] = 0.05 * amp * s(w["omega"])
        out["omega"] = omg
    return out


class Twin:
    """The hand-driven yardstick around a batch `env` made with autoreset=False and no pool."""

    def __init__(self, torch, env, fields, seed):
        self.torch, self.env, self.seed = torch, env, seed
        self.fields = {k: np.asarray(v, np.float64) for k, v in fields.items() if v is not None}
        self.count = next(iter(self.fields.values())).shape[0] if self.fields else 0
        n = env.num_envs
        self.episode = np.zeros(n, np.int64)          # j: resets since the stream was seeded
        self.index = np.full(n, -1, np.int64)         # the entry the current episode started from
        self.pending = np.zeros(n, bool)              # NEXT_STEP: finished on the previous call

    def _shape(self, mask):
        """reset(mask) has run: set_rod_shape(mask, pool[idx]) -> the observations."""
        env = self.env
        n = env.num_envs
        if not self.count:                            # no pool: straight starts, nothing counted
            return env.backend.observe(None)
        for e in np.nonzero(mask)[0]:
            self.index[e] = index(self.seed, e, self.episode[e], self.count)
            self.episode[e] += 1
        per_env = {}
        for name, v in self.fields.items():
            full = np.zeros((n,) + v.shape[1:])
            full[mask] = v[self.index[mask]]
            per_env[name] = full
        return env.set_rod_shape(mask, **per_env)

    def reset(self, seed=None, mask=None):
        n = self.env.num_envs
        m = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
        if seed is not None:
            self.episode[m] = 0
        self.env.reset(seed=seed, mask=mask)
        self.pending[m] = False
        return self._shape(m).clone()

    def step_same(self, a):
        """SAME_STEP by hand -> (obs, reward, terminated, truncated, done, final obs, clock before the reset, info)."""
        torch = self.torch
        o, r, te, tr, info = self.env.step(a)
        done = te | tr
        final = o.clone()
        clock = np.array(info["time"], np.float64)
        info = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in info.items()}
        r, te, tr = r.clone(), te.clone(), tr.clone()
        if bool(done.any()):
            m = done.cpu().numpy()
            self.env.reset(mask=m)
            robs = self._shape(m)
            o = torch.where(done[:, None], robs, final)
        else:
            o = final
        return o, r, te, tr, done, final, clock, info

    def step_next(self, a):
        """NEXT_STEP by hand, the composition VecRodEnvBase.step uses for the host-driven mode: an env that finished on
        the previous call restarts instead of stepping and reports its start's observation, reward 0 and clear flags
        -> (obs, reward, terminated, truncated, restarted)."""
        torch = self.torch
        env = self.env
        pending = self.pending.copy()
        saved = None
        if pending.any():
            saved = env.backend.prev_action_rows()[torch.from_numpy(pending)].clone()
        o, r, te, tr, _ = env.step(a)
        o, r, te, tr = o.clone(), r.clone(), te.clone(), tr.clone()
        if pending.any():
            env.backend.prev_action_rows()[torch.from_numpy(pending)] = saved
            env.reset(mask=pending)
            robs = self._shape(pending)
            pm = torch.from_numpy(pending).to(o.device)
            o = torch.where(pm[:, None], robs, o)
            r = torch.where(pm, torch.zeros_like(r), r)
            te = torch.where(pm, torch.zeros_like(te), te)
            tr = torch.where(pm, torch.zeros_like(tr), tr)
        self.pending = (te | tr).cpu().numpy().astype(bool)
        return o, r, te, tr, pending
