"""NumPy twin of the normalisation kernels (gym_softrobot_amd/csrc/softrod_normalize.hpp): the same arrays, the same
row rules, and every sum in the kernel's fixed order — partial p of 16 adds the rows e = p, p + 16, ... in ascending e
from +0.0, the partials are then added in ascending p from +0.0, each add one float64 rounding (np.add.accumulate is
sequential; np.sum is pairwise and is never used).  Every comparison against it is bitwise."""
import numpy as np

MANUAL, NEXT_STEP, SAME_STEP = 0, 1, 2
PARTIALS = 16
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
NAN64 = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]

# every resident array, by the name the backend's `normalize` views carry
ARRAYS = ("obs_mean", "obs_var", "obs_count", "obs_inv_std", "ret_mean", "ret_var", "ret_count", "ret_inv_std",
          "ret", "latch", "norm_obs", "norm_reward")


def osum(values):
    """The fixed-order sum of the rows of `values` (N,) or (N, D), float64."""
    v = np.asarray(values, np.float64)
    zero = np.zeros((1,) + v.shape[1:])
    parts = [np.add.accumulate(np.concatenate([zero, v[p::PARTIALS]]), axis=0)[-1] for p in range(PARTIALS)]
    return np.add.accumulate(np.concatenate([zero, np.stack(parts)]), axis=0)[-1]


def column_update(mean, var, count, x, counted, epsilon):
    """One update of the records (mean, var, count), each (D,), from x (N, D) with the row weights `counted` (N,):
    returns the new (mean, var, count, inv_std or None where the column keeps its record)."""
    x = np.asarray(x, np.float64)
    c = np.asarray(counted, bool)[:, None] & np.isfinite(x)
    n = c.sum(axis=0)
    dn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        bm = osum(np.where(c, x, 0.0)) / dn
        dev = x - bm
        bv = osum(np.where(c, dev * dev, 0.0)) / dn
        delta = bm - mean
        tot = count + dn
        mean1 = mean + (delta * dn) / tot
        m2 = ((var * count) + (bv * dn)) + ((((delta * delta) * count) * dn) / tot)
        var1 = m2 / tot
        inv1 = 1.0 / np.sqrt(var1 + epsilon)
    keep = n == 0
    return np.where(keep, mean, mean1), np.where(keep, var, var1), np.where(keep, count, tot), inv1, keep


class NormalizeRef:
    def __init__(self, n_envs, obs_dim, obs_on=True, reward_on=True, gamma=0.99, clip_obs=10.0, clip_reward=10.0,
                 epsilon=1e-8):
        n, d = int(n_envs), int(obs_dim)
        self.n_envs, self.obs_dim = n, d
        self.obs_on, self.reward_on = bool(obs_on), bool(reward_on)
        self.gamma, self.clip_obs, self.clip_reward, self.epsilon = float(gamma), float(clip_obs), float(clip_reward), float(epsilon)
        self.obs_mean, self.obs_var, self.obs_count = np.zeros(d), np.ones(d), np.full(d, 1e-4)
        self.obs_inv_std = 1.0 / np.sqrt(self.obs_var + self.epsilon)
        self.ret_mean, self.ret_var, self.ret_count = np.zeros(1), np.ones(1), np.full(1, 1e-4)
        self.ret_inv_std = 1.0 / np.sqrt(self.ret_var + self.epsilon)
        self.ret = np.zeros(n)
        self.latch = np.zeros(n, np.uint8)
        self.norm_obs = np.zeros((n, d), np.float32)
        self.norm_final_obs = np.zeros((n, d), np.float32)
        self.norm_reward = np.zeros(n)

    def _update_obs(self, obs, counted):
        m, v, c, inv, keep = column_update(self.obs_mean, self.obs_var, self.obs_count, obs, counted, self.epsilon)
        self.obs_mean, self.obs_var, self.obs_count = m, v, c
        self.obs_inv_std = np.where(keep, self.obs_inv_std, inv)

    def _norm_rows(self, obs):
        with np.errstate(all="ignore"):
            v = (np.asarray(obs, np.float32).astype(np.float64) - self.obs_mean) * self.obs_inv_std
            out = np.clip(v, -self.clip_obs, self.clip_obs).astype(np.float32)
        out[np.isnan(v)] = NAN32
        return out

    def step(self, obs, reward, terminated, truncated, final_obs=None, mode=MANUAL, update=True):
        """One softrod_normalize_step.  Returns the bool rows that finished on this call (the rows of norm_final_obs
        this call wrote when `final_obs` is given)."""
        obs = np.asarray(obs, np.float32).reshape(self.n_envs, self.obs_dim)
        reward = np.asarray(reward, np.float64).reshape(self.n_envs)
        done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
        open_ = self.latch == 0                         # the latch as the call found it
        finished = open_ & done
        if update:
            if self.obs_on:
                self._update_obs(obs, open_ if mode == MANUAL else np.ones(self.n_envs, bool))
            if self.reward_on:
                with np.errstate(all="ignore"):
                    self.ret = np.where(open_, (self.ret * self.gamma) + reward, self.ret)
                m, v, c, inv, keep = column_update(self.ret_mean, self.ret_var, self.ret_count, self.ret[:, None], open_,
                                                   self.epsilon)
                self.ret_mean, self.ret_var, self.ret_count = m, v, c
                self.ret_inv_std = np.where(keep, self.ret_inv_std, inv)
        if self.obs_on:
            self.norm_obs = self._norm_rows(obs)
            if final_obs is not None:
                rows = self._norm_rows(np.asarray(final_obs, np.float32).reshape(self.n_envs, self.obs_dim))
                self.norm_final_obs[finished] = rows[finished]
        if self.reward_on:
            with np.errstate(all="ignore"):
                v = reward * self.ret_inv_std[0]
                self.norm_reward = np.clip(v, -self.clip_reward, self.clip_reward)
            self.norm_reward[np.isnan(v)] = NAN64
        if update:
            self.ret[finished] = 0.0
            if mode == NEXT_STEP:
                self.latch[~open_] = 0
            self.latch[finished] = 1 if mode != SAME_STEP else 0
        return finished

    def reset(self, obs, mask=None, update=True):
        obs = np.asarray(obs, np.float32).reshape(self.n_envs, self.obs_dim)
        sel = np.ones(self.n_envs, bool) if mask is None else np.asarray(mask).astype(bool).reshape(self.n_envs)
        if self.obs_on:
            if update:
                self._update_obs(obs, sel)
            self.norm_obs = self._norm_rows(obs)
        self.ret[sel] = 0.0
        self.latch[sel] = 0

    def load(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count):
        self.obs_mean, self.obs_var, self.obs_count = (np.array(v, np.float64).reshape(self.obs_dim)
                                                       for v in (obs_mean, obs_var, obs_count))
        self.ret_mean, self.ret_var, self.ret_count = (np.array(v, np.float64).reshape(1) for v in (ret_mean, ret_var, ret_count))
        self.obs_inv_std = 1.0 / np.sqrt(self.obs_var + self.epsilon)
        self.ret_inv_std = 1.0 / np.sqrt(self.ret_var + self.epsilon)
