"""NumPy twin of softrod_episode_stats_kernel (gym_softrobot_amd/csrc/softrod_episode_stats.hpp): the same arrays, the
update written as a plain loop over the envs in index order with sequential ring pushes.  Every comparison against it is
bitwise: a return is a sequence of float64 adds in call order and nothing else is floating-point arithmetic."""
import numpy as np

MANUAL, NEXT_STEP, SAME_STEP = 0, 1, 2

# every resident array, by the name the backend's `episode_stats` views carry
ARRAYS = ("acc_return", "acc_length", "latch", "finished", "ep_r", "ep_l", "ep_t", "ep_mask",
          "ring_r", "ring_l", "ring_t", "ring_env")


class EpisodeStatsRef:
    def __init__(self, n_envs: int, ring: int):
        n, k = int(n_envs), int(ring)
        self.n_envs, self.ring = n, k
        self.acc_return = np.zeros(n, np.float64)
        self.acc_length = np.zeros(n, np.int32)
        self.latch = np.zeros(n, np.uint8)
        self.finished = np.zeros(n, np.int32)
        self.ep_r = np.zeros(n, np.float64)
        self.ep_l = np.zeros(n, np.int32)
        self.ep_t = np.zeros(n, np.float64)
        self.ep_mask = np.zeros(n, np.uint8)
        self.ring_r = np.zeros(k, np.float64)
        self.ring_l = np.zeros(k, np.int32)
        self.ring_t = np.zeros(k, np.float64)
        self.ring_env = np.zeros(k, np.int32)
        self.count = 0

    def _rows(self, e, r=0.0, l=0, t=0.0, m=0):
        self.ep_r[e], self.ep_l[e], self.ep_t[e], self.ep_mask[e] = r, l, t, m

    def update(self, reward, terminated, truncated, end_time, mode: int) -> None:
        reward = np.asarray(reward, np.float64)
        done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
        for e in range(self.n_envs):
            if self.latch[e]:                   # the env finished on an earlier call
                self._rows(e)
                if mode == NEXT_STEP:
                    self.latch[e] = 0           # this call was its reset call
                continue
            self.acc_return[e] = self.acc_return[e] + reward[e]
            self.acc_length[e] += 1
            if done[e]:
                t = 0.0 if end_time is None else float(end_time[e])
                self._rows(e, self.acc_return[e], self.acc_length[e], t, 1)
                slot = self.count % self.ring   # a sequential push
                self.ring_r[slot], self.ring_l[slot] = self.acc_return[e], self.acc_length[e]
                self.ring_t[slot], self.ring_env[slot] = t, e
                self.count += 1
                self.finished[e] += 1
                self.acc_return[e] = 0.0
                self.acc_length[e] = 0
                self.latch[e] = 1 if mode != SAME_STEP else 0
            else:
                self._rows(e)

    def reset(self, mask=None) -> None:
        sel = np.ones(self.n_envs, bool) if mask is None else np.asarray(mask).astype(bool)
        for a in (self.acc_return, self.acc_length, self.latch, self.ep_r, self.ep_l, self.ep_t, self.ep_mask):
            a[sel] = 0

    def recent(self):
        """(returns, lengths, times, envs) of the last min(count, ring) episodes, oldest first."""
        order = np.arange(max(0, self.count - self.ring), self.count) % self.ring
        return self.ring_r[order], self.ring_l[order], self.ring_t[order], self.ring_env[order]
