#!/usr/bin/env python3
"""Cost of observation and reward normalisation (set_normalization) on an env.step of autoreset="same_step", in one
process: three batches of the same build — one plain, one with the normalisation pass behind every step, one plain with
the same bookkeeping written as torch ops behind every step, what users do today — stepped in alternating windows with
device events around each window; each figure is the median over 7 windows (the method of tools/episode_stats_cost.py).
The pass's own kernel times are measured on the same handle with device events around 50 back-to-back calls, beside
what their bytes would need at the HBM's rate: the statistics kernel reads N * D * 4 bytes twice, the row kernel reads
and writes them once.  The queue top-ups are paused inside the windows and run between them, untimed.  The torch form
is a timing baseline only, never a test oracle: the kernels are tested against tests/normalize_ref.py.  What
profiles/normalize_cost.json records — a record, not a gate.

  python tools/normalize_cost.py [out.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402
from gym_softrobot_amd import _capi  # noqa: E402

WINDOWS, CALLS = 7, 24      # 24 calls use at most 24 of the 32 staged records per env
HBM_BYTES_PER_S = 8.0e12    # the MI355X's nominal HBM3E rate


class TorchNormalize:
    """VecNormalize's bookkeeping as torch ops on the env's stream, with no host read: the batch moments of the
    observation columns and of the discounted returns folded into running records (Gymnasium's
    update_mean_var_count_from_moments), the normalised observation, final observation and reward.  It does not mask
    non-finite rows and sums in torch's order: a timing baseline only."""

    def __init__(self, n, d, device, gamma=0.99, clip_obs=10.0, clip_reward=10.0, epsilon=1e-8):
        z = dict(device=device, dtype=torch.float64)
        self.n, self.gamma, self.clip_obs, self.clip_reward, self.epsilon = float(n), gamma, clip_obs, clip_reward, epsilon
        self.mean, self.var, self.count = torch.zeros(d, **z), torch.ones(d, **z), torch.full((), 1e-4, **z)
        self.rmean, self.rvar, self.rcount = torch.zeros((), **z), torch.ones((), **z), torch.full((), 1e-4, **z)
        self.ret = torch.zeros(n, **z)

    def _fold(self, mean, var, count, x):
        bv, bm = torch.var_mean(x, dim=0, unbiased=False)
        delta, tot = bm - mean, count + self.n
        m2 = var * count + bv * self.n + delta * delta * count * self.n / tot
        return mean + delta * self.n / tot, m2 / tot, tot

    def update(self, obs, reward, terminated, truncated, final_obs):
        x = obs.double()
        self.mean, self.var, self.count = self._fold(self.mean, self.var, self.count, x)
        inv = torch.rsqrt(self.var + self.epsilon)
        self.norm_obs = ((x - self.mean) * inv).clamp(-self.clip_obs, self.clip_obs).float()
        self.norm_final = ((final_obs.double() - self.mean) * inv).clamp(-self.clip_obs, self.clip_obs).float()
        self.ret = self.ret * self.gamma + reward
        self.rmean, self.rvar, self.rcount = self._fold(self.rmean, self.rvar, self.rcount, self.ret)
        self.norm_reward = (reward * torch.rsqrt(self.rvar + self.epsilon)).clamp(-self.clip_reward, self.clip_reward)
        self.ret = torch.where(terminated | truncated, torch.zeros_like(self.ret), self.ret)


def window(env, actions, book=None):
    env.top_up_paused = False
    env._top_up()                       # untimed; waits for the stream
    env.top_up_paused = True
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        _, r, te, tr, info = env.step(actions)
        if book is not None:
            book.update(env.backend.obs, r, te, tr, info["final_obs"])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def kernel_times(env, reps=50):
    """ms per call of the pass alone on the env's handle: (with the statistics kernel, the row kernel alone)."""
    be = env.backend
    out = []
    for update in (True, False):
        for timed in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                be.normalize_step(be.obs, be.reward, be.terminated, be.truncated, be.final_obs, 2, update)
            b.record()
            torch.cuda.synchronize()
            if timed:
                out.append(a.elapsed_time(b) / reps)
    return out[0], out[1]


def main():
    cases = []
    for env_id, n in (("SoftPendulum-v0", 4096), ("OctoFlat-v0", 1024)):
        plain, kernel, torched = (gsa.make_vec(env_id, n, autoreset="same_step") for _ in range(3))
        kernel.set_normalization()
        d = plain.obs_dim
        book = TorchNormalize(n, d, torched.backend.device)
        actions = torch.zeros((n, plain.action_dim), dtype=torch.float32, device=plain.backend.device)
        runs = ((plain, None), (kernel, None), (torched, book))
        for env, bk in runs:
            env.reset(seed=0)
            window(env, actions, bk)    # warm clock, code objects loaded
        ms = [[], [], []]
        for _ in range(WINDOWS):
            for out, (env, bk) in zip(ms, runs):
                out.append(window(env, actions, bk))
        med = [statistics.median(v) for v in ms]
        both, rows_only = kernel_times(kernel)
        nd4 = n * d * 4
        cases.append({"env": env_id, "n_envs": n, "obs_dim": d, "autoreset": "same_step",
                      "step_ms_plain": round(med[0], 5), "step_ms_plain_min_max": [round(min(ms[0]), 5), round(max(ms[0]), 5)],
                      "step_ms_with_pass": round(med[1], 5),
                      "step_ms_with_pass_min_max": [round(min(ms[1]), 5), round(max(ms[1]), 5)],
                      "step_ms_with_torch_form": round(med[2], 5),
                      "step_ms_with_torch_form_min_max": [round(min(ms[2]), 5), round(max(ms[2]), 5)],
                      "pass_cost_ms": round(med[1] - med[0], 5), "torch_form_cost_ms": round(med[2] - med[0], 5),
                      "pass_alone_ms": round(both, 5), "row_kernel_alone_ms": round(rows_only, 5),
                      "stats_kernel_alone_ms": round(both - rows_only, 5),
                      "stats_kernel_bytes": 2 * nd4, "stats_kernel_ms_at_hbm_rate": round(2 * nd4 / HBM_BYTES_PER_S * 1e3, 6),
                      "row_kernel_bytes": 2 * nd4, "row_kernel_ms_at_hbm_rate": round(2 * nd4 / HBM_BYTES_PER_S * 1e3, 6)})
        for env in (plain, kernel, torched):
            env.close()
    doc = {"method": "three batches per case on the same build in one process: plain, with set_normalization() (the statistics "
                     "kernel and the row kernel behind every step), and plain with the same bookkeeping as torch ops behind "
                     f"every step; one warm-up window each, then {WINDOWS} alternating windows of {CALLS} env.step calls with "
                     "resident zero actions, device events around each window (launches included), the reset queue topped up "
                     "between the windows, untimed; per-call time = window / calls, median over the windows; cost = with - "
                     "plain.  pass_alone_ms / row_kernel_alone_ms: 50 back-to-back softrod_normalize_step calls on the resident "
                     "outputs with update 1 / 0 between two device events, after 50 untimed ones; the statistics kernel is "
                     "their difference.  *_ms_at_hbm_rate: the bytes at 8 TB/s",
           "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
           "library_source_hash": _capi.library_source_hash(), "cases": cases,
           "note": "the statistics kernel runs ceil(obs_dim / 64) + 1 workgroups of 16 waves, each walking all n_envs rows "
                   "twice in a fixed order: it is bound by the latency of its row loads, not by bandwidth, which is why a wave "
                   "keeps 32 row loads in flight.  pass_alone_ms and its two parts include the launches' issue from Python, back "
                   "to back, so they are upper bounds of the kernel times; pass_cost_ms is what a step pays.  The torch form is "
                   "a timing baseline only (a few dozen small launches per step), not a test oracle"}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
