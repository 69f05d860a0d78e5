#!/usr/bin/env python3
"""Cost of the episode statistics (record_episode_statistics) on an env.step of autoreset="same_step", in one process:
three batches of the same build — one plain, one with the statistics kernel behind every step, one plain with the same
bookkeeping written as torch ops behind every step — stepped in alternating windows with device events around each
window; each figure is the median over 7 windows (the method of tools/reset_shapes_cost.py).  Two regimes for
SoftPendulum-v0: the default episode length, where almost no env finishes, and an episode end on every call
(final_time below one env.step), where every env pushes on the ring every call.  The queue top-ups are paused inside
the windows and run between them, untimed.  The torch form is a timing baseline only, never a test oracle: the kernel
is tested against tests/episode_stats_ref.py.  What profiles/episode_stats_cost.json records — a record, not a gate.

  python tools/episode_stats_cost.py [out.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402
from gym_softrobot_amd import _capi  # noqa: E402

WINDOWS, CALLS, RING = 7, 24, 100       # 24 calls use at most 24 of the 32 staged records per env


class TorchEpisodeStats:
    """The SAME_STEP bookkeeping of softrod_episode_stats_kernel as torch ops on the env's stream, with no host read:
    accumulators, info rows, the deterministic ring push (rank by cumsum; the envs without a slot write a spare slot
    behind the ring) and the counters.  No latch: SAME_STEP never sets one."""

    def __init__(self, n, ring, device):
        z = dict(device=device)
        self.ring = ring
        self.acc_r, self.acc_l = torch.zeros(n, dtype=torch.float64, **z), torch.zeros(n, dtype=torch.int32, **z)
        self.finished = torch.zeros(n, dtype=torch.int32, **z)
        self.ring_r, self.ring_t = torch.zeros(ring + 1, dtype=torch.float64, **z), torch.zeros(ring + 1, dtype=torch.float64, **z)
        self.ring_l, self.ring_e = torch.zeros(ring + 1, dtype=torch.int32, **z), torch.zeros(ring + 1, dtype=torch.int32, **z)
        self.count = torch.zeros((), dtype=torch.int64, **z)
        self.envs = torch.arange(n, dtype=torch.int32, **z)
        self.zero_r, self.zero_l = torch.zeros(n, dtype=torch.float64, **z), torch.zeros(n, dtype=torch.int32, **z)
        self.spare = torch.full((n,), ring, dtype=torch.int64, **z)

    def update(self, reward, terminated, truncated, end_time):
        done = terminated | truncated
        self.acc_r += reward
        self.acc_l += 1
        self.ep_r = torch.where(done, self.acc_r, self.zero_r)
        self.ep_l = torch.where(done, self.acc_l, self.zero_l)
        self.ep_t = torch.where(done, end_time, self.zero_r)
        self.ep_mask = done
        rank = torch.cumsum(done, 0) - 1
        total = rank[-1] + 1
        writes = done & (rank >= total - self.ring)
        slot = torch.where(writes, (self.count + rank) % self.ring, self.spare)
        self.ring_r.scatter_(0, slot, self.ep_r)
        self.ring_l.scatter_(0, slot, self.ep_l)
        self.ring_t.scatter_(0, slot, self.ep_t)
        self.ring_e.scatter_(0, slot, self.envs)
        self.count += total
        self.finished += done
        self.acc_r = torch.where(done, self.zero_r, self.acc_r)
        self.acc_l = torch.where(done, self.zero_l, self.acc_l)


def window(env, actions, book=None):
    env.top_up_paused = False
    env._top_up()                       # untimed; waits for the stream
    env.top_up_paused = True
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        _, r, te, tr, info = env.step(actions)
        if book is not None:
            book.update(r, te, tr, info["final_info"]["time"])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def main():
    cases = []
    for env_id, n, regime, kw in (("SoftPendulum-v0", 4096, "default episode length", {}),
                                  ("SoftPendulum-v0", 4096, "an episode end on every call", dict(final_time=1e-6)),
                                  ("OctoFlat-v0", 1024, "default episode length", {})):
        plain, kernel, torched = (gsa.make_vec(env_id, n, autoreset="same_step", **kw) for _ in range(3))
        kernel.record_episode_statistics(RING)
        book = TorchEpisodeStats(n, RING, torched.backend.device)
        actions = torch.zeros((n, plain.action_dim), dtype=torch.float32, device=plain.backend.device)
        runs = ((plain, None), (kernel, None), (torched, book))
        for env, bk in runs:
            env.reset(seed=0)
            window(env, actions, bk)    # warm clock, code objects loaded
        ms = [[], [], []]
        for _ in range(WINDOWS):
            for out, (env, bk) in zip(ms, runs):
                out.append(window(env, actions, bk))
        stats = kernel.episode_statistics()
        per_call = stats.count / ((WINDOWS + 1) * CALLS * n)
        assert stats.count == int(book.count), (stats.count, int(book.count))       # the two forms saw the same episodes
        med = [statistics.median(v) for v in ms]
        cases.append({"env": env_id, "n_envs": n, "autoreset": "same_step", "regime": regime, "ring": RING,
                      "episodes_finished_per_env_call": round(per_call, 4),
                      "step_ms_plain": round(med[0], 5), "step_ms_plain_min_max": [round(min(ms[0]), 5), round(max(ms[0]), 5)],
                      "step_ms_with_kernel": round(med[1], 5),
                      "step_ms_with_kernel_min_max": [round(min(ms[1]), 5), round(max(ms[1]), 5)],
                      "step_ms_with_torch_form": round(med[2], 5),
                      "step_ms_with_torch_form_min_max": [round(min(ms[2]), 5), round(max(ms[2]), 5)],
                      "kernel_cost_ms": round(med[1] - med[0], 5), "torch_form_cost_ms": round(med[2] - med[0], 5)})
        for env in (plain, kernel, torched):
            env.close()
    doc = {"method": f"three batches per case on the same build in one process: plain, with record_episode_statistics({RING}) (one "
                     "softrod_episode_stats_kernel launch behind every step), and plain with the same bookkeeping as torch ops "
                     f"behind every step; one warm-up window each, then {WINDOWS} alternating windows of {CALLS} env.step calls with "
                     "resident zero actions, device events around each window (launches included), the reset queue topped up "
                     "between the windows, untimed; per-call time = window / calls, median over the windows; cost = with - plain",
           "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
           "library_source_hash": _capi.library_source_hash(), "cases": cases,
           "note": "the kernel is one workgroup of 1024 threads that walks the envs in chunks of 1024, twice: its time grows with "
                   "ceil(n_envs / 1024).  The torch form is a timing baseline only (about twenty small launches per step), "
                   "not a test oracle"}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
