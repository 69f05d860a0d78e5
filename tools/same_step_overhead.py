#!/usr/bin/env python3
"""What autoreset="same_step" costs and buys against autoreset="device" (NEXT_STEP), on one build.

SoftPendulum-v0 at 4096 envs, one batch per case in ONE process, stepped with zero actions.  The auto-reset passes lie
outside the device events of softrod_set_timing on purpose (kernel_times_ms means the step), so everything here is a
host clock around a window of env.steps that ends in a device synchronise: the whole call, pass, top-ups and launch
overhead included.  The clock is pre-heated (--warmup steps per batch), the cases alternate window by window, and each
figure is the median of --windows windows.

  * full_episodes: per-step time at the env's own episode length (125 steps); both modes restart envs inside the windows;
  * short_episodes (3 steps: final_time 0.1): the useful env-steps per second of both modes, counting only calls in
    which an env stepped — under NEXT_STEP every fourth call of an env is its reset, under SAME_STEP none is;
  * top_up_deadline: full episodes again with `top_up_every` forced to 15 and to 30 in BOTH modes (an env there uses a
    record per 125 steps, so either is safe): separates what the pass costs from what same_step's halved deadline costs.

Prints one JSON object per part and writes them all to --out.

    python tools/same_step_overhead.py [--windows 5] [--steps 1500] [--out profiles/same_step_overhead.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import gym_softrobot_amd as gsa  # noqa: E402

ENV_ID, N_ENVS = "SoftPendulum-v0", 4096


def _make(mode, every, kw):
    env = gsa.make_vec(ENV_ID, N_ENVS, autoreset=mode, **kw)
    if every is not None:                                   # the deadline as an experiment's knob: this batch only
        env.__class__ = type(type(env).__name__, (type(env),), {"top_up_every": property(lambda self: every)})
    return env


def _window(env, a, k):
    """k env.steps -> (seconds, staged records the envs used meanwhile)."""
    before = int(env.backend.queue_status()[0].sum())          # (synchronises)
    t0 = time.perf_counter()
    for _ in range(k):
        env.step(a)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, int(env.backend.queue_status()[0].sum()) - before


def _measure(cases, kw, steps, windows, warmup):
    """cases: {label: (mode, forced top_up_every or None)} -> {label: figures}."""
    envs = {c: _make(m, every, kw) for c, (m, every) in cases.items()}
    a = torch.zeros((N_ENVS, 1), dtype=torch.float32, device="cuda")
    for e in envs.values():
        e.reset(seed=0)
        for _ in range(warmup):
            e.step(a)
    torch.cuda.synchronize()
    raw = {c: [] for c in cases}
    order = list(cases)
    for w in range(windows):
        for c in (order if w % 2 == 0 else order[::-1]):
            raw[c].append(_window(envs[c], a, steps))
    out = {}
    for c, (mode, _) in cases.items():
        ms = np.array([1e3 * dt / steps for dt, _ in raw[c]])
        # a call in which an env consumed a record under NEXT_STEP is that env's reset call; under SAME_STEP it stepped
        useful = np.array([(N_ENVS * steps - (used if mode == "device" else 0)) / dt for dt, used in raw[c]])
        env = envs[c]
        env.backend.set_timing(200)                         # the step kernel alone, by device events
        for _ in range(200):
            env.step(a)
        torch.cuda.synchronize()
        out[c] = {"top_up_every": env.top_up_every,
                  "step_ms_median": float(np.median(ms)), "step_ms_min": float(ms.min()), "step_ms_max": float(ms.max()),
                  "window_step_ms": [round(x, 5) for x in ms.tolist()],
                  "step_kernel_ms_median": float(np.median(env.backend.kernel_times_ms())),
                  "restarts_per_window": [used for _, used in raw[c]],
                  "useful_env_steps_per_s_median": float(np.median(useful)),
                  "window_useful_env_steps_per_s": [round(x) for x in useful.tolist()]}
        assert env.backend.queue_status()[1] == 0, "a window ran out of staged records"
        env.close()
    return out


def _compare(out, d="device", s="same_step"):
    d, s = out[d], out[s]
    return {"step_ms_ratio": s["step_ms_median"] / d["step_ms_median"],
            "device_window_spread_frac": (d["step_ms_max"] - d["step_ms_min"]) / d["step_ms_median"],
            "same_step_within_device_spread": bool(d["step_ms_min"] <= s["step_ms_median"] <= d["step_ms_max"]),
            "useful_rate_ratio": s["useful_env_steps_per_s_median"] / d["useful_env_steps_per_s_median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1500, help="env.steps per window")
    ap.add_argument("--warmup", type=int, default=400, help="env.steps per batch before the first window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    modes = {"device": ("device", None), "same_step": ("same_step", None)}
    forced = {f"{m}@{e}": (m, e) for m in ("device", "same_step") for e in (15, 30)}
    results = []
    for name, cases, kw, length in (("full_episodes", modes, {}, 125), ("short_episodes", modes, {"final_time": 0.1}, 3),
                                    ("top_up_deadline", forced, {}, 125)):
        rec = {"part": name, "env": ENV_ID, "n_envs": N_ENVS, "episode_steps": length, "steps_per_window": args.steps,
               "windows": args.windows, "expected_useful_rate_ratio": (length + 1) / length}
        rec.update(_measure(cases, kw, args.steps, args.windows, args.warmup))
        if cases is modes:
            rec.update(_compare(rec))
        else:
            rec["at_deadline_30"] = _compare(rec, "device@30", "same_step@30")
            rec["at_deadline_15"] = _compare(rec, "device@15", "same_step@15")
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0), "library_source_hash": gsa._capi.library_source_hash(),
               "method": "host clock around `steps` env.steps ending in a device synchronise (the auto-reset passes lie "
                         "outside softrod_set_timing's events); clock pre-heated; the cases alternate window by "
                         "window in one process; medians over the windows; useful env-steps exclude the calls an env "
                         "spends resetting under NEXT_STEP; step_kernel_ms: device events around the step alone",
               "results": results}
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
