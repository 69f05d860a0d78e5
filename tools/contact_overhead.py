#!/usr/bin/env python3
"""Step time of per-env contact (set_contact, the kFeatEnvContact step kernels) against the uniform kernel.

OctoArmSingle-v0 at 4096 envs in both math modes and OctoFlat-v0 at 1024 envs: two batches in ONE process, one
uniform and one with k, nu drawn per env across x0.5 .. x2 and friction multipliers across x0.25 .. x4 (symmetric or
not), stepped alternately with zero actions; after the warm-up every env.step is timed with device events on the
launch stream (softrod_set_timing: the step kernel alone).  Prints one JSON object per workload and writes them all
to --out.

    python tools/contact_overhead.py [--rounds 8] [--steps 20] [--out profiles/contact_overhead.json]

A kernel trace is a run of its own (never together with PMC counters):

    rocprofv3 --kernel-trace --stats -d <dir> -o trace --output-format csv -- python3 tools/contact_overhead.py --rounds 2
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import gym_softrobot_amd as gsa  # noqa: E402
from gym_softrobot_amd import _capi  # noqa: E402

# (env id, envs, math mode, timed env.steps per window; OctoFlat's step is 2857 substeps of 8 arms)
WORKLOADS = [("OctoArmSingle-v0", 4096, _capi.MATH_FAST, 20), ("OctoArmSingle-v0", 4096, _capi.MATH_LIBM, 4),
             ("OctoFlat-v0", 1024, _capi.MATH_FAST, 4)]


def _timed_steps(env, a, k):
    env.backend.set_timing(k)
    for _ in range(k):
        env.step(a)
    torch.cuda.synchronize()
    return list(env.backend.kernel_times_ms())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8, help="alternations uniform / per-env contact")
    ap.add_argument("--steps", type=int, default=None, help="timed env.steps per batch and round (default: per workload)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    for env_id, n, mode, steps in WORKLOADS:
        steps = args.steps or steps
        uni, con = gsa.make_vec(env_id, n, math_mode=mode), gsa.make_vec(env_id, n, math_mode=mode)
        c = con.cfg
        rng = np.random.default_rng(0)
        con.set_contact(contact_k=c.contact_k * 2.0 ** rng.uniform(-1, 1, n),
                        contact_nu=c.contact_nu * 2.0 ** rng.uniform(-1, 1, n),
                        friction_multiplier=2.0 ** rng.uniform(-2, 2, n), friction_symmetry=rng.random(n) < 0.5)
        a = torch.zeros((n, uni.action_dim), dtype=torch.float32, device="cuda")
        times = {"uniform": [], "env_contact": []}
        for e in (uni, con):
            e.reset(seed=0)
            for _ in range(args.warmup):
                e.step(a)
        torch.cuda.synchronize()
        for r in range(args.rounds):
            order = (("uniform", uni), ("env_contact", con)) if r % 2 == 0 else (("env_contact", con), ("uniform", uni))
            for name, e in order:
                e.reset(seed=r + 1)                 # every window from a fresh episode: the same physics each round
                times[name].append(float(np.median(_timed_steps(e, a, steps))))
        rec = {"env": env_id, "n_envs": n, "math_mode": "fast" if mode == _capi.MATH_FAST else "libm",
               "steps_per_window": steps, "windows": args.rounds,
               "kernel_tier": {"uniform": uni.backend.kernel_tier(), "env_contact": con.backend.kernel_tier()}}
        for name, t in times.items():
            t = np.array(t)
            rec[name] = {"step_ms_median": float(np.median(t)), "step_ms_min": float(t.min()),
                         "step_ms_max": float(t.max()), "window_medians_ms": [round(x, 5) for x in t.tolist()]}
        rec["overhead_frac"] = rec["env_contact"]["step_ms_median"] / rec["uniform"]["step_ms_median"] - 1.0
        print(json.dumps(rec), flush=True)
        results.append(rec)
        uni.close()
        con.close()
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "library_source_hash": gsa._capi.library_source_hash(),
               "method": "device events around each step kernel (softrod_set_timing); per window the median of "
                         "`steps` env.steps from a fresh reset; uniform and per-env-contact batches alternate "
                         "in one process", "results": results}
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
