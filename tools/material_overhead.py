#!/usr/bin/env python3
"""Step time of per-env material (set_material, the kFeatEnvMaterial step kernels) against the uniform kernel.

For each of SoftPendulum-v0, SoftPendulum3D-v0 and OctoArmSingle-v0: two batches of N envs in ONE process, one
uniform and one with E, rho, nu drawn per env across x0.5 .. x2, stepped alternately with zero actions; after the
warm-up every env.step is timed with device events on the launch stream (softrod_set_timing: the step kernel alone).
Prints one JSON object per env and writes them all to --out.

    python tools/material_overhead.py [--envs 4096] [--rounds 8] [--steps 20] [--out profiles/material_overhead.json]

A kernel trace is a run of its own (never together with PMC counters):

    rocprofv3 --kernel-trace --stats -d <dir> -o trace --output-format csv -- python3 tools/material_overhead.py --rounds 2
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

ENVS = ["SoftPendulum-v0", "SoftPendulum3D-v0", "OctoArmSingle-v0"]


def _timed_steps(env, a, k):
    env.backend.set_timing(k)
    for _ in range(k):
        env.step(a)
    torch.cuda.synchronize()
    return list(env.backend.kernel_times_ms())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=8, help="alternations uniform / per-env material")
    ap.add_argument("--steps", type=int, default=20, help="timed env.steps per batch and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.envs
    results = []
    for env_id in ENVS:
        uni, mat = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
        c = mat.cfg
        rng = np.random.default_rng(0)
        mat.set_material(youngs_modulus=c.youngs_modulus * 2.0 ** rng.uniform(-1, 1, n),
                         density=c.density * 2.0 ** rng.uniform(-1, 1, n),
                         damping_constant=c.damping_constant * 2.0 ** rng.uniform(-1, 1, n))
        a = torch.zeros((n, uni.action_dim), dtype=torch.float32, device="cuda")
        times = {"uniform": [], "env_material": []}
        for e in (uni, mat):
            e.reset(seed=0)
            for _ in range(args.warmup):
                e.step(a)
        torch.cuda.synchronize()
        for r in range(args.rounds):
            order = (("uniform", uni), ("env_material", mat)) if r % 2 == 0 else (("env_material", mat), ("uniform", uni))
            for name, e in order:
                e.reset(seed=r + 1)                 # every window from a fresh episode: the same physics each round
                times[name].append(float(np.median(_timed_steps(e, a, args.steps))))
        rec = {"env": env_id, "n_envs": n, "steps_per_window": args.steps, "windows": args.rounds,
               "kernel_tier": {"uniform": uni.backend.kernel_tier(), "env_material": mat.backend.kernel_tier()}}
        for name, t in times.items():
            t = np.array(t)
            rec[name] = {"step_ms_median": float(np.median(t)), "step_ms_min": float(t.min()),
                         "step_ms_max": float(t.max()), "window_medians_ms": [round(x, 5) for x in t.tolist()]}
        rec["overhead_frac"] = rec["env_material"]["step_ms_median"] / rec["uniform"]["step_ms_median"] - 1.0
        print(json.dumps(rec), flush=True)
        results.append(rec)
        uni.close()
        mat.close()
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "library_source_hash": gsa._capi.library_source_hash(),
               "method": "device events around each step kernel (softrod_set_timing); per window the median of "
                         "`steps` env.steps from a fresh reset; uniform and per-env-material batches alternate "
                         "in one process", "results": results}
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
