#!/usr/bin/env python3
"""Cost of rod_dynamics() beside ground_reaction() (the contact envs) or muscle_loads() (the muscle arm) on the same
handle, in one process: median of 20 calls after 5 warm-up calls, device events around each call.  What
profiles/rod_dynamics_cost.json records.

  python tools/rod_dynamics_cost.py [out.json]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402
from gym_softrobot_amd import _capi  # noqa: E402


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


cases = []
for env_id, n, beside in (("OctoArmSingle-v0", 4096, "ground_reaction"), ("OctoFlat-v0", 1024, "ground_reaction"),
                          ("OctoArmPush-v1", 4096, "muscle_loads")):
    env = gsa.make_vec(env_id, n)
    env.reset(seed=0)
    zero = np.zeros((n, env.action_dim), np.float32)
    for _ in range(2):
        env.step(zero)
    be = env.backend
    rods, ne = _capi.config_rods_per_env(env.cfg), int(env.cfg.n_elem)
    rows = {"ground_reaction": 6, "muscle_loads": 20}[beside]
    cases.append({"env": env_id, "n_envs": n, "rods_per_env": rods, "n_elem": ne,
                  "rod_dynamics_ms": round(timed(be.rod_dynamics), 5), beside + "_ms": round(timed(getattr(be, beside)), 5),
                  "out_bytes": n * rods * 18 * (ne + 1) * 8, beside + "_out_bytes": n * rods * rows * (ne + 1) * 8})
    env.close()
doc = {"method": "median of 20 calls after 5 warm-up calls, device events around each call (launch included), after "
                 "reset(seed=0) and 2 env.steps of zero actions",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
       "library_source_hash": _capi.library_source_hash(), "cases": cases,
       "note": "the other read-out on the same handle, in the same process, is the yardstick"}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
