#!/usr/bin/env python3
"""Cost of joint_loads() beside rod_energies() on the same handle, in one process: median of 20 calls after 5 warm-up
calls, device events around each call.  What profiles/joint_loads_cost.json records.

  python tools/joint_loads_cost.py [out.json]
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
for env_id, n in (("OctoFlat-v0", 1024), ("OctoCrawl-v0", 1024)):
    env = gsa.make_vec(env_id, n)
    env.reset(seed=0)
    zero = np.zeros((n, env.action_dim), np.float32)
    for _ in range(2):
        env.step(zero)
    be = env.backend
    rods = _capi.config_rods_per_env(env.cfg)
    cases.append({"env": env_id, "n_envs": n, "rods_per_env": rods, "n_elem": int(env.cfg.n_elem),
                  "joint_loads_ms": round(timed(be.joint_loads), 5), "rod_energies_ms": round(timed(be.rod_energies), 5),
                  "out_bytes": n * (rods + 1) * 16 * 8})
    env.close()
doc = {"method": "median of 20 calls after 5 warm-up calls, device events around each call (launch included), after "
                 "reset(seed=0) and 2 env.steps of zero actions",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0), "cases": cases,
       "note": "rod_energies() on the same handle, in the same process, is the yardstick"}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
