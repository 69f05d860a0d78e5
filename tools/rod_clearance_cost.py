#!/usr/bin/env python3
"""Cost of rod_clearance() beside the step kernel of the same handle, in one process: the clock is warmed with the
handle's own steps, then each figure is the median over 7 windows of back-to-back calls with device events around each
window (launches included), the two kinds of window alternating.  What profiles/rod_clearance_cost.json records.

  python tools/rod_clearance_cost.py [out.json]
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

WINDOWS = 7


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


cases = []
for env_id, n, kw in (("OctoFlat-v0", 1024, {}), ("OctoReach-v0", 1024, {}), ("OctoArmSingle-v0", 4096, {}),
                      ("OctoArmPush-v1", 4096, dict(n_elems=100))):
    env = gsa.make_vec(env_id, n, **kw)
    env.reset(seed=0)
    be = env.backend
    actions = torch.zeros((n, env.action_dim), dtype=torch.float32, device=be.device)
    step = lambda: be.step(actions)          # noqa: E731
    clearance = lambda: be.rod_clearance()   # noqa: E731
    for _ in range(30):                      # warm clock, code objects loaded, the read-out's buffer allocated
        step()
        clearance()
    torch.cuda.synchronize()
    step_ms, clearance_ms = [], []
    for _ in range(WINDOWS):
        step_ms.append(window(step, 10))
        clearance_ms.append(window(clearance, 50))
    rods, ne = _capi.config_rods_per_env(env.cfg), int(env.cfg.n_elem)
    s, c = statistics.median(step_ms), statistics.median(clearance_ms)
    prof = be._tables.get("radius_profile")
    radii = float(env.cfg.base_radius) if prof is None else np.frombuffer(prof, np.float64)
    cases.append({"env": env_id, "n_envs": n, "rods_per_env": rods, "n_elem": ne,
                  "self_gap": _capi.rod_clearance_self_gap(float(env.cfg.base_length) / ne, radii),
                  "waves": n * (rods * (rods + 1) // 2 + rods),
                  "element_pairs_per_env": rods * (rods - 1) // 2 * ne * ne + rods * ne * (ne - 1) // 2,
                  "rod_clearance_ms": round(c, 5), "rod_clearance_ms_min_max": [round(min(clearance_ms), 5), round(max(clearance_ms), 5)],
                  "step_ms": round(s, 5), "step_ms_min_max": [round(min(step_ms), 5), round(max(step_ms), 5)],
                  "ratio_to_step": round(c / s, 5), "out_bytes": n * rods * (rods + 1) * 6 * 8})
    env.close()
doc = {"method": f"30 warm-up rounds of step + rod_clearance, then {WINDOWS} alternating windows of 10 env.steps (zero actions) and "
                 "of 50 rod_clearance() calls at the default self_gap, device events around each window (launches "
                 "included), per-call time = window / calls, median over the windows; after reset(seed=0)",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
       "library_source_hash": _capi.library_source_hash(), "cases": cases,
       "note": "the step of the same handle, in the same process, is the yardstick; element_pairs_per_env counts the "
               "self pairs with j > i, of which those with j - i >= self_gap are evaluated"}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
