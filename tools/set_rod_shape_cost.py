#!/usr/bin/env python3
"""Cost of set_rod_shape() beside a masked reset + observe of the same handle, in one process: each figure is the
median over 7 windows of back-to-back calls with device events around each window (launches included), the two kinds
of window alternating.  The fields are float64 device tensors (used in place: no upload); the mask is a host array,
uploaded by each call as reset uploads its records.  What profiles/set_rod_shape_cost.json records — a record, not a
gate.

  python tools/set_rod_shape_cost.py [out.json]
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

WINDOWS, CALLS = 7, 20


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


cases = []
for env_id, n, kw in (("SoftPendulum-v0", 4096, {}), ("OctoFlat-v0", 1024, {}), ("OctoArmPush-v1", 4096, dict(n_elems=100))):
    env = gsa.make_vec(env_id, n, **kw)
    env.reset(seed=0)
    be = env.backend
    rods, ne = _capi.config_rods_per_env(env.cfg), int(env.cfg.n_elem)
    rng = np.random.default_rng(0)
    rv = float(env.cfg.base_length) / ne
    fields = {name: torch.as_tensor(rng.uniform(-0.05, 0.05, _capi.rod_shape_field_shape(env.cfg, n, name)) / (rv if name == "kappa" else 1.0),
                                    device=be.device) for name in _capi.ROD_SHAPE_FIELDS}
    mask = np.arange(n) % 2 == 0
    shape = lambda: env.set_rod_shape(mask, **fields)      # noqa: E731
    reset = lambda: env.reset(mask=mask)                   # noqa: E731  (ends in the same observe)
    for _ in range(10):                                    # warm clock, code objects loaded
        reset()
        shape()
    torch.cuda.synchronize()
    shape_ms, reset_ms = [], []
    for _ in range(WINDOWS):
        reset_ms.append(window(reset, CALLS))
        shape_ms.append(window(shape, CALLS))
    s, r = statistics.median(shape_ms), statistics.median(reset_ms)
    cases.append({"env": env_id, "n_envs": n, "rods_per_env": rods, "n_elem": ne, "waves": n * rods,
                  "set_rod_shape_ms": round(s, 5), "set_rod_shape_ms_min_max": [round(min(shape_ms), 5), round(max(shape_ms), 5)],
                  "masked_reset_ms": round(r, 5), "masked_reset_ms_min_max": [round(min(reset_ms), 5), round(max(reset_ms), 5)],
                  "ratio_to_masked_reset": round(s / r, 5),
                  "field_bytes": int(sum(t.numel() for t in fields.values())) * 8})
    env.close()
doc = {"method": f"10 warm-up rounds of masked reset + set_rod_shape, then {WINDOWS} alternating windows of {CALLS} env.reset(mask=) "
                 f"calls and of {CALLS} env.set_rod_shape(mask, kappa, sigma, velocity, omega) calls on every other env, all four "
                 "fields float64 device tensors, device events around each window (launches, the mask's upload and each "
                 "call's observe included), per-call time = window / calls, median over the windows",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
       "library_source_hash": _capi.library_source_hash(), "cases": cases,
       "note": "the masked reset of the same handle, in the same process, is the yardstick: both calls end in one observe; "
               "the reset draws its records on the host, set_rod_shape reads resident fields"}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
