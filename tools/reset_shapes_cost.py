#!/usr/bin/env python3
"""Cost of the shaped-start pass of set_reset_shapes() on an env.step of the device auto-reset modes, in one process:
two batches of the same build, one with a pool of K = 16 start shapes (all four fields) and one without, stepped in
alternating windows with device events around each window; each figure is the median over 7 windows.  Two regimes: the
default episode length, where the pass finds almost nothing to do (its three launches are the cost), and an episode end
on every step (final_time below one env.step), where every env is shaped on every call (same_step) or on every other
call (device: NEXT_STEP restarts on the call after the end).  The queue top-ups are paused inside the windows and run
between them, untimed: their host work is the same with and without a pool.  What profiles/reset_shapes_cost.json
records — a record, not a gate.

  python tools/reset_shapes_cost.py [out.json]
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

WINDOWS, CALLS, K = 7, 24, 16          # 24 calls use at most 24 of the 32 staged records per env
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window(env, actions):
    env.top_up_paused = False
    env._top_up()                       # untimed; waits for the stream
    env.top_up_paused = True
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        env.step(actions)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def pool(cfg, rng):
    rods, ne = _capi.config_rods_per_env(cfg), int(cfg.n_elem)
    rv = float(cfg.base_length) / ne
    fields = {name: rng.uniform(-0.02, 0.02, (K,) + _capi.rod_shape_field_shape(cfg, 0, name)[1:]) / (rv if name == "kappa" else 1.0)
              for name in _capi.ROD_SHAPE_FIELDS}
    if int(cfg.env_kind) == _capi.ENV_SOFTPENDULUM:
        # planar starts (set_rod_shape's rule), so that both batches step on the planar path and the difference is the
        # pass alone: an out-of-plane start sends the rod to the 3-D loop, sixteen times the step
        for name, rows in (("kappa", (0, 2)), ("sigma", (1,)), ("velocity", (2,)), ("omega", (0, 2))):
            fields[name][:, :, rows] = 0.0
    return fields


try:
    with open(os.path.join(ROOT, "profiles", "set_rod_shape_cost.json")) as f:
        shape_ms = {c["env"]: c["set_rod_shape_ms"] for c in json.load(f)["cases"]}
except OSError:
    shape_ms = {}

cases = []
for env_id, n in (("SoftPendulum-v0", 4096), ("OctoFlat-v0", 1024)):
    for mode in ("same_step", "device"):
        for regime, kw in (("default episode length", {}), ("an episode end on every step", dict(final_time=1e-6))):
            plain = gsa.make_vec(env_id, n, autoreset=mode, **kw)
            shaped = gsa.make_vec(env_id, n, autoreset=mode, **kw)
            shaped.set_reset_shapes(**pool(shaped.cfg, np.random.default_rng(0)), seed=1)
            actions = torch.zeros((n, plain.action_dim), dtype=torch.float32, device=plain.backend.device)
            for env in (plain, shaped):
                env.reset(seed=0)
                window(env, actions)    # warm clock, code objects loaded
            before = shaped.reset_shape_episode.clone()
            with_ms, without_ms = [], []
            for _ in range(WINDOWS):
                without_ms.append(window(plain, actions))
                with_ms.append(window(shaped, actions))
            shaped_per_call = float((shaped.reset_shape_episode - before).sum()) / (WINDOWS * CALLS * n)
            w, wo = statistics.median(with_ms), statistics.median(without_ms)
            case = {"env": env_id, "n_envs": n, "autoreset": mode, "regime": regime, "pool_entries": K,
                    "envs_shaped_per_call": round(shaped_per_call, 4),
                    "step_ms_with_pool": round(w, 5), "step_ms_with_pool_min_max": [round(min(with_ms), 5), round(max(with_ms), 5)],
                    "step_ms_without_pool": round(wo, 5),
                    "step_ms_without_pool_min_max": [round(min(without_ms), 5), round(max(without_ms), 5)],
                    "pass_ms": round(w - wo, 5)}
            if shaped_per_call > 0.25 and env_id in shape_ms:
                # per call that shapes the whole batch, against one full-batch set_rod_shape() of the same env
                per_full = (w - wo) / shaped_per_call
                case["pass_ms_per_full_batch"] = round(per_full, 5)
                case["set_rod_shape_ms"] = shape_ms[env_id]
                case["ratio_to_set_rod_shape"] = round(per_full / shape_ms[env_id], 3)
            cases.append(case)
            plain.close()
            shaped.close()
doc = {"method": f"two batches per case, one with a pool of {K} start shapes (kappa, sigma, velocity, omega; SoftPendulum-v0: their "
                 "in-plane rows, so that the planar step kernel keeps stepping) and one without, on the "
                 f"same build in one process; one warm-up window each, then {WINDOWS} alternating windows of {CALLS} env.step calls "
                 "with resident zero actions, device events around each window (launches included), the reset queue topped up "
                 "between the windows, untimed; per-call time = window / calls, median over the windows; pass_ms = with - without",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
       "library_source_hash": _capi.library_source_hash(), "cases": cases,
       "note": "the pass is three launches per env.step (pick, shape, observe) behind or in front of the auto-reset pass; with "
               "nothing to shape every block returns at its first load.  ratio_to_set_rod_shape compares a call that shapes "
               "the whole batch with profiles/set_rod_shape_cost.json's one kernel plus observe: the rest is the pick kernel, "
               "the masked observe and reading the pool through an index"}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
