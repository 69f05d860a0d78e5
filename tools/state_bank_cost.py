#!/usr/bin/env python3
"""Cost of the state bank beside fork() of the same handle and beside the host path, in one process: each figure is the
median over 7 windows of back-to-back calls with device events around each window (launches and the pairs' upload
included), the kinds of window alternating.  Per case: saving all n envs into n slots, loading n slots into all n envs,
and — like for like with fork(), which cannot write an env it reads — n / 2 pairs each of bank_save, bank_load and
copy_envs (the lower half of the batch into the upper half), at the backend (the library call and its host mirrors) and
at the env (with the per-env host bookkeeping); and one snapshot() + restore() round trip of the whole batch.  What
profiles/state_bank_cost.json records — a record, not a gate.

  python tools/state_bank_cost.py [out.json]
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
    env.create_state_bank(n)
    everything = np.arange(n, dtype=np.int32)
    slots = np.random.default_rng(0).permutation(n).astype(np.int32)      # no slot at its env's index
    lower, upper = everything[: n // 2], everything[n // 2:]
    snap = [None]

    def round_trip():
        snap[0] = be.snapshot()
        be.restore(snap[0])

    calls = {
        "bank_save_all": (lambda: be.bank_save(everything, slots), CALLS),
        "bank_load_all": (lambda: be.bank_load(slots, everything), CALLS),
        "bank_save_half": (lambda: be.bank_save(lower, slots[: n // 2]), CALLS),
        "bank_load_half": (lambda: be.bank_load(slots[: n // 2], upper), CALLS),
        "copy_envs_half": (lambda: be.copy_envs(lower, upper), CALLS),
        "save_states_half": (lambda: env.save_states(lower, slots[: n // 2]), CALLS),
        "load_states_half": (lambda: env.load_states(slots[: n // 2], upper), CALLS),
        "fork_half": (lambda: env.fork(lower, upper), CALLS),
        "snapshot_restore": (round_trip, 2),
    }
    for fn, _ in calls.values():                               # warm clock, code objects loaded, every slot filled
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(WINDOWS):
        for k, (fn, c) in calls.items():
            ms[k].append(window(fn, c))
    med = {k: statistics.median(v) for k, v in ms.items()}
    case = {"env": env_id, "n_envs": n, "n_elem": int(env.cfg.n_elem), "slots": n, "bytes_per_slot": env.state_bank_bytes}
    for k, v in ms.items():
        case[k + "_ms"] = round(med[k], 5)
        case[k + "_ms_min_max"] = [round(min(v), 5), round(max(v), 5)]
    case["bank_save_half_to_copy_envs_half"] = round(med["bank_save_half"] / med["copy_envs_half"], 4)
    case["bank_load_half_to_copy_envs_half"] = round(med["bank_load_half"] / med["copy_envs_half"], 4)
    case["save_states_half_to_fork_half"] = round(med["save_states_half"] / med["fork_half"], 4)
    case["load_states_half_to_fork_half"] = round(med["load_states_half"] / med["fork_half"], 4)
    case["snapshot_restore_to_bank_save_all_plus_load_all"] = round(
        med["snapshot_restore"] / (med["bank_save_all"] + med["bank_load_all"]), 2)
    cases.append(case)
    env.close()
doc = {"method": f"3 warm-up calls of each kind, then {WINDOWS} rounds of one window per kind: {CALLS} back-to-back calls (2 for the "
                 "snapshot() + restore() round trip), device events around each window (launches, the pairs' upload and the "
                 "host work of each call included), per-call time = window / calls, median over the windows.  _all: n pairs, "
                 "every env and every slot once, the slots a permutation of the envs.  _half: n / 2 pairs, envs 0 .. n/2 - 1 "
                 "saved, slots loaded into and envs forked into n/2 .. n - 1 (fork cannot write an env that it reads, so "
                 "n / 2 pairs with distinct sources is the most one call copies).  bank_* and copy_envs: the backend's "
                 "calls; save_states, load_states, fork: the env's, with the host bookkeeping of every pair",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
       "library_source_hash": _capi.library_source_hash(), "cases": cases,
       "note": "copy_envs / fork of the same handle, in the same process, is the yardstick: a save or a load moves the bytes "
               "per pair that a fork moves (bytes_per_slot)"}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
