#!/usr/bin/env python3
"""Cost of copy_envs() beside the host path it replaces and beside one env.step, on the same handle in one process.
What profiles/copy_envs_cost.json records, per workload:

  (a) copy_envs(0, every other env)               one source, n - 1 copies
  (b) copy_envs(a random half, the other half)    n / 2 sources, n / 2 copies
  (c) snapshot() + host row permutation + restore()   the only way before copy_envs; host clock, it synchronises
  (d) one env.step

The clock is warmed by steps first.  (a) and (b) twice: `loop_ms`, median of 7 windows of 20 back-to-back calls, device
events on the stream around each window — what a planning loop pays per call, the host's launch work included (each
call waits for its predecessor's upload of the pairs to leave the pinned buffer); and `device_ms`, median of 21 single
calls enqueued behind steps that keep the GPU busy meanwhile, device events around the call — the upload of the pairs
and the kernel on the device alone.  (d) like `loop_ms`.  (c): median of 5 calls, host clock around a call that ends in
a device synchronise.  Bytes moved by a copy: what one env holds, read once and written once per pair; GB/s from
`device_ms`.

  python tools/copy_envs_cost.py [out.json]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402
from gym_softrobot_amd import _capi  # noqa: E402

WINDOWS, CALLS = 7, 20


def windows_ms(fn):
    """Median over WINDOWS of the device time of CALLS calls, per call."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / CALLS)
    return statistics.median(out)


def behind_ms(fn, head, reps=21):
    """Median device time of ONE call enqueued while the GPU is still busy with `head`."""
    out = []
    for _ in range(reps):
        head()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def host_path_ms(be, src, dst, reps=5):
    axis0 = ("time", "env_memory", "prev_action", "prev_kappa", "env_material", "env_contact")
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        snap = be.snapshot()
        for k, v in snap.items():
            if k == "config_fingerprint":
                continue
            rows = v if k in axis0 else v.transpose(0, 1)
            rows[dst] = rows[src]
        be.restore(snap)                                      # ends in a device synchronise
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


cases = []
for env_id, n, head_steps in (("SoftPendulum-v0", 4096, 6), ("OctoFlat-v0", 1024, 1)):
    env = gsa.make_vec(env_id, n)
    env.reset(seed=0)
    be = env.backend
    rng = np.random.default_rng(0)
    act = torch.as_tensor(rng.uniform(-1, 1, (n, env.action_dim)).astype(np.float32), device=be.device)
    for _ in range(10):                                       # warm the clock and every code object
        env.step(act)
    env_bytes = sum(v.numel() * v.element_size() for v in be.state().values() if torch.is_tensor(v)) // n
    perm = rng.permutation(n)
    half_src, half_dst = np.sort(perm[: n // 2]), np.sort(perm[n // 2:])
    all_dst = np.arange(1, n)
    row = {"env": env_id, "n_envs": n, "bytes_per_env": env_bytes}
    for name, src, dst in (("one_to_all", 0, all_dst), ("half_to_half", half_src, half_dst)):
        loop = windows_ms(lambda: be.copy_envs(src, dst))
        ms = behind_ms(lambda: be.copy_envs(src, dst), lambda: [env.step(act) for _ in range(head_steps)])
        moved = 2 * env_bytes * len(dst)
        row[name] = {"pairs": len(dst), "loop_ms": round(loop, 5), "device_ms": round(ms, 5), "bytes_moved": moved,
                     "GB_per_s": round(moved / ms / 1e6, 1)}
    row["env_step_ms"] = round(windows_ms(lambda: env.step(act)), 5)
    row["snapshot_permute_restore_ms"] = round(host_path_ms(be, torch.as_tensor(half_src), torch.as_tensor(half_dst)), 3)
    cases.append(row)
    env.close()
doc = {"method": f"after reset(seed=0) and 10 warm-up steps.  loop_ms and env_step_ms: median of {WINDOWS} windows of {CALLS} "
                 "back-to-back calls, device events on the stream around each window (the host's launch work included); "
                 "device_ms: median of 21 single calls enqueued behind steps that keep the GPU busy, device events around "
                 "the call (upload of the pairs + kernel); snapshot_permute_restore_ms: median of 5 calls, host clock around "
                 "a call that ends in a device synchronise; bytes_moved = 2 x bytes_per_env x pairs, GB_per_s from device_ms",
       "device": "AMD Instinct MI355X (gfx950)", "device_reported": torch.cuda.get_device_name(0),
       "library_source_hash": _capi.library_source_hash(), "cases": cases}
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
print(json.dumps(doc, indent=1))
