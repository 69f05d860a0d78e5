#!/usr/bin/env python3
"""What a batch of frames costs: ms per softrod_render (render_frames) beside the same run's step kernel.

4096 SoftPendulum-v0 envs and 1024 OctoFlat-v0 envs, each at 84 x 84 and 64 x 64 through the env's default camera, RGB
alone and RGB with depth, in ONE process per case.  The bench.py way: the clock is pre-heated with env.steps, then
--windows windows of --calls render calls each are timed with device events around the window (launches included); the
figure is the median window.  Beside it: the step kernel's own time (softrod_set_timing / softrod_last_kernel_ms and the
median over the pre-heat steps), the bytes a call writes and the time the HBM would need for them alone at 6.3 TB/s,
which says whether the output or the work in front of it (projection, culling, the primitive loop, the launch) bounds the
call.  Writes profiles/render_overhead.json.

    python tools/render_bench.py [--windows 5] [--calls 100] [--out profiles/render_overhead.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import gym_softrobot_amd as gsa  # noqa: E402

HBM_BYTES_PER_S = 6.3e12          # the streaming ceiling an element-wise kernel reaches on the MI355X
CASES = (("SoftPendulum-v0", 4096, 60), ("OctoFlat-v0", 1024, 12))       # env, envs, pre-heat env.steps
SIZES = ((84, 84), (64, 64))


def _windows(fn, calls, windows):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="render calls per window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "render_overhead.json"))
    args = ap.parse_args()
    results = []
    for env_id, n, preheat in CASES:
        env = gsa.make_vec(env_id, n)
        env.reset(seed=0)
        be = env.backend
        zero = torch.zeros((n, env.action_dim), dtype=torch.float32, device=be.device)
        be.set_timing(preheat)
        for _ in range(preheat):                      # warms the clock and leaves a stepped (bent) batch to draw
            env.step(zero)
        torch.cuda.synchronize()
        step_ms = float(np.median(be.kernel_times_ms()))
        last_ms = float(be.last_kernel_ms())
        be.set_timing(0)
        cam = env.default_camera()
        prims = int(env.cfg.n_elem) * gsa._capi.config_rods_per_env(env.cfg)
        for w, h in SIZES:
            for depth in (False, True):
                fn = lambda: env.render_frames(w, h, depth=depth)      # noqa: E731
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                ms = _windows(fn, args.calls, args.windows)
                out_bytes = n * h * w * (3 + (4 if depth else 0))
                med = statistics.median(ms)
                rec = {"env": env_id, "n_envs": n, "width": w, "height": h, "depth": depth, "capsules_per_env": prims,
                       "half_width": float(cam.half_width), "render_ms": round(med, 5),
                       "window_render_ms": [round(x, 5) for x in ms], "step_kernel_ms": round(step_ms, 5),
                       "last_kernel_ms": round(last_ms, 5), "render_over_step": round(med / step_ms, 4),
                       "frames_per_s": round(n / (med * 1e-3)), "out_bytes": out_bytes,
                       "out_ms_at_hbm_rate": round(1e3 * out_bytes / HBM_BYTES_PER_S, 5),
                       "render_over_out_time": round(med / (1e3 * out_bytes / HBM_BYTES_PER_S), 2)}
                print(json.dumps(rec), flush=True)
                results.append(rec)
        env.close()
    worst = min(r["render_over_out_time"] for r in results)
    note = ("every case takes at least %.1fx the time its output bytes need at the HBM's streaming rate: the work in front "
            "of the stores (projection and culling per tile, the primitive loop, the launch), not the output, bounds the "
            "call" % worst) if worst >= 2.0 else \
           ("at least one case runs within %.1fx of the time its output bytes need at the HBM's streaming rate: there the "
            "output, not the primitive loop, is what bounds the call" % worst)
    doc = {"device": torch.cuda.get_device_name(0), "library_source_hash": gsa._capi.library_source_hash(),
           "method": "clock pre-heated with env.steps of zero actions (timed: step_kernel_ms is the median of their "
                     "device-event kernel times, last_kernel_ms softrod_last_kernel_ms after the last); then the median "
                     "of `windows` windows of `calls` render_frames() calls each, device events around a window, "
                     "launches included; default camera of the env",
           "windows": args.windows, "calls_per_window": args.calls, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "results": results, "note": note}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
