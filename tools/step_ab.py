#!/usr/bin/env python3
"""A/B of the flagship SoftPendulum-v0 env.step between builds of libsoftrod_hip.so: is it the same bytes, and what
does a step cost.

  python tools/step_ab.py PARENT_LIB BRANCH_LIB [MORE_LIBS ...] [--passes N] [--json out.json] [--timeout seconds]
                          [--attach NAME=file.json ...] [--no-bench] [--no-states]

The first library is the parent (a build of the parent commit, e.g. under variants/, which is git-ignored), the
second the branch; further libraries (store flavours and the like) are measured alongside.  A library written
LIB@TREE runs under the checkout TREE instead of this one — its bench.py, its Python package, its copy of this tool
for the state check — which is how a parent is measured whose library this tree's Python layer cannot load (an entry
point added since: the loader binds every declared symbol), e.g. `git archive HEAD~1 | tar -x -C variants/parent_tree`
built in place.  Per pass and per
library, alternating A, B, ..., A, B, ..., a FRESH child process runs the driver's own command

  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR

with SOFTROD_HIP_LIB set to that library, and `value`, `ms_per_step`, `kernel_ms_avg` of its result line and a
SHA-256 over the dumped obs / reward / terminated / truncated are recorded.  Every child runs under its own
`timeout -k 10`; the tool stops at the first child that does not exit 0 and starts nothing after it.

The state check (skipped with --no-states) runs once per library before the passes: a small mixed batch — planar
rods, one pushed out of the plane through the state view, one holding a NaN — at 50, 63 and 5 elements, whose
every state row (padding lanes included), clock and output is hashed after 1, 3 and 25 env.steps.

The verdict follows tools/readout_ab.py's rule: the change is a gain only if EVERY pass of the branch has a lower
ms_per_step than EVERY pass of the parent (disjoint spreads); the median gain is reported either way.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
OUTPUTS = ("obs", "reward", "terminated", "truncated")
STATE_ROWS = ("position", "velocity", "director", "omega", "tangents", "time")
STATE_SIZES = (50, 63, 5)
STATE_STEPS = (1, 3, 25)
STATE_ENVS = 6


def find_key(doc, key):
    """First value stored under `key` anywhere in a nested result line."""
    if isinstance(doc, dict):
        if key in doc and not isinstance(doc[key], (dict, list)):
            return doc[key]
        for v in doc.values():
            r = find_key(v, key)
            if r is not None:
                return r
    return None


def split_spec(spec):
    """LIB or LIB@TREE -> (absolute library path, absolute checkout the children run under)."""
    lib, _, tree = spec.partition("@")
    return str(Path(lib).resolve()), str(Path(tree).resolve() if tree else ROOT)


def run_child(cmd, lib, timeout, **kw):
    """The child under `timeout -k 10` in the library's checkout, SOFTROD_HIP_LIB set -> (exit status, CompletedProcess)."""
    lib, tree = lib
    full = ["timeout", "-k", "10", str(int(timeout))] + cmd
    p = subprocess.run(full, env={**os.environ, "SOFTROD_HIP_LIB": lib}, cwd=tree, **kw)
    return p.returncode, p


def hash_outputs(d):
    import numpy as np

    h = hashlib.sha256()
    for name in OUTPUTS:
        a = np.load(Path(d) / f"{name}.npy")
        h.update(name.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def bench_once(lib, timeout, tmp):
    out = os.path.join(tmp, "dump")
    rc, p = run_child([sys.executable] + BENCH + ["--dump-outputs", out], lib, timeout, stdout=subprocess.PIPE, text=True)
    if rc != 0:
        return rc
    line = next(json.loads(l) for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l)
    ms, k = line["ms_per_step"], find_key(line, "kernel_ms_avg")
    return {"value": line["value"], "ms_per_step": ms, "kernel_ms_avg": k,
            "gap_us": None if k is None else round((ms - k) * 1e3, 3), "outputs_sha256": hash_outputs(out),
            "library_source_hash": find_key(line, "library_source_hash")}


# ---- the state check's child ------------------------------------------------------------------------------------------
def state_child(out):
    import numpy as np
    import torch

    import gym_softrobot_amd as gsa

    doc = {}
    for ne in STATE_SIZES:
        env = gsa.make_vec("SoftPendulum-v0", STATE_ENVS, device=0, n_elems=ne)
        env.reset(seed=0)
        st = env.backend.state()
        st["velocity"][2, 1, 1:min(ne, 30)] = 0.3            # env 1 leaves the plane: the 3-D fallback
        st["velocity"][2, 2, 1:min(ne, 30)] = 1e-200         # env 2: the fallback on (numerically) the planar problem
        st["position"][0, 3, ne // 2] = float("nan")         # env 3 has blown up: the NaN fill
        acts = np.random.default_rng(7).uniform(-22, 22, (max(STATE_STEPS), STATE_ENVS)).astype(np.float32)
        for t in range(max(STATE_STEPS)):
            res = env.step(acts[t])
            if t + 1 in STATE_STEPS:
                torch.cuda.synchronize()
                h = hashlib.sha256()
                for name in STATE_ROWS:
                    h.update(st[name].cpu().numpy().tobytes())
                for r in res[:4]:
                    h.update(r.cpu().numpy().tobytes())
                doc[f"n{ne}_step{t + 1}"] = h.hexdigest()
        env.close()
    Path(out).write_text(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("libs", nargs="*", help="parent build, branch build, further builds")
    ap.add_argument("--passes", type=int, default=5, help="bench.py runs per library (5 or more)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "planar_launch_ab.json"))
    ap.add_argument("--timeout", type=float, default=240.0, help="per child, seconds")
    ap.add_argument("--attach", action="append", default=[], metavar="NAME=FILE", help="embed a JSON file under `attached`")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--no-states", action="store_true")
    ap.add_argument("--state-child", metavar="OUT", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.state_child:
        return state_child(args.state_child)
    if len(args.libs) < 2:
        ap.error("a parent and a branch library are needed")
    if args.passes < 5 and not args.no_bench:
        ap.error("at least five passes")
    libs = [split_spec(p) for p in args.libs]
    names = ["parent", "branch"] + [Path(p[0]).stem for p in libs[2:]]
    doc = {"about": "written by tools/step_ab.py: one run of it (state_check, passes, summary) on one box in one session; `attached` "
                    "holds the JSON files named with --attach, as they are (each says in its own `about` what it is)",
           "command": "python " + " ".join(BENCH) + " --dump-outputs DIR", "libraries": dict(zip(names, args.libs))}
    with tempfile.TemporaryDirectory() as tmp:
        if not args.no_states:
            states = {}
            for name, lib in zip(names, libs):
                out = os.path.join(tmp, f"states_{name}.json")
                tool = str(Path(lib[1]) / "tools" / "step_ab.py")      # (the checkout's own copy imports its own package)
                rc, _ = run_child([sys.executable, tool, "--state-child", out], lib, args.timeout)
                if rc != 0:
                    print(f"state check: the child on {lib} ended with {rc}; stopping", flush=True)
                    return rc if rc > 0 else 1
                states[name] = json.loads(Path(out).read_text())
            equal = {k: all(states[n][k] == v for n in names) for k, v in states["parent"].items()}
            doc["state_check"] = {"envs": STATE_ENVS, "sizes": STATE_SIZES, "after_steps": STATE_STEPS, "rows": STATE_ROWS,
                                  "kinds": "0, 4, 5 planar; 1, 2 out of plane (state view); 3 holds a NaN",
                                  "equal_to_parent": equal, "all_equal": all(equal.values())}
            print(f"state check: {sum(equal.values())} of {len(equal)} snapshots byte-equal across {names}", flush=True)
        runs = {n: [] for n in names}
        for i in range(0 if args.no_bench else args.passes):
            for name, lib in zip(names, libs):
                r = bench_once(lib, args.timeout, tmp)
                if isinstance(r, int):
                    print(f"pass {i + 1}: the child on {lib} ended with {r}; stopping", flush=True)
                    return r if r > 0 else 1
                runs[name].append(r)
                print(f"pass {i + 1} {name:10s} {r['ms_per_step']:.4f} ms/step  kernel {r['kernel_ms_avg']:.4f} ms  "
                      f"gap {r['gap_us']} us  outputs {r['outputs_sha256'][:12]}", flush=True)
    if not args.no_bench:
        doc["passes"] = runs
        ref = runs["parent"]
        summ = {}
        for name in names:
            ms = [r["ms_per_step"] for r in runs[name]]
            summ[name] = {"ms_per_step_min": min(ms), "ms_per_step_median": statistics.median(ms), "ms_per_step_max": max(ms),
                          "kernel_ms_avg_median": statistics.median(r["kernel_ms_avg"] for r in runs[name]),
                          "gap_us_median": statistics.median(r["gap_us"] for r in runs[name]),
                          "outputs_equal_to_parent": all(r["outputs_sha256"] == ref[0]["outputs_sha256"] for r in runs[name])}
            if name != "parent":
                summ[name]["disjoint_below_parent"] = max(ms) < summ["parent"]["ms_per_step_min"]
                summ[name]["median_gain"] = 1.0 - summ[name]["ms_per_step_median"] / summ["parent"]["ms_per_step_median"]
        doc["summary"] = summ
        for name, s in summ.items():
            print(name, json.dumps(s), flush=True)
    doc["attached"] = {}
    for item in args.attach:
        k, _, f = item.partition("=")
        doc["attached"][k] = json.loads(Path(f).read_text())
    Path(args.json).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
