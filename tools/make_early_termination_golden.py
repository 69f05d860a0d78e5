#!/usr/bin/env python3
"""Golden vectors of ArmPushEnv's early-termination branch, produced by EXECUTING the reference's own
`ArmPushEnv(mode=..., config_early_termination=True).step()` (gym_softrobot/envs/octopus/arm_push_env.py:288-347,
check_early_termination / cal_desired_Hamiltonian :441-456) in both modes, with the COOMM stand-ins, the oracle arm
and the scripted stepper of tools/make_muscle_env_golden.py (imported, not copied; tools/refshim.py explains how the
reference's files run here).

The stand-in rod's compute_translational_energy / compute_rotational_energy / compute_shear_energy /
compute_bending_energy return diagnostics.rod_energies_host of the state the scripted stepper installed (at the env's
post-step time, with the tapered arm's material).  WHAT THIS PINS: upstream's branch logic and its cut-off — which
energies are summed, `H < 1e-7`, terminated = truncated, the -10 survive reward, no forward reward, the skipped
_isnan_check, a NaN H comparing false, the time limit after it, the NaN-reward and NaN-observation checks.  WHAT IT
DOES NOT PIN: the energy formulas themselves, which are our recollection of pyelastica 1.0.0 (not on disk) — the
fixture holds the energies the twin computed, so the kernels are checked against the twin there, not against
PyElastica.

Cases: an oracle rollout (and the arm at rest, H ~ 0); the velocities of a resting arm scaled so that H = 1e-7 (1 -+
1e-3); NaN in x, v, Q and omega separately; time == final_time and just past it, each with and without a cut-off.

Output: tests/golden/ref_armpush_early_termination.npz — data only.  tests/test_gpu_arm_push_early_termination.py
replays it through the HIP library (state-view injection, n_substeps = 0, both math modes).

    python tools/make_early_termination_golden.py
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import refshim  # noqa: E402
from make_muscle_env_golden import Stack, fill_rod, install_coomm, oracle_arm, state_of  # noqa: E402

from gym_softrobot_amd import _capi  # noqa: E402
from gym_softrobot_amd.diagnostics import rod_energies_host, rod_material_host  # noqa: E402
from oracle import oracle_c  # noqa: E402

GOLD = ROOT / "tests" / "golden"
CUTOFF = 1e-7
warnings.filterwarnings("ignore", category=RuntimeWarning)


def main():
    refshim.install()
    install_coomm()
    oracle_c.build()
    mod = refshim.load("gym_softrobot.envs.octopus.arm_push_env")
    out = {}
    for mode in ("discrete", "continuous"):
        tag = "d_" if mode == "discrete" else "c_"
        cfg = _capi.arm_push_config(1, mode=mode, early_termination=True)
        mat = rod_material_host(cfg, _capi.arm_push_radii(int(cfg.n_elem)))
        env = mod.ArmPushEnv(mode=mode, config_early_termination=True)
        env.reset(seed=0)
        rod = env.shearable_rod
        orc = oracle_arm(mode)
        fill_rod(rod, orc)

        def energies():
            return rod_energies_host(rod.position_collection, rod.velocity_collection, rod.director_collection,
                                     rod.omega_collection, float(env.time), cfg, mat)

        rod.compute_translational_energy = lambda: energies()[0]
        rod.compute_rotational_energy = lambda: energies()[1]
        rod.compute_bending_energy = lambda: energies()[2]
        rod.compute_shear_energy = lambda: energies()[3]
        S = Stack()

        def ref_step(action, pre, post, time, label):
            # the scripted step of tools/make_muscle_env_golden.py: pre-step state in, post-step state out at `time`
            for k in ("x", "v", "Q", "w", "alpha"):
                getattr(rod, {"x": "position_collection", "v": "velocity_collection", "Q": "director_collection",
                              "w": "omega_collection", "alpha": "alpha_collection"}[k])[:] = pre[k]
            env.simulator._calls = 0

            def script(k, t, dt):
                if k == env.step_skip:
                    rod.position_collection[:] = post["x"]
                    rod.velocity_collection[:] = post["v"]
                    rod.director_collection[:] = post["Q"]
                    rod.omega_collection[:] = post["w"]
                    rod.alpha_collection[:] = post["alpha"]
                    return np.float64(time)
                return t
            env.simulator._script = script
            env.time = np.float64(0.0)
            obs, rew, term, trunc, info = env.step(action)
            assert env.simulator._calls == env.step_skip
            S.add(label=label, action=np.atleast_1d(np.asarray(action, np.float64))[:2] if mode == "continuous"
                  else np.array([float(action), 0.0]),
                  pre_x=pre["x"], x=post["x"], v=post["v"], Q=post["Q"], w=post["w"], time=np.float64(time),
                  energies=energies(), obs=obs, reward=np.float64(rew), terminated=bool(term), truncated=bool(trunc),
                  info_time=np.float64(info["time"]), info_trunc=bool(info["TimeLimit.truncated"]))

        acts = [0, 0, 1, 1, 0, 1] if mode == "discrete" else \
            [np.array(a, np.float32) for a in ([0.0, 0.8], [1.0, 0.3], [0.999, 0.5], [0.5, 0.0], [0.0125, 1.0])]
        rest = state_of(orc)
        ref_step(acts[0], rest, rest, 0.025, "rest")                     # the arm at rest: H ~ 0 < cut-off
        for k, a in enumerate(acts):                                      # an oracle rollout
            pre = state_of(orc)
            orc.env_step_push(np.atleast_1d(np.asarray(a, np.float32)))
            ref_step(a, pre, state_of(orc), orc.time, f"rollout{k}")
        base, t_end, a_last = state_of(orc), orc.time, acts[-1]
        # H scaled to 1e-7 (1 -+ 1e-3): a resting arm given the velocities of the rollout's last state
        for sgn, name in ((-1, "H_below"), (1, "H_above")):
            target = CUTOFF * (1 + sgn * 1e-3)
            lo, hi = 0.0, 1.0
            for _ in range(200):
                s = 0.5 * (lo + hi)
                st = {k: v.copy() for k, v in rest.items()}
                st["v"], st["w"] = s * base["v"], s * base["w"]
                h = rod_energies_host(st["x"], st["v"], st["Q"], st["w"], t_end, cfg, mat).sum()
                lo, hi = (s, hi) if h < target else (lo, s)
            st = {k: v.copy() for k, v in rest.items()}
            st["v"], st["w"] = hi * base["v"], hi * base["w"]
            if sgn < 0:
                st["v"], st["w"] = lo * base["v"], lo * base["w"]
            ref_step(a_last, base, st, t_end, name)
        # NaN in each array separately: the _isnan_check branch is skipped (a NaN H compares false)
        for label, key, idx in (("nan_x", "x", (1, 7)), ("nan_x0", "x", (0, 3)), ("nan_v", "v", (2, 40)),
                                ("nan_Q", "Q", (1, 2, 5)), ("nan_w", "w", (0, 39))):
            st = {k: v.copy() for k, v in base.items()}
            st[key][idx] = np.nan
            ref_step(a_last, base, st, t_end, label)
        # the time limit (strict `>`, :325-329), with and without a cut-off
        final = float(env.final_time)
        for state, cut in ((base, "nocut"), (rest, "cut")):
            ref_step(a_last, base, state, final, f"time_eq_final_{cut}")
            ref_step(a_last, base, state, np.nextafter(final, 2 * final), f"time_just_past_{cut}")
        out.update(S.arrays(tag + "et_"))
        H = out[tag + "et_energies"].sum(axis=1)
        print(mode, {str(l): f"{h:.3e}" for l, h in zip(out[tag + "et_label"], H)})

    GOLD.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLD / "ref_armpush_early_termination.npz", **out)
    print("ref_armpush_early_termination.npz", (GOLD / "ref_armpush_early_termination.npz").stat().st_size)


if __name__ == "__main__":
    main()
