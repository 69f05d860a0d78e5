#!/usr/bin/env python3
"""Golden record of upstream's friction knobs, produced by EXECUTING the reference's own build functions
(tools/refshim.py explains how they run here):

    build_arm      gym_softrobot/envs/octopus/build.py:220-292
    build_octopus  gym_softrobot/envs/octopus/build.py:52-217

each called with override_params = {"friction_multiplier": m, "friction_symmetry": s} for a few (m, s) pairs,
1 / False (the registered envs) among them.  What the recording stand-ins capture is what each build hands to
RodPlaneContactWithAnisotropicFriction: k, nu, slip_velocity_tol, kinetic_mu_array and static_mu_array (for
build_octopus, the first of its n_arm registrations, after checking that every arm gets the same ones).

Output: tests/golden/ref_friction_knobs.json, read by tests/test_env_contact.py, which holds
VecRodEnvBase.set_contact(friction_multiplier=..., friction_symmetry=...) to these arrays bit for bit (floats are
written with repr, which round-trips float64 exactly).

    python tools/make_friction_golden.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

import refshim  # noqa: E402

GOLD = ROOT / "tests" / "golden"
PAIRS = [(1.0, False), (1.0, True), (0.25, False), (0.5, True), (2.0, False), (4.0, True), (1.7, False)]


def contact_ops(sim):
    return [op for op in sim._ops if op["kind"] == "contact"
            and op["cls"].__name__ == "RodPlaneContactWithAnisotropicFriction"]


def record(op):
    kw = op["kwargs"]
    return {"k": float(kw["k"]), "nu": float(kw["nu"]), "slip_velocity_tol": float(kw["slip_velocity_tol"]),
            "kinetic_mu_array": [float(x) for x in np.asarray(kw["kinetic_mu_array"], np.float64)],
            "static_mu_array": [float(x) for x in np.asarray(kw["static_mu_array"], np.float64)]}


def main():
    refshim.install()
    build = refshim.load("gym_softrobot.envs.octopus.build")

    class Sim(refshim.BaseSystemCollection, refshim.Constraints, refshim.Connections, refshim.Forcing,
              refshim.Damping, refshim.Contact, refshim.CallBacks):
        pass

    out = {"_about": "what build_arm / build_octopus (octopus/build.py) hand to RodPlaneContactWithAnisotropicFriction "
                     "under override_params {friction_multiplier, friction_symmetry}, recorded while executing the "
                     "reference's own functions (tools/make_friction_golden.py)",
           "build_arm": [], "build_octopus": []}
    for m, s in PAIRS:
        params = {"friction_multiplier": m, "friction_symmetry": s}
        sim = Sim()
        build.build_arm(sim, n_elem=50, time_step=7e-5, override_params=dict(params))
        ops = contact_ops(sim)
        assert len(ops) == 1
        out["build_arm"].append({"friction_multiplier": m, "friction_symmetry": s, **record(ops[0])})
        sim = Sim()
        build.build_octopus(sim, n_arm=8, n_elem=10, time_step=7e-5, override_params=dict(params))
        ops = contact_ops(sim)
        assert len(ops) == 8 and all(record(o) == record(ops[0]) for o in ops)
        out["build_octopus"].append({"friction_multiplier": m, "friction_symmetry": s, **record(ops[0])})
    GOLD.mkdir(parents=True, exist_ok=True)
    path = GOLD / "ref_friction_knobs.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(path.name, path.stat().st_size)


if __name__ == "__main__":
    main()
