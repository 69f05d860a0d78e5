"""Every law the cold read-out kernels evaluate has ONE literal text, gym_softrobot_amd/csrc/softrod_literal.hpp, beside
the step kernels' own tuned text — checked on the header text, without a GPU: each law's signature statement occurs in
exactly one of the read-out headers, the shared one, and the step kernels' texts of the same laws (softrod_muscle.hpp,
libm_dynamic_step) stand as they were (line counts and pinned lines)."""
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "gym_softrobot_amd" / "csrc"
SHARED = "softrod_literal.hpp"
READOUT_HEADERS = (SHARED, "softrod_readout.hpp", "softrod_reaction.hpp", "softrod_strains.hpp", "softrod_muscle_readout.hpp",
                   "softrod_joint_readout.hpp", "softrod_dynamics_readout.hpp")
SIGNATURES = ("P.joint_k * dv[i]",                          # FixedJoint2Rigid's force
              "acos(0.5 * trace",                           # the bend / twist strain
              "M.shear[2] * (e * qt2 - 1.0)",               # the shear / stretch load
              "const double Fm = amp * w * rn")             # the muscle law


def test_each_law_is_written_once_among_the_read_outs():
    text = {h: (CSRC / h).read_text() for h in READOUT_HEADERS}
    for sig in SIGNATURES:
        assert {h: t.count(sig) for h, t in text.items() if sig in t} == {SHARED: 1}, sig
    kernels = (CSRC / "softrod_kernels.hpp").read_text()
    assert kernels.index('#include "softrod_literal.hpp"') < kernels.index('#include "softrod_readout.hpp"')
    # every function of the shared header is compiled without contraction
    shared = text[SHARED]
    assert shared.count("__device__ __forceinline__") == shared.count("#pragma clang fp contract(off)") == 6
    assert "__shared__" not in shared and "atomic" not in shared.replace("no atomics", "")
    # ... and every read-out that needs a law calls it there
    for header, calls in (("softrod_reaction.hpp", ("rod_literal_load(", "rod_literal_internal(", "rod_literal_joint(", "rod_literal_contact(")),
                          ("softrod_dynamics_readout.hpp", ("rod_literal_internal(", "rod_literal_joint(", "rod_literal_contact(",
                                                            "muscle_law_literal<1>(")),
                          ("softrod_muscle_readout.hpp", ("muscle_law_literal<EPL>(",)),
                          ("softrod_joint_readout.hpp", ("joint_load_literal(P, H, arm, x0, v0, x1);",))):
        for call in calls:
            assert text[header].count(call) == 1, (header, call)
    # the ONE second text among the read-outs, on purpose: the rod dynamics' own masked load (its header says why)
    load = "L.x[0][c] = S.pos[c * N * W + i];"
    assert {h for h, t in text.items() if load in t} == {SHARED, "softrod_dynamics_readout.hpp"}
    assert "rod_literal_load(" not in text["softrod_dynamics_readout.hpp"] and "WRITTEN AGAIN" in text["softrod_dynamics_readout.hpp"]
    for h in READOUT_HEADERS[1:]:
        assert "WRITTEN AGAIN" not in text[h] or h in ("softrod_strains.hpp", "softrod_dynamics_readout.hpp"), h


def test_the_step_kernels_texts_are_untouched():
    muscle = (CSRC / "softrod_muscle.hpp").read_text()
    assert muscle.count("\n") == 214
    assert "__device__ __forceinline__ void muscle_loads_n(const RodParams& P, const ConstN<EPL>& C, int lane, const LaneN<EPL>& L," \
        in muscle.split("\n")[31]
    assert muscle.split("\n")[103] == "            const double Fm = amp[s] * w * rn;"
    kernels = (CSRC / "softrod_kernels.hpp").read_text()
    start = kernels.index("__device__ __forceinline__ void libm_dynamic_step(")
    step = kernels[start:kernels.index("\n}\n", start) + 3]
    lines = step.split("\n")
    assert step.count("\n") == 161
    assert lines[21] == "    const double n2 = M.shear[2] * (e * qt2 - 1.0);"
    assert lines[46] == "    const double theta = acos(0.5 * trace - 0.5 - P.acos_shift);"
    assert lines[-4] == "        sucker_rates_n<kRuntimeFeatures, 1>(P, B, lane, L);"
