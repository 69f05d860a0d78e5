"""One step-kernel table decides what a handle runs, what softrod_kernel_tier reports and what softrod_set_env_material /
softrod_set_env_contact refuse (softrod_capi.hip, kStepRows).  For a matrix of handles, with and without each per-env
table: the tier string or the refusal text equals what the hand-written ladder of the previous build answered (EXPECT:
recorded from that build, not from the library under test), the Python copies of the two refusals accept exactly what
the library accepts, and a refused call leaves the handle stepping bit for bit like an untouched one."""
import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.backend import HipRodBackend

pytestmark = pytest.mark.gpu

OK = 0
EINVAL = -1          # SOFTROD_EINVAL
_EDGE = np.linspace(0.012, 0.001, 51)
TAPER50 = (_EDGE[:-1] + _EDGE[1:]) / 2
NO_WINDOW = {"SOFTROD_DEBUG_SWITCHES": "1", "SOFTROD_NO_WINDOW": "1"}


def _tilted_flat():
    cfg = _capi.octo_flat_config(2)
    cfg.plane_normal[0], cfg.plane_normal[2] = 0.6, 0.8
    return HipRodBackend(cfg, device=0)


# name -> (factory of an env or a backend, environment variables set while it is created)
VARIANTS = {env_id: (lambda env_id=env_id: gsa.make_vec(env_id, 2), {}) for env_id in
            ["OctoArmPullWeight-v0", "OctoArmPush-v0", "OctoArmPush-v1", "OctoArmSingle-v0", "OctoArmTwo-v0", "OctoCrawl-v0",
             "OctoFlat-v0", "OctoFlatLite-v0", "OctoReach-v0", "SoftArmTracking-v0", "SoftPendulum-v0", "SoftPendulum3D-v0"]}
VARIANTS.update({
    "arm-100": (lambda: gsa.make_vec("OctoArmSingle-v0", 2, n_elems=100), {}),
    "arm-100-no-window": (lambda: gsa.make_vec("OctoArmSingle-v0", 2, n_elems=100), NO_WINDOW),
    "arm-tapered": (lambda: gsa.make_vec("OctoArmSingle-v0", 2, radius_profile=TAPER50), {}),
    "push-40": (lambda: gsa.make_vec("OctoArmPush-v1", 2, n_elems=40), {}),
    "push-40-early-termination": (lambda: gsa.make_vec("OctoArmPush-v1", 2, n_elems=40, config_early_termination=True), {}),
    "push-100": (lambda: gsa.make_vec("OctoArmPush-v1", 2, n_elems=100), {}),
    "push-100-early-termination": (lambda: gsa.make_vec("OctoArmPush-v1", 2, n_elems=100, config_early_termination=True), {}),
    "flat-tilted-plane": (_tilted_flat, {}),
    "flat-4-waves": (lambda: HipRodBackend(_capi.octo_flat_config(2, n_elems=20), device=0), {}),
    "flat-8-waves": (lambda: HipRodBackend(_capi.octo_flat_config(2, n_elems=40), device=0), {}),
    "libm-SoftPendulum": (lambda: gsa.make_vec("SoftPendulum-v0", 2, math_mode=0), {}),
    "libm-SoftPendulum3D": (lambda: gsa.make_vec("SoftPendulum3D-v0", 2, math_mode=0), {}),
    "libm-OctoArmSingle": (lambda: gsa.make_vec("OctoArmSingle-v0", 2, math_mode=0), {}),
    "libm-OctoArmPush": (lambda: gsa.make_vec("OctoArmPush-v0", 2, math_mode=0), {}),
    "libm-OctoArmPush-early-termination":
        (lambda: gsa.make_vec("OctoArmPush-v1", 2, math_mode=0, config_early_termination=True), {}),
})
TABLES = {"material": ("softrod_set_env_material", _capi.env_material_defaults, _capi.env_material_refusal),
          "contact": ("softrod_set_env_contact", _capi.env_contact_defaults, _capi.env_contact_refusal)}
PROBES = [(), ("material",), ("contact",), ("material", "contact")]


def _make(name, monkeypatch):
    factory, env_vars = VARIANTS[name]
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    made = factory()
    for k in env_vars:
        monkeypatch.delenv(k)
    return made, getattr(made, "backend", made)


def _set_table(lib, be, table):
    """The C-ABI call itself with the config's own values (the backend would refuse in Python first): rc, error text."""
    entry, defaults, _ = TABLES[table]
    rows = np.tile(defaults(be.cfg), (be.n_envs, 1))
    rc = getattr(lib, entry)(be._h, rows.ctypes.data, None, be._stream())
    return rc, lib.softrod_last_error(be._h).decode()


def probe(lib, name, monkeypatch):
    """[answer for each of PROBES]: the tier string once the probe's tables are set, or the first refusal's text."""
    answers = []
    for tables in PROBES:
        made, be = _make(name, monkeypatch)
        answer = None
        for table in tables:
            rc, text = _set_table(lib, be, table)
            if rc != OK:
                assert rc == EINVAL
                answer = text
                break
        answers.append(be.kernel_tier() if answer is None else answer)
        made.close()
    return answers


# name -> the answers for PROBES: plain, + material, + contact, + material + contact
EXPECT = {
    "OctoArmPullWeight-v0": [
        "softrod_octo_step_kernel<ArmPullWeight,1 wave,1 env/wg,taper>",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "OctoArmPush-v0": [
        "softrod_step_fast_kernel<ArmPush,epl=1,taper>",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "OctoArmPush-v1": [
        "softrod_step_fast_kernel<ArmPush,epl=1,taper>",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "OctoArmSingle-v0": [
        "softrod_step_fast_kernel<ArmSingle,epl=1>",
        "softrod_step_fast_kernel<ArmSingle,epl=1>,env material",
        "softrod_step_fast_kernel<ArmSingle,epl=1>,env contact",
        "softrod_step_fast_kernel<ArmSingle,epl=1>,env material,env contact",
    ],
    "OctoArmTwo-v0": [
        "softrod_mocto_action_kernel | softrod_octo_step_kernel<muscle arms,1 wave,1 env/wg,taper> | softrod_mocto_epilogue_kernel",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "OctoCrawl-v0": [
        "softrod_mocto_action_kernel | softrod_octo_step_kernel<muscle arms,4 waves,1 env/wg,taper> | softrod_mocto_epilogue_kernel",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "OctoFlat-v0": [
        "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>,env contact",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "OctoFlatLite-v0": [
        "softrod_octo_step_kernel<zup,2 waves max,1 env/wg>",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "softrod_octo_step_kernel<zup,2 waves max,1 env/wg>,env contact",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "OctoReach-v0": [
        "softrod_mocto_action_kernel | softrod_octo_step_kernel<muscle arms,4 waves,1 env/wg,taper> | softrod_mocto_epilogue_kernel",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "SoftArmTracking-v0": [
        "softrod_step_fast_kernel<SoftArm,epl=1>",
        "per-env material: not for SoftArmTracking (its muscle torque scale depends on E)",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
        "per-env material: not for SoftArmTracking (its muscle torque scale depends on E)",
    ],
    "SoftPendulum-v0": [
        "softrod_step_fast_kernel<SoftPendulum,epl=1>",
        "softrod_step_fast_kernel<SoftPendulum,epl=1>,env material",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
    ],
    "SoftPendulum3D-v0": [
        "softrod_step_fast_kernel<SoftPendulum3D,epl=1>",
        "softrod_step_fast_kernel<SoftPendulum3D,epl=1>,env material",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
    ],
    "arm-100": [
        "softrod_step_window_kernel<ArmSingle,4 rods/wg> refresh=3 + softrod_step_fast_kernel<ArmSingle,epl=2> epilogue",
        "per-env material: rods of up to 63 elements only (not the two-slot or windowed long rods)",
        "per-env contact: rods of up to 63 elements only (not the two-slot or windowed long rods)",
        "per-env material: rods of up to 63 elements only (not the two-slot or windowed long rods)",
    ],
    "arm-100-no-window": [
        "softrod_step_fast_kernel<ArmSingle,epl=2>",
        "per-env material: rods of up to 63 elements only (not the two-slot or windowed long rods)",
        "per-env contact: rods of up to 63 elements only (not the two-slot or windowed long rods)",
        "per-env material: rods of up to 63 elements only (not the two-slot or windowed long rods)",
    ],
    "arm-tapered": [
        "softrod_step_fast_kernel<ArmSingle,epl=1,taper>",
        "per-env material: not for a tapered rod (softrod_set_radius_profile)",
        "per-env contact: not for a tapered rod (softrod_set_radius_profile)",
        "per-env material: not for a tapered rod (softrod_set_radius_profile)",
    ],
    "push-40": [
        "softrod_step_fast_kernel<ArmPush,epl=1,taper>",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "push-40-early-termination": [
        "softrod_step_fast_kernel<ArmPush,epl=1,taper>",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "push-100": [
        "softrod_step_fast_kernel<ArmPush,epl=2,taper>",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "push-100-early-termination": [
        "softrod_step_fast_kernel<ArmPush,epl=2,taper>",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "flat-tilted-plane": [
        "softrod_octo_step_kernel<general plane,2 waves max,1 env/wg>",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: a contact plane with normal e_z only",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "flat-4-waves": [
        "softrod_octo_step_kernel<zup,8 waves max,1 env/wg>",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: OctoFlat with at most two waves per env only (n_arm x segment <= 128 lanes; not the four- and eight-wave shapes)",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "flat-8-waves": [
        "softrod_octo_step_kernel<zup,8 waves max,1 env/wg>",
        "per-env material: not for OctoFlat or the muscle octopus envs",
        "per-env contact: OctoFlat with at most two waves per env only (n_arm x segment <= 128 lanes; not the four- and eight-wave shapes)",
        "per-env material: not for OctoFlat or the muscle octopus envs",
    ],
    "libm-SoftPendulum": [
        "softrod_step_libm_kernel",
        "softrod_step_libm_kernel,env material",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
    ],
    "libm-SoftPendulum3D": [
        "softrod_step_libm_kernel",
        "softrod_step_libm_kernel,env material",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
        "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only",
    ],
    "libm-OctoArmSingle": [
        "softrod_step_libm_kernel",
        "softrod_step_libm_kernel,env material",
        "softrod_step_libm_kernel,env contact",
        "softrod_step_libm_kernel,env material,env contact",
    ],
    "libm-OctoArmPush": [
        "softrod_step_libm_kernel",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
    "libm-OctoArmPush-early-termination": [
        "softrod_step_libm_kernel",
        "per-env material: not for the muscle envs",
        "per-env contact: not for the muscle envs",
        "per-env material: not for the muscle envs",
    ],
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_tier_or_refusal_is_what_the_ladder_answered(hip_lib, monkeypatch, name):
    got = probe(hip_lib, name, monkeypatch)
    for tables, answer in zip(PROBES, got):
        print(name, "+".join(tables) or "plain", "->", answer)
    assert got == EXPECT[name]


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_python_refusal_agrees_with_the_library(hip_lib, monkeypatch, name, table):
    made, be = _make(name, monkeypatch)
    why = TABLES[table][2](be.cfg, tapered="radius_profile" in be._tables)
    rc, text = _set_table(hip_lib, be, table)
    made.close()
    assert (why is None) == (rc == OK), (why, rc, text)
    if rc != OK:
        assert rc == EINVAL and text.startswith(f"per-env {table}: ")


REFUSED = [("OctoFlat-v0", "material"), ("SoftPendulum-v0", "contact"), ("flat-4-waves", "contact"),
           ("arm-tapered", "material"), ("arm-tapered", "contact"), ("arm-100", "material"), ("arm-100", "contact"),
           ("push-40-early-termination", "material"), ("push-40-early-termination", "contact")]


@pytest.mark.parametrize("name,table", REFUSED, ids=[f"{n}-{t}" for n, t in REFUSED])
def test_a_refused_table_leaves_the_handle_stepping_as_before(hip_lib, monkeypatch, name, table):
    (a_made, a), (b_made, b) = _make(name, monkeypatch), _make(name, monkeypatch)
    rc, _ = _set_table(hip_lib, b, table)
    assert rc == EINVAL
    assert b.kernel_tier() == a.kernel_tier()
    acts = np.random.default_rng(2).uniform(-1, 1, (2, a.n_envs, a.action_dim)).astype(np.float32)
    for made, be in ((a_made, a), (b_made, b)):
        if made is be:
            be.reset_octo(np.random.default_rng(5).uniform(0.5, 2.0, (be.n_envs, 2)))      # flat_env.py:221
        else:
            made.reset(seed=4)
    for t in range(2):
        out_a, out_b = a.step(acts[t]), b.step(acts[t])
        for x, y in zip(out_a, out_b):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    a_made.close()
    b_made.close()
