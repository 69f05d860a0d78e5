"""Every refusal softrod_create gives before it looks for a device, by its full text.

One case per `return fail(...)` between the top of softrod_create and hipGetDeviceCount, in the
order the checks stand in softrod_capi.hip: a `_capi` builder's config with the fewest fields
altered to reach that refusal and no earlier one.  The texts were recorded from the library before
the checks moved into config_why_not(); no refusal is unreachable (each check has a config that
passes every check in front of it), so none is listed apart.

The acceptance side: what the builders hand out gets past all of them."""
import ctypes as C

import pytest

from gym_softrobot_amd import _capi

EINVAL, ENODEV = -1, -4


def _set(builder, *args, **fields):
    def make():
        cfg = builder(*args)
        for name, value in fields.items():
            if isinstance(value, tuple):        # (index, value) of an array field
                getattr(cfg, name)[value[0]] = value[1]
            else:
                setattr(cfg, name, value)
        return cfg
    return make


def _crawl(**kw):
    return _capi.muscle_octopus_config(_capi.ENV_CRAWL, 2, **kw)


def _octo_flat_many_arms():
    cfg = _capi.octo_flat_config(2)
    cfg.n_arm = 33          # 33 arms x 16 slots = 528 > 512
    return cfg


REFUSALS = [
    ("struct_size", _set(_capi.softpendulum_config, 2, struct_size=8),
     "softrod_config.struct_size mismatch"),
    ("n_envs", _set(_capi.softpendulum_config, 2, n_envs=0),
     "need n_envs >= 1 and 2 <= n_elem <= 126"),
    ("n_elem_low", _set(_capi.softpendulum_config, 2, n_elem=1),
     "need n_envs >= 1 and 2 <= n_elem <= 126"),
    ("n_elem_high", _set(_capi.softpendulum_config, 2, n_elem=127),
     "need n_envs >= 1 and 2 <= n_elem <= 126"),
    ("two_slot_libm", _set(_capi.softpendulum_config, 2, n_elem=64, math_mode=_capi.MATH_LIBM),
     "rods longer than 63 elements (two per lane) exist for SOFTROD_MATH_FAST only"),
    ("dt", _set(_capi.softpendulum_config, 2, dt=0.0),
     "need n_substeps >= 0 and dt > 0"),
    ("n_substeps", _set(_capi.softpendulum_config, 2, n_substeps=-1),
     "need n_substeps >= 0 and dt > 0"),
    ("math_mode", _set(_capi.softpendulum_config, 2, math_mode=7),
     "unknown math_mode"),
    ("env_kind", _set(_capi.softpendulum_config, 2, env_kind=11),
     "unknown env_kind"),
    ("coomm_counts", _set(_capi.arm_push_config, 2, n_muscles=0),
     "COOMM muscles: 1 <= n_muscles <= 4, 0 <= muscle_fl_degree <= 7, one rod of up to 63 elements per env"),
    ("muscle_kind", _set(_capi.arm_push_config, 2, muscle_kind=(0, 5)),
     "muscle_kind: SOFTROD_MUSCLE_LONGITUDINAL or SOFTROD_MUSCLE_TRANSVERSE"),
    ("muscle_switches", _set(_capi.arm_push_config, 2, muscle_equiv_load_form=2),
     "muscle_equiv_load_form, muscle_position_current_radius, muscle_tm_length_law: 0 or 1"),
    ("coomm_fast_mix", _set(_capi.arm_push_config, 2, env_kind=_capi.ENV_NONE),
     "SOFTROD_MATH_FAST compiles the COOMM muscles for SOFTROD_FEATURES_ARM_PUSH with SOFTROD_ENV_ARM_PUSH "
     "(tapered) and for FIXED_BC | ANALYTICAL_DAMPER | COOMM_MUSCLES with SOFTROD_ENV_NONE (uniform rod); "
     "use SOFTROD_MATH_LIBM for any other mix"),
    ("pull_weight", _set(_capi.arm_pull_weight_config, 2, n_arm=2),
     "SOFTROD_ENV_ARM_PULL_WEIGHT: SOFTROD_FEATURES_ARM_PULL_WEIGHT, SOFTROD_MATH_FAST, n_arm = 1, "
     "head_length / head_radius / head_density > 0"),
    ("arm_push_needs", _set(_capi.arm_push_config, 2, arm_push_mode=2),
     "SOFTROD_ENV_ARM_PUSH needs the sucker constraint, three muscle layers and arm_push_mode 0 or 1"),
    ("damper_protocol", _set(_capi.softpendulum_config, 2, damper_protocol=2),
     "damper_protocol: 0 (per unit mass) or 1 (uniform)"),
    ("acos_shift", _set(_capi.softpendulum_config, 2, acos_shift=0.0),
     "SOFTROD_MATH_FAST needs acos_shift > 0 and 0 <= eps_sin <= 1e-3 sqrt(2 acos_shift); "
     "use SOFTROD_MATH_LIBM for other values"),
    ("spline_env", _set(_capi.softpendulum_config, 2, env_kind=_capi.ENV_SOFT_ARM),
     "SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES and SOFTROD_ENV_SOFT_ARM go together"),
    ("spline_counts", _set(_capi.soft_arm_config, 2, n_ctrl=5),
     "spline muscles need SOFTROD_MATH_FAST, 1 <= n_ctrl <= 4, 1 <= n_spline_pieces <= 8, "
     "max_activation_rate > 0"),
    ("octo_head_env", _set(_capi.octo_flat_config, 2, env_kind=_capi.ENV_ARM_SINGLE),
     "SOFTROD_FEAT_OCTO_HEAD goes with SOFTROD_ENV_OCTO_FLAT, SOFTROD_ENV_ARM_PULL_WEIGHT "
     "or the muscle octopus envs"),
    # (under SOFTROD_MATH_FAST the COOMM feature-mix check in front catches another feature set first)
    ("mocto_libm", lambda: _crawl(math_mode=_capi.MATH_LIBM),
     "the muscle octopus exists for SOFTROD_FEATURES_ARM_PULL_WEIGHT and SOFTROD_MATH_FAST only"),
    ("mocto_shape", _set(_crawl, n_arm=4),
     "the muscle octopus needs 16 <= n_elem <= 31, n_arm = 2 or 8, three muscle layers"),
    ("mocto_knots", _set(_crawl, n_knots=4),
     "the muscle octopus: n_knots (actions per arm) 3 / 9 / 3 n_elem and n_suckers 1 / 3 / 0 "
     "for CRAWL / ARM_TWO / REACH"),
    ("mocto_head", _set(_crawl, head_radius=0.0),
     "the muscle octopus needs head_radius, head_density, head_length > 0"),
    ("octo_flat_libm", _set(_capi.octo_flat_config, 2, math_mode=_capi.MATH_LIBM),
     "OctoFlat exists for SOFTROD_FEATURES_OCTO_FLAT and SOFTROD_MATH_FAST only"),
    ("octo_flat_knots", _set(_capi.octo_flat_config, 2, n_knots=0),
     "OctoFlat needs n_elem <= 63, n_arm >= 1, 1 <= n_knots <= n_elem"),
    ("octo_flat_slots", _octo_flat_many_arms,
     "OctoFlat: n_arm * slots-per-arm must not exceed 512"),
    ("octo_flat_head", _set(_capi.octo_flat_config, 2, head_density=0.0),
     "OctoFlat needs head_radius > 0 and head_density > 0"),
    ("n_suckers", _set(_capi.arm_push_config, 2, n_suckers=0),
     "ControllableFixConstraint: 1 <= n_suckers <= 4, not with OctoFlat"),
    ("sucker_index", _set(_capi.arm_push_config, 2, sucker_index=(0, 40)),
     "ControllableFixConstraint: 0 <= sucker_index < n_elem"),
    ("filter_order", _set(_capi.softpendulum3d_config, 2, filter_order=0),
     "LaplaceDissipationFilter needs filter_order >= 1"),
    ("early_termination_value", _set(_capi.arm_push_config, 2, early_termination=2),
     "early_termination is 0 or 1"),
    ("early_termination_env", _set(_capi.softpendulum_config, 2, early_termination=1),
     "early_termination (ArmPushEnv's Hamiltonian cut-off) exists for SOFTROD_ENV_ARM_PUSH / ARM_PULL_WEIGHT only"),
    ("two_bcs", _set(_capi.softpendulum_config, 2,
                     features=_capi.FEATURES_SOFTPENDULUM | _capi.FEAT_FIXED_BC),
     "at most one boundary condition"),
]


@pytest.mark.parametrize("make,text", [pytest.param(m, t, id=i) for i, m, t in REFUSALS])
def test_create_refuses_with_the_recorded_text(hip_lib, make, text):
    cfg = make()
    h = C.c_void_p()
    assert hip_lib.softrod_create(C.byref(cfg), 0, C.byref(h)) == EINVAL
    assert not h.value
    assert hip_lib.softrod_last_error(None).decode() == text


def test_create_refuses_null_arguments(hip_lib):
    h = C.c_void_p()
    assert hip_lib.softrod_create(None, 0, C.byref(h)) == EINVAL
    assert not h.value
    assert hip_lib.softrod_last_error(None).decode() == "null argument"
    cfg = _capi.softpendulum_config(2)
    assert hip_lib.softrod_create(C.byref(cfg), 0, None) == EINVAL
    assert hip_lib.softrod_last_error(None).decode() == "null argument"


ACCEPTED = [
    ("softpendulum", lambda: _capi.softpendulum_config(2)),
    ("softpendulum3d", lambda: _capi.softpendulum3d_config(2)),
    ("arm_single", lambda: _capi.arm_single_config(2)),
    ("octo_flat", lambda: _capi.octo_flat_config(2)),
    ("soft_arm", lambda: _capi.soft_arm_config(2)),
    ("arm_push", lambda: _capi.arm_push_config(2)),
    ("arm_pull_weight", lambda: _capi.arm_pull_weight_config(2)),
    ("crawl", lambda: _capi.muscle_octopus_config(_capi.ENV_CRAWL, 2)),
    ("arm_two", lambda: _capi.muscle_octopus_config(_capi.ENV_ARM_TWO, 2)),
    ("reach", lambda: _capi.muscle_octopus_config(_capi.ENV_REACH, 2)),
    ("softpendulum_100", lambda: _capi.softpendulum_config(2, n_elems=100)),
    ("arm_single_100", lambda: _capi.arm_single_config(2, n_elems=100)),
    ("arm_push_100", lambda: _capi.arm_push_config(2, n_elems=100)),
]


@pytest.mark.parametrize("make", [pytest.param(m, id=i) for i, m in ACCEPTED])
def test_create_lets_the_builders_configs_past_its_checks(hip_lib, make):
    """OK where a device is visible (the handle is destroyed again), ENODEV where none is: the config
    itself is never what softrod_create objects to."""
    cfg = make()
    h = C.c_void_p()
    rc = hip_lib.softrod_create(C.byref(cfg), 0, C.byref(h))
    assert rc in (0, ENODEV), (rc, hip_lib.softrod_last_error(None).decode())
    if rc == 0:
        assert h.value
        assert hip_lib.softrod_destroy(h) == 0
    else:
        assert not h.value
