"""softrod_rod_dynamics on the MI355X: every field of every rod of every env against the yardstick of
tests/rod_dynamics_ref.py (oracle/softrod_oracle_np.py used as a library) evaluated on the state read back from the same
handle, inside the band that tests/test_rod_dynamics.py calibrates without a GPU; the equation of motion on the device's
own output; the tie to ground_reaction(), joint_loads() and muscle_loads() on the same handle; the stale action; free
fall; the refusals; repeatability and read-only.  Worst figure seen on the MI355X over all cases and instants: 6.8e-14
band units against the yardstick (band 1e-12; the internal force is bitwise the oracle's), 1.4e-15 against the other
read-outs."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import RodDynamics

try:
    from tests import ground_reaction_ref as gr
    from tests import muscle_loads_ref as ml
    from tests import rod_dynamics_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import ground_reaction_ref as gr
    import muscle_loads_ref as ml
    import rod_dynamics_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1          # SOFTROD_EINVAL


def _make(case):
    _, env_id, n, _ = case
    return gsa.make_vec(env_id, n, **ref.make_kwargs(case))


def _stepped(case):
    """reset(seed=0), then 2 env.steps of the case's reference-module actions; arm-random under its drawn tables, the
    static cases with every rate scaled below the slip tolerance afterwards."""
    env = _make(case)
    if case == ref.RANDOM:
        mask, contact, material = ref.draw_tables(env.cfg, env.num_envs)
        env.set_contact(mask, **contact)
        env.set_material(mask, **material)
    env.reset(seed=ref.SEED)
    for a in ref.actions(env, case):
        env.step(a)
    if case in ref.STATIC:
        st = env.backend.state()
        st["velocity"] *= gr.RATE_SCALE
        st["omega"] *= gr.RATE_SCALE
        if env.cfg.features & _capi.FEAT_OCTO_HEAD:
            st["head"][3:6] *= gr.RATE_SCALE
            st["head"][15:18] *= gr.RATE_SCALE
        torch.cuda.synchronize()
    return env


def _states(env, case):
    cfgs = [gr.cfg_env(env, i) for i in range(env.num_envs)] if case == ref.RANDOM else None
    return ref.env_states(env, cfgs)


def _dynamics(env):
    return RodDynamics(*(t.cpu().numpy().copy() for t in env.rod_dynamics()))


def _check(env, case, tag):
    """Assertions 1 and 2 on the handle's state as it stands.  -> (the device's fields, the states)."""
    got = _dynamics(env)
    states = _states(env, case)
    n, rods, ne = env.num_envs, _capi.config_rods_per_env(env.cfg), int(env.cfg.n_elem)
    assert [t.shape for t in got] == [(n, rods, 3, ne + 1), (n, rods, 3, ne)] * 3
    top, eom, left, touch = {}, {"translation": 0.0, "rotation": 0.0}, 0, 0
    for e, st in enumerate(states):
        dev = RodDynamics(*(t[e] for t in got))
        assert all(np.isfinite(t).all() for t in dev)
        lo, tc = ref.check_env(dev, st, top)
        left, touch = left + lo, touch + tc
        # the equation of motion on the device's own output
        u = ref.band_units(st, ref.evaluate(st))
        mass, invJ, dil = ref.inertia(st)
        lin = np.abs(dev.acceleration * mass[:, None, :] - (dev.internal_force + dev.external_force)) / (u.acceleration * mass[:, None, :])
        rot = np.abs(dev.angular_acceleration - invJ * (dev.internal_torque + dev.external_torque) * dil[:, None, :]) / u.angular_acceleration
        eom = {"translation": max(eom["translation"], float(lin.max())), "rotation": max(eom["rotation"], float(rot.max()))}
    print(f"{tag}: worst |device - yardstick| in band units", {f: f"{v:.1e}" for f, v in top.items()},
          "| equation of motion", {f: f"{v:.1e}" for f, v in eom.items()}, "| left out", left, "of", touch, "in contact")
    for f, v in {**top, **eom}.items():
        assert v <= ref.BAND, (tag, f, v)
    if ref.has_contact(env.cfg):
        assert touch > 0 and left <= gr.CAP * touch, (left, touch)
    else:
        assert left == 0
    return got, states


def _waves(env, case_id):
    if case_id in gr.WAVES:
        assert env.backend.state()["position"].shape[2] == 64 * gr.WAVES[case_id]


@pytest.mark.parametrize("case", ref.NO_CONTACT, ids=lambda c: c[0])
def test_rods_without_contact_match_the_yardstick(hip_lib, case):
    env = _stepped(case)
    got, states = _check(env, case, case[0])
    assert all(st["point_force"] != 0.0 for st in states) or case[0] == "pendulum3d"
    assert np.abs(got.acceleration).max() > 0 and np.abs(got.angular_acceleration).max() > 0
    for e in range(1, env.num_envs):
        assert not np.array_equal(got.internal_force[0], got.internal_force[e])       # envs at their own rows
    env.close()


@pytest.mark.parametrize("case", ref.CONTACT, ids=lambda c: c[0])
def test_contact_rods_match_the_yardstick_and_the_other_read_outs(hip_lib, case):
    """Assertions 1 and 2, then the tie: external_force = gravity times nodal mass + joint_loads().arm_force on node 0 +
    ground_reaction()'s force, external_torque = joint_loads().arm_torque on element 0 + ground_reaction()'s torque."""
    env = _stepped(case)
    got, states = _check(env, case, case[0])
    _waves(env, case[0])
    force, torque = (t.cpu().numpy().copy() for t in env.ground_reaction())
    assert np.abs(force).max() > 0
    jointed = bool(env.cfg.features & _capi.FEAT_OCTO_HEAD)
    if jointed:
        j = env.joint_loads()
        arm_force, arm_torque = j.arm_force.cpu().numpy().copy(), j.arm_torque.cpu().numpy().copy()
        if got.external_force.shape[1] > 1:
            assert not np.array_equal(got.external_force[:, 0], got.external_force[:, 1])   # arms at their own stride
    tie = {"force": 0.0, "torque": 0.0}
    for e, st in enumerate(states):
        u = ref.band_units(st, ref.evaluate(st))
        mass, _, _ = ref.inertia(st)
        g = np.asarray(list(st["cfg"].gravity), float)
        f = g[None, :, None] * mass[:, None, :]
        t = np.zeros_like(torque[e])
        if jointed:
            f[:, :, 0] += arm_force[e]
            t[:, :, 0] += arm_torque[e]
        f, t = f + force[e], t + torque[e]
        tie["force"] = max(tie["force"], float((np.abs(got.external_force[e] - f) / u.external_force).max()))
        tie["torque"] = max(tie["torque"], float((np.abs(got.external_torque[e] - t) / u.external_torque).max()))
    print(f"{case[0]}: worst |rod_dynamics - (gravity + joint_loads + ground_reaction)| in band units", tie)
    assert tie["force"] <= ref.BAND and tie["torque"] <= ref.BAND
    env.close()


@pytest.mark.parametrize("instant", ["time0", "stepped"])
@pytest.mark.parametrize("case", ref.MUSCLE, ids=lambda c: c[0])
def test_muscle_rods_match_the_yardstick_and_the_other_read_outs(hip_lib, case, instant):
    """At time 0 with the seeded per-element activations written, and after 2 steps.  At time 0 muscle_loads()' instant is
    the state as it stands too: external_force = muscle_loads().external_force + the joint's share on node 0."""
    env = _make(case)
    env.reset(seed=ref.SEED)
    if instant == "time0":
        ml.write_activations(env, ml.seeded_activations(env))
    else:
        for a in ref.actions(env, case):
            env.step(a)
    got, states = _check(env, case, f"{case[0]} {instant}")
    assert all((st["time"] == 0.0) == (instant == "time0") for st in states)
    assert np.abs(got.external_force).max() > 0
    if instant == "time0":                             # (a step's action may drive the two longitudinal layers alike)
        assert np.abs(got.external_torque).max() > 0
    rods = _capi.config_rods_per_env(env.cfg)
    if rods > 1:
        assert not np.array_equal(got.external_force[:, 0], got.external_force[:, 1])
    if instant == "time0":
        assert not (env.cfg.features & (_capi.FEAT_GRAVITY | _capi.FEAT_PLANE_CONTACT_ANISO))
        m = env.muscle_loads()
        f, t = m.external_force.cpu().numpy().copy(), m.external_couple.cpu().numpy().copy()
        if env.cfg.features & _capi.FEAT_OCTO_HEAD:
            j = env.joint_loads()
            f[:, :, :, 0] += j.arm_force.cpu().numpy()
            t[:, :, :, 0] += j.arm_torque.cpu().numpy()
        worst = 0.0
        for e, st in enumerate(states):
            u = ref.band_units(st, ref.evaluate(st))
            worst = max(worst, float((np.abs(got.external_force[e] - f[e]) / u.external_force).max()),
                        float((np.abs(got.external_torque[e] - t[e]) / u.external_torque).max()))
        print(f"{case[0]}: worst |rod_dynamics - (muscle_loads + joint_loads)| in band units {worst:.1e}")
        assert worst <= ref.BAND
    env.close()


def test_the_point_force_is_the_resident_action_and_none_after_a_reset(hip_lib):
    """_prev_action survives reset, the point force does not: a fresh simulator has none until the first set_action."""
    env = gsa.make_vec("SoftPendulum-v0", 4)
    env.reset(seed=0)
    action = np.array([3.25, -7.5, 11.125, -0.3], np.float32)
    env.step(action)
    first = _dynamics(env).external_force[:, 0, 0, 0]
    assert first.tobytes() == action.astype(np.float64).tobytes()
    mask = np.array([False, True, False, True])
    env.reset(seed=5, mask=mask)
    assert env.backend.prev_action_rows().cpu().numpy()[:, 0].tobytes() == action.tobytes()   # the rows are still there
    after = _dynamics(env).external_force[:, 0, 0, 0]
    assert (after[mask] == 0.0).all() and not np.signbit(after[mask]).any()
    assert after[~mask].tobytes() == action[~mask].astype(np.float64).tobytes()
    env.close()


@pytest.mark.parametrize("kw", [dict(n_elems=3), {}, dict(n_elems=63, math_mode=_capi.MATH_LIBM)], ids=["3", "50", "63-libm"])
def test_a_pendulum_just_reset_falls_freely(hip_lib, kw):
    """Right after reset every node accelerates with gravity and no element turns, within the band."""
    env = gsa.make_vec("SoftPendulum-v0", 4, **kw)
    env.reset(seed=0)
    got, states = _check(env, ("free-fall", "SoftPendulum-v0", 4, kw), "free fall " + str(kw))
    worst = 0.0
    for e, st in enumerate(states):
        assert st["time"] == 0.0 and st["point_force"] == 0.0
        u = ref.band_units(st, ref.evaluate(st))
        g = np.asarray(list(st["cfg"].gravity), float)[:, None]
        worst = max(worst, float((np.abs(got.acceleration[e, 0] - g) / u.acceleration[0]).max()),
                    float((np.abs(got.angular_acceleration[e, 0]) / u.angular_acceleration[0]).max()))
    print(f"free fall {kw}: worst |acceleration - gravity|, |angular acceleration| in band units {worst:.1e}")
    assert worst <= ref.BAND
    env.close()


REFUSED = [("SoftArmTracking-v0", {}), ("OctoArmSingle-v0", dict(n_elems=100)), ("OctoArmPush-v1", dict(n_elems=64)),
           ("SoftPendulum-v0", dict(n_elems=64))]


@pytest.mark.parametrize("env_id,kw", REFUSED, ids=[r[0] + "".join(f"-{v}" for v in r[1].values()) for r in REFUSED])
def test_out_of_scope_handles_are_refused(hip_lib, env_id, kw):
    env = gsa.make_vec(env_id, 2, **kw)
    be = env.backend
    out = torch.zeros(2 * 18 * 128, dtype=torch.float64, device=be.device)
    assert hip_lib.softrod_rod_dynamics(be._h, C.c_void_p(out.data_ptr()), be._stream()) == EINVAL
    why = hip_lib.softrod_last_error(be._h).decode()
    assert why.startswith("rod dynamics: ")
    assert why == _capi.rod_dynamics_refusal(env.cfg)
    with pytest.raises(NotImplementedError) as e:
        env.rod_dynamics()
    assert str(e.value) == why
    assert hip_lib.softrod_rod_dynamics(be._h, None, be._stream()) == EINVAL
    assert hip_lib.softrod_last_error(be._h).decode() == "rod dynamics: null output buffer"
    torch.cuda.synchronize()
    assert not out.any()                                                      # nothing was launched
    env.close()


@pytest.mark.parametrize("case_id", ["pendulum-3", "flat-5", "crawl"])
def test_reading_twice_is_identical_and_moves_nothing(hip_lib, case_id):
    case = next(c for c in ref.NO_CONTACT + ref.CONTACT + ref.MUSCLE if c[0] == case_id)
    a_env, b_env = _stepped(case), _stepped(case)
    first, second = _dynamics(a_env), _dynamics(a_env)
    for u, v in zip(first, second):
        assert u.tobytes() == v.tobytes()
    r = a_env.rod_dynamics()
    assert r.internal_force.data_ptr() == a_env.rod_dynamics().internal_force.data_ptr()       # one buffer, overwritten
    buf = a_env.backend._readouts["rod_dynamics"].cpu().numpy()
    assert not buf[:, :, [3, 4, 5, 9, 10, 11, 15, 16, 17], -1].any()            # column n_elem of the per-element rows:
    assert not np.signbit(buf[:, :, [3, 4, 5, 9, 10, 11, 15, 16, 17], -1]).any()     # written, as +0.0
    keys = ["position", "velocity", "director", "omega", "time", "kappa", "rest_kappa", "prev_action"] + (
        ["head"] if a_env.cfg.features & _capi.FEAT_OCTO_HEAD else []) + (
        ["muscle_activation"] if a_env.cfg.features & _capi.FEAT_COOMM_MUSCLES else [])
    sa, sb = a_env.backend.state(), b_env.backend.state()
    for k in keys:
        assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), k
    act = ref.actions(a_env, case)[0]
    for u, v in zip(a_env.step(act)[:4], b_env.step(act)[:4]):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    for k in keys:
        assert sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), k
    a_env.close()
    b_env.close()


def test_numpy_output_and_the_single_env(hip_lib):
    env = gsa.make_vec("OctoArmSingle-v0", 2, numpy_output=True)
    env.reset(seed=0)
    r = env.rod_dynamics()
    assert all(isinstance(t, np.ndarray) for t in r)
    assert r.acceleration.shape == (2, 1, 3, 51) and r.angular_acceleration.shape == (2, 1, 3, 50)
    env.close()
    one = gsa.make("OctoFlat-v0")
    one.reset(seed=0)
    r = one.rod_dynamics()
    assert all(isinstance(t, np.ndarray) for t in r)
    assert r.external_force.shape == (8, 3, 11) and r.external_torque.shape == (8, 3, 10)
    one.close()
