"""Planar certificates on the MI355X (softrod_set_planar_certificates; csrc/softrod_planar.hpp): a SoftPendulum handle
whose step kernel trusts the certificates computes, byte for byte, what a handle that proves planarity at every launch
computes — every output and every resident row, padding lanes included — and every writer of resident state withdraws
the certificates of what it writes.

Each test builds two handles from the same starts, certificates on (the default) and off, drives both with the same
calls and compares.  Six envs:
  0, 1, 2  planar starts at three angles (certified from the first step on)
  3        a NaN velocity (set_rod_shape): the NaN fill, never certified
  4        a planar start with the normal reversed: d2_z of the other sign, the other certificate value
  5        a start tilted out of the plane: the 3-D loop, never certified
The state is read through a view taken after the last step only: a view switches the certificates off."""
import numpy as np
import pytest
import torch

from gym_softrobot_amd import _capi
from gym_softrobot_amd.backend import HipRodBackend

pytestmark = pytest.mark.gpu

N = 6
PLANAR, NAN_ENV, FLIPPED, TILTED = [0, 1, 2], 3, 4, 5
THETA = np.array([0.3, -1.1, 2.0, 0.7, -0.4, 1.3])
ROWS = ("position", "velocity", "director", "omega", "tangents", "time", "bc_targets", "control", "prev_action",
        "kappa", "rest_kappa", "env_memory")
# (n_elem, per-env material): 5 and 50, the lane-filling 63, the two-slot instantiation, the per-env-material one
CASES = [(5, False), (50, False), (63, False), (70, False), (50, True)]
CASE_IDS = ["n5", "n50", "n63", "n70_two_slots", "n50_env_material"]


def _frames(theta, tilt=0.0, flip=False):
    """start, unit direction, unit normal of reset_straight for a pendulum at angle theta: softrod_reset's own frame
    (direction (cos, sin, 0), normal (sin, -cos, 0)), tilted out of the x-y plane by `tilt`, normal reversed by `flip`."""
    c, s = np.cos(theta), np.sin(theta)
    d = np.array([c * np.cos(tilt), s * np.cos(tilt), np.sin(tilt)])
    n = np.array([s, -c, 0.0]) * (-1.0 if flip else 1.0)
    return np.zeros(3), d, n


def _mask(*envs):
    m = np.zeros(N, np.uint8)
    m[list(envs)] = 1
    return m


def _reset_straight(be, envs, **kw):
    """reset_straight of `envs` (their THETA) with _frames' keywords; the other envs stay."""
    start, direction, normal = np.zeros((N, 3)), np.tile([1.0, 0.0, 0.0], (N, 1)), np.tile([0.0, -1.0, 0.0], (N, 1))
    for e in envs:
        start[e], direction[e], normal[e] = _frames(THETA[e], **kw)
    be.reset_straight(start, direction, normal, _mask(*envs))


def _start(be):
    """The six starts of the module docstring."""
    be.reset(THETA)
    _reset_straight(be, [FLIPPED], flip=True)
    _reset_straight(be, [TILTED], tilt=0.2)
    ne = int(be.cfg.n_elem)
    vel = np.zeros((N, 1, 3, ne + 1))
    vel[NAN_ENV, 0, 0, ne // 2] = np.nan
    be.set_rod_shape(_mask(NAN_ENV), velocity=vel)


def _pair(n_elem=50, material=False, **cfg_kw):
    """(certificates on, certificates off), started alike."""
    pair = []
    for on in (True, False):
        be = HipRodBackend(_capi.softpendulum_config(N, n_elems=n_elem, **cfg_kw))
        if not on:
            be.set_planar_certificates(False)
        if material:
            rows = np.tile(_capi.env_material_defaults(be.cfg), (N, 1)) * np.linspace(0.8, 1.3, N)[:, None]
            be.set_env_material(rows)
        _start(be)
        pair.append(be)
    return pair


def _actions(seed, steps):
    return np.random.default_rng(seed).uniform(-22.0, 22.0, (steps, N)).astype(np.float32)


def _outputs(be):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (be.obs, be.reward, be.terminated, be.truncated)]


def _certs(be):
    return be.planar_certificates().cpu().numpy()


def _step_both(pair, actions, what):
    on, off = pair
    for t, a in enumerate(actions):
        on.step(a)
        off.step(a)
        assert _outputs(on) == _outputs(off), f"{what}: outputs of step {t + 1}"


def _assert_states_equal(pair, what):
    """Every resident row of the two handles, read through views (which ends the on handle's certificates)."""
    on, off = pair
    torch.cuda.synchronize()
    a, b = on.state(), off.state()
    for k in ROWS:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), f"{what}: {k}"
    assert not _certs(on).any()


def _assert_usual(c):
    """Certificates after at least one step from _start: the planar envs', the reversed one's with the other value."""
    assert c[0] in (1, 2) and (c[PLANAR] == c[0]).all() and c[FLIPPED] == 3 - c[0], c
    assert c[NAN_ENV] == 0 and c[TILTED] == 0, c


def _assert_usual_certificates(pair):
    on, off = pair
    _assert_usual(_certs(on))
    assert not _certs(off).any()


def _close(pair):
    for be in pair:
        be.close()


@pytest.mark.parametrize("steps", [1, 2, 5])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_outputs_and_state_rows_equal_byte_for_byte(hip_lib, case, steps):
    pair = _pair(*case)
    assert not _certs(pair[0]).any()                      # nothing is certified before the first step
    _step_both(pair, _actions(3, steps), "plain steps")
    _assert_usual_certificates(pair)
    _assert_states_equal(pair, f"after {steps} steps")
    _close(pair)


@pytest.mark.parametrize("n_elem", [50, 70])
def test_masked_reset_withdraws_certificates(hip_lib, n_elem):
    pair = _pair(n_elem)
    _step_both(pair, _actions(4, 2), "certified steps")
    _assert_usual_certificates(pair)
    for be in pair:                 # env 1 leaves the plane, env 2 comes back with d2_z reversed
        _reset_straight(be, [1], tilt=-0.3)
        _reset_straight(be, [2], flip=True)
    assert not _certs(pair[0]).any()
    _step_both(pair, _actions(5, 3), "after the masked resets")
    c = _certs(pair[0])
    assert c[1] == 0 and c[2] == c[FLIPPED] == 3 - c[0] and c[0] in (1, 2), c
    _assert_states_equal(pair, "after the masked resets")
    _close(pair)


@pytest.mark.parametrize("n_elem", [50, 70])
def test_set_rod_shape_withdraws_certificates(hip_lib, n_elem):
    pair = _pair(n_elem)
    _step_both(pair, _actions(6, 2), "certified steps")
    kappa = np.zeros((N, 1, 3, n_elem - 1))
    kappa[1, 0, 0] = 0.8                                   # a bend about d1: env 1 curls out of the plane
    kappa[1, 0, 1] = -0.5
    for be in pair:
        be.set_rod_shape(_mask(1), kappa=kappa)
    assert _certs(pair[0])[1] == 0
    _step_both(pair, _actions(7, 3), "after set_rod_shape")
    c = _certs(pair[0])
    assert c[1] == 0 and c[0] in (1, 2) and c[2] == c[0], c
    _assert_states_equal(pair, "after set_rod_shape")
    _close(pair)


def test_reset_shapes_withdraw_certificates(hip_lib):
    pair = _pair(50)
    ne = 50
    kappa = np.zeros((2, 1, 3, ne - 1))
    kappa[:, 0, 2] = 0.6                                   # both entries twist and bend out of the plane
    kappa[:, 0, 0] = [[0.4], [-0.7]]
    for be in pair:
        be.set_reset_shapes(kappa=kappa, seed=5)
    _step_both(pair, _actions(8, 2), "certified steps")
    for be in pair:
        be.reset(THETA, _mask(0, 2))
        be.apply_reset_shapes(_mask(0, 2))
    assert not _certs(pair[0]).any()
    _step_both(pair, _actions(9, 3), "after the shaped resets")
    c = _certs(pair[0])
    assert c[0] == 0 and c[2] == 0 and c[1] in (1, 2), c
    _assert_states_equal(pair, "after the shaped resets")
    _close(pair)


def test_copy_envs_copies_certificates_with_the_rows(hip_lib):
    pair = _pair(50)
    _step_both(pair, _actions(10, 2), "certified steps")
    for be in pair:
        be.copy_envs([TILTED], [1])                        # the tilted env onto a certified one
    c = _certs(pair[0])
    assert c[1] == 0 and c[0] in (1, 2), c
    _step_both(pair, _actions(11, 2), "after the copy onto a certified env")
    for be in pair:
        be.copy_envs([0, FLIPPED], [TILTED, 1])            # and certified ones back onto the two tilted envs
    c = _certs(pair[0])
    assert c[TILTED] == c[0] and c[1] == c[FLIPPED] == 3 - c[0], c
    _step_both(pair, _actions(12, 3), "after the copies back")
    _assert_states_equal(pair, "after copy_envs")
    _close(pair)


def test_bank_slots_keep_their_own_certificates(hip_lib):
    pair = _pair(50)
    for be in pair:
        be.bank_create(3)
    _step_both(pair, _actions(13, 2), "certified steps")
    for be in pair:
        be.bank_save([0, TILTED, FLIPPED], [2, 0, 1])
    _step_both(pair, _actions(14, 2), "between save and load")
    for be in pair:                                        # the tilted state onto env 2, the certified ones onto 5 and 1
        be.bank_load([0, 2, 1], [2, TILTED, 1])
    c = _certs(pair[0])
    assert c[2] == 0 and c[TILTED] == c[0] and c[1] == 3 - c[0] and c[0] in (1, 2), c
    _step_both(pair, _actions(15, 3), "after the load")
    for be in pair:                                        # a reset of the batch leaves the slots' certificates alone
        be.reset(THETA)
        be.bank_load([0, 2], [0, 3])
    c = _certs(pair[0])
    assert c[0] == 0 and c[3] in (1, 2) and not c[[1, 2, 4, 5]].any(), c
    _step_both(pair, _actions(16, 2), "after the second load")
    _assert_states_equal(pair, "after the bank")
    _close(pair)


def test_snapshot_restore_withdraws_certificates(hip_lib):
    pair = _pair(50)
    for be in pair:
        _reset_straight(be, [1], tilt=0.25)
    snaps = [be.snapshot() for be in pair]                 # env 1 out of the plane
    for be in pair:
        _reset_straight(be, [1])                           # ... and back in it
    _step_both(pair, _actions(17, 2), "certified steps")
    c = _certs(pair[0])
    assert c[1] == c[0] and c[0] in (1, 2), c              # (the snapshot left the certificates on)
    for be, snap in zip(pair, snaps):
        be.restore(snap)
    assert not _certs(pair[0]).any()
    _step_both(pair, _actions(18, 3), "after the restore")
    c = _certs(pair[0])
    assert c[1] == 0 and c[0] in (1, 2), c
    _assert_states_equal(pair, "after the restore")
    _close(pair)


@pytest.mark.parametrize("same_step", [False, True], ids=["next_step", "same_step"])
def test_device_auto_reset_withdraws_the_restarted_envs_certificates(hip_lib, same_step):
    """Episodes of two steps (final_time between the first and the second step's clock).  Envs 0, 1, 2 find a staged
    record when they finish — a planar one, a tilted one, one with the normal reversed — and restart on the device;
    the others find none and go on stepping their finished episode."""
    pair = _pair(50, final_time=0.07)
    for be in pair:
        be.autoreset_enable(4)
        if same_step:
            be.autoreset_same_step(True)
        start, direction, normal = np.zeros((N, 1, 3)), np.tile([1.0, 0.0, 0.0], (N, 1, 1)), np.tile([0.0, -1.0, 0.0], (N, 1, 1))
        for e, kw in ((0, {}), (1, {"tilt": 0.3}), (2, {"flip": True})):
            start[e, 0], direction[e, 0], normal[e, 0] = _frames(THETA[e] + 0.5, **kw)
        be.queue_push_straight(start, direction, normal, _mask(0, 1, 2).astype(np.int32))
    _step_both(pair, _actions(19, 1), "the first step")
    _assert_usual_certificates(pair)
    _step_both(pair, _actions(20, 1 if same_step else 2), "the step that ends the episodes, and the restart")
    c = _certs(pair[0])
    assert not c[[0, 1, 2]].any() and c[FLIPPED] in (1, 2), c      # the restarted envs', and nobody else's
    _step_both(pair, _actions(21, 3), "the new episodes")
    c = _certs(pair[0])
    assert c[1] == 0 and c[0] in (1, 2) and c[2] == 3 - c[0] == c[FLIPPED], c
    _assert_states_equal(pair, "after the device auto-reset")
    _close(pair)


def test_a_view_in_mid_run_is_honoured_on_the_next_step(hip_lib):
    pair = _pair(50)
    _step_both(pair, _actions(22, 2), "certified steps")
    _assert_usual_certificates(pair)
    views = [be.state() for be in pair]
    assert not _certs(pair[0]).any()
    for st in views:
        st["velocity"][2, 1, 1:30] = 0.3                   # env 1 leaves the plane
        st["director"][5, 2, :50] *= -1.0                  # env 2: d2_z of the other sign (d1 no longer d2 x d3)
    _step_both(pair, _actions(23, 2), "after the writes through the views")
    assert not _certs(pair[0]).any()                       # off for good
    for st in views:
        st["position"][2, 0, 10] = 1e-3                    # ... so a later write counts as well
    _step_both(pair, _actions(24, 2), "after the second write")
    _assert_states_equal(pair, "after the views")
    _close(pair)


def test_a_launch_without_substeps_leaves_a_rod_uncertified(hip_lib):
    pair = _pair(50)
    a = torch.zeros(N, dtype=torch.float32, device=pair[0].device)
    for be in pair:
        be.substeps(a, 0)
    assert not _certs(pair[0]).any()
    _step_both(pair, _actions(25, 2), "certified steps")
    _assert_usual_certificates(pair)
    for be in pair:
        be.substeps(a, 0)
    assert not _certs(pair[0]).any()
    for be in pair:
        be.substeps(a, 3)                                  # softrod_substeps' form issues certificates like a step
    _assert_usual_certificates(pair)
    _step_both(pair, _actions(26, 2), "after the bare substeps")
    _assert_states_equal(pair, "after the launch without substeps")
    _close(pair)


def test_the_switch(hip_lib):
    on, off = pair = _pair(50)
    _step_both(pair, _actions(27, 1), "the first step")
    on.set_planar_certificates(False)
    assert not _certs(on).any()
    _step_both(pair, _actions(28, 1), "switched off")
    assert not _certs(on).any()
    on.set_planar_certificates(True)
    off.set_planar_certificates(True)                      # and the other way round
    assert not _certs(on).any() and not _certs(off).any()
    _step_both(pair, _actions(29, 2), "switched on")
    _assert_usual(_certs(on))
    _assert_usual(_certs(off))
    off.set_planar_certificates(False)
    _step_both(pair, _actions(30, 1), "one off again")
    _assert_states_equal(pair, "after the switches")
    _close(pair)


def test_other_handles_have_no_certificates(hip_lib):
    """The libm SoftPendulum and SoftPendulum3D: both calls succeed and do nothing."""
    for cfg in (_capi.softpendulum_config(N, math_mode=_capi.MATH_LIBM), _capi.softpendulum3d_config(N)):
        be = HipRodBackend(cfg)
        be.set_planar_certificates(True)
        assert not _certs(be).any()
        be.close()
