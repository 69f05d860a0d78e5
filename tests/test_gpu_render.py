"""softrod_render on the MI355X: frames of every env kind against the NumPy float64 restatement of the image model
(tests/render_ref.py) evaluated on the state read back from the same handle.  The rule (render_ref.compare): on the
pixels the reference decides, coverage and the winning body agree exactly, every channel is within 1, depth within
1e-5 max(1, half_width); the reference must decide at least 98 % of a scene's pixels and cover at least 3 % of them
before anything is compared (render_ref.check_conditions).  Then what a frame must not depend on: the depth buffer,
the call count, a fork, another env's NaN state, a graph capture — all bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi

try:
    from tests import render_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import render_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1


def _stepped(env_id, n=3, seed=3, **kw):
    """n envs reset with distinct seeds (seed + i) and stepped twice with random actions."""
    env = gsa.make_vec(env_id, n, **kw)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed + 100)
    for _ in range(2):
        lo, hi = env.action_space.low, env.action_space.high
        env.step(rng.uniform(np.maximum(lo, -1.0), np.minimum(hi, 1.0)).astype(np.float32))
    return env


def _frames(env, cam):
    rgb, depth = env.render_frames(camera=cam, depth=True)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), depth.cpu().numpy().astype(np.float64)


def _check(env, cam, tag):
    """The scene's reference meets its conditions; the device's frames meet the rule.  -> (rgb, depth, reference)"""
    want = ref.render(ref.backend_primitives(env), cam)
    ref.check_conditions(want, tag)
    rgb, depth = _frames(env, cam)
    n = env.num_envs
    assert rgb.shape == (n, cam.height, cam.width, 3) and rgb.dtype == np.uint8
    assert depth.shape == (n, cam.height, cam.width)
    ref.compare(rgb, depth, want, cam.half_width, tag)
    return rgb, depth, want


def _camera(env, width, height, center=None, half_width=None, target_radius=None, follow=None):
    cam = env.default_camera()
    cam.width, cam.height = width, height
    if center is not None:
        cam.center[0], cam.center[1], cam.center[2] = center
    if half_width is not None:
        cam.half_width = half_width
    if target_radius is not None:
        cam.target_radius = target_radius
    if follow is not None:
        cam.follow = follow
    return cam


# (id, env id, kwargs, (W, H), camera edits).  The cameras put the reset geometry in the frame: the pendulum stands on
# the origin along +y (length 1), the single arms lie along +x from the origin (OctoArmSingle 0.35, the muscle arm 0.2).
SCENES = [
    ("pendulum-5", "SoftPendulum-v0", dict(n_elems=5), (37, 23), dict(center=(0.0, 0.5, 0.0), half_width=0.75)),      # byte path, partial tiles
    ("pendulum-50", "SoftPendulum-v0", dict(n_elems=50), (64, 48), dict(center=(0.0, 0.5, 0.0), half_width=0.75)),    # the aligned path
    ("push-100", "OctoArmPush-v1", dict(n_elems=100), (84, 84), dict(center=(0.1, 0.0, 0.0), half_width=0.11)),       # two-slot rows
    ("push-40", "OctoArmPush-v1", dict(n_elems=40), (33, 17), dict(center=(0.1, 0.0, 0.0), half_width=0.11)),         # tapered radii
    ("arm-single", "OctoArmSingle-v0", {}, (40, 40), dict(center=(0.5, 0.0, 0.0), half_width=0.6, target_radius=0.15)),   # the target sphere
    ("arm-single-100", "OctoArmSingle-v0", dict(n_elems=100), (40, 20),
     dict(center=(0.175, 0.0, 0.0), half_width=0.19)),                                                                  # a windowed long arm
    ("reach", "OctoReach-v0", {}, (32, 32), {}),                                                                        # 3-component target from env_aux
    ("soft-arm", "SoftArmTracking-v0", {}, (32, 32), dict(half_width=600.0)),                                           # the oblique camera
    ("pull-weight", "OctoArmPullWeight-v0", {}, (32, 32), dict(center=(0.11, 0.0, 0.0), half_width=0.13)),              # one arm and a rigid body
]


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_frames_equal_the_reference(hip_lib, scene):
    tag, env_id, kw, (w, h), edits = scene
    env = _stepped(env_id, **kw)
    cam = _camera(env, w, h, **edits)
    rgb, depth, want = _check(env, cam, tag)
    bodies = set(np.unique(want.body[~want.undecided]).tolist())
    if env_id in ("OctoArmSingle-v0",) and "n_elems" not in kw or env_id in ("OctoReach-v0", "SoftArmTracking-v0"):
        assert _capi.RENDER_BODY_TARGET in bodies, tag
    if env_id in ("OctoReach-v0", "OctoArmPullWeight-v0"):
        assert _capi.RENDER_BODY_HEAD in bodies, tag
    if env_id == "OctoReach-v0":
        assert bodies >= set(range(8)), tag                     # every arm in its own colour
    env.close()


def test_octo_flat_follows_its_head_in_float64(hip_lib):
    """OctoFlat-v0 at 48 x 48: 8 arms, head and target through the default camera (follow = 1).  Then one env is moved
    by (+100, -50, 0): its frame does not change, because the anchor is subtracted in float64."""
    env = _stepped("OctoFlat-v0")
    # (the arms are 0.8 pixels wide: half a pixel off the head, so that the arms along x and y pass over pixel centres)
    cam = _camera(env, 48, 48, center=(0.009, 0.009, 0.0), target_radius=0.05)
    assert cam.follow == 1
    st = env.backend.state()
    st["head"][18] = st["head"][0] + 0.25                       # the targets, into the frame
    st["head"][19] = st["head"][1] + 0.2
    rgb, depth, want = _check(env, cam, "flat")
    bodies = set(np.unique(want.body[~want.undecided]).tolist())
    assert bodies >= set(range(10)), bodies                     # eight arms, head, target
    e = 1
    shift = torch.tensor([100.0, -50.0, 0.0], dtype=torch.float64, device=st["position"].device)
    st["position"][:, e, :] += shift[:, None]
    st["head"][0:3, e] += shift
    st["head"][18:20, e] += shift[:2]
    rgb2, depth2, want2 = _check(env, cam, "flat moved")
    ok = ~(want.undecided[e] | want2.undecided[e])
    assert np.array_equal(depth2[e][ok] > -np.inf, depth[e][ok] > -np.inf)
    assert np.abs(rgb2[e].astype(int) - rgb[e].astype(int))[ok].max() <= 1
    both = ok & (depth[e] > -np.inf)
    assert np.abs(depth2[e][both] - depth[e][both]).max() <= 1e-5
    for other in (0, 2):
        assert rgb2[other].tobytes() == rgb[other].tobytes() and depth2[other].tobytes() == depth[other].tobytes()
    env.close()


def _pendulum_chord_camera(env, width, height):
    """A camera centred on the middle node of env 0, its right axis along the rod's chord."""
    x = env.backend.state()["position"][:, 0, : int(env.cfg.n_elem) + 1].cpu().numpy()
    chord = x[:, -1] - x[:, 0]
    a = chord / np.linalg.norm(chord)
    b = np.cross([0.0, 0.0, 1.0], a)
    cam = _camera(env, width, height, center=tuple(x[:, x.shape[1] // 2]), half_width=0.75)
    for i in range(3):
        cam.right[i], cam.up[i] = a[i], b[i]
    return cam


@pytest.mark.parametrize("size", [(1, 1), (1024, 1)], ids=["1x1", "1024x1"])
def test_degenerate_frame_sizes(hip_lib, size):
    env = _stepped("SoftPendulum-v0", n=1)
    cam = _pendulum_chord_camera(env, *size)
    rgb, depth, want = _check(env, cam, f"{size[0]}x{size[1]}")
    assert want.body[0, 0, size[0] // 2] == 0                   # the centre pixel sits on the rod
    env.close()


def test_depth_is_optional_and_calls_repeat_and_forks_agree(hip_lib):
    env = _stepped("SoftPendulum-v0", n_elems=20)
    cam = _camera(env, 37, 23, center=(0.0, 0.5, 0.0), half_width=0.75)
    be = env.backend
    n = env.num_envs
    bufs = []
    for with_depth in (True, False, True):
        out = torch.full((n, 23, 37, 3), 77, dtype=torch.uint8, device=be.device)
        z = torch.full((n, 23, 37), 5.0, dtype=torch.float32, device=be.device) if with_depth else None
        torch.cuda.synchronize()
        assert hip_lib.softrod_render(be._h, C.byref(cam), C.c_void_p(out.data_ptr()),
                                      C.c_void_p(z.data_ptr()) if with_depth else None, be._stream()) == 0
        torch.cuda.synchronize()
        bufs.append((out.cpu().numpy(), None if z is None else z.cpu().numpy()))
    assert bufs[0][0].tobytes() == bufs[1][0].tobytes() == bufs[2][0].tobytes()
    assert bufs[0][1].tobytes() == bufs[2][1].tobytes()
    assert (bufs[0][1] > -np.inf).any() and np.isneginf(bufs[0][1]).any()          # every pixel was written
    assert not (bufs[0][1] == 5.0).any()
    # one buffer per (H, W), overwritten; render_frames() without depth returns the same RGB
    a = env.render_frames(camera=cam)
    assert a.data_ptr() == env.render_frames(camera=cam).data_ptr() and a.dtype == torch.uint8
    assert a.cpu().numpy().tobytes() == bufs[0][0].tobytes()
    assert env.render_frames(64, 48).shape == (n, 48, 64, 3)                        # width / height override the default camera
    # a fork's frame is its source's
    env.fork(0, [1, 2])
    rgb, depth = _frames(env, cam)
    for e in (1, 2):
        assert rgb[e].tobytes() == rgb[0].tobytes() == bufs[0][0][0].tobytes()
        assert depth[e].tobytes() == depth[0].tobytes()
    env.close()


def test_a_non_finite_env_renders_as_background_and_disturbs_no_other(hip_lib):
    env = _stepped("SoftPendulum-v0", n_elems=20)
    cam = _camera(env, 40, 40, center=(0.0, 0.5, 0.0), half_width=0.75)
    rgb, depth = _frames(env, cam)
    assert (depth > -np.inf).any(axis=(1, 2)).all()
    env.backend.state()["position"][:, 1, :] = float("nan")
    rgb2, depth2 = _frames(env, cam)
    assert (rgb2[1] == np.array(_capi.RENDER_BACKGROUND, np.uint8)).all() and np.isneginf(depth2[1]).all()
    for e in (0, 2):
        assert rgb2[e].tobytes() == rgb[e].tobytes() and depth2[e].tobytes() == depth[e].tobytes()
    # the state is left as it was: the next step reports the env as terminated, as it always has
    term = env.step(np.zeros((3, 1), np.float32))[2]
    assert term.cpu().numpy().tolist() == [False, True, False]
    env.close()


def test_a_bad_camera_is_refused_and_nothing_is_written(hip_lib):
    env = _stepped("SoftPendulum-v0")
    be = env.backend
    out = torch.full((3, 8, 8, 3), 7, dtype=torch.uint8, device=be.device)
    z = torch.full((3, 8, 8), 7.0, dtype=torch.float32, device=be.device)
    for field, value in (("half_width", 0.0), ("ambient", 2.0), ("width", 0), ("struct_size", 4)):
        cam = _camera(env, 8, 8)
        setattr(cam, field, value)
        assert hip_lib.softrod_render(be._h, C.byref(cam), C.c_void_p(out.data_ptr()), C.c_void_p(z.data_ptr()),
                                      be._stream()) == EINVAL, field
        assert b"render:" in hip_lib.softrod_last_error(be._h), field
    cam = _camera(env, 8, 8)
    assert hip_lib.softrod_render(be._h, C.byref(cam), None, None, be._stream()) == EINVAL
    assert hip_lib.softrod_last_error(be._h) == b"render: null rgb buffer"
    assert hip_lib.softrod_render(be._h, None, C.c_void_p(out.data_ptr()), None, be._stream()) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7).all().item() and (z == 7.0).all().item()
    with pytest.raises(_capi.SoftrodError, match="render:"):
        env.render_frames(width=2000)
    env.close()


@pytest.mark.parametrize("kw", [{}, {"autoreset": "device"}], ids=["no-autoreset", "device-autoreset"])
def test_a_pixel_policy_under_capture_equals_the_eager_loop(hip_lib, kw):
    """A policy whose input is render_frames() under capture_policy_step: four replayed steps give frames (and
    observations) bitwise equal to the un-captured loop.  Everything is enqueued on the one capture stream."""
    n, steps = 4, 4

    def run(graphed):
        env = gsa.make_vec("SoftPendulum-v0", n, device=0, **kw)
        obs, _ = env.reset(seed=5)
        cam = _camera(env, 32, 32, center=(0.0, 0.5, 0.0), half_width=0.75)

        def policy(o):
            rgb, depth = env.render_frames(camera=cam, depth=True)
            seen = rgb.to(torch.float32).mean(dim=(1, 2, 3)) / 255.0 + torch.isfinite(depth).to(torch.float32).mean(dim=(1, 2))
            return (seen.reshape(n, 1) - 1.0) * 20.0 + o[:, :1] * 0.0

        replay = env.capture_policy_step(policy) if graphed else None
        rec = []
        for _ in range(steps):
            out = replay() if graphed else env.step(policy(obs))[:4]
            obs = out[0]
            rgb, depth = (env.backend._frames[k] for k in ((32, 32), (32, 32, "depth")))
            rec.append(tuple(x.detach().cpu().clone() for x in (*out, rgb, depth)))
        torch.cuda.synchronize()
        env.close()
        return rec

    a, b = run(False), run(True)
    for t, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("obs", "reward", "terminated", "truncated", "rgb", "depth"), x, y):
            assert np.array_equal(u.numpy(), v.numpy().astype(u.numpy().dtype), equal_nan=True), f"step {t + 1}: {name} differs"
    assert not np.array_equal(a[0][5].numpy(), a[-1][5].numpy())          # the frames follow the rods
    assert (a[-1][5].numpy() > -np.inf).any()
