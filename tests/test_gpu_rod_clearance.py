"""softrod_rod_clearance on the MI355X against the NumPy float64 restatement of its definition
(tests/rod_clearance_ref.py) on the state read back from the same handle.  Geometry is PLACED by writing the writable
position views, so answers are known and cases are small.  The rule (rod_clearance_ref.compare), for every record:
|gap - ref| and |distance - ref| within the band (4e-12 L; 1e-7 L for an exact crossing), and the distance recomputed
in NumPy between the points the device's own (i, s), (j, t) name reproduces the device's distance within the band —
indices are not compared, they are legitimately ambiguous where a closest point is a shared node; the special records
(no pair, non-finite) exactly.  Then what a call must not depend on or disturb: the call count, the state, another env's
NaN, a graph capture — all bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi

try:
    from tests import rod_clearance_ref as ref
except ImportError:                                  # imported with tests/ itself on the path
    import rod_clearance_ref as ref

pytestmark = pytest.mark.gpu

EINVAL = -1


def _records(env, self_gap=None):
    """One call -> the whole (N, rods, rods + 1, 6) buffer as NumPy, and the RodClearance it returned."""
    out = env.rod_clearance(self_gap)
    torch.cuda.synchronize()
    buf = env.backend._readouts["rod_clearance"]
    rods = _capi.config_rods_per_env(env.cfg)
    assert tuple(buf.shape) == (env.num_envs, rods, rods + 1, 6) and buf.dtype == torch.float64
    return buf.cpu().numpy().copy(), out


def _default_gap(env, radii):
    return _capi.rod_clearance_self_gap(float(env.cfg.base_length) / int(env.cfg.n_elem), radii)


def _check(env, tag, self_gap=None, crossing=()):
    """Every record of every env against the yardstick on the state read back.  -> (device records, yardstick)"""
    x, radii, target, L = ref.env_geometry(env)
    g = _default_gap(env, radii) if self_gap is None else self_gap
    got, _ = _records(env, self_gap)
    want = np.stack([ref.clearance(x[e], radii, g, None if target is None else target[e]) for e in range(env.num_envs)])
    worst = 0.0
    for e in range(env.num_envs):
        worst = max(worst, ref.compare(got[e], want[e], x[e], L, f"{tag} env {e}", None if target is None else target[e],
                                       crossing))
    print(f"{tag}: worst error / band = {worst:.2e}")
    return got, want


def _stepped(env_id, n=3, seed=3, steps=2, **kw):
    env = gsa.make_vec(env_id, n, **kw)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed + 100)
    for _ in range(steps):
        lo, hi = env.action_space.low, env.action_space.high
        env.step(rng.uniform(np.maximum(lo, -1.0), np.minimum(hi, 1.0)).astype(np.float32))
    return env


# ---- 1. two arms, placed ------------------------------------------------------------------------------------------------
def test_two_arms_parallel_skew_and_crossing(hip_lib):
    env = gsa.make_vec("OctoArmTwo-v0", 3)
    env.reset(seed=1)
    n, L = int(env.cfg.n_elem), float(env.cfg.base_length)
    _, radii, _, _ = ref.env_geometry(env)
    aux = env.backend.state()["env_aux"]
    for e in range(3):                                              # the targets, beside the rods
        aux[0, e], aux[1, e] = ref.FAR[0] + 0.3 * L * (e + 1), ref.FAR[1] + 0.2 * L
    # parallel rods, a different D per env (env indexing)
    D = [0.3 * L, 0.5 * L, 0.8 * L]
    ref.place(env, np.stack([ref.parallel_rods(n, L, d) for d in D]))
    got, want = _check(env, "parallel")
    for e in range(3):
        assert got[e, 0, 1, 1] == pytest.approx(D[e], abs=4e-12 * L)
        assert got[e, 0, 1, 0] == pytest.approx(D[e] - 2 * radii[0], abs=4e-12 * L)      # the thickest elements, at the base
        assert got[e, 0, 1, 2:4].tolist() == [0.0, 0.0]
        assert got[e, 1, 0].tolist() == got[e, 0, 1][[0, 1, 3, 2, 5, 4]].tolist()          # the mirror
        assert got[e, 0, 2, 3] == -1.0 and got[e, 0, 2, 5] == 0.0                          # the target column
    # a skew pass with negative gap, at a different height per env; then the exact crossing
    i = int(0.4375 * n)
    h = [0.5 * radii[i], 1.0 * radii[i], 1.5 * radii[i]]
    assert min(h) >= 1e-3 * L
    ref.place(env, np.stack([ref.skew_rods(n, L, v) for v in h]))
    got, want = _check(env, "skew")
    for e in range(3):
        # (the arms taper: the least GAP may be one element down rod 1, where it is thicker, a little further than h)
        assert got[e, 0, 1, 0] < 0.0 and h[e] - 4e-12 * L <= got[e, 0, 1, 1] < h[e] + L / n
        assert got[e, 0, 1, 2] == i
        assert got[e, 1, 0].tolist() == got[e, 0, 1][[0, 1, 3, 2, 5, 4]].tolist()
        assert got[e, 1, 0, 4] == got[e, 0, 1, 5] != got[e, 0, 1, 4]                       # s <-> t, not a copy
    ref.place(env, np.stack([ref.skew_rods(n, L, 0.0)] * 3))
    got, want = _check(env, "crossing", crossing=((0, 1),))
    assert (got[:, 0, 1, 1] <= 1e-7 * L).all() and (got[:, 0, 1, 0] < 0).all()
    env.close()


# ---- 2. eight arms at OctoFlat's packing ---------------------------------------------------------------------------------
def test_octo_flat_every_record_after_two_steps(hip_lib):
    env = _stepped("OctoFlat-v0")
    assert int(env.backend.state()["arm_stride"]) >= int(env.cfg.n_elem) + 1
    got, want = _check(env, "flat")
    assert got.shape == (3, 8, 9, 6) and np.isfinite(got).all()
    assert not np.array_equal(got[0], got[1])                        # distinct seeds, distinct records
    for a in range(8):
        for b in range(a + 1, 8):
            assert got[:, b, a].tolist() == got[:, a, b][:, [0, 1, 3, 2, 5, 4]].tolist()
    env.close()


# ---- 3. one long arm folded onto itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_elems", [2, 5, 63, 64, 126])
def test_arm_push_hairpin_self_record(hip_lib, n_elems):
    env = gsa.make_vec("OctoArmPush-v1", 2, n_elems=n_elems)
    env.reset(seed=2)
    L = float(env.cfg.base_length)
    _, radii, target, _ = ref.env_geometry(env)
    assert target is None
    ref.place(env, np.stack([ref.hairpin(n_elems, L, 0.1), ref.hairpin(n_elems, L, 0.16)]))
    g = _default_gap(env, radii)
    got, want = _check(env, f"hairpin-{n_elems}")
    if n_elems <= g:
        assert got[:, 0, 0].tolist() == [ref.NO_PAIR.tolist()] * 2
    else:
        assert np.isfinite(got[:, 0, 0]).all() and got[0, 0, 0, 0] < got[1, 0, 0, 0]      # the wider fold leaves more room
        assert (got[:, 0, 0, 3] - got[:, 0, 0, 2] >= g).all()
    assert got[:, 0, 1].tolist() == [ref.NO_PAIR.tolist()] * 2      # no target
    # an explicit self_gap
    g2 = 2 if n_elems < 10 else g + 3
    got2, _ = _check(env, f"hairpin-{n_elems} self_gap {g2}", self_gap=g2)
    if n_elems > g2:
        assert (got2[:, 0, 0, 3] - got2[:, 0, 0, 2] >= g2).all()
        if g2 > g:
            assert (got2[:, 0, 0, 0] >= got[:, 0, 0, 0]).all()       # fewer pairs: no smaller minimum
    else:
        assert got2[:, 0, 0].tolist() == [ref.NO_PAIR.tolist()] * 2
    env.close()


# ---- 4. the targets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,rods", [("OctoReach-v0", 8), ("OctoArmSingle-v0", 1), ("SoftArmTracking-v0", 1)])
def test_targets(hip_lib, env_id, rods):
    env = _stepped(env_id)
    x, radii, target, L = ref.env_geometry(env)
    assert target is not None and (env_id != "OctoReach-v0" or (target[:, 2] != 0.0).any())
    assert env_id != "OctoArmSingle-v0" or (target == [float(env.cfg.target[0]), float(env.cfg.target[1]), 0.0]).all()
    got, want = _check(env, env_id)
    out = env.rod_clearance()
    torch.cuda.synchronize()
    assert tuple(out.target_gap.shape) == (3, rods) and np.isfinite(out.target_distance.cpu().numpy()).all()
    assert np.array_equal(out.target_distance.cpu().numpy(), got[:, :, rods, 1])
    assert np.array_equal(out.target_element.cpu().numpy(), got[:, :, rods, 2])
    assert np.array_equal(out.target_point.cpu().numpy(), got[:, :, rods, 4])
    assert (got[:, :, rods, 3] == -1.0).all() and (got[:, :, rods, 5] == 0.0).all()
    env.close()


def test_an_env_without_a_target_returns_none_fields(hip_lib):
    env = _stepped("SoftPendulum-v0", n_elems=20)
    got, want = _check(env, "pendulum")
    out = env.rod_clearance()
    assert out.target_gap is None and out.target_distance is None and out.target_element is None and out.target_point is None
    assert got[:, 0, 1].tolist() == [ref.NO_PAIR.tolist()] * 3
    assert tuple(out.gap.shape) == (3, 1, 1) and tuple(out.element.shape) == (3, 1, 1, 2)
    env.close()


# ---- 5. a non-finite env ------------------------------------------------------------------------------------------------------
def test_a_nan_node_marks_its_rows_and_columns_and_disturbs_no_other(hip_lib):
    env = _stepped("OctoFlat-v0")
    before, _ = _records(env)
    st = env.backend.state()
    stride, n = int(st["arm_stride"]), int(env.cfg.n_elem)
    was = st["position"][1, 1, 3 * stride + n].clone()
    st["position"][1, 1, 3 * stride + n] = float("nan")             # the LAST node of arm 3 of env 1
    after, _ = _records(env)
    for b in range(9):
        assert np.array_equal(after[1, 3, b], ref.NON_FINITE, equal_nan=True), b
    for a in range(8):
        assert np.array_equal(after[1, a, 3], ref.NON_FINITE, equal_nan=True), a
    keep = np.ones((8, 9), bool)
    keep[3, :] = keep[:, 3] = False
    assert after[1][keep].tobytes() == before[1][keep].tobytes()
    for e in (0, 2):
        assert after[e].tobytes() == before[e].tobytes()
    _check(env, "flat with a NaN node")                               # the yardstick's NaN rule is the device's
    # a non-finite target: its column only
    st["position"][1, 1, 3 * stride + n] = was
    st["head"][19, 2] = float("inf")
    last, _ = _records(env)
    assert np.isnan(last[2, :, 8, 0]).all() and (last[2, :, 8, 2] == -1.0).all()
    assert last[2, :, :8].tobytes() == before[2, :, :8].tobytes() and last[0].tobytes() == before[0].tobytes()
    env.close()


# ---- 6. calls repeat; 7. the state is not written -----------------------------------------------------------------------------
def test_calls_repeat_share_one_buffer_and_leave_the_state_alone(hip_lib):
    env, twin = (_stepped("OctoArmTwo-v0", seed=4) for _ in range(2))
    snap = env.backend.snapshot()
    a, out_a = _records(env)
    b, out_b = _records(env)
    assert a.tobytes() == b.tobytes() and np.isfinite(a[:, :, :2]).all()
    assert out_a.gap.data_ptr() == out_b.gap.data_ptr() == env.backend._readouts["rod_clearance"].data_ptr()
    assert out_a.gap.dtype == torch.float64 and tuple(out_a.point.shape) == (3, 2, 2, 2)
    again = env.backend.snapshot()
    assert set(snap) == set(again)
    for k in snap:
        assert snap[k].numpy().tobytes() == again[k].numpy().tobytes(), k
    lo, hi = env.action_space.low, env.action_space.high
    act = np.random.default_rng(9).uniform(np.maximum(lo, -1.0), np.minimum(hi, 1.0)).astype(np.float32)
    for x, y in zip(env.step(act)[:4], twin.step(act)[:4]):          # the twin never called it
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    env.close(), twin.close()
    host = _stepped("OctoArmTwo-v0", seed=4, numpy_output=True)
    out = host.rod_clearance()
    assert all(isinstance(t, np.ndarray) for t in out)
    assert np.array_equal(out.gap, a[:, :, :2, 0]) and np.array_equal(out.target_gap, a[:, :, 2, 0])
    host.close()


# ---- 8. the C level -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written(hip_lib):
    env = _stepped("SoftPendulum-v0", n=2)
    be = env.backend
    out = torch.full((2, 1, 2, 6), 7.0, dtype=torch.float64, device=be.device)
    for g in (1, 127, 0, -5):
        assert hip_lib.softrod_rod_clearance(be._h, g, C.c_void_p(out.data_ptr()), be._stream()) == EINVAL, g
        assert hip_lib.softrod_last_error(be._h) == b"rod clearance: self_gap must be 2 .. 126", g
    assert hip_lib.softrod_rod_clearance(be._h, 2, None, be._stream()) == EINVAL
    assert hip_lib.softrod_last_error(be._h) == b"rod clearance: null output buffer"
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()
    with pytest.raises(_capi.SoftrodError, match="rod clearance: self_gap"):
        env.rod_clearance(self_gap=1)
    for g in (2, 126):
        assert hip_lib.softrod_rod_clearance(be._h, g, C.c_void_p(out.data_ptr()), be._stream()) == 0
    torch.cuda.synchronize()
    assert out[:, 0, 0].cpu().numpy().tolist() == [ref.NO_PAIR.tolist()] * 2       # 126 > n_elem = 50: no pair
    env.close()


# ---- 9. inside a captured policy step ----------------------------------------------------------------------------------------
def test_a_clearance_policy_under_capture_equals_the_eager_loop(hip_lib):
    """A policy whose input is rod_clearance() under capture_policy_step: four replayed steps give records (and
    observations) bitwise equal to the un-captured loop."""
    n, steps = 4, 4

    def run(graphed):
        env = gsa.make_vec("SoftPendulum-v0", n, device=0)
        obs, _ = env.reset(seed=5)
        env.rod_clearance()                                           # the buffer exists before anything is captured

        def policy(o):
            c = env.rod_clearance()
            return ((c.gap[:, 0, 0] - c.distance[:, 0, 0]).reshape(n, 1) * 100.0 + c.point[:, 0, 0, :1]).to(torch.float32) + o[:, :1] * 0.0

        replay = env.capture_policy_step(policy) if graphed else None
        rec = []
        for _ in range(steps):
            out = replay() if graphed else env.step(policy(obs))[:4]
            obs = out[0]
            rec.append(tuple(x.detach().cpu().clone() for x in (*out, env.backend._readouts["rod_clearance"])))
        torch.cuda.synchronize()
        env.close()
        return rec

    a, b = run(False), run(True)
    for t, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("obs", "reward", "terminated", "truncated", "records"), x, y):
            assert np.array_equal(u.numpy(), v.numpy().astype(u.numpy().dtype), equal_nan=True), f"step {t + 1}: {name} differs"
    assert not np.array_equal(a[0][4].numpy(), a[-1][4].numpy())              # the records follow the rods
    assert np.isfinite(a[-1][4].numpy()[:, 0, 0]).all()
