"""Per-env ground contact and friction on the MI355X (set_contact / softrod_set_env_contact): the config's own values
give byte-identical rollouts, randomised envs match the CPU oracle built with each env's own config, untouched envs
are bit-identical to a uniform batch, auto-resets, masked updates, snapshots and captured graphs keep the table, a
frictionless env does not drift, and out-of-scope handles refuse."""
import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.backend import HipRodBackend

pytestmark = pytest.mark.gpu

RTOL = 1e-5
EINVAL = -1          # SOFTROD_EINVAL
MODES = [(0, "libm"), (1, "fast")]
MAT_KEYS = ("youngs_modulus", "shear_modulus", "density", "damping_constant")


def _acts(env, T, seed):
    rng = np.random.default_rng(seed)
    hi = 6.0 if env.cfg.env_kind == _capi.ENV_ARM_SINGLE else 22.0
    return rng.uniform(-hi, hi, (T, env.num_envs, env.action_dim)).astype(np.float32)


def _outputs(env, a):
    obs, rew, term, trunc, _ = env.step(a)
    return [x.cpu().numpy().copy() for x in (obs, rew, term, trunc)]


def _state(env):
    st = env.backend.state()
    keys = ["position", "velocity", "director", "omega", "time"]
    if env.cfg.env_kind == _capi.ENV_OCTO_FLAT:
        keys.append("head")
    return {k: st[k].cpu().numpy().copy() for k in keys}


def _draw(n, seed):
    """Friction multipliers across x0.25 .. x4 with random symmetry, k and nu across x0.5 .. x2 of the config's."""
    rng = np.random.default_rng(seed)
    return dict(friction_multiplier=2.0 ** rng.uniform(-2, 2, n), friction_symmetry=rng.random(n) < 0.5,
                k=2.0 ** rng.uniform(-1, 1, n), nu=2.0 ** rng.uniform(-1, 1, n))


def _randomise(env, d, mask=None):
    c = env.cfg
    env.set_contact(mask, contact_k=c.contact_k * d["k"], contact_nu=c.contact_nu * d["nu"],
                    friction_multiplier=d["friction_multiplier"], friction_symmetry=d["friction_symmetry"])


def _rows(cfg, d):
    """(n, 8) rows of softrod_set_env_contact for a draw (what set_contact computes)."""
    n = len(d["k"])
    out = np.empty((n, 8))
    for i in range(n):
        kin, stat = _capi.friction_mu_arrays(cfg, float(d["friction_multiplier"][i]), bool(d["friction_symmetry"][i]))
        out[i] = [cfg.contact_k * d["k"][i], cfg.contact_nu * d["nu"][i], *kin, *stat]
    return out


def _cfg_row(cfg, row, material=None):
    c = cfg.copy()
    c.n_envs = 1
    c.contact_k, c.contact_nu = float(row[0]), float(row[1])
    for j in range(3):
        c.kinetic_mu[j], c.static_mu[j] = float(row[2 + j]), float(row[5 + j])
    if material is not None:
        for k, v in zip(MAT_KEYS, material):
            setattr(c, k, float(v))
    return c


def _mat_draw(n, seed):
    rng = np.random.default_rng(seed)
    return {k: 2.0 ** rng.uniform(-1, 1, n) for k in ("youngs_modulus", "density", "damping_constant")}


def _targets(n, seed=0):
    from gym_softrobot_amd.seeding import np_random

    out = np.empty((n, 2))
    for i in range(n):
        rng, _ = np_random(seed + i)
        out[i] = (2 - 0.5) * rng.random(2) + 0.5      # flat_env.py:221
    return out


def _flat(ob):
    return np.concatenate([ob["individual"].ravel(), ob["shared"]])


# ---- the config's own values -------------------------------------------------------------------------------------
SAME = [("OctoArmSingle-v0", 1, False), ("OctoArmSingle-v0", 0, False), ("OctoArmSingle-v0", 1, True),
        ("OctoArmSingle-v0", 0, True), ("OctoFlat-v0", 1, False), ("OctoFlatLite-v0", 1, False)]


@pytest.mark.parametrize("env_id,math_mode,material", SAME,
                         ids=["arm-fast", "arm-libm", "arm-fast-material", "arm-libm-material", "flat", "flat-lite"])
def test_config_values_are_byte_identical(hip_lib, env_id, math_mode, material):
    n, T = 13, 2
    a_env = gsa.make_vec(env_id, n, math_mode=math_mode)
    b_env = gsa.make_vec(env_id, n, math_mode=math_mode)
    c = b_env.cfg
    if material:        # both batches carry the config's material table: only the contact table differs
        for e in (a_env, b_env):
            e.set_material(**{k: getattr(c, k) for k in MAT_KEYS})
    b_env.set_contact(contact_k=c.contact_k, contact_nu=c.contact_nu, kinetic_mu=list(c.kinetic_mu),
                      static_mu=list(c.static_mu))
    assert b_env.backend.kernel_tier().endswith(",env contact")
    assert not a_env.backend.kernel_tier().endswith(",env contact")
    a_env.reset(seed=5)
    b_env.reset(seed=5)
    for a in _acts(a_env, T, 1):
        for x, y in zip(_outputs(a_env, a), _outputs(b_env, a)):
            assert x.tobytes() == y.tobytes()
    sa, sb = _state(a_env), _state(b_env)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    a_env.close()
    b_env.close()


# ---- randomised batches against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("material", [False, True], ids=["contact", "contact+material"])
@pytest.mark.parametrize("math_mode,mode_id", MODES, ids=[m[1] for m in MODES])
def test_randomised_arm_batch_matches_the_oracle_per_env(hip_lib, oracle_built, math_mode, mode_id, material):
    n, T = 64, 2
    env = gsa.make_vec("OctoArmSingle-v0", n, math_mode=math_mode)
    c = env.cfg
    d = _draw(n, 11)
    _randomise(env, d)
    np.testing.assert_array_equal(env.backend.env_contact(), _rows(c, d))
    mats = None
    if material:
        f = _mat_draw(n, 12)
        env.set_material(youngs_modulus=c.youngs_modulus * f["youngs_modulus"], density=c.density * f["density"],
                         damping_constant=c.damping_constant * f["damping_constant"])
        m = env.material()
        mats = np.stack([m[k] for k in MAT_KEYS], axis=1)
    env.reset(seed=0)
    rows = env.backend.env_contact()
    rods, ctrl = [], []
    for i in range(n):
        ci = _cfg_row(c, rows[i], None if mats is None else mats[i])
        for lst, kw in ((rods, {}), (ctrl, dict(omp="fma"))):
            r = oracle_built.OracleRod(ci, **kw)
            r.reset_arm()
            lst.append(r)

    def err(x, ref, atol):                  # worst |x - ref| in units of the tolerance band
        return float(np.max(np.abs(np.asarray(x, np.float64) - ref) / (RTOL * np.abs(ref) + atol)))
    # Strong friction makes a few envs' stick / slip switches sensitive to rounding: the oracle and the same source
    # built with FMA contraction (the rounding control of DESIGN.md section 3) already differ by a tolerance band
    # there within 2 env.steps (with this draw: env 44, multiplier 3.1, 1.1 bands).  Envs whose control differs by
    # more than a quarter band are held to ten times the control's difference instead; every other env to the band.
    sens = np.zeros(n)
    got = []
    for a in _acts(env, T, 2):
        obs, rew, term, trunc = _outputs(env, a)
        step = []
        for i, (r, q) in enumerate(zip(rods, ctrl)):
            o, rw, te, tr = r.env_step_arm(a[i])
            oc, rwc = q.env_step_arm(a[i])[:2]
            sens[i] = max(sens[i], err(oc, o, 1e-7), err(rwc, rw, 1e-9))
            step.append((err(obs[i], o, 1e-7), err(rew[i], rw, 1e-9)))
            assert bool(term[i]) == te and bool(trunc[i]) == tr
        got.append(step)
    sn = env.backend.state_numpy()
    sensitive = sens > 0.25
    assert sensitive.sum() <= n // 16, np.nonzero(sensitive)[0]
    for i, r in enumerate(rods):
        band = 10.0 * sens[i] if sensitive[i] else 1.0
        assert max(max(s[i]) for s in got) <= band, (i, [s[i] for s in got], sens[i])
        for name in ("x", "Q"):
            ref = r.get(name)
            assert np.max(np.abs(sn[name][i] - ref)) <= band * RTOL * np.max(np.abs(ref)), (i, name, sens[i])
    env.close()


def _compare_octo_state(be, oracles):
    st = be.octo_state_numpy()
    for i, o in enumerate(oracles):
        hd = o.head()
        np.testing.assert_allclose(st["head_x"][i], hd["x"], rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(st["head_v"][i], hd["v"], rtol=RTOL, atol=1e-7)
        for a in range(o.n_arm):
            arm = o.arm(a)
            np.testing.assert_allclose(st["x"][i, a], arm.get("x"), rtol=RTOL, atol=1e-8)
            np.testing.assert_allclose(st["v"][i, a], arm.get("v"), rtol=RTOL, atol=1e-6)
            np.testing.assert_allclose(st["Q"][i, a], arm.get("Q"), rtol=RTOL, atol=1e-7)


@pytest.mark.parametrize("n_arm,n_action", [(8, 3), (1, 8)], ids=["OctoFlat", "OctoFlatLite"])
def test_randomised_octo_batch_matches_the_oracle_over_200_substep_windows(hip_lib, oracle_built, n_arm, n_action):
    """test_gpu_octo.py's short-step protocol (200 substeps per env.step, 3 env.steps) with every env on its own
    ground; 10 envs: the four-envs-per-workgroup shape has a partly idle last workgroup."""
    n, T = 10, 3
    cfg = _capi.octo_flat_config(n, n_arm=n_arm, n_action=n_action)
    cfg.n_substeps = 200
    be = HipRodBackend(cfg, device=0)
    rows = _rows(cfg, _draw(n, 21))
    be.set_env_contact(rows)
    assert be.kernel_tier().endswith(",env contact")
    tg = _targets(n, 11)
    be.reset_octo(tg)
    oracles = []
    for i in range(n):
        o = oracle_built.OracleOcto(_cfg_row(cfg, rows[i]))
        o.reset(tg[i])
        oracles.append(o)
    acts = np.random.default_rng(3).uniform(-22, 22, (T, n, n_arm * n_action)).astype(np.float32)
    for t in range(T):
        obs, rew, term, trunc = (x.cpu().numpy() for x in be.step(acts[t]))
        for i, o in enumerate(oracles):
            ob, rw, te, tr = o.env_step(acts[t, i])
            np.testing.assert_allclose(obs[i], _flat(ob), rtol=RTOL, atol=2e-7)
            np.testing.assert_allclose(rew[i], rw, rtol=RTOL, atol=1e-13 / (200 * cfg.dt) + 1e-9)
            assert bool(term[i]) == te and bool(trunc[i]) == tr
    _compare_octo_state(be, oracles)
    be.close()


def test_randomised_octo_first_full_step_matches_the_oracle(hip_lib, oracle_built):
    """The first whole OctoFlat env.step (2857 substeps from rest) per env against OracleOcto(cfg_i), at
    test_gpu_octo.py's tolerances; later whole steps are chaotic at rounding level.  Already
    within this step an env on a strongly rubbing ground can switch between stick and slip on a rounding difference:
    an env whose oracle and the oracle's FMA build (the rounding control) differ by more than a quarter band is held
    to ten times that difference instead (at most one of the six)."""
    n = 6
    env = gsa.make_vec("OctoFlat-v0", n, device=0)
    _randomise(env, _draw(n, 31))
    env.reset(seed=5)
    tg = _targets(n, 5)
    rows = env.backend.env_contact()
    acts = np.random.default_rng(9).uniform(-22, 22, (n, 24)).astype(np.float32)
    obs, rew, term, trunc, info = env.step(acts)
    obs, rew, term, trunc = (x.cpu().numpy() for x in (obs, rew, term, trunc))

    def err(x, ref, atol):
        return float(np.max(np.abs(np.asarray(x, np.float64) - ref) / (RTOL * np.abs(ref) + atol)))
    sensitive = 0
    for i in range(n):
        runs = []
        for variant in (False, "fma"):
            o = oracle_built.OracleOcto(_cfg_row(env.cfg, rows[i]), variant=variant)
            o.reset(tg[i])
            ob, rw, te, tr = o.env_step(acts[i])
            runs.append((_flat(ob), rw, te, tr))
        (ob, rw, te, tr), (obc, rwc, _, _) = runs
        sens = max(err(obc, ob, 2e-6), err(rwc, rw, 1e-7))
        band = 1.0
        if sens > 0.25:
            sensitive += 1
            band = 10.0 * sens
        assert err(obs[i], ob, 2e-6) <= band and err(rew[i], rw, 1e-7) <= band, (i, sens)
        assert bool(term[i]) == te and bool(trunc[i]) == tr
    assert sensitive <= 1
    env.close()


# ---- untouched envs, persistence -------------------------------------------------------------------------------
ENVS = ["OctoArmSingle-v0", "OctoFlat-v0"]


@pytest.mark.parametrize("env_id", ENVS)
def test_untouched_envs_are_bit_identical_to_a_uniform_batch(hip_lib, env_id):
    n, T = 9, 2
    uni, rnd = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    mask = np.ones(n, bool)
    mask[[0, n // 2, n - 1]] = False                                  # first, middle and last env keep the config
    _randomise(rnd, _draw(n, 3), mask)
    uni.reset(seed=9)
    rnd.reset(seed=9)
    for a in _acts(uni, T, 4):
        for x, y in zip(_outputs(uni, a), _outputs(rnd, a)):
            assert x[~mask].tobytes() == y[~mask].tobytes()
            if x.dtype.kind == "f":
                assert not np.array_equal(x[mask], y[mask])
    su, sr = _state(uni), _state(rnd)
    for k in ("position", "velocity", "director", "omega"):
        assert su[k][:, ~mask].tobytes() == sr[k][:, ~mask].tobytes(), k
    uni.close()
    rnd.close()


@pytest.mark.parametrize("env_id,final_time", [("OctoArmSingle-v0", 0.02), ("OctoFlat-v0", 0.4)])
def test_device_autoreset_equals_host_autoreset(hip_lib, env_id, final_time):
    n, T = 8, 5
    outs = []
    for mode in ("host", "device"):
        env = gsa.make_vec(env_id, n, autoreset=mode, final_time=final_time)
        _randomise(env, _draw(n, 8))
        env.reset(seed=4)
        outs.append([_outputs(env, a) for a in _acts(env, T, 6)])
        np.testing.assert_array_equal(env.backend.env_contact(), _rows(env.cfg, _draw(n, 8)))   # kept through resets
        env.close()
    assert any(s[3].any() for s in outs[0]), "no episode ended: the auto-reset was not exercised"
    for x, y in zip(*outs):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("env_id", ENVS)
def test_masked_update_between_steps_changes_only_those_envs_from_the_next_step(hip_lib, env_id):
    n = 6
    a_env, b_env = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    for e in (a_env, b_env):
        _randomise(e, _draw(n, 1))
        e.reset(seed=0)
    acts = _acts(a_env, 3, 7)
    for e in (a_env, b_env):
        e.step(acts[0])
    mask = np.array([0, 1, 0, 0, 1, 0], bool)
    b_env.set_contact(mask, kinetic_mu=b_env.contact()["kinetic_mu"] * 3.0)
    assert _state(a_env)["position"].tobytes() == _state(b_env)["position"].tobytes()   # nothing moved yet
    for a in acts[1:]:
        xa, xb = _outputs(a_env, a), _outputs(b_env, a)
        assert xa[0][~mask].tobytes() == xb[0][~mask].tobytes()
        assert not np.array_equal(xa[0][mask], xb[0][mask])
    a_env.close()
    b_env.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_snapshot_restore_reproduces_the_rollout(hip_lib, env_id):
    n = 5
    env = gsa.make_vec(env_id, n)
    _randomise(env, _draw(n, 13))
    env.reset(seed=1)
    acts = _acts(env, 3, 8)
    env.step(acts[0])
    sd = env.state_dict()
    assert "env_contact" in sd["backend"]
    want = env.contact()
    first = [_outputs(env, a) for a in acts[1:]]
    env.set_contact(contact_k=5.0, kinetic_mu=0.0)          # the restore must bring back the snapshot's ground
    env.load_state_dict(sd)
    for k in want:
        np.testing.assert_array_equal(env.contact()[k], want[k])
    again = [_outputs(env, a) for a in acts[1:]]
    for x, y in zip(first, again):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    del sd["backend"]["env_contact"]                         # a snapshot without the key: the config's values
    env.load_state_dict(sd)
    np.testing.assert_array_equal(env.backend.env_contact(), np.tile(_capi.env_contact_defaults(env.cfg), (n, 1)))
    env.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_captured_graph_matches_eager_and_sees_in_place_updates(hip_lib, env_id):
    n = 8
    eager, graphed = gsa.make_vec(env_id, n), gsa.make_vec(env_id, n)
    W = torch.randn(eager.obs_dim, eager.action_dim, device="cuda", dtype=torch.float32) * 0.1

    def policy(obs):
        return torch.tanh(obs @ W) * 6.0

    d = _draw(n, 17)
    for e in (eager, graphed):
        _randomise(e, d)
        e.reset(seed=3)
    replay = graphed.capture_policy_step(policy)
    for t in range(4):
        if t == 2:                                           # in-place update between replays, on the env's stream
            for e in (eager, graphed):
                e.set_contact(np.arange(n) % 3 == 0, friction_multiplier=4.0, friction_symmetry=True)
        obs_e, rew_e, te, tr, _ = eager.step(policy(eager.backend.obs))
        obs_g, rew_g, tg, trg = replay()
        assert obs_e.cpu().numpy().tobytes() == obs_g.cpu().numpy().tobytes()
        assert rew_e.cpu().numpy().tobytes() == rew_g.cpu().numpy().tobytes()
    eager.close()
    graphed.close()


# ---- a known answer --------------------------------------------------------------------------------------------
# On the CPU oracle (OracleRod, the arm of build_arm from rest, 4 env.steps of random actions in [-6, 6]) the
# horizontal centre of mass of an arm with kinetic_mu = static_mu = 0 moves by at most 6e-17 (every horizontal force
# on it is internal, the damper scales the momentum it has: none), while with the config's friction it moves by
# 1.1e-4 after one env.step and 1.4e-3 after four.  The bound below leaves the GPU's fast math four orders of
# magnitude of rounding and stays seven below the rubbing neighbours.
FRICTIONLESS_DRIFT_BOUND = 1e-12
RUBBING_DRIFT_FLOOR = 1e-6


def test_frictionless_envs_do_not_drift(hip_lib):
    n, T = 8, 3
    env = gsa.make_vec("OctoArmSingle-v0", n)
    slick = np.arange(n) % 2 == 0
    env.set_contact(slick, kinetic_mu=0.0, static_mu=0.0)
    env.reset(seed=0)
    w = np.full(int(env.cfg.n_elem) + 1, 1.0)
    w[0] = w[-1] = 0.5                                      # node masses of the uniform rod, up to one factor

    def com_xy():
        x = env.backend.state_numpy()["x"]                  # (N, 3, n + 1)
        return (x[:, :2] * w).sum(-1) / w.sum()
    c0 = com_xy()
    acts = _acts(env, T, 1)
    acts[:] = acts[:, :1]                                   # the same actions for every env
    for a in acts:
        env.step(a)
    drift = np.hypot(*(com_xy() - c0).T)
    print("drift", drift)
    assert drift[slick].max() < FRICTIONLESS_DRIFT_BOUND, drift
    assert drift[~slick].min() > RUBBING_DRIFT_FLOOR, drift
    env.close()


# ---- refusals --------------------------------------------------------------------------------------------------
REFUSED = [("SoftPendulum-v0", {}), ("SoftPendulum3D-v0", {}), ("SoftArmTracking-v0", {}), ("OctoArmPush-v1", {}),
           ("OctoCrawl-v0", {}), ("OctoArmSingle-v0", dict(n_elems=100)), ("OctoFlat-v0", dict(n_elems=20))]


@pytest.mark.parametrize("env_id,kw", REFUSED, ids=[r[0] + ("-" + str(r[1]["n_elems"]) if r[1] else "") for r in REFUSED])
def test_out_of_scope_handles_refuse_at_the_c_abi(hip_lib, env_id, kw):
    env = gsa.make_vec(env_id, 2, **kw)
    be = env.backend
    c = np.tile(_capi.env_contact_defaults(be.cfg), (2, 1))
    rc = hip_lib.softrod_set_env_contact(be._h, c.ctypes.data, None, be._stream())
    assert rc == EINVAL
    assert b"per-env contact" in hip_lib.softrod_last_error(be._h)
    assert not be.kernel_tier().endswith(",env contact")
    with pytest.raises(NotImplementedError):
        env.set_contact(contact_k=50.0)
    env.close()


def test_tapered_arm_and_bad_values_refuse_at_the_c_abi(hip_lib):
    edge = np.linspace(0.012, 0.001, 51)
    env = gsa.make_vec("OctoArmSingle-v0", 2, radius_profile=(edge[:-1] + edge[1:]) / 2)
    be = env.backend
    c = np.tile(_capi.env_contact_defaults(be.cfg), (2, 1))
    assert hip_lib.softrod_set_env_contact(be._h, c.ctypes.data, None, be._stream()) == EINVAL
    assert b"per-env contact" in hip_lib.softrod_last_error(be._h)
    env.close()
    env = gsa.make_vec("OctoArmSingle-v0", 2)
    be = env.backend
    for col, bad in ((0, np.nan), (1, -1.0), (2, -0.1), (7, np.inf), (4, -1e-12)):
        c = np.tile(_capi.env_contact_defaults(be.cfg), (2, 1))
        c[1, col] = bad
        assert hip_lib.softrod_set_env_contact(be._h, c.ctypes.data, None, be._stream()) == EINVAL
        mask = np.array([1, 0], np.uint8)                    # the bad row masked out: accepted
        assert hip_lib.softrod_set_env_contact(be._h, c.ctypes.data, mask.ctypes.data, be._stream()) == 0
    env.close()
