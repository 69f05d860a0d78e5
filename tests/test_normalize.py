"""Observation and reward normalisation without a GPU: the NumPy twin (tests/normalize_ref.py) against np.mean / np.var
over everything it counted; non-finite elements and uncounted rows leave the other columns' records bitwise alone; the
row rules of the three modes by hand; the header declares the five entry points, the library exports them and returns
its refusals with no device; set_normalization validates its arguments."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import NormalizationState
from tests.normalize_ref import MANUAL, NEXT_STEP, SAME_STEP, NormalizeRef, column_update, osum
from tests.oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("softrod_normalize_enable", "softrod_normalize_step", "softrod_normalize_reset", "softrod_normalize_view",
         "softrod_normalize_load")
KW = dict(final_time=5e-4, time_step=1e-4, recording_fps=5000, n_elems=6)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def test_osum_is_the_fixed_order_sum():
    """37 rows: partial p adds rows p, p + 16, p + 32 from +0.0, the partials are added in ascending p from +0.0 —
    written out as a plain loop."""
    x = np.random.default_rng(0).standard_normal((37, 3)) * 10.0 ** np.arange(3)
    want = np.zeros(3)
    parts = []
    for p in range(16):
        s = np.zeros(3)
        for e in range(p, 37, 16):
            s = s + x[e]
        parts.append(s)
    for s in parts:
        want = want + s
    assert np.array_equal(_bits(osum(x)), _bits(want))
    assert np.array_equal(_bits(osum(x[:, 0])), _bits(want[0]))
    assert np.array_equal(_bits(osum(np.full((3, 2), -0.0))), _bits(np.zeros(2)))       # +0.0 + -0.0 = +0.0
    assert np.array_equal(_bits(osum(np.zeros((0, 2)))), _bits(np.zeros(2)))


def test_twin_agrees_with_numpy_over_everything_it_counted():
    """30 updates of seeded data, 2000 rows by 5 columns each (6e4 terms per column): mean and var equal np.mean /
    np.var over all counted rows with the initial pseudo-count of 1e-4 at mean 0, var 1 folded in, to relative 1e-10 —
    two orders over n * eps for 6e4 float64 terms; a sanity bound on the formula."""
    rng = np.random.default_rng(1)
    n, d, calls = 2000, 5, 30
    ref = NormalizeRef(n, d)
    seen_obs = []
    for c in range(calls):
        obs = (rng.standard_normal((n, d)) * [1.0, 10.0, 0.1, 3.0, 100.0] + [0.0, 5.0, -2.0, 100.0, -1e3]).astype(np.float32)
        reward = rng.standard_normal(n) + 0.5
        done = rng.random(n) < 0.05
        ref.step(obs, reward, done, np.zeros(n, bool), mode=SAME_STEP)
        seen_obs.append(obs.astype(np.float64))
    x = np.concatenate(seen_obs)

    def folded(values):          # the pseudo-count: 1e-4 observations at mean 0, var 1 (second moment 1)
        w, m = float(len(values)), values.mean(axis=0)
        tot = w + 1e-4
        mean = m * w / tot
        second = ((values ** 2).mean(axis=0) * w + 1e-4 * 1.0) / tot
        return mean, second - mean ** 2, tot

    mean, var, tot = folded(x)
    assert np.allclose(ref.obs_mean, mean, rtol=1e-10, atol=0.0)
    assert np.allclose(ref.obs_var, var, rtol=1e-10, atol=0.0)
    assert np.allclose(ref.obs_count, tot, rtol=1e-12, atol=0.0) and np.isclose(ref.ret_count[0], tot, rtol=1e-12, atol=0.0)
    assert np.array_equal(_bits(ref.obs_inv_std), _bits(1.0 / np.sqrt(ref.obs_var + 1e-8)))


def test_the_return_column_follows_the_discounted_returns():
    """The same check for the return: replay ret = ret * gamma + r by hand, with ret = 0 after an episode end."""
    rng = np.random.default_rng(2)
    n, calls, gamma = 500, 30, 0.9
    ref = NormalizeRef(n, 2, gamma=gamma)
    ret, seen = np.zeros(n), []
    for c in range(calls):
        reward, done = rng.standard_normal(n) + 1.0, rng.random(n) < 0.1
        ref.step(np.zeros((n, 2), np.float32), reward, done, np.zeros(n, bool), mode=SAME_STEP)
        ret = ret * gamma + reward
        seen.append(ret.copy())
        ret[done] = 0.0
        assert np.array_equal(_bits(ref.ret), _bits(ret))
    v = np.concatenate(seen)
    w, tot = float(v.size), v.size + 1e-4
    mean = v.mean() * w / tot
    var = ((v ** 2).mean() * w + 1e-4) / tot - mean ** 2
    assert np.isclose(ref.ret_mean[0], mean, rtol=1e-10, atol=0.0) and np.isclose(ref.ret_var[0], var, rtol=1e-10, atol=0.0)
    assert np.array_equal(_bits(ref.norm_reward), _bits(np.clip(reward * ref.ret_inv_std[0], -10.0, 10.0)))


def test_non_finite_elements_and_uncounted_rows_leave_the_other_records_bitwise_alone():
    rng = np.random.default_rng(3)
    n, d = 40, 4
    x = rng.standard_normal((n, d)).astype(np.float32)
    rec = (np.array([0.1, 0.2, 0.3, 0.4]), np.array([1.0, 2.0, 3.0, 4.0]), np.full(d, 7.0))
    clean = column_update(*rec, x, np.ones(n, bool), 1e-8)
    # NaN / inf in column 1 only: columns 0, 2, 3 must not move by a bit; column 1 counts 38 rows
    bad = x.copy()
    bad[5, 1], bad[17, 1] = np.nan, -np.inf
    got = column_update(*rec, bad, np.ones(n, bool), 1e-8)
    for a, b in zip(clean[:4], got[:4]):
        assert np.array_equal(_bits(a[[0, 2, 3]]), _bits(b[[0, 2, 3]]))
    assert got[2][1] == 7.0 + 38 and np.isfinite(got[0][1]) and np.isfinite(got[1][1])
    # an uncounted row equals a row of non-finite values: rows 5 and 17 out of every column
    counted = np.ones(n, bool)
    counted[[5, 17]] = False
    skipped = column_update(*rec, x, counted, 1e-8)
    nan_rows = x.copy()
    nan_rows[[5, 17]] = np.nan
    as_nan = column_update(*rec, nan_rows, np.ones(n, bool), 1e-8)
    for a, b in zip(skipped[:4], as_nan[:4]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(skipped[0][1]), _bits(got[0][1])) and np.array_equal(_bits(skipped[1][1]), _bits(got[1][1]))
    # nothing counted: the record stays
    none = column_update(*rec, x, np.zeros(n, bool), 1e-8)
    assert none[4].all() and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(none[:3], rec))


def test_outputs_clip_and_pass_nan():
    ref = NormalizeRef(3, 2, clip_obs=2.0, clip_reward=0.5)
    obs = np.array([[np.nan, 1.0], [np.inf, -np.inf], [100.0, -0.25]], np.float32)
    ref.step(obs, [np.nan, 3.0, -0.1], [0, 0, 0], [0, 0, 0], update=False)
    inv = 1.0 / np.sqrt(1.0 + 1e-8)
    assert _bits(ref.norm_obs)[0, 0] == 0x7FC00000 and ref.norm_obs[0, 1] == np.float32(1.0 * inv)
    assert ref.norm_obs[1].tolist() == [2.0, -2.0] and ref.norm_obs[2].tolist() == [2.0, float(np.float32(-0.25 * inv))]
    assert _bits(ref.norm_reward)[0] == 0x7FF8000000000000 and ref.norm_reward[1:].tolist() == [0.5, -0.1 * inv]
    assert ref.obs_count.tolist() == [1e-4, 1e-4] and ref.ret_count[0] == 1e-4 and not ref.ret.any()      # update=False


def test_row_rules_by_hand():
    """Three envs; env 0 ends on call 1.  Which rows each mode counts, by the counts alone."""
    obs = np.ones((3, 1), np.float32)
    flags = [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]]
    counts, refs = {}, {}
    for mode in (MANUAL, NEXT_STEP, SAME_STEP):
        ref = refs[mode] = NormalizeRef(3, 1, gamma=0.5)
        rows = []
        for c in range(4):
            ref.step(obs, [1.0, 1.0, 1.0], flags[c], [0, 0, 0], mode=mode)
            rows.append((round(ref.obs_count[0] - 1e-4), round(ref.ret_count[0] - 1e-4), ref.latch.tolist(), ref.ret.tolist()))
        counts[mode] = rows
    # SAME_STEP: every row and every reward counts, no latch; env 0's return restarts after call 1
    assert [r[:2] for r in counts[SAME_STEP]] == [(3, 3), (6, 6), (9, 9), (12, 12)]
    assert counts[SAME_STEP][3][2] == [0, 0, 0] and counts[SAME_STEP][3][3] == [1.5, 1.875, 1.875]
    # NEXT_STEP: call 2 is env 0's reset call: its row counts, its reward does not, the latch clears
    assert [r[:2] for r in counts[NEXT_STEP]] == [(3, 3), (6, 6), (9, 8), (12, 11)]
    assert counts[NEXT_STEP][1][2] == [1, 0, 0] and counts[NEXT_STEP][2][2] == [0, 0, 0]
    assert counts[NEXT_STEP][3][3] == [1.0, 1.875, 1.875]
    # MANUAL: env 0 is ignored until a reset names it
    assert [r[:2] for r in counts[MANUAL]] == [(3, 3), (6, 6), (8, 8), (10, 10)]
    assert counts[MANUAL][3][2] == [1, 0, 0] and counts[MANUAL][3][3] == [0.0, 1.875, 1.875]
    ref = refs[MANUAL]
    ref.reset(obs, [True, False, False])
    assert ref.latch.tolist() == [0, 0, 0] and round(ref.obs_count[0] - 1e-4) == 11 and round(ref.ret_count[0] - 1e-4) == 10
    # final_obs rows: only those of the envs that finished on the call are written
    ref = NormalizeRef(3, 1)
    ref.norm_final_obs[:] = 7.0
    fin = ref.step(obs, [0.0, 0.0, 0.0], [0, 1, 0], [0, 0, 0], final_obs=np.full((3, 1), 3.0, np.float32), mode=SAME_STEP)
    assert fin.tolist() == [False, True, False] and ref.norm_final_obs[[0, 2], 0].tolist() == [7.0, 7.0]
    assert ref.norm_final_obs[1, 0] != 7.0 and round(ref.obs_count[0] - 1e-4) == 3      # never counted


def test_header_declares_the_entry_points_and_abi_stays_17():
    header = (ROOT / "include" / "softrod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(rf"int\s+{name}\(softrod_handle\*\s*h,", code), name
    assert "#define SOFTROD_ABI_VERSION 17" in header and _capi.ABI_VERSION == 17
    fields = re.findall(r"\b(\w+);", code[code.index("struct softrod_normalize_view {"):code.index("int softrod_normalize_enable")])
    assert fields[:len(_capi.NORMALIZE_ARRAYS)] == [n for n, _, _ in _capi.NORMALIZE_ARRAYS]
    assert [n for n, _ in _capi.SoftrodNormalizeView._fields_] == fields
    doc = header[header.index("OBSERVATION AND REWARD NORMALISATION"):header.index("struct softrod_normalize_view {")]
    for word in ("null handle", "the feature is off", "is outside [0, 1]", "is not positive", "is outside 0 .. 2",
                 "final_obs needs mode 2", "null obs, reward, terminated or truncated", "capturable"):
        assert word in doc, word
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert all(name in integration for name in NAMES)


def test_capi_binds_them_and_refuses_with_no_device(hip_lib):
    for name in NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and getattr(hip_lib, name).restype is C.c_int
    err = lambda: hip_lib.softrod_last_error(None)      # noqa: E731
    one = np.zeros(4)
    p = one.ctypes.data
    assert hip_lib.softrod_normalize_enable(None, 1, 1, 0.99, 10.0, 10.0, 1e-8) == -1 and err() == b"normalize: null handle"
    for gamma in (-0.1, 1.5, float("nan")):
        assert hip_lib.softrod_normalize_enable(None, 1, 1, gamma, 10.0, 10.0, 1e-8) == -1
        assert err().endswith(b"is outside [0, 1]") and err().startswith(b"normalize: gamma")
    for args, text in (((0.0, 10.0, 1e-8), b"clip_obs 0"), ((10.0, -1.0, 1e-8), b"clip_reward -1"), ((10.0, 10.0, 0.0), b"epsilon 0")):
        assert hip_lib.softrod_normalize_enable(None, 1, 0, 0.5, *args) == -1
        assert err() == b"normalize: " + text + b" is not positive"
    assert hip_lib.softrod_normalize_enable(None, 0, 0, 7.0, -1.0, -1.0, -1.0) == -1 and err() == b"normalize: null handle"
    for mode in (-1, 3):
        assert hip_lib.softrod_normalize_step(None, p, p, p, p, None, mode, 1, None) == -1
        assert err() == f"normalize: mode {mode} is outside 0 .. 2".encode()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert hip_lib.softrod_normalize_step(None, *args, None, 0, 1, None) == -1
        assert err() == b"normalize: null obs, reward, terminated or truncated"
    for mode in (0, 1):
        assert hip_lib.softrod_normalize_step(None, p, p, p, p, p, mode, 1, None) == -1
        assert err() == b"normalize: final_obs needs mode 2"
    assert hip_lib.softrod_normalize_step(None, p, p, p, p, p, 2, 1, None) == -1 and err() == b"normalize: null handle"
    assert hip_lib.softrod_normalize_reset(None, None, None, 1, None) == -1 and err() == b"normalize: null obs"
    assert hip_lib.softrod_normalize_reset(None, p, None, 1, None) == -1 and err() == b"normalize: null handle"
    assert hip_lib.softrod_normalize_view(None, None) == -1 and err() == b"normalize: null argument"
    assert hip_lib.softrod_normalize_view(None, C.byref(_capi.SoftrodNormalizeView())) == -1 and err() == b"normalize: null handle"
    assert hip_lib.softrod_normalize_load(None, p, p, None, p, p, p, None) == -1 and err() == b"normalize: null argument"
    assert hip_lib.softrod_normalize_load(None, p, p, p, p, p, p, None) == -1 and err() == b"normalize: null handle"


def test_set_normalization_validates_its_arguments():
    env = gsa.VecSoftPendulumEnv(2, backend=OracleBackend(_capi.softpendulum_config(2, **KW)), **KW)
    for kw, text in ((dict(gamma=1.5), "gamma 1.5 is outside"), (dict(gamma=-0.1), "gamma -0.1 is outside"),
                     (dict(gamma=float("nan")), "gamma nan is outside"), (dict(clip_obs=0.0), "clip_obs 0.0 is not positive"),
                     (dict(clip_reward=-1.0), "clip_reward -1.0 is not positive"), (dict(epsilon=0.0), "epsilon 0.0 is not positive")):
        with pytest.raises(ValueError, match=text):
            env.set_normalization(**kw)
    with pytest.raises(TypeError):
        env.set_normalization(True, True, 0.9)              # gamma and the rest are keyword-only
    with pytest.raises(NotImplementedError, match="normalisation needs the HIP backend, not OracleBackend"):
        env.set_normalization()
    with pytest.raises(_capi.SoftrodError, match="normalisation is off"):
        env.normalization_state()
    with pytest.raises(_capi.SoftrodError, match="normalisation is off"):
        env.normalization_info
    assert env.normalization_training is True
    env.normalization_training = False
    assert env.normalization_training is False
    _, infos = env.reset(seed=0)
    assert "raw_obs" not in infos
    assert not {"raw_obs", "raw_reward"} & set(env.step(np.zeros((2, 1), np.float32))[4])
    assert NormalizationState._fields == ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")
    assert gsa.NormalizationState is NormalizationState
