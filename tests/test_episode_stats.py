"""Episode statistics without a GPU: known answers of the NumPy twin (tests/episode_stats_ref.py) worked out by hand in
all three modes, more finished envs than ring slots in one call, the ring wrapping, the manual-mode latch; the header
declares the four entry points, the library exports them and refuses a null handle; an env on a backend without the
feature refuses, a negative length is a ValueError."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from gym_softrobot_amd.diagnostics import EpisodeStatistics, episode_ring_order
from tests.episode_stats_ref import MANUAL, NEXT_STEP, SAME_STEP, EpisodeStatsRef
from tests.oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("softrod_episode_stats_enable", "softrod_episode_stats_update", "softrod_episode_stats_reset",
         "softrod_episode_stats_view")
KW = dict(final_time=5e-4, time_step=1e-4, recording_fps=5000, n_elems=6)

# three envs, four calls: env 0 ends on call 1, env 1 on call 2 (truncated), env 2 never; powers of two add exactly
REWARD = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0], [64.0, 128.0, 256.0], [512.0, 1024.0, 2048.0]])
TERM = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]], np.uint8)
TRUNC = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8)
TIME = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3], [0.4, 0.4, 0.4]])


def _run(mode, ring=4):
    ref, rows = EpisodeStatsRef(3, ring), []
    for c in range(4):
        ref.update(REWARD[c], TERM[c], TRUNC[c], TIME[c], mode)
        rows.append((ref.ep_r.copy(), ref.ep_l.copy(), ref.ep_t.copy(), ref.ep_mask.copy()))
    return ref, rows


def test_known_answers_same_step():
    ref, rows = _run(SAME_STEP)
    assert [r[3].tolist() for r in rows] == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert rows[1][0].tolist() == [9.0, 0.0, 0.0] and rows[1][1].tolist() == [2, 0, 0] and rows[1][2].tolist() == [0.2, 0.0, 0.0]
    assert rows[2][0].tolist() == [0.0, 146.0, 0.0] and rows[2][1].tolist() == [0, 3, 0] and rows[2][2].tolist() == [0.0, 0.3, 0.0]
    # the next episode starts with the next call: env 0 has 64 + 512 behind it, env 1 1024, env 2 everything
    assert ref.acc_return.tolist() == [576.0, 1024.0, 2340.0] and ref.acc_length.tolist() == [2, 1, 4]
    assert ref.latch.tolist() == [0, 0, 0] and ref.finished.tolist() == [1, 1, 0] and ref.count == 2
    assert ref.ring_r.tolist() == [9.0, 146.0, 0.0, 0.0] and ref.ring_env.tolist() == [0, 1, 0, 0]
    assert ref.ring_l.tolist() == [2, 3, 0, 0] and ref.ring_t.tolist() == [0.2, 0.3, 0.0, 0.0]


def test_known_answers_next_step():
    ref, rows = _run(NEXT_STEP)
    assert [r[3].tolist() for r in rows] == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert rows[1][0].tolist() == [9.0, 0.0, 0.0] and rows[2][0].tolist() == [0.0, 146.0, 0.0]
    # call 2 was env 0's reset call and call 3 env 1's: counted in no episode
    assert ref.acc_return.tolist() == [512.0, 0.0, 2340.0] and ref.acc_length.tolist() == [1, 0, 4]
    assert ref.latch.tolist() == [0, 0, 0] and ref.count == 2
    assert ref.ring_r.tolist() == [9.0, 146.0, 0.0, 0.0]


def test_known_answers_manual_and_the_latch_until_reset():
    ref, rows = _run(MANUAL)
    assert [r[3].tolist() for r in rows] == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert rows[1][0].tolist() == [9.0, 0.0, 0.0] and rows[2][0].tolist() == [0.0, 146.0, 0.0]
    # a finished env is ignored until it is reset
    assert ref.latch.tolist() == [1, 1, 0] and ref.acc_return.tolist() == [0.0, 0.0, 2340.0]
    assert ref.acc_length.tolist() == [0, 0, 4] and ref.count == 2
    ref.update([1.0, 1.0, 1.0], [1, 1, 0], [0, 0, 0], None, MANUAL)
    assert ref.count == 2 and ref.ep_mask.tolist() == [0, 0, 0] and ref.latch.tolist() == [1, 1, 0]
    ref.reset([True, False, True])              # env 0 unlatched, env 2's partial episode discarded
    assert ref.latch.tolist() == [0, 1, 0] and ref.acc_return.tolist() == [0.0, 0.0, 0.0] and ref.acc_length.tolist() == [0, 0, 0]
    assert ref.count == 2 and ref.finished.tolist() == [1, 1, 0] and ref.ring_r.tolist() == [9.0, 146.0, 0.0, 0.0]
    ref.update([3.0, 3.0, 3.0], [1, 1, 1], [0, 0, 0], None, MANUAL)
    assert ref.ep_mask.tolist() == [1, 0, 1] and ref.ep_r.tolist() == [3.0, 0.0, 3.0] and ref.ep_t.tolist() == [0.0, 0.0, 0.0]
    assert ref.count == 4 and ref.ring_env.tolist() == [0, 1, 0, 2] and ref.finished.tolist() == [2, 1, 1]


def test_more_finished_envs_than_slots_in_one_call():
    ref = EpisodeStatsRef(7, 3)
    ref.update(np.arange(7.0), np.ones(7, np.uint8), np.zeros(7, np.uint8), None, SAME_STEP)
    # seven sequential pushes into three slots: episodes 4, 5, 6 survive, episode c in slot c % 3
    assert ref.count == 7 and ref.ring_env.tolist() == [6, 4, 5] and ref.ring_r.tolist() == [6.0, 4.0, 5.0]
    assert [a.tolist() for a in ref.recent()][3] == [4, 5, 6]
    assert episode_ring_order(7, 3).tolist() == [1, 2, 0]


def test_the_ring_wraps():
    ref = EpisodeStatsRef(2, 3)
    for c in range(4):                           # env 1 ends every call, env 0 on calls 1 and 3
        ref.update([1.0, 10.0 + c], [c % 2, 1], [0, 0], [c, c], SAME_STEP)
    # pushes: (1: 10) (0: 2, 1: 11) (1: 12) (0: 2, 1: 13) -> episodes 0 .. 5, the last three in slots 0, 1, 2
    assert ref.count == 6 and ref.ring_r.tolist() == [12.0, 2.0, 13.0] and ref.ring_env.tolist() == [1, 0, 1]
    r, l, t, e = ref.recent()
    assert r.tolist() == [12.0, 2.0, 13.0] and l.tolist() == [1, 2, 1] and t.tolist() == [2.0, 3.0, 3.0] and e.tolist() == [1, 0, 1]
    assert episode_ring_order(6, 3).tolist() == [0, 1, 2] and episode_ring_order(2, 3).tolist() == [0, 1]
    assert episode_ring_order(0, 3).size == 0 and episode_ring_order(4, 3).tolist() == [1, 2, 0]


def test_header_declares_the_entry_points_and_abi_stays_17():
    header = (ROOT / "include" / "softrod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+softrod_episode_stats_enable\(softrod_handle\*\s*h,\s*int ring\);", code)
    assert re.search(r"int\s+softrod_episode_stats_update\(softrod_handle\*\s*h,\s*const double\*\s*reward,\s*const uint8_t\*\s*"
                     r"terminated,\s*const uint8_t\*\s*truncated,\s*const double\*\s*end_time,\s*int mode,\s*void\*\s*stream\);", code)
    assert re.search(r"int\s+softrod_episode_stats_reset\(softrod_handle\*\s*h,\s*const uint8_t\*\s*mask,\s*void\*\s*stream\);", code)
    assert re.search(r"int\s+softrod_episode_stats_view\(softrod_handle\*\s*h,\s*struct softrod_episode_stats_view\*\s*out\);", code)
    assert "#define SOFTROD_ABI_VERSION 17" in header and _capi.ABI_VERSION == 17
    doc = header[header.index("EPISODE STATISTICS"):header.index("struct softrod_episode_stats_view {")]
    for word in ("No reference counterpart: upstream has a single env and no statistics", "ceil(n_envs / 1024)",
                 "ascending env index", "episode stats: null handle", "is negative", "the feature is off",
                 "null reward, terminated or truncated", "is outside 0 .. 2", "capturable"):
        assert word in doc, word
    fields = re.findall(r"\b(\w+);", code[code.index("struct softrod_episode_stats_view {"):code.index("int softrod_episode_stats_enable")])
    assert fields[:-2] == [n for n, _, _ in _capi.EPISODE_STATS_ARRAYS] and fields[-2:] == ["n_envs", "ring"]
    assert [n for n, _ in _capi.SoftrodEpisodeStatsView._fields_] == fields


def test_capi_binds_them_and_a_null_handle_is_refused(hip_lib):
    for name in NAMES:
        assert name in _capi.EXPORTED_SYMBOLS and getattr(hip_lib, name).restype is C.c_int
    one = np.zeros(1)
    assert hip_lib.softrod_episode_stats_enable(None, 4) == -1
    assert hip_lib.softrod_last_error(None) == b"episode stats: null handle"
    assert hip_lib.softrod_episode_stats_update(None, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, 0, None) == -1
    assert hip_lib.softrod_episode_stats_reset(None, None, None) == -1
    assert hip_lib.softrod_episode_stats_view(None, C.byref(_capi.SoftrodEpisodeStatsView())) == -1
    assert hip_lib.softrod_last_error(None) == b"episode stats: null handle"


def test_env_refuses_off_the_hip_backend_and_a_negative_length():
    env = gsa.VecSoftPendulumEnv(2, backend=OracleBackend(_capi.softpendulum_config(2, **KW)), **KW)
    with pytest.raises(NotImplementedError, match="episode statistics need the HIP backend, not OracleBackend"):
        env.record_episode_statistics()
    with pytest.raises(ValueError, match="buffer_length -1 is negative"):
        env.record_episode_statistics(-1)
    with pytest.raises(_capi.SoftrodError, match="episode statistics are off"):
        env.episode_statistics()
    env.reset(seed=0)
    assert "episode" not in env.step(np.zeros((2, 1), np.float32))[4]
    assert EpisodeStatistics._fields == ("count", "returns", "lengths", "times", "envs", "finished")
    assert gsa.EpisodeStatistics is EpisodeStatistics
