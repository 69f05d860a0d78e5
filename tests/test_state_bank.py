"""The state bank without a GPU: the header declares its four entry points, the library exports them, _capi binds
them, the ABI stays 17, the argument normalisation of bank_save / bank_load (a pure function, _capi.state_bank_pairs,
sharing copy_envs_pairs' code), fork()'s texts stand, and an env on a backend without bank_create refuses."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi
from tests.oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("softrod_bank_create", "softrod_bank_save", "softrod_bank_load", "softrod_bank_info")
KW = dict(final_time=5e-4, time_step=1e-4, recording_fps=5000, n_elems=6)


def test_header_declares_the_four_entry_points_and_abi_stays_17():
    header = (ROOT / "include" / "softrod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+softrod_bank_create\(softrod_handle\*\s*h,\s*int slots\);", code)
    assert re.search(r"int\s+softrod_bank_save\(softrod_handle\*\s*h,\s*const int32_t\*\s*envs,\s*const int32_t\*\s*slots,"
                     r"\s*int count,\s*void\*\s*stream\);", code)
    assert re.search(r"int\s+softrod_bank_load\(softrod_handle\*\s*h,\s*const int32_t\*\s*slots,\s*const int32_t\*\s*envs,"
                     r"\s*int count,\s*void\*\s*stream\);", code)
    assert re.search(r"int\s+softrod_bank_info\(softrod_handle\*\s*h,\s*int32_t\*\s*slots,\s*uint64_t\*\s*bytes_per_slot,"
                     r"\s*uint8_t\*\s*filled\);", code)
    assert "#define SOFTROD_ABI_VERSION 17" in header
    assert _capi.ABI_VERSION == 17
    # the comments name what the bank replaces, the rule for arrays created later, and every refusal
    doc = header[header.index("State bank:"):header.index("int softrod_bank_info(")]
    for word in ("snapshot()", "restore()", "NOT graph-capturable", "softrod_copy_envs", "softrod_set_env_material",
                 "softrod_set_reset_shapes", "had nothing touched it since the save", "max(n_envs, slots)",
                 "bank create: null handle", "already has a state bank", "is not positive", "SOFTROD_ENOMEM",
                 "device-side auto-reset", "bank save: null handle", "has no state bank", "bank save: count",
                 "null envs or slots", "bank save: env index", "bank save: slot index", "appears twice",
                 "bank load: count", "holds no state", "bank load: env"):
        assert word in doc, word


def test_capi_binds_them(hip_lib):
    for name in NAMES:
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(hip_lib, name).restype is C.c_int
    assert hip_lib.softrod_bank_create.argtypes == [C.c_void_p, C.c_int]
    for name in ("softrod_bank_save", "softrod_bank_load"):
        assert getattr(hip_lib, name).argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert hip_lib.softrod_bank_info.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_void_p]
    assert hip_lib.softrod_abi_version() == 17


def test_null_handle_is_refused_before_any_device_is_needed(hip_lib):
    one = np.zeros(1, np.int32)
    assert hip_lib.softrod_bank_create(None, 4) == -1
    assert hip_lib.softrod_last_error(None) == b"bank create: null handle"
    assert hip_lib.softrod_bank_save(None, one.ctypes.data, one.ctypes.data, 1, None) == -1
    assert hip_lib.softrod_last_error(None) == b"bank save: null handle"
    assert hip_lib.softrod_bank_load(None, one.ctypes.data, one.ctypes.data, 1, None) == -1
    assert hip_lib.softrod_last_error(None) == b"bank load: null handle"
    slots, nbytes = C.c_int32(), C.c_uint64()
    assert hip_lib.softrod_bank_info(None, C.byref(slots), C.byref(nbytes), None) == -1
    assert hip_lib.softrod_last_error(None) == b"bank info: null handle"


def test_pairs_coerce_as_copy_envs_pairs_does():
    e, s = _capi.state_bank_pairs([1, 4], (3, 0), ("envs", "slots"))
    assert e.dtype == s.dtype == np.int32 and e.flags.c_contiguous and s.flags.c_contiguous
    assert e.tolist() == [1, 4] and s.tolist() == [3, 0]
    s, e = _capi.state_bank_pairs(2, range(5), ("slots", "envs"))          # one slot into every env
    assert s.tolist() == [2] * 5 and e.tolist() == [0, 1, 2, 3, 4]
    s, e = _capi.state_bank_pairs(np.int64(3), 5, ("slots", "envs"))       # two scalars: one pair
    assert s.tolist() == [3] and e.tolist() == [5]
    for dtype in (np.int8, np.int32, np.int64, np.uint16):
        e, s = _capi.state_bank_pairs(np.array([0, 0, 3], dtype), np.array([1, 2, 5], dtype), ("envs", "slots"))
        assert e.dtype == s.dtype == np.int32 and e.tolist() == [0, 0, 3] and s.tolist() == [1, 2, 5]
    e, s = _capi.state_bank_pairs([], [], ("envs", "slots"))
    assert e.shape == s.shape == (0,) and e.dtype == np.int32
    e, s = _capi.state_bank_pairs([-1, 7], [1, 10**6], ("envs", "slots"))  # the library's to refuse
    assert e.tolist() == [-1, 7] and s.tolist() == [1, 10**6]


def test_pairs_take_tensors():
    torch = pytest.importorskip("torch")
    s, e = _capi.state_bank_pairs(torch.tensor([4, 1]), torch.tensor([0, 2], dtype=torch.int32), ("slots", "envs"))
    assert s.dtype == e.dtype == np.int32 and s.tolist() == [4, 1] and e.tolist() == [0, 2]


@pytest.mark.parametrize("a,b,names,what", [
    ([0, 1], [2], ("envs", "slots"), "state_bank: envs has 2 entries, slots has 1"),
    ([0], [1, 2], ("slots", "envs"), "state_bank: slots has 1 entries, envs has 2"),
    ([], [1], ("envs", "slots"), "state_bank: envs has 0 entries, slots has 1"),
    ([0.0], [1], ("envs", "slots"), "state_bank: envs must hold integers, got dtype float64"),
    ([0], [1.5], ("envs", "slots"), "state_bank: slots must hold integers, got dtype float64"),
    ([True], [1], ("slots", "envs"), "state_bank: slots must hold integers, got dtype bool"),
    ([[0, 1]], [[2, 3]], ("envs", "slots"), "state_bank: envs must be a scalar or one-dimensional, got shape (1, 2)"),
    ([0], [2**31], ("envs", "slots"), "state_bank: slots does not fit an int32"),
])
def test_pairs_refuse_what_is_not_index_arrays_of_one_length(a, b, names, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        _capi.state_bank_pairs(a, b, names)


@pytest.mark.parametrize("src,dst,what", [
    ([0, 1], [2], "copy_envs: src has 2 entries, dst has 1"),
    ([0.0], [1], "copy_envs: src must hold integers, got dtype float64"),
    ([0], [1.5], "copy_envs: dst must hold integers, got dtype float64"),
    ([[0, 1]], [[2, 3]], "copy_envs: src must be a scalar or one-dimensional, got shape (1, 2)"),
    ([2**31], [1], "copy_envs: src does not fit an int32"),
])
def test_forks_error_texts_are_unchanged(src, dst, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        _capi.copy_envs_pairs(src, dst)


def test_a_backend_without_bank_create_refuses(oracle_built):
    env = gsa.VecSoftPendulumEnv(2, backend=OracleBackend(_capi.softpendulum_config(2, **KW)), **KW)
    for call, args in ((env.create_state_bank, (4,)), (env.save_states, ([0], [1])), (env.load_states, ([1], [0]))):
        with pytest.raises(NotImplementedError, match=f"{call.__name__} needs the HIP backend, not OracleBackend"):
            call(*args)
    assert env.state_bank_slots == 0 and env.state_bank_bytes == 0 and env.state_bank_filled.shape == (0,)


def test_device_autoreset_refuses_with_forks_wording(oracle_built):
    env = gsa.VecSoftPendulumEnv(2, backend=OracleBackend(_capi.softpendulum_config(2, **KW)), autoreset="device", **KW)
    with pytest.raises(NotImplementedError, match=re.escape("fork() with autoreset='device': staged reset records are not copied")):
        env.fork(0, [1])
    for call, args in ((env.create_state_bank, (4,)), (env.save_states, ([0], [1])), (env.load_states, ([1], [0]))):
        with pytest.raises(NotImplementedError, match=re.escape(f"{call.__name__}() with autoreset='device': staged reset "
                                                                "records are not copied")):
            call(*args)


def test_docs_describe_the_bank():
    for name, words in (("README.md", ("create_state_bank(", "state_bank_cost.json")),
                        ("DESIGN.md", ("softrod_bank_save", "state_bank_cost.json")),
                        ("INTEGRATION.md", NAMES)):
        text = (ROOT / name).read_text()
        for w in words:
            assert w in text, (name, w)
