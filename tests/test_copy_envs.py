"""softrod_copy_envs without a GPU: the header declares it, the library exports it, _capi binds it, the ABI stays
17, and the argument normalisation of backend.copy_envs / env.fork (a pure function, _capi.copy_envs_pairs)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from gym_softrobot_amd import _capi

ROOT = Path(__file__).resolve().parents[1]


def test_header_declares_copy_envs_and_abi_stays_17():
    header = (ROOT / "include" / "softrod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+softrod_copy_envs\(softrod_handle\*\s*h,\s*const int32_t\*\s*src,\s*const int32_t\*\s*dst,"
                     r"\s*int count,\s*void\*\s*stream\);", code)
    assert "#define SOFTROD_ABI_VERSION 17" in header
    assert _capi.ABI_VERSION == 17
    # the comment names what it replaces, what is copied and every refusal
    doc = header[header.index("Fork resident envs on the device"):header.index("int softrod_copy_envs(")]
    for word in ("snapshot()", "restore()", "NOT graph-capturable", "muscle_activation", "prev_kappa", "sucker_index",
                 "softrod_set_env_material", "softrod_set_env_contact", "copy envs: null handle",
                 "copy envs: null src or dst", "copy envs: count", "copy envs: env index", "appears twice in dst",
                 "is the dst of one pair and the src of another", "device-side auto-reset"):
        assert word in doc, word


def test_capi_binds_copy_envs(hip_lib):
    assert "softrod_copy_envs" in _capi.EXPORTED_SYMBOLS
    fn = hip_lib.softrod_copy_envs
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert hip_lib.softrod_abi_version() == 17


def test_null_handle_is_refused_before_any_device_is_needed(hip_lib):
    pair = np.zeros(1, np.int32)
    assert hip_lib.softrod_copy_envs(None, pair.ctypes.data, pair.ctypes.data, 1, None) == -1
    assert hip_lib.softrod_last_error(None) == b"copy envs: null handle"


def test_pairs_scalar_src_broadcasts_over_dst():
    s, d = _capi.copy_envs_pairs(0, range(1, 5))
    assert s.dtype == d.dtype == np.int32 and s.flags.c_contiguous and d.flags.c_contiguous
    assert s.tolist() == [0, 0, 0, 0] and d.tolist() == [1, 2, 3, 4]
    s, d = _capi.copy_envs_pairs(np.int64(3), [5])
    assert s.tolist() == [3] and d.tolist() == [5]
    s, d = _capi.copy_envs_pairs(2, 4)                      # two scalars: one pair
    assert s.tolist() == [2] and d.tolist() == [4]


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64, np.uint16])
def test_pairs_take_any_integer_dtype(dtype):
    s, d = _capi.copy_envs_pairs(np.array([0, 0, 3], dtype), np.array([1, 2, 5], dtype))
    assert s.dtype == d.dtype == np.int32
    assert s.tolist() == [0, 0, 3] and d.tolist() == [1, 2, 5]


def test_pairs_take_lists_tuples_and_tensors():
    torch = pytest.importorskip("torch")
    s, d = _capi.copy_envs_pairs([0, 0, 3], (1, 2, 5))
    assert s.tolist() == [0, 0, 3] and d.tolist() == [1, 2, 5]
    s, d = _capi.copy_envs_pairs(torch.tensor([4, 1]), torch.tensor([0, 2], dtype=torch.int32))
    assert s.dtype == d.dtype == np.int32 and s.tolist() == [4, 1] and d.tolist() == [0, 2]


def test_pairs_empty_is_an_empty_call():
    s, d = _capi.copy_envs_pairs([], [])
    assert s.shape == d.shape == (0,) and s.dtype == d.dtype == np.int32
    s, d = _capi.copy_envs_pairs(0, [])
    assert s.shape == d.shape == (0,)


def test_pairs_negative_and_large_indices_pass_through_for_the_library_to_refuse():
    s, d = _capi.copy_envs_pairs([-1, 7], [1, 10**6])
    assert s.tolist() == [-1, 7] and d.tolist() == [1, 10**6]


@pytest.mark.parametrize("src,dst,what", [
    ([0, 1], [2], "src has 2 entries, dst has 1"),
    ([0], [1, 2], "src has 1 entries, dst has 2"),
    ([], [1], "src has 0 entries, dst has 1"),
    ([0.0], [1], "src must hold integers"),
    ([0], [1.5], "dst must hold integers"),
    ([True], [1], "src must hold integers"),
    ([[0, 1]], [[2, 3]], "one-dimensional"),
    ([2**31], [1], "does not fit an int32"),
])
def test_pairs_refuse_what_is_not_index_arrays_of_one_length(src, dst, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        _capi.copy_envs_pairs(src, dst)


def test_docs_describe_the_call():
    for name, words in (("README.md", ("fork(",)), ("DESIGN.md", ("softrod_copy_envs", "copy_envs_cost.json")),
                        ("INTEGRATION.md", ("softrod_copy_envs",))):
        text = (ROOT / name).read_text()
        for w in words:
            assert w in text, (name, w)
