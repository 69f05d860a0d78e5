"""set_reset_shapes() without a GPU: the C-ABI's additions (the library loads without a device), the index function on
both sides, and the env layer through a recording stand-in backend."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi

try:
    from tests import reset_shapes_ref as ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import reset_shapes_ref as ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"
EINVAL = -1
DECLARATIONS = (
    "int softrod_set_reset_shapes(softrod_handle* h, int count, const double* kappa, const double* sigma, const double* velocity,\n"
    "                             const double* omega, uint64_t seed, void* stream)",
    "int softrod_apply_reset_shapes(softrod_handle* h, const uint8_t* mask, void* stream)",
    "int softrod_reset_shapes_view(softrod_handle* h, int32_t** index, int32_t** episode)",
    "uint32_t softrod_reset_shape_index(uint64_t seed, uint32_t env, uint32_t episode, uint32_t count)",
)


# ---- 1. the interface --------------------------------------------------------------------------------------------------
def test_symbols_header_and_table(hip_lib):
    header = (ROOT / "include" / "softrod.h").read_text()
    source = (CSRC / "softrod_capi.hip").read_text()
    for d in DECLARATIONS:
        assert d + ";" in header, d
        assert d + " {" in source, d
    for words in ("straight_rod only", "x *= 0xBF58476D1CE4E5B9", "x *= 0x94D049BB133111EB", "0x9E3779B97F4A7C15 * (e + 1)",
                  "[[2,1,1],[2,2,1],[2,1,1],[0,2,2],[2,1,2],[1,2,0]]", "CAPTURE AGAIN", "[count][rods_per_env][3][n_elem - 1]",
                  "Starts that every reset repeats, automatic ones included, are softrod_set_reset_shapes'"):
        assert words in header, words
    names = ("softrod_set_reset_shapes", "softrod_apply_reset_shapes", "softrod_reset_shapes_view", "softrod_reset_shape_index")
    for name in names:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    vp = C.c_void_p
    assert hip_lib.softrod_set_reset_shapes.argtypes == [vp, C.c_int, vp, vp, vp, vp, C.c_uint64, vp]
    assert hip_lib.softrod_apply_reset_shapes.argtypes == [vp, vp, vp]
    assert hip_lib.softrod_reset_shapes_view.argtypes == [vp, C.POINTER(vp), C.POINTER(vp)]
    assert hip_lib.softrod_reset_shape_index.argtypes == [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    assert hip_lib.softrod_reset_shape_index.restype == C.c_uint32
    assert _capi.ABI_VERSION == 17 and hip_lib.softrod_abi_version() == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)
    # one shape kernel: the pool is an indirection of softrod_rod_shape_kernel, not a second kernel
    code = "".join(re.sub(r"//.*", "", p.read_text()) for p in sorted(CSRC.glob("*.hpp")))
    assert len(re.findall(r"\bsoftrod_rod_shape_kernel\s*\(", code)) == 1 and "pool_index" in code
    assert len(re.findall(r"softrod_rod_shape_kernel<1>", source)) == 2       # set_rod_shape's launch and the pass's


def test_refusals_are_found_before_a_device_is_needed(hip_lib):
    assert hip_lib.softrod_set_reset_shapes(None, 1, None, None, None, None, 0, None) == EINVAL
    assert hip_lib.softrod_last_error(None) == b"set reset shapes: null handle"
    assert hip_lib.softrod_apply_reset_shapes(None, None, None) == EINVAL
    assert hip_lib.softrod_last_error(None) == b"apply reset shapes: null handle"
    ix, ep = C.c_void_p(), C.c_void_p()
    assert hip_lib.softrod_reset_shapes_view(None, C.byref(ix), C.byref(ep)) == EINVAL
    assert hip_lib.softrod_last_error(None) == b"reset shapes view: null handle"
    source = (CSRC / "softrod_capi.hip").read_text()
    for d, texts in zip(DECLARATIONS[:3], (("null handle", "negative count"), ("null handle", "no pool is set"),
                                           ("null handle", "no pool is set"))):
        body = source[source.index(d + " {"):]
        body = body[:body.index("\n}\n")]
        device = body.index("SR_ON_DEVICE(h)") if "SR_ON_DEVICE(h)" in body else len(body)
        for t in texts:
            assert body.index(t) < device, (d, t)


# ---- 2. the index function ---------------------------------------------------------------------------------------------
def test_known_answers(hip_lib):
    e = np.arange(6)[:, None]
    j = np.arange(3)[None, :]
    assert gsa.reset_shape_index(ref.KNOWN_SEED, e, j, ref.KNOWN_K).tolist() == ref.KNOWN
    assert [[hip_lib.softrod_reset_shape_index(ref.KNOWN_SEED, a, b, ref.KNOWN_K) for b in range(3)] for a in range(6)] == ref.KNOWN
    assert [[ref.index(ref.KNOWN_SEED, a, b, ref.KNOWN_K) for b in range(3)] for a in range(6)] == ref.KNOWN
    assert gsa.reset_shape_index is _capi.reset_shape_index and isinstance(gsa.reset_shape_index(1, 0, 0, 3), int)


def test_library_and_numpy_agree(hip_lib):
    rng = np.random.default_rng(0)
    seeds = rng.integers(0, 2**64, 1000, dtype=np.uint64)
    seeds[:100] |= np.uint64(1 << 63)                                   # seeds above 2^63
    envs = rng.integers(0, 2**20, 1000)
    eps = rng.integers(0, 2**31, 1000)
    counts = rng.integers(1, 1000, 1000)
    counts[::7] = 1
    counts[3::11] = 2**32 - 1
    got = gsa.reset_shape_index(seeds, envs, eps, counts)
    assert got.shape == (1000,) and (got[counts == 1] == 0).all() and (got >= 0).all() and (got < counts).all()
    assert int((seeds > np.uint64(2**63)).sum()) >= 100
    for s, e, j, k, g in zip(seeds.tolist(), envs.tolist(), eps.tolist(), counts.tolist(), got.tolist()):
        assert hip_lib.softrod_reset_shape_index(s, e, j, k) == g == ref.index(s, e, j, k), (s, e, j, k)
    assert gsa.reset_shape_index(2**64 - 1, 5, 2, 7) == ref.index(2**64 - 1, 5, 2, 7)      # a Python int above 2^63


# ---- 3. the env layer ---------------------------------------------------------------------------------------------------
class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


class StubBackend:
    """Records what VecRodEnvBase hands to set_reset_shapes / apply_reset_shapes, in order, among the resets and
    observes around them."""

    def __init__(self, cfg):
        import torch

        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}
        self.calls = []
        self.device = torch.device("cpu")
        self.reset_shape_index = torch.full((self.n_envs,), -1, dtype=torch.int32)
        self.reset_shape_episode = torch.zeros((self.n_envs,), dtype=torch.int32)
        self.obs = torch.zeros((self.n_envs, _capi.config_obs_dim(cfg)), dtype=torch.float32)
        self.done = torch.zeros((self.n_envs,), dtype=torch.uint8)      # what the next step reports as truncated

    def set_reset_shapes(self, seed=0, **fields):
        self.calls.append(("set", seed, fields))
        return _capi.reset_shapes_pool(self.cfg, fields)

    def apply_reset_shapes(self, mask=None):
        self.calls.append(("apply", None if mask is None else np.array(mask, bool).tolist()))
        sel = np.ones(self.n_envs, bool) if mask is None else np.asarray(mask, bool)
        self.reset_shape_episode[np.nonzero(sel)[0].tolist()] += 1

    def observe(self, prev_action=None):
        self.calls.append(("observe",))
        return self.obs

    def step(self, a):
        import torch

        self.calls.append(("step",))
        return self.obs, torch.zeros(self.n_envs, dtype=torch.float64), torch.zeros(self.n_envs, dtype=torch.uint8), self.done.clone()

    def prev_action_rows(self):
        import torch

        return torch.zeros((self.n_envs, _capi.config_action_dim(self.cfg)))

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name.startswith("reset") or name.startswith("queue"):
            return lambda *a, **k: self.calls.append((name,))
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


def _kinds(calls):
    return [c[0] for c in calls]


def test_fields_reach_the_backend():
    env = _vec("SoftPendulum-v0", 3, StubBackend)
    ne = int(env.cfg.n_elem)
    kappa = np.zeros((4, 1, 3, ne - 1))
    sigma = np.zeros((4, 3, ne))                                        # the rods axis left out
    assert env.set_reset_shapes(kappa, sigma, seed=7) is None
    kind, seed, fields = env.backend.calls[-1]
    assert kind == "set" and seed == 7 and fields["kappa"] is kappa and fields["sigma"] is sigma
    assert fields["velocity"] is None and fields["omega"] is None and env._reset_shapes == 4
    env.set_reset_shapes(omega=np.zeros((1, 1, 3, ne)))                 # K = 1; keywords
    assert env._reset_shapes == 1 and env.backend.calls[-1][1] == 0
    env.set_reset_shapes()                                              # no field: the pool is cleared
    assert env._reset_shapes == 0 and all(v is None for v in env.backend.calls[-1][2].values())


@pytest.mark.parametrize("env_id,rods", [("SoftPendulum-v0", 1), ("OctoFlat-v0", 8), ("OctoArmTwo-v0", 2)])
def test_wrong_shapes_counts_and_dtypes_are_refused(env_id, rods):
    import torch

    env = _vec(env_id, 2, StubBackend)
    ne = int(env.cfg.n_elem)
    K = 3
    good = dict(kappa=(K, rods, 3, ne - 1), sigma=(K, rods, 3, ne), velocity=(K, rods, 3, ne + 1), omega=(K, rods, 3, ne))
    for name, shape in good.items():
        env.set_reset_shapes(**{name: np.zeros(shape)})
        env.set_reset_shapes(**{name: torch.zeros(shape, dtype=torch.float64)})
        bad = [np.zeros(shape[:-1] + (shape[-1] + 1,)), np.zeros(shape[:2] + (2,) + shape[3:]), np.zeros(shape[2:]),
               np.zeros(shape).reshape(-1), np.zeros((0,) + shape[1:]), np.zeros((K, rods + 1) + shape[2:])]
        if rods > 1:                    # the rods axis is optional for a one-rod env only; the pool axis never is
            bad += [np.zeros(shape[:1] + shape[2:]), np.zeros(shape[1:])]       # (one rod: (1, 3, w) is a pool of one)
        for v in bad:
            with pytest.raises(ValueError, match=f"set_reset_shapes: {name} must have shape"):
                env.set_reset_shapes(**{name: v})
        for v in (np.zeros(shape, np.float32), torch.zeros(shape, dtype=torch.float32), np.zeros(shape, np.int64)):
            with pytest.raises(ValueError, match=f"set_reset_shapes: {name} must be float64"):
                env.set_reset_shapes(**{name: v})
    calls = len(env.backend.calls)
    with pytest.raises(ValueError, match="set_reset_shapes: sigma has 2 pool entries, the fields before it 3"):
        env.set_reset_shapes(kappa=np.zeros(good["kappa"]), sigma=np.zeros((2,) + good["sigma"][1:]))
    assert len(env.backend.calls) == calls == 2 * len(good)             # a refused call never reaches the backend
    assert env._reset_shapes == K


def test_resets_apply_the_pool_between_the_reset_and_the_observe():
    n = 4
    env = _vec("SoftPendulum-v0", n, StubBackend, autoreset=True)
    be = env.backend
    ne = int(env.cfg.n_elem)
    env.reset(seed=0)
    assert "apply" not in _kinds(be.calls)                              # no pool: never called
    env.step(np.zeros((n, 1), np.float32))
    assert "apply" not in _kinds(be.calls)
    env.set_reset_shapes(np.zeros((2, 1, 3, ne - 1)))
    del be.calls[:]
    env.reset()
    kinds = _kinds(be.calls)
    assert kinds.count("apply") == 1 and be.calls[kinds.index("apply")][1] is None
    assert kinds.index("reset") < kinds.index("apply") < kinds.index("observe")
    del be.calls[:]
    m = np.array([False, True, True, False])
    env.reset(mask=m)
    kinds = _kinds(be.calls)
    assert kinds.count("apply") == 1 and be.calls[kinds.index("apply")][1] == m.tolist()
    assert kinds.index("reset") < kinds.index("apply") < kinds.index("observe")
    # the host-driven auto-reset: the envs that finished on the previous call
    be.done[:] = torch_u8([0, 0, 1, 1])
    env.step(np.zeros((n, 1), np.float32))
    be.done[:] = 0
    del be.calls[:]
    env.step(np.zeros((n, 1), np.float32))
    kinds = _kinds(be.calls)
    assert kinds.count("apply") == 1 and be.calls[kinds.index("apply")][1] == [False, False, True, True]
    assert kinds.index("step") < kinds.index("reset") < kinds.index("apply") < kinds.index("observe")
    del be.calls[:]
    env.step(np.zeros((n, 1), np.float32))                              # nobody finished: no reset, no apply
    assert _kinds(be.calls) == ["step"]
    env.set_reset_shapes()
    del be.calls[:]
    env.reset()
    assert "apply" not in _kinds(be.calls)                              # the pool is cleared


def torch_u8(values):
    import torch

    return torch.tensor(values, dtype=torch.uint8)


def test_reseeding_zeroes_the_ordinals():
    n = 4
    env = _vec("SoftPendulum-v0", n, StubBackend)
    be = env.backend
    env.set_reset_shapes(np.zeros((2, 1, 3, int(env.cfg.n_elem) - 1)))
    env.reset(seed=0)
    env.reset()
    env.reset(mask=np.array([True, False, False, False]))
    assert be.reset_shape_episode.tolist() == [3, 2, 2, 2]              # the stand-in counts what apply is handed
    env.reset(seed=[None, 5, None, 6], mask=np.array([True, True, False, True]))
    assert be.reset_shape_episode.tolist() == [4, 1, 2, 1]              # the re-seeded envs start their sequence again
    env.reset(seed=9)
    assert be.reset_shape_episode.tolist() == [1, 1, 1, 1]


def test_arm_two_observes_the_reset_before_it_is_shaped():
    """ArmTwoEnv's get_state moves _prev_kappa: reset() followed by set_rod_shape() observes twice, and so does a shaped
    reset."""
    env = _vec("OctoArmTwo-v0", 2, StubBackend)
    ne = int(env.cfg.n_elem)
    env.set_reset_shapes(np.zeros((2, 2, 3, ne - 1)))
    del env.backend.calls[:]
    env.reset(seed=0)
    kinds = [k for k in _kinds(env.backend.calls) if k in ("observe", "apply")]
    assert kinds == ["observe", "apply", "observe"]


def test_oracle_backend_has_no_set_reset_shapes(oracle_built):
    env = _vec("SoftPendulum-v0", 2, OracleBackend)
    with pytest.raises(NotImplementedError, match="set_reset_shapes needs the HIP backend, not OracleBackend"):
        env.set_reset_shapes()


def test_single_env_shell_keeps_the_pool_axis():
    from gym_softrobot_amd.envs.octo_flat import FlatEnv
    from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

    for cls, rods in ((SoftPendulumEnv, 1), (FlatEnv, 8)):
        probe = cls(backend=_Probe())
        env = cls(backend=StubBackend(probe._vec.cfg))
        be = env._vec.backend
        ne = int(env._vec.cfg.n_elem)
        env.set_reset_shapes(np.zeros((5, rods, 3, ne - 1)), seed=3)
        assert be.calls[-1][1] == 3 and be.calls[-1][2]["kappa"].shape == (5, rods, 3, ne - 1)
        if rods == 1:
            env.set_reset_shapes(sigma=np.zeros((2, 3, ne)))            # the rods axis is optional, the pool axis is not
            assert be.calls[-1][2]["sigma"].shape == (2, 3, ne)
        with pytest.raises(ValueError, match="must have shape"):
            env.set_reset_shapes(omega=np.zeros((rods, 3, ne)) if rods > 1 else np.zeros((3, ne)))
        assert env.reset_shape_index == -1 and env.reset_shape_episode == 0
        env.reset(seed=1)
        env.reset()
        assert env.reset_shape_episode == 2 and "apply" in _kinds(be.calls)
        env.reset(seed=1)
        assert env.reset_shape_episode == 1                             # a re-seeded env begins again
