"""set_rod_shape() without a GPU (softrod_set_rod_shape, VecRodEnvBase.set_rod_shape): the symbol in header, library
source and bindings with the ABI still 17; the null-handle refusal, which needs no device; the known answers of the
yardstick (tests/rod_shape_ref.py), its round trip through the strain read-out's twin and its own float64 error
against long double; the env layer's refusals through a stub backend."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi, diagnostics

try:
    from tests import rod_shape_ref as ref
    from tests import rod_strains_ref as strains_ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import rod_shape_ref as ref
    import rod_strains_ref as strains_ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"
EINVAL = -1
DECLARATION = ("int softrod_set_rod_shape(softrod_handle* h, const double* kappa, const double* sigma, const double* velocity,\n"
               "                          const double* omega, const uint8_t* mask, void* stream)")


# ---- 1. the interface --------------------------------------------------------------------------------------------------
def test_symbol_header_and_table(hip_lib):
    header = (ROOT / "include" / "softrod.h").read_text()
    assert DECLARATION + ";" in header
    for words in ("Q_{k+1} = exp(-[kappa_k D^]x) Q_k", "x_{k+1} - x_k = l^ Q_k^T (sigma_k + e3)", "KEEPS THE BASE POSE",
                  "[n_envs][rods_per_env][3][n_elem - 1]", "[n_envs][rods_per_env][3][n_elem + 1]", "straight_rod only",
                  "build.py:54-61", "a NaN spoils its own rod only", "set rod shape: null handle"):
        assert words in header, words
    source = (CSRC / "softrod_capi.hip").read_text()
    assert DECLARATION + " {" in source
    assert source.index('#include "softrod_copy_envs.hpp"') < source.index('#include "softrod_shape.hpp"')
    kernel = (CSRC / "softrod_shape.hpp").read_text()
    code = re.sub(r"//.*", "", kernel)
    assert "softrod_rod_shape_kernel" in code and "slot_kappa(P," in code and "readout_rod(P," in code
    assert "atomic" not in code and "__shared__" not in code and "float " not in code.replace("float a[", "")
    assert "softrod_set_rod_shape" in _capi.EXPORTED_SYMBOLS and hasattr(hip_lib, "softrod_set_rod_shape")
    assert hip_lib.softrod_set_rod_shape.argtypes == [C.c_void_p] * 7
    assert _capi.ABI_VERSION == 17 and hip_lib.softrod_abi_version() == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)


def test_null_handle_is_refused_before_any_device_is_needed(hip_lib):
    assert hip_lib.softrod_set_rod_shape(None, None, None, None, None, None, None) == EINVAL
    assert hip_lib.softrod_last_error(None) == b"set rod shape: null handle"
    source = (CSRC / "softrod_capi.hip").read_text()
    body = source[source.index(DECLARATION + " {"):]
    assert body.index("null handle") < body.index("SR_ON_DEVICE(h)")


# ---- 2. the yardstick's known answers ---------------------------------------------------------------------------------
L, N_EL = 0.2, 10
ELL = L / N_EL
X0 = np.array([0.3, -0.1, 0.05])


def test_constant_in_plane_kappa_is_the_inscribed_polygon():
    """kappa about d2 with Q_0 = I: element j points along (sin j th, 0, cos j th), th = kappa D^; the nodes lie on a
    circle of radius l^ / (2 sin(th / 2)) and node m has the closed form below; d1 of the tip turns with it."""
    k = 4.0
    th = k * ELL
    kappa = np.zeros((3, N_EL - 1))
    kappa[1] = k
    x, Q = ref.build(X0, np.eye(3), kappa, None, ELL)
    m = np.arange(N_EL + 1)
    chord = ELL * np.sin(m * th / 2) / np.sin(th / 2)
    want = X0[:, None] + np.stack([chord * np.sin((m - 1) * th / 2), 0 * m, chord * np.cos((m - 1) * th / 2)])
    assert np.abs(x - want).max() <= 1e-15
    radius = ELL / (2 * np.sin(th / 2))
    centre = X0 + np.array([radius * np.cos(th / 2), 0.0, radius * np.sin(th / 2)])     # on the first chord's bisector
    assert np.abs(np.linalg.norm(x - centre[:, None], axis=0) - radius).max() <= 1e-15
    j = N_EL - 1
    tip = np.array([[np.cos(j * th), 0, -np.sin(j * th)], [0, 1, 0], [np.sin(j * th), 0, np.cos(j * th)]])
    assert np.abs(Q[:, :, j] - tip).max() <= 1e-15
    assert x[0, -1] > X0[0] + 0.05 * L                                  # positive kappa_2 bends d3 towards +d1


def test_pure_twist_leaves_the_centre_line_straight():
    tau = 7.0
    ph = -tau * ELL
    kappa = np.zeros((3, N_EL - 1))
    kappa[2] = tau
    x, Q = ref.build(X0, np.eye(3), kappa, None, ELL)
    want = X0[:, None] + np.stack([0 * np.arange(N_EL + 1.0)] * 2 + [ELL * np.arange(N_EL + 1.0)])
    assert np.abs(x - want).max() <= 1e-15                             # N_EL additions at 0.5 ulp(0.5) each
    for j in (1, N_EL - 1):
        c, s = np.cos(j * ph), np.sin(j * ph)
        assert np.abs(Q[:, :, j] - np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])).max() <= 1e-15


def test_stretch_and_shear():
    sigma = np.zeros((3, N_EL))
    sigma[2] = 0.1
    x, Q = ref.build(X0, np.eye(3), None, sigma, ELL)
    assert np.linalg.norm(x[:, -1] - x[:, 0]) == pytest.approx(1.1 * L, abs=1e-15)
    assert np.array_equal(Q, np.repeat(np.eye(3)[:, :, None], N_EL, axis=2))
    sigma = np.zeros((3, N_EL))
    sigma[0] = 0.03
    Q0 = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])      # d1 = e_y, d2 = e_z, d3 = e_x
    x, _ = ref.build(X0, Q0, None, sigma, ELL)
    assert np.abs(x[:, -1] - (X0 + [L, 0.03 * L, 0.0])).max() <= 1e-15     # L along d3, 0.03 L along d1
    x, Q = ref.build(X0, Q0, None, None, ELL, n=N_EL)
    assert np.abs(x[:, -1] - (X0 + [L, 0, 0])).max() <= 1e-15              # no field: the straight rod along d3


def _random_rod(n, seed):
    rng = np.random.default_rng(seed)
    ell = L / n
    kappa, sigma, _, _ = ref.random_fields(rng, 1, 1, n, ell, rates=False)
    Q0 = ref.rotation(rng.uniform(-1, 1, 3))
    return ell, kappa[0, 0], sigma[0, 0], rng.uniform(-0.5, 0.5, 3), Q0


@pytest.mark.parametrize("n", ref.SIZES)
def test_round_trip_through_the_strain_twin(n):
    """build -> diagnostics.rod_strains (the twin rod_strains() is held to) returns sigma inside that twin's band and
    kappa inside it once the read-out's own guard is accounted for: acos(cos th - acos_shift) for th scales kappa by
    th' sin(th) / (th sin(th' + eps_sin)) = 1 + acos_shift / 3 + ...; against the raw input, BAND_KAPPA."""
    ell, kappa, sigma, x0, Q0 = _random_rod(n, 100 + n)
    x, Q = ref.build(x0, Q0, kappa, sigma, ell)
    cfg = _capi.softpendulum_config(1)
    s = diagnostics.rod_strains(x, Q, ell, 1.0, float(cfg.acos_shift), float(cfg.eps_sin))
    assert np.abs(s["sigma"] - sigma).max() <= strains_ref.BAND
    th = np.linalg.norm(kappa * ell, axis=0).astype(np.longdouble)
    th2 = np.arccos(np.cos(th) - np.longdouble(cfg.acos_shift))
    guard = (th2 * np.sin(th) / (th * np.sin(th2 + np.longdouble(cfg.eps_sin)))).astype(np.float64)
    assert np.abs(guard - (1 + float(cfg.acos_shift) / 3)).max() < 1e-11
    err = np.abs(s["kappa"] - kappa * guard).max() * ell
    raw = np.abs(s["kappa"] - kappa).max() / np.abs(kappa).max()
    print(f"n = {n}: |twin - guard * kappa| D^ = {err:.2e}, |twin - kappa| / max|kappa| = {raw:.2e}")
    assert err <= strains_ref.BAND
    assert raw <= ref.BAND_KAPPA
    tangents, kap = ref.derived(x, Q, cfg, ell)
    assert np.array_equal(kap, s["kappa"])
    # unit up to reset's eps_length in the divisor
    assert np.abs(np.linalg.norm(tangents, axis=0) - 1).max() <= 2 * float(cfg.eps_length) / (0.9 * ell)


@pytest.mark.parametrize("n", ref.SIZES)
def test_the_yardsticks_own_error_is_a_tenth_of_the_band(n):
    """float64 against long double: director entries, positions, orthonormality."""
    assert np.finfo(np.longdouble).eps < 1e-18
    ell, kappa, sigma, x0, Q0 = _random_rod(n, 200 + n)
    lo = ref.build(x0, Q0, kappa, sigma, ell)
    hi = ref.build(x0, Q0, kappa, sigma, ell, dtype=np.longdouble)
    ex = float(np.abs(hi[0] - lo[0]).max()) / L
    eq = float(np.abs(hi[1] - lo[1]).max())
    orth = ref.orthonormality(lo[1])
    print(f"n = {n}: |float64 - long double| = {ex:.2e} L on positions, {eq:.2e} on directors; orthonormality {orth:.2e}")
    assert ex <= 0.1 * ref.BAND_X and eq <= 0.1 * ref.BAND_Q and orth <= 0.1 * ref.BAND_Q
    assert hi[0].dtype == np.longdouble and ref.rotation(kappa[:, 0] * ell, np.longdouble).dtype == np.longdouble
    assert np.abs(kappa * ell).max() > 0.1 and np.linalg.norm(kappa * ell, axis=0).max() <= ref.MAX_ANGLE


# ---- 3. the env layer ---------------------------------------------------------------------------------------------------
class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


class StubBackend:
    """A backend with a set_rod_shape that records what VecRodEnvBase hands on and returns zeros as observations."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}
        self.calls = []

    def set_rod_shape(self, mask=None, **fields):
        import torch

        self.calls.append((mask, fields))
        return torch.zeros((self.n_envs, _capi.config_obs_dim(self.cfg)), dtype=torch.float32)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


def test_fields_reach_the_backend_and_observations_come_back():
    env = _vec("SoftPendulum-v0", 3, StubBackend, numpy_output=True)
    ne = int(env.cfg.n_elem)
    kappa = np.zeros((3, 1, 3, ne - 1))
    obs = env.set_rod_shape([True, False, True], kappa=kappa, sigma=np.zeros((3, 3, ne)))       # rods axis left out
    assert isinstance(obs, np.ndarray) and obs.shape == (3, _capi.config_obs_dim(env.cfg))
    mask, fields = env.backend.calls[0]
    assert mask.tolist() == [True, False, True] and fields["kappa"] is kappa and fields["velocity"] is None
    env.set_rod_shape()
    assert env.backend.calls[1][0] is None and all(v is None for v in env.backend.calls[1][1].values())
    assert (env._steps == 0).all() and not env._needs_reset.any()


@pytest.mark.parametrize("env_id,rods", [("SoftPendulum-v0", 1), ("OctoFlat-v0", 8), ("OctoArmTwo-v0", 2)])
def test_wrong_shapes_and_dtypes_are_refused(env_id, rods):
    import torch

    n = 2
    env = _vec(env_id, n, StubBackend)
    ne = int(env.cfg.n_elem)
    good = dict(kappa=(n, rods, 3, ne - 1), sigma=(n, rods, 3, ne), velocity=(n, rods, 3, ne + 1), omega=(n, rods, 3, ne))
    for name, shape in good.items():
        assert _capi.rod_shape_field_shape(env.cfg, n, name) == shape
        env.set_rod_shape(**{name: np.zeros(shape)})
        env.set_rod_shape(**{name: torch.zeros(shape, dtype=torch.float64)})
        bad = [np.zeros(shape[:-1] + (shape[-1] + 1,)), np.zeros((n + 1,) + shape[1:]), np.zeros(shape[:2] + (2,) + shape[3:]),
               np.zeros(shape[1:]), np.zeros(shape).reshape(-1)]
        if rods > 1:
            bad.append(np.zeros(shape[:1] + shape[2:]))                 # the rods axis is optional for a one-rod env only
        for v in bad:
            with pytest.raises(ValueError, match=f"set_rod_shape: {name} must have shape"):
                env.set_rod_shape(**{name: v})
        for v in (np.zeros(shape, np.float32), torch.zeros(shape, dtype=torch.float32), np.zeros(shape, np.int64)):
            with pytest.raises(ValueError, match=f"set_rod_shape: {name} must be float64"):
                env.set_rod_shape(**{name: v})
    calls = len(env.backend.calls)
    with pytest.raises(ValueError, match="mask: expected shape"):
        env.set_rod_shape(np.ones(n + 1, bool))
    assert len(env.backend.calls) == calls == 2 * len(good)             # a refused call never reaches the backend


def test_a_stepped_env_is_refused():
    env = _vec("SoftPendulum-v0", 3, StubBackend)
    env._steps[1] = 4                                                   # what step() books
    with pytest.raises(ValueError, match=r"envs \[1\] have stepped since their reset"):
        env.set_rod_shape()
    with pytest.raises(ValueError, match="have stepped"):
        env.set_rod_shape([False, True, False])
    env.set_rod_shape([True, False, True])
    assert len(env.backend.calls) == 1 and env._steps.tolist() == [0, 4, 0]


def test_single_env_shell_adds_the_env_axis():
    from gym_softrobot_amd.envs.octo_flat import FlatEnv
    from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

    for cls, rods in ((SoftPendulumEnv, 1), (FlatEnv, 8)):
        probe = cls(backend=_Probe())
        env = cls(backend=StubBackend(probe._vec.cfg))
        ne = int(env._vec.cfg.n_elem)
        env.set_rod_shape(kappa=np.zeros((rods, 3, ne - 1)))
        assert env._vec.backend.calls[-1][1]["kappa"].shape == (1, rods, 3, ne - 1)
        if rods == 1:
            env.set_rod_shape(sigma=np.zeros((3, ne)))
            assert env._vec.backend.calls[-1][1]["sigma"].shape == (1, 3, ne)
        with pytest.raises(ValueError, match="must have shape"):
            env.set_rod_shape(omega=np.zeros((rods, 3, ne + 1)))


def test_oracle_backend_has_no_set_rod_shape(oracle_built):
    env = _vec("SoftPendulum-v0", 2, OracleBackend)
    with pytest.raises(NotImplementedError, match="set_rod_shape needs the HIP backend, not OracleBackend"):
        env.set_rod_shape()
