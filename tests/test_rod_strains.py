"""rod_strains() without a GPU (softrod_rod_strains, VecRodEnvBase.rod_strains, diagnostics.rod_strains_host): the symbol
in header, library source and bindings; the refusal of other backends; the NumPy twin against its parts and against
rod_energies_host; the calibration of the bands tests/test_gpu_rod_strains.py holds the device to; the new kernel's
scratch and LDS."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi, diagnostics
from gym_softrobot_amd.diagnostics import RodStrains, rod_energies_host

try:
    from tests import rod_strains_ref as ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import rod_strains_ref as ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    kw = {k: v for k, v in kw.items() if k != "math_mode" or backend_cls is not OracleBackend}
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


class StubBackend:
    """A backend with a rod_strains of the device's shapes (zeros): what VecRodEnvBase hands on."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}

    def rod_strains(self):
        import torch

        buf = torch.zeros((self.n_envs, _capi.config_rods_per_env(self.cfg), 14, int(self.cfg.n_elem)), dtype=torch.float64)
        return diagnostics.rod_strains_views(buf)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


# ---- 1. header, library and bindings agree ---------------------------------------------------------------------------
def test_symbol_in_header_library_and_bindings():
    header = (ROOT / "include" / "softrod.h").read_text()
    assert "int softrod_rod_strains(softrod_handle* h, double* out, void* stream);" in header
    assert "callback_func.py:23-41" in header and "PASSIVE" in header and "pyelastica 1.0.0 (not on disk)" in header
    source = (CSRC / "softrod_capi.hip").read_text()
    assert "int softrod_rod_strains(softrod_handle* h, double* out, void* stream) {" in source
    assert set(re.findall(r'"(rod strains: [^"]*)"', source)) == {"rod strains: null handle", "rod strains: null output buffer"}
    assert "softrod_rod_strains" in _capi.EXPORTED_SYMBOLS
    assert _capi._EXPORTS["softrod_rod_strains"] == _capi._EXPORTS["softrod_rod_energies"]
    assert _capi.ABI_VERSION == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)


def test_other_backends_raise(oracle_built):
    env = _vec("SoftPendulum-v0", 2, OracleBackend)
    with pytest.raises(NotImplementedError) as e:
        env.rod_strains()
    assert str(e.value) == "rod strains need the HIP backend, not OracleBackend"


@pytest.mark.parametrize("env_id,n,rods,ne", [("SoftPendulum-v0", 3, 1, 50), ("OctoFlat-v0", 2, 8, 10),
                                              ("OctoCrawl-v0", 2, 8, 20)])
def test_shapes_numpy_output_and_single_env_shell(env_id, n, rods, ne):
    shapes = [(rods, 3, ne), (rods, 3, ne - 1), (rods, ne), (rods, ne - 1), (rods, 3, ne), (rods, 3, ne - 1)]
    r = _vec(env_id, n, StubBackend).rod_strains()
    assert isinstance(r, RodStrains) and r._fields == ("sigma", "kappa", "dilatation", "voronoi_dilatation",
                                                       "internal_force", "internal_couple")
    assert [tuple(t.shape) for t in r] == [(n,) + s for s in shapes]
    r = _vec(env_id, n, StubBackend, numpy_output=True).rod_strains()
    assert all(isinstance(t, np.ndarray) for t in r) and [t.shape for t in r] == [(n,) + s for s in shapes]
    if env_id == "SoftPendulum-v0":
        from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

        probe = SoftPendulumEnv(backend=_Probe())
        r = SoftPendulumEnv(backend=StubBackend(probe._vec.cfg)).rod_strains()
        assert isinstance(r, RodStrains) and all(isinstance(t, np.ndarray) for t in r)
        assert [t.shape for t in r] == shapes


# ---- 2. / 3. the twin against its parts and against the energies ---------------------------------------------------------
def _stepped(env_id, n_elems, steps=2):
    env = _vec(env_id, 2, OracleBackend, n_elems=n_elems)
    env.reset(seed=ref.SEED)
    for a in ref.actions(env, env_id, steps):
        env.step(a)
    return env


@pytest.mark.parametrize("env_id,n_elems", [("SoftPendulum-v0", 5), ("OctoArmSingle-v0", 7)])
def test_twin_equals_its_parts_bit_for_bit(oracle_built, env_id, n_elems):
    for steps in (2, 0):
        env = _stepped(env_id, n_elems, steps)
        for d in ref.rod_states(env):
            cfg, m = d["cfg"], d["material"]
            assert (d["time"] != 0.0) == (steps != 0)
            x, Q = d["x"].copy(), d["Q"].copy()
            if steps:
                x, Q = diagnostics.mid_substep_configuration(d["x"], d["v"], d["Q"], d["w"], float(cfg.dt), float(cfg.eps_rot_axis))
                if "bc" in d:
                    diagnostics.constrain_values_host(int(cfg.features), x, Q, **d["bc"])
                assert not np.array_equal(x, d["x"])
            s = diagnostics.rod_strains(x, Q, m["rest_length"], 1.0, float(cfg.acos_shift), float(cfg.eps_sin))
            got = ref.twin(d)
            rk = 0.0 if d["rest_kappa"] is None else d["rest_kappa"]
            want = RodStrains(s["sigma"], s["kappa"], s["dilatation"], s["voronoi_dilatation"], m["shear"] * s["sigma"],
                              m["bend"] * (s["kappa"] - rk))
            for f, g, w in zip(RodStrains._fields, got, want):
                assert g.shape == w.shape and g.tobytes() == w.tobytes(), f
            assert got.sigma.shape == (3, n_elems) and got.kappa.shape == (3, n_elems - 1)
            assert got.dilatation.shape == (n_elems,) and got.voronoi_dilatation.shape == (n_elems - 1,)


@pytest.mark.parametrize("env_id,n_elems", [("SoftPendulum-v0", 5), ("OctoArmSingle-v0", 7)])
def test_energy_identity_on_the_twin(oracle_built, env_id, n_elems):
    """1/2 sum sigma . n l^ and 1/2 sum (kappa - rest_kappa) . m D^ are rod_energies_host's shear and bending entries:
    rtol 1e-12 (both sides sum at most 126 non-negative terms: 126 x a few ulp ~ 1e-13, one order of margin)."""
    env = _stepped(env_id, n_elems)
    for d in ref.rod_states(env):
        E = rod_energies_host(d["x"], d["v"], d["Q"], d["w"], d["time"], d["cfg"], d["material"], d["rest_kappa"],
                              **d.get("bc", {}))
        bend, shear = ref.energies_from_strains(ref.twin(d), d)
        assert E[2] > 0 and E[3] > 0
        np.testing.assert_allclose([bend, shear], E[2:], rtol=1e-12, atol=0)


# ---- 4. band calibration ---------------------------------------------------------------------------------------------------
_EPS = 2.0 ** -52


# (the oracle backend holds no per-env material table: "arm-material" is the same env and state as "arm")
@pytest.mark.parametrize("case", [c for c in ref.CASES if not c[3].get("material")], ids=lambda c: c[0])
def test_bands_are_ten_times_the_twins_own_conditioning(oracle_built, case):
    """For every case of the GPU matrix, on the oracle backend's state after the same reset and actions: the twin's
    answer moves by less than a tenth of the band when x, v, Q, w are each scaled by 1 +- 2^-52.  Every case passed
    with the matrix's own states (2 steps, actions within [-1, 1] of the action space): none had to be changed."""
    _, env_id, n, kw = case
    env = _vec(env_id, n, OracleBackend, **ref.make_kwargs(kw))
    env.reset(seed=ref.SEED)
    for a in ref.actions(env, env_id):
        env.step(a)
    states = ref.rod_states(env)
    assert len(states) == n * _capi.config_rods_per_env(env.cfg)
    top = {}
    for d in states:
        base = ref.twin(d)
        assert all(np.isfinite(np.asarray(t)).all() for t in base)
        for k in range(4):
            for sgn in (1.0, -1.0):
                sc = [1.0] * 4
                sc[k] = 1.0 + sgn * _EPS
                for f, v in ref.worst(ref.twin(d, sc), base, d).items():
                    top[f] = max(top.get(f, 0.0), v)
    print(f"{case[0]}: the twin moves by at most", {f: f"{v:.1e}" for f, v in top.items()})
    for f, v in top.items():
        assert v < 0.1 * ref.BAND, (f, v)


# ---- codegen of the new kernel ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa_text(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa") / "capi.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(asm), str(CSRC / "softrod_capi.hip")], check=True, timeout=900,
                   stderr=subprocess.DEVNULL)
    return asm.read_text()


def _meta(isa_text, mangled_substr):
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa_text, re.S):
        blk = m.group(0)
        if mangled_substr in re.search(r"\.name:\s+(\S+)", blk).group(1):
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))      # noqa: E731
            return {k: g(k) for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
                                      "vgpr_count")}
    raise AssertionError(f"kernel {mangled_substr} not found")


@pytest.mark.parametrize("key", ["softrod_rod_strains_kernelILi1E", "softrod_rod_strains_kernelILi2E"])
def test_strains_kernel_has_no_scratch_and_no_lds(isa_text, key):
    m = _meta(isa_text, key)
    print(f"{key}: {m['vgpr_count']} VGPRs")
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 0, m
