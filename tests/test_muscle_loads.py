"""muscle_loads() without a GPU (softrod_muscle_loads, VecRodEnvBase.muscle_loads, diagnostics.muscle_loads_host): the
symbol in header, library source and bindings; the NumPy twin against the oracle's independent transcription of the
muscle law (oracle.softrod_oracle_np.muscle_equivalent_loads, which tests/test_muscles.py holds the C oracle to); the
calibration of the band tests/test_gpu_muscle_loads.py holds the device to; identities of the twin; the shells; the new
kernels' scratch and LDS."""
import functools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi, diagnostics
from gym_softrobot_amd.diagnostics import MuscleLoads

try:
    from tests import muscle_loads_ref as ref
    from tests.oracle_backend import OracleBackend
except ImportError:                                  # imported with tests/ itself on the path
    import muscle_loads_ref as ref
    from oracle_backend import OracleBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


class RecordingOracle(OracleBackend):
    """The oracle backend, keeping the layers it is handed where the HIP backend keeps them."""

    def set_muscle_layers(self, ratio_position, strength):
        rp, st = np.ascontiguousarray(ratio_position, np.float64), np.ascontiguousarray(strength, np.float64)
        self._tables = {"muscle_layers": rp.tobytes() + st.tobytes()}
        super().set_muscle_layers(ratio_position, strength)


def _vec(env_id, n, backend_cls, **kw):
    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


class StubBackend:
    """A backend with a muscle_loads of the device's shapes (zeros): what VecRodEnvBase hands on."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}

    def muscle_loads(self):
        import torch

        buf = torch.zeros((self.n_envs, _capi.config_rods_per_env(self.cfg), 20, int(self.cfg.n_elem) + 1), dtype=torch.float64)
        return diagnostics.muscle_loads_views(buf)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


@functools.lru_cache(maxsize=None)
def _states(case_id):
    """The oracle backend's rods of one case at the two instants of the GPU test — after reset(seed=0) with the seeded
    activations written (time 0), and after 2 steps of the seeded actions (mid-substep) — computed once per case."""
    _, env_id, n, kw = next(c for c in ref.CASES if c[0] == case_id)
    env = _vec(env_id, n, RecordingOracle, **kw)
    env.reset(seed=ref.SEED)
    ref.write_activations(env, ref.seeded_activations(env))
    fresh = ref.rod_states(env)
    for a in ref.actions(env, env_id):
        env.step(a)
    stepped = ref.rod_states(env)
    assert len(fresh) == len(stepped) == n * _capi.config_rods_per_env(env.cfg)
    assert all(d["time"] == 0.0 for d in fresh) and all(d["time"] != 0.0 for d in stepped)
    env.close()
    return fresh, stepped


# ---- 1. header, library and bindings agree ---------------------------------------------------------------------------
def test_symbol_in_header_library_and_bindings():
    header = (ROOT / "include" / "softrod.h").read_text()
    assert "int softrod_muscle_loads(softrod_handle* h, double* out, void* stream);" in header
    assert "arm_push_env.py:197-212" in header and "octopus/build.py:295-338" in header and "PARITY UNPINNED" in header
    source = (CSRC / "softrod_capi.hip").read_text()
    assert "int softrod_muscle_loads(softrod_handle* h, double* out, void* stream) {" in source
    assert set(re.findall(r'"(muscle loads: [^"]*)"', source)) == {
        "muscle loads: null handle", "muscle loads: null output buffer", "muscle loads: this handle has no COOMM muscles",
        "muscle loads: softrod_set_muscle_layers has not been called"}
    assert "kMuscleRows = 20" in (CSRC / "softrod_muscle_readout.hpp").read_text()
    assert "softrod_muscle_loads" in _capi.EXPORTED_SYMBOLS
    assert _capi._EXPORTS["softrod_muscle_loads"] == _capi._EXPORTS["softrod_rod_energies"]
    assert _capi.ABI_VERSION == 17
    assert re.search(r"#define\s+SOFTROD_ABI_VERSION\s+17\b", header)
    assert _capi.muscle_loads_refusal(_capi.softpendulum_config(2)) == "muscle loads: this handle has no COOMM muscles"
    assert _capi.muscle_loads_refusal(_capi.arm_push_config(2)) is None


# ---- 2. the twin against an independent transcription of the law -------------------------------------------------------
def _oracle_loads(d, cfg):
    """oracle.softrod_oracle_np.muscle_equivalent_loads on the strains of the twin's instant."""
    from oracle import softrod_oracle_np as onp

    x, Q = np.array(d["x"]), np.array(d["Q"])
    if d["time"] != 0.0:
        x, Q = diagnostics.mid_substep_configuration(d["x"], d["v"], d["Q"], d["w"], float(cfg.dt), float(cfg.eps_rot_axis))
        if "bc" in d:
            diagnostics.constrain_values_host(int(cfg.features), x, Q, **d["bc"])
    m = d["material"]
    s = diagnostics.rod_strains(x, Q, m["rest_length"], d["radius"], float(cfg.acos_shift), float(cfg.eps_sin))
    ratio, strength = d["layers"]
    layers = [{"kind": int(cfg.muscle_kind[k]), "ratio": ratio[k], "strength": strength[k], "activation": d["activation"][k]}
              for k in range(int(cfg.n_muscles))]
    return onp.muscle_equivalent_loads(
        Q, s["sigma"], s["kappa"], s["tangents"], s["radius"], d["radius"], m["rest_length"], m["rest_voronoi"],
        s["dilatation"], s["voronoi_dilatation"], layers, [cfg.muscle_fl_coef[k] for k in range(int(cfg.muscle_fl_degree) + 1)],
        form=int(cfg.muscle_equiv_load_form), current_radius=bool(cfg.muscle_position_current_radius),
        tm_law=int(cfg.muscle_tm_length_law))


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_twin_equals_the_oracles_transcription(oracle_built, case):
    """External force, external couple and per-layer force of muscle_loads_host against the function the steppers'
    oracle is held to, for both muscle_form, muscle_cur_radius and muscle_tm_law values, at 1e-12 in band units."""
    top = {}
    for states in _states(case[0]):
        for d in states:
            for form in (0, 1):
                for cur in (0, 1):
                    for law in (0, 1):
                        cfg = d["cfg"].copy()
                        cfg.muscle_equiv_load_form, cfg.muscle_position_current_radius, cfg.muscle_tm_length_law = form, cur, law
                        got = ref.twin(d, cfg=cfg)
                        f, c, forces = _oracle_loads(d, cfg)
                        nm = int(cfg.n_muscles)
                        assert forces.shape == (nm, int(cfg.n_elem)) and not got.layer_force[nm:].any()
                        u = ref.band_units(d, cfg)
                        dev = {"external_force": np.abs(got.external_force - f) / u.external_force,
                               "external_couple": np.abs(got.external_couple - c) / u.external_couple,
                               "layer_force": np.abs(got.layer_force[:nm] - forces) / u.layer_force}
                        for k, v in dev.items():
                            top[k] = max(top.get(k, 0.0), float(v.max()))
    print(f"{case[0]}: worst |twin - oracle transcription| in band units", {k: f"{v:.1e}" for k, v in top.items()})
    for k, v in top.items():
        assert v <= 1e-12, (k, v)


def test_stepped_states_carry_active_layers(oracle_built):
    """The comparison above is not one of zeros: after the steps a layer force is non-zero in every case."""
    for case in ref.CASES:
        assert any(np.abs(ref.twin(d).layer_force).max() > 0 for d in _states(case[0])[1]), case[0]


# ---- 3. band calibration -----------------------------------------------------------------------------------------------
_EPS = 2.0 ** -52


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_band_is_ten_times_the_twins_own_conditioning(oracle_built, case):
    """For every case of the GPU matrix, on the oracle backend's states at both instants: the twin's answer moves by
    less than a tenth of BAND when x, v, Q, w are each scaled by 1 +- 2^-52."""
    top = {}
    for states in _states(case[0]):
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
    assert ref.BAND == 10.0 ** round(np.log10(ref.BAND))          # a power of ten


# ---- 4. identities on the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["push", "crawl"])
def test_zero_activation_gives_zero_loads_and_defined_lengths(oracle_built, case_id):
    for states in _states(case_id):
        for d in states:
            r = ref.twin(d, activation=np.zeros_like(d["activation"]))
            nm = int(d["cfg"].n_muscles)
            for f in ("layer_force", "internal_force", "internal_couple", "external_force", "external_couple"):
                assert (getattr(r, f) == 0.0).all(), f
            assert np.isfinite(r.layer_length[:nm]).all() and (r.layer_length[:nm] > 0).all()
            assert (r.layer_length[nm:] == 0.0).all()


def test_straight_unstretched_rod():
    """sigma = 0 and kappa = 0 exactly: every layer length is exactly 1, F_m = activation * strength * max(fl(1), 0), and
    f is along d3.  (The element length is 256: rod_strains adds 1e-14 to every length, which only a length of 128 or
    more absorbs; the identity itself has no scale.)"""
    n = 4
    cfg = _capi.arm_push_config(1, mode="continuous", n_elems=n)
    cfg.base_length = 256.0 * n
    radius = _capi.arm_push_radii(n)
    layers = _capi.es_muscle_layers(radius, 0.012)
    material = diagnostics.rod_material_host(cfg, radius)
    assert material["rest_length"] == 256.0
    x = np.zeros((3, n + 1))
    x[0] = 256.0 * np.arange(n + 1)
    Q = np.zeros((3, 3, n))
    Q[0, 1], Q[1, 2], Q[2, 0] = 1.0, 1.0, 1.0                     # d1 = e_y, d2 = e_z, d3 = e_x: the tangent
    act = np.random.default_rng(4).uniform(0.1, 1.0, (4, n))
    r = diagnostics.muscle_loads_host(x, np.zeros((3, n + 1)), Q, np.zeros((3, n)), 0.0, cfg, material, layers, act, radius)
    assert (r.layer_length[:3] == 1.0).all() and (r.layer_length[3] == 0.0).all()
    fl = 0.0
    for p in range(int(cfg.muscle_fl_degree), -1, -1):
        fl = fl * 1.0 + float(cfg.muscle_fl_coef[p])
    assert fl > 0.9
    np.testing.assert_array_equal(r.layer_force[:3], act[:3] * layers[1] * max(fl, 0.0))
    assert (r.internal_force[:2] == 0.0).all()
    np.testing.assert_array_equal(r.internal_force[2], r.layer_force[0] + r.layer_force[1] + r.layer_force[2])
    assert np.abs(r.internal_force[2]).min() > 0


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_external_force_sums_to_zero(oracle_built, case):
    """The external force is the difference of an element field padded with zeros: its sum over the nodes telescopes to
    zero, to 1e-12 of the rod's largest A (at most 127 terms of a few ulp of A each: ~3e-14, one order of margin)."""
    for states in _states(case[0]):
        for d in states:
            total = ref.twin(d).external_force.sum(axis=1)
            assert np.abs(total).max() <= 1e-12 * ref.strength_sum(d).max(), total


# ---- 5. shapes and shells ----------------------------------------------------------------------------------------------
def test_other_backends_raise(oracle_built):
    env = _vec("OctoArmPush-v1", 2, OracleBackend)
    with pytest.raises(NotImplementedError) as e:
        env.muscle_loads()
    assert str(e.value) == "muscle loads need the HIP backend, not OracleBackend"


def test_an_env_without_muscles_raises_the_librarys_text():
    env = _vec("SoftPendulum-v0", 2, StubBackend)
    with pytest.raises(ValueError) as e:
        env.muscle_loads()
    assert str(e.value) == "muscle loads: this handle has no COOMM muscles"


@pytest.mark.parametrize("env_id,n,rods,ne", [("OctoArmPush-v1", 3, 1, 40), ("OctoCrawl-v0", 2, 8, 20)])
def test_shapes_numpy_output_and_single_env_shell(env_id, n, rods, ne):
    shapes = [(rods, 4, ne), (rods, 4, ne), (rods, 3, ne), (rods, 3, ne - 1), (rods, 3, ne + 1), (rods, 3, ne)]
    r = _vec(env_id, n, StubBackend).muscle_loads()
    assert isinstance(r, MuscleLoads) and r._fields == ("layer_force", "layer_length", "internal_force", "internal_couple",
                                                        "external_force", "external_couple")
    assert [tuple(t.shape) for t in r] == [(n,) + s for s in shapes]
    r = _vec(env_id, n, StubBackend, numpy_output=True).muscle_loads()
    assert all(isinstance(t, np.ndarray) for t in r) and [t.shape for t in r] == [(n,) + s for s in shapes]
    if env_id == "OctoArmPush-v1":
        from gym_softrobot_amd.envs.arm_push import ArmPushEnv

        probe = ArmPushEnv(mode="continuous", backend=_Probe())
        r = ArmPushEnv(mode="continuous", backend=StubBackend(probe._vec.cfg)).muscle_loads()
        assert isinstance(r, MuscleLoads) and all(isinstance(t, np.ndarray) for t in r)
        assert [t.shape for t in r] == shapes


def test_views_cut_the_buffer_at_each_rows_range():
    buf = np.arange(2 * 20 * 6, dtype=np.float64).reshape(2, 20, 6)         # n_elem = 5
    v = diagnostics.muscle_loads_views(buf)
    assert [t.shape for t in v] == [(2, 4, 5), (2, 4, 5), (2, 3, 5), (2, 3, 4), (2, 3, 6), (2, 3, 5)]
    assert v.layer_length[1, 2, 3] == buf[1, 6, 3] and v.internal_couple[0, 1, 3] == buf[0, 12, 3]
    assert v.external_force[1, 2, 5] == buf[1, 16, 5] and v.external_couple[1, 0, 4] == buf[1, 17, 4]


# ---- 6. codegen of the new kernels -------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("key", ["softrod_muscle_loads_kernelILi1E", "softrod_muscle_loads_kernelILi2E"])
def test_muscle_loads_kernel_has_no_scratch_and_no_lds(isa_text, key):
    m = _meta(isa_text, key)
    print(f"{key}: {m['vgpr_count']} VGPRs")
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 0, m
