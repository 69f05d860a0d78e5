"""Per-env rod material (VecRodEnvBase.set_material, softrod_set_env_material) without a GPU: the argument handling
against a stub backend, the refusals of the oracle backend and of out-of-scope envs, and the code generation of the
three kFeatEnvMaterial step-kernel instantiations against their uniform twins."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gym_softrobot_amd import _capi
from gym_softrobot_amd.backend import HipRodBackend

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"


class StubBackend:
    """Records what VecRodEnvBase.set_material hands to the backend; keeps the host copy like HipRodBackend."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}
        self.calls = []

    def set_env_material(self, material, mask=None):
        m = np.asarray(material, np.float64).reshape(self.n_envs, 4).copy()
        k = None if mask is None else np.asarray(mask, np.uint8).copy()
        self.calls.append((m, k))
        cur = self.env_material()
        self._env_material = np.where(k[:, None] != 0, m, cur) if k is not None else m

    env_material = HipRodBackend.env_material

    def set_radius_profile(self, radius):
        self._tables["radius_profile"] = np.asarray(radius, np.float64).tobytes()

    def __getattr__(self, name):            # the other table setters the env constructors call: no-ops
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls=StubBackend, **kw):
    import gym_softrobot_amd as gsa

    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


@pytest.mark.parametrize("env_id", ["SoftPendulum-v0", "SoftPendulum3D-v0", "OctoArmSingle-v0"])
def test_material_defaults_are_the_config_values(env_id):
    env = _vec(env_id, 5)
    m = env.material()
    assert list(m) == ["youngs_modulus", "shear_modulus", "density", "damping_constant"]
    c = env.cfg
    for k in m:
        assert m[k].shape == (5,) and m[k].dtype == np.float64
        np.testing.assert_array_equal(m[k], getattr(c, k))
    np.testing.assert_allclose(m["shear_modulus"], m["youngs_modulus"] / 3.0, rtol=1e-15)


def test_scalars_arrays_masks_and_omitted_shear_modulus():
    import torch

    n = 6
    env = _vec("SoftPendulum-v0", n)
    c = env.cfg
    env.set_material(youngs_modulus=2e6)
    m, k = env.backend.calls[-1]
    assert k.tolist() == [1] * n
    np.testing.assert_array_equal(m[:, 0], 2e6)
    np.testing.assert_array_equal(m[:, 1], 2e6 / 3.0)                 # G = E / 3
    np.testing.assert_array_equal(m[:, 2], c.density)
    np.testing.assert_array_equal(m[:, 3], c.damping_constant)
    rho = np.linspace(500.0, 2000.0, n)
    mask = np.array([1, 0, 1, 0, 0, 1], bool)
    env.set_material(mask, density=torch.tensor(rho), damping_constant=0.0)
    m, k = env.backend.calls[-1]
    assert k.tolist() == mask.astype(int).tolist()
    got = env.material()
    np.testing.assert_array_equal(got["density"], np.where(mask, rho, c.density))
    np.testing.assert_array_equal(got["damping_constant"], np.where(mask, 0.0, c.damping_constant))
    np.testing.assert_array_equal(got["youngs_modulus"], 2e6)          # kept
    env.set_material(shear_modulus=np.full(n, 5e5))                    # G alone leaves E
    got = env.material()
    np.testing.assert_array_equal(got["youngs_modulus"], 2e6)
    np.testing.assert_array_equal(got["shear_modulus"], 5e5)
    env.set_material(torch.tensor(mask), youngs_modulus=np.arange(1, n + 1) * 1e6, shear_modulus=1e5)
    got = env.material()
    np.testing.assert_array_equal(got["youngs_modulus"], np.where(mask, np.arange(1, n + 1) * 1e6, 2e6))
    np.testing.assert_array_equal(got["shear_modulus"], np.where(mask, 1e5, 5e5))


@pytest.mark.parametrize("kw", [dict(youngs_modulus=np.inf), dict(density=np.nan), dict(youngs_modulus=0.0),
                                dict(shear_modulus=-1.0), dict(density=-5.0), dict(damping_constant=-1e-3),
                                dict(youngs_modulus=np.ones(3)), dict(density=np.ones((6, 1)))])
def test_bad_values_and_shapes_are_rejected_before_any_upload(kw):
    env = _vec("SoftPendulum3D-v0", 6)
    with pytest.raises(ValueError):
        env.set_material(**kw)
    assert env.backend.calls == []
    with pytest.raises(ValueError):
        env.set_material(np.ones(4, bool), density=2.0)                 # mask of the wrong length


def test_a_bad_value_outside_the_mask_does_not_matter():
    env = _vec("SoftPendulum-v0", 3)
    env.set_material(np.array([1, 0, 1], bool), density=np.array([900.0, -1.0, 1100.0]))
    np.testing.assert_array_equal(env.material()["density"], [900.0, env.cfg.density, 1100.0])


def test_oracle_backend_refuses(oracle_built):
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend

    env = _vec("SoftPendulum-v0", 2, backend_cls=OracleBackend)
    with pytest.raises(NotImplementedError):
        env.set_material(density=1200.0)
    np.testing.assert_array_equal(env.material()["density"], env.cfg.density)


@pytest.mark.parametrize("env_id,kw", [("OctoFlat-v0", {}), ("SoftArmTracking-v0", {}), ("OctoArmPush-v1", {}),
                                       ("OctoArmSingle-v0", dict(n_elems=100)), ("SoftPendulum3D-v0", dict(n_elems=100))])
def test_out_of_scope_envs_refuse_before_any_upload(env_id, kw):
    env = _vec(env_id, 2, **kw)
    with pytest.raises(NotImplementedError):
        env.set_material(youngs_modulus=2e6)
    assert env.backend.calls == []


def test_tapered_arm_refuses():
    env = _vec("OctoArmSingle-v0", 2)
    env.backend._tables["radius_profile"] = b"x"
    with pytest.raises(NotImplementedError, match="tapered"):
        env.set_material(density=900.0)


def test_single_envs_forward_with_one_env():
    from gym_softrobot_amd.envs.base import SingleEnvMaterial
    from gym_softrobot_amd.envs.soft_pendulum import SoftPendulumEnv

    assert issubclass(SoftPendulumEnv, SingleEnvMaterial)
    e = SingleEnvMaterial()
    e._vec = _vec("OctoArmSingle-v0", 1)
    e.set_material(youngs_modulus=3e6, density=800.0)
    assert e.material() == {"youngs_modulus": 3e6, "shear_modulus": 1e6, "density": 800.0,
                            "damping_constant": e._vec.cfg.damping_constant}


def test_header_and_exports_carry_the_entry_point():
    h = (ROOT / "include" / "softrod.h").read_text()
    assert "int softrod_set_env_material(softrod_handle* h, const double* material, const uint8_t* mask, void* stream);" in h
    assert "softrod_set_env_material" in _capi.EXPORTED_SYMBOLS
    assert _capi.ABI_VERSION == 17


# ---- code generation ---------------------------------------------------------------------------------------------
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
            return {k: g(k) for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "agpr_count")}
    raise AssertionError(f"kernel {mangled_substr} not found")


ENV_MAT = 1 << 28           # kFeatEnvMaterial
# (uniform twin, the same with kFeatEnvMaterial in F, loop budget: VALU, register copies, v_readlane)
TWINS = [
    ("fast_kernelILj15ELi1ELi1ELb0E", f"fast_kernelILj{15 | ENV_MAT}ELi1ELi1ELb0E", (102, 0, 0)),
    ("fast_kernelILj201ELi2ELi1ELb0E", f"fast_kernelILj{201 | ENV_MAT}ELi2ELi1ELb0E", (550, 10, 4)),
    ("fast_kernelILj1073742601ELi3ELi1ELb0E", f"fast_kernelILj{1073742601 | ENV_MAT}ELi3ELi1ELb0E", (535, 8, 4)),
]


@pytest.mark.parametrize("twin,key,budget", TWINS, ids=["SoftPendulum", "SoftPendulum3D", "OctoArmSingle"])
def test_env_material_kernels_match_their_uniform_twins(isa_text, twin, key, budget):
    sys.path.insert(0, str(ROOT / "tools"))
    import hot_path_isa

    m, t = _meta(isa_text, key), _meta(isa_text, twin)
    print(f"{key}: {m}; twin {t}")
    # the same register allocation: the same waves per SIMD (__launch_bounds__ and VGPRs), no more spilled VGPRs
    # and no more scratch than the twin (whose scratch brackets the SoftPendulum kernel's out-of-line 3-D fallback
    # and holds the 3-D kernels' spill slots outside the loop)
    assert m["vgpr_count"] == t["vgpr_count"] and m["agpr_count"] == t["agpr_count"], (m, t)
    assert m["vgpr_spill_count"] <= t["vgpr_spill_count"], (m, t)
    assert m["private_segment_fixed_size"] <= t["private_segment_fixed_size"], (m, t)
    ins, labels = hot_path_isa.function_body(isa_text, key)
    path = hot_path_isa.hot_path(ins, labels)
    valu = [x for x in path if x.startswith("v_")]
    valu_max, copies_max, readlane_max = budget
    assert len(valu) <= valu_max, f"{key}: {len(valu)} VALU instructions per substep"
    assert sum(x.startswith("v_mov_b64") for x in valu) <= copies_max, key
    assert sum(x.startswith("v_readlane") for x in valu) <= readlane_max, key
    assert not [x for x in path if x.startswith(("scratch", "global", "buffer", "flat"))], key
    tins, tlabels = hot_path_isa.function_body(isa_text, twin)
    assert len(valu) == len([x for x in hot_path_isa.hot_path(tins, tlabels) if x.startswith("v_")])
    # the env's row arrives through scalar loads (wave-uniform address): no more vector loads than the twin
    assert sum(x.startswith("global_load") for x in ins) == sum(x.startswith("global_load") for x in tins)
