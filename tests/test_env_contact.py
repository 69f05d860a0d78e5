"""Per-env ground contact and friction (VecRodEnvBase.set_contact, softrod_set_env_contact) without a GPU: the
argument handling against a stub backend, upstream's friction knobs against the executed reference's build
functions (tests/golden/ref_friction_knobs.json, tools/make_friction_golden.py), the refusals of the oracle backend
and of out-of-scope envs, and the code generation of the kFeatEnvContact step-kernel instantiations against their
uniform twins."""
import json
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
GOLD = ROOT / "tests" / "golden" / "ref_friction_knobs.json"


class StubBackend:
    """Records what VecRodEnvBase.set_contact hands to the backend; keeps the host copy like HipRodBackend."""

    def __init__(self, cfg):
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self._tables = {}
        self.calls = []

    def set_env_contact(self, contact, mask=None):
        c = np.asarray(contact, np.float64).reshape(self.n_envs, 8).copy()
        k = None if mask is None else np.asarray(mask, np.uint8).copy()
        self.calls.append((c, k))
        cur = self.env_contact()
        self._env_contact = np.where(k[:, None] != 0, c, cur) if k is not None else c

    env_contact = HipRodBackend.env_contact

    def __getattr__(self, name):            # the other table setters the env constructors call: no-ops
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: None


class _Probe:
    def __getattr__(self, name):
        return lambda *a, **k: None


def _vec(env_id, n, backend_cls=StubBackend, **kw):
    import gym_softrobot_amd as gsa

    cls, base_kw = gsa._VEC[env_id]
    probe = cls(n, **{**base_kw, **kw}, backend=_Probe())        # the config the env builds
    return cls(n, **{**base_kw, **kw}, backend=backend_cls(probe.cfg))


IN_SCOPE = ["OctoArmSingle-v0", "OctoFlat-v0", "OctoFlatLite-v0"]


@pytest.mark.parametrize("env_id", IN_SCOPE)
def test_contact_defaults_are_the_config_values(env_id):
    env = _vec(env_id, 5)
    c = env.contact()
    assert list(c) == ["contact_k", "contact_nu", "kinetic_mu", "static_mu"]
    cfg = env.cfg
    assert c["contact_k"].shape == (5,) and c["contact_nu"].shape == (5,)
    assert c["kinetic_mu"].shape == (5, 3) and c["static_mu"].shape == (5, 3)
    np.testing.assert_array_equal(c["contact_k"], cfg.contact_k)
    np.testing.assert_array_equal(c["contact_nu"], cfg.contact_nu)
    np.testing.assert_array_equal(c["kinetic_mu"], np.tile(list(cfg.kinetic_mu), (5, 1)))
    np.testing.assert_array_equal(c["static_mu"], np.tile(list(cfg.static_mu), (5, 1)))
    np.testing.assert_array_equal(_capi.env_contact_defaults(cfg),
                                  [cfg.contact_k, cfg.contact_nu, *cfg.kinetic_mu, *cfg.static_mu])


def test_scalars_triples_rows_torch_and_masks():
    import torch

    n = 6
    env = _vec("OctoArmSingle-v0", n)
    cfg = env.cfg
    env.set_contact(contact_k=250.0)
    c, k = env.backend.calls[-1]
    assert k.tolist() == [1] * n
    np.testing.assert_array_equal(c[:, 0], 250.0)
    np.testing.assert_array_equal(c[:, 1], cfg.contact_nu)
    np.testing.assert_array_equal(c[:, 2:], np.tile([*cfg.kinetic_mu, *cfg.static_mu], (n, 1)))
    env.set_contact(kinetic_mu=0.3, static_mu=[0.5, 0.6, 0.7])            # scalar and (3,)
    got = env.contact()
    np.testing.assert_array_equal(got["kinetic_mu"], 0.3)
    np.testing.assert_array_equal(got["static_mu"], np.tile([0.5, 0.6, 0.7], (n, 1)))
    rows = np.arange(3 * n, dtype=np.float64).reshape(n, 3) / 10
    mask = np.array([1, 0, 1, 0, 0, 1], bool)
    env.set_contact(mask, contact_nu=torch.arange(n, dtype=torch.float64), kinetic_mu=torch.tensor(rows),
                    static_mu=rows + 1)
    c, k = env.backend.calls[-1]
    assert k.tolist() == mask.astype(int).tolist()
    got = env.contact()
    np.testing.assert_array_equal(got["contact_nu"], np.where(mask, np.arange(n), cfg.contact_nu))
    np.testing.assert_array_equal(got["kinetic_mu"], np.where(mask[:, None], rows, 0.3))
    np.testing.assert_array_equal(got["static_mu"], np.where(mask[:, None], rows + 1, [0.5, 0.6, 0.7]))
    np.testing.assert_array_equal(got["contact_k"], 250.0)                 # kept
    env.set_contact(torch.tensor(~mask), contact_k=np.full(n, 80.0))
    np.testing.assert_array_equal(env.contact()["contact_k"], np.where(mask, 250.0, 80.0))


def test_kinetic_alone_sets_static_to_twice_kinetic():
    n = 4
    env = _vec("OctoFlat-v0", n)
    kin = np.array([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0], [1.0, 1.5, 2.0], [0.05, 0.07, 0.09]])
    env.set_contact(kinetic_mu=kin)
    got = env.contact()
    np.testing.assert_array_equal(got["kinetic_mu"], kin)
    np.testing.assert_array_equal(got["static_mu"], 2 * kin)
    env.set_contact(static_mu=0.4)                                          # static alone leaves kinetic
    np.testing.assert_array_equal(env.contact()["kinetic_mu"], kin)
    np.testing.assert_array_equal(env.contact()["static_mu"], 0.4)


@pytest.mark.parametrize("builder,env_id", [("build_arm", "OctoArmSingle-v0"), ("build_octopus", "OctoFlat-v0")])
def test_friction_knobs_reproduce_the_executed_reference(builder, env_id):
    """friction_multiplier / friction_symmetry give exactly the mu arrays the reference's own build function hands
    to RodPlaneContactWithAnisotropicFriction (recorded by executing it), and the reference's k and nu are the
    config's; 1 / False is the config itself."""
    recs = json.loads(GOLD.read_text())[builder]
    assert any(r["friction_multiplier"] == 1.0 and not r["friction_symmetry"] for r in recs)
    n = len(recs)
    env = _vec(env_id, n)
    cfg = env.cfg
    for r in recs:
        assert r["k"] == cfg.contact_k and r["nu"] == cfg.contact_nu and r["slip_velocity_tol"] == cfg.slip_velocity_tol
        if r["friction_multiplier"] == 1.0 and not r["friction_symmetry"]:
            assert r["kinetic_mu_array"] == list(cfg.kinetic_mu) and r["static_mu_array"] == list(cfg.static_mu)
    env.set_contact(friction_multiplier=np.array([r["friction_multiplier"] for r in recs]),
                    friction_symmetry=np.array([r["friction_symmetry"] for r in recs]))
    got = env.contact()
    for i, r in enumerate(recs):
        assert got["kinetic_mu"][i].tolist() == r["kinetic_mu_array"], (i, r)
        assert got["static_mu"][i].tolist() == r["static_mu_array"], (i, r)
    # scalar knobs, one at a time (the other at upstream's default)
    env.set_contact(friction_symmetry=True)
    want = next(r for r in recs if r["friction_multiplier"] == 1.0 and r["friction_symmetry"])
    assert got["contact_k"].tolist() == [cfg.contact_k] * n
    assert env.contact()["kinetic_mu"][0].tolist() == want["kinetic_mu_array"]
    env.set_contact(friction_multiplier=1.0)
    assert env.contact()["static_mu"][n - 1].tolist() == list(cfg.static_mu)


def test_friction_knobs_exclude_explicit_arrays():
    env = _vec("OctoArmSingle-v0", 2)
    with pytest.raises(ValueError):
        env.set_contact(friction_multiplier=2.0, kinetic_mu=0.1)
    with pytest.raises(ValueError):
        env.set_contact(friction_symmetry=True, static_mu=0.1)
    assert env.backend.calls == []


@pytest.mark.parametrize("kw", [dict(contact_k=np.inf), dict(contact_nu=np.nan), dict(contact_k=-1.0),
                                dict(contact_nu=-1e-3), dict(kinetic_mu=-0.1), dict(static_mu=[0.1, -0.2, 0.3]),
                                dict(kinetic_mu=[0.1, np.inf, 0.3]), dict(friction_multiplier=-1.0),
                                dict(friction_multiplier=np.nan), dict(contact_k=np.ones(3)),
                                dict(kinetic_mu=np.ones((6, 2))), dict(static_mu=np.ones(6)),
                                dict(friction_multiplier=np.ones(4)), dict(friction_symmetry=np.ones(3, bool)),
                                dict(friction_symmetry=0.5)])
def test_bad_values_and_shapes_are_rejected_before_any_upload(kw):
    env = _vec("OctoArmSingle-v0", 6)
    with pytest.raises(ValueError):
        env.set_contact(**kw)
    assert env.backend.calls == []
    with pytest.raises(ValueError):
        env.set_contact(np.ones(4, bool), contact_k=2.0)                    # mask of the wrong length
    assert env.backend.calls == []


def test_a_bad_value_outside_the_mask_does_not_matter():
    env = _vec("OctoFlat-v0", 3)
    env.set_contact(np.array([1, 0, 1], bool), contact_k=np.array([90.0, -1.0, 110.0]),
                    kinetic_mu=np.array([[0.1, 0.2, 0.3], [np.nan, 0, 0], [0.4, 0.5, 0.6]]))
    got = env.contact()
    np.testing.assert_array_equal(got["contact_k"], [90.0, env.cfg.contact_k, 110.0])
    np.testing.assert_array_equal(got["kinetic_mu"][1], list(env.cfg.kinetic_mu))


def test_oracle_backend_refuses(oracle_built):
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend

    env = _vec("OctoArmSingle-v0", 2, backend_cls=OracleBackend)
    with pytest.raises(NotImplementedError):
        env.set_contact(contact_k=50.0)
    np.testing.assert_array_equal(env.contact()["contact_k"], env.cfg.contact_k)


REFUSED = [("SoftPendulum-v0", {}), ("SoftPendulum3D-v0", {}), ("SoftArmTracking-v0", {}), ("OctoArmPush-v1", {}),
           ("OctoCrawl-v0", {}), ("OctoArmSingle-v0", dict(n_elems=100))]


@pytest.mark.parametrize("env_id,kw", REFUSED, ids=[r[0] + ("-n100" if r[1] else "") for r in REFUSED])
def test_out_of_scope_envs_refuse_before_any_upload(env_id, kw):
    env = _vec(env_id, 2, **kw)
    with pytest.raises(NotImplementedError, match="per-env contact"):
        env.set_contact(contact_k=50.0)
    assert env.backend.calls == []


def test_tapered_arm_wider_octoflat_and_other_planes_refuse():
    env = _vec("OctoArmSingle-v0", 2)
    env.backend._tables["radius_profile"] = b"x"
    with pytest.raises(NotImplementedError, match="tapered"):
        env.set_contact(contact_k=50.0)
    env = _vec("OctoFlat-v0", 2, n_elems=20)                   # 8 arms x 32 lanes: four waves per env
    assert _capi.octo_waves_per_env(env.cfg) == 4
    with pytest.raises(NotImplementedError, match="more than two waves|at most two waves"):
        env.set_contact(contact_k=50.0)
    cfg = _capi.arm_single_config(2)
    assert _capi.env_contact_refusal(cfg) is None
    cfg.plane_normal[0], cfg.plane_normal[2] = 0.6, 0.8
    assert "e_z" in _capi.env_contact_refusal(cfg)
    assert _capi.octo_waves_per_env(_capi.octo_flat_config(1)) == 2
    assert _capi.octo_waves_per_env(_capi.octo_flat_config(1, n_arm=1, n_action=8)) == 1


def test_single_envs_forward_with_one_env():
    from gym_softrobot_amd.envs.arm_single import ArmSingleEnv
    from gym_softrobot_amd.envs.base import SingleEnvContact
    from gym_softrobot_amd.envs.octo_flat import FlatEnv

    assert issubclass(ArmSingleEnv, SingleEnvContact) and issubclass(FlatEnv, SingleEnvContact)
    for env_id in ("OctoArmSingle-v0", "OctoFlat-v0"):
        e = SingleEnvContact()
        e._vec = _vec(env_id, 1)
        e.set_contact(contact_k=300.0, kinetic_mu=[0.1, 0.2, 0.3])
        got = e.contact()
        assert got["contact_k"] == 300.0 and got["contact_nu"] == e._vec.cfg.contact_nu
        assert got["kinetic_mu"].tolist() == [0.1, 0.2, 0.3] and got["static_mu"].tolist() == [0.2, 0.4, 0.6]
        e.set_contact(friction_multiplier=1.0)
        assert e.contact()["kinetic_mu"].tolist() == list(e._vec.cfg.kinetic_mu)


def test_header_and_exports_carry_the_entry_point():
    h = (ROOT / "include" / "softrod.h").read_text()
    assert "int softrod_set_env_contact(softrod_handle* h, const double* contact, const uint8_t* mask, void* stream);" in h
    assert "softrod_set_env_contact" in _capi.EXPORTED_SYMBOLS
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


def _loop(isa_text, key):
    sys.path.insert(0, str(ROOT / "tools"))
    import hot_path_isa

    ins, labels = hot_path_isa.function_body(isa_text, key)
    return ins, hot_path_isa.hot_path(ins, labels)


ENV_CONTACT, ENV_MAT = 1 << 27, 1 << 28      # kFeatEnvContact, kFeatEnvMaterial
ARM, OCTO = 1073742601, 1073743625           # SOFTROD_FEATURES_ARM_SINGLE | zup, SOFTROD_FEATURES_OCTO_FLAT | zup
# (uniform twin, the new instantiation, loop budget of test_codegen.py: VALU, register copies, v_readlane)
FAST_TWINS = [
    ("fast_kernelILj1073742601ELi3ELi1ELb0E", f"fast_kernelILj{ARM | ENV_CONTACT}ELi3ELi1ELb0E", (535, 8, 4)),
    ("fast_kernelILj1073742601ELi3ELi1ELb0E", f"fast_kernelILj{ARM | ENV_CONTACT | ENV_MAT}ELi3ELi1ELb0E", (535, 8, 4)),
]


@pytest.mark.parametrize("twin,key,budget", FAST_TWINS, ids=["contact", "contact+material"])
def test_env_contact_fast_kernels_match_their_uniform_twin(isa_text, twin, key, budget):
    m, t = _meta(isa_text, key), _meta(isa_text, twin)
    print(f"{key}: {m}; twin {t}")
    assert m["vgpr_count"] == t["vgpr_count"] and m["agpr_count"] == t["agpr_count"], (m, t)
    assert m["vgpr_spill_count"] <= t["vgpr_spill_count"], (m, t)
    assert m["private_segment_fixed_size"] <= t["private_segment_fixed_size"], (m, t)
    ins, path = _loop(isa_text, key)
    tins, tpath = _loop(isa_text, twin)
    valu = [x for x in path if x.startswith("v_")]
    valu_max, copies_max, readlane_max = budget
    assert len(valu) <= valu_max, f"{key}: {len(valu)} VALU instructions per substep"
    assert len(valu) == len([x for x in tpath if x.startswith("v_")])
    assert sum(x.startswith("v_mov_b64") for x in valu) <= copies_max, key
    assert sum(x.startswith("v_readlane") for x in valu) <= readlane_max, key
    assert not [x for x in path if x.startswith(("scratch", "global", "buffer", "flat"))], key
    # the env's row arrives through scalar loads (wave-uniform address): no more vector loads than the twin
    assert sum(x.startswith("global_load") for x in ins) == sum(x.startswith("global_load") for x in tins)


def test_env_contact_octo_kernels_keep_their_twins_budget(isa_text):
    """The OctoFlat instantiations read their env slot's LDS table where the uniform ones read the workgroup's one.
    One env per workgroup (OctoFlatLite-v0): slot 0, the same registers, scratch and loop as the twin.  Four envs per
    workgroup (OctoFlat-v0): the slot's address is one more live VGPR in a kernel that has none to spare, so one
    more VGPR is spilled — the LDS post address of the head exchange, reloaded once per substep (3 scratch reloads
    on the walked path against the twin's 2); the VALU count is the twin's."""
    for twin, key, extra in ((f"octo_step_kernelILj{OCTO}ELi2ELi1E", f"octo_step_kernelILj{OCTO | ENV_CONTACT}ELi2ELi1E", 0),
                             (f"octo_step_kernelILj{OCTO}ELi2ELi4E", f"octo_step_kernelILj{OCTO | ENV_CONTACT}ELi2ELi4E", 1)):
        m, t = _meta(isa_text, key), _meta(isa_text, twin)
        print(f"{key}: {m}; twin {t}")
        assert m["vgpr_count"] == t["vgpr_count"] and m["agpr_count"] == t["agpr_count"], (m, t)
        assert m["vgpr_spill_count"] <= t["vgpr_spill_count"] + extra, (m, t)
        assert m["private_segment_fixed_size"] <= t["private_segment_fixed_size"] + 4 * extra, (m, t)
        _, path = _loop(isa_text, key)
        _, tpath = _loop(isa_text, twin)
        valu = [x for x in path if x.startswith("v_")]
        assert len(valu) <= 685 and len(valu) == len([x for x in tpath if x.startswith("v_")]), key
        assert sum(x.startswith("v_mov_b64") for x in valu) <= 16, key
        assert sum(x.startswith("v_readlane") for x in valu) <= 10, key
        mem = [x for x in path if x.startswith(("scratch", "global", "buffer", "flat"))]
        tmem = [x for x in tpath if x.startswith(("scratch", "global", "buffer", "flat"))]
        assert all(x.startswith("scratch_load") for x in mem) and len(mem) <= len(tmem) + extra, (key, mem)
