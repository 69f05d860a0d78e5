"""The pin: the oracle — and, with -m gpu, the HIP library — against outputs of
the REFERENCE itself (gym_softrobot on pyelastica 1.0.0), recorded by tools/make_pyelastica_golden.py
into tests/golden/pyelastica_<env>_seed<k>.npz where `import elastica` works.  While those files do
not exist (pyelastica cannot be installed in the build container: no network, no wheel) the two
pin tests SKIP, and the stepper's parity stays "unpinned"; the remaining tests exercise the very
same record / replay code on fixtures the C oracle produces, so that the day the files arrive the
harness is known to work:
  * a replay of an oracle-made fixture through the oracle deviates by exactly 0;
  * a fixture made with a recalled detail flipped is NOT matched (the harness can fail);
  * (-m gpu) the HIP library replays oracle-made fixtures of all four envs within 1e-5 up to each
    env's strict horizon (tools/pyelastica_pin.py ENVS), raw substeps included.
Tolerance: 1e-5 relative to each record's scale with the per-field floors of pyelastica_pin.FLOOR
(BASELINE.json north_star: "within 1e-5 relative float tolerance")."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

import pyelastica_pin as pin  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
PINNED = pin.fixture_files(GOLDEN, "pyelastica")
TOL = 1e-5
needs_fixtures = pytest.mark.skipif(not PINNED, reason="no tests/golden/pyelastica_*.npz yet: run "
                                    "tools/make_pyelastica_golden.py where pyelastica 1.0.0 is installed")


def _check(driver_cls, files, switches, **kw):
    report = []
    for f in files:
        fx = dict(np.load(f, allow_pickle=False))
        env_id = str(fx["env_id"])
        drv = driver_cls(env_id, switches, **kw)
        dev = pin.compare_case(drv, fx)
        drv.close()
        n_strict = pin.ENVS[env_id]["strict_steps"]
        strict = {k: v for k, v in dev.items() if not k.startswith("step") or int(k[4:].split("_")[0]) <= n_strict}
        worst_rec = max(strict, key=lambda k: strict[k])
        report.append((f.name, pin.strict_worst(dev, env_id), pin.horizon(dev, TOL), len(fx["obs"]), worst_rec))
    for name, w, h, n, rec in report:
        print(f"{name}: strict-horizon deviation {w:.2e} (at {rec}); within {TOL:g} for the first {h} of {n} env.steps")
    bad = [(name, w, rec) for name, w, _, _, rec in report if not w <= TOL]
    assert not bad, f"outside {TOL:g}: {bad}"


@needs_fixtures
def test_oracle_matches_the_pyelastica_fixtures(oracle_built):
    _check(pin.OracleDriver, PINNED, pin.load_switches(GOLDEN))


@needs_fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("math_mode", [0, 1], ids=["libm", "fast"])
def test_hip_matches_the_pyelastica_fixtures(hip_lib, math_mode):
    _check(pin.HipDriver, PINNED, pin.load_switches(GOLDEN), math_mode=math_mode)


# ---- the harness itself, on fixtures the oracle makes -----------------------------------------

@pytest.fixture(scope="module")
def oracle_made(tmp_path_factory, oracle_built):
    import make_pyelastica_golden as gen

    out = tmp_path_factory.mktemp("oracle_made")
    assert gen.main(["--source", "oracle", "--out", str(out), "--seeds", "42", "--steps", "3"]) == 0
    files = pin.fixture_files(out, "oracle")
    assert len(files) == 4
    return files


def test_generator_refuses_to_pass_oracle_output_off_as_the_reference(tmp_path):
    import make_pyelastica_golden as gen

    with pytest.raises(SystemExit, match="refusing"):
        gen.main(["--source", "oracle", "--prefix", "pyelastica"])
    with pytest.raises(SystemExit, match="import elastica"):     # this container: no pyelastica -> nothing written
        gen.main(["--out", str(tmp_path)])
    assert not list(tmp_path.iterdir())


def test_fixture_layout(oracle_made):
    fx = dict(np.load([f for f in oracle_made if "SoftPendulum-v0" in f.name][0]))
    for n in pin.RAW_SUBSTEPS:
        assert fx[f"sub{n}_x"].shape == (3, 51) and fx[f"sub{n}_Q"].shape == (3, 3, 50)
    assert fx["obs"].shape == (3, 4) and fx["actions"].shape == (3, 1) and fx["actions"].dtype == np.float32
    assert fx["step1_x"].shape == (3, 51) and fx["step3_w"].shape == (3, 50) and "step2_x" not in fx
    assert float(fx["time"][0]) == pytest.approx(0.04, abs=1e-9)
    # the first draw of seed 42: theta0 = 92.7396 deg -> obs[3] = -0.04781435
    np.testing.assert_allclose(fx["reset_obs"], [0, 0, 0, -0.04781435], atol=1e-8)
    octo = dict(np.load([f for f in oracle_made if "OctoFlat" in f.name][0]))
    assert octo["sub100_x"].shape == (8, 3, 11) and octo["step1_head_Q"].shape == (3, 3) and octo["obs"].shape == (3, 461)


def test_oracle_replays_its_own_fixtures_exactly(oracle_made):
    for f in oracle_made:
        fx = dict(np.load(f))
        drv = pin.OracleDriver(str(fx["env_id"]))
        dev = pin.compare_case(drv, fx)
        assert pin.worst(dev) == 0.0, (f.name, {k: v for k, v in dev.items() if v})


@pytest.mark.parametrize("flip", [{"alpha_c": 4.0 / 3.0}, {"shear_modulus_over_E": 1 / 1.5}, {"time_two_half_adds": 0},
                                  {"damper_protocol": "uniform"}])
def test_a_flipped_detail_is_not_matched(oracle_made, flip):
    """The harness can fail: every large switch moves a one-rod env out of 1e-5 within the raw
    substeps or the first env.steps; the clock switch shows in the `time` records alone."""
    f = [f for f in oracle_made if "SoftPendulum3D" in f.name][0]
    fx = dict(np.load(f))
    drv = pin.OracleDriver("SoftPendulum3D-v0", flip)
    dev = pin.compare_case(drv, fx)
    if "time_two_half_adds" in flip:
        assert max(v for k, v in dev.items() if k.endswith("_time")) > 0
        assert pin.worst(dev, skip_time=True) < 1e-9
    else:
        assert pin.strict_worst(dev, "SoftPendulum3D-v0") > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("math_mode", [0, 1], ids=["libm", "fast"])
def test_hip_replays_oracle_made_fixtures(hip_lib, oracle_made, math_mode):
    """The -m gpu leg of the pin, run on what exists today: HipDriver (reset, raw substeps, env.steps,
    state read-back for one-rod envs and for the 8-arm octopus) against oracle-made files."""
    files = [f for f in oracle_made if not (math_mode == 0 and "OctoFlat" in f.name)]   # OctoFlat: fast mode only
    _check(pin.HipDriver, files, None, math_mode=math_mode)


FLIPPED = {
    "alpha_c + damp order + damper protocol": {"alpha_c": 4.0 / 3.0, "damp_before_constrain": 1, "damper_protocol": "uniform"},
    "shear modulus + contact order + clock": {"shear_modulus_over_E": 1.0 / 1.5, "contact_before_forcing": 1, "time_two_half_adds": 0},
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(FLIPPED), ids=list(FLIPPED))
def test_hip_follows_every_switch_the_sweep_can_select(hip_lib, oracle_built, tmp_path, which):
    """Whatever combination of recalled details a PyElastica fixture turns out to demand, the product
    path must need no kernel work: every switch of tools/pyelastica_pin.SWITCHES is a field of
    softrod_config that the HIP library honours like the oracle does.  Oracle-made fixtures with three
    switches flipped at a time are replayed through the HIP library under the same switches (1e-5,
    strict horizons) — and are NOT matched under the shipped defaults."""
    import make_pyelastica_golden as gen

    sw = FLIPPED[which]
    flips = []
    for k, v in sw.items():
        flips += ["--flip", f"{k}={v}" if isinstance(v, str) else f"{k}={v!r}"]
    assert gen.main(["--source", "oracle", "--out", str(tmp_path), "--prefix", "flipped", "--seeds", "1",
                     "--steps", "3"] + flips) == 0
    files = pin.fixture_files(tmp_path, "flipped")
    assert len(files) == 4
    one_rod = [f for f in files if "OctoFlat" not in f.name]
    _check(pin.HipDriver, one_rod, sw, math_mode=1)
    _check(pin.HipDriver, one_rod, sw, math_mode=0)
    # OctoFlat: a single force evaluation and ten substeps strictly (an operator in the wrong place shows
    # there at O(1)); the records further on at 1e-4 of the pin's floors — with the contact ahead of the
    # weight the arms bounce on the soft plane from the first substep on, and that chatter amplifies the
    # last bit faster than the default order does (1.7e-5 of the velocity floor after 100 substeps)
    (octo,) = [f for f in files if "OctoFlat" in f.name]
    fx = dict(np.load(octo, allow_pickle=False))
    drv = pin.HipDriver("OctoFlat-v0", sw, math_mode=1)
    dev = pin.compare_case(drv, fx)
    drv.close()
    early = {k: v for k, v in dev.items() if k.startswith(("reset", "sub1_", "sub10_"))}
    assert len(early) >= 17 and max(early.values()) <= TOL, early
    assert pin.strict_worst(dev, "OctoFlat-v0") <= 1e-4 and all(v == 0.0 for k, v in dev.items() if k.endswith(("_time", "_flags")))
    mismatched = 0
    for f in files:
        fx = dict(np.load(f, allow_pickle=False))
        drv = pin.HipDriver(str(fx["env_id"]), None, math_mode=1)
        dev = pin.compare_case(drv, fx)
        drv.close()
        mismatched += not pin.strict_worst(dev, str(fx["env_id"])) <= TOL
    assert mismatched >= 3                     # the defaults do not reproduce these files
