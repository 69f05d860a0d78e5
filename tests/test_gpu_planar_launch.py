"""The SoftPendulum launch around its substep loop: a planar rod in range stores only the twelve rows its step
changes and keeps nothing of the 3-D lane state; every other rod — pushed out of the plane through the state
view, holding a NaN, or in a launch with nothing to integrate — goes HBM -> HBM through the out-of-line cold
call and is read back for the epilogue (softrod_fast.hpp).  Held here: the kinds do not disturb each other in
one batch, the rows a planar step does not write stay the bytes they were, and all kinds match the C oracle.

Rod sizes: 50 elements (13 padding lanes), 63 (no padding lane), 5.

Padding lanes (the lanes past the end node's: 13 at 50 elements, none at 63) of the rows a planar step DOES
write.  x, v, d3 and the tangents' x, y are not written there at all (planar_store's `stepped`; it rests on the
kernel's prologue touching only node 0 / element 0): equal BYTES from the first step on.  d1, omega_2 and the
tangents' z are written in every lane because the planar path REBUILDS them, exactly as the launch before this
rework did (every state row is held byte-equal to that build's, tools/step_ab.py), and nothing reads those lanes:
  * d1 = (-s2 s, s2 c) from d3 (softrod_planar.hpp: "the only non-identical step", one rounding away from the
    frame a reset fills those lanes with): the FIRST step after a reset may move it by at most one ulp of 1
    (2^-52: director entries are <= 1 in magnitude); d3 does not move there, so the rebuilt d1 is a fixed point
    and every later step leaves the bytes alone;
  * omega_2 = s2 * 0 and the tangents' z = 0 are zeros whose SIGN the first step may set (s2 = -1): equal values
    on the first step, equal bytes from the second on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5
SIZES = (50, 63, 5)
KINDS = ("planar", "out-of-plane", "nan", "planar", "tiny-out-of-plane")
STEPS = 3
FIRST_STEP_PADDING_ULP = 2.0 ** -52
REBUILT_D1 = {("director", 0), ("director", 1)}          # rows the planar path rebuilds in every lane (see above)
REBUILT_ZEROS = {("omega", 1), ("tangents", 2)}
ROWS = {"position": 3, "velocity": 3, "director": 9, "omega": 3, "tangents": 3}
WRITTEN = {"position": (0, 1), "velocity": (0, 1), "director": (0, 1, 6, 7), "omega": (1,), "tangents": (0, 1, 2)}


def _theta(seed):
    from gym_softrobot_amd.seeding import initial_angle, np_random

    rng, _ = np_random(seed)
    return initial_angle(rng)


def _perturb(st, slot, kind, ne):
    """Writes the kind's disturbance through the state view; returns (array name, component, node slice, value)."""
    nodes = slice(1, min(ne, 30))
    if kind == "out-of-plane":
        what = ("velocity", 2, nodes, 0.3)
    elif kind == "tiny-out-of-plane":
        what = ("velocity", 2, nodes, 1e-200)
    elif kind == "nan":
        what = ("velocity", 0, slice(ne // 2, ne // 2 + 1), float("nan"))
    else:
        return None
    st[what[0]][what[1], slot, what[2]] = what[3]
    return what


def _snapshot(st):
    import torch

    torch.cuda.synchronize()
    out = {k: st[k].cpu().numpy().copy() for k in ROWS}
    out["time"] = st["time"].cpu().numpy().copy()
    return out


def _outputs(res):
    return [r.cpu().numpy().copy() for r in res[:4]]


@pytest.fixture(scope="module")
def runs(hip_lib, oracle_built):
    """Per rod size: the mixed batch's snapshots and outputs, each env's run alone, the oracle's outputs — once."""
    import torch

    import gym_softrobot_amd as gsa

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    out = {}
    for ne in SIZES:
        n = len(KINDS)
        acts = np.random.default_rng(11 + ne).uniform(-22, 22, (STEPS, n)).astype(np.float32)
        env = gsa.make_vec("SoftPendulum-v0", n, device=0, n_elems=ne)
        env.reset(seed=0)
        st = env.backend.state()
        rods = []
        for i, kind in enumerate(KINDS):
            what = _perturb(st, i, kind, ne)
            r = oracle_built.OracleRod(env.cfg)
            r.reset_pendulum(_theta(i))
            if what is not None:
                v = r.get("v")
                v[what[1], what[2]] = what[3]
                r.set("v", v)
            rods.append(r)
        snaps, outs = [_snapshot(st)], []
        for t in range(STEPS):
            outs.append(_outputs(env.step(acts[t])))
            snaps.append(_snapshot(st))
        env.close()
        alone = []
        for i, kind in enumerate(KINDS):
            e1 = gsa.make_vec("SoftPendulum-v0", 1, device=0, n_elems=ne)
            e1.reset(seed=[i])
            s1 = e1.backend.state()
            _perturb(s1, 0, kind, ne)
            o1, p1 = [], [_snapshot(s1)]
            for t in range(STEPS):
                o1.append(_outputs(e1.step(acts[t, i:i + 1])))
                p1.append(_snapshot(s1))
            e1.close()
            alone.append((p1, o1))
        oracle = [[r.env_step(acts[t, i]) for i, r in enumerate(rods)] for t in range(STEPS)]
        out[ne] = {"snaps": snaps, "outs": outs, "alone": alone, "oracle": oracle}
    return out


@pytest.mark.parametrize("ne", SIZES, ids=lambda n: f"n{n}")
def test_mixed_batch_equals_each_env_alone(runs, ne):
    r = runs[ne]
    for i, kind in enumerate(KINDS):
        p1, o1 = r["alone"][i]
        for t in range(STEPS + 1):
            for k in ROWS:
                assert r["snaps"][t][k][:, i].tobytes() == p1[t][k][:, 0].tobytes(), (kind, t, k)
            assert r["snaps"][t]["time"][i].tobytes() == p1[t]["time"][0].tobytes(), (kind, t)
        for t in range(STEPS):
            for a, b in zip(r["outs"][t], o1[t]):
                assert a[i].tobytes() == b[0].tobytes(), (kind, t)


@pytest.mark.parametrize("ne", SIZES, ids=lambda n: f"n{n}")
def test_planar_step_leaves_the_rows_it_does_not_write(runs, ne):
    snaps = runs[ne]["snaps"]
    planar = [i for i, k in enumerate(KINDS) if k == "planar"]
    for t in range(STEPS):
        before, after = snaps[t], snaps[t + 1]
        for k, comps in ROWS.items():
            for c in range(comps):
                for i in planar:
                    a, b = before[k][c, i], after[k][c, i]
                    if c not in WRITTEN[k]:                   # the nine rows planar_store does not write: whole rows
                        assert a.tobytes() == b.tobytes(), (t, k, c, i)
                        continue
                    first = ne + 1        # padding lanes: past the end node's lane (which steps, element slot included)
                    if t == 0 and (k, c) in REBUILT_D1:
                        assert np.all(np.abs(a[first:] - b[first:]) <= FIRST_STEP_PADDING_ULP), (t, k, c, i)
                    elif t == 0 and (k, c) in REBUILT_ZEROS:
                        assert np.all(a[first:] == 0.0) and np.all(b[first:] == 0.0), (t, k, c, i)
                    else:
                        assert a[first:].tobytes() == b[first:].tobytes(), (t, k, c, i)
    for i in planar:                                          # and the step did move the rod
        assert not np.array_equal(snaps[0]["position"][0, i, : ne + 1], snaps[1]["position"][0, i, : ne + 1])


@pytest.mark.parametrize("ne", SIZES, ids=lambda n: f"n{n}")
def test_all_kinds_match_the_oracle(runs, ne):
    r = runs[ne]
    for t in range(STEPS):
        obs, rew, term, trunc = r["outs"][t]
        for i, kind in enumerate(KINDS):
            o, rw, te, tr = r["oracle"][t][i]
            print(f"n{ne} step {t} {kind}: obs {obs[i]} oracle {o} reward {rew[i]} oracle {rw}")
            np.testing.assert_allclose(obs[i], o, rtol=RTOL, atol=1e-7, err_msg=f"{kind} step {t}")
            np.testing.assert_allclose(rew[i], rw, rtol=RTOL, atol=1e-9, err_msg=f"{kind} step {t}")
            assert bool(term[i]) == te and bool(trunc[i]) == tr, (kind, t)
    x = r["snaps"][STEPS]["position"]
    assert np.all(x[2, 0] == 0.0) and np.abs(x[2, 1]).max() > 1e-4          # env 0 stayed planar, env 1 really left
    assert np.isnan(x[:, 2, : ne + 1]).all()                                 # the dead env is NaN throughout


def test_zero_substep_launch(hip_lib, oracle_built):
    """n_substeps = 0 is reachable through the C API (softrod_config allows it): the launch constrains, stores and
    runs the epilogue on the resident state — through the cold call now.  Mixed batch against each env alone,
    bitwise; the state keeps its values; the outputs match the oracle's prologue + epilogue."""
    import torch

    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    ne, kinds = 50, ("planar", "out-of-plane", "nan")
    act = np.array([3.0, -7.0, 11.0], np.float32)

    def launch(n, seeds, which):
        cfg = _capi.softpendulum_config(n, n_elems=ne)
        cfg.n_substeps = 0
        be = HipRodBackend(cfg, 0)
        be.reset(np.array([_theta(s) for s in seeds]))
        st = be.state()
        for slot, kind in enumerate(which):
            _perturb(st, slot, kind, ne)
        before = _snapshot(st)
        res = _outputs(be.step(torch.from_numpy(act[list(seeds)]).cuda()))
        after = _snapshot(st)
        be.close()
        return cfg, before, res, after

    cfg, before, res, after = launch(3, (0, 1, 2), kinds)
    for k in ROWS:
        np.testing.assert_array_equal(before[k], after[k])               # (NaN equals NaN here)
    for i, kind in enumerate(kinds):
        _, _, r1, a1 = launch(1, (i,), (kind,))
        for k in ROWS:
            assert after[k][:, i].tobytes() == a1[k][:, 0].tobytes(), (kind, k)
        for a, b in zip(res, r1):
            assert a[i].tobytes() == b[0].tobytes(), kind
        rod = oracle_built.OracleRod(cfg)
        rod.reset_pendulum(_theta(i))
        what = _perturb({k: np.zeros((c, 1, 64)) for k, c in ROWS.items()}, 0, kind, ne)
        if what is not None:
            v = rod.get("v")
            v[what[1], what[2]] = what[3]
            rod.set("v", v)
        o, rw, te, tr = rod.env_step(act[i])
        print(f"zero-substep {kind}: obs {res[0][i]} oracle {o} reward {res[1][i]} oracle {rw}")
        np.testing.assert_allclose(res[0][i], o, rtol=RTOL, atol=1e-7, err_msg=kind)
        np.testing.assert_allclose(res[1][i], rw, rtol=RTOL, atol=1e-9, err_msg=kind)
        assert bool(res[2][i]) == te and bool(res[3][i]) == tr, kind
