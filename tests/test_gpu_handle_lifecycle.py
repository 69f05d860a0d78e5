"""Two lives of a handle in one process: nothing of a destroyed handle survives into the next one.

Every device buffer, pinned buffer and event of a handle is a member that releases itself when softrod_destroy
deletes the handle (csrc/softrod_owned.hpp).  The allocation patterns — a plain rod with a per-env material table and
the auto-reset ring; the tapered muscle arm with early_termination's aux rows; the muscle octopus with its per-arm
suckers, aux rows and prev_kappa; an arm with every feature that brings memory of its own; a same-step pendulum with
a pool, statistics and normalisation — are each created, set up, reset, stepped once, read out and closed, twice;
every call returns OK (the binding raises otherwise) and the second life's observation, reward and read-outs
equal the first's bit for bit.  A row of lives of the fullest one leaves free device memory where it was."""
import gc

import numpy as np
import pytest
import torch

import gym_softrobot_amd as gsa
from gym_softrobot_amd import _capi

pytestmark = pytest.mark.gpu

N = 2


def _soft_pendulum():
    env = gsa.make_vec("SoftPendulum-v0", N, n_elems=2)      # (softrod_create: 2 <= n_elem)
    material = np.tile(_capi.env_material_defaults(env.cfg), (N, 1))
    material[1] *= (0.5, 0.5, 1.25, 2.0)
    env.backend.set_env_material(material, np.array([0, 1], np.uint8))
    env.backend.autoreset_enable(2)
    return env


def _arm_push():
    return gsa.make_vec("OctoArmPush-v0", N, config_early_termination=True)    # (its radius profile and muscle layers)


def _crawl():
    return gsa.make_vec("OctoCrawl-v0", N)


def _arm_single_all(n=N, slots=2, ring=8, entries=3, sizes=None):
    """OctoArmSingle-v0 with every feature that brings device memory of its own: both per-env tables, a state bank (the
    life saves, forks and loads: _arm_single_after_reset), a pool of start shapes, episode statistics, normalisation,
    timing.  `sizes`: filled with the device bytes of each feature's allocation, from bank_info's bytes_per_slot — which
    grows by one table row with each per-env table — and the shapes of the views."""
    env = gsa.make_vec("OctoArmSingle-v0", n)
    be = env.backend
    per_slot = [be.bank_info()[1]]
    material = np.tile(_capi.env_material_defaults(env.cfg), (n, 1))
    material[1] *= (0.5, 0.5, 1.25, 2.0)
    be.set_env_material(material)
    per_slot.append(be.bank_info()[1])
    contact = np.tile(_capi.env_contact_defaults(env.cfg), (n, 1))
    contact[1] *= 0.5
    be.set_env_contact(contact)
    per_slot.append(be.bank_info()[1])
    kappa = np.random.default_rng(2).uniform(-0.5, 0.5, (entries, 1, 3, int(env.cfg.n_elem) - 1))
    env.set_reset_shapes(kappa=kappa, seed=4)
    env.create_state_bank(slots)
    env.record_episode_statistics(ring)
    env.set_normalization(True, True)
    be.set_timing(4)
    if sizes is not None:
        nbytes = lambda views: sum(v.numel() * v.element_size() for v in views.values())     # noqa: E731
        sizes.update(material=n * (per_slot[1] - per_slot[0]), contact=n * (per_slot[2] - per_slot[1]), pool=kappa.nbytes,
                     bank=slots * be.bank_info()[1], statistics=nbytes(be.episode_stats), normalization=nbytes(be.normalize))
    return env


def _arm_single_after_reset(env):
    env.save_states([0, 1], [1, 0])
    env.fork([0], [1])                  # env 1 becomes env 0 ...
    env.load_states([0], [1])           # ... and then itself again, from the slot
    assert env.backend.bank_info()[2][:2].all()


_arm_single_all.after_reset = _arm_single_after_reset


def _soft_pendulum_same_step():
    """SoftPendulum-v0 whose first step ends every episode and restarts it in the same call, from the pool."""
    env = gsa.make_vec("SoftPendulum-v0", N, autoreset="same_step", final_time=0.03)
    kappa = np.random.default_rng(2).uniform(-0.5, 0.5, (3, 1, 3, int(env.cfg.n_elem) - 1))
    env.set_reset_shapes(kappa=kappa, seed=4)
    env.record_episode_statistics(8)
    env.set_normalization(True, True)
    return env


def _life(make):
    env = make()
    out = {}
    obs, _ = env.reset(seed=0)
    out["reset_obs"] = obs.clone()          # (a view of the buffer the step overwrites)
    if hasattr(make, "after_reset"):
        make.after_reset(env)
    obs, reward, term, trunc, _ = env.step(np.zeros((N, env.action_dim), np.float32))
    out.update(obs=obs, reward=reward, terminated=term, truncated=trunc)
    be = env.backend
    for name, views in (("statistics.", be.episode_stats), ("normalization.", be.normalize)):
        out.update({name + k: v for k, v in (views or {}).items()})
    if getattr(be, "same_step", False):
        out.update(final_obs=be.final_obs, final_time=be.final_time)
    if be.reset_shapes_count:
        out.update(shape_index=be.reset_shape_index, shape_episode=be.reset_shape_episode)
    out["energies"] = env.rod_energies()
    out.update({"strains." + k: v for k, v in env.rod_strains()._asdict().items()})
    if _capi.ground_reaction_refusal(env.cfg) is None:
        out["reaction.force"], out["reaction.torque"] = env.ground_reaction()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    env.close()
    return out


@pytest.mark.parametrize("make", [_soft_pendulum, _arm_push, _crawl, _arm_single_all, _soft_pendulum_same_step],
                         ids=["soft_pendulum", "arm_push", "crawl", "arm_single_all", "soft_pendulum_same_step"])
def test_second_life_equals_the_first(hip_lib, make):
    first, second = _life(make), _life(make)
    assert first.keys() == second.keys()
    for k in first:
        assert first[k].shape == second[k].shape and first[k].tobytes() == second[k].tobytes(), k
    assert np.isfinite(first["obs"]).all() and np.isfinite(first["energies"]).all()


def test_closed_handles_give_their_device_memory_back(hip_lib):
    """Lives of the maker with every feature, created, reset, stepped once and closed in a row: free device memory after
    the last life is within 2 MiB of what it was after the second (the first two settle torch's own allocator).

    Sensitivity: the batch, the features' own sizes and the number of lives are chosen so that (lives - 2) times the
    smallest allocation a feature makes — the per-env tables, the pool, the bank, the statistics block, the
    normalisation block, each computed here from bank_info's bytes_per_slot and the views' shapes — is at least 8 MiB:
    lives that each kept any one of them would hold four times the bound at the end.  (The rows of n_envs ints or
    bytes beside them are below what hipMemGetInfo resolves.)  Positive control: while such a handle is open, free memory is lower than after it is closed by at least
    half those bytes, so the reading does see these allocations.  The reading takes in the Python side of a life too:
    a closed backend that kept its zero-copy views kept itself, and 1 MiB of torch buffers per life with it
    (HipRodBackend.close drops them).  Device memory only: pinned buffers and events do not
    show in this number; that they are released rests on every one of them being a member that owns it
    (csrc/softrod_owned.hpp)."""
    n, lives, mib = 8192, 13, 1 << 20
    sizes = {}

    def free_after_life():
        sizes.clear()
        env = _arm_single_all(n, slots=128, ring=65536, entries=4096, sizes=sizes)
        env.reset(seed=0)
        env.step(np.zeros((n, env.action_dim), np.float32))
        torch.cuda.synchronize()
        held = torch.cuda.mem_get_info(0)[0]
        env.close()
        del env
        # torch's side of a life — output buffers, the pool's tensor — is not the subject: the views and their backend
        # refer to each other, so they go with a collection, and the allocator's cached segments go back with them
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return held, torch.cuda.mem_get_info(0)[0]

    readings = [free_after_life() for _ in range(lives)]
    print("free MiB (open, closed) per life:", [(a >> 20, b >> 20) for a, b in readings], "feature bytes:", sizes)
    assert (lives - 2) * min(sizes.values()) >= 8 * mib, sizes
    open_, closed = readings[-1]
    assert closed - open_ >= sum(sizes.values()) // 2, f"an open handle shows {(closed - open_) / mib:.1f} MiB of {sizes}"
    leaked = readings[1][1] - readings[-1][1]
    assert abs(leaked) < 2 * mib, f"{leaked / mib:.1f} MiB between the second and the last of {lives} lives"
