"""Product-library hygiene (VERDICT r4 "next" #7):

* the A/B switches of the measurement builds (SOFTROD_NO_WINDOW, ...) change the
  kernel tier ONLY together with SOFTROD_DEBUG_SWITCHES=1 — a stray variable in a product process does
  nothing (softrod_kernel_tier, ABI v15, reports what softrod_create selected);
* every set-up entry point (softrod_autoreset_enable, softrod_bank_create, ...) leaves the handle as it was when one
  of its calls fails, holds nothing of the failed attempt, and can be retried.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch


def test_switches_change_the_kernel_tier_only_behind_the_gate(torch_gpu, hip_lib, monkeypatch):
    from gym_softrobot_amd import _capi
    from gym_softrobot_amd.backend import HipRodBackend

    octo, arm = _capi.octo_flat_config(4), _capi.arm_single_config(4, n_elems=100)
    plain = {}
    for name, cfg in (("octo", octo), ("arm", arm)):
        be = HipRodBackend(cfg, device=0)
        plain[name] = be.kernel_tier()
        be.close()
    assert plain["octo"] == "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>"
    assert plain["arm"].startswith("softrod_step_window_kernel<ArmSingle,4 rods/wg>")
    stray = {"SOFTROD_OCTO_ONE_WAVE": "1", "SOFTROD_OCTO_ONE_ENV_PER_BLOCK": "1", "SOFTROD_NO_WINDOW": "1",
             "SOFTROD_WINDOW_PAIRED": "0", "SOFTROD_WINDOW_REFRESH": "1"}
    for k, v in stray.items():
        monkeypatch.setenv(k, v)
    for name, cfg in (("octo", octo), ("arm", arm)):                 # stray variables alone: nothing changes
        be = HipRodBackend(cfg, device=0)
        assert be.kernel_tier() == plain[name]
        be.close()
    monkeypatch.setenv("SOFTROD_DEBUG_SWITCHES", "1")                 # with the gate they are honoured
    be = HipRodBackend(octo, device=0)                                # the retired OctoFlat switches stay retired
    assert be.kernel_tier() == "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>"
    be.close()
    be = HipRodBackend(arm, device=0)
    assert "window" not in be.kernel_tier() and "epl=2" in be.kernel_tier()
    be.close()
    monkeypatch.delenv("SOFTROD_NO_WINDOW")
    be = HipRodBackend(arm, device=0)
    assert "1 rod/wg,s_barrier" in be.kernel_tier() and "refresh=1 " in be.kernel_tier()
    be.close()


def test_tiers_of_the_registered_envs(torch_gpu, hip_lib):
    import gym_softrobot_amd as gsa

    want = {"SoftPendulum-v0": "softrod_step_fast_kernel<SoftPendulum,epl=1>",
            "SoftPendulum3D-v0": "softrod_step_fast_kernel<SoftPendulum3D,epl=1>",
            "OctoArmSingle-v0": "softrod_step_fast_kernel<ArmSingle,epl=1>",
            "OctoFlat-v0": "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>"}
    for env_id, tier in want.items():
        env = gsa.make_vec(env_id, 2, device=0)
        assert env.backend.kernel_tier() == tier
        env.close()


# ---- a failed set-up leaves the handle as it was and can be retried -------------------------------------------------
N_SETUP = 64
MIB = 1 << 20
PENDULUM = ("SoftPendulum-v0", dict(final_time=0.1))          # (truncation on the third step)


def _host(tensors):
    return [np.array(t.detach().cpu().numpy()) for t in tensors]


def _refused(be, entry, args, text):
    """The view `entry` still refuses the handle, in the words it has for a feature that is off."""
    from gym_softrobot_amd import _capi

    with pytest.raises(_capi.SoftrodError, match=text):
        _capi.check(getattr(be._lib, entry)(be._h, *args), be._h)


def _steps(be, acts, extra=lambda be: ()):
    out = []
    for a in acts:
        out += _host(be.step(a)) + _host(extra(be))
    return out


def _material(be):
    from gym_softrobot_amd import _capi

    return np.tile(_capi.env_material_defaults(be.cfg), (N_SETUP, 1)) * np.linspace(0.5, 1.5, N_SETUP)[:, None]


def _kappa_pool(be, entries):
    ne = int(be.cfg.n_elem)
    return np.random.default_rng(5).uniform(-0.5, 0.5, (entries, 1, 3, ne - 1))


class _Setup:
    """One set-up entry point: the env it runs on, what the handle has before it (`prepare`), the call, what says that
    the feature is still off, the device bytes a successful call allocates where the call has a size parameter of its own
    (`sized`; None: sized by n_envs x obs_dim alone), and four steps that exercise the feature (`exercise` -> arrays)."""
    env = PENDULUM
    sized = None

    def prepare(self, be):
        pass

    def still_off(self, be):
        pass


class _AutoresetEnable(_Setup):
    depth = 512

    def sized(self, be):
        return N_SETUP * self.depth * 18 * 8                 # the ring: [depth][n_envs][18] doubles

    def call(self, be):
        be.autoreset_enable(self.depth)

    def still_off(self, be):
        _refused(be, "softrod_queue_status_begin", (None,), "call softrod_autoreset_enable first")

    def exercise(self, be, acts):
        from gym_softrobot_amd import _capi

        with pytest.raises(_capi.SoftrodError, match="already enabled"):
            be.autoreset_enable(4)
        be.queue_push(np.linspace(1.5, 1.6, N_SETUP)[:, None], np.ones(N_SETUP, np.int32))
        out = _steps(be, acts)                               # the first truncates every env, the second restarts it
        assert out[3].all() and not out[7].any(), "the auto-reset did not restart the truncated envs"
        consumed, underflow = be.queue_status()
        return out + [np.asarray(consumed), np.asarray(underflow)]


class _AutoresetSameStep(_Setup):
    def prepare(self, be):
        be.autoreset_enable(4)          # two starts per env: the first and the fourth of the four steps end an episode
        be.queue_push(np.linspace(1.5, 1.6, 2 * N_SETUP).reshape(N_SETUP, 2), np.full(N_SETUP, 2, np.int32))

    def call(self, be):
        be.autoreset_same_step(True)

    def still_off(self, be):
        import ctypes as C

        ptrs = [C.c_void_p() for _ in range(3)]
        _refused(be, "softrod_final_view", [C.byref(p) for p in ptrs], "call softrod_autoreset_same_step first")

    def exercise(self, be, acts):
        out = _steps(be, acts, lambda be: (be.final_obs, be.final_time))
        assert out[3].all(), "the first step did not truncate"
        return out


class _EnvMaterial(_Setup):
    def call(self, be):
        be.set_env_material(_material(be))

    def exercise(self, be, acts):
        assert be.kernel_tier().endswith(",env material")
        return _steps(be, acts)


class _EnvContact(_Setup):
    env = ("OctoArmSingle-v0", {})

    def call(self, be):
        from gym_softrobot_amd import _capi

        be.set_env_contact(np.tile(_capi.env_contact_defaults(be.cfg), (N_SETUP, 1)) * np.linspace(0.5, 1.5, N_SETUP)[:, None])

    def exercise(self, be, acts):
        assert be.kernel_tier().endswith(",env contact")
        return _steps(be, acts)


class _BankCreate(_Setup):
    """On a handle that already has a material table and a pool, so that the bank twins their rows too."""

    def prepare(self, be):
        be.set_env_material(_material(be))
        be.set_reset_shapes(kappa=_kappa_pool(be, 3), seed=1)

    def slots(self, be):
        return 4 * MIB // be.bank_info()[1] + 1

    def sized(self, be):
        return self.slots(be) * be.bank_info()[1]

    def call(self, be):
        be.bank_create(self.slots(be))

    def still_off(self, be):
        assert be.bank_info()[0] == 0

    def exercise(self, be, acts):
        envs = np.arange(N_SETUP)
        out = _steps(be, acts[:1])
        be.bank_save(envs, envs[::-1].copy())
        out += _steps(be, acts[1:3])
        be.bank_load(envs, envs)                             # every env goes on from its mirror image's saved state
        return out + _steps(be, acts[3:]) + [be.bank_info()[2]]


class _EpisodeStats(_Setup):
    ring = 200_000

    def sized(self, be):
        return self.ring * (8 + 4 + 8 + 4)                   # the ring's return, length, time and env arrays

    def call(self, be):
        be.episode_stats_enable(self.ring)

    def still_off(self, be):
        import ctypes as C
        from gym_softrobot_amd import _capi

        _refused(be, "softrod_episode_stats_view", (C.byref(_capi.SoftrodEpisodeStatsView()),), "the feature is off")

    def exercise(self, be, acts):
        out = _steps(be, acts, lambda be: [be.episode_stats[k] for k in ("acc_return", "acc_length", "count")])
        assert out[3].all() and int(be.episode_stats["count"][0]) == N_SETUP, "the first step did not end every episode"
        return out + _host([be.episode_stats["ring_r"][:N_SETUP], be.episode_stats["ring_env"][:N_SETUP]])


class _Normalize(_Setup):
    def call(self, be):
        be.normalize_enable(True, True)

    def still_off(self, be):
        import ctypes as C
        from gym_softrobot_amd import _capi

        _refused(be, "softrod_normalize_view", (C.byref(_capi.SoftrodNormalizeView()),), "the feature is off")

    def exercise(self, be, acts):
        return _steps(be, acts, lambda be: [be.normalize[k] for k in ("norm_obs", "norm_reward", "obs_mean", "ret_var")])


class _ResetShapes(_Setup):
    """The first pool of a handle that already has a bank, so that the bank twins the two new rows."""
    entries = 3600

    def prepare(self, be):
        be.bank_create(4)

    def sized(self, be):
        return self.entries * 3 * (int(be.cfg.n_elem) - 1) * 8      # the kappa field: [entries][1][3][n_elem - 1] doubles

    pool = None         # on the device once, ahead of the memory readings: torch's allocator takes no new segment between them

    def call(self, be):
        import torch

        if self.pool is None:
            self.pool = torch.as_tensor(_kappa_pool(be, self.entries), device=be.device)
        be.set_reset_shapes(kappa=self.pool, seed=7)

    def still_off(self, be):
        import ctypes as C

        ptrs = [C.c_void_p() for _ in range(2)]
        _refused(be, "softrod_reset_shapes_view", [C.byref(p) for p in ptrs], "no pool is set")

    def exercise(self, be, acts):
        mask = (np.arange(N_SETUP) % 3 == 0).astype(np.uint8)
        out = _steps(be, acts[:2])
        be.reset(np.linspace(1.5, 1.6, N_SETUP), mask)
        be.apply_reset_shapes(mask)
        out += _host([be.observe(None), be.reset_shape_index, be.reset_shape_episode])
        assert (out[-2][mask != 0] >= 0).all() and (out[-2][mask == 0] == -1).all()
        return out + _steps(be, acts[2:])


SETUPS = {"autoreset_enable": _AutoresetEnable, "autoreset_same_step": _AutoresetSameStep, "set_env_material": _EnvMaterial,
          "set_env_contact": _EnvContact, "bank_create": _BankCreate, "episode_stats_enable": _EpisodeStats,
          "normalize_enable": _Normalize, "set_reset_shapes": _ResetShapes}


@pytest.mark.parametrize("name", list(SETUPS))
def test_a_failed_setup_leaves_the_handle_as_it_was_and_can_be_retried(torch_gpu, hip_lib, monkeypatch, name):
    """SOFTROD_DEBUG_FAIL_SETUP_CALL=k (honoured only under SOFTROD_DEBUG_SWITCHES=1) makes the k-th fallible call of a
    set-up fail without being made.  For each set-up entry point, k = 1, 2, ... until the call succeeds (on a handle of
    its own; by k = 64 at the latest), which gives the number K of its fallible calls without naming it here; then every
    k = 1 .. K on the handle under test.  After every failed attempt, host checks first: the error names the injection,
    kernel_tier() is what it was, and the feature is still off by its own view's refusal (bank_info's slots for the
    bank; the per-env tables have no view, their tier says it).  Then the handle steps twice like an untouched twin of
    the same seed, the retry without the variable succeeds, and four steps that exercise the feature equal the twin's,
    on which the same call succeeded at the first go — bit for bit.

    Free device memory is compared (within 2 MiB after four rounds of all K failures) only for the set-ups with a size
    parameter of their own — queue depth, ring length, bank slots, pool entries — chosen so that one successful call
    allocates at least 4 MiB, asserted from the shapes.  The set-ups sized by n_envs x obs_dim alone (same-step rows,
    per-env tables, normalisation) allocate a few KiB at 64 envs, below what hipMemGetInfo resolves, so a memory
    assertion on them would pass whatever the code did and is left out."""
    import gym_softrobot_amd as gsa
    from gym_softrobot_amd import _capi

    setup = SETUPS[name]()
    env_id, kw = setup.env

    def make():
        e = gsa.make_vec(env_id, N_SETUP, device=0, **kw)
        e.reset(seed=3)
        setup.prepare(e.backend)
        return e

    def attempt_fails(be, k):
        tier = be.kernel_tier()
        monkeypatch.setenv("SOFTROD_DEBUG_FAIL_SETUP_CALL", str(k))         # around this call only: `prepare` makes set-ups too
        try:
            setup.call(be)
        except _capi.SoftrodError as err:
            assert f"injected failure at call {k}" in str(err), str(err)
            assert be.kernel_tier() == tier
            setup.still_off(be)
            return True
        finally:
            monkeypatch.delenv("SOFTROD_DEBUG_FAIL_SETUP_CALL")
        return False

    monkeypatch.setenv("SOFTROD_DEBUG_SWITCHES", "1")
    probe = make()
    calls = next((k - 1 for k in range(1, 65) if not attempt_fails(probe.backend, k)), None)
    probe.close()
    assert calls is not None, "the set-up still fails at k = 64"
    assert calls >= 1, "the set-up made no fallible call through the injection point"

    env, twin = make(), make()
    be = env.backend
    sized = setup.sized(be) if setup.sized else None
    if sized is not None:
        assert sized >= 4 * MIB, f"a successful call allocates {sized} bytes: too little to show in hipMemGetInfo"
    torch_gpu.cuda.synchronize()
    free0 = torch_gpu.cuda.mem_get_info(0)[0]
    for _ in range(4 if sized is not None else 1):
        for k in range(1, calls + 1):
            assert attempt_fails(be, k), f"call {k} of {calls} did not fail"
    torch_gpu.cuda.synchronize()
    if sized is not None:
        held = free0 - torch_gpu.cuda.mem_get_info(0)[0]
        assert held < 2 * MIB, f"{held / MIB:.1f} MiB still allocated after four rounds of {calls} failed attempts"
    monkeypatch.delenv("SOFTROD_DEBUG_SWITCHES")

    lo, hi = (-22, 22) if env_id == "SoftPendulum-v0" else (-1, 1)
    acts = np.random.default_rng(0).uniform(lo, hi, (6, N_SETUP, be.action_dim)).astype(np.float32)
    for x, y in zip(_steps(be, acts[:2]), _steps(twin.backend, acts[:2])):      # the failed attempts left the stepping path alone
        np.testing.assert_array_equal(x, y)
    setup.call(be)                                  # the retry
    setup.call(twin.backend)
    a, b = setup.exercise(be, acts[2:]), setup.exercise(twin.backend, acts[2:])
    assert len(a) == len(b) and len(a) >= 16
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    env.close()
    twin.close()
