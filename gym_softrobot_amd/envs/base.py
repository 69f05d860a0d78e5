"""Shared host logic of the batched envs: seeding, masked/auto reset, step bookkeeping.

The reference has a single-env API only (no vector env, no auto-reset: a finished env is
reset by the caller, gym_softrobot/debug/make.py:16-23).  The batched form adds, per
SURVEY.md §8(f) N2:
  * `reset(mask=...)`  partial reset of a subset of the resident envs,
  * `autoreset=True`   Gymnasium-1.0 VectorEnv NEXT_STEP semantics: an env that returned
                       terminated/truncated at step t is reset (instead of stepped) by the
                       call at t+1, which returns its reset observation, reward 0 and both
                       flags False.  Costs one small device->host read of the flags per step.
  * `autoreset="device"`  the same semantics with no host round trip: the next
                       `queue_depth` resets of every env are drawn ahead of time from the
                       env's own NumPy stream (so the streams are the ones `autoreset=True`
                       would consume, draw for draw) and staged on the device
                       (softrod_queue_push*); the step applies them itself.  The host tops
                       the queue up within every `queue_depth` steps (one small non-blocking read).  `infos`
                       then carry device tensors.
  * `autoreset="same_step"`  Gymnasium-1.x AutoresetMode.SAME_STEP on the same staged queue: the call
                       that ends an env's episode returns that step's reward and flags, the NEW episode's
                       first observation in `obs`, and the terminal observation in infos["final_obs"]
                       (rows where infos["_final_obs"] = terminated | truncated), its clock in
                       infos["final_info"]["time"].  No env ever spends a call resetting, and value
                       targets of truncated episodes can bootstrap from the terminal observation.  One
                       cold kernel behind the step (csrc/softrod_autoreset.hpp); an env can use a
                       record per step, so the queue is topped up twice as often (`top_up_every`).
"""
from __future__ import annotations

import copy
from collections import deque
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np

from .. import _capi
from ..seeding import np_random
from ..spaces import Box

try:  # pragma: no cover
    from gymnasium import Env as GymEnv  # type: ignore
except Exception:  # noqa: BLE001
    class GymEnv:  # minimal stand-in for gymnasium.Env
        metadata: Dict[str, Any] = {}
        render_mode = None
        _np_random = None

        def reset(self, *, seed=None, options=None):
            if seed is not None:
                self._np_random, self._np_random_seed = np_random(seed)

        @property
        def np_random(self):
            if self._np_random is None:
                self._np_random, self._np_random_seed = np_random()
            return self._np_random

        @property
        def unwrapped(self):
            return self

        def close(self):
            pass


class SingleEnvMaterial:
    """set_material / material of a single env (its one-env vec env `_vec`): VecRodEnvBase.set_material with N = 1."""

    def set_material(self, *, youngs_modulus=None, shear_modulus=None, density=None, damping_constant=None):
        self._vec.set_material(youngs_modulus=youngs_modulus, shear_modulus=shear_modulus, density=density,
                               damping_constant=damping_constant)

    def material(self) -> Dict[str, float]:
        return {k: float(v[0]) for k, v in self._vec.material().items()}


class SingleEnvContact:
    """set_contact / contact of a single env (its one-env vec env `_vec`): VecRodEnvBase.set_contact with N = 1."""

    def set_contact(self, *, contact_k=None, contact_nu=None, kinetic_mu=None, static_mu=None,
                    friction_multiplier=None, friction_symmetry=None):
        self._vec.set_contact(contact_k=contact_k, contact_nu=contact_nu, kinetic_mu=kinetic_mu, static_mu=static_mu,
                              friction_multiplier=friction_multiplier, friction_symmetry=friction_symmetry)

    def contact(self) -> Dict[str, Any]:
        c = self._vec.contact()
        return {"contact_k": float(c["contact_k"][0]), "contact_nu": float(c["contact_nu"][0]),
                "kinetic_mu": c["kinetic_mu"][0].copy(), "static_mu": c["static_mu"][0].copy()}


class SingleRodEnv(GymEnv):
    """The N = 1 drop-in classes' common shell: one env of the reference's Gymnasium surface over a one-env batch
    `_vec` (numpy_output=True).  reset / step / get_state / render / close / save_data live here, once; a class adds
    its constructor (the reference's keywords, spaces and attributes) and overrides the hooks it needs:

      _action_row(action)   the caller's action -> the batch's (1, action_dim) float32 row
      _obs(rows)            the batch's (1, obs_dim) NumPy observation -> what the class hands back
      _book_reset()         the host counters of a fresh episode (also sets them up at construction)
      _book_step(...)       the host counters after a step; returns step's `info`

    `shares_rng`: reset hands env.np_random to the batch, so what the env's build draws advances the env's own stream
    (soft_pendulum.py:114,123); False where the build draws nothing.  `obs_dtype`: the observation space's dtype."""

    shares_rng = True
    obs_dtype = np.float32
    mirrored = ("final_time", "time_step", "total_steps", "recording_fps", "step_skip")   # the batch's, kept on the env too

    def __init__(self, render_mode, vec_class, /, *args, **kwargs):
        """`vec_class(1, *args, numpy_output=True, **kwargs)` is the one-env batch."""
        super().__init__()
        if render_mode not in {None, *self.metadata["render_modes"]}:
            raise ValueError(f"Unsupported render mode: {render_mode}")
        self.render_mode = render_mode
        self._vec = vec_class(1, *args, numpy_output=True, **kwargs)
        self._book_reset()
        for k in self.mirrored:
            setattr(self, k, getattr(self._vec, k))

    # -- hooks ---------------------------------------------------------------------
    def _action_row(self, action):
        return np.asarray(action, dtype=np.float32).reshape(1, self._vec.action_dim)

    def _obs(self, rows):
        return np.array(rows[0], dtype=self.obs_dtype)        # always the caller's own copy

    def _book_reset(self) -> None:
        self.time = np.float64(0.0)
        self.counter = 0

    def _book_step(self, action, row, infos, terminated) -> Dict[str, Any]:
        self.time = np.float64(infos["time"][0])
        self.counter += 1
        return {"time": self.time, "TimeLimit.truncated": bool(infos["TimeLimit.truncated"][0])}

    # -- API -----------------------------------------------------------------------
    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None):
        super().reset(seed=seed)
        if self.shares_rng:
            self._vec._rngs[0] = self.np_random
        if seed is not None and getattr(self._vec, "_reset_shapes", 0):
            self._vec.backend.reset_shape_episode[0] = 0      # a re-seeded env begins its sequence of starts again
        obs, _ = self._vec.reset(seed=None)
        self._book_reset()
        return self._obs(obs), {}

    def step(self, action):
        row = self._action_row(action)
        obs, reward, term, trunc, infos = self._vec.step(row)
        terminated = bool(term[0])
        info = self._book_step(action, row, infos, terminated)
        return self._obs(obs), float(reward[0]), terminated, bool(trunc[0]), info

    def get_state(self):
        """Current observation (the reference's get_state).  ArmSingleEnv: like the reference's
        (arm_single_env.py:186-224), a call moves the `prev_kappa_state` / `prev_com_state` the rate entries are
        taken against."""
        obs = self._vec.backend.observe(None)
        return self._obs(obs.cpu().numpy() if hasattr(obs, "cpu") else obs)

    def ground_reaction(self):
        """VecRodEnvBase.ground_reaction of this env, without the env axis: force (rods, 3, n_elem + 1) and torque
        (rods, 3, n_elem) as NumPy arrays; NotImplementedError for an env without plane contact."""
        force, torque = self._vec.ground_reaction()
        return force[0], torque[0]

    def rod_strains(self):
        """VecRodEnvBase.rod_strains of this env, without the env axis, as NumPy arrays: RodStrains(sigma (rods, 3,
        n_elem), kappa (rods, 3, n_elem - 1), dilatation (rods, n_elem), voronoi_dilatation (rods, n_elem - 1),
        internal_force (rods, 3, n_elem), internal_couple (rods, 3, n_elem - 1))."""
        r = self._vec.rod_strains()
        return type(r)(*(t[0] for t in r))

    def muscle_loads(self):
        """VecRodEnvBase.muscle_loads of this env, without the env axis, as NumPy arrays: MuscleLoads(layer_force
        (rods, 4, n_elem), layer_length (rods, 4, n_elem), internal_force (rods, 3, n_elem), internal_couple (rods, 3,
        n_elem - 1), external_force (rods, 3, n_elem + 1), external_couple (rods, 3, n_elem))."""
        r = self._vec.muscle_loads()
        return type(r)(*(t[0] for t in r))

    def joint_loads(self):
        """VecRodEnvBase.joint_loads of this env, without the env axis, as NumPy arrays: JointLoads(body_force (rods, 3),
        body_torque (rods, 3), arm_force (rods, 3), arm_torque (rods, 3), gap (rods, 3), gap_length (rods,), net_force
        (3,), net_torque (3,), acceleration (3,), angular_acceleration (3,))."""
        r = self._vec.joint_loads()
        return type(r)(*(t[0] for t in r))

    def rod_dynamics(self):
        """VecRodEnvBase.rod_dynamics of this env, without the env axis, as NumPy arrays: RodDynamics(internal_force
        (rods, 3, n_elem + 1), internal_torque (rods, 3, n_elem), external_force (rods, 3, n_elem + 1), external_torque
        (rods, 3, n_elem), acceleration (rods, 3, n_elem + 1), angular_acceleration (rods, 3, n_elem))."""
        r = self._vec.rod_dynamics()
        return type(r)(*(t[0] for t in r))

    def rod_clearance(self, self_gap=None):
        """VecRodEnvBase.rod_clearance of this env, without the env axis, as NumPy arrays: RodClearance(gap (rods, rods),
        distance (rods, rods), element (rods, rods, 2), point (rods, rods, 2), target_gap (rods,), target_distance
        (rods,), target_element (rods,), target_point (rods,)); the target fields None for an env without a target."""
        r = self._vec.rod_clearance(self_gap)
        return type(r)(*(None if t is None else t[0] for t in r))

    def set_rod_shape(self, *, kappa=None, sigma=None, velocity=None, omega=None):
        """VecRodEnvBase.set_rod_shape of this env, without the env axis: kappa (rods, 3, n_elem - 1), sigma (rods, 3,
        n_elem), velocity (rods, 3, n_elem + 1), omega (rods, 3, n_elem), float64, the rods axis optional for a one-rod
        env.  After reset(), before the first step.  -> the new observation."""
        fields = {k: None if v is None else v[None] if hasattr(v, "shape") else np.asarray(v, np.float64)[None]
                  for k, v in dict(kappa=kappa, sigma=sigma, velocity=velocity, omega=omega).items()}
        return self._obs(self._vec.set_rod_shape(None, **fields))

    def set_reset_shapes(self, kappa=None, sigma=None, velocity=None, omega=None, *, seed: int = 0) -> None:
        """VecRodEnvBase.set_reset_shapes of this env: a pool of K start shapes, one of which every later reset() starts
        from — kappa (K, rods, 3, n_elem - 1), sigma (K, rods, 3, n_elem), velocity (K, rods, 3, n_elem + 1), omega
        (K, rods, 3, n_elem), float64; the pool axis stays, the rods axis is optional for a one-rod env.  No field: the
        pool is cleared.  `reset_shape_index` is the entry the current episode started from."""
        self._vec.set_reset_shapes(kappa, sigma, velocity, omega, seed=seed)

    @property
    def reset_shape_index(self) -> int:
        """The pool entry this env's current episode started from; -1: no shaped start yet."""
        return int(self._vec.reset_shape_index[0])

    @property
    def reset_shape_episode(self) -> int:
        """The ordinal of this env's next reset in the sequence of shaped starts."""
        return int(self._vec.reset_shape_episode[0])

    # the host counters the _book_reset / _book_step hooks of the classes keep: saved and loaded with a state
    booked = ("time", "counter", "tick", "time_tracker", "_prev_action", "final_time")

    def create_state_bank(self, slots: int) -> None:
        """VecRodEnvBase.create_state_bank of this env: `slots` saved states on the device beside the env, for tree
        search and any other method that returns to a state it has visited.  Once per env."""
        self._vec.create_state_bank(slots)
        self._bank_book = [None] * int(slots)

    def save_state(self, slot: int) -> None:
        """Keep the env's current state in `slot` (VecRodEnvBase.save_states): the resident state, the host counters
        and the state of env.np_random where the env's resets draw from it."""
        self._vec.save_states([0], [slot])
        self._bank_book[slot] = {k: copy.deepcopy(getattr(self, k)) for k in self.booked if hasattr(self, k)}

    def load_state(self, slot: int, copy_rng: bool = True) -> None:
        """Return to the state saved in `slot` (VecRodEnvBase.load_states): the same actions then give the same
        observations, rewards and flags again, bit for bit.  `copy_rng=False`: the env keeps its random stream where
        it is.  The slot keeps its state; load it as often as needed."""
        self._vec.load_states([slot], [0], copy_rng=copy_rng)
        for k, v in self._bank_book[slot].items():
            setattr(self, k, copy.deepcopy(v))

    def save_data(self, filename_video, fps):
        """The reference renders `rod_parameters_dict` to a video here (soft_pendulum.py:253-256, flat_env.py:410-420);
        drawing is out of scope: the data is in `rod_parameters_dict`, nothing is written."""
        if getattr(self._vec, "config_generate_video", False):
            raise NotImplementedError("video generation is outside the hot path; use rod_parameters_dict")

    def render(self):
        """None without a render mode; an (H, W, 3) uint8 frame for "rgb_array" (render.py)."""
        from ..render import render_env

        return render_env(self)

    def close(self):
        from ..render import close_env

        close_env(self)
        self._vec.close()


class SingleEnvSummary:
    """summary() of the two single envs whose reference class has one."""

    def summary(self):
        """As the reference's summary() (octopus/arm_single_env.py:116-133, octopus/flat_env.py:153-170)."""
        print(
            f"""
        {self.final_time=}
        {self.time_step=}
        {self.total_steps=}
        {self.step_skip=}
        simulation time per action: {1.0/self.step_skip=}
        max number of action per episode: {self.total_steps / self.step_skip}

        {self.n_elems=}
        {self.action_space=}
        {self.observation_space=}
        {self.reward_range=}
        """
        )


def _as_numpy(v) -> np.ndarray:
    """A NumPy view or copy of a scalar, a sequence, an array or a CPU / device torch tensor."""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def _per_env(v, n: int, name: str) -> Optional[np.ndarray]:
    """A scalar or an (n,) array -> (n,) float64; None stays None."""
    if v is None:
        return None
    a = _as_numpy(v).astype(np.float64)
    if a.ndim == 0:
        a = np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError(f"{name}: expected a scalar or shape ({n},), got {a.shape}")
    return a


def _per_env3(v, n: int, name: str) -> Optional[np.ndarray]:
    """A scalar, a (3,) or an (n, 3) array -> (n, 3) float64; None stays None."""
    if v is None:
        return None
    a = _as_numpy(v).astype(np.float64)
    if a.ndim == 0:
        a = np.full((n, 3), float(a))
    elif a.shape == (3,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 3):
        raise ValueError(f"{name}: expected a scalar, shape (3,) or ({n}, 3), got {a.shape}")
    return a


def _env_mask(mask, n: int) -> np.ndarray:
    """None (every env) or an (n,) mask -> (n,) bool."""
    if mask is None:
        return np.ones(n, bool)
    sel = _as_numpy(mask).astype(bool).reshape(-1)
    if sel.shape != (n,):
        raise ValueError(f"mask: expected shape ({n},), got {sel.shape}")
    return sel


def time_table(cfg: _capi.SoftrodConfig, n_steps: int) -> np.ndarray:
    """float64 simulated time after k env.steps, accumulated exactly as
    `self.time = self.do_step(self.simulator, self.time, self.time_step)` does
    (soft_pendulum.py:183-184): PositionVerlet adds dt/2 twice per substep.

    `np.add.accumulate` performs the same additions in the same order as the Python loop it
    replaces (t = t + h, one after the other), so the table is bit-identical to it
    (tests/test_host_logic.py) — and 300 times faster: growing the table in the middle of a
    rollout used to stall the launch stream for 10-20 ms on step 64, 128, 256, ..."""
    per = int(cfg.n_substeps) * (2 if cfg.time_two_half_adds else 1)
    inc = np.float64(0.5) * np.float64(cfg.dt) if cfg.time_two_half_adds else np.float64(cfg.dt)
    out = np.empty(n_steps + 1, np.float64)
    out[0] = 0.0
    if n_steps > 0 and per > 0:
        acc = np.add.accumulate(np.full(n_steps * per, inc, np.float64))
        out[1:] = acc[per - 1 :: per]
    elif n_steps > 0:
        out[1:] = 0.0
    return out


class VecRodEnvBase:
    """N parallel envs resident on one GPU.

    reset(seed=None|int|sequence, options=None, mask=None) -> (obs[N,obs_dim] float32, infos)
    step(actions[N,action_dim])  -> (obs, reward[N] float64, terminated[N] bool,
                                     truncated[N] bool, infos)
    Outputs are torch tensors on the device (zero-copy views of the backend's buffers,
    overwritten by the next call) unless `numpy_output=True`.
    """

    metadata: Dict[str, Any] = {"render_modes": ["rgb_array"], "render_fps": 25}
    action_low: float = -1.0
    action_high: float = 1.0

    def __init__(self, num_envs: int, cfg: _capi.SoftrodConfig, *, render_mode, config_generate_video,
                 device: int, numpy_output: bool, autoreset: bool, backend):
        if render_mode not in {None, *self.metadata["render_modes"]}:
            raise ValueError(f"Unsupported render mode: {render_mode}")  # soft_pendulum.py:69-70
        self.config_generate_video = bool(config_generate_video)
        self.render_mode = render_mode
        self.num_envs = int(num_envs)
        self.cfg = cfg
        self.numpy_output = numpy_output
        if autoreset not in (False, True, "host", "device", "same_step"):
            raise ValueError("autoreset must be False, True/'host', 'device' or 'same_step'")
        self.same_step = autoreset == "same_step"        # the device mode with SAME_STEP semantics
        self.device_autoreset = autoreset == "device" or self.same_step
        self.autoreset = bool(autoreset) and not self.device_autoreset
        self._queue_depth = self._ring_depth = 32      # (queue_depth / top_up_every properties)
        self.action_dim = _capi.config_action_dim(cfg)
        self.obs_dim = _capi.config_obs_dim(cfg)
        self.n_action = self.action_dim
        lo, hi = self.action_low, self.action_high
        self.single_action_space = Box(lo, hi, shape=(self.action_dim,), dtype=np.float32)
        self.single_observation_space = Box(-np.inf, np.inf, shape=(self.obs_dim,), dtype=np.float32)
        self.action_space = Box(lo, hi, shape=(self.num_envs, self.action_dim), dtype=np.float32)
        self.observation_space = Box(-np.inf, np.inf, shape=(self.num_envs, self.obs_dim), dtype=np.float32)
        if backend is None:
            from ..backend import HipRodBackend

            backend = HipRodBackend(cfg, device=device)
        self.backend = backend
        self._rngs: List[Optional[np.random.Generator]] = [None] * self.num_envs
        self._steps = np.zeros(self.num_envs, np.int64)  # env.steps since each env's reset
        self._time_tab = time_table(cfg, 128)     # (one SoftPendulum episode; grows by doubling)
        self._needs_reset = np.zeros(self.num_envs, bool)
        self._produced = np.zeros(self.num_envs, np.int64)   # reset records staged per env
        self._staged = [deque() for _ in range(self.num_envs)]   # their draws, oldest first
        self._popped = np.zeros(self.num_envs, np.int64)     # draws removed from _staged so far
        self._since_top_up = 0
        self._status_in_flight = False
        self.top_up_paused = False     # True: the caller reads the queue counters and stages records itself (tests)
        self._reset_shapes = 0         # entries of the pool of start shapes (set_reset_shapes); 0: straight starts
        self._episode_ring = 0         # ring length of the episode statistics (record_episode_statistics); 0: off
        self._norm_obs = self._norm_reward = False    # what set_normalization switched on
        self._norm_training = True     # normalization_training: False freezes the running statistics
        if self.same_step and not hasattr(self.backend, "autoreset_same_step"):
            raise NotImplementedError(f"same-step auto-reset needs the HIP backend, not {type(self.backend).__name__}")
        if self.device_autoreset:
            self.backend.autoreset_enable(self.queue_depth)
        if self.same_step:
            self.backend.autoreset_same_step(True)
        # soft_pendulum.py:117-126: RodCallBack -> rod_parameters_dict, one sample per env.step.
        # Video/plot generation from it stays out of scope; the data tap is here (env 0, or
        # `record_envs` set before reset).
        self.record_envs = (0,)
        self.recorder = None

    def _set_timing(self, final_time, time_step, recording_fps) -> None:
        """The reference's timing attributes (soft_pendulum.py:74-78), for the envs whose constructor takes them."""
        self.final_time = final_time
        self.time_step = time_step
        self.total_steps = int(self.final_time / self.time_step)
        self.recording_fps = recording_fps
        self.step_skip = int(1.0 / (recording_fps * time_step))

    spec = None      # set by gymnasium.make_vec (`env.unwrapped.spec = ...`)

    @property
    def unwrapped(self):
        return self

    @property
    def queue_depth(self) -> int:
        """Unconsumed reset records the host keeps staged per env (device auto-reset).  May be
        lowered at any time; it cannot exceed the device ring allocated when the env was built."""
        return self._queue_depth

    @queue_depth.setter
    def queue_depth(self, depth: int) -> None:
        depth = int(depth)
        if depth < 3:
            raise ValueError("queue_depth must be at least 3")
        if self.device_autoreset and depth > self._ring_depth:
            raise ValueError(f"queue_depth {depth} exceeds the device ring ({self._ring_depth} records per env)")
        self._queue_depth = depth

    @property
    def top_up_every(self) -> int:
        """Deadline of the non-blocking top-up in steps (see _top_up_tick), DERIVED from
        queue_depth so that the two cannot drift apart: an env uses at most one record per two
        steps, so between a reading of the counters and the end of the NEXT top-up (fewer than
        2 * top_up_every steps) it uses at most top_up_every records — fewer than the
        queue_depth - 1 that are certainly staged at the reading.

        autoreset="same_step": the step that ends an episode also restarts it, so an env can use one record
        PER step (episodes of one step).  Between a reading and the end of the next top-up lie fewer than
        2 * top_up_every steps, hence fewer than 2 * top_up_every records: the deadline is halved,
        (queue_depth - 2) // 2, which keeps that number within queue_depth - 2."""
        if self.same_step:
            return max(1, (self._queue_depth - 2) // 2)
        every = max(1, self._queue_depth - 2)
        assert every <= self._queue_depth - 1
        return every

    # -- hooks ---------------------------------------------------------------------
    def _reset_backend(self, mask: np.ndarray, use_mask: bool, draws: Optional[dict] = None) -> None:
        """Reset the masked rods on the backend from what the env's build function draws from
        self._rngs[i] (`self._draw(i, draws)`: a draw taken earlier for env i, if given)."""
        raise NotImplementedError

    def _draw(self, i: int, draws: Optional[dict]):
        return draws[i] if draws is not None and i in draws else self._draw_reset(i)

    def _draw_reset(self, i: int):
        """What one reset of env i draws from self._rngs[i], as the tuple of per-env arguments
        `_reset_backend` / `_queue_from_draws` understand."""
        raise NotImplementedError

    def _queue_from_draws(self, draws, counts) -> None:
        """backend.queue_push*(...) from draws[i] = list of counts[i] draws."""
        raise NotImplementedError

    def _top_up(self, status=None) -> None:
        """Stage resets until every env has `queue_depth` unconsumed records (device mode).

        `status` = (consumed, underflow) from a finished non-blocking read; without it the
        counters are read now, which waits for the stream."""
        consumed = self._sync_staged(status)
        counts = (self.queue_depth - (self._produced - consumed)).astype(np.int32)
        need = np.nonzero(counts > 0)[0]
        if need.size:
            draws = [()] * self.num_envs
            for i in need:
                d = [self._draw_reset(i) for _ in range(int(counts[i]))]
                draws[i] = d
                self._staged[i].extend(d)
            self._queue_from_draws(draws, counts)
            self._produced += counts
        self._since_top_up = 0
        self._status_in_flight = False

    def _top_up_tick(self) -> None:
        """Called once per step in device mode.  Right after a top-up the queue counters start
        their way to the host without stalling the stream (softrod_queue_status_begin); from
        half way to the deadline (`top_up_every` steps since the last top-up) each step looks
        whether they have arrived and tops up if so; at the deadline it waits for that read
        only — the steps enqueued after it keep the GPU busy while the host draws and stages
        (a host that runs ahead of the GPU, as a rollout loop without a policy does, always ends
        up there; one that reads every step's outputs tops up at the half-way mark).

        Why an old reading is enough: the counters only grow, so records computed from it always
        fit; which draw an env's k-th reset uses does not depend on when it was staged; and an
        env uses at most one record per two steps (the step that resets does not also end an
        episode), so between a reading and the end of the NEXT top-up — fewer than
        2 * top_up_every steps — it uses at most top_up_every < queue_depth records."""
        if self.top_up_paused:
            return
        self._since_top_up += 1
        due = self._since_top_up >= self.top_up_every
        if self._status_in_flight:
            if 2 * self._since_top_up >= self.top_up_every:
                st = self.backend.queue_status_poll(due)
                if st is not None:
                    self._top_up(st)
        elif due:
            self._top_up()
        elif hasattr(self.backend, "queue_status_begin"):
            self.backend.queue_status_begin()
            self._status_in_flight = True

    def _sync_staged(self, status=None) -> np.ndarray:
        """Read how many staged records the device has used and forget their draws."""
        from .. import _capi as capi

        consumed, underflow = self.backend.queue_status() if status is None else status
        if underflow:
            raise capi.SoftrodError(
                f"{underflow} auto-resets found no staged record: top up more often or raise queue_depth")
        for i in np.nonzero(consumed > self._popped)[0]:
            for _ in range(int(consumed[i] - self._popped[i])):
                self._staged[i].popleft()
            self._popped[i] = consumed[i]
        return consumed

    def _infos(self, times: np.ndarray) -> Dict[str, Any]:
        return {"time": times, "TimeLimit.truncated": times > self.cfg.final_time}

    def _validate_actions(self, actions) -> None:
        pass

    # -- helpers -------------------------------------------------------------------
    def _times(self) -> np.ndarray:
        kmax = int(self._steps.max()) if self.num_envs else 0
        if kmax >= len(self._time_tab):
            self._time_tab = time_table(self.cfg, max(2 * kmax, 16))
        return self._time_tab[self._steps]

    def _out(self, t):
        return t.cpu().numpy() if self.numpy_output else t

    def _seed_rngs(self, seed, mask: np.ndarray) -> None:
        n = self.num_envs
        if seed is None or isinstance(seed, (int, np.integer)):
            seeds = [None if seed is None else int(seed) + i for i in range(n)]
        else:
            seeds = list(seed)
            if len(seeds) != n:
                raise ValueError("need one seed per env")
        reseeded = np.zeros(n, bool)
        for i in range(n):
            if mask[i] and (seeds[i] is not None or self._rngs[i] is None):
                self._rngs[i], _ = np_random(seeds[i])
                reseeded[i] = True
        return reseeded

    # -- API -----------------------------------------------------------------------
    def reset(
        self,
        *,
        seed: Optional[Union[int, Sequence[Optional[int]]]] = None,
        options: Optional[dict] = None,
        mask: Optional[np.ndarray] = None,
    ):
        n = self.num_envs
        m = np.ones(n, bool) if mask is None else np.asarray(mask, bool).reshape(n)
        reseeded = self._seed_rngs(seed, m)
        draws = None
        if self.device_autoreset and self._produced.any():
            # The next draws of these envs' streams are already staged on the device.  A manual
            # reset takes the env's NEXT draw, i.e. the oldest staged one (and marks it used);
            # a re-seeded env starts a new stream, so everything staged for it is dropped.
            self._sync_staged()
            by = np.zeros(n, np.int32)
            draws = {}
            for i in np.nonzero(m)[0]:
                if reseeded[i]:
                    by[i] = -1
                    self._popped[i] += len(self._staged[i])
                    self._staged[i].clear()
                elif self._staged[i]:
                    by[i] = 1
                    draws[i] = self._staged[i].popleft()
                    self._popped[i] += 1
            self.backend.queue_advance(by)
        self._reset_backend(m, mask is not None, draws)
        if self._episode_ring:      # a manual reset discards a partial episode and opens the latch
            self.backend.episode_stats_reset(m if mask is not None else None)
        if self._reset_shapes:
            self._apply_reset_shapes(m if mask is not None else None, reseeded)
        self._steps[m] = 0
        self._needs_reset[m] = False
        # _prev_action lives with the resident state (softrod_state_view.prev_action): it
        # survives reset except where the reference clears it (soft_pendulum_3d.py:68)
        obs = self.backend.observe(None)
        infos: Dict[str, Any] = {}
        if self._norm_obs or self._norm_reward:     # the reset rows are counted; the masked envs' returns start anew
            self.backend.normalize_reset(obs, m if mask is not None else None)
            if self._norm_obs:
                infos["raw_obs"] = self._out(obs)
                obs = self.backend.normalize["norm_obs"]
        if self.device_autoreset:
            self._top_up()
        if self.config_generate_video and not self.is_octo:
            from ..diagnostics import RodRecorder

            self.recorder = RodRecorder(self.backend, self.record_envs)   # fresh dict per reset (:118)
        elif self.is_octo and (self.config_generate_video or getattr(self, "config_save_head_data", False)):
            from ..diagnostics import OctoRecorder

            # flat_env.py:188-206: per-arm RodCallBack dicts and the head's dict, fresh per reset
            self.recorder = OctoRecorder(self.backend, self.record_envs[0], rods=self.config_generate_video,
                                         head=self.config_save_head_data)
        return self._out(obs), infos

    @property
    def is_octo(self) -> bool:
        return int(self.cfg.env_kind) == _capi.ENV_OCTO_FLAT

    @property
    def rod_parameters_dict(self):
        """The reference's `rod_parameters_dict` for the first recorded env."""
        return None if self.recorder is None or self.is_octo else self.recorder.params[0]

    @property
    def rod_parameters_dict_list(self):
        """FlatEnv.rod_parameters_dict_list (octopus/flat_env.py:190-198): one dict per arm."""
        return getattr(self.recorder, "rod_parameters_dict_list", None)

    @property
    def head_dict(self):
        """FlatEnv.head_dict (octopus/flat_env.py:199-206)."""
        return getattr(self.recorder, "head_dict", None)

    def _step_device_autoreset(self, a):
        import torch

        obs, reward, term, trunc = self.backend.step(a)    # auto-reset pass + step kernel
        self._top_up_tick()
        if getattr(self, "_dev_time", None) is None:
            # the clock row, kept and only read: on the HIP backend through the view that leaves planar certificates on
            views = getattr(self.backend, "_views", None)
            if views is None:
                self._dev_time = self.backend.state()["time"]
            else:
                with views() as st:
                    self._dev_time = st["time"]
        # TimeLimit.truncated is the time limit alone; with ArmPush's early termination `truncated` carries the
        # cut-off as well, and the epilogue writes the time-limit flag on its own (backend.time_limit)
        tl = self.backend.time_limit() if getattr(self.cfg, "early_termination", 0) else trunc.view(torch.bool)
        infos = {"time": self._out(self._dev_time), "TimeLimit.truncated": self._out(tl)}
        if self.same_step:
            infos.update(self._final_infos(term, trunc))
        if self._episode_ring:
            infos.update(self._episode_infos())
        if self._norm_obs or self._norm_reward:
            obs, reward = self._normalized(obs, reward, infos)
        return (self._out(obs), self._out(reward), self._out(term.view(torch.bool)),
                self._out(trunc.view(torch.bool)), infos)

    aux_info_key: Optional[str] = None     # what the backend's aux column is called in `infos` (SoftPendulum3D: "tilt")

    def _final_infos(self, term, trunc) -> Dict[str, Any]:
        """autoreset="same_step": Gymnasium's SAME_STEP keys.  `final_obs` (N, obs_dim) and `final_info` hold the
        finished step's observation, clock and aux value in the rows where `_final_obs` = terminated | truncated is
        set; the other rows are unspecified (an earlier episode end of that env).  `obs`, infos["time"] (0 for a
        restarted env) and the aux key describe the new episode.  The flags, the reward and
        infos["TimeLimit.truncated"] are the finished step's: the reset leaves the time-limit row of env_aux alone."""
        import torch

        be = self.backend
        final_info = {"time": self._out(be.final_time)}
        out = {"final_obs": self._out(be.final_obs), "_final_obs": self._out((term | trunc).view(torch.bool)),
               "final_info": final_info}
        if self.aux_info_key is not None:
            out[self.aux_info_key] = self._out(be.aux[:, 0])
            final_info[self.aux_info_key] = self._out(be.final_aux)
        return out

    def step(self, actions):
        import torch

        self._validate_actions(actions)
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.backend.device)
        a = a.reshape(self.num_envs, self.action_dim)
        if self.device_autoreset:
            return self._step_device_autoreset(a)
        pending = self._needs_reset.copy() if self.autoreset else None
        saved_prev = None
        if pending is not None and pending.any():
            # the action of a restarting env is ignored (NEXT_STEP): its _prev_action must stay
            # the one of its last real step, as env.reset() would find it
            saved_prev = self.backend.prev_action_rows()[torch.from_numpy(pending)].clone()
        obs, reward, term, trunc = self.backend.step(a)   # also records _prev_action[:] = action
        self._steps += 1
        if pending is not None and pending.any():
            # NEXT_STEP auto-reset: these envs finished on the previous call; their step above
            # is discarded, they restart and report their reset observation
            keep = obs.clone()
            self.backend.prev_action_rows()[torch.from_numpy(pending)] = saved_prev
            self._seed_rngs(None, pending)
            self._reset_backend(pending, True)
            if self._reset_shapes:
                self._apply_reset_shapes(pending)
            self._steps[pending] = 0
            robs = self.backend.observe(None)
            pm = torch.from_numpy(pending).to(robs.device)
            obs = torch.where(pm[:, None], robs, keep)
            reward = torch.where(pm, torch.zeros_like(reward), reward)
            term = torch.where(pm, torch.zeros_like(term), term)
            trunc = torch.where(pm, torch.zeros_like(trunc), trunc)
        if self.autoreset:
            self._needs_reset = (term | trunc).cpu().numpy().astype(bool)
        if self.recorder is not None:
            self.recorder.record()
        times = self._times()
        infos = self._infos(times)
        if self._episode_ring:
            infos.update(self._episode_infos())
        if self._norm_obs or self._norm_reward:
            if self.autoreset:      # host-driven NEXT_STEP: the pass sees the composed rows, not the discarded step's
                self.backend.normalize_step(obs.contiguous(), reward, term, trunc, None, _capi.NORMALIZE_NEXT_STEP)
            obs, reward = self._normalized(obs, reward, infos)
        return (
            self._out(obs),
            self._out(reward),
            self._out(term.view(torch.bool)),     # uint8 0/1 -> bool, zero-copy
            self._out(trunc.view(torch.bool)),
            infos,
        )

    def rod_energies(self):
        """(N, rods_per_env, 4) float64: translational, rotational, bending and shear energy of every rod
        (PyElastica's compute_*_energy, our recollection of pyelastica 1.0.0: include/softrod.h
        softrod_rod_energies).  THE INSTANT is the reference's: the strains (sigma, kappa, dilatation) of the
        mid-substep configuration of the last substep, where its force evaluation cached them, with the
        end-of-step velocities; right after a reset, the reset state.  OctoFlat / the muscle octopus: one row
        per arm (rigid bodies have none).  A device tensor overwritten by the next call (NumPy with
        numpy_output=True)."""
        return self._out(self.backend.rod_energies())

    def ground_reaction(self):
        """(force, torque): what the ground does to the body.  force (N, rods_per_env, 3, n_elem + 1) is the
        lab-frame force RodPlaneContactWithAnisotropicFriction adds to every node — plane response with its elastic
        and damping terms plus kinetic and static friction, axial and rolling —, torque (N, rods_per_env, 3, n_elem)
        the material-frame torque it adds to every element.  The reference evaluates both in every substep and
        returns neither.  THE INSTANT: one fresh force evaluation at the state as it stands (no half kinematic
        step), with the external loads gathered in the substep's order; not the value the last substep applied,
        which depends on that substep's pre-update rates (include/softrod.h softrod_ground_reaction).  Per-env
        contact, per-env material and a radius profile are honoured.  OctoArmSingle (up to 63 elements), OctoFlat
        and OctoFlatLite on the HIP backend; elsewhere NotImplementedError.  Device tensors, views of one buffer
        overwritten by the next call (NumPy copies with numpy_output=True).  Inside a capture_policy_step graph
        only if the policy itself calls it: the captured step does not."""
        be = self.backend
        if not hasattr(be, "ground_reaction"):
            raise NotImplementedError(f"ground reaction needs the HIP backend, not {type(be).__name__}")
        why = _capi.ground_reaction_refusal(self.cfg)
        if why is not None:
            raise NotImplementedError(why)
        force, torque = be.ground_reaction()
        return self._out(force), self._out(torque)

    def rod_strains(self):
        """RodStrains(sigma, kappa, dilatation, voronoi_dilatation, internal_force, internal_couple) of every rod:
        the strain fields the reference's RodCallBack records once per env.step (callback_func.py:23-41) and the
        passive elastic loads they stand for — what curvature and strain gauges along the arm would sense — without
        leaving the device.  sigma (N, rods_per_env, 3, n_elem) and kappa (N, rods_per_env, 3, n_elem - 1; not
        reduced by the rest curvature) in the material frame, dilatation (N, rods_per_env, n_elem),
        voronoi_dilatation (N, rods_per_env, n_elem - 1), internal_force S sigma (.., 3, n_elem), internal_couple
        B (kappa - rest_kappa) (.., 3, n_elem - 1); on the COOMM muscle envs the loads exclude the muscle layers'
        force and couple.  THE INSTANT is rod_energies()': the caches of the last force evaluation, or the reset
        state for an env just reset, per env (include/softrod.h softrod_rod_strains).  Every env kind, rods of up
        to 126 elements, tapered rods and per-env material on the HIP backend; elsewhere NotImplementedError.
        Device tensors, views of one buffer overwritten by the next call (NumPy copies with numpy_output=True)."""
        be = self.backend
        if not hasattr(be, "rod_strains"):
            raise NotImplementedError(f"rod strains need the HIP backend, not {type(be).__name__}")
        r = be.rod_strains()
        return type(r)(*(self._out(t) for t in r))

    def muscle_loads(self):
        """MuscleLoads(layer_force, layer_length, internal_force, internal_couple, external_force, external_couple)
        of every rod of a COOMM muscle env: what the reference's ApplyMuscles computes in every substep and returns
        none of — muscle tension and length for proprioception, actuation effort for a reward — without leaving the
        device.  layer_force (N, rods_per_env, 4, n_elem) = activation * strength * max(fl(length), 0) and
        layer_length (N, rods_per_env, 4, n_elem) per layer (zero rows for layers the env does not have; the length
        is defined whatever the activation is), the muscle internal_force (.., 3, n_elem) and internal_couple
        (.., 3, n_elem - 1) in the material frame, the equivalent external_force (.., 3, n_elem + 1) on the nodes
        (lab frame) and external_couple (.., 3, n_elem) on the elements.  THE INSTANT is rod_strains()'; the
        activations are the resident rows as the last action left them, read per element (include/softrod.h
        softrod_muscle_loads, which also names the one stepper that applies them differently).  The law is labelled
        parity-unpinned, like the muscle envs themselves.  HIP backend only: elsewhere NotImplementedError; an env
        without COOMM muscles raises ValueError.  Device tensors, views of one buffer overwritten by the next call
        (NumPy copies with numpy_output=True)."""
        be = self.backend
        if not hasattr(be, "muscle_loads"):
            raise NotImplementedError(f"muscle loads need the HIP backend, not {type(be).__name__}")
        why = _capi.muscle_loads_refusal(self.cfg)
        if why is not None:
            raise ValueError(why)
        r = be.muscle_loads()
        return type(r)(*(self._out(t) for t in r))

    def joint_loads(self):
        """JointLoads(body_force, body_torque, arm_force, arm_torque, gap, gap_length, net_force, net_torque,
        acceleration, angular_acceleration) of an env whose arms are joined to a rigid body (OctoFlat, OctoFlatLite,
        OctoArmPullWeight, OctoCrawl, OctoArmTwo, OctoReach): what the reference's FixedJoint2Rigid computes in every
        substep and returns none of — the pull on the weight, the propulsive force and turning moment the arms give the
        head, what an IMU on the head would read — without leaving the device.  Per arm (N, rods_per_env, 3): body_force
        = contact_force, added to the body (lab frame); body_torque, added to the body (body frame); arm_force =
        -body_force, added to the arm's node 0; arm_torque, added to the arm's element 0 (its material frame); gap, node
        0 minus its connection point, and gap_length (N, rods_per_env).  For the body (N, 3): net_force and net_torque,
        summed over the arms in arm order; acceleration = net_force / head mass with a_z = 0; angular_acceleration =
        (0, 0, net_torque_z / J_3), body frame; both zero for the held head of OctoReach.  THE INSTANT is
        ground_reaction()'s: one evaluation at the resident state, not the value the last substep applied
        (include/softrod.h softrod_joint_loads).  HIP backend only: elsewhere NotImplementedError; an env without a
        rigid body raises ValueError.  Device tensors, views of one buffer overwritten by the next call (NumPy copies
        with numpy_output=True)."""
        be = self.backend
        if not hasattr(be, "joint_loads"):
            raise NotImplementedError(f"joint loads need the HIP backend, not {type(be).__name__}")
        why = _capi.joint_loads_refusal(self.cfg)
        if why is not None:
            raise ValueError(why)
        r = be.joint_loads()
        return type(r)(*(self._out(t) for t in r))

    def rod_dynamics(self):
        """RodDynamics(internal_force, internal_torque, external_force, external_torque, acceleration,
        angular_acceleration) of every rod: the two sides of its equation of motion, what PyElastica keeps on every
        rod (internal_forces / internal_torques, external_forces / external_torques, and acceleration_collection /
        alpha_collection after update_accelerations) and the reference returns none of — what an accelerometer or a
        gyro-rate sensor on the arm would read, and what a reward that penalises jerk or effort needs — without leaving
        the device.  internal_force, external_force and acceleration (N, rods_per_env, 3, n_elem + 1) on the nodes,
        lab frame; internal_torque, external_torque and angular_acceleration (N, rods_per_env, 3, n_elem) on the
        elements, material frame.  external_* hold everything synchronize adds, gathered in the substep's own order:
        FixedJoint2Rigid on node 0 / element 0, then gravity, the point force, the tip force and the COOMM layers'
        equivalent loads, and the plane contact before or after them as contact_before_forcing says.  acceleration =
        (internal_force + external_force) / mass, angular_acceleration = J^-1 (internal_torque + external_torque) e;
        constraints, dampers and suckers act on values and rates and do not enter.  THE INSTANT is
        ground_reaction()'s: one fresh evaluation at the state as it stands, not the value the last substep applied
        (include/softrod.h softrod_rod_dynamics); the point force is the resident previous action (none for an env
        just reset), the muscle activations the resident rows as the last action left them.  Per-env material,
        per-env contact and a radius profile are honoured.  Every env but SoftArmTracking, rods of up to 63 elements,
        on the HIP backend; elsewhere NotImplementedError.  Device tensors, views of one buffer overwritten by the
        next call (NumPy copies with numpy_output=True)."""
        be = self.backend
        if not hasattr(be, "rod_dynamics"):
            raise NotImplementedError(f"rod dynamics need the HIP backend, not {type(be).__name__}")
        why = _capi.rod_dynamics_refusal(self.cfg)
        if why is not None:
            raise NotImplementedError(why)
        r = be.rod_dynamics()
        return type(r)(*(self._out(t) for t in r))

    def rod_clearance(self, self_gap=None):
        """RodClearance(gap, distance, element, point, target_gap, target_distance, target_element, target_point):
        where the rods of every env are relative to each other, to themselves and to the env's target — upstream has
        no rod-rod contact in any env (arms pass through each other, a long arm through itself), and this is what a
        collision penalty, a planner on fork() that rejects interpenetrating gaits, or a grasping reward needs —
        without leaving the device.  Element k of a rod is the capsule around the segment node k -> node k + 1 with
        the element's REST radius (a radius profile is honoured, the dilatation ignored); the rigid head / weight is
        deliberately not a body: the arms are joined to it.  gap (N, rods_per_env, rods_per_env) is the least
        (centre-line distance - r_i - r_j) over the element pairs of row rod a and column rod b, negative when the
        capsules interpenetrate; distance that pair's centre-line distance; element (.., 2) its (i, j) as exact
        float64; point (.., 2) the closest points' parameters (s, t) in [0, 1] along the two elements; [b][a] is
        [a][b] with i <-> j, s <-> t.  The diagonal is the rod against itself, over the pairs with j - i >= self_gap
        (None: the first separation at which two elements of the straight rest rod no longer overlap,
        _capi.rod_clearance_self_gap; 2 .. 126); +inf, +inf, -1, -1, 0, 0 where no such pair exists.  target_distance
        (N, rods_per_env) is the distance from the env's target (the one render_frames() draws) to the nearest point
        of the rod's centre line, target_gap = target_distance - r_i, target_element i, target_point s; the four are
        None for an env without a target.  Among equal gaps the lowest i, then the lowest j wins.  A rod with a
        non-finite node has NaN, NaN, -1, -1, NaN, NaN in its rows and columns and disturbs no other (include/softrod.h
        softrod_rod_clearance).  THE INSTANT is the state as it stands.  Every env kind, rods of up to 126 elements, on
        the HIP backend; elsewhere NotImplementedError.  Device tensors, views of one buffer overwritten by the next
        call (NumPy copies with numpy_output=True).  Inside a capture_policy_step graph when the policy calls it."""
        be = self.backend
        if not hasattr(be, "rod_clearance"):
            raise NotImplementedError(f"rod clearance needs the HIP backend, not {type(be).__name__}")
        r = be.rod_clearance(self_gap)
        return type(r)(*(None if t is None else self._out(t) for t in r))

    # -- initial shapes (exploring starts, curricula, restarts from a recorded pose) ------------
    def set_rod_shape(self, mask=None, *, kappa=None, sigma=None, velocity=None, omega=None):
        """Start envs from any strain field instead of upstream's straight rod (its builds call straight_rod only):
        randomised initial shapes — curled, twisted, pre-stretched arms —, exploring starts, curricula that begin near
        a goal pose, restarts from a pose recorded with rod_strains().  Called after reset(), before the first step
        of the envs it writes; `mask`: None (every env) or (N,) booleans.

        Every rod of a masked env keeps its base pose as reset left it (node 0's position, element 0's directors: the
        boundary-condition targets, head joints and pendulum / moving-base constraints stay consistent) and is rebuilt
        on the device from the fields, in rod_strains()' own conventions and shapes, float64:
          kappa     (N, rods_per_env, 3, n_elem - 1)  material frame, not reduced by rest curvature:
                    Q_{k+1} = exp(-[kappa_k D^]x) Q_k with D^ the rest Voronoi length
          sigma     (N, rods_per_env, 3, n_elem)      x_{k+1} - x_k = l^ Q_k^T (sigma_k + e3), l^ the rest length
          velocity  (N, rods_per_env, 3, n_elem + 1)  lab frame, written as given
          omega     (N, rods_per_env, 3, n_elem)      material frame, written as given
        A field left None is zero: set_rod_shape() alone rebuilds the straight, unstretched rod at rest along the base
        director.  For a one-rod env the rods axis may be left out.  A float64 torch tensor on the env's device is
        used in place; NumPy arrays and sequences are coerced once.  rod_strains() afterwards returns sigma as given
        and kappa scaled by 1 + acos_shift / 3 (the read-out's own guard: 3.3e-11 relative).

        What reset derives from the shape is derived again: the tangent and kappa rows, OctoArmSingle's
        prev_kappa_state and prev_com_state.  OctoArmTwo's _prev_kappa moves in the observation, as upstream's
        get_state moves it: the one observe this call makes is the right number.  Not touched: rest_kappa, muscle
        activations, suckers, the rigid head, prev_action, the clock, per-env material and contact, the RNG streams,
        `_steps` and pending resets; unmasked envs stay bitwise as they were.  Values are not validated: a NaN spoils
        its own rod only.  SoftPendulum-v0 takes any shape, but only a planar one keeps the fast planar path:
        kappa[:, :, 0] = kappa[:, :, 2] = 0 and sigma[:, :, 1] = 0, kappa[:, :, 1] (about d2) being the in-plane bend;
        otherwise the 3-D loop steps the rod.

        -> the new observations in reset()'s form (one backend.observe(None)).  Refusals, each before anything is
        written: ValueError for a masked env that has stepped since its reset (a teleported state has no mid-substep
        configuration for the read-outs' instant), for a field that is not float64 or has the wrong shape;
        NotImplementedError with autoreset="device" / "same_step" (staged reset records are straight rods, as for
        fork()) and on a backend other than the HIP one.  Not offered on the sharded env."""
        if self.device_autoreset:
            raise NotImplementedError(f"set_rod_shape() with autoreset='{'same_step' if self.same_step else 'device'}': "
                                      "staged reset records are straight rods")
        be = self.backend
        if not hasattr(be, "set_rod_shape"):
            raise NotImplementedError(f"set_rod_shape needs the HIP backend, not {type(be).__name__}")
        sel = _env_mask(mask, self.num_envs)
        if (self._steps[sel] != 0).any():
            raise ValueError(f"set_rod_shape: envs {np.nonzero(sel & (self._steps != 0))[0].tolist()} have stepped since "
                             "their reset; it is a reset-time call")
        fields = dict(kappa=kappa, sigma=sigma, velocity=velocity, omega=omega)
        for name, v in fields.items():
            _capi.rod_shape_check_field(self.cfg, self.num_envs, name, v)
        return self._out(be.set_rod_shape(None if mask is None else sel, **fields))

    def set_reset_shapes(self, kappa=None, sigma=None, velocity=None, omega=None, *, seed: int = 0) -> None:
        """Shaped episode starts under EVERY reset: a resident pool of K start shapes, one of which each reset of an env
        starts from — reset() and reset(mask=...), the host-driven autoreset=True, autoreset="device" and "same_step"
        alike.  Where set_rod_shape() shapes the envs once and is gone at the first episode end, this is what exploring
        starts, shape randomisation and near-goal curricula need while training in the device modes.  Upstream has no
        counterpart (its builds call straight_rod only).

        The fields follow set_rod_shape()'s conventions and dtypes with a leading pool axis K >= 1 instead of the env
        axis: kappa (K, rods_per_env, 3, n_elem - 1), sigma (K, rods, 3, n_elem), velocity (K, rods, 3, n_elem + 1),
        omega (K, rods, 3, n_elem), float64; the rods axis may be left out for a one-rod env; a field left out is zero;
        every given field has the same K.  The library copies the pool into device buffers of its own in this call, so
        the arguments may be released.  A call with no field clears the pool: starts are straight again and the steps
        launch nothing extra.  For a weighted draw repeat entries.  SoftPendulum-v0 takes any pool, but only planar
        entries keep the fast planar path (set_rod_shape()'s rule: kappa rows 0 and 2, sigma row 1, velocity row 2 and
        omega rows 0 and 2 zero); an out-of-plane start is stepped by the 3-D loop until the env's next planar start.

        While a pool is set every reset of an env leaves it exactly as reset followed by set_rod_shape(pool[idx])
        leaves it, bit for bit, and the observation the resetting call returns for the env is the shaped start's; with
        autoreset="same_step" final_obs / final_info stay the finished step's.  Which entry does not depend on the
        mode: idx = gym_softrobot_amd.reset_shape_index(seed, e, j, K) with e the env's index in the batch and j the
        number of resets env e has had since its RNG stream was last seeded — reset(seed=...) zeroes j for the envs it
        re-seeds, so a seed reproduces the sequence of starts together with the base poses.  `reset_shape_index` holds
        each env's current entry (to credit returns to start shapes), `reset_shape_episode` the next j.

        The call shapes nothing itself: envs in mid-episode stay bitwise as they are and the pool takes effect at each
        env's next reset; it sets reset_shape_index to -1 and reset_shape_episode to 0 for every env.  In the device
        modes an env that finds no staged reset record did not restart and is neither shaped nor counted.  A graph
        captured with capture_policy_step must be captured again after set_reset_shapes.  fork() copies
        reset_shape_index, and reset_shape_episode with copy_rng=True; state_dict() carries both rows but not the pool.
        set_rod_shape() itself is unchanged, its refusals included.

        ValueError for a field that is not float64, has the wrong shape or another K than the fields before it;
        NotImplementedError on a backend other than the HIP one.  Not offered on the sharded env."""
        be = self.backend
        if not hasattr(be, "set_reset_shapes"):
            raise NotImplementedError(f"set_reset_shapes needs the HIP backend, not {type(be).__name__}")
        fields = dict(kappa=kappa, sigma=sigma, velocity=velocity, omega=omega)
        _capi.reset_shapes_pool(self.cfg, fields)
        self._reset_shapes = int(be.set_reset_shapes(**fields, seed=int(seed)))

    def _apply_reset_shapes(self, mask: Optional[np.ndarray], reseeded: Optional[np.ndarray] = None) -> None:
        """Between _reset_backend and the observe of a host-driven reset: the masked envs (None: all) start from their
        pool entries; the envs the reset re-seeded begin their sequence of starts again."""
        be = self.backend
        if reseeded is not None and reseeded.any():
            be.reset_shape_episode[np.nonzero(reseeded)[0].tolist()] = 0
        if int(self.cfg.env_kind) == _capi.ENV_ARM_TWO:
            be.observe(None)     # ArmTwoEnv's get_state moves _prev_kappa: the reset's own observation comes first,
                                 # as in reset() followed by set_rod_shape() and in the device passes
        be.apply_reset_shapes(mask)

    @property
    def reset_shape_index(self):
        """(N,) int32, zero-copy device row (NumPy copy with numpy_output=True): the pool entry each env's current
        episode started from; -1 for no shaped start yet.  Needs a pool (set_reset_shapes)."""
        return self._out(self.backend.reset_shape_index)

    @property
    def reset_shape_episode(self):
        """(N,) int32, zero-copy device row (NumPy copy with numpy_output=True): the ordinal j of each env's next reset
        in its sequence of shaped starts.  Needs a pool (set_reset_shapes)."""
        return self._out(self.backend.reset_shape_episode)

    # -- per-env material (domain randomisation) ----------------------------------------
    _MATERIAL_KEYS = ("youngs_modulus", "shear_modulus", "density", "damping_constant")

    def set_material(self, mask=None, *, youngs_modulus=None, shear_modulus=None, density=None,
                     damping_constant=None):
        """Give each env its own rod material: Young's modulus E, shear modulus G, density rho and the
        AnalyticalLinearDamper's damping constant nu.  Upstream builds every env's rod with one
        CosseratRod.straight_rod(density, youngs_modulus, shear_modulus) and has no counterpart; here a batch
        can randomise them per env without leaving the GPU.

        Each value is a scalar or an (N,) array (NumPy, or a CPU / device torch tensor); None keeps the current
        value.  `youngs_modulus` without `shear_modulus` sets G = E / 3 (PyElastica's default at Poisson ratio
        0.5, which the env builds use).  `mask` (N,) bool, or None for every env: only those envs change.  Values
        must be finite, with E, G, rho > 0 and nu >= 0.

        Material belongs to the env slot, not to the episode: it persists through host and device auto-resets.
        To resample per episode, call set_material(mask=finished, ...) between two steps; under NEXT_STEP
        auto-reset the restarted episode then runs with the new values from its first step.  Takes effect at
        the next launch on the env's stream.  SoftPendulum, SoftPendulum3D and OctoArmSingle (uniform rods of up
        to 63 elements) on the HIP backend only; elsewhere NotImplementedError."""
        be = self.backend
        if not hasattr(be, "set_env_material"):
            raise NotImplementedError(f"per-env material needs the HIP backend, not {type(be).__name__}")
        why = _capi.env_material_refusal(self.cfg, tapered="radius_profile" in getattr(be, "_tables", {}))
        if why is not None:
            raise NotImplementedError(why)
        n = self.num_envs
        cols = [_per_env(v, n, k) for v, k in zip((youngs_modulus, shear_modulus, density, damping_constant),
                                                  self._MATERIAL_KEYS)]
        if cols[0] is not None and cols[1] is None:
            cols[1] = cols[0] / 3.0
        sel = _env_mask(mask, n)
        m = be.env_material()
        for j, c in enumerate(cols):
            if c is not None:
                m[sel, j] = c[sel]
        rows = m[sel]
        if not np.isfinite(rows).all():
            raise ValueError("set_material: values must be finite")
        if not ((rows[:, :3] > 0.0).all() and (rows[:, 3] >= 0.0).all()):
            raise ValueError("set_material: E, G and density must be > 0, damping_constant >= 0")
        be.set_env_material(m, sel.astype(np.uint8))

    def material(self) -> Dict[str, np.ndarray]:
        """Every env's rod material: youngs_modulus, shear_modulus, density, damping_constant as (N,) float64
        arrays (the config's values until set_material)."""
        be = self.backend
        m = be.env_material() if hasattr(be, "env_material") else np.tile(_capi.env_material_defaults(self.cfg),
                                                                          (self.num_envs, 1))
        return {k: m[:, j].copy() for j, k in enumerate(self._MATERIAL_KEYS)}

    # -- per-env ground contact and friction (domain randomisation) ---------------------
    def set_contact(self, mask=None, *, contact_k=None, contact_nu=None, kinetic_mu=None, static_mu=None,
                    friction_multiplier=None, friction_symmetry=None):
        """Give each env its own ground: the contact stiffness k and damping nu and the kinetic / static friction
        coefficients (forward, backward, sideways) of RodPlaneContactWithAnisotropicFriction
        (octopus/build.py:236-283).  Upstream builds every env with one set; here a batch can randomise them per
        env without leaving the GPU.

        `contact_k`, `contact_nu`: a scalar or an (N,) array.  `kinetic_mu`, `static_mu`: a scalar, a (3,) or an
        (N, 3) array.  NumPy or a CPU / device torch tensor; None keeps the current value.  `kinetic_mu` without
        `static_mu` sets static = 2 * kinetic (upstream's static_mu_array = 2 * kinetic_mu_array).
        `friction_multiplier` (scalar or (N,)) and `friction_symmetry` (bool or (N,) bool) are upstream's
        override_params knobs (build.py:30-44,178-190): both mu arrays are recomputed as build_arm / build_octopus
        do, mu = L0 / (period^2 |g| froude), [mu, mu, mu] or [mu, 1.5 mu, 2 mu] times the multiplier, static twice
        kinetic (a multiplier of 1 without symmetry gives the config's arrays bit for bit); given either, the
        other defaults to 1 / False, and explicit `kinetic_mu` / `static_mu` are a ValueError.  `mask` (N,) bool,
        or None for every env: only those envs change.  Values must be finite and >= 0.

        Contact belongs to the env slot, not to the episode: it persists through host and device auto-resets and
        is carried by state_dict().  Takes effect at the next launch on the env's stream.  OctoArmSingle (uniform
        rods of up to 63 elements, both math modes), OctoFlat and OctoFlatLite on the HIP backend only;
        elsewhere NotImplementedError."""
        be = self.backend
        if not hasattr(be, "set_env_contact"):
            raise NotImplementedError(f"per-env contact needs the HIP backend, not {type(be).__name__}")
        why = _capi.env_contact_refusal(self.cfg, tapered="radius_profile" in getattr(be, "_tables", {}))
        if why is not None:
            raise NotImplementedError(why)
        n = self.num_envs
        k, nu = _per_env(contact_k, n, "contact_k"), _per_env(contact_nu, n, "contact_nu")
        kin, stat = _per_env3(kinetic_mu, n, "kinetic_mu"), _per_env3(static_mu, n, "static_mu")
        if friction_multiplier is not None or friction_symmetry is not None:
            if kin is not None or stat is not None:
                raise ValueError("friction_multiplier / friction_symmetry recompute both mu arrays: "
                                 "not together with kinetic_mu / static_mu")
            mult = _per_env(1.0 if friction_multiplier is None else friction_multiplier, n, "friction_multiplier")
            sym = _as_numpy(False if friction_symmetry is None else friction_symmetry)
            if sym.dtype.kind not in "bui":
                raise ValueError(f"friction_symmetry: expected a bool or ({n},) bools, got dtype {sym.dtype}")
            sym = np.broadcast_to(sym.astype(bool), (n,)) if sym.ndim == 0 else sym.astype(bool)
            if sym.shape != (n,):
                raise ValueError(f"friction_symmetry: expected a bool or shape ({n},), got {sym.shape}")
            kin, stat = np.empty((n, 3)), np.empty((n, 3))
            for i in range(n):
                kin[i], stat[i] = _capi.friction_mu_arrays(self.cfg, float(mult[i]), bool(sym[i]))
        elif kin is not None and stat is None:
            stat = 2 * kin
        sel = _env_mask(mask, n)
        c = be.env_contact()
        for sl, v in ((slice(0, 1), k), (slice(1, 2), nu), (slice(2, 5), kin), (slice(5, 8), stat)):
            if v is not None:
                c[sel, sl] = v[sel].reshape(-1, sl.stop - sl.start)
        rows = c[sel]
        if not np.isfinite(rows).all():
            raise ValueError("set_contact: values must be finite")
        if not (rows >= 0.0).all():
            raise ValueError("set_contact: contact_k, contact_nu and every mu must be >= 0")
        be.set_env_contact(c, sel.astype(np.uint8))

    def contact(self) -> Dict[str, np.ndarray]:
        """Every env's ground: contact_k, contact_nu as (N,) and kinetic_mu, static_mu as (N, 3) float64 arrays
        (forward, backward, sideways; the config's values until set_contact)."""
        be = self.backend
        c = be.env_contact() if hasattr(be, "env_contact") else np.tile(_capi.env_contact_defaults(self.cfg),
                                                                        (self.num_envs, 1))
        return {"contact_k": c[:, 0].copy(), "contact_nu": c[:, 1].copy(), "kinetic_mu": c[:, 2:5].copy(),
                "static_mu": c[:, 5:8].copy()}

    def default_camera(self) -> "_capi.SoftrodCamera":
        """The camera render_frames() uses when given none: _capi.camera_default(cfg), an orthographic 84 x 84 view that
        frames a freshly reset env (softrod_camera_default, include/softrod.h).  A fresh object: edit its fields (centre,
        axes, half_width, size, follow, target_radius, light, ambient) and pass it back."""
        return _capi.camera_default(self.cfg)

    def render_frames(self, width=None, height=None, camera=None, depth=False):
        """RGB frames of EVERY env without leaving the device: an (N, H, W, 3) uint8 tensor, or (rgb, depth) with depth
        (N, H, W) float32 (camera-frame depth of the surface, -inf where nothing is drawn) when `depth` is true — pixel
        observations, RGB-D policies and per-env video logging of a resident batch.  The single-env `render()` (one
        matplotlib frame from a host snapshot) is what it was; the reference has no batched counterpart.

        `camera`: a _capi.SoftrodCamera shared by all envs (default: default_camera()); `width` / `height` override
        its size.  Rods are drawn as shaded capsules of their rest radius, one colour per arm, the rigid body and the
        env's target as spheres; an env whose state is not finite renders as background.  The image model is
        include/softrod.h's softrod_render.  One HIP kernel (csrc/softrod_render.hpp) on the current stream; the
        tensors are allocated on first use per (H, W) and overwritten by the next call; usable inside
        capture_policy_step once a first call has allocated them.  Device tensors (NumPy copies with
        numpy_output=True).  HIP backend only."""
        be = self.backend
        if not hasattr(be, "render"):
            raise NotImplementedError(f"render_frames needs the HIP backend, not {type(be).__name__}")
        cam = self.default_camera() if camera is None else camera
        if width is not None or height is not None:
            cam = cam.copy()
            if width is not None:
                cam.width = int(width)
            if height is not None:
                cam.height = int(height)
        out = be.render(cam, depth=bool(depth))
        return (self._out(out[0]), self._out(out[1])) if depth else self._out(out)

    # -- episode statistics: returns and lengths of finished episodes, kept on the device ---------
    def record_episode_statistics(self, buffer_length: int = 100) -> None:
        """Keep the return, length and end time of every episode that ends, on the device: what Gymnasium's
        RecordEpisodeStatistics does for a host env, for a resident batch under every reset mode — by hand,
        autoreset=True, "device" and "same_step" — where the host never sees which env finished on which call.
        Upstream has a single env and no statistics.  `buffer_length` >= 1 switches them on (or on anew: everything
        starts from zero, episodes under way are counted from this call) with a ring of that many recent episodes; 0
        switches them off.  One cold kernel behind every step (csrc/softrod_episode_stats.hpp), none while they are off.

        While they are on step() adds Gymnasium's vector keys to `infos`:
          infos["episode"] = {"r": (N,) float64 return, "l": (N,) int32 length in steps, "t": (N,) float64}
          infos["_episode"]  (N,) bool, True for the envs whose episode ended on this call
        with zero rows where `_episode` is False.  "t" is the episode's SIMULATED end time — the env clock at its last
        step — not elapsed wall-clock time as in Gymnasium's wrapper.  Device views overwritten by the next call (NumPy
        copies with numpy_output=True); `episode_info` gives the same views to a capture_policy_step loop, whose
        replay() keeps returning its four tensors.  Under NEXT_STEP auto-reset (True or "device") the call that
        returns an env's reset observation counts in no episode.  reset(mask=...) discards the masked envs' partial
        episodes; with autoreset=False an env that has finished is ignored until it is reset.  episode_statistics()
        reads the ring.

        Out of scope: step_packed raises NotImplementedError while statistics are on; not offered on the sharded env;
        not part of state_dict(), snapshot(), fork() or the state bank — a forked or loaded env keeps its own
        accumulators, so reset(mask=...) or a new record_episode_statistics() is the way to clear them; reward and
        observation normalisation are set_normalization()'s; no single-env wrapper (Gymnasium's own serves those).  A graph captured with
        capture_policy_step must be captured again after this call.

        ValueError for a negative length; NotImplementedError on a backend other than the HIP one."""
        ring = int(buffer_length)
        if ring < 0:
            raise ValueError(f"record_episode_statistics: buffer_length {ring} is negative")
        be = self.backend
        if not hasattr(be, "episode_stats_enable"):
            raise NotImplementedError(f"episode statistics need the HIP backend, not {type(be).__name__}")
        mode = (_capi.EPISODE_STATS_SAME_STEP if self.same_step
                else _capi.EPISODE_STATS_NEXT_STEP if self.autoreset or self.device_autoreset
                else _capi.EPISODE_STATS_MANUAL)
        be.episode_stats_enable(ring, mode)
        self._episode_ring = ring

    def _episode_infos(self) -> Dict[str, Any]:
        import torch

        st = self.backend.episode_stats
        return {"episode": {"r": self._out(st["ep_r"]), "l": self._out(st["ep_l"]), "t": self._out(st["ep_t"])},
                "_episode": self._out(st["ep_mask"].view(torch.bool))}

    @property
    def episode_info(self) -> Dict[str, Any]:
        """The infos["episode"] / infos["_episode"] entries of the last step or replay (record_episode_statistics):
        {"episode": {"r", "l", "t"}, "_episode"}.  The device views are the same objects' memory at every call."""
        if not self._episode_ring:
            raise _capi.SoftrodError("episode statistics are off (record_episode_statistics)")
        return self._episode_infos()

    def episode_statistics(self):
        """EpisodeStatistics(count, returns, lengths, times, envs, finished) as NumPy values (diagnostics.py): the
        number of episodes the batch has finished since record_episode_statistics(), the last min(count,
        buffer_length) of them in chronological order, oldest first — return, length, simulated end time and env —
        and the episodes ended per env.  The logging call: it waits for the env's stream."""
        from ..diagnostics import EpisodeStatistics, episode_ring_order

        if not self._episode_ring:
            raise _capi.SoftrodError("episode statistics are off (record_episode_statistics)")
        import torch

        st = self.backend.episode_stats
        torch.cuda.synchronize(self.backend.device)
        count = int(st["count"].cpu()[0])
        order = episode_ring_order(count, self._episode_ring)
        ring = [st[k].cpu().numpy()[order] for k in ("ring_r", "ring_l", "ring_t", "ring_env")]
        return EpisodeStatistics(count, *ring, st["finished"].cpu().numpy().copy())

    # -- observation and reward normalisation: running statistics kept on the device -------------
    def set_normalization(self, obs: bool = True, reward: bool = True, *, gamma: float = 0.99, clip_obs: float = 10.0,
                          clip_reward: float = 10.0, epsilon: float = 1e-8) -> None:
        """Normalise observations and / or rewards on the device with running statistics: what Gymnasium's
        NormalizeObservation / NormalizeReward and Stable-Baselines3's VecNormalize do for host envs, for a resident
        batch under every reset mode — by hand, autoreset=True, "device" and "same_step".  Upstream has single envs and
        no normalisation.  Call it before reset().  Called again it starts the statistics anew; obs=False,
        reward=False switches it off.  Two cold kernels behind every step (csrc/softrod_normalize.hpp), none while off.

        The statistics are Gymnasium's RunningMeanStd (mean 0, var 1, count 1e-4 at the start), one per observation
        column and one for the discounted return ret = ret * gamma + reward of every env.  While it is on
          step() / reset() return obs = clip((obs - mean) / sqrt(var + epsilon), -clip_obs, clip_obs), float32, and
          step() returns reward = clip(reward / sqrt(ret_var + epsilon), -clip_reward, clip_reward), float64 — no mean
          is subtracted, as in VecNormalize —
        computed with the statistics AFTER the call's own rows were counted; dtypes and shapes do not change.
        infos["raw_obs"] / infos["raw_reward"] hold the untouched device views; in same-step mode info["final_obs"]
        is normalised too (never counted) and infos["raw_final_obs"] is the raw one.  `normalization_info` gives the same
        views to a capture_policy_step loop, whose policy then reads the normalised observation.  Episode statistics
        (record_episode_statistics) keep reading the raw reward.  Non-finite values are not counted (an env that blew
        up does not poison the statistics): a NaN comes out as NaN, an infinity as +-clip.  Under NEXT_STEP auto-reset
        the call that returns an env's reset observation counts that observation, and its zero reward enters no return;
        with autoreset=False an env that has finished is not counted until reset(mask=...) names it; reset() counts
        the reset observations of the masked envs and starts their returns at zero.
        `normalization_training = False` freezes the statistics (evaluation); normalization_state() /
        load_normalization_state() carry them to another env or a checkpoint.

        Out of scope: step_packed raises NotImplementedError while normalisation is on; not offered on the sharded env
        (an all-reduce of the moments is a follow-up); not part of state_dict(), snapshot(), fork() or the state bank —
        a forked or loaded env keeps its own discounted return and latch; no single-env wrapper (Gymnasium's own serve
        those).  A graph captured with capture_policy_step must be captured again after this call.

        ValueError for gamma outside [0, 1] or a clip or epsilon that is not positive; NotImplementedError on a backend
        other than the HIP one."""
        gamma, clip_obs, clip_reward, epsilon = float(gamma), float(clip_obs), float(clip_reward), float(epsilon)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"set_normalization: gamma {gamma} is outside [0, 1]")
        for name, v in (("clip_obs", clip_obs), ("clip_reward", clip_reward), ("epsilon", epsilon)):
            if not v > 0.0:
                raise ValueError(f"set_normalization: {name} {v} is not positive")
        be = self.backend
        if not hasattr(be, "normalize_enable"):
            raise NotImplementedError(f"normalisation needs the HIP backend, not {type(be).__name__}")
        mode = (_capi.NORMALIZE_SAME_STEP if self.same_step
                else _capi.NORMALIZE_NEXT_STEP if self.autoreset or self.device_autoreset
                else _capi.NORMALIZE_MANUAL)
        be.normalize_enable(obs, reward, gamma=gamma, clip_obs=clip_obs, clip_reward=clip_reward, epsilon=epsilon,
                            mode=mode, in_step=not self.autoreset)
        be.normalize_update = self._norm_training
        self._norm_obs, self._norm_reward = bool(obs), bool(reward)

    @property
    def normalization_training(self) -> bool:
        """True (the default): every step and reset updates the running statistics.  False: they are frozen — the
        outputs keep following them, the discounted returns and latches stand still — as for evaluation.  A graph
        captured with capture_policy_step must be captured again after a change."""
        return self._norm_training

    @normalization_training.setter
    def normalization_training(self, on: bool) -> None:
        self._norm_training = bool(on)
        if hasattr(self.backend, "normalize_enable"):
            self.backend.normalize_update = self._norm_training

    def _normalized(self, obs, reward, infos):
        """The step's return values with normalisation on: adds the raw views to `infos`, swaps final_obs."""
        st = self.backend.normalize
        if self._norm_obs:
            infos["raw_obs"] = self._out(obs)
            obs = st["norm_obs"]
            if self.same_step:
                infos["raw_final_obs"] = infos["final_obs"]
                infos["final_obs"] = self._out(st["norm_final_obs"])
        if self._norm_reward:
            infos["raw_reward"] = self._out(reward)
            reward = st["norm_reward"]
        return obs, reward

    @property
    def normalization_info(self) -> Dict[str, Any]:
        """The normalisation entries of the last step or replay (set_normalization), for a capture_policy_step loop:
        {"obs", "raw_obs"} with observation normalisation on (and {"final_obs", "raw_final_obs"} in same-step mode),
        {"reward", "raw_reward"} with reward normalisation on.  The device views are the same memory at every call."""
        if not (self._norm_obs or self._norm_reward):
            raise _capi.SoftrodError("normalisation is off (set_normalization)")
        be, out = self.backend, {}
        if self._norm_obs:
            out.update(obs=self._out(be.normalize["norm_obs"]), raw_obs=self._out(be.obs))
            if self.same_step:
                out.update(final_obs=self._out(be.normalize["norm_final_obs"]), raw_final_obs=self._out(be.final_obs))
        if self._norm_reward:
            out.update(reward=self._out(be.normalize["norm_reward"]), raw_reward=self._out(be.reward))
        return out

    def normalization_state(self):
        """NormalizationState(obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count) as NumPy values
        (diagnostics.py): the running statistics as they stand.  It waits for the env's stream."""
        from ..diagnostics import NormalizationState

        if not (self._norm_obs or self._norm_reward):
            raise _capi.SoftrodError("normalisation is off (set_normalization)")
        import torch

        st = self.backend.normalize
        torch.cuda.synchronize(self.backend.device)
        return NormalizationState(*(st[k].cpu().numpy().copy() for k in ("obs_mean", "obs_var", "obs_count")),
                                  *(float(st[k].cpu()[0]) for k in ("ret_mean", "ret_var", "ret_count")))

    def load_normalization_state(self, state) -> None:
        """Set the running statistics from a NormalizationState (or any 6-tuple in its order), bit for bit; the
        discounted returns under way stay.  normalization_state() of one env loaded into another makes the two
        normalise alike."""
        if not (self._norm_obs or self._norm_reward):
            raise _capi.SoftrodError("normalisation is off (set_normalization)")
        self.backend.normalize_load(*state)

    def capture_policy_step(self, policy):
        """One HIP graph for `actions = policy(obs); step(actions)` — the launch-bound tail of an on-device
        rollout (a small policy is half a dozen tiny kernels per step) becomes ONE graph launch per env.step.
        `softrod_step` is capturable: it enqueues kernels on the caller's stream and does nothing else (no
        allocation, no synchronisation, no host read) while timing is off.

        policy: obs (N, obs_dim) float32 device tensor -> actions (N, action_dim) float32, pure device work.
        Returns replay() -> (obs, reward, terminated, truncated): the backend's resident output tensors, overwritten
        by every replay (as `step` does).  The observation the policy reads is the one the previous step wrote —
        call `reset` BEFORE capturing.  Needs autoreset off, "device" or "same_step" (the host-driven NEXT_STEP mode
        reads flags back every step and cannot live in a graph); the queue top-ups of the device modes stay outside
        the graph and run between replays.  In same-step mode the pass behind the step is one more kernel of the
        same straight line, and the finished observations are in backend.final_obs / final_time.  Results are
        bit-identical to the eager loop (tests/test_gpu_policy_loop.py, tests/test_gpu_same_step.py).
        The kernel arguments (RodParams, array pointers) are baked into the graph BY VALUE at capture: after
        anything that changes them (a radius profile, an action basis, enabling auto-reset, enabling per-env material or contact,
        setting or clearing a pool of start shapes with set_reset_shapes, switching episode statistics on or off with
        record_episode_statistics, switching normalisation on or off with set_normalization, changing
        normalization_training) capture again.  With normalisation on (set_normalization) the policy reads the normalised
        observation, the pass is two more kernels of the captured line, replay() returns the normalised observation and
        reward, and `normalization_info` holds the raw views.  With episode statistics on their update is one more kernel of the captured line and
        `episode_info` holds its rows after every replay.  Once per-env material is on, later set_material calls update its table in place: replays
        issued on the env's stream see them.  The same holds for per-env contact (set_contact).
        Kernel timing (set_timing) is switched off by the capture and stays off."""
        import torch

        if self.autoreset:
            raise NotImplementedError("capture_policy_step needs autoreset=False, 'device' or 'same_step'")
        if self.recorder is not None:
            raise NotImplementedError("capture_policy_step with a diagnostics recorder: the per-step host tap "
                                      "cannot live in a graph (config_generate_video=False)")
        be = self.backend
        if hasattr(be, "set_timing"):
            be.set_timing(0)                      # event records around the kernel are not part of the graph:
                                                  # kernel timing is OFF from here on (call set_timing again to re-arm)
        side = torch.cuda.Stream(device=be.device)
        side.wait_stream(torch.cuda.current_stream(be.device))
        seen = be.normalize["norm_obs"] if self._norm_obs else be.obs      # what the policy reads
        with torch.cuda.stream(side):             # warm-up off the capture: the POLICY only (lazy BLAS handles,
            for _ in range(3):                    # allocator pools); it is a pure function of the observation, and
                policy(seen)                      # softrod_step has nothing lazy to warm up, so no state moves
        torch.cuda.current_stream(be.device).wait_stream(side)
        torch.cuda.synchronize(be.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            be.step(policy(seen))
        out_obs = seen
        out_reward = be.normalize["norm_reward"] if self._norm_reward else be.reward

        def replay():
            graph.replay()
            if self.device_autoreset:
                self._top_up_tick()
            else:
                self._steps += 1                  # what step() books: infos["time"] of a later eager step stays right
            return out_obs, out_reward, be.terminated.view(torch.bool), be.truncated.view(torch.bool)

        replay.graph = graph
        return replay

    def step_packed(self, actions, out=None):
        """step() with every per-env output in one (N, packed_width) float32 buffer written
        by the kernel itself (distributed.unpack_outputs gives views); no host auto-reset.  NotImplementedError while
        episode statistics (record_episode_statistics) or normalisation (set_normalization) are on."""
        import torch

        if self.autoreset:
            raise NotImplementedError("step_packed does not auto-reset on the host; use autoreset='device'")
        self._validate_actions(actions)
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.backend.device)
        a = a.reshape(self.num_envs, self.action_dim)
        packed = self.backend.step_packed(a) if out is None else self.backend.step_packed(a, out)
        if self.device_autoreset:
            self._top_up_tick()
            # same-step mode: the packed row has no room for a second observation; the finished one is the dense
            # resident buffer, valid in the rows whose packed flags are set
            return packed, ({"final_obs": self._out(self.backend.final_obs)} if self.same_step else {})
        self._steps += 1
        return packed, self._infos(self._times())

    # -- fork: many rollouts from one env's current state (planning) --------------------
    def fork(self, src, dst, copy_rng: bool = True) -> None:
        """Make env dst[i] an exact copy of env src[i], now, without leaving the GPU: what CEM, MPPI, population-based
        training or branching a rollout for a value estimate start from.  `src`, `dst`: array-likes of env indices of
        one length; a scalar `src` broadcasts, so fork(0, range(1, N)) makes every env a copy of env 0.  The reference
        has no counterpart (one env is one Python object there).

        Copied: the whole resident state of the env and its per-env material and contact (backend.copy_envs:
        softrod_copy_envs, include/softrod.h), and the host bookkeeping — steps since reset, a pending host
        auto-reset, the reset target (`targets`) and the tracked trajectory where the env has them.  With
        `copy_rng=True` dst also takes the state of src's NumPy stream: the copies then draw the same resets as their
        source.  With `copy_rng=False` dst keeps its own stream and the copies' next episodes differ.  A copy and its
        source, stepped with the same actions, return bitwise-equal observations, rewards and flags.

        SoftrodError for indices outside the batch, an env twice in dst, or an env that is the dst of one pair and the
        src of another (fork in two calls instead); nothing changes then.  NotImplementedError with
        autoreset="device" (reset records staged on the device belong to each env's RNG future, as for state_dict()).
        Not offered on the sharded env (distributed.py: src and dst may live on different GPUs) nor on the N = 1
        single-env classes (SingleRodEnv: there is nothing to fork into)."""
        if self.device_autoreset:
            raise NotImplementedError(f"fork() with autoreset='{'same_step' if self.same_step else 'device'}': "
                                      "staged reset records are not copied")
        be = self.backend
        if not hasattr(be, "copy_envs"):
            raise NotImplementedError(f"fork needs the HIP backend, not {type(be).__name__}")
        s, d = _capi.copy_envs_pairs(src, dst)
        # shaped starts: reset_shape_index is copied; reset_shape_episode belongs to the RNG future, so without
        # copy_rng dst keeps its own
        own = be.reset_shape_episode[d.tolist()].clone() if self._reset_shapes and not copy_rng and d.size else None
        be.copy_envs(s, d)
        if own is not None:
            be.reset_shape_episode[d.tolist()] = own
        self._steps[d] = self._steps[s]
        self._needs_reset[d] = self._needs_reset[s]
        for k in ("targets", "_traj"):
            rows = getattr(self, k, None)
            if rows is not None:
                rows[d] = rows[s]
        if copy_rng:
            for i, j in zip(s.tolist(), d.tolist()):
                if i == j:
                    continue
                if self._rngs[i] is None:
                    self._rngs[j] = None
                else:
                    if self._rngs[j] is None:
                        self._rngs[j], _ = np_random(0)
                    self._rngs[j].bit_generator.state = self._rngs[i].bit_generator.state

    # -- the state bank: states held beside the batch, loaded into any envs, many times ---------
    def _state_bank_backend(self, what: str):
        if self.device_autoreset:
            raise NotImplementedError(f"{what}() with autoreset='{'same_step' if self.same_step else 'device'}': "
                                      "staged reset records are not copied")
        if not hasattr(self.backend, "bank_create"):
            raise NotImplementedError(f"{what} needs the HIP backend, not {type(self.backend).__name__}")
        return self.backend

    def create_state_bank(self, slots: int) -> None:
        """Give this batch a state bank: `slots` off-batch slots on the device, each holding one complete env state —
        everything fork() copies — that no step and no reset touches.  save_states() fills slots from envs,
        load_states() makes envs copies of slots, any subset, any number of times: restart distributions over visited
        states (Go-Explore archives, backplay, demonstration states), branched rollouts from stored states, tree
        search that returns to a node, a planner that parks its trajectory while all N envs explore.  Where fork()
        needs a live env per kept state, and snapshot() / restore() move the whole batch through the host.  The
        reference has no counterpart.  Once per env; `state_bank_bytes` device bytes per slot.

        The bank is no part of state_dict(): a checkpoint carries the batch, not the slots.  NotImplementedError with
        autoreset="device" / "same_step" (as fork()) and on a backend without bank_create.  Not offered on the
        sharded env (distributed.py).  softrod_bank_create, include/softrod.h."""
        self._state_bank_backend("create_state_bank").bank_create(slots)
        self._bank_book: List[Optional[dict]] = [None] * int(slots)      # the host bookkeeping saved with each slot

    def save_states(self, envs, slots) -> None:
        """Slot slots[i] becomes an exact copy of env envs[i], now, without leaving the GPU.  Array-likes of indices of
        one length; a scalar `envs` broadcasts over `slots`.  An env may go into several slots, a slot may appear once;
        saving into a filled slot replaces what it held.  Saved with the resident state (backend.bank_save:
        softrod_bank_save) is the host bookkeeping fork() moves: steps since reset, a pending host auto-reset, the
        reset target (`targets`) and the tracked trajectory where the env has them, and the state of the env's NumPy
        stream.  SoftrodError for an index outside the batch or the bank, or a slot twice; nothing changes then."""
        be = self._state_bank_backend("save_states")
        e, s = _capi.state_bank_pairs(envs, slots, ("envs", "slots"))
        be.bank_save(e, s)
        for i, k in zip(e.tolist(), s.tolist()):
            book = {"steps": int(self._steps[i]), "needs_reset": bool(self._needs_reset[i]),
                    "rng": None if self._rngs[i] is None else self._rngs[i].bit_generator.state}
            for name in ("targets", "_traj"):
                rows = getattr(self, name, None)
                if rows is not None:
                    book[name] = np.array(rows[i])
            self._bank_book[k] = book

    def load_states(self, slots, envs, copy_rng: bool = True) -> None:
        """Env envs[i] becomes an exact copy of slot slots[i] — of the env that was saved there, as it stood then — and,
        stepped with the same actions, continues bitwise as that env did.  A scalar `slots` broadcasts over `envs`; a
        slot may feed many envs, an env may appear once; the slot keeps its state.  The host bookkeeping saved with
        the slot comes back too (save_states).  With `copy_rng=True` the env also takes the NumPy stream saved with
        the slot: its next reset draws what the saved env's would have.  With `copy_rng=False` it keeps its own
        stream and, with a pool of reset shapes, its own `reset_shape_episode`, as fork(copy_rng=False) does.  A
        per-env material / contact table or a pool of reset shapes set after the save: the slot loads as its env would
        be now, had nothing touched it since (the config's row; reset_shape_index -1, episode 0).  SoftrodError for an
        index outside the batch or the bank, an env twice, or a slot that was never saved; nothing changes then."""
        be = self._state_bank_backend("load_states")
        s, d = _capi.state_bank_pairs(slots, envs, ("slots", "envs"))
        own = be.reset_shape_episode[d.tolist()].clone() if self._reset_shapes and not copy_rng and d.size else None
        be.bank_load(s, d)
        if own is not None:
            be.reset_shape_episode[d.tolist()] = own
        for k, j in zip(s.tolist(), d.tolist()):
            book = self._bank_book[k]
            self._steps[j] = book["steps"]
            self._needs_reset[j] = book["needs_reset"]
            for name in ("targets", "_traj"):
                if name in book:
                    getattr(self, name)[j] = book[name]
            if copy_rng:
                if book["rng"] is None:
                    self._rngs[j] = None
                else:
                    if self._rngs[j] is None:
                        self._rngs[j], _ = np_random(0)
                    self._rngs[j].bit_generator.state = book["rng"]

    @property
    def state_bank_slots(self) -> int:
        """Slots of the state bank; 0 before create_state_bank."""
        return self.backend.bank_info()[0] if hasattr(self.backend, "bank_info") else 0

    @property
    def state_bank_filled(self) -> np.ndarray:
        """(state_bank_slots,) bool: True where a slot holds a saved state."""
        return self.backend.bank_info()[2] if hasattr(self.backend, "bank_info") else np.zeros(0, bool)

    @property
    def state_bank_bytes(self) -> int:
        """Device bytes of one slot: one env's whole resident state, what a save or a load moves per pair."""
        return self.backend.bank_info()[1] if hasattr(self.backend, "bank_info") else 0

    # -- checkpoint / resume ----------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """Everything needed to continue this batch exactly where it is: the resident state
        (backend.snapshot()) and the host bookkeeping (steps since reset, pending auto-resets,
        every env's RNG state).  The reference never serialises an env; this is
        an addition.  Not available with autoreset="device" (reset records staged on the device
        belong to the RNG streams' future).  The state bank (create_state_bank) is not part of it:
        the slots' states stay on the device and are not carried by a checkpoint."""
        if self.device_autoreset:
            raise NotImplementedError(f"state_dict() with autoreset='{'same_step' if self.same_step else 'device'}': "
                                      "staged reset records are not captured")
        extra = {k: np.array(getattr(self, k)) for k in ("targets", "_traj") if getattr(self, k, None) is not None}
        return {
            "backend": self.backend.snapshot(),
            "steps": self._steps.copy(),
            "needs_reset": self._needs_reset.copy(),
            "rng": [None if g is None else g.bit_generator.state for g in self._rngs],
            "extra": extra,
        }

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        self.backend.restore(sd["backend"])
        self._steps[:] = sd["steps"]
        self._needs_reset[:] = sd["needs_reset"]
        for i, st in enumerate(sd["rng"]):
            if st is None:
                self._rngs[i] = None
            else:
                if self._rngs[i] is None:
                    self._rngs[i], _ = np_random(0)
                self._rngs[i].bit_generator.state = st
        for k, v in sd.get("extra", {}).items():
            setattr(self, k, np.array(v))

    def close(self):
        if self.backend is not None and hasattr(self.backend, "close"):
            self.backend.close()
