"""Device backend: one `softrod_handle` (include/softrod.h) per GPU, fed with torch-ROCm
tensors.  torch is plumbing only (device memory, streams); all arithmetic of the hot
path happens in libsoftrod_hip.so.  There is no CPU fallback here by design."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import LANE_STRIDE, SoftrodConfig, SoftrodStateView, check, load_library
from .diagnostics import (JointLoads, MuscleLoads, RodClearance, RodDynamics, RodStrains, joint_loads_views,
                          muscle_loads_views, rod_clearance_views, rod_dynamics_views, rod_strains_views)


class _DevArray:
    """Borrowed device memory exposed through __cuda_array_interface__ (zero-copy)."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self._owner = owner  # keeps the handle alive
        self.__cuda_array_interface__ = {
            "shape": tuple(shape),
            "typestr": typestr,
            "data": (int(ptr), False),
            "version": 2,
            "strides": None,
        }


def _set_env_table(self, name: str, width: int, values, mask) -> None:
    """HipRodBackend.set_env_<name>: one per-env table (softrod_set_env_<name>): refusal, upload, and the host copy."""
    why = getattr(_capi, f"env_{name}_refusal")(self.cfg, tapered="radius_profile" in self._tables)
    if why is not None:
        raise NotImplementedError(why)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(self.n_envs, width)
    k = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n_envs)
    check(getattr(self._lib, f"softrod_set_env_{name}")(self._h, v.ctypes.data, None if k is None else k.ctypes.data,
                                                        self._stream()), self._h)
    cur = _env_table(self, name)
    setattr(self, f"_env_{name}", np.where(k[:, None] != 0, v, cur) if k is not None else v.copy())

def _env_table(self, name: str) -> np.ndarray:
    """HipRodBackend.env_<name>() (a function of the backend, so that a stand-in backend can borrow the method)."""
    cur = getattr(self, f"_env_{name}", None)
    if cur is None:
        return np.tile(getattr(_capi, f"env_{name}_defaults")(self.cfg), (self.n_envs, 1))
    return cur.copy()


class HipRodBackend:
    """Resident batch of rods on one MI355X."""

    def __init__(self, cfg: SoftrodConfig, device: int = 0):
        if not torch.cuda.is_available():
            raise _capi.SoftrodError(
                "HipRodBackend needs a ROCm device (torch.cuda.is_available() is False); "
                "the hot path has no CPU fallback"
            )
        self._lib = load_library()
        self.cfg = cfg.copy()
        self.n_envs = int(cfg.n_envs)
        self.action_dim = _capi.config_action_dim(cfg)
        self.obs_dim = _capi.config_obs_dim(cfg)
        # FlatEnv's host API (reset_octo, Dict observations); the muscle arm with a weight (ENV_ARM_PULL_WEIGHT) has a
        # rigid body too but resets and observes like any single rod
        self.is_octo = bool(cfg.features & _capi.FEAT_OCTO_HEAD) and int(cfg.env_kind) == _capi.ENV_OCTO_FLAT
        # the muscle octopus envs (CrawlEnv / ArmTwoEnv / ReachEnv): FlatEnv's reset API with their own arm frames,
        # three numbers per target
        self.is_mocto = int(cfg.env_kind) in _capi.MUSCLE_OCTOPUS_ENVS
        self.aux_dim = _capi.aux_dim(cfg.env_kind)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self._h = C.c_void_p()
        # per-handle physics tables that live outside softrod_config (action basis, spline table,
        # radius profile): their bytes go into config_fingerprint()
        self._tables: Dict[str, bytes] = {}
        self._readouts: Dict[str, torch.Tensor] = {}     # rod_energies / ground_reaction / rod_strains / muscle_loads / joint_loads / rod_dynamics / rod_clearance buffers (_readout)
        self._frames: Dict[tuple, torch.Tensor] = {}      # render(): the RGB and depth frames per (H, W)
        check(self._lib.softrod_create(C.byref(self.cfg), self.device_index, C.byref(self._h)))
        if self.cfg.features & _capi.FEAT_REST_KAPPA_ACTION:
            if self.is_octo:
                basis = _capi.octo_action_basis(int(cfg.n_elem), int(cfg.n_knots))
            else:
                basis = _capi.action_basis(int(cfg.n_elem), self.action_dim)
            check(self._lib.softrod_set_action_basis(self._h, basis.ctypes.data), self._h)
            self._tables["action_basis"] = basis.tobytes()
        if int(cfg.env_kind) == _capi.ENV_ARM_TWO:
            basis, _ = _capi.arm_two_activation_basis(int(cfg.n_elem), 3)
            check(self._lib.softrod_set_action_basis(self._h, basis.ctypes.data), self._h)
            self._tables["action_basis"] = basis.tobytes()
        if self.cfg.features & _capi.FEAT_SPLINE_MUSCLE_TORQUES:
            breaks, coef = _capi.spline_table(float(cfg.base_length), int(cfg.n_ctrl))
            if len(breaks) != int(cfg.n_spline_pieces) + 1:
                raise _capi.SoftrodError("n_spline_pieces does not match the interpolant")
            check(self._lib.softrod_set_spline_table(self._h, breaks.ctypes.data, coef.ctypes.data), self._h)
            self._tables["spline_table"] = breaks.tobytes() + coef.tobytes()
        n = self.n_envs
        with torch.cuda.device(self.device):
            self.obs = torch.empty((n, self.obs_dim), dtype=torch.float32, device=self.device)
            self.reward = torch.empty((n,), dtype=torch.float64, device=self.device)
            self.terminated = torch.empty((n,), dtype=torch.uint8, device=self.device)
            self.truncated = torch.empty((n,), dtype=torch.uint8, device=self.device)
            self.aux = (
                torch.empty((n, self.aux_dim), dtype=torch.float64, device=self.device)
                if self.aux_dim else None
            )

    # -- lifetime -------------------------------------------------------------------
    # The zero-copy views of the handle's memory that the backend keeps on itself.  Each is a tensor over a _DevArray that
    # names this backend as its owner, through a reference torch holds outside Python's sight: backend -> view -> backend
    # is a cycle no collection breaks, and with it every tensor of a closed backend (obs, reward, ...) would stay allocated.
    _HANDLE_VIEWS = ("episode_stats", "normalize", "_reset_shape_rows", "reset_shapes_count", "final_obs", "final_time",
                     "final_aux", "_episode_clock", "_prev_rows")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.softrod_destroy(self._h)
            self._h = C.c_void_p()
            for name in self._HANDLE_VIEWS:         # they point into freed memory now; the class's "off" values show again
                self.__dict__.pop(name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _actions(self, actions) -> torch.Tensor:
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device).reshape(-1)
        if a.numel() != self.n_envs * self.action_dim:
            raise ValueError(f"expected {self.n_envs}x{self.action_dim} actions, got {a.numel()}")
        return a.contiguous()

    # -- C-ABI calls ----------------------------------------------------------------
    def set_radius_profile(self, radius) -> None:
        """CosseratRod.straight_rod(base_radius=<array>): a tapered rod (octopus/arm_push_env.py:
        160-179).  Before the first reset."""
        r = np.ascontiguousarray(radius, dtype=np.float64).reshape(int(self.cfg.n_elem))
        check(self._lib.softrod_set_radius_profile(self._h, r.ctypes.data), self._h)
        self._tables["radius_profile"] = r.tobytes()

    def set_muscle_layers(self, ratio_position, strength) -> None:
        """The layers handed to COOMM's ApplyMuscles (softrod_set_muscle_layers): ratio_position
        (n_muscles, 3, n_elem), strength = max_muscle_stress * rest_muscle_area (n_muscles, n_elem), signed."""
        m, n = int(self.cfg.n_muscles), int(self.cfg.n_elem)
        rp = np.ascontiguousarray(ratio_position, dtype=np.float64).reshape(m, 3, n)
        st = np.ascontiguousarray(strength, dtype=np.float64).reshape(m, n)
        check(self._lib.softrod_set_muscle_layers(self._h, rp.ctypes.data, st.ctypes.data), self._h)
        self._tables["muscle_layers"] = rp.tobytes() + st.tobytes()

    def set_env_material(self, material, mask: Optional[np.ndarray] = None) -> None:
        """softrod_set_env_material: per-env (E, G, rho, nu), host (n_envs, 4) float64; only rows with mask != 0
        change.  Takes effect at the next launch on the current stream; persists through resets."""
        _set_env_table(self, "material", 4, material, mask)

    def env_material(self) -> np.ndarray:
        """(n_envs, 4) float64 host copy of every env's (E, G, rho, nu): the config's until set_env_material."""
        return _env_table(self, "material")

    def set_env_contact(self, contact, mask: Optional[np.ndarray] = None) -> None:
        """softrod_set_env_contact: per-env (contact_k, contact_nu, kinetic_mu[3], static_mu[3]), host (n_envs, 8)
        float64; only rows with mask != 0 change.  Takes effect at the next launch on the current stream; persists
        through resets."""
        _set_env_table(self, "contact", 8, contact, mask)

    def env_contact(self) -> np.ndarray:
        """(n_envs, 8) float64 host copy of every env's (k, nu, kinetic_mu[3], static_mu[3]): the config's until
        set_env_contact."""
        return _env_table(self, "contact")

    def copy_envs(self, src, dst) -> None:
        """softrod_copy_envs: fork on the device — env dst[i] becomes a bitwise copy of env src[i] as it stood before
        the call: its part of every array of state(), and its row of the per-env material / contact tables where they
        exist.  `src`, `dst`: array-likes of ints of one length; a scalar `src` broadcasts over `dst`
        (copy_envs(0, range(1, n))).  One small upload and one kernel on the current stream, no synchronisation —
        where snapshot() / restore() move the whole batch through the host.  Not graph-capturable.  SoftrodError
        where the library refuses (include/softrod.h): an index outside the batch, an env twice in dst, an env that
        is the dst of one pair and the src of another, a handle with device-side auto-reset; a refused call changes
        nothing.  An empty call and a pair with src == dst are no-ops.  env_material() / env_contact() and a later
        snapshot() follow the copy."""
        s, d = _capi.copy_envs_pairs(src, dst)
        check(self._lib.softrod_copy_envs(self._h, s.ctypes.data if s.size else None, d.ctypes.data if d.size else None,
                                          int(s.size), self._stream()), self._h)
        for name in ("_env_material", "_env_contact"):
            tab = getattr(self, name, None)
            if tab is not None:
                tab[d] = tab[s]

    # -- the state bank (softrod_bank_create / _save / _load / _info) ---------------------------------
    def bank_create(self, slots: int) -> None:
        """softrod_bank_create: `slots` off-batch slots on the device, each holding one complete env state — everything
        copy_envs copies.  Steps and resets never touch a slot.  Once per backend.  SoftrodError where the library
        refuses (include/softrod.h): a second bank, slots < 1, a handle with device-side auto-reset, no memory."""
        check(self._lib.softrod_bank_create(self._h, int(slots)), self._h)
        # the per-slot mirrors of _env_material / _env_contact: the config's row until a save brings another
        self._bank_tables = {name: np.tile(getattr(_capi, f"env_{name}_defaults")(self.cfg), (int(slots), 1))
                             for name in ("material", "contact")}

    def bank_save(self, envs, slots) -> None:
        """softrod_bank_save: slot slots[i] becomes a bitwise copy of env envs[i], its row of the per-env material /
        contact tables included.  Array-likes of ints of one length; a scalar `envs` broadcasts over `slots`.  An env
        may go into several slots, a slot may appear once.  One small upload and one kernel on the current stream, no
        synchronisation.  Not graph-capturable.  SoftrodError where the library refuses; a refused call changes nothing."""
        e, s = _capi.state_bank_pairs(envs, slots, ("envs", "slots"))
        check(self._lib.softrod_bank_save(self._h, e.ctypes.data if e.size else None, s.ctypes.data if s.size else None,
                                          int(e.size), self._stream()), self._h)
        for name, rows in getattr(self, "_bank_tables", {}).items():
            tab = getattr(self, f"_env_{name}", None)
            if tab is not None:         # no table yet: every env and every slot is at the config's row
                rows[s] = tab[e]

    def bank_load(self, slots, envs) -> None:
        """softrod_bank_load: env envs[i] becomes a bitwise copy of slot slots[i].  A scalar `slots` broadcasts over
        `envs`; a slot may feed many envs, an env may appear once, a slot never saved is refused.  env_material() /
        env_contact() and a later snapshot() follow the load.  Otherwise as bank_save."""
        s, e = _capi.state_bank_pairs(slots, envs, ("slots", "envs"))
        check(self._lib.softrod_bank_load(self._h, s.ctypes.data if s.size else None, e.ctypes.data if e.size else None,
                                          int(s.size), self._stream()), self._h)
        for name, rows in getattr(self, "_bank_tables", {}).items():
            tab = getattr(self, f"_env_{name}", None)
            if tab is not None:
                tab[e] = rows[s]

    def bank_info(self) -> Tuple[int, int, np.ndarray]:
        """softrod_bank_info: (slots, bytes_per_slot, filled) — slots 0 without a bank; bytes_per_slot the device bytes
        of one env's state, what a save or load moves per pair; filled (slots,) bool, True where a slot holds a state."""
        slots, nbytes = C.c_int32(0), C.c_uint64(0)
        check(self._lib.softrod_bank_info(self._h, C.byref(slots), C.byref(nbytes), None), self._h)
        filled = np.zeros(slots.value, np.uint8)
        if slots.value:
            check(self._lib.softrod_bank_info(self._h, C.byref(slots), C.byref(nbytes), filled.ctypes.data), self._h)
        return int(slots.value), int(nbytes.value), filled.astype(bool)

    def set_rod_shape(self, mask=None, *, kappa=None, sigma=None, velocity=None, omega=None) -> torch.Tensor:
        """softrod_set_rod_shape: rebuild every rod of the envs with mask != 0 (None: all) from its base pose and the
        strain fields, in rod_strains()' conventions (include/softrod.h) — kappa (n_envs, rods_per_env, 3, n_elem - 1),
        sigma (.., 3, n_elem), velocity (.., 3, n_elem + 1), omega (.., 3, n_elem), float64; None: all zero.  A float64
        torch tensor on this device is used in place; anything else is coerced once, as step()'s actions are.  One
        kernel on the current stream and one observe(None): -> the new observations (`obs`).  Between a reset and the
        first step only; the env layer checks that, this method does not."""
        ptrs, keep = [], []
        for name, v in zip(_capi.ROD_SHAPE_FIELDS, (kappa, sigma, velocity, omega)):
            if v is None:
                ptrs.append(None)
                continue
            shape = _capi.rod_shape_field_shape(self.cfg, self.n_envs, name)
            t = torch.as_tensor(v, dtype=torch.float64, device=self.device)
            if t.numel() != int(np.prod(shape)):
                raise ValueError(f"set_rod_shape: {name} must have shape {shape}, got {tuple(t.shape)}")
            t = t.reshape(shape).contiguous()
            keep.append(t)
            ptrs.append(t.data_ptr())
        m = None
        if mask is not None:
            host = mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask)
            m = torch.as_tensor(np.ascontiguousarray(host != 0, dtype=np.uint8).reshape(self.n_envs), device=self.device)
        check(self._lib.softrod_set_rod_shape(self._h, *ptrs, m.data_ptr() if m is not None else None, self._stream()),
              self._h)
        return self.observe(None)

    # -- shaped starts under every reset (softrod_set_reset_shapes) -------------------------------
    reset_shapes_count = 0      # entries of the pool; 0: none set

    def set_reset_shapes(self, *, kappa=None, sigma=None, velocity=None, omega=None, seed: int = 0) -> int:
        """softrod_set_reset_shapes: a resident pool of K start shapes, the fields of set_rod_shape with the pool axis
        in place of the env axis — kappa (K, rods_per_env, 3, n_elem - 1), sigma (.., 3, n_elem), velocity
        (.., 3, n_elem + 1), omega (.., 3, n_elem), float64; None: all zero; every given field the same K.  The library
        copies them into buffers of its own in this call.  No field at all clears the pool.  While a pool is set every
        reset of an env — apply_reset_shapes after a reset by hand, the device auto-reset passes on their own — starts
        it from entry _capi.reset_shape_index(seed, env, reset_shape_episode[env], K).  A call sets reset_shape_index
        to -1 and reset_shape_episode to 0 for every env and shapes nothing itself.  -> K.  A captured graph must be
        captured again after the call."""
        fields = dict(zip(_capi.ROD_SHAPE_FIELDS, (kappa, sigma, velocity, omega)))
        count = _capi.reset_shapes_pool(self.cfg, fields)
        ptrs, keep = [], []
        for name in _capi.ROD_SHAPE_FIELDS:
            v = fields[name]
            if v is None:
                ptrs.append(None)
                continue
            shape = (count,) + _capi.rod_shape_field_shape(self.cfg, 0, name)[1:]
            t = torch.as_tensor(v, dtype=torch.float64, device=self.device).reshape(shape).contiguous()
            keep.append(t)
            ptrs.append(t.data_ptr())
        check(self._lib.softrod_set_reset_shapes(self._h, count, *ptrs, int(seed) % 2**64, self._stream()), self._h)
        self.reset_shapes_count = count
        if count and getattr(self, "_reset_shape_rows", None) is None:
            ix, ep = C.c_void_p(), C.c_void_p()
            check(self._lib.softrod_reset_shapes_view(self._h, C.byref(ix), C.byref(ep)), self._h)
            self._reset_shape_rows = tuple(torch.as_tensor(_DevArray(p.value, (self.n_envs,), "<i4", self), device=self.device)
                                           for p in (ix, ep))
        return count

    def apply_reset_shapes(self, mask=None) -> None:
        """softrod_apply_reset_shapes: after a reset by hand, shape the envs with mask != 0 (None: all) from their pool
        entries, record the indices and count the resets.  Two kernels on the current stream; observe afterwards."""
        m = None
        if mask is not None:
            host = mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask)
            m = torch.as_tensor(np.ascontiguousarray(host != 0, dtype=np.uint8).reshape(self.n_envs), device=self.device)
        check(self._lib.softrod_apply_reset_shapes(self._h, m.data_ptr() if m is not None else None, self._stream()), self._h)

    def _reset_shape_row(self, i: int) -> torch.Tensor:
        if not self.reset_shapes_count:
            raise _capi.SoftrodError("no pool of reset shapes is set (set_reset_shapes)")
        return self._reset_shape_rows[i]

    @property
    def reset_shape_index(self) -> torch.Tensor:
        """(n_envs,) int32 zero-copy view: the pool entry each env's current episode started from, -1: none yet."""
        return self._reset_shape_row(0)

    @property
    def reset_shape_episode(self) -> torch.Tensor:
        """(n_envs,) int32 zero-copy view: resets counted per env = the next reset's ordinal; writable."""
        return self._reset_shape_row(1)

    def reset(self, theta0: np.ndarray, mask: Optional[np.ndarray] = None) -> None:
        th =np.ascontiguousarray(theta0, dtype=np.float64).reshape(self.n_envs)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n_envs)
        check(
            self._lib.softrod_reset(
                self._h, th.ctypes.data, m.ctypes.data if m is not None else None, self._stream()
            ),
            self._h,
        )

    def reset_straight(self, start, direction, normal, mask: Optional[np.ndarray] = None) -> None:
        arrs = [
            np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (self.n_envs, 3)))
            for v in (start, direction, normal)
        ]
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n_envs)
        check(
            self._lib.softrod_reset_straight(
                self._h, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                m.ctypes.data if m is not None else None, self._stream(),
            ),
            self._h,
        )

    def _arm_frames(self):
        if self.is_mocto:
            pos, dirs, _ = _capi.muscle_octopus_arm_frames(int(self.cfg.env_kind), float(self.cfg.head_radius))
            return pos, dirs
        return _capi.octo_arm_frames(int(self.cfg.n_arm), float(self.cfg.head_radius))

    def reset_octo(self, targets, mask: Optional[np.ndarray] = None) -> None:
        """FlatEnv.reset: targets (n_envs, 2); the arm frames are build_octopus's.  The muscle octopus envs: targets
        (n_envs, 4) — x, y, z and the episode's final_time (0: the config's) —, the frames of build_octopus_muscles / build_two_arms."""
        na = int(self.cfg.n_arm)
        pos, dirs = self._arm_frames()
        pos = np.ascontiguousarray(np.broadcast_to(pos, (self.n_envs, na, 3)))
        dirs = np.ascontiguousarray(np.broadcast_to(dirs, (self.n_envs, na, 3)))
        tg = np.ascontiguousarray(targets, dtype=np.float64).reshape(self.n_envs, 4 if self.is_mocto else 2)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n_envs)
        check(
            self._lib.softrod_reset_octo(
                self._h, pos.ctypes.data, dirs.ctypes.data, tg.ctypes.data,
                m.ctypes.data if m is not None else None, self._stream(),
            ),
            self._h,
        )

    # -- device-side auto-reset (softrod_autoreset_enable / softrod_queue_*) ---------------------
    def autoreset_enable(self, depth: int) -> None:
        check(self._lib.softrod_autoreset_enable(self._h, int(depth)), self._h)
        self.queue_depth = int(depth)

    def autoreset_same_step(self, on: bool = True) -> None:
        """softrod_autoreset_same_step: Gymnasium's SAME_STEP semantics on the staged queue (after autoreset_enable).
        A step that ends an env's episode keeps its reward and flags, leaves the NEW episode's first observation in
        `obs` and the finished one in `final_obs` / `final_time` / `final_aux`: zero-copy device views, valid for the
        backend's life, of which a call rewrites the rows of the envs it finished (terminated | truncated) and no
        others.  `on=False` returns to NEXT_STEP.  A captured graph must be captured again after a switch."""
        check(self._lib.softrod_autoreset_same_step(self._h, int(bool(on))), self._h)
        self.same_step = bool(on)
        if on and getattr(self, "final_obs", None) is None:
            fo, ft, fa = C.c_void_p(), C.c_void_p(), C.c_void_p()
            check(self._lib.softrod_final_view(self._h, C.byref(fo), C.byref(ft), C.byref(fa)), self._h)
            n = self.n_envs
            self.final_obs = torch.as_tensor(_DevArray(fo.value, (n, self.obs_dim), "<f4", self), device=self.device)
            self.final_time = torch.as_tensor(_DevArray(ft.value, (n,), "<f8", self), device=self.device)
            self.final_aux = torch.as_tensor(_DevArray(fa.value, (n,), "<f8", self), device=self.device)

    @staticmethod
    def _counts(counts, n):
        return np.ascontiguousarray(counts, dtype=np.int32).reshape(n)

    def queue_push(self, theta0, counts) -> None:
        th = np.ascontiguousarray(theta0, dtype=np.float64).reshape(self.n_envs, -1)
        c = self._counts(counts, self.n_envs)
        check(self._lib.softrod_queue_push(self._h, th.ctypes.data, c.ctypes.data, th.shape[1], self._stream()),
              self._h)

    def queue_push_straight(self, start, direction, normal, counts) -> None:
        arrs = [np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_envs, -1, 3)
                for v in (start, direction, normal)]
        c = self._counts(counts, self.n_envs)
        check(self._lib.softrod_queue_push_straight(
            self._h, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, c.ctypes.data,
            arrs[0].shape[1], self._stream()), self._h)

    def queue_push_octo(self, targets, counts) -> None:
        na = int(self.cfg.n_arm)
        tg = np.ascontiguousarray(targets, dtype=np.float64).reshape(self.n_envs, -1, 4 if self.is_mocto else 2)
        m = tg.shape[1]
        pos, dirs = self._arm_frames()
        pos = np.ascontiguousarray(np.broadcast_to(pos, (self.n_envs, m, na, 3)))
        dirs = np.ascontiguousarray(np.broadcast_to(dirs, (self.n_envs, m, na, 3)))
        c = self._counts(counts, self.n_envs)
        check(self._lib.softrod_queue_push_octo(
            self._h, pos.ctypes.data, dirs.ctypes.data, tg.ctypes.data, c.ctypes.data, m, self._stream()),
            self._h)

    def queue_status(self):
        """(consumed[n_envs], underflow) — synchronises the stream."""
        cons = np.zeros(self.n_envs, np.int32)
        uf = C.c_int32(0)
        check(self._lib.softrod_queue_status(self._h, cons.ctypes.data, C.byref(uf), self._stream()), self._h)
        return cons, int(uf.value)

    def queue_status_begin(self) -> None:
        """Start a non-blocking read of the queue counters (softrod_queue_status_begin)."""
        check(self._lib.softrod_queue_status_begin(self._h, self._stream()), self._h)

    def queue_status_poll(self, wait: bool = False):
        """None while the read is in flight, else (consumed[n_envs], underflow) as of when it was
        started; `wait` blocks until that read (not the whole stream) has arrived."""
        cons = np.zeros(self.n_envs, np.int32)
        uf = C.c_int32(0)
        rc = self._lib.softrod_queue_status_poll(self._h, int(bool(wait)), cons.ctypes.data, C.byref(uf))
        if rc < 0:
            check(rc, self._h)
        return None if rc == 0 else (cons, int(uf.value))

    def queue_advance(self, by) -> None:
        """Mark by[e] staged records of env e as used (by[e] < 0: all of them)."""
        b = np.ascontiguousarray(by, dtype=np.int32).reshape(self.n_envs)
        check(self._lib.softrod_queue_advance(self._h, b.ctypes.data, self._stream()), self._h)

    def observe(self, prev_action: Optional[torch.Tensor] = None) -> torch.Tensor:
        pa = None
        if prev_action is not None:
            pa = self._actions(prev_action)
        check(
            self._lib.softrod_observe(
                self._h, pa.data_ptr() if pa is not None else None, self.obs.data_ptr(), self._stream()
            ),
            self._h,
        )
        return self.obs

    def step(self, actions) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        a = self._actions(actions)
        check(
            self._lib.softrod_step(
                self._h, a.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                self.terminated.data_ptr(), self.truncated.data_ptr(),
                self.aux.data_ptr() if self.aux is not None else None, self._stream(),
            ),
            self._h,
        )
        if self.episode_stats is not None:       # softrod_episode_stats_update behind the step, on the same stream
            self.episode_stats_update(self.reward, self.terminated, self.truncated,
                                      self.final_time if self.episode_stats_mode == _capi.EPISODE_STATS_SAME_STEP
                                      else self._episode_clock, self.episode_stats_mode)
        if self.normalize is not None and self.normalize_in_step:      # softrod_normalize_step behind it, same stream
            self.normalize_step(self.obs, self.reward, self.terminated, self.truncated,
                                getattr(self, "final_obs", None) if self.normalize_mode == _capi.NORMALIZE_SAME_STEP else None)
        return self.obs, self.reward, self.terminated, self.truncated

    # -- episode statistics (softrod_episode_stats_enable / _update / _reset / _view) ------------------
    episode_stats: Optional[Dict[str, torch.Tensor]] = None     # the resident arrays while the feature is on
    episode_stats_mode = _capi.EPISODE_STATS_MANUAL             # what step() passes as `mode`

    def episode_stats_enable(self, ring: int, mode: Optional[int] = None) -> None:
        """softrod_episode_stats_enable: ring >= 1 allocates (or allocates anew) and zeroes the statistics arrays with a
        ring of `ring` finished episodes, 0 switches the feature off and frees them.  While it is on `episode_stats`
        holds zero-copy device views of every array (_capi.EPISODE_STATS_ARRAYS; `count` as int64) — new ones after
        every call — and step() runs the update behind softrod_step with its own reward / terminated / truncated and
        `mode` (None: SAME_STEP on a same-step handle, NEXT_STEP with device auto-reset, else MANUAL; a host-driven
        NEXT_STEP loop passes 1), the env clock row or, in SAME_STEP mode, `final_time` as the end time.  While it is
        off step() does one attribute test and nothing else.  A captured graph must be captured again after the
        call."""
        check(self._lib.softrod_episode_stats_enable(self._h, int(ring)), self._h)
        self.episode_stats = None
        if int(ring) == 0:
            return
        v = _capi.SoftrodEpisodeStatsView()
        check(self._lib.softrod_episode_stats_view(self._h, C.byref(v)), self._h)
        size = {"n": self.n_envs, "k": int(v.ring), "1": 1}
        views = {name: torch.as_tensor(_DevArray(getattr(v, name), (size[per],), typestr, self), device=self.device)
                 for name, typestr, per in _capi.EPISODE_STATS_ARRAYS}
        if mode is None:
            mode = (_capi.EPISODE_STATS_SAME_STEP if getattr(self, "same_step", False)
                    else _capi.EPISODE_STATS_NEXT_STEP if getattr(self, "queue_depth", 0) else _capi.EPISODE_STATS_MANUAL)
        self.episode_stats_mode = int(mode)
        if getattr(self, "_episode_clock", None) is None:
            with self._views() as st:           # the clock row, kept and only read
                self._episode_clock = st["time"]
        self.episode_stats = views

    def episode_stats_update(self, reward, terminated, truncated, end_time, mode: int) -> None:
        """softrod_episode_stats_update: one update from device tensors reward f64 (n_envs,), terminated / truncated
        uint8 or bool (n_envs,), end_time f64 (n_envs,) or None (t = 0); mode 0 manual, 1 NEXT_STEP, 2 SAME_STEP.  One
        kernel on the current stream; capturable.  step() calls it itself while the feature is on."""
        check(self._lib.softrod_episode_stats_update(
            self._h, reward.data_ptr() if reward is not None else None,
            terminated.data_ptr() if terminated is not None else None,
            truncated.data_ptr() if truncated is not None else None,
            end_time.data_ptr() if end_time is not None else None, int(mode), self._stream()), self._h)

    def episode_stats_reset(self, mask=None) -> None:
        """softrod_episode_stats_reset: zero the accumulators, the latch and the info rows of the envs with mask != 0
        (None: all); the ring, `finished` and `count` stay.  `mask`: anything (n_envs,), uploaded once unless it is a
        uint8 / bool tensor on this device."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device)
            if m.dtype not in (torch.uint8, torch.bool):
                m = m != 0
            m = m.reshape(self.n_envs).contiguous()
        check(self._lib.softrod_episode_stats_reset(self._h, m.data_ptr() if m is not None else None, self._stream()),
              self._h)

    # -- observation / reward normalisation (softrod_normalize_enable / _step / _reset / _view / _load) ----------
    normalize: Optional[Dict[str, torch.Tensor]] = None     # the resident arrays while the feature is on
    normalize_obs_on = normalize_reward_on = False
    normalize_mode = _capi.NORMALIZE_MANUAL                 # what step() passes as `mode`
    normalize_in_step = True            # False: the caller runs normalize_step itself (the host-driven NEXT_STEP loop)
    normalize_update = True             # False: evaluation, step() and reset passes leave the statistics alone

    def normalize_enable(self, obs: bool = True, reward: bool = True, *, gamma: float = 0.99, clip_obs: float = 10.0,
                         clip_reward: float = 10.0, epsilon: float = 1e-8, mode: Optional[int] = None,
                         in_step: bool = True) -> None:
        """softrod_normalize_enable: allocates (or allocates anew) the running statistics — Gymnasium's RunningMeanStd
        per observation column and one for the discounted return — and the output buffers; obs = reward = False
        switches the feature off and frees them.  While it is on `normalize` holds zero-copy device views of every array
        (_capi.NORMALIZE_ARRAYS) — new ones after every call — and, with `in_step`, step() runs normalize_step behind
        softrod_step (and behind the episode statistics, which keep reading the raw reward) on its own obs / reward /
        flags, `final_obs` in SAME_STEP mode, `mode` (None: SAME_STEP on a same-step handle, NEXT_STEP with device
        auto-reset, else MANUAL) and `normalize_update`.  A loop that composes its rows on the host after the step
        (host-driven NEXT_STEP) passes in_step=False and calls normalize_step itself.  While it is off step() does
        one attribute test and nothing else.  A captured graph must be captured again after the call."""
        check(self._lib.softrod_normalize_enable(self._h, int(bool(obs)), int(bool(reward)), float(gamma), float(clip_obs),
                                                 float(clip_reward), float(epsilon)), self._h)
        self.normalize = None
        self.normalize_obs_on, self.normalize_reward_on = bool(obs), bool(reward)
        if not (obs or reward):
            return
        v = _capi.SoftrodNormalizeView()
        check(self._lib.softrod_normalize_view(self._h, C.byref(v)), self._h)
        size = {"n": (self.n_envs,), "d": (self.obs_dim,), "nd": (self.n_envs, self.obs_dim), "1": (1,)}
        if mode is None:
            mode = (_capi.NORMALIZE_SAME_STEP if getattr(self, "same_step", False)
                    else _capi.NORMALIZE_NEXT_STEP if getattr(self, "queue_depth", 0) else _capi.NORMALIZE_MANUAL)
        self.normalize_mode = int(mode)
        self.normalize_in_step = bool(in_step)
        self.normalize = {name: torch.as_tensor(_DevArray(getattr(v, name), size[per], typestr, self), device=self.device)
                          for name, typestr, per in _capi.NORMALIZE_ARRAYS}

    def normalize_step(self, obs, reward, terminated, truncated, final_obs=None, mode: Optional[int] = None,
                       update: Optional[bool] = None) -> None:
        """softrod_normalize_step: one pass from contiguous device tensors obs f32 (n_envs, obs_dim), reward f64
        (n_envs,), terminated / truncated uint8 or bool (n_envs,), final_obs f32 (n_envs, obs_dim) or None (mode 2
        only); mode 0 manual, 1 NEXT_STEP, 2 SAME_STEP (None: normalize_mode); update False freezes the statistics
        (None: normalize_update).  At most two kernels on the current stream; capturable.  The results are in
        `normalize`: norm_obs, norm_final_obs, norm_reward.  step() calls it itself while normalize_in_step."""
        ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
        check(self._lib.softrod_normalize_step(
            self._h, ptr(obs), ptr(reward), ptr(terminated), ptr(truncated), ptr(final_obs),
            int(self.normalize_mode if mode is None else mode),
            int(bool(self.normalize_update if update is None else update)), self._stream()), self._h)

    def normalize_reset(self, obs, mask=None, update: Optional[bool] = None) -> None:
        """softrod_normalize_reset: the pass over a reset observation obs f32 (n_envs, obs_dim): the rows of the envs with
        mask != 0 (None: all) are counted unless the statistics are frozen, their discounted return and latch become
        zero, and every row of norm_obs is written.  `mask`: anything (n_envs,), uploaded once unless it is a uint8 /
        bool tensor on this device."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device)
            if m.dtype not in (torch.uint8, torch.bool):
                m = m != 0
            m = m.reshape(self.n_envs).contiguous()
        check(self._lib.softrod_normalize_reset(
            self._h, obs.data_ptr() if obs is not None else None, m.data_ptr() if m is not None else None,
            int(bool(self.normalize_update if update is None else update)), self._stream()), self._h)

    def normalize_load(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count) -> None:
        """softrod_normalize_load: set the records from host values (obs_* (obs_dim,) float64, ret_* scalars); inv_std is
        recomputed.  Waits for the stream."""
        o = [np.ascontiguousarray(v, dtype=np.float64).reshape(self.obs_dim) for v in (obs_mean, obs_var, obs_count)]
        r = [np.ascontiguousarray(v, dtype=np.float64).reshape(1) for v in (ret_mean, ret_var, ret_count)]
        check(self._lib.softrod_normalize_load(self._h, *(a.ctypes.data for a in o + r), self._stream()), self._h)

    supports_early_termination = True    # softrod_config.early_termination runs in the step kernels' epilogue

    def _readout(self, entry: str, rods: int, *tail: int, args: tuple = ()) -> torch.Tensor:
        """One per-rod read-out softrod_<entry>: its (n_envs, rods, *tail) float64 device buffer, allocated on first
        use and filled by the call.  `args`: what the entry point takes between the handle and the buffer."""
        buf = self._readouts.get(entry)
        if buf is None:
            buf = self._readouts[entry] = torch.empty((self.n_envs, rods, *tail), dtype=torch.float64, device=self.device)
        check(getattr(self._lib, "softrod_" + entry)(self._h, *args, buf.data_ptr(), self._stream()), self._h)
        return buf

    def rod_energies(self) -> torch.Tensor:
        """softrod_rod_energies: (n_envs, rods_per_env, 4) float64 device tensor — translational, rotational,
        bending, shear energy of every rod at PyElastica's instant (the mid-substep strains of the last force
        evaluation with the end-of-step rates; the state itself right after a reset).  Overwritten by the next call."""
        return self._readout("rod_energies", _capi.config_rods_per_env(self.cfg), 4)

    def ground_reaction(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """softrod_ground_reaction: (force, torque) float64 device tensors — force (n_envs, rods_per_env, 3, n_elem + 1),
        the lab-frame force RodPlaneContactWithAnisotropicFriction adds to every node; torque (n_envs, rods_per_env, 3,
        n_elem), the material-frame torque it adds to every element — from ONE fresh force evaluation at the resident
        state (not the value the last substep applied: include/softrod.h).  Views of one buffer allocated on first
        use and overwritten by the next call."""
        rods = int(self.cfg.n_arm) if int(self.cfg.env_kind) == _capi.ENV_OCTO_FLAT else 1
        out = self._readout("ground_reaction", rods, 6, int(self.cfg.n_elem) + 1)
        return out[:, :, :3], out[:, :, 3:, :-1]

    def rod_strains(self) -> RodStrains:
        """softrod_rod_strains: RodStrains(sigma, kappa, dilatation, voronoi_dilatation, internal_force,
        internal_couple) of float64 device tensors — (n_envs, rods_per_env, 3, n_elem), (.., 3, n_elem - 1),
        (.., n_elem), (.., n_elem - 1), (.., 3, n_elem), (.., 3, n_elem - 1) — RodCallBack's strain fields and the
        passive elastic loads S sigma, B (kappa - rest_kappa), at the instant of rod_energies() (include/softrod.h).
        Views of one (n_envs, rods_per_env, 14, n_elem) buffer allocated on first use and overwritten by the next
        call."""
        rods = _capi.config_rods_per_env(self.cfg)
        return rod_strains_views(self._readout("rod_strains", rods, 14, int(self.cfg.n_elem)))

    def muscle_loads(self) -> MuscleLoads:
        """softrod_muscle_loads: MuscleLoads(layer_force, layer_length, internal_force, internal_couple,
        external_force, external_couple) of float64 device tensors — (n_envs, rods_per_env, 4, n_elem), (.., 4, n_elem),
        (.., 3, n_elem), (.., 3, n_elem - 1), (.., 3, n_elem + 1), (.., 3, n_elem) — what ApplyMuscles computes from the
        resident activation rows at the instant of rod_strains() (include/softrod.h).  Views of one (n_envs,
        rods_per_env, 20, n_elem + 1) buffer allocated on first use and overwritten by the next call."""
        rods = _capi.config_rods_per_env(self.cfg)
        return muscle_loads_views(self._readout("muscle_loads", rods, 20, int(self.cfg.n_elem) + 1))

    def joint_loads(self) -> JointLoads:
        """softrod_joint_loads: JointLoads(body_force, body_torque, arm_force, arm_torque, gap, gap_length, net_force,
        net_torque, acceleration, angular_acceleration) of float64 device tensors — (n_envs, rods_per_env, 3) five
        times, (n_envs, rods_per_env), (n_envs, 3) four times — what FixedJoint2Rigid exchanges between every arm and
        the rigid body, and the body's net load and accelerations, from ONE evaluation at the resident state (not the
        value the last substep applied: include/softrod.h).  Views of one (n_envs, rods_per_env + 1, 16) buffer
        allocated on first use and overwritten by the next call."""
        rods = _capi.config_rods_per_env(self.cfg)
        return joint_loads_views(self._readout("joint_loads", rods + 1, 16))

    def rod_dynamics(self) -> RodDynamics:
        """softrod_rod_dynamics: RodDynamics(internal_force, internal_torque, external_force, external_torque,
        acceleration, angular_acceleration) of float64 device tensors — (n_envs, rods_per_env, 3, n_elem + 1) for the
        three nodal fields (lab frame), (n_envs, rods_per_env, 3, n_elem) for the three per-element ones (material
        frame) — every load the substep's force evaluation applies and the accelerations they give, from ONE
        evaluation at the resident state (not the value the last substep applied: include/softrod.h).  Views of one
        (n_envs, rods_per_env, 18, n_elem + 1) buffer allocated on first use and overwritten by the next call."""
        rods = _capi.config_rods_per_env(self.cfg)
        return rod_dynamics_views(self._readout("rod_dynamics", rods, 18, int(self.cfg.n_elem) + 1))

    def rod_clearance(self, self_gap: Optional[int] = None) -> RodClearance:
        """softrod_rod_clearance: RodClearance(gap, distance, element, point, target_gap, target_distance,
        target_element, target_point) of float64 device tensors — (n_envs, rods_per_env, rods_per_env) twice,
        (n_envs, rods_per_env, rods_per_env, 2) twice, (n_envs, rods_per_env) four times (None for an env kind without
        a target) — the least capsule gap between every two rods, within every rod (element pairs at least `self_gap`
        apart) and from every rod to the env's target (include/softrod.h).  self_gap None:
        _capi.rod_clearance_self_gap of the rest element length and the radii this handle was built with (the radius
        profile if one was set, else base_radius).  Views of one (n_envs, rods_per_env, rods_per_env + 1, 6) buffer
        allocated on first use and overwritten by the next call."""
        rods, n = _capi.config_rods_per_env(self.cfg), int(self.cfg.n_elem)
        if self_gap is None:
            prof = self._tables.get("radius_profile")
            radii = float(self.cfg.base_radius) if prof is None else np.frombuffer(prof, np.float64)
            self_gap = _capi.rod_clearance_self_gap(float(self.cfg.base_length) / n, radii)
        buf = self._readout("rod_clearance", rods, rods + 1, 6, args=(int(self_gap),))
        return rod_clearance_views(buf, int(self.cfg.env_kind) in _capi.TARGET_ENVS)

    def render(self, camera: "_capi.SoftrodCamera", depth: bool = False):
        """softrod_render: one (n_envs, H, W, 3) uint8 device tensor of RGB frames of every env through `camera`
        (an orthographic _capi.SoftrodCamera shared by the batch; _capi.camera_default(cfg) frames a fresh env), or
        (rgb, depth) with depth (n_envs, H, W) float32 — the surface's camera-frame depth, -inf where nothing is
        drawn — when `depth` is true.  The image model is include/softrod.h's.  One kernel on the current stream, no
        upload, capturable once the buffers exist: they are allocated on first use per (H, W) and overwritten by
        the next call, like the read-outs'."""
        h, w = int(camera.height), int(camera.width)
        key = (h, w)
        rgb = self._frames.get(key)
        if rgb is None:
            check(self._lib.softrod_camera_check(C.byref(camera)))      # before sizes from it are trusted
            rgb = self._frames[key] = torch.empty((self.n_envs, h, w, 3), dtype=torch.uint8, device=self.device)
        z = None
        if depth:
            z = self._frames.get(key + ("depth",))
            if z is None:
                z = self._frames[key + ("depth",)] = torch.empty((self.n_envs, h, w), dtype=torch.float32, device=self.device)
        check(self._lib.softrod_render(self._h, C.byref(camera), rgb.data_ptr(), z.data_ptr() if depth else None,
                                       self._stream()), self._h)
        return (rgb, z) if depth else rgb

    def time_limit(self) -> torch.Tensor:
        """early_termination handles: the last step's time-limit flag per env (row 0 of softrod_state_view.env_aux)
        as a bool device tensor — info["TimeLimit.truncated"], which `truncated` no longer is."""
        return self.state()["env_aux"][0] != 0.0

    def step_packed(self, actions, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """softrod_step_packed: (n_envs, packed_width(obs_dim)) float32 words per env, into
        `out` if given (the overlapped multi-GPU path alternates two buffers).  NotImplementedError while episode
        statistics or normalisation are on: the packed row keeps reward and flags as float32 words, not the buffers
        those passes read."""
        from .distributed import packed_width

        if self.episode_stats is not None:
            raise NotImplementedError("step_packed with episode statistics on (episode_stats_enable(0) switches them off)")
        if self.normalize is not None:
            raise NotImplementedError("step_packed with normalisation on (normalize_enable(False, False) switches it off)")
        a = self._actions(actions)
        if out is None:
            if getattr(self, "packed", None) is None:
                self.packed = torch.empty((self.n_envs, packed_width(self.obs_dim)), dtype=torch.float32,
                                          device=self.device)
            out = self.packed
        check(
            self._lib.softrod_step_packed(
                self._h, a.data_ptr(), out.data_ptr(),
                self.aux.data_ptr() if self.aux is not None else None, self._stream(),
            ),
            self._h,
        )
        return out

    def scatter_rows(self, packed: torch.Tensor, peer_ptrs, first_row: int, tag_word: int = -1, tag: int = 0) -> None:
        """softrod_scatter_rows: this batch's packed rows into rows first_row.. of every buffer in
        `peer_ptrs` (device pointers: the ranks' exchange buffers), one small kernel on the current
        stream; tag_word >= 0: word `tag_word` of every buffer receives `tag` once all rows have landed."""
        tab = np.ascontiguousarray(peer_ptrs, dtype=np.uint64)
        check(
            self._lib.softrod_scatter_rows(
                self._h, packed.data_ptr(), tab.ctypes.data, int(tab.size), int(packed.shape[1]), int(first_row),
                int(tag_word), int(tag) & 0xFFFFFFFF, self._stream(),
            ),
            self._h,
        )

    # -- exchange buffers of ShardedVecEnv(transport="p2p") (softrod_exchange_*) ------------------
    def exchange_alloc(self, n_words: int):
        """Uncached device memory the other GPUs may store into: (tensor float32[n_words] — a
        zero-copy view —, device pointer, 64-byte IPC handle, memory kind)."""
        ptr, kind = C.c_void_p(), C.c_int()
        handle = (C.c_uint8 * 64)()
        check(self._lib.softrod_exchange_alloc(self.device_index, int(n_words) * 4, C.byref(ptr), handle, C.byref(kind)))
        t = torch.as_tensor(_DevArray(ptr.value, (int(n_words),), "<f4", self), device=self.device)
        return t, int(ptr.value), bytes(handle), {1: "uncached", 2: "fine-grained"}[int(kind.value)]

    def exchange_open(self, handle: bytes, owner_device: int) -> int:
        """Map a peer process's exchange buffer; -> the device pointer valid in this process."""
        ptr = C.c_void_p()
        buf = (C.c_uint8 * 64).from_buffer_copy(handle)
        check(self._lib.softrod_exchange_open(self.device_index, buf, int(owner_device), C.byref(ptr)))
        return int(ptr.value)

    def exchange_close(self, ptr: int) -> None:
        check(self._lib.softrod_exchange_close(self.device_index, C.c_void_p(ptr)))

    def exchange_free(self, ptr: int) -> None:
        check(self._lib.softrod_exchange_free(self.device_index, C.c_void_p(ptr)))

    def substeps(self, actions, n: int) -> None:
        a = self._actions(actions) if actions is not None else None
        check(
            self._lib.softrod_substeps(
                self._h, a.data_ptr() if a is not None else None, int(n), self._stream()
            ),
            self._h,
        )

    def set_timing(self, n_launches: int) -> None:
        """Time the next `n_launches` steps with HIP events attached to their own kernel dispatches (0 = off)."""
        check(self._lib.softrod_set_timing(self._h, int(n_launches)), self._h)

    def kernel_times_ms(self) -> np.ndarray:
        """Durations of the launches timed since set_timing (synchronises)."""
        cap = 1 << 16
        out = np.zeros(cap, np.float32)
        cnt = C.c_int()
        check(self._lib.softrod_kernel_times_ms(self._h, out.ctypes.data, cap, C.byref(cnt)), self._h)
        return out[: cnt.value].copy()

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        check(self._lib.softrod_last_kernel_ms(self._h, C.byref(ms)), self._h)
        return float(ms.value)

    def prev_action_rows(self) -> torch.Tensor:
        """Writable (n_envs, action_dim) view of the resident `_prev_action`."""
        if getattr(self, "_prev_rows", None) is None:
            with self._views() as st:
                self._prev_rows = st["prev_action"]
            if not self.is_octo and not self.is_mocto:
                self._prev_rows = self._prev_rows[:, : self.action_dim]
        return self._prev_rows

    # -- planar certificates (softrod_set_planar_certificates; SoftPendulum-v0 under MATH_FAST, a no-op elsewhere) -----
    def set_planar_certificates(self, on: bool) -> None:
        """softrod_set_planar_certificates: let the SoftPendulum step kernels trust (and issue) per-env planar
        certificates instead of proving planarity at every launch (include/softrod.h).  Default on; state() switches
        them off for good, only this call switches them back on — do that only once nothing writes resident rows
        through a view any more.  Waits for the device; every env is proved again at its next step."""
        check(self._lib.softrod_set_planar_certificates(self._h, int(bool(on))), self._h)
        self._planar_cert_on = bool(on)

    def planar_certificates(self) -> torch.Tensor:
        """softrod_planar_certificates: (n_envs,) uint8 device copy of the certificates on the current stream — 0
        unknown, 1 / 2 certified planar with d2_z > 0 / < 0; all zero while they are off or the handle has none."""
        out = torch.empty((self.n_envs,), dtype=torch.uint8, device=self.device)
        check(self._lib.softrod_planar_certificates(self._h, C.c_void_p(out.data_ptr()), self._stream()), self._h)
        return out

    @contextlib.contextmanager
    def _views(self):
        """state() for this class's own use — reads and writes that are over (synchronised) when the block ends, or
        views it keeps of arrays no certificate vouches for (prev_action, time): planar certificates that were on are
        switched back on behind the block."""
        was_on = getattr(self, "_planar_cert_on", True)
        try:
            yield self.state()
        finally:
            if was_on:
                self.set_planar_certificates(True)

    def state(self) -> Dict[str, torch.Tensor]:
        """Zero-copy torch views of the resident SoA state (softrod_state_view).  The caller may write through them
        at any later time, so the call switches planar certificates off on this backend (set_planar_certificates)."""
        self._planar_cert_on = False
        v = SoftrodStateView()
        check(self._lib.softrod_state_view_get(self._h, C.byref(v)), self._h)
        n, s = self.n_envs, int(v.lane_stride)

        def view(ptr, comps):
            return torch.as_tensor(_DevArray(ptr, (comps, n, s), "<f8", self), device=self.device)

        extra = {}
        ns = n * (int(self.cfg.n_arm) if self.is_mocto else 1)      # SuckerControllers: per env, per arm of the muscle octopus
        if v.env_aux:
            extra["env_aux"] = torch.as_tensor(_DevArray(v.env_aux, (8, n), "<f8", self), device=self.device)
        if v.prev_kappa:
            extra["prev_kappa"] = torch.as_tensor(
                _DevArray(v.prev_kappa, (n, int(self.cfg.n_arm) * (int(self.cfg.n_elem) - 1)), "<f4", self), device=self.device)
        if v.muscle_activation:
            extra["muscle_activation"] = torch.as_tensor(
                _DevArray(v.muscle_activation, (_capi.MAX_MUSCLES, n, s), "<f8", self), device=self.device)
        return {
            **extra,
            "sucker_index": torch.as_tensor(_DevArray(v.sucker_index, (_capi.MAX_SUCKERS, ns), "<i4", self),
                                            device=self.device),
            "position": view(v.position, 3),
            "velocity": view(v.velocity, 3),
            "director": view(v.director, 9),
            "omega": view(v.omega, 3),
            "tangents": view(v.tangents, 3),
            "time": torch.as_tensor(_DevArray(v.time, (n,), "<f8", self), device=self.device),
            "control": torch.as_tensor(_DevArray(v.control, (4, n), "<f8", self), device=self.device),
            "kappa": view(v.kappa, 3),
            "rest_kappa": view(v.rest_kappa, 3),
            "env_memory": torch.as_tensor(_DevArray(v.env_memory, (n, s), "<f8", self), device=self.device),
            "prev_action": torch.as_tensor(_DevArray(v.prev_action, (n, max(7, self.action_dim)), "<f4", self),
                                           device=self.device),
            "head": torch.as_tensor(_DevArray(v.head, (20, n), "<f8", self), device=self.device),
            "bc_targets": torch.as_tensor(_DevArray(v.bc_targets, (12, n), "<f8", self), device=self.device),
            "sucker_ratio": torch.as_tensor(_DevArray(v.sucker_ratio, (_capi.MAX_SUCKERS, ns), "<f8", self),
                                            device=self.device),
            "arm_stride": int(v.arm_stride),
        }

    _SNAPSHOT_KEYS = ("position", "velocity", "director", "omega", "tangents", "time", "control", "kappa",
                      "rest_kappa", "env_memory", "prev_action", "head", "bc_targets", "sucker_ratio", "sucker_index")

    def _snapshot_keys(self):
        return (self._SNAPSHOT_KEYS + (("muscle_activation",) if self.cfg.features & _capi.FEAT_COOMM_MUSCLES else ())
                + (("env_aux", "prev_kappa") if self.is_mocto else ()))

    def config_fingerprint(self) -> bytes:
        """What a snapshot is only valid for: the ABI, every field of softrod_config except the
        batch size (checked through the shapes), and a digest of the per-handle tables that hold
        physics outside the config — the radius profile of a tapered rod (masses, stiffnesses,
        damping per lane), the spline table and the action basis.  A snapshot taken under another
        dt, substep count, feature set, material or taper continues with the wrong physics
        otherwise."""
        import hashlib

        c = self.cfg.copy()
        c.n_envs = 0
        d = hashlib.sha256()
        for k in sorted(self._tables):
            d.update(k.encode() + b"\0" + self._tables[k])
        return bytes([_capi.ABI_VERSION]) + bytes(memoryview(c).cast("B")) + d.digest()

    def snapshot(self) -> Dict[str, torch.Tensor]:
        """Host copy of the whole resident batch (every array of softrod_state_view): what
        `restore` needs to put the batch back exactly — checkpoint / resume, or branching a
        rollout.  The reference has no counterpart (its env state is never serialised).  While a pool of reset shapes
        is set (set_reset_shapes) the snapshot also carries reset_shape_index and reset_shape_episode; the pool itself
        is NOT part of a snapshot: set it again before restoring into another backend."""
        if getattr(self, "queue_depth", 0):
            raise _capi.SoftrodError("snapshot/restore of a handle with device-side auto-reset is not supported: "
                                     "the pending-reset flags and the staged queue are not part of the state view")
        with self._views() as st:
            torch.cuda.synchronize(self.device)
            snap = {k: st[k].cpu().clone() for k in self._snapshot_keys()}
        if getattr(self, "_env_material", None) is not None:        # per-env material (set_env_material)
            snap["env_material"] = torch.from_numpy(self._env_material.copy())
        if getattr(self, "_env_contact", None) is not None:         # per-env contact (set_env_contact)
            snap["env_contact"] = torch.from_numpy(self._env_contact.copy())
        if self.reset_shapes_count:        # shaped starts: the two per-env rows; the pool itself is not part of a snapshot
            snap["reset_shape_index"] = self.reset_shape_index.cpu().clone()
            snap["reset_shape_episode"] = self.reset_shape_episode.cpu().clone()
        snap["config_fingerprint"] = torch.frombuffer(bytearray(self.config_fingerprint()), dtype=torch.uint8).clone()
        return snap

    def restore(self, snap: Dict[str, torch.Tensor]) -> None:
        if getattr(self, "queue_depth", 0):
            raise _capi.SoftrodError("snapshot/restore of a handle with device-side auto-reset is not supported: "
                                     "stale needs_reset / skip flags would reset or skip the wrong envs")
        fp = snap.get("config_fingerprint")
        if fp is None or bytes(fp.numpy().tobytes()) != self.config_fingerprint():
            raise ValueError("snapshot was taken under a different softrod_config / ABI version / table set "
                             "(dt, n_substeps, features, env_kind, material, radius profile, spline table, "
                             "action basis ...): refusing to load it")
        with self._views() as st:       # (switching certificates back on waits for these copies and withdraws every one)
            for k in self._snapshot_keys():
                if tuple(snap[k].shape) != tuple(st[k].shape):
                    raise ValueError(f"snapshot field {k!r} has shape {tuple(snap[k].shape)}, expected {tuple(st[k].shape)}")
            for k in self._snapshot_keys():
                st[k].copy_(snap[k].to(self.device))
        # the material the snapshot was taken under; no key: the config's own values
        if "env_material" in snap:
            self.set_env_material(snap["env_material"].numpy())
        elif getattr(self, "_env_material", None) is not None:
            self.set_env_material(np.tile(_capi.env_material_defaults(self.cfg), (self.n_envs, 1)))
        # shaped starts: the rows travel when both sides have a pool (set the pool again before restoring into a fresh backend)
        if self.reset_shapes_count and "reset_shape_index" in snap:
            self.reset_shape_index.copy_(snap["reset_shape_index"].to(self.device))
            self.reset_shape_episode.copy_(snap["reset_shape_episode"].to(self.device))
        # the same for per-env contact
        if "env_contact" in snap:
            self.set_env_contact(snap["env_contact"].numpy())
        elif getattr(self, "_env_contact", None) is not None:
            self.set_env_contact(np.tile(_capi.env_contact_defaults(self.cfg), (self.n_envs, 1)))
        torch.cuda.synchronize(self.device)

    def rod_snapshot(self, env_indices) -> Dict[str, np.ndarray]:
        """Host copy of a few rods only (diagnostic taps): x, v (k,3,n+1); Q (k,3,3,n);
        w (k,3,n); time (k,).  One small device->host copy per field."""
        idx = torch.as_tensor(list(env_indices), dtype=torch.long, device=self.device)
        ne = int(self.cfg.n_elem)
        with self._views() as st:
            def rows(name, width):
                return st[name].index_select(1, idx)[:, :, :width].permute(1, 0, 2).cpu().numpy()

            return {
                "x": rows("position", ne + 1), "v": rows("velocity", ne + 1), "w": rows("omega", ne),
                "Q": rows("director", ne).reshape(len(env_indices), 3, 3, ne),
                "time": st["time"].index_select(0, idx).cpu().numpy(),
            }

    def kernel_tier(self) -> str:
        """softrod_kernel_tier: which step kernel this batch runs (follows from the config alone; the
        A/B switches in the environment count only under SOFTROD_DEBUG_SWITCHES=1)."""
        return self._lib.softrod_kernel_tier(self._h).decode()

    def octo_state_numpy(self) -> Dict[str, np.ndarray]:
        """Host copy of an OctoFlat batch: arms as x,v (N,A,3,n+1), Q (N,A,3,3,n), w (N,A,3,n),
        kappa/rest_kappa (N,A,3,n-1); head as x,v,w (N,3), Q (N,3,3); target (N,2); time (N,)."""
        st = self.state()
        ne, na, seg = int(self.cfg.n_elem), int(self.cfg.n_arm), int(st["arm_stride"])
        torch.cuda.synchronize(self.device)

        def arms(t, comps, width):
            a = t[:, :, : na * seg].reshape(comps, self.n_envs, na, seg)[..., :width]
            return a.permute(1, 2, 0, 3).cpu().numpy()

        hd = st["head"].cpu().numpy()
        return {
            "x": arms(st["position"], 3, ne + 1),
            "v": arms(st["velocity"], 3, ne + 1),
            "w": arms(st["omega"], 3, ne),
            "Q": arms(st["director"], 9, ne).reshape(self.n_envs, na, 3, 3, ne),
            "kappa": arms(st["kappa"], 3, ne - 1),
            "rest_kappa": arms(st["rest_kappa"], 3, ne - 1),
            "head_x": hd[0:3].T.copy(), "head_v": hd[3:6].T.copy(),
            "head_Q": hd[6:15].T.reshape(self.n_envs, 3, 3).copy(), "head_w": hd[15:18].T.copy(),
            "target": hd[18:20].T.copy(),
            "time": st["time"].cpu().numpy(),
        }

    def state_numpy(self) -> Dict[str, np.ndarray]:
        """Host copy in the reference's per-rod shapes: x,v (N,3,n+1); Q (N,3,3,n); w (N,3,n)."""
        ne = int(self.cfg.n_elem)
        with self._views() as st:
            torch.cuda.synchronize(self.device)
            out = {
                "x": st["position"][:, :, : ne + 1].permute(1, 0, 2).cpu().numpy(),
                "v": st["velocity"][:, :, : ne + 1].permute(1, 0, 2).cpu().numpy(),
                "w": st["omega"][:, :, :ne].permute(1, 0, 2).cpu().numpy(),
                "tangents": st["tangents"][:, :, :ne].permute(1, 0, 2).cpu().numpy(),
                "time": st["time"].cpu().numpy(),
                "control": st["control"].permute(1, 0).cpu().numpy(),
                "kappa": st["kappa"][:, :, : ne - 1].permute(1, 0, 2).cpu().numpy(),
                "rest_kappa": st["rest_kappa"][:, :, : ne - 1].permute(1, 0, 2).cpu().numpy(),
            }
            q = st["director"][:, :, :ne].permute(1, 0, 2).cpu().numpy()
        out["Q"] = q.reshape(self.n_envs, 3, 3, ne)
        return out
