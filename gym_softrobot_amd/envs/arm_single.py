"""OctoArmSingle-v0 on the MI355X batched Cosserat-rod stepper.

Mirrors gym_softrobot/envs/octopus/arm_single_env.py:41-316 and build_arm
(gym_softrobot/envs/octopus/build.py:220-292): one arm lying on a frictional plane,
actuated by its rest curvature (7 cubic-spline knots), reaching for a target with its
centre of mass.  GravityForces, RodPlaneContactWithAnisotropicFriction and
AnalyticalLinearDamper are compiled-in features (SOFTROD_FEATURES_ARM_SINGLE); the
cubic `interp1d` of `set_action` is a constant basis matrix applied in the kernel
prologue.  `n_elems` other than 50 generalise the reference's hard-coded 7x7 binning of
the curvature observation (:193-194) to np.array_split-style bins.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import _capi
from ..spaces import Box
from .base import SingleEnvContact, SingleEnvMaterial, SingleEnvSummary, SingleRodEnv, VecRodEnvBase


class VecArmSingleEnv(VecRodEnvBase):
    """N parallel OctoArmSingle-v0 envs resident on one GPU (see VecRodEnvBase)."""

    metadata = {"render_modes": ["rgb_array", "human"], "render_fps": 20}
    action_low, action_high = -22.0, 22.0             # arm_single_env.py:84-90

    def __init__(
        self,
        num_envs: int,
        final_time: float = 10.0,
        time_step: float = 7.0e-5,
        recording_fps: int = 20,
        n_elems: int = 50,
        n_action: int = 7,
        control_penalty_coeff: float = 0.001,
        config_generate_video: bool = False,
        policy_mode: str = "centralized",
        render_mode: Optional[str] = None,
        *,
        device: int = 0,
        math_mode: int = _capi.MATH_FAST,
        numpy_output: bool = False,
        autoreset: bool = False,
        backend=None,
        radius_profile=None,
    ):
        """`radius_profile` (extension, n_elems radii): a TAPERED arm, as the reference's muscle arms
        are built (`CosseratRod.straight_rod(base_radius=<array>)`, octopus/arm_push_env.py:160-179);
        None = the uniform arm of build_arm."""
        if n_action != 7:
            raise NotImplementedError("the observation layout of the reference fixes n_action = 7")
        cfg = _capi.arm_single_config(
            num_envs, final_time=final_time, time_step=time_step, recording_fps=recording_fps,
            n_elems=n_elems, control_penalty_coeff=control_penalty_coeff, math_mode=math_mode,
        )
        super().__init__(num_envs, cfg, render_mode=render_mode,
                         config_generate_video=config_generate_video, device=device,
                         numpy_output=numpy_output, autoreset=autoreset, backend=backend)
        self._set_timing(final_time, time_step, recording_fps)
        self.control_penalty_coeff = control_penalty_coeff
        self.n_elems = n_elems
        self.n_seg = n_elems - 1
        self.policy_mode = policy_mode
        if radius_profile is not None:
            self.backend.set_radius_profile(np.asarray(radius_profile, np.float64))

    def _draw_reset(self, i):
        return None                                   # build_arm draws nothing from the RNG

    def _queue_from_draws(self, draws, counts):
        n, m = self.num_envs, max(1, int(counts.max()))
        start = np.zeros((n, m, 3))
        direction = np.tile(np.array([1.0, 0.0, 0.0]), (n, m, 1))
        normal = np.tile(np.array([0.0, 0.0, 1.0]), (n, m, 1))
        self.backend.queue_push_straight(start, direction, normal, counts)

    def _reset_backend(self, mask, use_mask, draws=None):
        # build_arm draws nothing from the RNG: every reset starts from the same straight arm
        n = self.num_envs
        start = np.zeros((n, 3))
        direction = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1))   # octopus/build.py:236-238
        normal = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
        self.backend.reset_straight(start, direction, normal, mask.astype(np.uint8) if use_mask else None)


class ArmSingleEnv(SingleEnvMaterial, SingleEnvContact, SingleEnvSummary, SingleRodEnv):
    """Drop-in for gym_softrobot's ArmSingleEnv (octopus/arm_single_env.py:41-316), N = 1; get_state :186-224,
    summary :116-133."""

    metadata = {"render_modes": ["rgb_array", "human"], "render_fps": 20}
    shares_rng = False                                # build_arm draws nothing from the RNG

    def __init__(
        self,
        final_time=10.0,
        time_step=7.0e-5,
        recording_fps=20,
        n_elems=50,
        n_action=7,
        control_penalty_coeff=0.001,
        config_generate_video=False,
        policy_mode="centralized",
        render_mode: Optional[str] = None,
        *,
        device: int = 0,
        math_mode: int = _capi.MATH_FAST,
        backend=None,
    ):
        super().__init__(render_mode, VecArmSingleEnv, final_time, time_step, recording_fps, n_elems, n_action,
                         control_penalty_coeff, config_generate_video, policy_mode, None, device=device,
                         math_mode=math_mode, backend=backend)
        self.control_penalty_coeff = control_penalty_coeff
        self.n_elems = n_elems
        self.n_seg = n_elems - 1
        self.policy_mode = policy_mode
        self.n_action = n_action
        self.action_space = Box(-22.0, 22.0, shape=(7,), dtype=np.float32)
        self.observation_space = Box(-np.inf, np.inf, shape=(25,), dtype=np.float32)
        self.reward_range = 10.0
        self.kappa_range = [-49.33508476187419, 49.33545827754751]
        self.kappa_rate_range = [-21.063520620377012, 24.664591289161944]
        self._target = np.array([1.0, 0.0])
