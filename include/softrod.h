/*
 * softrod.h — C-ABI of the MI355X-native batched Cosserat-rod stepper.
 *
 * This is the drop-in boundary for the ONE hot path of skim0119/gym-softrobot
 * that BASELINE.json names: `env.step()` of SoftPendulum-v0, i.e.
 *
 *     for _ in range(self.step_skip):
 *         self.time = self.do_step(self.simulator, self.time, self.time_step)
 *                                   (gym_softrobot/envs/soft_pendulum/soft_pendulum.py:183-184)
 *
 * where `do_step` is PyElastica's `PositionVerlet().step` (soft_pendulum.py:137-139)
 * applied to the simulator assembled by `build_soft_pendulum`
 * (gym_softrobot/envs/soft_pendulum/build.py:29-115), followed by the NaN check,
 * reward, truncation test and observation of soft_pendulum.py:196-251 — and for
 * the identical loops of the envs SURVEY.md §8 lists next to it
 * (soft_pendulum_3d.py:127-128, octopus/arm_single_env.py:247-248).
 *
 * The reference has no FFI for this path: its "operator API" is a set of Python
 * classes PyElastica calls back into once per substep (ConstraintBase /
 * NoForces subclasses, build.py:65-79,94-101) plus the registration DSL
 * (build.py:62,81-113).  Those per-substep Python callbacks ARE the bottleneck,
 * so this boundary replaces them with compiled-in, bit-selected features.  Each
 * entry point below cites the reference interface it stands in for.
 *
 * Conventions: every function returns 0 on success or a negative
 * SOFTROD_E* code and never throws; plain pointers and sizes only (no torch
 * types).  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Pointers documented "device" must be device-accessible; "host" must be host
 * memory.  One handle = one device; a handle is not re-entrant, independent
 * handles are thread-safe.
 *
 * The same declarations are implemented by the HIP library
 * (gym_softrobot_amd/csrc → libsoftrod_hip.so).  The CPU oracle
 * (oracle/softrod_oracle.c) shares only `softrod_config` and is test
 * infrastructure, not a fallback.
 */
#ifndef SOFTROD_H
#define SOFTROD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOFTROD_ABI_VERSION 17

/* error codes */
#define SOFTROD_OK 0
#define SOFTROD_EINVAL (-1)   /* bad argument / unsupported configuration   */
#define SOFTROD_ENOMEM (-2)   /* device or host allocation failed           */
#define SOFTROD_EHIP (-3)     /* a HIP runtime call failed (see last_error) */
#define SOFTROD_ENODEV (-4)   /* no usable gfx950 device                    */

/*
 * Feature bits: the compiled-in replacements of the reference's per-substep
 * Python hooks.  Order of application inside a substep is fixed to the order
 * PyElastica's PositionVerlet.step gives them (DESIGN.md "substep order").
 * File names below are relative to gym_softrobot/envs/.
 */
enum softrod_feature {
    /* GravityForces(acc_gravity)                  soft_pendulum/build.py:88-91 */
    SOFTROD_FEAT_GRAVITY = 1u << 0,
    /* PendulumPointForces.apply_forces: external_forces[0,0] = action
     * (ASSIGNS, after gravity was added)          soft_pendulum/build.py:94-105 */
    SOFTROD_FEAT_POINT_FORCE_NODE0_X = 1u << 1,
    /* PendulumBoundaryConditions                  soft_pendulum/build.py:65-85 */
    SOFTROD_FEAT_PENDULUM_BC = 1u << 2,
    /* AnalyticalLinearDamper(damping_constant, time_step)
     *                                             soft_pendulum/build.py:108-113 */
    SOFTROD_FEAT_ANALYTICAL_DAMPER = 1u << 3,
    /* PyElastica OneEndFixedBC on node 0 / element 0 (known-answer tests)      */
    SOFTROD_FEAT_FIXED_BC = 1u << 4,
    /* constant force on the last node, PyElastica EndpointForces with
     * start_force = 0 and no ramp (known-answer tests)                          */
    SOFTROD_FEAT_TIP_FORCE = 1u << 5,
    /* MovingBaseConstraint: node 0 pinned to the commanded base position,
     * element 0 director fixed, base velocity imposed
     *                                             soft_pendulum_3d/build.py:23-40 */
    SOFTROD_FEAT_MOVING_BASE_BC = 1u << 6,
    /* LaplaceDissipationFilter(filter_order)      soft_pendulum_3d/build.py:82-85 */
    SOFTROD_FEAT_LAPLACE_FILTER = 1u << 7,
    /* Plane + RodPlaneContactWithAnisotropicFriction(k, nu, slip_velocity_tol,
     * static_mu_array, kinetic_mu_array)          octopus/build.py:236-283    */
    SOFTROD_FEAT_PLANE_CONTACT_ANISO = 1u << 8,
    /* set_action: rest_kappa[0, :] = cubic interp1d of the action
     *                                             octopus/arm_single_env.py:226-235 */
    SOFTROD_FEAT_REST_KAPPA_ACTION = 1u << 9,
    /* OctoFlat: n_arm rods per env joined to a rigid Cylinder head by
     * FixedJoint2Rigid, head held by BodyBoundaryCondition
     *   octopus/build.py:52-132, utils/custom_elastica/joint.py:20-225,
     *   utils/custom_elastica/constraint.py:8-85                               */
    SOFTROD_FEAT_OCTO_HEAD = 1u << 10,
    /* two MuscleTorquesWithVaryingBetaSplines ("normal", "binormal"): control points from the
     * action, rate-limited, a cubic interpolating spline through them evaluated at the
     * cumulative element lengths whenever the points changed, added to external_torques
     *   soft_arm/soft_arm_tracking.py:352-383,
     *   utils/custom_elastica/muscle_torque/muscle_torques_with_bspline.py:128-225       */
    SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES = 1u << 11,
    /* ControllableFixConstraint ("sucker"): constrain_rates scales the velocity of node `index`
     * and the angular velocity of element `index` by (1 - reduction_ratio) while the
     * SuckerController's flag is on; constrain_values is a no-op
     *   octopus/controllable_constraint.py:24-69; registered at octopus/arm_push_env.py:188-195,
     *   587-595, arm_two_env.py:137-152 (several per arm, ratio set from the action :228),
     *   crawl_env.py:148-161.  Up to SOFTROD_MAX_SUCKERS per rod (softrod_config.sucker_index);
     *   the per-env effective ratio lives in softrod_state_view.sucker_ratio.                */
    SOFTROD_FEAT_SUCKER_CONSTRAINT = 1u << 12,
    /* ApplyMuscles(muscles=[LongitudinalMuscle, ..., TransverseMuscle]) of COOMM, registered as a forcing at
     *   octopus/arm_push_env.py:197-212,596-604, build_muscle_octopus.py:160-172,270-282 with the layers of
     *   create_es_muscle_layers (octopus/build.py:295-338).
     * COOMM (git pin uv.lock:173-175, branch refactor-numba-hotloops) is NOT on disk and not installable:
     * what this bit computes restates the published model (Chang, Halder, Gribkova, Tekinalp, Naughton,
     * Gazzola, Mehta: "Energy-shaping control of a muscular octopus arm moving in three dimensions",
     * Proc. R. Soc. A 479:20220593, 2023, section 2(c)) in the operation order recalled from
     * coomm/actuations/muscles/muscle.py — PARITY UNPINNED.  Per substep, per muscle m, per element:
     *   x_m   = radius * ratio_position_m                  muscle position in the material frame
     *   nu_m  = (sigma + e_3) + average(kappa) x x_m       muscle strain; l_m = |nu_m|, t_m = nu_m / l_m
     *   F_m   = activation_m * strength_m * max(fl(l_m), 0)   strength = max_muscle_stress * rest_muscle_area
     *   f     = sum F_m t_m ;  c = sum x_m x (F_m t_m)     internal force / couple of the actuation
     * and the equivalent external loads  F_ext += D^h(Q^T f),  tau_ext += D^h(c_v) + A^h(kappa x c_v D^) +
     * (e Q t) x f l^  with c_v the element couples averaged onto the Voronoi vertices.  The force-length law
     * fl, the layer geometry and strengths are DATA (softrod_config.muscle_fl_coef, softrod_set_muscle_layers);
     * every other recalled detail is a named switch of softrod_config (muscle_*).  Activations live in
     * softrod_state_view.muscle_activation (apply_activation, arm_push_env.py:257-271).                       */
    SOFTROD_FEAT_COOMM_MUSCLES = 1u << 13,
};
#define SOFTROD_MAX_MUSCLES 4
#define SOFTROD_MUSCLE_LONGITUDINAL 0 /* l_m = |nu_m|                                             */
#define SOFTROD_MUSCLE_TRANSVERSE 1   /* on the axis; l_m follows softrod_config.muscle_tm_length_law */
#define SOFTROD_MAX_FL_COEF 8
/* arm_push_env.py:160-196: the damped tapered arm with one sucker and the three muscle layers */
#define SOFTROD_FEATURES_ARM_PUSH                                                 \
    (SOFTROD_FEAT_ANALYTICAL_DAMPER | SOFTROD_FEAT_SUCKER_CONSTRAINT | SOFTROD_FEAT_COOMM_MUSCLES)
/* arm_push_env.py:520-618: the same arm + Cylinder + BodyBoundaryCondition + FixedJoint2Rigid (n_arm = 1) */
#define SOFTROD_FEATURES_ARM_PULL_WEIGHT (SOFTROD_FEATURES_ARM_PUSH | SOFTROD_FEAT_OCTO_HEAD)

#define SOFTROD_FEATURES_SOFTPENDULUM                                             \
    (SOFTROD_FEAT_GRAVITY | SOFTROD_FEAT_POINT_FORCE_NODE0_X |                   \
     SOFTROD_FEAT_PENDULUM_BC | SOFTROD_FEAT_ANALYTICAL_DAMPER)
#define SOFTROD_FEATURES_SOFTPENDULUM3D                                           \
    (SOFTROD_FEAT_GRAVITY | SOFTROD_FEAT_MOVING_BASE_BC |                        \
     SOFTROD_FEAT_ANALYTICAL_DAMPER | SOFTROD_FEAT_LAPLACE_FILTER)
#define SOFTROD_FEATURES_ARM_SINGLE                                               \
    (SOFTROD_FEAT_GRAVITY | SOFTROD_FEAT_PLANE_CONTACT_ANISO |                   \
     SOFTROD_FEAT_ANALYTICAL_DAMPER | SOFTROD_FEAT_REST_KAPPA_ACTION)
#define SOFTROD_FEATURES_OCTO_FLAT                                                \
    (SOFTROD_FEATURES_ARM_SINGLE | SOFTROD_FEAT_OCTO_HEAD)
#define SOFTROD_FEATURES_SOFT_ARM                                                 \
    (SOFTROD_FEAT_FIXED_BC | SOFTROD_FEAT_ANALYTICAL_DAMPER |                    \
     SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES)

/* env_kind: which env's set_action / NaN check / reward / observation the step
 * kernel's prologue and epilogue implement.                                     */
#define SOFTROD_ENV_NONE 0           /* bare rod: softrod_substeps only            */
#define SOFTROD_ENV_SOFTPENDULUM 1   /* soft_pendulum/soft_pendulum.py:149-251     */
#define SOFTROD_ENV_SOFTPENDULUM3D 2 /* soft_pendulum_3d/soft_pendulum_3d.py:93-174 */
#define SOFTROD_ENV_ARM_SINGLE 3     /* octopus/arm_single_env.py:186-316           */
#define SOFTROD_ENV_OCTO_FLAT 4      /* octopus/flat_env.py:231-408                 */
#define SOFTROD_ENV_SOFT_ARM 5       /* soft_arm/soft_arm_tracking.py:160-259       */
#define SOFTROD_ENV_ARM_PUSH 6       /* octopus/arm_push_env.py:225-347 (OctoArmPush-v0 / -v1; parity unpinned: COOMM) */
#define SOFTROD_ENV_ARM_PULL_WEIGHT 7 /* octopus/arm_push_env.py:516-618 ArmPullWeightEnv (OctoArmPullWeight-v0): the same
                                        arm and step(), joined to a rigid Cylinder "weight" by FixedJoint2Rigid; with
                                        SOFTROD_FEATURES_ARM_PULL_WEIGHT (parity unpinned: COOMM)                     */
/* The muscle octopus (octopus/build_muscle_octopus.py): n_arm tapered 20-element arms with COOMM muscle layers joined to a
 * rigid head, SOFTROD_FEATURES_ARM_PULL_WEIGHT's feature set on several arms (parity unpinned: COOMM).  Their set_action /
 * get_state / step live in two small kernels either side of the step kernel (csrc/softrod_mocto.hpp). */
#define SOFTROD_ENV_CRAWL 8          /* octopus/crawl_env.py:175-318 CrawlEnv (OctoCrawl-v0): 8 arms, one sucker each      */
#define SOFTROD_ENV_ARM_TWO 9        /* octopus/arm_two_env.py:166-343 ArmTwoEnv (OctoArmTwo-v0): 2 arms, 3 suckers each   */
#define SOFTROD_ENV_REACH 10         /* octopus/reach_env.py:150-290 ReachEnv (OctoReach-v0): 8 arms, head held            */

/* math_mode (HIP library only; the oracle always uses libm). */
#define SOFTROD_MATH_LIBM 0 /* sqrt/sin/cos/acos/pow evaluated as written   */
#define SOFTROD_MATH_FAST 1 /* range-checked polynomial forms, no libm      */

/*
 * Everything that is identical for all rods of a batch.  Defaults are filled by
 * softrod_config_softpendulum() / softrod_config_softpendulum3d(); the
 * "PyElastica numerics" block holds the constants SURVEY.md App. A marks (?) so
 * that a session with pyelastica==1.0.0 importable can flip them without
 * touching a kernel.
 */
typedef struct softrod_config {
    uint32_t struct_size; /* = sizeof(softrod_config); ABI guard            */
    uint32_t features;    /* OR of softrod_feature                          */
    int32_t n_envs;       /* rods in this handle (batch shard)              */
    int32_t n_elem;       /* elements per rod (n_elems, soft_pendulum.py:64) */
    int32_t n_substeps;   /* step_skip = int(1/(fps*dt)), soft_pendulum.py:78 */
    int32_t math_mode;    /* SOFTROD_MATH_*                                 */
    int32_t env_kind;     /* SOFTROD_ENV_*                                  */
    int32_t filter_order; /* LaplaceDissipationFilter order                 */
    double dt;            /* time_step, soft_pendulum.py:62                 */
    double final_time;    /* soft_pendulum.py:61                            */
    /* straight_rod arguments, build.py:18-26,54-61 */
    double base_length;
    double base_radius;
    double density;
    double youngs_modulus;
    double shear_modulus; /* build.py passes none -> PyElastica default     */
    double gravity[3];    /* build.py:87-91                                 */
    double damping_constant; /* build.py:108                                */
    double tip_force[3];  /* SOFTROD_FEAT_TIP_FORCE only                    */
    /* SoftPendulum3D set_action, soft_pendulum_3d.py:57-58,99-113 */
    double base_step;     /* 1e-3 (applied in float32, as the reference)    */
    double base_limit;    /* 0.5                                            */
    /* PyElastica numerics (UNVERIFIED recollection) */
    double alpha_c;       /* 27/28 shear correction                         */
    double eps_length;    /* 1e-14 added to |dx|                            */
    double eps_rot_axis;  /* 1e-14 added to |w| before normalising the axis */
    double acos_shift;    /* 1e-10 subtracted inside arccos of _inv_rotate  */
    double eps_sin;       /* 1e-14 added inside sin of _inv_rotate          */
                          /* SOFTROD_MATH_FAST expands theta / sin(theta + eps_sin) to
                             first order in eps_sin: softrod_create refuses
                             acos_shift <= 0 or eps_sin > 1e-3 sqrt(2 acos_shift)
                             in that mode (SOFTROD_MATH_LIBM takes any values)  */
    int32_t time_two_half_adds; /* 1: t += dt/2 twice per substep; 0: += dt */
    int32_t damp_before_constrain; /* order inside PyElastica's constrain_rates
                                      operator group.  0 (default): registration
                                      order of the build function — constrain()
                                      before dampen() (build.py:81-113,
                                      soft_pendulum_3d/build.py:66-85), pyelastica
                                      1.0 OperatorGroupFIFO; 1: dampers first
                                      (mixin-__init__ order of pyelastica 0.3.x) */
    /* ---- OctoArmSingle-v0 (octopus/build.py:220-292, arm_single_env.py) ---- */
    int32_t contact_before_forcing; /* order inside synchronize(): 0 (default) =
                                       registration order, gravity then contact
                                       (octopus/build.py:236-283)              */
    int32_t damper_protocol;  /* AnalyticalLinearDamper: 0 (default) = the per-unit-mass protocol the bare
                                 `damping_constant=` keyword selects (build.py:108-113): v *= exp(-nu dt),
                                 omega *= exp(-nu dt m_elem J^-1)^dilatation; 1 = the uniform protocol
                                 (`uniform_damping_constant=`): exp(-nu dt) on every rate.  A switch for
                                 tools/sweep_switches.py like the ones above (was reserved1: same layout) */
    double plane_origin[3];   /* (0, 0, -r0)            octopus/build.py:244   */
    double plane_normal[3];   /* (0, 0, 1)              octopus/build.py:233   */
    double contact_k;         /* 1e2                    :241                    */
    double contact_nu;        /* 1e1                    :242                    */
    double slip_velocity_tol; /* 1e-8                   :245                    */
    double surface_tol;       /* PyElastica class default 1e-4                  */
    double kinetic_mu[3];     /* forward, backward, sideways   :248-256         */
    double static_mu[3];      /* 2 x kinetic                   :257             */
    double control_penalty_coeff; /* 0.001              arm_single_env.py:62    */
    double target[2];         /* (1, 0)                 arm_single_env.py:165   */
    double kappa_range[2];    /* arm_single_env.py:111                          */
    double kappa_rate_range[2]; /* :113                                         */
    /* ---- OctoFlat-v0 (octopus/build.py:30-132, flat_env.py:55-110) ---- */
    int32_t n_arm;            /* 8 rods per env (n_elem is per arm: 10)         */
    int32_t n_knots;          /* n_action per arm: 3 (flat_env.py:62)           */
    double head_radius;       /* 0.04                   octopus/build.py:38     */
    double head_density;      /* 700                    :39                     */
    double joint_k;           /* body_arm_k  1e6        :36                     */
    double joint_nu;          /* 1e-3                   :128                    */
    double joint_kt;          /* body_arm_kt 1e0        :37                     */
    /* ---- SoftArmTracking-v0 (soft_arm/soft_arm_tracking.py:107-158,261-383) ---- */
    int32_t n_ctrl;           /* number_of_control_points per direction: 4  :132 */
    int32_t n_spline_pieces;  /* polynomial pieces of the interpolant (3 for 4 + 2
                                 points, not-a-knot); see softrod_set_spline_table */
    double muscle_torque_scale; /* alpha = torque_scale * radius * E   :350        */
    double max_activation_rate; /* max_rate_of_change_of_activation: inf  :143     */
    double arm_target[3];     /* target_location (game_mode 1)          :147      */
    /* ---- ControllableFixConstraint (octopus/controllable_constraint.py:24-69) ---- */
    int32_t n_suckers;        /* constraints of this kind registered on the rod (0..4)      */
    int32_t sucker_index[4];  /* SuckerController.index of each (node AND element index)    */
    int32_t early_termination; /* ArmPushEnv(config_early_termination=True) (arm_push_env.py:310-313, 441-456):
                                 1 = every step ends with terminated = truncated = (H < 1e-7), survive reward -10,
                                 no forward reward and no _isnan_check; H = translational + rotational + shear +
                                 bending energy at the instant softrod_rod_energies describes.  0 or 1; 1 only
                                 with SOFTROD_ENV_ARM_PUSH / SOFTROD_ENV_ARM_PULL_WEIGHT.  The time-limit flag of
                                 the step (info["TimeLimit.truncated"], :325-329) then lands in row 0 of
                                 softrod_state_view.env_aux (was reserved2: same layout)                  */
    double sucker_reduction_ratio; /* initial reduction_ratio of every sucker (1.0, :11); the
                                 controllers are on after finalize (arm_push_env.py:222)  */
    /* ---- SOFTROD_FEAT_COOMM_MUSCLES (octopus/build.py:295-338; COOMM itself NOT on disk: every field below
     *      restates a recalled detail and is a switch for the day the muscle-env fixtures exist) ---- */
    int32_t n_muscles;        /* layers of create_es_muscle_layers: 3 (two longitudinal, one transverse)   */
    int32_t muscle_kind[4];   /* SOFTROD_MUSCLE_* of each layer                                            */
    int32_t muscle_fl_degree; /* degree of the force-length polynomial (3)                                 */
    int32_t muscle_equiv_load_form; /* internal load -> equivalent external load: 0 (default) = the physical form,
                                 F = D^h(Q^T f), tau = D^h(c) + A^h(kappa x c D^) + (e Q t) x f l^;
                                 1 = PyElastica's own internal-load form applied to (f, c): Q^T f / e, c / eps^3,
                                 (Q t) x f l^                                                               */
    int32_t muscle_position_current_radius; /* 1 (default): x_m = rod.radius * ratio, the CURRENT (volume-preserving)
                                 radius; 0: the rest radius                                               */
    int32_t muscle_tm_length_law; /* TransverseMuscle's normalised length: 0 (default) = 1 / sqrt(|nu_m|)
                                 (incompressible cross-section: the radial fibre shortens as the arm extends);
                                 1 = |nu_m| like a longitudinal muscle                                      */
    int32_t arm_push_mode;    /* ArmPushEnv(mode=...): 0 "discrete" (OctoArmPush-v0), 1 "continuous" (-v1)
                                 arm_push_env.py:90-130                                                    */
    int32_t head_fixed;       /* 1: the rigid body ALSO carries OneEndFixedBC (reach_env.py:126-130): position, directors
                                 held at their initial values, velocities at zero — the head does not move          */
    double muscle_fl_coef[8]; /* fl(l) = sum_k coef[k] l^k, clipped at 0 from below; the cubic of the paper,
                                 max{3.06 l^3 - 13.64 l^2 + 18.01 l - 6.44, 0}: (-6.44, 18.01, -13.64, 3.06)      */
    /* ---- the rigid body of the SOFTROD_FEAT_OCTO_HEAD sets, as Cylinder(start, direction = e_z, normal = e_y,
     *      base_length, base_radius = head_radius, density = head_density) allocates it, and its joints ---- */
    double head_center[3];    /* start + direction * base_length / 2.  FlatEnv: (0, 0, 0) (octopus/build.py:95-105);
                                 ArmPullWeightEnv: (-0.9 * 0.015, 0, -0.012) (arm_push_env.py:553-566)            */
    double head_length;       /* Cylinder base_length.  FlatEnv: 2 r0; ArmPullWeightEnv: 2 * radius_base = 0.024  */
    double joint_angle0;      /* FixedJoint2Rigid(angle=...) of arm a, degrees: joint_angle0 + a * joint_angle_step. */
    double joint_angle_step;  /* FlatEnv: 0, 360 / n_arm (octopus/build.py:73-74,117-132); ArmPullWeightEnv: 0, 0
                                 (arm_push_env.py:585-587); build_octopus_muscles: 22.5, 45; build_two_arms: 90, 180
                                 (build_muscle_octopus.py:85-86,202-203)                                           */
    double damper_time_step;  /* AnalyticalLinearDamper(time_step=...) when it is NOT the stepper's dt: the muscle octopus
                                 registers its dampers with 7e-5 (build_muscle_octopus.py:101-106,217-222) and is stepped
                                 with 5e-5 (crawl_env.py:63).  0 = dt.                                              */
} softrod_config;

#define SOFTROD_MAX_SUCKERS 4
#define SOFTROD_MAX_CTRL 8           /* control points per direction             */
#define SOFTROD_MAX_SPLINE_PIECES 8

/* Per-env I/O widths implied by env_kind (OctoFlat: at the reference's n_arm = 8,
 * n_elem = 10, n_knots = 3; ArmPush: continuous mode at n_elem = 40). */
int softrod_action_dim(int env_kind); /* 1, 2, 7, 24, 8, 2                  */
int softrod_obs_dim(int env_kind);    /* 4, 9, 25, 8*56 + 13 = 461, 14, 84  */
int softrod_aux_dim(int env_kind);    /* 0, 1 (info["tilt"], float64), 0    */
/* The same for a given configuration: OctoFlat widths follow n_arm, n_elem and n_knots
 * (flat_env.py:112-141): action n_arm*n_knots; obs n_arm*((n-1) + 4(n+1) + n_knots) + 13,
 * the "individual" rows followed by "shared" (flat_env.py:231-286).  ArmPush (arm_push_env.py:100-130): action 1
 * (discrete: the index 0 / 1 as a float32) or 2 (continuous); obs 2 (n_elem + 1) + 2. */
int softrod_config_action_dim(const softrod_config* cfg);
int softrod_config_obs_dim(const softrod_config* cfg);

typedef struct softrod_handle softrod_handle;

/*
 * Borrowed device pointers to the resident state (valid until destroy).
 * Layout (DESIGN.md "HBM layout"): structure-of-arrays, component-major, one
 * row of `lane_stride` entries per rod (64 for n_elem <= 63: lane k of the rod's
 * wavefront owns node k, element k and Voronoi vertex k; 128 for n_elem <= 126:
 * lane k owns indices 2k and 2k+1; OctoFlat: 64 per wavefront of the env's
 * workgroup, arms `arm_stride` slots apart):
 *     position[(c * n_envs + env) * lane_stride + node]        c = 0..2
 *     director[((r*3 + c) * n_envs + env) * lane_stride + elem]  row r of Q, lab comp. c
 * Mirrors rod.position_collection / velocity_collection / director_collection /
 * omega_collection / tangents of the reference (soft_pendulum.py:152-154).
 */
typedef struct softrod_state_view {
    int32_t n_envs, n_elem, lane_stride;
    int32_t arm_stride; /* OctoFlat: arm a of an env is slots a*arm_stride ..
                           a*arm_stride + n_elem of the env's row; else 0        */
    double* position; /* [3][n_envs][lane_stride] */
    double* velocity; /* [3][n_envs][lane_stride] */
    double* director; /* [9][n_envs][lane_stride] */
    double* omega;    /* [3][n_envs][lane_stride] */
    double* tangents; /* [3][n_envs][lane_stride]  as of the last force evaluation */
    double* time;     /* [n_envs]  simulated time (soft_pendulum.py:141,184) */
    double* control;  /* [4][n_envs]  MovingBaseController position x,y and
                         velocity x,y (soft_pendulum_3d/build.py:15-20);
                         SoftArmTracking: tick (substeps since reset, :222) and
                         the target position x,y,z (wsol[tick], :218-219)     */
    double* kappa;    /* [3][n_envs][lane_stride]  rod.kappa as of the last force
                         evaluation (arm_single_env.py:189); maintained by the
                         feature sets with SOFTROD_FEAT_REST_KAPPA_ACTION     */
    double* rest_kappa; /* [3][n_envs][lane_stride]  rod.rest_kappa (:235);
                         SoftArmTracking: rows 0, 1 = torque_magnitude_cache of the
                         normal / binormal muscle (muscle_torques_with_bspline.py:156) */
    double* env_memory; /* [n_envs][lane_stride]  ArmSingle: prev_kappa_state
                         [0..n-2] (arm_single_env.py:172,190-198); its
                         prev_com_state lives in control[0..1].  SoftArmTracking:
                         [0 .. 2 n_ctrl) points_cached[1, 1:-1] of the two muscles,
                         [16], [17] their initial_call_flag                    */
    float* prev_action; /* [n_envs][7]  the env's _prev_action, written by
                         softrod_step (soft_pendulum.py:165), cleared by reset
                         only where the reference does (soft_pendulum_3d.py:68);
                         OctoFlat: [n_envs][n_arm*n_knots]                     */
    double* head;     /* [20][n_envs]  OctoFlat rigid head (octopus/build.py:103-105):
                         position[3], velocity[3], directors[9] (row-major),
                         omega[3], target[2] (flat_env.py:221); else unused    */
    double* bc_targets; /* [12][n_envs]  what the boundary condition holds node 0 / element 0
                         to: fixed_position[3], fixed_directors[9] (row-major), captured at
                         reset (build.py:81-85: constrained_position_idx=(0,),
                         constrained_director_idx=(0,)).  With the rows above it makes the
                         view a complete snapshot: copying every array out and back in
                         restores a batch exactly (checkpoint / resume).            */
    double* sucker_ratio; /* [SOFTROD_MAX_SUCKERS][n_envs]  effective reduction ratio of each
                         ControllableFixConstraint: SuckerController.reduction_ratio while its
                         flag is on, 0 while it is off (x * (1 - 0) is x).  Written by the
                         caller between steps (arm_two_env.py:228 sets it from the action) */
    double* muscle_activation; /* [SOFTROD_MAX_MUSCLES][n_envs][lane_stride]  MuscleForce.activation of each layer, per
                         element (apply_activation broadcasts a scalar, arm_push_env.py:257-271, or takes an
                         array, arm_two_env.py:246-248, reach_env.py:176-179).  Written by the ArmPush prologue
                         from the action; with env_kind NONE by the caller between steps.  NULL without
                         SOFTROD_FEAT_COOMM_MUSCLES                                                          */
    int32_t* sucker_index; /* [SOFTROD_MAX_SUCKERS][n_envs]  SuckerController.index of each sucker of each env,
                         Python indexing: i >= 0 holds node i and element i; i < 0 holds node n_elem + 1 + i and
                         element n_elem + i (`velocity_collection[..., -1]` is the LAST NODE, `omega_collection
                         [..., -1]` the LAST ELEMENT: arm_push_env.py:262, controllable_constraint.py:66-69).
                         Starts as softrod_config.sucker_index; the ArmPush prologue rewrites row 0 from the
                         action (arm_push_env.py:257,262,270; crawl_env.py:236-238 does the same)              */
    double* material; /* [SOFTROD_MATERIAL_ROWS][lane_stride]  per-node / per-element constants of
                         a TAPERED rod (softrod_set_radius_profile), shared by all envs; NULL
                         for a uniform rod.  Read-only for the caller.                     */
    /* ---- the muscle octopus envs (SOFTROD_ENV_CRAWL / _ARM_TWO / _REACH); NULL otherwise.  Their sucker_ratio /
     *      sucker_index rows are [SOFTROD_MAX_SUCKERS][n_envs * n_arm] (arm a of env e at e * n_arm + a) ---- */
    double* env_aux;  /* [8][n_envs]  ArmPush / ArmPullWeight with early_termination = 1: row 0 is the last step's
                         time-limit flag (1.0 when time > final_time, arm_push_env.py:325-329; 0.0 after an auto-reset);
                         NULL for the other single rods.  The muscle octopus envs: rows 0-2 the env's target (crawl_env.py:172, arm_two_env.py:160: (5, 0);
                         reach_env.py:141-143: np_random.random(3) * sum(rest_lengths)), rows 3-4 the head's x, y before
                         the step (`xposbefore`, crawl_env.py:248), row 5 the episode's own final_time (0: the config's).  (rod.kappa[0] of get_state, crawl_env.py:178,
                         is row 0 of `kappa`: what the last substep's force evaluation cached; zeros after a reset)  */
    float* prev_kappa; /* [n_envs][n_arm * (n_elem - 1)]  ArmTwoEnv._prev_kappa (arm_two_env.py:103,196-203): float32,
                         NOT cleared by reset() — it belongs to the env object, as in the reference            */
} softrod_state_view;

/* Fill `cfg` with SoftPendulumEnv.__init__ defaults (soft_pendulum.py:59-78)
 * and build_soft_pendulum's constants (build.py:18-26,87-113).             */
int softrod_config_softpendulum(softrod_config* cfg, int n_envs);
/* Same for SoftPendulum3DEnv (soft_pendulum_3d.py:28-58) and
 * build_soft_pendulum_3d (soft_pendulum_3d/build.py:43-86).                 */
int softrod_config_softpendulum3d(softrod_config* cfg, int n_envs);
/* Same for ArmSingleEnv (octopus/arm_single_env.py:55-113) and build_arm
 * (octopus/build.py:220-292).                                               */
int softrod_config_arm_single(softrod_config* cfg, int n_envs);
/* Same for FlatEnv (octopus/flat_env.py:55-110) and build_octopus
 * (octopus/build.py:30-217): 8 arms of 10 elements, rigid head, joints.     */
int softrod_config_octo_flat(softrod_config* cfg, int n_envs);
/* Same for SoftArmTrackingEnv (soft_arm/soft_arm_tracking.py:107-158) and the
 * simulator its reset builds (:261-383), game_mode 1.                       */
int softrod_config_soft_arm(softrod_config* cfg, int n_envs);

/* Replaces the constant part of
 *   make_interp_spline(points_cached[0], points_cached[1])(cumsum(system.lengths))
 * (muscle_torques_with_bspline.py:150-158): the interpolant through the n_ctrl + 2 control
 * points (the two end values are zero) is linear in the control values,
 *   S(s) = sum_j y_j phi_j(s),
 * and every phi_j is a piecewise cubic on fixed breakpoints.  The caller passes that form:
 *   breaks: host [n_spline_pieces + 1] float64, ascending
 *   coef:   host [n_spline_pieces][n_ctrl][4] float64, ascending powers of (s - breaks[p])
 * (scipy: PPoly.from_spline(make_interp_spline(x, e_j)); s outside the breaks uses the end
 * pieces, as BSpline's default extrapolation does).  Needed before the first softrod_step
 * of a handle with SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES.                          */
int softrod_set_spline_table(softrod_handle* h, const double* breaks, const double* coef);

/* Replaces: CosseratRod.straight_rod(..., base_radius=<array of n_elements radii>, ...) — a
 * TAPERED rod, as the muscle-arm envs allocate it
 *   radius = np.linspace(radius_base, radius_tip, n_elem + 1); radius_mean = (radius[:-1] + radius[1:]) / 2
 *                                   octopus/arm_push_env.py:160-179, build_muscle_octopus.py
 * Every per-element constant of the allocation (area, volume, nodal masses, second moments,
 * shear / bend matrices and their Voronoi average, the damper's per-element coefficients,
 * the contact radius) then varies along the rod: the library keeps them as per-lane rows
 * (softrod_state_view.material) instead of kernel-argument scalars and runs its general
 * instantiation.  radius: host [n_elem] float64.  Call before the first reset; rods of up to
 * 63 elements, or up to 126 for SOFTROD_FEATURES_ARM_PUSH with SOFTROD_ENV_ARM_PUSH under
 * SOFTROD_MATH_FAST (two slots per lane); not with SOFTROD_FEAT_OCTO_HEAD.                  */
#define SOFTROD_MATERIAL_ROWS 16
int softrod_set_radius_profile(softrod_handle* h, const double* radius);

/* Replaces: the geometry and strength of the muscle layers handed to ApplyMuscles — for the reference's
 * create_es_muscle_layers(radius_mean, radius_base) (octopus/build.py:295-338):
 *   LongitudinalMuscle(muscle_init_angle = +-pi/2, ratio_muscle_position = (0, -6/9, 0) per element,
 *                      rest_muscle_area = (radius_mean / radius_base)^2, max_muscle_stress = 0.5)  x 2
 *   TransverseMuscle(rest_muscle_area = (radius_mean / radius_base)^2, max_muscle_stress = 1.0)
 * ratio_position: host [n_muscles][3][n_elem] float64, the muscle's position in the material frame in units of
 *                 the element radius (how muscle_init_angle enters it is the caller's: _capi.es_muscle_layers);
 * strength:       host [n_muscles][n_elem] float64 = max_muscle_stress * rest_muscle_area, SIGNED (a transverse
 *                 muscle extends the arm: negative).
 * Needed before the first softrod_step / softrod_substeps of a handle with SOFTROD_FEAT_COOMM_MUSCLES; rods of
 * up to 63 elements (126 for SOFTROD_FEATURES_ARM_PUSH with SOFTROD_ENV_ARM_PUSH under SOFTROD_MATH_FAST), one
 * rod per env.                                                                                            */
int softrod_set_muscle_layers(softrod_handle* h, const double* ratio_position, const double* strength);

/* Same for ArmPullWeightEnv (octopus/arm_push_env.py:516-618; registered as OctoArmPullWeight-v0 with mode
 * "continuous", gym_softrobot/__init__.py:48-52): time_step 2.5e-5 (1000 substeps per env.step), damper 0.05 * 2 * 5e2,
 * the sucker at reduction_ratio 0.9, a Cylinder of radius 0.015 / length 0.024 / density 700 joined to node 0 by
 * FixedJoint2Rigid(k = 1e6, nu = 1e-2, kt = 1, angle = 0, radius = 0.015) and held by BodyBoundaryCondition.      */
int softrod_config_arm_pull_weight(softrod_config* cfg, int n_envs);

/* The muscle octopus envs: env_kind = SOFTROD_ENV_CRAWL (CrawlEnv.__init__ / reset, crawl_env.py:61-174 over
 * build_octopus_muscles, build_muscle_octopus.py:66-179), SOFTROD_ENV_ARM_TWO (arm_two_env.py:55-164 over build_two_arms,
 * :182-291) or SOFTROD_ENV_REACH (reach_env.py:53-148).  Arms: 20 elements, 0.25 long, density 1000, E 1.5e4, G 1e4,
 * radii linspace(0.013, 0.0042, n) through softrod_set_radius_profile, layers through softrod_set_muscle_layers (both
 * once: every arm is the same rod); head Cylinder(start (0, 0, -0.026), e_z, e_y, 0.026, 0.04, 50); joints k 1e6, kt 1e2,
 * nu 1e-3; dampers 0.2 * 1e-2 at time_step 7e-5; dt 5e-5, 800 substeps per env.step.  Resets go through softrod_reset_octo
 * / softrod_queue_push_octo (arm frames from the caller, build_muscle_octopus.py:87-93; `target`: FOUR numbers per env
 * here — the target's x, y, z (CrawlEnv / ArmTwoEnv: 5, 0, 0; ReachEnv: its random point) and the episode's own
 * final_time, 0 = softrod_config.final_time (CrawlEnv(config_random_final_time=True) draws one per reset,
 * crawl_env.py:135-136)).                                                                                         */
int softrod_config_muscle_octopus(softrod_config* cfg, int n_envs, int env_kind);

/* Same as softrod_config_arm_single for ArmPushEnv (octopus/arm_push_env.py:65-224): the 40-element arm tapered
 * 12:1 (the radii themselves go through softrod_set_radius_profile), damper, one sucker, three muscle layers
 * (softrod_set_muscle_layers); mode 0 = "discrete" (OctoArmPush-v0), 1 = "continuous" (OctoArmPush-v1).      */
int softrod_config_arm_push(softrod_config* cfg, int n_envs, int mode);

/* Replaces the constant part of set_action's
 *   interp1d(linspace(0,1,n_action), action, kind="cubic")(linspace(0,1,n_seg))
 * (octopus/arm_single_env.py:226-235): cubic not-a-knot interpolation through fixed
 * knots evaluated at fixed abscissae is linear in the action, rest_kappa[0,:] = W a.
 * basis: host [n_elem-1][action_dim] float64 (row-major), computed by the caller
 * with the same scipy call on unit vectors.                                  */
int softrod_set_action_basis(softrod_handle* h, const double* basis);

/* Replaces: BaseSimulator() + build_soft_pendulum(...) + simulator.finalize()
 * (soft_pendulum.py:115-138) for a whole batch: allocates resident device
 * state for cfg->n_envs rods on HIP device `device`.                        */
int softrod_create(const softrod_config* cfg, int device, softrod_handle** out);

/* Replaces: the state part of SoftPendulumEnv.reset (soft_pendulum.py:108-147)
 * i.e. CosseratRod.straight_rod with direction=(cos t, sin t, 0),
 * normal=(sin t, -cos t, 0) (build.py:47-61), time = 0.
 * theta0: host [n_envs] radians (drawn by the caller exactly as build.py:47-49).
 * mask:   host [n_envs] (non-zero = reset this rod) or NULL = all.          */
int softrod_reset(softrod_handle* h, const double* theta0, const uint8_t* mask,
                  void* stream);

/* General straight rod (CosseratRod.straight_rod arguments, build.py:54-61):
 * start/direction/normal are host [n_envs][3]; mask as above.  Also clears the
 * moving-base controller of the reset rods (soft_pendulum_3d.py:67).  Used by
 * SoftPendulum3D (direction = (sin tilt, 0, cos tilt), normal = +y,
 * soft_pendulum_3d/build.py:51-53) and by the known-answer tests.           */
int softrod_reset_straight(softrod_handle* h, const double* start,
                           const double* direction, const double* normal,
                           const uint8_t* mask, void* stream);

/* Replaces: the state part of FlatEnv.reset (octopus/flat_env.py:171-229) ->
 * build_octopus (octopus/build.py:52-217): n_arm straight rods (normal e_z), the
 * Cylinder head at the origin, finalize()'s first constraint pass, time = 0.
 *   arm_start, arm_direction  host [n_envs][n_arm][3]: the
 *       Rotation.from_euler("z", 360/n_arm * i, degrees=True).apply(...) results of
 *       build.py:76-80, computed by the caller as the reference does
 *   target                    host [n_envs][2]: (2 - 0.5) * np_random.random(2) + 0.5
 *   mask                      as softrod_reset                                 */
int softrod_reset_octo(softrod_handle* h, const double* arm_start,
                       const double* arm_direction, const double* target,
                       const uint8_t* mask, void* stream);

/* Replaces: Env.step for every rod (soft_pendulum.py:176-251,
 * soft_pendulum_3d.py:115-174): set_action -> n_substeps x PositionVerlet.step
 * -> NaN check -> reward -> truncation -> get_state.  Asynchronous on `stream`.
 *   actions     device [n_envs][action_dim] float32
 *   obs         device [n_envs][obs_dim]    float32
 *   reward      device [n_envs]             float64
 *   terminated  device [n_envs]             uint8
 *   truncated   device [n_envs]             uint8
 *   aux         device [n_envs][aux_dim]    float64 or NULL (info extras)    */
int softrod_step(softrod_handle* h, const float* actions, float* obs,
                 double* reward, uint8_t* terminated, uint8_t* truncated,
                 double* aux, void* stream);

/* softrod_step with all per-env outputs in ONE buffer, for the multi-GPU path (one
 * all-gather per env.step, unpacked with views only): packed is device
 * [n_envs][ro + 4] 32-bit words per env, ro = obs_dim rounded up to even:
 *   [ obs (obs_dim x float32) | pad to ro | reward (float64, 2 words, 8-byte
 *     aligned) | terminated, truncated (bytes 0 and 1 of one word) | 0 ]       */
int softrod_step_packed(softrod_handle* h, const float* actions, float* packed,
                        double* aux, void* stream);

/* ---- Device-side auto-reset ---------------------------------
 * The reference has no vector env and no auto-reset: a finished env is reset by its
 * caller (gym_softrobot/debug/make.py:16-23).  For a resident batch that would cost a
 * device->host read of the flags on every step.  Instead the caller stages, ahead of
 * time, the next `depth` resets of every env — drawn on the host from the env's own
 * NumPy stream exactly as the reference's build function draws them
 * (build.py:47-49, soft_pendulum_3d/build.py:51, flat_env.py:221), so the streams stay
 * bit-identical — and softrod_step / softrod_step_packed then apply Gymnasium-1.0
 * VectorEnv NEXT_STEP semantics on the device: an env whose previous step returned
 * terminated or truncated consumes its next staged reset INSTEAD of stepping; that call
 * returns its reset observation, reward 0 and both flags clear.  An env that needs a
 * record when none is staged stays finished and is counted in `underflow`.
 *
 *   softrod_autoreset_enable   once per handle; depth = records kept per env
 *   softrod_queue_push*        stage counts[e] (<= max_count) more resets of env e; the
 *                              arrays are host [n_envs][max_count]... with the per-reset
 *                              layout of softrod_reset / _reset_straight / _reset_octo.
 *                              Fails if staged-but-unconsumed + new records would exceed
 *                              depth (as of the last softrod_queue_status).
 *   softrod_queue_status       synchronises; consumed: host [n_envs] records used so far
 *   softrod_queue_status_begin / _poll   the same read without stalling the stream: _begin
 *                              enqueues the copy of the counters (pinned host memory) and an
 *                              event; _poll returns 1 and fills consumed / underflow once the
 *                              event has passed, 0 before; with wait != 0 it waits for that
 *                              event only (work enqueued after _begin keeps the GPU busy
 *                              meanwhile).  The values are as of _begin, which is safe:
 *                              consumed only grows, so a top-up computed from them stages
 *                              at most what fits.  A second _begin SUPERSEDES a read still in
 *                              flight (its result is dropped; _poll then reports the newer
 *                              one); _poll without a _begin is an error.  An env that found no
 *                              record goes on stepping its finished episode and goes on
 *                              reporting truncated (its clock only grows) or terminated (a NaN
 *                              state stays NaN), so a shortage shows in the step outputs at once
 *                              and in `underflow` at the next status read
 *   softrod_queue_advance      mark by[e] staged records of env e as used (a manual reset
 *                              took the env's next draw), or all of them if by[e] < 0
 *                              (the env's stream was re-seeded); synchronises
 * softrod_reset* of an env clears its pending auto-reset.
 *
 * SAME_STEP semantics (Gymnasium 1.x AutoresetMode.SAME_STEP), on the same queue:
 *   softrod_autoreset_same_step(h, on)   after softrod_autoreset_enable (else SOFTROD_EINVAL, "call
 *                              softrod_autoreset_enable first").  on != 0: the pass in front of the step is no
 *                              longer launched; one cold pass runs BEHIND everything softrod_step /
 *                              softrod_step_packed enqueue (csrc/softrod_autoreset.hpp; behind the timing
 *                              record too, so softrod_kernel_times_ms keeps meaning the step).  An env whose step
 *                              ended its episode keeps that step's reward and flags, hands out its terminal
 *                              observation, clock and aux value through the final buffers, consumes its next staged
 *                              record and has the NEW episode's first observation in its obs row (and, for
 *                              SOFTROD_ENV_SOFTPENDULUM3D, that observation's value in `aux`) when the call
 *                              returns; the next call steps the new episode with its own action, so no env ever
 *                              spends a call resetting.  An env may now use one record per step.  An env that
 *                              finds no staged record stays finished exactly as above (its obs row keeps the
 *                              final observation).  Envs that did not finish are not touched.  on = 0 returns to
 *                              NEXT_STEP.  Switch while no env is finished (right after enabling, or after a reset).
 *                              The first on != 0 allocates the final buffers (released by softrod_destroy);
 *                              a captured graph must be captured again after a switch.
 *   softrod_final_view         device pointers, valid for the handle's life: final_obs float [n_envs][obs_dim]
 *                              (dense also under softrod_step_packed), final_time double [n_envs], final_aux
 *                              double [n_envs].  Row e holds the last episode end of env e; which rows the last
 *                              call wrote is that call's terminated | truncated.  SOFTROD_EINVAL while same-step
 *                              is off.                                                  */
int softrod_autoreset_enable(softrod_handle* h, int depth);
int softrod_autoreset_same_step(softrod_handle* h, int on);
int softrod_final_view(softrod_handle* h, float** final_obs, double** final_time, double** final_aux);
int softrod_queue_push(softrod_handle* h, const double* theta0, const int32_t* counts,
                       int max_count, void* stream);
int softrod_queue_push_straight(softrod_handle* h, const double* start,
                                const double* direction, const double* normal,
                                const int32_t* counts, int max_count, void* stream);
int softrod_queue_push_octo(softrod_handle* h, const double* arm_start,
                            const double* arm_direction, const double* target,
                            const int32_t* counts, int max_count, void* stream);
int softrod_queue_status(softrod_handle* h, int32_t* consumed, int32_t* underflow,
                         void* stream);
int softrod_queue_status_begin(softrod_handle* h, void* stream);
int softrod_queue_status_poll(softrod_handle* h, int wait, int32_t* consumed, int32_t* underflow);
int softrod_queue_advance(softrod_handle* h, const int32_t* by, void* stream);

/* Multi-GPU without a collective call per step (no reference counterpart; gym_softrobot_amd/
 * distributed.py, transport "p2p"): copy this handle's `n_envs` packed rows (`row_words` 32-bit
 * words each, as softrod_step_packed wrote them) into rows first_row .. first_row + n_envs - 1 of
 * EVERY buffer in `peer_buffers` (host array of n_peers <= SOFTROD_MAX_PEERS device pointers: the
 * other ranks' exchange buffers, IPC-mapped, and this rank's own), with ONE small kernel on `stream`
 * — enqueued right behind the step kernel it is a few microseconds in order, where a collective on
 * a second stream costs this workload ~37 us of cross-queue dependency latency per step (DESIGN.md
 * §4).  The stores are system-scope write-through; between GPUs they travel over xGMI.
 * tag_word >= 0: once ALL rows of this call have been acknowledged, 32-bit word `tag_word` of every
 * peer buffer receives `tag` (system-scope release): the generation word of this rank in the
 * receivers' buffers (distributed.py keeps `world` of them behind the rows and checks them in
 * sync()).  tag_word < 0: rows only.  The tagged form counts arrivals in ONE per-handle word
 * (allocated and zeroed in softrod_create): tagged scatters of one handle must be stream-ordered
 * with each other — two in flight on different streams would corrupt each other's tag.         */
#define SOFTROD_MAX_PEERS 16
int softrod_scatter_rows(softrod_handle* h, const float* packed, const uint64_t* peer_buffers,
                         int n_peers, int row_words, int64_t first_row, int64_t tag_word,
                         uint32_t tag, void* stream);

/* Exchange buffers of transport "p2p": device memory that OTHER GPUs store into.  A GPU's L2 does
 * not snoop a peer's stores into its HBM, so such a buffer must not be an ordinary (coarse-grained,
 * L2-cached) allocation: softrod_exchange_alloc returns UNCACHED device memory
 * (hipDeviceMallocUncached; *memory_kind = SOFTROD_EXCHANGE_FINEGRAINED where only
 * hipDeviceMallocFinegrained is granted), zeroed, together with its 64-byte IPC handle (NULL: not
 * wanted).  softrod_exchange_open maps a handle received from the process that owns `owner_device`
 * (peer access device -> owner_device is enabled first when they differ; pass -1 to skip) and
 * returns the pointer valid in THIS process; _close unmaps it, _free releases an allocation of
 * _alloc.  No handle argument: these belong to the process, not to a batch.                     */
#define SOFTROD_IPC_HANDLE_BYTES 64
#define SOFTROD_EXCHANGE_UNCACHED 1
#define SOFTROD_EXCHANGE_FINEGRAINED 2
int softrod_exchange_alloc(int device, uint64_t bytes, void** dev_ptr, uint8_t* ipc_handle,
                           int* memory_kind);
int softrod_exchange_open(int device, const uint8_t* ipc_handle, int owner_device, void** dev_ptr);
int softrod_exchange_close(int device, void* dev_ptr);
int softrod_exchange_free(int device, void* dev_ptr);

/* Replaces: get_state() at reset (soft_pendulum.py:145-161,
 * soft_pendulum_3d.py:93-98).  prev_action is device [n_envs][action_dim]
 * float32, or NULL = the resident copy of the last stepped action.          */
int softrod_observe(softrod_handle* h, const float* prev_action, float* obs,
                    void* stream);

/* Replaces: CosseratRod.compute_translational_energy, compute_rotational_energy,
 * compute_bending_energy and compute_shear_energy (pyelastica 1.0.0; called by
 * octopus/arm_push_env.py:446-456 cal_desired_Hamiltonian, and in commented-out code by
 * flat_env.py:336-338, crawl_env.py:269-272, arm_two_env.py:284-287) of every rod of
 * every env.  out: device [n_envs][rods_per_env][4] float64 in the order translational,
 * rotational, bending, shear; rods_per_env = n_arm for OctoFlat and the muscle octopus,
 * else 1 (rigid bodies have none here).  Asynchronous on `stream`, like softrod_observe.
 * THE INSTANT: the reference's sigma / kappa / dilatation are the caches of the last force
 * evaluation, at the mid-substep configuration x - dt/2 v, R(dt/2 omega)^T Q followed by the
 * boundary condition's constrain_values; v and omega are the end-of-step rates.  An env
 * whose time is 0 (just reset) is evaluated at its state as it stands.
 * THE FORMS (recalled from pyelastica 1.0.0, which is not on disk):
 *   translational  1/2 sum_i m_i |v_i|^2
 *   rotational     1/2 sum_e omega_e . (J_e omega_e) / e_e          e_e the dilatation
 *   bending        1/2 sum_k (kappa_k - kappa^_k) . B_k (kappa_k - kappa^_k) D^_k
 *   shear          1/2 sum_e sigma_e . S_e sigma_e  l^_e           (rest sigma 0)  */
int softrod_rod_energies(softrod_handle* h, double* out, void* stream);

/* Ground reaction: what RodPlaneContactWithAnisotropicFriction.apply_contact (registered by
 * octopus/build.py:193-200,274-283; the law as recalled from pyelastica 1.0.0, softrod_contact.hpp) adds to
 * external_forces and external_torques of every rod of every env.  The reference evaluates it in every substep
 * and returns none of it.  out: device [n_envs][rods_per_env][6][n_elem + 1] float64, rods_per_env = n_arm for
 * OctoFlat, else 1:
 *   rows 0-2  the lab-frame force added to each node: the sum of the five contributions after
 *             elements_to_nodes — plane response with its elastic and damping terms, kinetic axial, kinetic
 *             rolling, static axial, static rolling friction
 *   rows 3-5  the material-frame torque added to each element (the two rolling frictions); column n_elem is 0.
 * Asynchronous on `stream`, like softrod_rod_energies; capturable.
 * THE INSTANT: ONE FRESH force evaluation at the state as it stands in device memory — x, v, Q, omega,
 * rest_kappa — with no half kinematic step and no constrain_values before it.  Internal forces and torques are
 * computed from that state; the external loads are gathered in the substep's own order (FixedJoint2Rigid on node
 * 0 / element 0 of each OctoFlat arm first, then the forcing group and the contact in the order
 * contact_before_forcing says), and `out` is what the contact operator added (its static friction reads
 * f_int + f_ext, t_int + t_ext of that moment).  It is NOT the value the last substep applied: that one was
 * evaluated at the mid-substep configuration with the pre-update rates, and the law depends on those rates
 * (normal damping, slip velocities, the static / kinetic blend), so it cannot be recovered from the end state.
 * ARITHMETIC: float64 as written (IEEE division and sqrt, libm acos / sin / cos; no fast-math forms), the same
 * kernel for SOFTROD_MATH_LIBM and SOFTROD_MATH_FAST handles, any plane normal.  The per-env tables of
 * softrod_set_env_contact / softrod_set_env_material and the radius profile of a tapered arm are honoured.
 * Scope: handles with SOFTROD_FEAT_PLANE_CONTACT_ANISO, without COOMM muscles, rods of up to 63 elements:
 * SOFTROD_ENV_ARM_SINGLE (uniform or tapered) and SOFTROD_ENV_OCTO_FLAT (OctoFlat, OctoFlatLite; every wave shape).
 * Anything else (envs without contact, the muscle envs, the two-slot and windowed arms of 64 or more elements,
 * a feature set with a point force or spline muscle torques) -> SOFTROD_EINVAL with "ground reaction: <reason>"
 * in softrod_last_error.                                                                                       */
int softrod_ground_reaction(softrod_handle* h, double* out, void* stream);

/* Rod strains: the fields the reference's diagnostic callback records once per env.step (RodCallBack,
 * utils/custom_elastica/callback_func.py:23-41: sigma, kappa, dilatation, voronoi_dilatation — the interface this
 * call replaces) and the internal loads they stand for, for every rod of every env, on the device: what a
 * curvature or strain gauge senses, for a policy, a reward term or a logger that lives there.  THE FORMS are our
 * recollection of pyelastica 1.0.0 (not on disk).  out: device [n_envs][rods_per_env][14][n_elem] float64,
 * rods_per_env as for softrod_rod_energies (n_arm for OctoFlat and the muscle octopus, else 1; rigid bodies have
 * no rows):
 *   rows 0-2    sigma, the shear / stretch strain in the material frame: e Q t - (0, 0, 1)
 *   rows 3-5    kappa = -log(Q_{k+1} Q_k^T) / D^, material frame, NOT reduced by the rest curvature
 *   row  6      dilatation e = l / l^
 *   row  7      voronoi_dilatation (l_k + l_{k+1}) / (2 D^)
 *   rows 8-10   internal force n = S sigma, material frame; S from the config, the env's row of
 *               softrod_set_env_material or the tapered rod's table (softrod_set_radius_profile), as
 *               softrod_rod_energies picks it
 *   rows 11-13  internal couple m = B (kappa - rest_kappa); rest_kappa only with SOFTROD_FEAT_REST_KAPPA_ACTION
 * Rows 0-2, 6 and 8-10 hold n_elem values; rows 3-5, 7 and 11-13 live on the n_elem - 1 Voronoi vertices and
 * their last column is written as 0.  Every column of every row is written by every call.
 * Rows 8-13 are the PASSIVE elastic loads: on the COOMM muscle envs they exclude the muscle layers' force and
 * couple — that law stays labelled data (DESIGN.md §3 "Muscles").  With them 1/2 sum sigma . n l^ and
 * 1/2 sum (kappa - rest_kappa) . m D^ are the shear and bending energies of softrod_rod_energies.
 * THE INSTANT is the one softrod_rod_energies documents, the reference's: the caches of the last force
 * evaluation, i.e. the mid-substep configuration x - dt/2 v, R(dt/2 omega)^T Q followed by the boundary
 * condition's constrain_values; an env whose time is 0 (just reset) is evaluated at its state as it stands.  The
 * choice is made per env, so a batch may hold both after a masked reset.
 * ARITHMETIC: float64 as written (IEEE division and sqrt, libm acos / sin / cos), one kernel for
 * SOFTROD_MATH_LIBM and SOFTROD_MATH_FAST handles, the statements softrod_rod_energies evaluates.
 * Asynchronous on `stream`, like softrod_rod_energies; capturable.  It reads the state and writes `out` only.
 * Scope: every handle softrod_create accepts — one-slot rods up to 63 elements, two-slot rods up to 126
 * (windowed arms included), tapered rods, every OctoFlat wave shape, per-env material.  The only errors are a
 * null handle or a null `out`: SOFTROD_EINVAL with "rod strains: <reason>" in softrod_last_error.            */
int softrod_rod_strains(softrod_handle* h, double* out, void* stream);

/* Muscle loads: what the reference's ApplyMuscles computes in every substep and returns none of
 * (gym_softrobot/envs/octopus/arm_push_env.py:197-212 over the layers of create_es_muscle_layers,
 * octopus/build.py:295-338): every COOMM layer's force and length, the muscle internal force and couple, and the
 * equivalent external loads they become, for every rod of every env, on the device — muscle length and tension
 * for a policy's proprioception, actuation effort for a reward term.  It completes softrod_rod_strains, whose
 * loads are the passive ones.  PARITY UNPINNED: the law is softrod_muscle.hpp's restatement of COOMM, which is not
 * on disk; every recalled detail is a field of softrod_config (muscle_kind, muscle_tm_length_law,
 * muscle_equiv_load_form, muscle_position_current_radius, muscle_fl_degree / muscle_fl_coef, n_muscles), all
 * honoured here.  out: device [n_envs][rods_per_env][20][n_elem + 1] float64, rods_per_env as for
 * softrod_rod_energies:
 *   rows 0-3    layer force F_m = activation * strength * max(fl(l_m), 0), layers 0..3           n_elem columns
 *   rows 4-7    layer length l_m: |nu_m|, or |nu_m|^-1/2 for a transverse layer under
 *               muscle_tm_length_law 0; nu_m = e Q t + kappa_e x x_m                             n_elem
 *   rows 8-10   muscle internal force f = sum F_m t_m, material frame                            n_elem
 *   rows 11-13  muscle internal couple on the Voronoi vertices c_v = 1/2 (c_k + c_{k+1}),
 *               c = sum x_m x F_m t_m, material frame                                            n_elem - 1
 *   rows 14-16  equivalent external force on the nodes, lab frame: what ApplyMuscles adds to
 *               external_forces                                                                  n_elem + 1
 *   rows 17-19  equivalent external couple on the elements, material frame: what it adds to
 *               external_torques                                                                 n_elem
 * Every column of every row is written by every call: the columns past a row's range, and every row of a layer
 * m >= n_muscles, as +0.0.  A layer is evaluated whatever its activation is (the step kernels skip a layer that is
 * off in the whole rod): the length rows are always defined.
 * THE INSTANT is the one softrod_rod_strains documents: the mid-substep configuration of the last force evaluation,
 * or the state as it stands for an env whose time is 0, per env.
 * THE ACTIVATIONS are the resident rows softrod_state_view.muscle_activation as they stand, read per element: after
 * a step, what that step's action wrote.  For an env whose time is not 0 rows 14-19 are therefore the loads the last
 * substep's force evaluation added, to rounding.  One exception: the SOFTROD_MATH_FAST OctoArmPush stepper in
 * continuous mode applies element 0's value of the rows of layers 0 and 1 to every element, this call reads every
 * element; the two agree where those rows are uniform over the elements, which is what a step leaves behind.
 * ARITHMETIC: float64 as written (IEEE division and sqrt), one kernel for SOFTROD_MATH_LIBM and SOFTROD_MATH_FAST
 * handles.  Asynchronous on `stream`, like softrod_rod_energies; capturable.  It reads the state and writes `out` only.
 * Errors, each SOFTROD_EINVAL with its text in softrod_last_error: "muscle loads: null handle", "muscle loads: null
 * output buffer", "muscle loads: this handle has no COOMM muscles" (no SOFTROD_FEAT_COOMM_MUSCLES), "muscle loads:
 * softrod_set_muscle_layers has not been called".                                                               */
int softrod_muscle_loads(softrod_handle* h, double* out, void* stream);

/* Joint loads: what the reference's FixedJoint2Rigid (gym_softrobot/utils/custom_elastica/joint.py:47-219) computes in
 * every substep and returns none of — _apply_forces returns contact_force and apply_forces drops it — for every arm
 * of every env whose arms are joined to a rigid body, and what the body makes of their sum, on the device: the pull
 * on the weight of OctoArmPullWeight, the propulsive force and turning moment the arms give the head of OctoFlat and
 * OctoCrawl, the acceleration an IMU on the head would read.  out: device [n_envs][rods_per_env + 1][16] float64,
 * rods_per_env as for softrod_rod_energies (n_arm for OctoFlat, OctoFlatLite and the muscle octopus, 1 for
 * OctoArmPullWeight).
 * Row a < rods_per_env is the joint of arm a, in the reference's words:
 *   columns 0-2    contact_force: what the joint adds to the body's external_forces, lab frame
 *   columns 3-5    -Q_body . torque: what it adds to the body's external_torques, body frame
 *   columns 6-8    -contact_force: added to the arm's node 0; the exact negation of columns 0-2
 *   columns 9-11   Q_arm[..., 0] . torque: added to the arm's element 0, that element's material frame
 *   columns 12-14  end_distance_vector: the arm's node 0 minus its connection point, rigid_rod_pos (the body's
 *                  position with z zeroed) plus rigid_rod_connection_dir * head_radius
 *   column  15     end_distance
 * Row rods_per_env is the body:
 *   columns 0-2    net force: columns 0-2 summed over the arms in arm order 0, 1, ..., added left to right (the
 *                  order of the reference's loop over its connections; bitwise the same from run to run)
 *   columns 3-5    net torque, summed the same way
 *   columns 6-8    linear acceleration f / head_mass under the body's constraints:
 *                  BodyBoundaryCondition.compute_constrain_rates holds v_z, so a_z = +0.0
 *   columns 9-11   angular acceleration in the body frame, (+0.0, +0.0, t_z / J_3).  The gyroscopic term (J w) x w of
 *                  update_accelerations vanishes identically for the constrained body: its omega is held to
 *                  (0, 0, w_z) and its inertia is diagonal, so J w is parallel to w
 *   columns 12-15  +0.0
 * With softrod_config.head_fixed (OneEndFixedBC on the body: OctoReach) columns 6-11 of the body's row are all +0.0;
 * the forces and torques are still reported.  Every column of every row is written by every call.
 * THE INSTANT is softrod_ground_reaction's: ONE evaluation at x, v, Q of the arms and of the body as they stand in
 * memory — no half kinematic step, no constrain_values.  It is NOT the value the last substep applied, which was
 * taken at the mid-substep configuration.
 * ARITHMETIC: float64 as written (IEEE division and sqrt, no contraction), one kernel for SOFTROD_MATH_LIBM and
 * SOFTROD_MATH_FAST handles.  Asynchronous on `stream`, like softrod_rod_energies; capturable.  It reads the state
 * and writes `out` only.
 * Errors, each SOFTROD_EINVAL with its text in softrod_last_error: "joint loads: null handle", "joint loads: null
 * output buffer", "joint loads: this handle has no rigid body" (no SOFTROD_FEAT_OCTO_HEAD).                      */
int softrod_joint_loads(softrod_handle* h, double* out, void* stream);

/* Rod dynamics: the two sides of every rod's equation of motion — what PyElastica keeps on every rod as
 * internal_forces / internal_torques, external_forces / external_torques and, once update_accelerations has run,
 * acceleration_collection / alpha_collection, and the reference returns none of — for every rod of every env, on the
 * device: what an accelerometer or a gyro-rate sensor on a soft arm would read, what a reward that penalises jerk or
 * effort needs.  The other read-outs return one contribution each (softrod_ground_reaction the contact's,
 * softrod_muscle_loads the muscles', softrod_joint_loads the joint's); this one returns their sum.
 * out: device [n_envs][rods_per_env][18][n_elem + 1] float64, rods_per_env as for softrod_rod_energies:
 *   rows 0-2    internal force on the nodes, lab frame: CosseratRod._compute_internal_forces           n_elem + 1 columns
 *   rows 3-5    internal torque on the elements, material frame: _compute_internal_torques — bend/twist
 *               difference, kappa x B kappa, shear couple, (J w / e) x w, unsteady dilatation          n_elem
 *   rows 6-8    external force on the nodes, lab frame: everything synchronize adds                    n_elem + 1
 *   rows 9-11   external torque on the elements, material frame: everything it adds                    n_elem
 *   rows 12-14  acceleration = (internal force + external force) / mass, lab frame                     n_elem + 1
 *   rows 15-17  angular acceleration = J^-1 (internal torque + external torque) e, material frame      n_elem
 * Column n_elem of the per-element rows is written as +0.0; every column of every row is written by every call.
 * THE INSTANT is softrod_ground_reaction's: ONE FRESH evaluation at x, v, Q, omega, rest_kappa (and the rigid body's
 * state) as they stand in device memory, with no half kinematic step and no constrain_values before it.  It is NOT
 * the value the last substep applied: that one was taken at the mid-substep configuration with the pre-update rates.
 * Constraints, the analytical damper, the Laplace filter and the suckers act on values and rates, not on loads, and
 * do not enter: this is update_accelerations, before constrain_rates.
 * THE ORDER in which the external loads are gathered is the substep's own: FixedJoint2Rigid on node 0 / element 0 of
 * every arm of a handle with SOFTROD_FEAT_OCTO_HEAD; then the forcing group — gravity times nodal mass, the point
 * force of SOFTROD_FEAT_POINT_FORCE_NODE0_X (which ASSIGNS component x of node 0), the tip force, the COOMM layers'
 * equivalent loads — and the plane contact (the literal law of softrod_ground_reaction, reading f_int + f_ext and
 * t_int + t_ext of its moment), before or after that group as contact_before_forcing says.
 * THE ACTION-BORNE INPUTS are read from the resident state.  The point force is the env's resident previous action
 * as the step prologue applies it, (double)prev_action[0], and 0.0 for an env whose time is 0: a fresh simulator has
 * no point force until the first set_action, while _prev_action survives reset.  The muscle activations are the
 * rows softrod_state_view.muscle_activation as they stand, read per element, and the muscle law (PARITY UNPINNED, as
 * for softrod_muscle_loads) is evaluated on the strains of THIS state — softrod_muscle_loads' instant is another
 * one unless the env's time is 0.
 * ARITHMETIC: float64 as written (IEEE division and sqrt, libm acos / sin / cos, no contraction), one kernel for
 * SOFTROD_MATH_LIBM and SOFTROD_MATH_FAST handles.  The per-env tables of softrod_set_env_material /
 * softrod_set_env_contact and the radius profile of a tapered rod are honoured.  Asynchronous on `stream`, like
 * softrod_rod_energies; capturable.  It reads the state and writes `out` only.
 * Scope: every handle whose rods have one slot per lane (n_elem <= 63), either math mode, every env kind except
 * SOFTROD_ENV_SOFT_ARM.  Errors, each SOFTROD_EINVAL with its text in softrod_last_error: "rod dynamics: null
 * handle", "rod dynamics: null output buffer", "rod dynamics: not with spline muscle torques (loads that are not in
 * the resident state)", "rod dynamics: rods of up to 63 elements only (not the two-slot or windowed long rods)",
 * "rod dynamics: softrod_set_muscle_layers has not been called".                                                */
int softrod_rod_dynamics(softrod_handle* h, double* out, void* stream);

/* Per-env rod material, for domain randomisation of single-rod envs.  Upstream has no counterpart: there
 * every env builds its rod with CosseratRod.straight_rod(..., density, youngs_modulus, shear_modulus) and
 * AnalyticalLinearDamper(damping_constant, ...), and a batch of them shares one softrod_config.  This call
 * gives env i its own (E, G, rho, nu):
 *   material  host [n_envs][4] float64: youngs_modulus, shear_modulus, density, damping_constant;
 *             each finite, E, G, rho > 0, nu >= 0 (checked for the rows that change)
 *   mask      host [n_envs], or NULL for every env: only rows with mask[i] != 0 change.
 * Each row holds what fill_params derives from the four values (J, 1/J, shear and bend stiffnesses, node and
 * rod mass, the damper's factors), computed by fill_params itself on a copy of the config: a row set to the
 * config's own values holds the kernel arguments' doubles bit for bit.  The first call allocates the table
 * with every row at the config's values; the rest geometry, reset records and the auto-reset queue do not
 * depend on it.  A row takes effect at the next launch on `stream` (step, reset, observe, device auto-reset,
 * softrod_rod_energies).  A graph captured before the first call does not see the table (capture again);
 * later calls update it in place.
 * Scope: uniform rods of up to 63 elements of SOFTROD_ENV_SOFTPENDULUM, _SOFTPENDULUM3D and _ARM_SINGLE with
 * their own feature sets, both math modes.  Anything else (tapered rods, the two-slot and windowed long rods,
 * OctoFlat, the muscle envs, SoftArmTracking) -> SOFTROD_EINVAL, with the reason in softrod_last_error.   */
int softrod_set_env_material(softrod_handle* h, const double* material, const uint8_t* mask, void* stream);

/* Per-env ground contact and friction, for domain randomisation of the contact envs.  Upstream registers
 * RodPlaneContactWithAnisotropicFriction(k, nu, slip_velocity_tol, static_mu_array, kinetic_mu_array) once per
 * build (octopus/build.py:236-283 for build_arm, the same block in build_octopus), with k = 1e2, nu = 1e1 marked
 * "These need to be global parameter to tune", and the mu arrays from override_params' friction_multiplier and
 * friction_symmetry (build.py:30-44,178-190); a batch of them shares one softrod_config.  This call gives env i
 * its own contact law inputs:
 *   contact   host [n_envs][8] float64: contact_k, contact_nu, kinetic_mu[3], static_mu[3] (each mu array
 *             forward, backward, sideways, as in softrod_config); each finite and >= 0 (checked for the rows
 *             that change)
 *   mask      host [n_envs], or NULL for every env: only rows with mask[i] != 0 change.
 * The first call allocates the table with every row at the config's values (a row set to them gives the kernel
 * arguments' doubles bit for bit); slip_velocity_tol, the plane and the rest of the config stay shared.  A row
 * takes effect at the next launch of the step on `stream` (reset, observe, auto-reset and the energies do not
 * read contact).  A graph captured before the first call does not see the table (capture again); later calls
 * update it in place.  A handle may carry this table and softrod_set_env_material's.
 * Scope: SOFTROD_ENV_ARM_SINGLE with its own feature set on a plane with normal e_z, uniform rods of up to 63
 * elements, both math modes; SOFTROD_ENV_OCTO_FLAT (OctoFlat, OctoFlatLite) on an e_z plane with at most two
 * waves per env, i.e. n_arm x segment <= 128 lanes (OctoFlat-v0: four envs per workgroup; OctoFlatLite-v0: one).
 * Anything else (tapered arms, the long and windowed arms, the muscle envs, other planes, envs without contact,
 * OctoFlat's four- and eight-wave shapes, and a handle with early_termination set, in either math mode: the
 * fast kernels that evaluate it do not carry the table, and the scope stays one for both modes) ->
 * SOFTROD_EINVAL with "per-env contact" in softrod_last_error.  */
int softrod_set_env_contact(softrod_handle* h, const double* contact, const uint8_t* mask, void* stream);

/* Fork resident envs on the device, for planning: after the call, on `stream`, env dst[i] is an exact (bitwise) copy
 * of env src[i] as it stood before the call, for i = 0 .. count - 1 — what CEM, MPPI, population-based training and
 * branching a rollout for a value estimate begin with.  Upstream has no counterpart (an env there is one Python
 * object; its state is never copied).  Here it replaces the host path of the Python layer, backend.snapshot() +
 * restore(), which moves the WHOLE batch to the host and back, synchronises the device twice and re-uploads the
 * per-env tables.  src, dst: host [count] env indices.  Asynchronous on `stream`, like softrod_observe: one small
 * upload of the pairs (through a pinned buffer the handle owns, sized for n_envs pairs at create: no allocation per
 * call) and one cold kernel, softrod_copy_envs_kernel (csrc/softrod_copy_envs.hpp), one workgroup per pair.
 * NOT graph-capturable: the arguments are validated on the host and the pairs are uploaded by the call.
 * WHAT IS COPIED is every per-env datum the handle keeps:
 *   - env src's part of every array of softrod_state_view: the rows position, velocity, director, omega, tangents,
 *     kappa, rest_kappa, env_memory, muscle_activation; the columns time, control, head, bc_targets, env_aux;
 *     prev_action, prev_kappa; sucker_ratio and sucker_index (the muscle octopus's [4][n_envs * n_arm] form: all
 *     n_arm entries of the env).  Arrays the handle does not have (NULL in the view) are skipped
 *   - the env's row of the device tables of softrod_set_env_material and softrod_set_env_contact, where they exist
 *     (before the first softrod_set_env_* call there is no table and every env runs on the config's values).
 * softrod_create allocates nothing else per env.  The arrays shared by all envs — `material`, the spline table, the
 * action basis, the muscle layers — are not touched.  With it softrod_state_view's promise ("a complete snapshot")
 * holds on the device: a copy and its source, stepped with the same actions, stay bitwise equal.
 * count == 0 is a successful no-op, and so is a pair with src[i] == dst[i].  One src may feed any number of dst.
 * Errors, each SOFTROD_EINVAL with its text in softrod_last_error, found on the host before anything is enqueued (a
 * refused call changes nothing):
 *   "copy envs: null handle"
 *   "copy envs: not on a handle with device-side auto-reset ..." (softrod_autoreset_enable: the pending-reset flags
 *       and the staged queue belong to each env's RNG future)
 *   "copy envs: count <c> is outside 0 .. n_envs = <N>"
 *   "copy envs: null src or dst" (with count > 0)
 *   "copy envs: env index <e> (pair <i>) is outside 0 .. <N - 1>"
 *   "copy envs: env <e> appears twice in dst"
 *   "copy envs: env <e> is the dst of one pair and the src of another" (the kernel reads and writes in place: that
 *       result would depend on scheduling; copy in two calls instead).                                            */
int softrod_copy_envs(softrod_handle* h, const int32_t* src, const int32_t* dst, int count, void* stream);

/* State bank: `slots` off-batch slots on the device, each holding one complete env state — everything
 * softrod_copy_envs copies — saved from any env and loaded into any env, any number of times.  What restart
 * distributions over visited states (Go-Explore archives, backplay, resets to demonstration states), branched rollouts
 * from stored states, tree search that returns to a node, and a planner that parks its controlled trajectory while the
 * whole batch explores are built on.  Upstream has no counterpart.  Here it replaces the host path backend.snapshot()
 * -> row surgery -> restore(), two round trips of the whole batch for a change to a few envs, and it frees the live
 * env that softrod_copy_envs needs to keep a state in: steps and resets never touch a slot.
 * softrod_bank_create allocates, for every per-env array the handle has (the list under softrod_copy_envs: the arrays
 * of softrod_state_view, the tables of softrod_set_env_material / _contact and the rows of softrod_set_reset_shapes
 * where they exist), a twin with `slots` rows in place of n_envs, zeroed, and a pinned staging buffer of its own for
 * max(n_envs, slots) pairs.  The list is the one softrod_copy_envs walks, not a second one.  Once per handle; the bank
 * lives until softrod_destroy.  A per-env table or the reset-shape rows created AFTER the bank get their twin at that
 * moment, every slot's row at the value the new array gives an untouched env (the config's material or contact;
 * index -1, episode 0), and softrod_set_reset_shapes, which restarts every env's sequence of starts, restarts every
 * slot's.  The rule: a slot loads as the env it was saved from would be now, had nothing touched it since the save.
 * Errors (SOFTROD_EINVAL unless noted; the handle is unchanged and has no bank):
 *   "bank create: null handle"
 *   "bank create: not on a handle with device-side auto-reset ..." (softrod_copy_envs' reason)
 *   "bank create: the handle already has a state bank of <K> slots"
 *   "bank create: slots <k> is not positive"
 *   SOFTROD_ENOMEM "bank create: ..." when the device or the host cannot hold it.                                 */
int softrod_bank_create(softrod_handle* h, int slots);

/* Save: after the call, on `stream`, slot slots[i] is an exact (bitwise) copy of env envs[i] as it stood before the
 * call, for i = 0 .. count - 1, and holds a state from then on.  envs, slots: host [count].  One env may go into any
 * number of slots; a slot may appear once.  Asynchronous on `stream`: one small upload of the pairs through the bank's
 * pinned buffer and one cold kernel, softrod_bank_copy_kernel (csrc/softrod_state_bank.hpp), one workgroup per pair —
 * the bytes softrod_copy_envs moves per pair.  NOT graph-capturable: the arguments are validated on the host and the
 * pairs are uploaded by the call.  count == 0 is a successful no-op.
 * Errors, each SOFTROD_EINVAL with its text in softrod_last_error, found on the host before anything is enqueued (a
 * refused call changes nothing):
 *   "bank save: null handle"
 *   "bank save: the handle has no state bank ..." (softrod_bank_create)
 *   "bank save: not on a handle with device-side auto-reset ..."
 *   "bank save: count <c> is outside 0 .. slots = <K>"
 *   "bank save: null envs or slots" (with count > 0)
 *   "bank save: env index <e> (pair <i>) is outside 0 .. <N - 1>"
 *   "bank save: slot index <k> (pair <i>) is outside 0 .. <K - 1>"
 *   "bank save: slot <k> appears twice".                                                                          */
int softrod_bank_save(softrod_handle* h, const int32_t* envs, const int32_t* slots, int count, void* stream);

/* Load: after the call, on `stream`, env envs[i] is an exact (bitwise) copy of slot slots[i], for i = 0 .. count - 1:
 * stepped with the same actions it continues bitwise as the env it was saved from did.  slots, envs: host [count].
 * One slot may feed any number of envs; an env may appear once.  The slot keeps its state.  The pinned host copies of
 * the material and contact tables follow the load, so a later softrod_set_env_* uploads the loaded rows.  Asynchronous
 * and NOT graph-capturable, as softrod_bank_save; count == 0 is a successful no-op.
 * Errors (SOFTROD_EINVAL, host only, a refused call changes nothing): softrod_bank_save's with "bank load: " in front,
 * and in place of its last two
 *   "bank load: count <c> is outside 0 .. n_envs = <N>"
 *   "bank load: slot <k> holds no state" (never saved)
 *   "bank load: env <e> appears twice".                                                                           */
int softrod_bank_load(softrod_handle* h, const int32_t* slots, const int32_t* envs, int count, void* stream);

/* The bank's shape: *slots (0: the handle has no bank), *bytes_per_slot — the device bytes of one env's state, the sum
 * over the arrays softrod_copy_envs walks, which is what one slot takes and one save or load moves — and, where `filled`
 * is not NULL, filled[k] != 0 for every slot k that holds a state (host [slots]).  Host only.                        */
int softrod_bank_info(softrod_handle* h, int32_t* slots, uint64_t* bytes_per_slot, uint8_t* filled);

/* Render: batched RGB and depth frames of the resident envs, on the device.  Replaces: render() of
 * render_mode="rgb_array", which upstream ships on every env (metadata["render_modes"]) and draws one env at a time on
 * the host; here it is what pixel observations, RGB-D policies and per-env video logging of a resident batch need.  A
 * small software rasteriser (csrc/softrod_render.hpp) reads the resident state and writes
 *   rgb    device [n_envs][H][W][3] uint8
 *   depth  device [n_envs][H][W] float32, or NULL: not wanted (RGB is bitwise the same either way)
 * on `stream`.  Nothing of upstream's renderers is reproduced (no POV-Ray parity, no perspective, no ground plane, no
 * anti-aliasing): THE IMAGE MODEL below is this library's own and is the whole contract.
 * CAMERA (softrod_camera; orthographic, shared by all envs of the handle): `center`; unit, mutually orthogonal axes
 *   `right` = a and `up` = b; the direction towards the viewer is n = a x b; `half_width` > 0 in world units; `width` W
 *   and `height` H in pixels; `follow` 0: center is absolute, 1: center is added to the env's anchor — the rigid body's
 *   position (`head` rows 0-2) for a handle with SOFTROD_FEAT_OCTO_HEAD, else node 0 of rod 0; `target_radius`;
 *   `light`, a unit vector in camera coordinates; `ambient` in [0, 1].  A world point X maps to
 *   (u, v, w) = ((X - c) . a, (X - c) . b, (X - c) . n), computed in float64 from the float64 state (a crawling octopus
 *   may be far from the origin) and only then rounded to float32; everything per pixel is float32.
 * PIXELS: row i, column j has its centre at u = ((j + 0.5) / W * 2 - 1) * half_width,
 *   v = (1 - (i + 0.5) / H * 2) * half_width * H / W.
 * PRIMITIVES, in this order (the order decides ties):
 *   1. for rod 0 .. rods - 1, for element k = 0 .. n_elem - 1: the capsule between nodes k and k + 1, its radius the
 *      element's REST radius (base_radius, or element k of softrod_set_radius_profile's array; the dilatation is ignored)
 *   2. the rigid body of a handle with SOFTROD_FEAT_OCTO_HEAD: a sphere of head_radius
 *   3. the env's target, a sphere of target_radius: SOFTROD_ENV_ARM_SINGLE softrod_config.target with z = 0;
 *      SOFTROD_ENV_OCTO_FLAT `head` rows 18-19 with z = 0; the muscle octopus envs `env_aux` rows 0-2, with z = 0 for
 *      the two-component targets of SOFTROD_ENV_CRAWL / _ARM_TWO; SOFTROD_ENV_SOFT_ARM `control` rows 1-3; the other
 *      envs have none.
 * COVERAGE AND DEPTH of a primitive with projected end points A, B and depths wA, wB (a sphere: A = B), at pixel p:
 *   t = clamp((p - A) . (B - A) / |B - A|^2, 0, 1), t = 0 when |B - A|^2 == 0;  q = A + t (B - A);  d = |p - q|;
 *   covered iff d < r;  h = sqrt(r^2 - d^2);  surface depth z = wA + t (wB - wA) + h;
 *   camera-frame normal m = (p_u - q_u, p_v - q_v, h) / r.
 *   This is a sphere-swept impostor: exact for the silhouette, and exact for the depth where the element is
 *   perpendicular to the view.  The covering primitive with the greatest z wins; on equal z the lowest index wins.
 * COLOUR: palette[body] * (ambient + (1 - ambient) * max(0, m . light)) per channel, stored as floor(255 x + 0.5)
 *   clamped to 0 .. 255; body = the arm index modulo 8 for a rod (entries 0-7), 8 the rigid body, 9 the target.  An
 *   uncovered pixel gets SOFTROD_RENDER_BACKGROUND and depth -inf.
 * NON-FINITE STATE: a primitive with a non-finite coordinate or radius (after rounding to float32) covers no pixel: a
 *   blown-up env renders as background and disturbs no other env.
 * The call validates with softrod_camera_check before it enqueues anything, then launches ONE kernel: asynchronous on
 * `stream`, capturable — the camera travels in the kernel arguments, the radii live in a device table made by
 * softrod_create and rewritten by softrod_set_radius_profile, nothing is uploaded per call.  It reads the state and
 * writes the two outputs only.  Scope: every handle softrod_create accepts — one- and two-slot rows, windowed long arms,
 * tapered rods, every OctoFlat wave shape, handles with device-side auto-reset — of at most 8 * 126 + 2 primitives per
 * env.  Errors, each SOFTROD_EINVAL with its text in softrod_last_error: "render: null handle", "render: null camera",
 * "render: null rgb buffer", every refusal of softrod_camera_check, "render: more than 1010 primitives per env".
 *
 * softrod_camera_default   host only (no device): a view that frames a freshly reset env of `cfg`, 84 x 84 pixels.
 *                          Planar SoftPendulum: looking along -z, x right, y up, half_width 1.1 base_length.  The
 *                          ground-plane envs (ArmSingle, ArmPush, OctoFlat, the muscle envs): from above, x right, y up;
 *                          those with a rigid body follow it and span 1.1 (head_radius + base_length).  SoftPendulum3D
 *                          and SoftArmTracking: a fixed oblique view from (+x, -y, +z), right (0.8, 0.6, 0), up
 *                          (-0.36, 0.48, 0.8), centred on the middle of the reset rod, half_width 0.75 base_length.
 *                          target_radius 0.05 base_length, light (-0.48, 0.6, 0.64), ambient 0.35.
 * softrod_camera_check     host only: SOFTROD_EINVAL with "render: <reason>" in softrod_last_error(NULL) for a null
 *                          camera, a wrong struct_size, width or height outside 1 .. 1024, a non-finite field,
 *                          half_width <= 0, axes whose norms differ from 1 or whose dot product differs from 0 by more
 *                          than 1e-6, a light that is not unit to 1e-6, ambient outside [0, 1], target_radius < 0, a
 *                          follow that is neither 0 nor 1.                                                              */
typedef struct softrod_camera {
    uint32_t struct_size; /* = sizeof(softrod_camera); ABI guard */
    int32_t width, height;
    int32_t follow;
    double center[3];
    double right[3];
    double up[3];
    double half_width;
    double target_radius;
    double light[3];
    double ambient;
} softrod_camera;
/* 0xRRGGBB: arm index modulo 8 (entries 0-7), the rigid body, the target; mirrored in _capi.RENDER_PALETTE */
#define SOFTROD_RENDER_PALETTE                                                                             \
    { 0x1F77B4u, 0xFF7F0Eu, 0x2CA02Cu, 0xD62728u, 0x9467BDu, 0x8C564Bu, 0xE377C2u, 0x17BECFu, 0x7F7F7Fu, 0xBCBD22u }
#define SOFTROD_RENDER_BACKGROUND 0xF5F5F5u
int softrod_camera_default(const softrod_config* cfg, softrod_camera* cam);
int softrod_camera_check(const softrod_camera* cam);
int softrod_render(softrod_handle* h, const softrod_camera* cam, uint8_t* rgb, float* depth, void* stream);

/* Rod clearance: where the rods of an env are relative to each other, to themselves and to the env's target, on the
 * device — arm-arm, self and target proximity.  Upstream has no rod-rod contact in any env (arms pass through each
 * other, a long arm through itself) and rewards reaching by tip or head distance only; this is what a collision
 * penalty, a planner that rejects interpenetrating gaits on forked envs, a sucker-based grasping reward or a
 * tactile-proximity observation needs.  One cold kernel (csrc/softrod_clearance.hpp) reads the resident positions and
 * writes `out`.
 * BODIES: element k of a rod is the capsule around the segment node k -> node k + 1; its radius is the element's REST
 * radius, the table softrod_render draws with (base_radius, or element k of softrod_set_radius_profile's array), so a
 * radius profile is honoured and the dilatation is ignored.  The rigid head / weight of a handle with
 * SOFTROD_FEAT_OCTO_HEAD is deliberately NOT a body here: the arms are joined to it, so their first element always
 * "touches".
 * out: device [n_envs][rods_per_env][rods_per_env + 1][6] float64, rods_per_env as for softrod_rod_energies.  For env
 * e, row rod a and column b, out[e][a][b][0..5] is one record
 *     gap, distance, i, j, s, t
 *   b < rods_per_env, b != a (arm-arm), over all element pairs (i of rod a, j of rod b): gap = the minimum of
 *     (centre-line distance - r_i) - r_j, negative when the capsules interpenetrate; distance = that pair's
 *     centre-line distance; i, j the element indices; s, t in [0, 1] the closest points' parameters along element i
 *     and element j.  Record [b][a] is the SAME pair with i <-> j and s <-> t: it is evaluated once, as rod a < b
 *     against rod b, and written twice.
 *   b == a (self): the same over the pairs with j - i >= self_gap; 2 <= self_gap <= 126.  If no such pair exists
 *     (n_elem <= self_gap) the record is +inf, +inf, -1, -1, 0, 0.  There is no default: the first separation at
 *     which two elements of a STRAIGHT rod no longer overlap by construction is max(2, 1 + ceil(2 max(r) / rest
 *     element length)), which the Python layer passes (_capi.rod_clearance_self_gap).
 *   b == rods_per_env (target): distance = the distance from the env's target point to the nearest point of rod a's
 *     centre line, gap = distance - r_i, i the element, s the parameter along it, j = -1, t = 0.  The target is the
 *     one softrod_render draws (PRIMITIVES, 3): SOFTROD_ENV_ARM_SINGLE softrod_config.target with z = 0;
 *     SOFTROD_ENV_OCTO_FLAT `head` rows 18-19 with z = 0; the muscle octopus envs `env_aux` rows 0-2, with z = 0 for
 *     SOFTROD_ENV_CRAWL / _ARM_TWO; SOFTROD_ENV_SOFT_ARM `control` rows 1-3.  The other envs have none: their target
 *     records are +inf, +inf, -1, -1, 0, 0 whatever the state.
 *   The indices are stored as exact doubles.  Every record is written by every call.
 * ARITHMETIC: float64 as written — IEEE division and sqrt, no contraction, u . v = (u0 v0 + u1 v1) + u2 v2.  Every
 *   coordinate (rod a's nodes, rod b's nodes, the target) is taken relative to node 0 of rod a BEFORE any product: a
 *   crawling octopus may be metres from the origin, and the products cancel.  clamp(x) = 0 if x < 0, 1 if x > 1, else x.
 * THE SEGMENT-SEGMENT RULE is the clamped closest-point construction (Ericson, Real-Time Collision Detection,
 *   5.1.9) for P1 + s d1 (element i: P1 node i, d1 = node i + 1 - node i) and P2 + t d2 (element j):
 *     r = P1 - P2;  a = d1 . d1;  e = d2 . d2;  f = d2 . r;  c = d1 . r;  b = d1 . d2
 *     a zero-length element is a point:   not a > 0 and not e > 0:  s = t = 0
 *                                         not a > 0:                s = 0, t = clamp(f / e)
 *                                         not e > 0:                t = 0, s = clamp(-c / a)
 *     otherwise  denom = a e - b b;  s = clamp((b f - c e) / denom) if denom > 0, else s = 0 (parallel elements take
 *                s = 0 first);  t = (b s + f) / e;
 *                if t < 0: t = 0, s = clamp(-c / a);   else if t > 1: t = 1, s = clamp((b - c) / a)
 *     distance = |(P1 + d1 s) - (P2 + d2 t)|;   gap = (distance - r_i) - r_j.
 *   THE POINT-SEGMENT RULE of the target X: s = clamp(((X - P1) . d1) / a), s = 0 when not a > 0;
 *     distance = |X - (P1 + d1 s)|;  gap = distance - r_i.
 * TIES: among exactly equal gaps the lowest i wins, then the lowest j ((gap, i, j) compared lexicographically in the
 *   lanes and across the wave, no atomics): the answer does not depend on scheduling, and two calls on one state are
 *   bitwise equal.
 * NON-FINITE STATE: if any of nodes 0 .. n_elem of rod a is NaN or +-inf, every record of row a and of column a is
 *   NaN, NaN, -1, -1, NaN, NaN (the target record too, in an env that has a target); a non-finite target does the same
 *   to the target column only.  Other rods and other envs are not disturbed.  Every test is a comparison that is false
 *   for a NaN; no state is converted from float to int.
 * Asynchronous on `stream`, like softrod_rod_energies; it allocates and uploads nothing and is capturable.  It reads
 * the state (slots past a rod are never read) and writes `out` only.  Scope: every handle softrod_create accepts —
 * every env kind, 2 .. 126 elements, one- and two-slot rows, windowed long arms, tapered rods, every OctoFlat wave
 * shape.  Errors, each SOFTROD_EINVAL with its text in softrod_last_error, found before a device is looked for:
 * "rod clearance: null handle", "rod clearance: null output buffer", "rod clearance: self_gap must be 2 .. 126".    */
int softrod_rod_clearance(softrod_handle* h, int self_gap, double* out, void* stream);

/* Set rod shape: start resident envs from any strain field, on the device — the write side of softrod_rod_strains.
 * Upstream has no counterpart: its builds call CosseratRod.straight_rod only (soft_pendulum/build.py:54-61 and the
 * other build files), so every episode starts from a straight rod.  This is what randomised initial shapes (curled,
 * twisted, pre-stretched arms), exploring starts, curricula that begin near a goal pose and restarts from a pose
 * recorded with softrod_rod_strains need.  It is a RESET-TIME call: between a reset and the first step of the envs it
 * writes (the read-outs' instant reconstructs a mid-substep configuration for time != 0, which a teleported state
 * does not have; the library does not check this, the Python layer does).
 * For every env with mask != 0 (mask: device [n_envs] uint8, or NULL: every env) and every rod of it (rods_per_env as
 * for softrod_rod_energies) ONE cold kernel (csrc/softrod_shape.hpp, one wave per rod) KEEPS THE BASE POSE — node 0's
 * position and element 0's directors as they stand, so bc_targets, the head joints and the pendulum / moving-base
 * constraints stay consistent — and rebuilds the rest of the rod from device arrays in softrod_rod_strains' own
 * conventions, each float64, C-contiguous, or NULL: all zero
 *   kappa     [n_envs][rods_per_env][3][n_elem - 1]  material frame, NOT reduced by rest curvature:
 *             Q_{k+1} = exp(-[kappa_k D^]x) Q_k  with Q's rows the directors, [a]x b = a x b and D^ the rest Voronoi
 *             length — the inverse of what softrod_rod_strains reports, kappa = -log(Q_{k+1} Q_k^T) / D^
 *   sigma     [n_envs][rods_per_env][3][n_elem]      x_{k+1} - x_k = l^ Q_k^T (sigma_k + e3), l^ the rest length
 *   velocity  [n_envs][rods_per_env][3][n_elem + 1]  lab frame, written as given
 *   omega     [n_envs][rods_per_env][3][n_elem]      material frame, written as given
 * With all four NULL the rod becomes the straight, unstretched rod at rest along the base director d3.
 * The rotation of every Voronoi vertex is exact (Rodrigues, libm sin / cos; a series below |kappa D^|^2 = 1e-6); the
 * products along the rod are a wave scan in a fixed order: two calls with the same arguments are bitwise equal.
 * WHAT FOLLOWS FROM THE SHAPE is derived again with reset's statements: `tangents` (unit, reset's division with
 * eps_length), `kappa` (what a force evaluation at this state caches), SOFTROD_ENV_ARM_SINGLE's prev_kappa_state
 * (`env_memory` = row 0 of that kappa) and prev_com_state (`control` rows 0-1).  SOFTROD_ENV_ARM_TWO's prev_kappa
 * moves in softrod_observe, as upstream's get_state moves it.
 * WHAT IS NOT TOUCHED: slot 0 of `position` and `director`, the slots past a rod's own (the ghost slots between packed
 * arms), rest_kappa, the muscle activations, the suckers, the rigid head, prev_action, time, bc_targets,
 * the per-env material and contact tables, and every array of an env with mask == 0 (bitwise).
 * Values are not validated: a NaN spoils its own rod only.  A planar SoftPendulum start needs kappa rows 0 and 2 and
 * sigma row 1 zero (row 1 of kappa, about d2, is the in-plane bend); otherwise the 3-D loop steps the rod.
 * Asynchronous on `stream`, like softrod_observe: no host synchronisation, no allocation, no upload; capturable.
 * Scope: every handle softrod_create accepts — every env kind, 2 .. 126 elements, one- and two-slot rows, packed arms.
 * The staged records of device-side auto-reset are straight rods: a later automatic reset does not repeat the shape
 * of THIS call.  Starts that every reset repeats, automatic ones included, are softrod_set_reset_shapes' (below).
 * Error, found before a device is looked for: SOFTROD_EINVAL "set rod shape: null handle".                           */
int softrod_set_rod_shape(softrod_handle* h, const double* kappa, const double* sigma, const double* velocity,
                          const double* omega, const uint8_t* mask, void* stream);

/* Reset shapes: shaped episode starts under EVERY reset — by hand, host-driven, NEXT_STEP and SAME_STEP on the device.
 * Upstream has no counterpart: its builds call CosseratRod.straight_rod only (soft_pendulum/build.py:54-61 and the
 * other build files), and softrod_set_rod_shape alone stops at the first episode end.  The handle keeps a resident POOL
 * of `count` start shapes; while one is set, every reset of an env leaves the env exactly as that reset followed by
 * softrod_set_rod_shape with one entry's fields leaves it, bit for bit (the same kernel shapes both, csrc/softrod_shape.hpp),
 * and the observation row the resetting call reports is the shaped start's.
 *
 * WHICH ENTRY does not depend on the mode: env e's reset number j (j counts from 0) starts from entry
 *   mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *   index = mix(mix(seed + 0x9E3779B97F4A7C15 * (e + 1)) + j) % count                      all uint64, mod 2^64
 * softrod_reset_shape_index is this function on the host: no handle, no device (count 0 gives 0).  Known answers:
 * seed 1, count 3, rows e = 0..5, columns j = 0..2: [[2,1,1],[2,2,1],[2,1,1],[0,2,2],[2,1,2],[1,2,0]].
 *
 *   softrod_set_reset_shapes(h, count, kappa, sigma, velocity, omega, seed, stream)
 *       device pointers in softrod_set_rod_shape's conventions with the entry axis in place of the env axis —
 *       kappa [count][rods_per_env][3][n_elem - 1], sigma [count][rods_per_env][3][n_elem], velocity
 *       [count][rods_per_env][3][n_elem + 1], omega [count][rods_per_env][3][n_elem], float64, C-contiguous — or NULL:
 *       all zero (count > 0 with all four NULL is a pool of straight starts).  The library COPIES them on `stream` into
 *       buffers it owns, allocated in this call and never inside a step: the caller's arrays may be released once the
 *       copy has run, and a captured graph sees stable pointers.  A call also sets every env's `index` to -1 and its
 *       `episode` to 0: a new pool starts a new sequence; it shapes nothing itself, so envs in mid-episode stay as
 *       they are and the pool takes effect at each env's next reset.  count == 0 clears the pool: starts are straight
 *       again and the steps launch nothing extra.  The call waits for the device where it releases an earlier pool.
 *       A graph captured before the call holds the old pool's pointers (or no pass at all): CAPTURE AGAIN after
 *       softrod_set_reset_shapes, as after softrod_autoreset_same_step.
 *   softrod_apply_reset_shapes(h, mask, stream)
 *       for the host-driven reset paths: call it right after softrod_reset* / softrod_reset_octo with the same envs
 *       (mask: DEVICE [n_envs] uint8, or NULL: every env), before softrod_observe.  For each env of the mask it draws
 *       index(e, episode[e]), shapes the env's rods from that entry, records the index and increments episode[e].
 *       Two kernels on `stream`; no synchronisation, allocation or upload; capturable.
 *   softrod_reset_shapes_view(h, &index, &episode)
 *       device pointers, valid for the handle's life once a pool has been set: index int32 [n_envs], the entry each
 *       env's current episode started from (-1: no shaped start yet) — what credits returns to start shapes —, and
 *       episode int32 [n_envs], the next reset's ordinal j.  The caller may write `episode` (the Python layer zeroes
 *       it for the envs a reset re-seeds, so that a seed reproduces the starts together with the base poses).
 *
 * THE DEVICE MODES need no call: while a pool is set softrod_step / softrod_step_packed launch the same pass for exactly
 * the envs the call's auto-reset pass restarted — under NEXT_STEP right behind that pass, in front of the step's first
 * dispatch; under SAME_STEP behind softrod_autoreset_same_step's pass; both outside the step's time stamps, so
 * softrod_kernel_times_ms keeps meaning the step.  The pass rewrites those envs' observation rows (dense or packed;
 * SOFTROD_ENV_SOFTPENDULUM3D's aux tilt; SOFTROD_ENV_ARM_TWO's prev_kappa moves as in any get_state); final_obs /
 * final_time / final_aux stay the finished step's.  An env that found no staged record did not restart: it is neither
 * shaped nor counted, and is shaped once a record arrives.  A manual reset in a device mode is shaped by
 * softrod_apply_reset_shapes alone.  Three small kernels per step, none without a pool (csrc/softrod_reset_shapes.hpp).
 * softrod_copy_envs copies an env's `index` and `episode` with the rest of it.  The pool itself is no part of the state
 * view.  Errors, each found before a device is looked for (SOFTROD_EINVAL): "set reset shapes: null handle", "set reset
 * shapes: negative count", "apply reset shapes: null handle", "apply reset shapes: no pool is set
 * (softrod_set_reset_shapes)", "reset shapes view: null handle", "reset shapes view: null argument", "reset shapes view:
 * no pool is set (softrod_set_reset_shapes)".                                                                         */
int softrod_set_reset_shapes(softrod_handle* h, int count, const double* kappa, const double* sigma, const double* velocity,
                             const double* omega, uint64_t seed, void* stream);
int softrod_apply_reset_shapes(softrod_handle* h, const uint8_t* mask, void* stream);
int softrod_reset_shapes_view(softrod_handle* h, int32_t** index, int32_t** episode);
uint32_t softrod_reset_shape_index(uint64_t seed, uint32_t env, uint32_t episode, uint32_t count);

/* EPISODE STATISTICS on the device: the return, length and end time of every episode that ends, and a ring of the last
 * `ring` finished episodes of the batch.  No reference counterpart: upstream has a single env and no statistics (a
 * single Gymnasium env takes gymnasium.wrappers.RecordEpisodeStatistics; that wrapper cannot wrap a batch of device
 * tensors, and in the device reset modes the host never sees which env finished on which call).  One cold kernel per
 * env.step, softrod_episode_stats_kernel (csrc/softrod_episode_stats.hpp says what it keeps and in which order), on the
 * caller's stream behind softrod_step.  softrod_step itself is unchanged and launches nothing for this: the update is
 * the caller's call, and nothing runs while the feature is off.
 *
 *   softrod_episode_stats_enable(h, ring)
 *       ring >= 1: allocates the resident arrays — acc_return f64, acc_length i32, latch u8, finished i32, the call's
 *       info rows ep_r f64, ep_l i32, ep_t f64, ep_mask u8, all [n_envs]; ring_r f64, ring_l i32, ring_t f64,
 *       ring_env i32, all [ring]; count u64 [1] — all zero.  On a handle that has them already they are released and
 *       allocated anew (the pointers of an earlier softrod_episode_stats_view die; a graph captured with the update in
 *       it must be captured again).  ring == 0: switches the feature off and releases them.  Waits for the device; not
 *       capturable.  softrod_destroy releases them too.  SOFTROD_ENOMEM / SOFTROD_EHIP leave the handle as it was.
 *   softrod_episode_stats_update(h, reward, terminated, truncated, end_time, mode, stream)
 *       one update from the outputs of the softrod_step before it: DEVICE reward f64 [n_envs], terminated and truncated
 *       u8 [n_envs], end_time f64 [n_envs] or NULL (t = 0) — the env clock row (softrod_state_view.time) in modes 0 and
 *       1, softrod_final_view's final_time in mode 2.  mode 0: the caller resets finished envs by hand (an env that
 *       finished is ignored until softrod_episode_stats_reset names it); 1: NEXT_STEP auto-reset (the call after an
 *       env's last step is its reset call and counts in no episode); 2: SAME_STEP auto-reset (the env's next episode
 *       starts with the next call).  Within a call the finished envs enter the ring in ascending env index; finished
 *       episode number c since enabling (0-based) is in slot c % ring.  One kernel of one workgroup: its cost grows
 *       with ceil(n_envs / 1024).  It only enqueues work — no allocation, synchronisation or host read: capturable.
 *   softrod_episode_stats_reset(h, mask, stream)
 *       mask: DEVICE u8 [n_envs], or NULL: every env.  Zeroes acc_return, acc_length, latch and the info rows of those
 *       envs: a manual reset discards a partial episode.  The ring, finished and count stay.  Capturable.
 *   softrod_episode_stats_view(h, &view)
 *       the device pointers, n_envs and ring; good until the next softrod_episode_stats_enable or softrod_destroy.
 * Errors, each SOFTROD_EINVAL and found before a device is looked for (a refused call changes nothing):
 *   "episode stats: null handle", "episode stats: ring <k> is negative",
 *   "episode stats: the feature is off (softrod_episode_stats_enable)" (update, reset, view),
 *   "episode stats: null reward, terminated or truncated", "episode stats: mode <m> is outside 0 .. 2",
 *   "episode stats: null argument" (view).                                                                          */
struct softrod_episode_stats_view {      /* a struct tag only: the entry point of the same name fills it */
    double* acc_return;
    int32_t* acc_length;
    uint8_t* latch;
    int32_t* finished;
    double* ep_r;
    int32_t* ep_l;
    double* ep_t;
    uint8_t* ep_mask;
    double* ring_r;
    int32_t* ring_l;
    double* ring_t;
    int32_t* ring_env;
    uint64_t* count;
    int32_t n_envs;
    int32_t ring;
};
int softrod_episode_stats_enable(softrod_handle* h, int ring);
int softrod_episode_stats_update(softrod_handle* h, const double* reward, const uint8_t* terminated, const uint8_t* truncated,
                                 const double* end_time, int mode, void* stream);
int softrod_episode_stats_reset(softrod_handle* h, const uint8_t* mask, void* stream);
int softrod_episode_stats_view(softrod_handle* h, struct softrod_episode_stats_view* out);

/* OBSERVATION AND REWARD NORMALISATION on the device: Gymnasium's RunningMeanStd kept per observation column and once
 * for the discounted return, the observations centred, scaled and clipped by it, the rewards scaled by the return's
 * deviation and clipped (no mean subtracted, as Stable-Baselines3's VecNormalize does).  No reference counterpart:
 * upstream has single envs, which take gymnasium.wrappers.NormalizeObservation / NormalizeReward; those cannot wrap a
 * batch of device tensors.  Cold kernels on the caller's stream behind softrod_step (csrc/softrod_normalize.hpp gives the
 * arithmetic, its fixed summation order and the row rules); softrod_step itself is unchanged and launches nothing for
 * this: the pass is the caller's call, and nothing runs while the feature is off.
 *
 *   softrod_normalize_enable(h, obs_on, reward_on, gamma, clip_obs, clip_reward, epsilon)
 *       allocates the resident arrays — the records mean, var, count, inv_std f64 [obs_dim] and one of each for the
 *       return, ret f64 [n_envs], latch u8 [n_envs], norm_obs f32 [n_envs][obs_dim], norm_final_obs f32
 *       [n_envs][obs_dim], norm_reward f64 [n_envs] — with every record at mean 0, var 1, count 1e-4 and everything
 *       else zero.  Called again it starts them anew (the pointers of an earlier softrod_normalize_view die; a graph
 *       captured with the pass in it must be captured again).  obs_on: the observation columns are kept and norm_obs /
 *       norm_final_obs written; reward_on: ret, the return's record and norm_reward.  Both 0: switches the feature off
 *       and releases the arrays.  Waits for the device; not capturable.  softrod_destroy releases them too.
 *       SOFTROD_ENOMEM / SOFTROD_EHIP leave the handle as it was.
 *   softrod_normalize_step(h, obs, reward, terminated, truncated, final_obs, mode, update, stream)
 *       one pass over the outputs of the softrod_step before it: DEVICE obs f32 [n_envs][obs_dim], reward f64 [n_envs],
 *       terminated and truncated u8 [n_envs], final_obs f32 [n_envs][obs_dim] (softrod_final_view) or NULL.  mode 0: the
 *       caller resets finished envs by hand; 1: NEXT_STEP auto-reset (the call after an env's last step is its reset
 *       call: its reward enters no return, its observation row is counted); 2: SAME_STEP auto-reset (final_obs rows of
 *       the envs that finished are normalised into norm_final_obs, never counted).  update 0: evaluation, the records,
 *       ret and latch stay and the outputs are still written.  The outputs use the records after this call's update.
 *       Two launches (one with update 0); no allocation, synchronisation or host read: capturable.
 *   softrod_normalize_reset(h, obs, mask, update, stream)
 *       the reset observation: DEVICE obs, DEVICE mask u8 [n_envs] or NULL (every env).  With update the masked envs'
 *       rows are counted; their ret and latch become zero; every row of norm_obs is written.  Capturable.
 *   softrod_normalize_view(h, &view)
 *       the device pointers and the settings; good until the next softrod_normalize_enable or softrod_destroy.
 *   softrod_normalize_load(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count, stream)
 *       HOST arrays f64 [obs_dim] and three HOST f64 scalars by pointer: sets the records and recomputes
 *       inv_std = 1 / sqrt(var + epsilon); ret and latch stay.  What a checkpointed policy carries its statistics with.
 *       Waits for the stream; not capturable.
 * Errors, each SOFTROD_EINVAL and found before a device is looked for (a refused call changes nothing); the checks of
 * the arguments come before those of the handle:
 *   "normalize: gamma <g> is outside [0, 1]", "normalize: clip_obs <c> is not positive",
 *   "normalize: clip_reward <c> is not positive", "normalize: epsilon <e> is not positive" (enable),
 *   "normalize: mode <m> is outside 0 .. 2", "normalize: null obs, reward, terminated or truncated",
 *   "normalize: final_obs needs mode 2" (step), "normalize: null obs" (reset), "normalize: null argument" (view, load),
 *   "normalize: null handle", "normalize: the feature is off (softrod_normalize_enable)" (step, reset, view, load).  */
struct softrod_normalize_view {          /* a struct tag only: the entry point of the same name fills it */
    double* obs_mean;
    double* obs_var;
    double* obs_count;
    double* obs_inv_std;
    double* ret_mean;
    double* ret_var;
    double* ret_count;
    double* ret_inv_std;
    double* ret;
    uint8_t* latch;
    float* norm_obs;
    float* norm_final_obs;
    double* norm_reward;
    int32_t n_envs;
    int32_t obs_dim;
    int32_t obs_on;
    int32_t reward_on;
    double gamma;
    double clip_obs;
    double clip_reward;
    double epsilon;
};
int softrod_normalize_enable(softrod_handle* h, int obs_on, int reward_on, double gamma, double clip_obs, double clip_reward,
                             double epsilon);
int softrod_normalize_step(softrod_handle* h, const float* obs, const double* reward, const uint8_t* terminated,
                           const uint8_t* truncated, const float* final_obs, int mode, int update, void* stream);
int softrod_normalize_reset(softrod_handle* h, const float* obs, const uint8_t* mask, int update, void* stream);
int softrod_normalize_view(softrod_handle* h, struct softrod_normalize_view* out);
int softrod_normalize_load(softrod_handle* h, const double* obs_mean, const double* obs_var, const double* obs_count,
                           const double* ret_mean, const double* ret_var, const double* ret_count, void* stream);

/* Run `n` bare PositionVerlet substeps with fixed per-env forcing inputs and no
 * env epilogue (the inner loop of soft_pendulum.py:183-184 alone); `actions`
 * (device [n_envs] float32 or NULL) feeds SOFTROD_FEAT_POINT_FORCE_NODE0_X.
 * Used by the known-answer tests and by the kernel micro-benchmarks.        */
int softrod_substeps(softrod_handle* h, const float* actions, int n, void* stream);

/* Raw device pointers to the resident state.  On a handle with planar certificates (below) the call switches them off
 * for good (the first such call waits for the device): the caller may write through these pointers at any later time,
 * so from here on every launch proves planarity again.  Only softrod_set_planar_certificates(h, 1) switches them back
 * on.                                                                                                                  */
int softrod_state_view_get(softrod_handle* h, softrod_state_view* out);

/* PLANAR CERTIFICATES — SOFTROD_ENV_SOFTPENDULUM with SOFTROD_FEATURES_SOFTPENDULUM under SOFTROD_MATH_FAST only; on
 * every other handle both calls succeed and do nothing (softrod_planar_certificates writes zeros).
 *
 * The SoftPendulum step kernels take their planar substep loop after proving, at every launch, that the rod lies in the
 * x-y plane: eighteen state rows loaded, eleven of them only to be compared with constants.  The state a planar step
 * leaves behind is planar again, exactly, until somebody else writes it.  So the kernel leaves one byte per env —
 * 0 unknown, 1 certified planar with d2_z > 0, 2 with d2_z < 0 — and a launch that finds it set loads the seven rows
 * of the planar state and skips the proof (csrc/softrod_planar.hpp says what a certificate vouches for and why the
 * results are the same bits).  An env that takes the 3-D loop, holds a NaN or is launched with zero substeps loses its
 * certificate.  Every other writer of an env's rows or boundary-condition targets withdraws certificates:
 *   softrod_reset / softrod_reset_straight (full or masked), softrod_set_rod_shape, softrod_apply_reset_shapes
 *                          all of them, on the call's stream;
 *   the NEXT_STEP and SAME_STEP auto-reset passes, with or without a pool of reset shapes
 *                          those of the envs they restart, inside their kernels;
 *   softrod_copy_envs, softrod_bank_save, softrod_bank_load
 *                          copy the byte with the rows it vouches for (a bank slot keeps its own);
 *   softrod_state_view_get all of them, and the feature goes off on this handle (above);
 *   a step by a kernel that does not know certificates (after softrod_set_radius_profile)
 *                          all of them, in front of it.
 * A caller that writes resident rows by any other means — through a view taken before certificates were switched back
 * on, say — must switch them off first.
 *
 *   softrod_set_planar_certificates(h, on)
 *       default: on.  Waits for the device and withdraws every certificate.  on = 0: from the next launch on the kernels
 *       neither read nor write one and run the proof at every launch.  on != 0: they issue and trust them again.
 *       Synchronous; not capturable.  The switch lives in device memory and the kernels read it at every launch, so a
 *       graph captured earlier follows it (and follows softrod_state_view_get's switching off).
 *   softrod_planar_certificates(h, out, stream)
 *       copies the bytes, uint8 [n_envs], to DEVICE memory `out` on `stream` (diagnostics and tests).
 * Errors (SOFTROD_EINVAL): "set planar certificates: null handle", "planar certificates: null argument".             */
int softrod_set_planar_certificates(softrod_handle* h, int on);
int softrod_planar_certificates(softrod_handle* h, uint8_t* out, void* stream);

/* Kernel timing with one pair of HIP events per softrod_step / softrod_substeps
 * call, attached to the call's own kernel dispatches (start: begin of its first
 * kernel; stop: end of its last): no packet in front of or behind the kernels and
 * no host synchronisation, so a timed launch costs what an untimed one costs and
 * a duration is the kernels' own, first begin to last end.  Switch it off before
 * capturing a graph (the events are not part of one).
 *   softrod_set_timing(h, n)      n > 0: keep event pairs for the next n launches
 *                                 (ring restarts at 0); n = 0: off (default).
 *   softrod_kernel_times_ms(...)  synchronises on the recorded events and writes
 *                                 the per-launch durations, oldest first; *count
 *                                 receives how many were written (<= cap).
 *   softrod_last_kernel_ms(...)   duration of the most recent timed launch.    */
int softrod_set_timing(softrod_handle* h, int n_launches);
int softrod_kernel_times_ms(softrod_handle* h, float* out_ms, int cap, int* count);
int softrod_last_kernel_ms(softrod_handle* h, float* ms);

/* Which step-kernel tier softrod_step launches for this handle, as a short stable string: the
 * kernel template's name, its specialisation and the workgroup shape, e.g.
 * "softrod_step_fast_kernel<SoftPendulum,epl=1>" or "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>".
 * The tier follows from softrod_config alone.  The A/B switches of the measurement builds
 * (SOFTROD_NO_WINDOW, SOFTROD_WINDOW_PAIRED, SOFTROD_WINDOW_REFRESH) are honoured by softrod_create ONLY when SOFTROD_DEBUG_SWITCHES=1 is set as
 * well, so a stray variable cannot change what a product process runs; this call is how a host (and
 * tests/test_gpu_debug_switches.py) sees the outcome.  No reference counterpart (ABI v15).        */
const char* softrod_kernel_tier(softrod_handle* h);

const char* softrod_last_error(softrod_handle* h);
int softrod_destroy(softrod_handle* h);
int softrod_abi_version(void);
/* First 16 hex digits of the SHA-256 over the sources this library was built from (the .hpp files of csrc/ in
 * name order, softrod_capi.hip, include/softrod.h; the Makefile passes it as SOFTROD_SOURCE_HASH).
 * Profiles record it, and bench.py refuses to price a kernel against instruction counts / traffic
 * measured on a different build (profiles/valu_counts.json, hbm_traffic.json).  No reference
 * counterpart: measurement plumbing.                                                            */
const char* softrod_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* SOFTROD_H */
