// softrod_capi.hip — host side of the C-ABI declared in include/softrod.h.
//
// Owns the resident device state of one batch shard and launches the kernels of
// softrod_kernels.hpp.  No CPU implementation of the physics lives here: the only
// host arithmetic is the rod *allocation* (CosseratRod.straight_rod constants and the
// initial frame of each rod, build.py:46-61), which the reference also performs once
// per reset on the host.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "softrod_kernels.hpp"
#include "softrod_dynamics_readout.hpp"
#include "softrod_copy_envs.hpp"
#include "softrod_state_bank.hpp"
#include "softrod_episode_stats.hpp"
#include "softrod_normalize.hpp"
#include "softrod_shape.hpp"
#include "softrod_reset_shapes.hpp"
#include "softrod_owned.hpp"

using namespace softrod;

// Every resource below is an owner of softrod_owned.hpp, or a struct or vector of them: one struct per feature, which
// a set-up builds locally and moves into the handle once nothing can fail any more.  Dropping a feature is assigning
// a fresh value of its struct.

// One per-env table (set_env_table), empty until the first call: dev [N]; host pinned [N], every row as last uploaded
template <class Row>
using EnvTable = Upload<Row>;

// The state bank (softrod_bank_create): a twin with `slots` rows of every array copy_table(h) lists, keyed by the
// batch array it twins, so that the bank's table is the batch's with the bases swapped (bank_table).
struct StateBank {
    int slots = 0;                  // 0: the handle has no bank
    struct Twin { const void* of; DeviceBuf<unsigned char> dev; };
    std::vector<Twin> twins;        // `of`: the batch array's base
    std::vector<uint8_t> filled;    // [slots] the slot holds a saved state
    std::vector<uint8_t> seen;      // [max(N, slots)] scratch of the validation, all zero between calls
    std::vector<EnvMaterial> mat;   // [slots] the slot's row of env_mat.host, where that table exists
    std::vector<EnvContact> contact;    // [slots] the same for env_contact.host
    Upload<int2> pairs;             // [max(N, slots)] the (from, to) pairs of a call on their way to the device
    unsigned char* twin_of(const void* base) const {
        for (const Twin& t : twins) if (t.of == base) return t.dev.get();
        return nullptr;
    }
};

// Reset staging (softrod_create): the start records and the mask of a masked reset on their way to the device
struct ResetStaging {
    Upload<double> init;            // [N][init_stride]; init.ev guards reuse of both pinned buffers
    DeviceBuf<uint8_t> d_mask;      // [N]
    PinnedBuf<uint8_t> h_mask;      // [N]
};

// Device-side auto-reset (softrod_autoreset_enable)
struct ResetQueue {
    int depth = 0;                  // 0: off
    Upload<double> ring;            // [depth][N][init_stride] and its pinned mirror; ring.ev guards reuse of the mirror and h_produced
    DeviceBuf<int> d_consumed;      // [N]
    DeviceBuf<int> d_produced;      // [N]
    DeviceBuf<int> d_underflow;     // [1]
    DeviceBuf<uint8_t> d_flags;     // [2][N]: needs_reset, skip
    PinnedBuf<int> h_produced;      // [N]
    PinnedBuf<double> h_stage;      // the pending records, compacted
    PinnedBuf<int2> h_where;
    DeviceBuf<double> d_stage;
    DeviceBuf<int2> d_where;
    size_t stage_cap = 0;           // records the staging buffers hold
    PinnedBuf<int> h_status;        // [N + 1]: consumed, underflow (softrod_queue_status_begin)
    Event ev_status;
};

// Same-step auto-reset (softrod_autoreset_same_step): allocated by the first call that switches it on and kept through
// on = 0, so that the pointers softrod_final_view hands out stay good for the handle's life
struct FinalRows {
    DeviceBuf<float> obs;           // [N][obs_dim] the finished step's observation
    DeviceBuf<double> time;         // [N] the finished episode's clock
    DeviceBuf<double> aux;          // [N] the finished step's aux value (SoftPendulum3D's tilt)
};

// Shaped starts (softrod_set_reset_shapes): the pool is replaced by every call that sets one; the three rows are
// allocated by the first and kept for the handle's life, so that softrod_reset_shapes_view's pointers stay good
struct ResetShapes {
    int count = 0;                  // entries of the pool; 0: none set
    unsigned long long seed = 0;
    DeviceBuf<double> field[4];     // kappa, sigma, velocity, omega [count][rods][3][..] or empty
    DeviceBuf<int> index;           // [N] the entry each env's current episode started from, -1: none
    DeviceBuf<int> episode;         // [N] resets counted = the next reset's ordinal
    DeviceBuf<uint8_t> picked;      // [N] scratch of the pass: the envs it shapes
};

struct softrod_handle {
    softrod_config cfg;
    int device = 0;
    int epl = 1;            // nodes/elements per lane: 1 (n_elem <= 63) or 2 (<= 126)
    int nw = 1;             // wavefronts per env: 1, or ceil(n_arm*seg/64) for OctoFlat
    size_t init_stride = 18;  // doubles of reset staging per env
    int window_refresh = 0;   // > 0: the rod runs on two overlapping wave windows (softrod_window.hpp),
                              // halo refreshed every so many substeps
    bool window_paired = true;            // A/B switch SOFTROD_WINDOW_PAIRED=0: one rod per workgroup with s_barrier
    std::string tier;                     // softrod_kernel_tier
    RodParams P{};
    StatePtrs S{};
    // every device buffer that lives as long as the handle: what softrod_create allocates into the raw pointers below
    // and into S, and softrod_set_radius_profile's table
    std::vector<DeviceBuf<unsigned char>> owned;
    ResetStaging reset;
    double* d_basis = nullptr;    // [(n_elem-1)][7] action basis (zero until set)
    double* d_spline = nullptr;   // breaks[MAX_PIECES + 1], coef[pieces][n_ctrl][4] (softrod_set_spline_table)
    bool spline_set = false;
    RodParams* d_params = nullptr;  // device copy of P
    StatePtrs* d_state = nullptr;   // device copy of S (re-uploaded whenever S changes)
    double* d_time_tab = nullptr;   // clock after k env.steps from a reset (clock_after, softrod_fast.hpp)
    double* d_mat = nullptr;        // [kMatRows][64 * epl] material table of a tapered rod
    double* d_render_radius = nullptr;  // [n_elem] rest radius of every element, for softrod_render and
                                        // softrod_rod_clearance: base_radius, or the profile of softrod_set_radius_profile
    double* d_mtab = nullptr;       // [SOFTROD_MAX_MUSCLES][4][64 * epl] ratio_position x, y, z, strength
    bool muscles_set = false;
    unsigned* d_ticket = nullptr;   // softrod_scatter_rows: blocks that have finished storing (tagged form)
    bool tapered = false;
    bool was_reset = false;
    bool basis_set = false;
    std::vector<Event> ev_start, ev_stop;   // timing ring (softrod_set_timing)
    int timed = 0;                  // launches recorded since set_timing
    ResetQueue q;                   // softrod_autoreset_enable
    std::vector<int> seen_consumed; // as of the last softrod_queue_status
    std::vector<int2> pending;      // (env, slot) written into q.ring.host since the last commit
    bool status_pending = false;
    bool same_step = false;         // softrod_autoreset_same_step
    FinalRows final;
    ResetShapes rs;                 // softrod_set_reset_shapes
    EnvTable<EnvMaterial> env_mat;      // softrod_set_env_material
    EnvTable<EnvContact> env_contact;   // softrod_set_env_contact
    Upload<int2> pairs;             // [N] softrod_copy_envs: the (src, dst) pairs of a call on their way to the device
    std::vector<uint8_t> is_dst;    // [N] scratch of its validation, all zero between calls
    StateBank bank;                 // softrod_bank_create
    // episode statistics (softrod_episode_stats_enable): one device block carved into the arrays of EpisodeStats
    EpisodeStats stats{};           // stats.ring == 0: off
    DeviceBuf<unsigned char> d_stats;   // the block
    // observation / reward normalisation (softrod_normalize_enable): one device block carved into the arrays of NormState
    NormState norm{};               // norm.rec == nullptr: off
    DeviceBuf<unsigned char> d_norm;    // the block
    // failure injection of the set-ups (arm_setup, SR_SETUP): 0 in production
    const char* setup_name = "";    // the entry point that armed it
    int setup_fail_at = 0;          // > 0: the set-up call of this ordinal is not made and fails
    int setup_calls = 0;            // set-up calls counted since it was armed
    // planar certificates (StatePtrs.planar_cert, softrod_planar.hpp)
    bool cert_on = true;            // softrod_set_planar_certificates; softrod_state_view_get switches it off for good
    bool cert_live = false;         // a launch since the last clear may have issued certificates
    std::string err;
};

namespace {

thread_local std::string g_err;  // errors raised before a handle exists

int fail(softrod_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_err = msg;
    return code;
}

// Every entry point runs on the handle's device and leaves the caller's current device as it
// found it (a process may hold handles on several GPUs, or have torch's current device elsewhere).
struct DeviceGuard {
    int prev = -1, want = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) : want(device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != want) err = hipSetDevice(want);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define SR_ON_DEVICE(h)                                                                  \
    DeviceGuard guard_((h)->device);                                                     \
    if (guard_.err != hipSuccess)                                                        \
        return fail(h, SOFTROD_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

#define SR_HIP(h, call)                                                                 \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(h, SOFTROD_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- set-ups: the entry points that allocate after softrod_create ----
// A set-up builds what it needs in local owners (softrod_owned.hpp), makes every fallible call through SR_SETUP, and
// touches the handle, h->S, the bank and d_state only after the last of them has succeeded — the StatePtrs upload, where
// there is one, is that last call.  An early return is therefore always clean: the locals release what was made, the
// handle is as it was, and the call can be repeated.
//
// Failure injection (tests/test_gpu_debug_switches.py): SOFTROD_DEBUG_FAIL_SETUP_CALL=k, honoured only with
// SOFTROD_DEBUG_SWITCHES=1, makes the k-th SR_SETUP call of a set-up fail without being made.  Each set-up arms the
// counter at its top; nothing is read from the environment while the gate is off, and nothing on the step path.
void arm_setup(softrod_handle* h, const char* entry_point) {
    const char* dbg = std::getenv("SOFTROD_DEBUG_SWITCHES");
    const char* k = (dbg && dbg[0] == '1') ? std::getenv("SOFTROD_DEBUG_FAIL_SETUP_CALL") : nullptr;
    h->setup_name = entry_point;
    h->setup_fail_at = k ? std::atoi(k) : 0;
    h->setup_calls = 0;
}
// What a failed set-up call returns.  Without `prefix`: SR_HIP's text and code.  With one: the entry point's own text;
// oom_is_enomem: hipErrorOutOfMemory is SOFTROD_ENOMEM.
int setup_error(softrod_handle* h, hipError_t e, const char* call, const char* prefix = nullptr, bool oom_is_enomem = false) {
    if (!prefix) return fail(h, SOFTROD_EHIP, std::string(call) + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    return fail(h, oom_is_enomem && e == hipErrorOutOfMemory ? SOFTROD_ENOMEM : SOFTROD_EHIP, std::string(prefix) + hipGetErrorString(e));
}
#define SR_SETUP(h, call, ...)                                                                              \
    do {                                                                                                    \
        if ((h)->setup_fail_at > 0 && ++(h)->setup_calls == (h)->setup_fail_at)                             \
            return fail(h, SOFTROD_EHIP, std::string((h)->setup_name) + ": injected failure at call " +     \
                                             std::to_string((h)->setup_calls));                             \
        if (const hipError_t e_ = (call)) return setup_error(h, e_, #call, ##__VA_ARGS__);                  \
    } while (0)

// Sizes in, one zeroed device block and the offsets out: arrays of `sizes` bytes in that order, each at a multiple of
// 256 bytes of `block` (two set-up calls; failures in the words of `what`).
int carve_block(softrod_handle* h, const char* what, const std::vector<size_t>& sizes, DeviceBuf<unsigned char>& block,
                std::vector<size_t>& at) {
    size_t bytes = 0;
    for (const size_t n : sizes) { at.push_back(bytes); bytes += (n + 255) & ~(size_t)255; }
    SR_SETUP(h, block.alloc(bytes), what, true);
    SR_SETUP(h, hipMemset(block.get(), 0, bytes), what, true);
    return SOFTROD_OK;
}

// Constants of a uniform straight rod — CosseratRod.straight_rod
// (elastica/rod/factory_function.py allocate(), called at build.py:54-61) and
// AnalyticalLinearDamper.__init__ (build.py:108-113).
void fill_params(const softrod_config& c, RodParams& P) {
    std::memset(&P, 0, sizeof(P));
    P.n_envs = c.n_envs;
    P.n_elem = c.n_elem;
    P.time_two_half_adds = c.time_two_half_adds;
    P.features = c.features;
    P.env_kind = c.env_kind;
    P.filter_order = c.filter_order;
    P.damp_before_constrain = c.damp_before_constrain;
    P.dt = c.dt;
    P.half_dt = 0.5 * c.dt;
    P.final_time = c.final_time;
    const int n = c.n_elem;
    const double rest_len = c.base_length / (double)n;
    P.rest_len = rest_len;
    P.inv_rest_len = 1.0 / rest_len;
    P.rest_vor = 0.5 * (rest_len + rest_len);
    P.inv_rest_vor = 1.0 / P.rest_vor;
    const double r = c.base_radius;
    const double A0 = M_PI * r * r;
    const double I1 = A0 * A0 / (4.0 * M_PI);
    const double I[3] = {I1, I1, 2.0 * I1};
    for (int i = 0; i < 3; ++i) {
        P.J[i] = I[i] * (c.density * rest_len);
        P.invJ[i] = 1.0 / P.J[i];
    }
    P.shear[0] = c.alpha_c * c.shear_modulus * A0;
    P.shear[1] = c.alpha_c * c.shear_modulus * A0;
    P.shear[2] = c.youngs_modulus * A0;
    P.bend[0] = c.youngs_modulus * I[0];
    P.bend[1] = c.youngs_modulus * I[1];
    P.bend[2] = c.shear_modulus * I[2];
    const double volume = M_PI * (r * r) * rest_len;
    P.mass_node = c.density * volume;  // two half-element contributions
    for (int i = 0; i < 3; ++i) { P.gravity[i] = c.gravity[i]; P.tip_force[i] = c.tip_force[i]; }
    // AnalyticalLinearDamper(time_step=...): the stepper's dt unless the build hands it another one
    // (build_muscle_octopus.py:101-106: 7e-5 under a stepper run at 5e-5)
    const double ddt = c.damper_time_step > 0.0 ? c.damper_time_step : c.dt;
    P.damp_t = std::exp(-c.damping_constant * ddt);
    // element mass seen by the damper: 0.5(m_k+m_{k+1}), ends augmented by half their
    // outer node -> rho*V for every element of a uniform rod
    const double me = P.mass_node;
    for (int i = 0; i < 3; ++i) {      // (damper_protocol 1: the uniform protocol, the same exp(-nu dt) on every rate)
        P.damp_logr[i] = c.damper_protocol == 1 ? -c.damping_constant * ddt : -c.damping_constant * ddt * me * P.invJ[i];
        P.damp_r[i] = std::exp(P.damp_logr[i]);
    }
    P.eps_length = c.eps_length;
    P.eps_rot_axis = c.eps_rot_axis;
    P.acos_shift = c.acos_shift;
    P.eps_sin = c.eps_sin;
    P.two_acos_shift = 2.0 * c.acos_shift + 1.0e-200;
    P.neg_eps_sin = -c.eps_sin;
    P.base_limit = c.base_limit;
    P.step_time = (double)c.n_substeps * c.dt;  // step_skip * time_step, soft_pendulum_3d.py:110-112
    P.base_step = (float)c.base_step;
    // OctoArmSingle-v0
    P.control_penalty_coeff = (float)c.control_penalty_coeff;
    P.contact_before_forcing = c.contact_before_forcing;
    P.n_action = 7;
    {   // mass.sum() in the order compute_position_center_of_mass adds it
        double ms = 0.0;
        for (int k = 0; k <= n; ++k) ms += (k == 0 || k == n) ? 0.5 * P.mass_node : P.mass_node;
        P.mass_total = ms;
    }
    for (int i = 0; i < 2; ++i) {
        P.target[i] = c.target[i];
        P.kappa_range[i] = c.kappa_range[i];
        P.kappa_rate_range[i] = c.kappa_rate_range[i];
    }
    for (int i = 0; i < 3; ++i) {
        P.plane_origin[i] = c.plane_origin[i];
        P.plane_normal[i] = c.plane_normal[i];
        P.kin_mu[i] = c.kinetic_mu[i];
        P.stat_mu[i] = c.static_mu[i];
    }
    P.contact_k = c.contact_k;
    P.contact_nu = c.contact_nu;
    P.slip_tol = c.slip_velocity_tol;
    P.surface_tol = c.surface_tol;
    P.r0_sqrt_rest_len = r * std::sqrt(rest_len);   // radius = sqrt(V/(pi l)) = r0 sqrt(l_rest/l)
    if ((c.features & SOFTROD_FEAT_PLANE_CONTACT_ANISO) && c.plane_normal[0] == 0.0 &&
        c.plane_normal[1] == 0.0 && c.plane_normal[2] == 1.0)
        P.features |= kFeatPlaneZup;   // what both reference builds use (octopus/build.py:233)
    if (c.features & SOFTROD_FEAT_OCTO_HEAD) {
        // arms `seg` slots apart; Cylinder(length = 2 r0, radius = head_radius, density)
        // (octopus/build.py:95-105; elastica/rigidbody/cylinder.py)
        P.seg_shift = n <= 15 ? 4 : (n <= 31 ? 5 : 6);
        P.seg = 1 << P.seg_shift;
        P.n_arm = c.n_arm;
        P.n_action = c.n_knots;
        if (c.env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT) P.seg_shift = 6, P.seg = 64;    // the muscle arm with a weight: one arm, one wave
        P.head_fixed = c.head_fixed;
        const double hl = c.head_length > 0.0 ? c.head_length : 2.0 * c.base_radius, hr = c.head_radius;
        for (int i = 0; i < 3; ++i) P.head_center[i] = c.head_length > 0.0 ? c.head_center[i] : 0.0;
        P.joint_angle0 = c.head_length > 0.0 ? c.joint_angle0 : 0.0;
        P.joint_angle_step = c.head_length > 0.0 ? c.joint_angle_step : 360 / (double)c.n_arm;
        const double harea = M_PI * hr * hr;
        P.head_mass = (M_PI * hr * hr * hl) * c.head_density;
        const double s1 = harea * harea / (4.0 * M_PI);
        const double smoa[3] = {s1, s1, 2.0 * s1};
        for (int i = 0; i < 3; ++i) {
            P.head_invJ[i] = 1.0 / (smoa[i] * c.head_density * hl);
        }
        P.head_radius = hr;
        P.joint_k = c.joint_k;
        P.joint_nu = c.joint_nu;
        P.joint_kt = c.joint_kt;
    }
    // SoftArmTracking-v0
    P.n_ctrl = c.n_ctrl;
    P.n_pieces = c.n_spline_pieces;
    P.muscle_scale = c.muscle_torque_scale;
    P.max_rate = c.max_activation_rate;
    P.base_length = c.base_length;
    for (int i = 0; i < 3; ++i) P.arm_target[i] = c.arm_target[i];
    P.n_suckers = c.n_suckers;
    for (int j = 0; j < SOFTROD_MAX_SUCKERS; ++j) P.sucker_index[j] = c.sucker_index[j];
    if (c.early_termination) P.features |= kFeatEarlyTerm;
    P.sucker_ratio0 = c.sucker_reduction_ratio;
    // COOMM muscle layers
    P.n_muscles = (c.features & SOFTROD_FEAT_COOMM_MUSCLES) ? c.n_muscles : 0;
    for (int m = 0; m < SOFTROD_MAX_MUSCLES; ++m) P.muscle_kind[m] = c.muscle_kind[m];
    P.fl_degree = c.muscle_fl_degree;
    for (int k = 0; k < SOFTROD_MAX_FL_COEF; ++k) P.fl_coef[k] = c.muscle_fl_coef[k];
    P.muscle_form = c.muscle_equiv_load_form;
    P.muscle_cur_radius = c.muscle_position_current_radius;
    P.muscle_tm_law = c.muscle_tm_length_law;
    P.push_mode = c.arm_push_mode;
}

bool is_octo(const softrod_handle* h) { return (h->cfg.features & SOFTROD_FEAT_OCTO_HEAD) != 0; }
// the rigid-body set whose host API is FlatEnv's (softrod_reset_octo, softrod_queue_push_octo); the muscle arm with a
// weight (SOFTROD_ENV_ARM_PULL_WEIGHT) runs the same kernels but resets like any single rod (softrod_reset_straight)
bool is_flat(const softrod_handle* h) { return h->cfg.env_kind == SOFTROD_ENV_OCTO_FLAT; }
bool is_pull(const softrod_handle* h) { return h->cfg.env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT; }
// the muscle octopus envs (softrod_mocto.hpp): FlatEnv's host API (arm frames + target), the muscle arm's tables
bool mocto_kind(int e) { return e == SOFTROD_ENV_CRAWL || e == SOFTROD_ENV_ARM_TWO || e == SOFTROD_ENV_REACH; }
bool is_mocto(const softrod_handle* h) { return mocto_kind(h->cfg.env_kind); }
// Which kernel a cold pass launches: the body one (a workgroup of kLanes * nw threads per env) or the one-rod one (a
// 64-lane block per env).  Two rules on purpose: the muscle arm with a weight restarts as a body (octo_reset_env resets
// its weight with it) but observes as the single rod it is (softrod_observe_kernel's push_get_state_n).
bool restarts_as_body(const softrod_handle* h) { return is_octo(h); }
bool observes_as_body(const softrod_handle* h) { return is_mocto(h) || (is_octo(h) && !is_pull(h)); }
// the one- or the two-slot instantiation of a kernel, by the handle's slots per lane
template <class K> K by_epl(const softrod_handle* h, K one, K two) { return h->epl == 2 ? two : one; }
// Where a handle's rods lie in its resident rows (softrod_state_view): rods per env, the width of an env's row,
// the slots between two arms of an env.
struct RodLayout { int rods, lane_stride, arm_stride; };
RodLayout rod_layout(const softrod_handle* h) {
    const bool arms = is_flat(h) || is_mocto(h);
    return {arms ? h->cfg.n_arm : 1, kLanes * h->epl * h->nw, arms ? h->P.seg : 0};
}
// One row of the per-env table: fill_params itself on the config with this env's (E, G, rho, nu).
void env_material_row(const softrod_config& c, const double m[4], EnvMaterial& R) {
    softrod_config ci = c;
    ci.youngs_modulus = m[0];
    ci.shear_modulus = m[1];
    ci.density = m[2];
    ci.damping_constant = m[3];
    RodParams Q;
    fill_params(ci, Q);
    std::memset(&R, 0, sizeof(R));
    for (int i = 0; i < 3; ++i) {
        R.J[i] = Q.J[i]; R.invJ[i] = Q.invJ[i]; R.shear[i] = Q.shear[i]; R.bend[i] = Q.bend[i];
        R.damp_r[i] = Q.damp_r[i]; R.damp_logr[i] = Q.damp_logr[i];
    }
    R.mass_node = Q.mass_node; R.mass_total = Q.mass_total; R.damp_t = Q.damp_t;
}
// One row of the per-env contact table from (k, nu, kinetic_mu[3], static_mu[3]): the means and half differences with
// contact_params()' operations, so that the config's own values give the kernels' doubles bit for bit.
void env_contact_row(const double c[8], EnvContact& R) {
    std::memset(&R, 0, sizeof(R));
    R.k = c[0];
    R.nu = c[1];
    for (int i = 0; i < 3; ++i) { R.kin_mu[i] = c[2 + i]; R.stat_mu[i] = c[5 + i]; }
    R.kin_am[0] = 0.5 * (R.kin_mu[0] + R.kin_mu[1]); R.kin_am[1] = 0.5 * (R.kin_mu[0] - R.kin_mu[1]);
    R.stat_am[0] = 0.5 * (R.stat_mu[0] + R.stat_mu[1]); R.stat_am[1] = 0.5 * (R.stat_mu[0] - R.stat_mu[1]);
}

// Withdraw every planar certificate of the handle on `st`: what each host entry point that may write an env's rows or
// BC targets does first (cold paths all; the device passes clear the byte of the envs they restart inside their
// kernels).  `always` = false: only if a launch may have issued one since the last clear.
int clear_planar_certs(softrod_handle* h, hipStream_t st, bool always = true) {
    if (!h->S.planar_cert || !(always || h->cert_live)) return SOFTROD_OK;
    SR_HIP(h, hipMemsetAsync(h->S.planar_cert, 0, (size_t)h->cfg.n_envs, st));
    h->cert_live = false;
    return SOFTROD_OK;
}

// NEXT_STEP auto-reset pass in front of a step: finished envs restart instead of stepping
int launch_autoreset(softrod_handle* h, float* obs, double* reward, uint8_t* term, uint8_t* trunc, double* aux, int pack,
                     hipStream_t st) {
    const dim3 grid((unsigned)h->cfg.n_envs), block(kLanes * h->nw);
    if (restarts_as_body(h))
        hipLaunchKernelGGL(softrod_octo_autoreset_kernel, grid, block, 0, st, h->P, h->S, obs, reward, term, trunc, pack);
    else
        hipLaunchKernelGGL(by_epl(h, softrod_autoreset_kernel<1>, softrod_autoreset_kernel<2>), grid, block, 0, st, h->P, h->S,
                           obs, reward, term, trunc, aux, pack);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// SAME_STEP auto-reset pass behind a step (softrod_autoreset.hpp): envs the step just finished hand out their final
// observation and restart within the call
int launch_autoreset_same_step(softrod_handle* h, float* obs, double* aux, int pack, hipStream_t st) {
    const dim3 grid((unsigned)h->cfg.n_envs), block(kLanes * h->nw);
    if (restarts_as_body(h))
        hipLaunchKernelGGL(softrod_octo_autoreset_same_step_kernel, grid, block, 0, st, h->P, h->S, obs, pack, h->final.obs.get(),
                           h->final.time.get());
    else
        hipLaunchKernelGGL(by_epl(h, softrod_autoreset_same_step_kernel<1>, softrod_autoreset_same_step_kernel<2>), grid, block,
                           0, st, h->P, h->S, obs, aux, pack, h->final.obs.get(), h->final.time.get(), h->final.aux.get());
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// Shaped starts (softrod_reset_shapes.hpp), only while a pool is set: pick the envs this call restarted (`mode`: by
// the caller's mask, by the NEXT_STEP pass's skip flag, or by the SAME_STEP pass's flags), shape them from their pool
// entries with softrod_set_rod_shape's own kernel, and — with `obs` — rewrite their observation rows from the shaped
// state.  Kernels on `st` only: no synchronisation, no allocation, no upload.
int launch_reset_shapes(softrod_handle* h, int mode, const uint8_t* mask, float* obs, const uint8_t* term, const uint8_t* trunc,
                        double* aux, int pack, hipStream_t st) {
    const int N = h->cfg.n_envs;
    const ResetShapes& rs = h->rs;
    uint8_t* const picked = rs.picked.get();
    ResetShapesPick pick{};
    pick.index = rs.index.get(); pick.episode = rs.episode.get(); pick.picked = picked;
    pick.seed = rs.seed; pick.count = rs.count; pick.mode = mode; pick.mask = mask;
    pick.terminated = pack ? nullptr : term; pick.truncated = pack ? nullptr : trunc;
    pick.packed = (mode == kPickFinished && pack) ? obs : nullptr;
    pick.od = softrod_config_obs_dim(&h->cfg);
    hipLaunchKernelGGL(softrod_reset_shapes_pick_kernel, dim3((unsigned)((N + kPickThreads - 1) / kPickThreads)), dim3(kPickThreads),
                       0, st, h->P, h->S, pick);
    const RodLayout y = rod_layout(h);
    const RodShapeArgs args{rs.field[0].get(), rs.field[1].get(), rs.field[2].get(), rs.field[3].get(), picked, rs.index.get()};
    hipLaunchKernelGGL(by_epl(h, softrod_rod_shape_kernel<1>, softrod_rod_shape_kernel<2>), dim3((unsigned)(N * y.rods)),
                       dim3(kLanes), 0, st, h->P, h->S, y.rods, y.lane_stride, y.arm_stride, args);
    if (obs) {      // the kernel softrod_observe would launch for this handle, for the picked envs
        if (observes_as_body(h))
            hipLaunchKernelGGL(softrod_reset_shapes_octo_observe_kernel, dim3((unsigned)N), dim3(kLanes * h->nw), 0, st, h->P, h->S,
                               picked, obs, pack);
        else
            hipLaunchKernelGGL(by_epl(h, softrod_observe_kernel<1>, softrod_observe_kernel<2>), dim3((unsigned)N), dim3(kLanes), 0,
                               st, h->P, h->S, picked, nullptr, obs, aux, pack);
    }
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// ---- the step kernels: one table (kStepRows) decides what a handle runs, what it refuses and what its tier says ----
// What a handle may carry that a step kernel must not ignore, each by the bit that marks it in a kernel's feature mask:
// select_step() takes only a row that honours every option active on the handle.
enum : unsigned { kOptMuscles = SOFTROD_FEAT_COOMM_MUSCLES, kOptEarlyTerm = kFeatEarlyTerm, kOptEnvMaterial = kFeatEnvMaterial,
                  kOptEnvContact = kFeatEnvContact, kOptCompiledFor = kOptEarlyTerm | kOptEnvMaterial | kOptEnvContact };
constexpr int kAny = -1, kMoctoEnvs = -2;    // StepRow: every value / (env) the three muscle octopus envs
constexpr unsigned kAnyFeatures = kRuntimeFeatures;
using StepKernel = void (*)(RodParams, StatePtrs, const float*, float*, double*, uint8_t*, uint8_t*, double*, int, int, int);
using OctoKernel = void (*)(RodParams, StatePtrs, const float*, float*, double*, uint8_t*, uint8_t*, int, int, int);
using WindowKernel = void (*)(RodParams, StatePtrs, const float*, int, int);

struct StepRow {
    // when it applies
    unsigned feats;           // softrod_config.features, or kAnyFeatures
    int env;                  // softrod_config.env_kind, kAny or kMoctoEnvs
    int math, epl;            // SOFTROD_MATH_*; slots per lane
    int taper, zup;           // 0, 1 or kAny: softrod_set_radius_profile was called; the contact plane is e_z
    int nw_min, nw_max;       // waves per env
    bool windowed;            // env.step of a two-window handle (window_refresh > 0 and the epilogue asked for)
    unsigned needs, honours;  // options it is compiled FOR (the handle must have them) / honours (the handle may)
    StepKernel step; OctoKernel octo; WindowKernel window;    // exactly one of the three is set
    bool cert;                // `step` is a SoftPendulum planar kernel: it reads and issues planar certificates
    int epb, waves;           // launch shape: envs per workgroup, waves per workgroup (0: the handle's waves per env)
    const char* label;        // softrod_kernel_tier; {waves}: the handle's waves per env, {refresh}: its window_refresh
};

// The "when" and the options of an instantiation compiled for the feature mask F follow from F itself.
constexpr StepRow compiled_row(unsigned F, int env, int epl, int taper, int nw_min, int nw_max, const char* label) {
    const bool rt = F == kRuntimeFeatures;
    StepRow r{};
    r.feats = rt ? kAnyFeatures : F & ~(kFeatPlaneZup | kOptCompiledFor);
    r.env = env; r.math = SOFTROD_MATH_FAST; r.epl = epl; r.taper = taper; r.nw_min = nw_min; r.nw_max = nw_max;
    r.zup = rt ? kAny : (F & kFeatPlaneZup) != 0;
    r.needs = rt ? 0u : F & kOptCompiledFor;
    r.honours = rt ? 0u : F & (kOptCompiledFor | kOptMuscles);
    r.epb = 1; r.label = label;
    return r;
}
template <unsigned F, int E, int EPL, bool TAPER = false>
constexpr StepRow fast_row(const char* label) {
    StepRow r = compiled_row(F, E, EPL, TAPER, 1, 1, label);
    r.step = softrod_step_fast_kernel<F, E, EPL, TAPER>;
    r.cert = (F & ~kFeatEnvMaterial) == SOFTROD_FEATURES_SOFTPENDULUM;      // (kPlanarKernel)
    return r;
}
template <unsigned F, int MAXW, int EPB>
constexpr StepRow octo_row(int env, int nw_min, int nw_max, const char* label) {
    StepRow r = compiled_row(F, env, 1, kAny, nw_min, nw_max, label);
    r.octo = softrod_octo_step_kernel<F, MAXW, EPB>;
    r.epb = EPB; r.waves = EPB == 1 ? 0 : MAXW * EPB;
    return r;
}
template <unsigned F, int RPB>     // RPB rods per workgroup: 4 (a rod's two windows on one SIMD) or 1 (with s_barrier)
constexpr StepRow window_row(const char* label) {
    StepRow r = compiled_row(F, SOFTROD_ENV_ARM_SINGLE, 2, 0, 1, 1, label);
    r.window = softrod_step_window_kernel<F, RPB>;
    r.windowed = true; r.epb = RPB; r.waves = 2 * RPB;
    return r;
}
// The LIBM kernel evaluates any feature mix and reads the per-env tables at run time; the tables themselves exist for
// the uniform rods of the envs named here.
template <bool ET>
constexpr StepRow libm_row(unsigned feats, int env, int zup, int taper, unsigned honours) {
    StepRow r{};
    r.feats = feats; r.env = env; r.math = SOFTROD_MATH_LIBM; r.epl = 1; r.taper = taper; r.zup = zup;
    r.nw_min = r.nw_max = r.epb = 1;
    r.needs = ET ? kOptEarlyTerm : 0u; r.honours = r.needs | kOptMuscles | honours;
    r.step = softrod_step_libm_kernel<ET>;
    r.label = "softrod_step_libm_kernel";
    return r;
}

constexpr unsigned kArmSingleZup = SOFTROD_FEATURES_ARM_SINGLE | kFeatPlaneZup, kOctoFlatZup = SOFTROD_FEATURES_OCTO_FLAT | kFeatPlaneZup;
// One row per instantiation; the first row that serves a handle is its kernel, so the run-time-mask rows (custom
// feature mixes, known-answer tests) stand behind the specialised ones of their (epl, taper).
const StepRow kStepRows[] = {
    // the muscle arm with a weight, and the muscle octopus (action kernel | this | epilogue kernel, softrod_mocto.hpp)
    octo_row<SOFTROD_FEATURES_ARM_PULL_WEIGHT | kFeatEarlyTerm, 2, 1>(SOFTROD_ENV_ARM_PULL_WEIGHT, 1, 1, "softrod_octo_step_kernel<ArmPullWeight,1 wave,1 env/wg,taper>"),
    octo_row<SOFTROD_FEATURES_ARM_PULL_WEIGHT, 2, 1>(SOFTROD_ENV_ARM_PULL_WEIGHT, 1, 1, "softrod_octo_step_kernel<ArmPullWeight,1 wave,1 env/wg,taper>"),
    octo_row<SOFTROD_FEATURES_ARM_PULL_WEIGHT, 4, 1>(kMoctoEnvs, 1, 4, "softrod_mocto_action_kernel | softrod_octo_step_kernel<muscle arms,"
                                                                       "{waves},1 env/wg,taper> | softrod_mocto_epilogue_kernel"),
    // OctoFlat; the reference shape (two waves per env) runs four envs per workgroup, partner waves on one SIMD
    octo_row<kOctoFlatZup | kFeatEnvContact, 2, 4>(SOFTROD_ENV_OCTO_FLAT, 2, 2, "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>"),
    octo_row<kOctoFlatZup | kFeatEnvContact, 2, 1>(SOFTROD_ENV_OCTO_FLAT, 1, 1, "softrod_octo_step_kernel<zup,2 waves max,1 env/wg>"),
    octo_row<kOctoFlatZup, 2, 4>(SOFTROD_ENV_OCTO_FLAT, 2, 2, "softrod_octo_step_kernel<zup,2 waves,4 envs/wg>"),
    octo_row<kOctoFlatZup, 2, 1>(SOFTROD_ENV_OCTO_FLAT, 1, 1, "softrod_octo_step_kernel<zup,2 waves max,1 env/wg>"),
    octo_row<kOctoFlatZup, 8, 1>(SOFTROD_ENV_OCTO_FLAT, 3, 8, "softrod_octo_step_kernel<zup,8 waves max,1 env/wg>"),
    octo_row<SOFTROD_FEATURES_OCTO_FLAT, 2, 1>(SOFTROD_ENV_OCTO_FLAT, 1, 2, "softrod_octo_step_kernel<general plane,2 waves max,1 env/wg>"),
    octo_row<SOFTROD_FEATURES_OCTO_FLAT, 8, 1>(SOFTROD_ENV_OCTO_FLAT, 3, 8, "softrod_octo_step_kernel<general plane,8 waves max,1 env/wg>"),
    // OctoArmSingle of 64..102 elements: substeps on two overlapping one-node-per-lane windows (softrod_window.hpp), then
    // reward / observation by the two-slot row below with n_sub = 0
    window_row<kArmSingleZup, 4>("softrod_step_window_kernel<ArmSingle,4 rods/wg> refresh={refresh}"),
    window_row<kArmSingleZup, 1>("softrod_step_window_kernel<ArmSingle,1 rod/wg,s_barrier> refresh={refresh}"),
    fast_row<kArmSingleZup, SOFTROD_ENV_ARM_SINGLE, 2>("softrod_step_fast_kernel<ArmSingle,epl=2>"),
    // tapered rods (per-lane material constants): the ArmPush arm of 64..126 and of up to 63 elements, the tapered
    // OctoArmSingle (`bench.py --taper`), the damped arm with suckers of arm_push_env.py:160-196 without its muscles
    fast_row<SOFTROD_FEATURES_ARM_PUSH | kFeatEarlyTerm, SOFTROD_ENV_ARM_PUSH, 2, true>("softrod_step_fast_kernel<ArmPush,epl=2,taper>"),
    fast_row<SOFTROD_FEATURES_ARM_PUSH, SOFTROD_ENV_ARM_PUSH, 2, true>("softrod_step_fast_kernel<ArmPush,epl=2,taper>"),
    fast_row<kArmSingleZup, SOFTROD_ENV_ARM_SINGLE, 1, true>("softrod_step_fast_kernel<ArmSingle,epl=1,taper>"),
    fast_row<kFeaturesTaperedSuckerArm, SOFTROD_ENV_NONE, 1, true>("softrod_step_fast_kernel<damped sucker arm,epl=1,taper>"),
    fast_row<SOFTROD_FEATURES_ARM_PUSH | kFeatEarlyTerm, SOFTROD_ENV_ARM_PUSH, 1, true>("softrod_step_fast_kernel<ArmPush,epl=1,taper>"),
    fast_row<SOFTROD_FEATURES_ARM_PUSH, SOFTROD_ENV_ARM_PUSH, 1, true>("softrod_step_fast_kernel<ArmPush,epl=1,taper>"),
    fast_row<kRuntimeFeatures, kRuntimeEnv, 1, true>("softrod_step_fast_kernel<runtime mask,epl=1,taper>"),
    // uniform rods, two slots per lane, and the uniform muscle rod of the known-answer tests
    fast_row<SOFTROD_FEATURES_SOFTPENDULUM, SOFTROD_ENV_SOFTPENDULUM, 2>("softrod_step_fast_kernel<SoftPendulum,epl=2>"),
    fast_row<SOFTROD_FEATURES_SOFTPENDULUM3D, SOFTROD_ENV_SOFTPENDULUM3D, 2>("softrod_step_fast_kernel<SoftPendulum3D,epl=2>"),
    fast_row<SOFTROD_FEATURES_SOFT_ARM, SOFTROD_ENV_SOFT_ARM, 2>("softrod_step_fast_kernel<SoftArm,epl=2>"),
    fast_row<kFeaturesMuscleRod, SOFTROD_ENV_NONE, 1>("softrod_step_fast_kernel<muscle rod,epl=1>"),
    fast_row<kRuntimeFeatures, kRuntimeEnv, 2>("softrod_step_fast_kernel<runtime mask,epl=2>"),
    // uniform rods, one slot per lane: with the per-env tables, then without
    fast_row<kArmSingleZup | kFeatEnvContact | kFeatEnvMaterial, SOFTROD_ENV_ARM_SINGLE, 1>("softrod_step_fast_kernel<ArmSingle,epl=1>"),
    fast_row<kArmSingleZup | kFeatEnvContact, SOFTROD_ENV_ARM_SINGLE, 1>("softrod_step_fast_kernel<ArmSingle,epl=1>"),
    fast_row<SOFTROD_FEATURES_SOFTPENDULUM | kFeatEnvMaterial, SOFTROD_ENV_SOFTPENDULUM, 1>("softrod_step_fast_kernel<SoftPendulum,epl=1>"),
    fast_row<SOFTROD_FEATURES_SOFTPENDULUM3D | kFeatEnvMaterial, SOFTROD_ENV_SOFTPENDULUM3D, 1>("softrod_step_fast_kernel<SoftPendulum3D,epl=1>"),
    fast_row<kArmSingleZup | kFeatEnvMaterial, SOFTROD_ENV_ARM_SINGLE, 1>("softrod_step_fast_kernel<ArmSingle,epl=1>"),
    fast_row<SOFTROD_FEATURES_SOFTPENDULUM, SOFTROD_ENV_SOFTPENDULUM, 1>("softrod_step_fast_kernel<SoftPendulum,epl=1>"),
    fast_row<SOFTROD_FEATURES_SOFTPENDULUM3D, SOFTROD_ENV_SOFTPENDULUM3D, 1>("softrod_step_fast_kernel<SoftPendulum3D,epl=1>"),
    fast_row<kArmSingleZup, SOFTROD_ENV_ARM_SINGLE, 1>("softrod_step_fast_kernel<ArmSingle,epl=1>"),
    fast_row<SOFTROD_FEATURES_SOFT_ARM, SOFTROD_ENV_SOFT_ARM, 1>("softrod_step_fast_kernel<SoftArm,epl=1>"),
    fast_row<kRuntimeFeatures, kRuntimeEnv, 1>("softrod_step_fast_kernel<runtime mask,epl=1>"),
    // SOFTROD_MATH_LIBM
    libm_row<true>(kAnyFeatures, kAny, kAny, kAny, 0u),
    libm_row<false>(SOFTROD_FEATURES_SOFTPENDULUM, SOFTROD_ENV_SOFTPENDULUM, kAny, 0, kOptEnvMaterial),
    libm_row<false>(SOFTROD_FEATURES_SOFTPENDULUM3D, SOFTROD_ENV_SOFTPENDULUM3D, kAny, 0, kOptEnvMaterial),
    libm_row<false>(SOFTROD_FEATURES_ARM_SINGLE, SOFTROD_ENV_ARM_SINGLE, 1, 0, kOptEnvMaterial | kOptEnvContact),
    libm_row<false>(kAnyFeatures, kAny, kAny, kAny, 0u),
};

unsigned active_options(const softrod_handle* h) {
    return (h->cfg.features & kOptMuscles) | (h->cfg.early_termination ? kOptEarlyTerm : 0u) |
           (h->env_mat.dev.get() ? kOptEnvMaterial : 0u) | (h->env_contact.dev.get() ? kOptEnvContact : 0u);
}

// The wording of a refusal, consulted only once no row of kStepRows serves the handle with the options `opts`: the
// first reason that applies.  nullptr: none of these.
const char* material_why_not(const softrod_handle* h) {
    const unsigned f = h->cfg.features;
    const int e = h->cfg.env_kind;
    if (is_octo(h) || is_mocto(h)) return "per-env material: not for OctoFlat or the muscle octopus envs";
    if (f & SOFTROD_FEAT_COOMM_MUSCLES) return "per-env material: not for the muscle envs";
    if (e == SOFTROD_ENV_SOFT_ARM) return "per-env material: not for SoftArmTracking (its muscle torque scale depends on E)";
    if (h->tapered) return "per-env material: not for a tapered rod (softrod_set_radius_profile)";
    if (h->epl != 1 || h->window_refresh > 0)
        return "per-env material: rods of up to 63 elements only (not the two-slot or windowed long rods)";
    return "per-env material: SoftPendulum, SoftPendulum3D and OctoArmSingle with their own feature sets only";
}
const char* contact_why_not(const softrod_handle* h) {
    const unsigned f = h->cfg.features;
    const int e = h->cfg.env_kind;
    if (is_mocto(h) || is_pull(h) || (f & SOFTROD_FEAT_COOMM_MUSCLES)) return "per-env contact: not for the muscle envs";
    if (!(f & SOFTROD_FEAT_PLANE_CONTACT_ANISO) || !((f == SOFTROD_FEATURES_ARM_SINGLE && e == SOFTROD_ENV_ARM_SINGLE) ||
                                                    (f == SOFTROD_FEATURES_OCTO_FLAT && e == SOFTROD_ENV_OCTO_FLAT)))
        return "per-env contact: OctoArmSingle, OctoFlat and OctoFlatLite with their own feature sets only";
    if (!(h->P.features & kFeatPlaneZup)) return "per-env contact: a contact plane with normal e_z only";
    if (h->cfg.early_termination) return "per-env contact: not with early_termination";
    if (is_octo(h))
        return "per-env contact: OctoFlat with at most two waves per env only (n_arm x segment <= 128 lanes; "
               "not the four- and eight-wave shapes)";
    if (h->tapered) return "per-env contact: not for a tapered rod (softrod_set_radius_profile)";
    return "per-env contact: rods of up to 63 elements only (not the two-slot or windowed long rods)";
}
// softrod_ground_reaction's scope: the first reason that applies, nullptr when the handle is served (the Python copy
// is ground_reaction_refusal in _capi.py).
const char* ground_reaction_why_not(const softrod_handle* h) {
    const unsigned f = h->cfg.features;
    if (is_mocto(h) || is_pull(h) || (f & SOFTROD_FEAT_COOMM_MUSCLES)) return "ground reaction: not for the muscle envs";
    if (!(f & SOFTROD_FEAT_PLANE_CONTACT_ANISO)) return "ground reaction: this env has no plane contact";
    if ((f & SOFTROD_FEAT_OCTO_HEAD) && !is_flat(h)) return "ground reaction: of the rigid-head envs OctoFlat and OctoFlatLite only";
    if (f & (SOFTROD_FEAT_POINT_FORCE_NODE0_X | SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES))
        return "ground reaction: not with a point force or spline muscle torques (loads that are not in the resident state)";
    if (h->cfg.n_elem > 63)          // (up to 63 elements a rod has one slot per lane and no windows: softrod_create)
        return "ground reaction: rods of up to 63 elements only (not the two-slot or windowed long rods)";
    return nullptr;
}
// softrod_rod_dynamics' scope, as ground_reaction_why_not (the Python copy is rod_dynamics_refusal in _capi.py).
const char* rod_dynamics_why_not(const softrod_handle* h) {
    const unsigned f = h->cfg.features;
    if (f & SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES)
        return "rod dynamics: not with spline muscle torques (loads that are not in the resident state)";
    if (h->cfg.n_elem > 63)          // (up to 63 elements a rod has one slot per lane and no windows: softrod_create)
        return "rod dynamics: rods of up to 63 elements only (not the two-slot or windowed long rods)";
    if ((f & SOFTROD_FEAT_COOMM_MUSCLES) && !h->muscles_set)
        return "rod dynamics: softrod_set_muscle_layers has not been called";
    return nullptr;
}
const char* why_no_row(const softrod_handle* h, unsigned opts) {
    if ((opts & kOptEarlyTerm) && h->cfg.math_mode == SOFTROD_MATH_FAST && !is_pull(h) &&
        !(h->tapered && h->cfg.features == SOFTROD_FEATURES_ARM_PUSH && h->cfg.env_kind == SOFTROD_ENV_ARM_PUSH))
        return "early_termination (SOFTROD_MATH_FAST) runs on the tapered SOFTROD_FEATURES_ARM_PUSH arm "
               "and on SOFTROD_ENV_ARM_PULL_WEIGHT only; other feature mixes: SOFTROD_MATH_LIBM";
    if (opts & kOptEnvMaterial) return material_why_not(h);
    if (opts & kOptEnvContact) return contact_why_not(h);
    return nullptr;
}

// The handle's step kernel: the first row of kStepRows that applies to it and honours every option it has, together
// with `with` (an option about to be added).  epilogue = 0: softrod_substeps' form, which a windowed handle takes on
// its two-slot kernel.  No such row: `why` says so, naming `with` first.
struct StepChoice { const StepRow* row; const char* why; };
StepChoice select_step(const softrod_handle* h, int epilogue = 1, unsigned with = 0u) {
    const unsigned opts = active_options(h) | with;
    const int e = h->cfg.env_kind, zup = (h->P.features & kFeatPlaneZup) != 0;
    const bool windowed = h->window_refresh > 0 && epilogue;
    for (const StepRow& r : kStepRows)
        if (r.math == h->cfg.math_mode && (r.feats == kAnyFeatures || r.feats == h->cfg.features) &&
            (r.env == kAny || (r.env == kMoctoEnvs ? mocto_kind(e) : r.env == e)) && r.epl == h->epl &&
            (r.taper == kAny || r.taper == (int)h->tapered) && (r.zup == kAny || r.zup == zup) &&
            r.nw_min <= h->nw && h->nw <= r.nw_max && r.windowed == windowed &&
            (!r.window || r.epb == (h->window_paired ? 4 : 1)) && !(r.needs & ~opts) && !(opts & ~r.honours))
            return {&r, nullptr};
    const char* why = why_no_row(h, with);
    if (!why) why = why_no_row(h, opts);
    return {nullptr, why ? why : "no step kernel is compiled for this handle's feature set, env kind and options"};
}

// the state bank, below
int bank_twin(softrod_handle* h, int slots, const void* base, size_t comps, size_t row_bytes, std::vector<StateBank::Twin>& out,
              const char* prefix, bool oom_is_enomem);
std::vector<EnvMaterial>& bank_host_rows(StateBank& b, const EnvMaterial*);
std::vector<EnvContact>& bank_host_rows(StateBank& b, const EnvContact*);

// softrod_set_env_material / softrod_set_env_contact: W doubles per env in, one Row per env on the device.  Refused
// unless a step kernel honours `option` on this handle; `bad` names what is wrong with an env's values (nullptr: nothing);
// the first call (a set-up, `entry_point`) allocates the table with every row at the config's `own` values and points
// h->S.*slot at it; only rows with mask != 0 change.
template <int W, class Row, class Bad, class Build>
int set_env_table(softrod_handle* h, EnvTable<Row>& T, const Row* StatePtrs::*slot, unsigned option, const char* entry_point,
                  const char* what, const double* values, const double (&own)[W], const uint8_t* mask, void* stream, Bad bad,
                  Build build) {
    const StepChoice serves = select_step(h, 1, option);
    if (!serves.row) return fail(h, SOFTROD_EINVAL, serves.why);
    const size_t N = (size_t)h->cfg.n_envs;
    for (size_t i = 0; i < N; ++i) {
        if (mask && !mask[i]) continue;
        if (const char* why = bad(values + W * i)) return fail(h, SOFTROD_EINVAL, what + std::to_string(i) + why);
    }
    SR_ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    if (!T.dev.get()) {
        arm_setup(h, entry_point);
        EnvTable<Row> fresh;
        SR_SETUP(h, fresh.dev.alloc(N * sizeof(Row)));
        SR_SETUP(h, fresh.host.alloc(N * sizeof(Row)));
        SR_SETUP(h, fresh.ev.create(hipEventDisableTiming));
        Row R0;
        build(own, R0);
        for (size_t i = 0; i < N; ++i) fresh.host.get()[i] = R0;
        // A table created after the bank: its twin, with every slot at the row the new table gives an untouched env, so
        // that a slot saved before the table existed loads as its env would be now.  (No twin, no table: copy_table
        // must not list an array the bank cannot follow.)
        StateBank& bank = h->bank;
        std::vector<StateBank::Twin> twin;
        std::vector<Row> rows;
        if (bank.slots) {
            if (const int rc = bank_twin(h, bank.slots, fresh.dev.get(), 1, sizeof(Row), twin, "state bank: ", false)) return rc;
            rows.assign((size_t)bank.slots, R0);
            bank.twins.reserve(bank.twins.size() + 1);
            SR_SETUP(h, hipMemcpy(twin[0].dev.get(), rows.data(), rows.size() * sizeof(Row), hipMemcpyHostToDevice),
                     "state bank: ", false);
        }
        StatePtrs S = h->S;
        S.*slot = fresh.dev.get();
        SR_SETUP(h, hipMemcpy(h->d_state, &S, sizeof(StatePtrs), hipMemcpyHostToDevice));
        // nothing below can fail
        h->S = S;
        T = std::move(fresh);
        if (bank.slots) {
            bank.twins.push_back(std::move(twin[0]));
            bank_host_rows(bank, T.dev.get()).swap(rows);
        }
    } else {
        SR_HIP(h, T.wait());    // the previous upload has left the staging buffer
    }
    for (size_t i = 0; i < N; ++i)
        if (!mask || mask[i]) build(values + W * i, T.host.get()[i]);
    SR_HIP(h, T.send(N, st));
    return SOFTROD_OK;
}

// One kernel of an env.step.  Untimed (no event): the plain launch.  Timed: the kernel's own dispatch carries the time
// stamps — `t0` takes the dispatch's begin, `t1` its end — instead of an event record in front of it and one behind,
// each a packet of its own with a system-scope release that the stream waits out.  So a timed step costs what an
// untimed one costs, and hipEventElapsedTime(t0, t1) is the kernels' own duration, first begin to last end.
// (Measured against the event records and against records of hipEventReleaseToDevice events, alternating fresh
// processes at 4096 envs: profiles/planar_step_ab.json.)
template <class K, class... A>
void launch_stamped(K kernel, const dim3& grid, const dim3& block, hipStream_t st, hipEvent_t t0, hipEvent_t t1, A... args) {
    if (t0 || t1) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, t0, t1, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
}

int launch_step(softrod_handle* h, const float* actions, float* obs, double* reward,
                uint8_t* term, uint8_t* trunc, double* aux, int n_sub, int epilogue, int pack,
                hipStream_t st) {
    if (h->q.depth > 0 && epilogue && !h->same_step) {
        if (const int rc = launch_autoreset(h, obs, reward, term, trunc, aux, pack, st)) return rc;
        // shaped starts for the envs the pass just restarted, in front of the step's first dispatch and its time stamp
        if (h->rs.count > 0)
            if (const int rc = launch_reset_shapes(h, kPickSkipped, nullptr, obs, term, trunc, aux, pack, st)) return rc;
    }
    if ((h->cfg.features & SOFTROD_FEAT_COOMM_MUSCLES) && h->cfg.math_mode == SOFTROD_MATH_FAST) {
        // what the muscle handles need set before they step
        const bool push = h->cfg.env_kind == SOFTROD_ENV_ARM_PUSH || is_pull(h) || is_mocto(h);
        if (is_mocto(h) && (!h->tapered || !h->muscles_set || (h->cfg.env_kind == SOFTROD_ENV_ARM_TWO && !h->basis_set)))
            return fail(h, SOFTROD_EINVAL, "the muscle octopus needs softrod_set_radius_profile and softrod_set_muscle_layers "
                                           "(and SOFTROD_ENV_ARM_TWO softrod_set_action_basis) before it steps");
        if (push && !h->tapered)
            return fail(h, SOFTROD_EINVAL, "SOFTROD_ENV_ARM_PUSH (SOFTROD_MATH_FAST): call softrod_set_radius_profile first "
                                           "(the reference's arm is tapered, arm_push_env.py:160-179)");
        if (!push && h->tapered)
            return fail(h, SOFTROD_EINVAL, "a tapered muscle rod outside SOFTROD_ENV_ARM_PUSH runs under SOFTROD_MATH_LIBM only");
    }
    const StepChoice c = select_step(h, epilogue);
    if (!c.row) return fail(h, SOFTROD_EINVAL, c.why);
    // a windowed env.step: its substeps, then reward / observation by the row of the same handle's plain substeps
    const StepChoice after = c.row->windowed ? select_step(h, 0) : StepChoice{nullptr, nullptr};
    if (c.row->windowed && !after.row) return fail(h, SOFTROD_EINVAL, after.why);
    // Planar certificates: a kernel that knows them may issue some (it reads the switch itself, from device memory);
    // any other kernel writes rows without knowing of them, so what earlier launches issued is withdrawn in front of it.
    if (c.row->cert) h->cert_live = true;
    else if (const int rc = clear_planar_certs(h, st, false)) return rc;
    auto launch = [&](const StepRow& r, int n, int epi, hipEvent_t t0, hipEvent_t t1) {
        const dim3 grid((unsigned)((h->cfg.n_envs + r.epb - 1) / r.epb)), block(kLanes * (r.waves ? r.waves : h->nw));
        if (r.window) launch_stamped(r.window, grid, block, st, t0, t1, h->P, h->S, actions, n, h->window_refresh);
        else if (r.octo) launch_stamped(r.octo, grid, block, st, t0, t1, h->P, h->S, actions, obs, reward, term, trunc, n, epi, pack);
        else launch_stamped(r.step, grid, block, st, t0, t1, h->P, h->S, actions, obs, reward, term, trunc, aux, n, epi, pack);
    };
    // A timed step: its pair of events rides on the step's own dispatches (launch_stamped) — the start on the first
    // kernel of the step, the stop on the last, one pair per step whatever the number of kernels.
    const bool timing = h->timed < (int)h->ev_start.size();
    const hipEvent_t t0 = timing ? h->ev_start[h->timed].get() : nullptr, t1 = timing ? h->ev_stop[h->timed].get() : nullptr;
    // the muscle octopus: set_action | the body's substeps | get_state + reward; the timing events bracket all three
    const bool mocto = c.row->env == kMoctoEnvs;
    const bool action_first = mocto && epilogue && actions, epilogue_last = mocto && epilogue;
    const dim3 grid((unsigned)h->cfg.n_envs), block(kLanes * h->nw);
    if (action_first)
        launch_stamped(softrod_mocto_action_kernel, grid, block, st, t0, nullptr, h->P, h->S, actions, n_sub);
    launch(*c.row, n_sub, epilogue, action_first ? nullptr : t0, (after.row || epilogue_last) ? nullptr : t1);
    if (after.row) launch(*after.row, 0, 1, nullptr, epilogue_last ? nullptr : t1);
    if (epilogue_last)
        launch_stamped(softrod_mocto_epilogue_kernel, grid, block, st, nullptr, t1, h->P, h->S, obs, reward, term, trunc, 1, pack);
    SR_HIP(h, hipGetLastError());
    if (timing) ++h->timed;
    // behind the timing record, so that kernel_times_ms keeps meaning the step (as for the NEXT_STEP pass in front)
    if (h->q.depth > 0 && epilogue && h->same_step) {
        if (const int rc = launch_autoreset_same_step(h, obs, aux, pack, st)) return rc;
        if (h->rs.count > 0)      // shaped starts for the envs that pass just restarted
            if (const int rc = launch_reset_shapes(h, kPickFinished, nullptr, obs, term, trunc, aux, pack, st)) return rc;
    }
    return SOFTROD_OK;
}

int upload_and_reset(softrod_handle* h, hipStream_t st, bool use_mask) {
    const size_t N = (size_t)h->cfg.n_envs;
    if (const int rc = clear_planar_certs(h, st)) return rc;
    double* const d_init = h->reset.init.dev.get();
    uint8_t* const d_mask = h->reset.d_mask.get();
    SR_HIP(h, hipMemcpyAsync(d_init, h->reset.init.host.get(), N * h->init_stride * sizeof(double), hipMemcpyHostToDevice, st));
    if (use_mask)
        SR_HIP(h, hipMemcpyAsync(d_mask, h->reset.h_mask.get(), N, hipMemcpyHostToDevice, st));
    ResetArgs A{d_init, use_mask ? d_mask : nullptr};
    if (is_octo(h)) {
        OctoResetArgs OA{d_init, d_init + N * (size_t)h->cfg.n_arm * 18, use_mask ? d_mask : nullptr};   // (targets: 2 numbers per env, 4 for the muscle octopus)
        hipLaunchKernelGGL(softrod_octo_reset_kernel, dim3((unsigned)N), dim3(kLanes * h->nw), 0, st, h->P, h->S, OA);
    } else
        hipLaunchKernelGGL(by_epl(h, softrod_reset_kernel<1>, softrod_reset_kernel<2>), dim3((unsigned)N), dim3(kLanes), 0, st,
                           h->P, h->S, A);
    SR_HIP(h, hipGetLastError());
    SR_HIP(h, hipEventRecord(h->reset.init.ev.get(), st));
    h->was_reset = true;
    return SOFTROD_OK;
}

// host part of straight_rod for one rod: start, step, end, Q rows
void straight_init(const softrod_config& c, const double start[3], const double direction[3],
                   const double normal_in[3], double out[18]) {
    const int n = c.n_elem;
    double end[3], normal[3], t[3], d[3];
    for (int i = 0; i < 3; ++i) end[i] = start[i] + direction[i] * c.base_length;
    const double nn = std::sqrt(normal_in[0] * normal_in[0] + normal_in[1] * normal_in[1] +
                                normal_in[2] * normal_in[2]);
    for (int i = 0; i < 3; ++i) normal[i] = normal_in[i] / nn;
    for (int i = 0; i < 3; ++i) {
        out[i] = start[i];
        out[3 + i] = (end[i] - start[i]) / (double)n;
        out[6 + i] = end[i];
        d[i] = (start[i] + 1.0 * out[3 + i]) - start[i];  // x[1]-x[0] as linspace produces it
    }
    const double l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int i = 0; i < 3; ++i) t[i] = d[i] / l;
    for (int i = 0; i < 3; ++i) out[9 + i] = normal[i];
    out[12] = t[1] * normal[2] - t[2] * normal[1];
    out[13] = t[2] * normal[0] - t[0] * normal[2];
    out[14] = t[0] * normal[1] - t[1] * normal[0];
    for (int i = 0; i < 3; ++i) out[15 + i] = t[i];
}

// ---- One start record per kind of draw, written once for the masked reset (frames in h_init, the targets in a block
// of their own behind N * n_arm * 18) and for the staged queue (a record carries its target inline): the callers differ
// only in where `frames` and `tgt` point and in the index of the draw.
// SoftPendulum's theta0 -> its frame (build.py:46-52)
void theta_record(const softrod_handle* h, double th, double* frames) {
    const double start[3] = {0.0, 0.0, 0.0};
    const double direction[3] = {1.0 * std::cos(th), 1.0 * std::sin(th), 0.0};
    const double normal[3] = {1.0 * std::sin(th), -1.0 * std::cos(th), 0.0};
    straight_init(h->cfg, start, direction, normal, frames);
}
// start / direction / normal -> frame.  ArmPullWeightEnv: the one arm's record where the rigid-body reset kernel expects
// the arms', a zero target behind it (the slot is unused); every other env has no target and `tgt` is not touched
void straight_record(const softrod_handle* h, const double* start, const double* direction, const double* normal,
                     double* frames, double* tgt) {
    straight_init(h->cfg, start, direction, normal, frames);
    if (is_pull(h)) { tgt[0] = 0.0; tgt[1] = 0.0; }
}
// one env's n_arm starts and directions -> its frames (normal e_z: octopus/build.py:82, build_muscle_octopus.py:92) and its
// target: 2 numbers, or the muscle octopus' 4 (x, y, z and the episode's final_time; 0: the config's)
size_t octo_target_dim(const softrod_handle* h) { return is_mocto(h) ? 4 : 2; }
void octo_record(const softrod_handle* h, const double* arm_start, const double* arm_direction, const double* target,
                 double* frames, double* tgt) {
    const double normal[3] = {0.0, 0.0, 1.0};
    for (int a = 0; a < h->cfg.n_arm; ++a)
        straight_init(h->cfg, arm_start + 3 * a, arm_direction + 3 * a, normal, frames + (size_t)a * 18);
    for (size_t i = 0; i < octo_target_dim(h); ++i) tgt[i] = target[i];
}

void config_common(softrod_config* cfg, int n_envs) {
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(softrod_config);
    cfg->n_envs = n_envs;
    cfg->n_elem = 50;                                   // soft_pendulum.py:64
    cfg->dt = 1.0e-4;                                   // :62
    cfg->n_substeps = (int)(1.0 / (25 * cfg->dt));      // :78 (recording_fps = 25, :63)
    cfg->math_mode = SOFTROD_MATH_FAST;
    cfg->final_time = 5.0;                              // :61
    cfg->alpha_c = 27.0 / 28.0;
    cfg->eps_length = 1e-14;
    cfg->eps_rot_axis = 1e-14;
    cfg->acos_shift = 1e-10;
    cfg->eps_sin = 1e-14;
    cfg->time_two_half_adds = 1;
    cfg->damp_before_constrain = 0;   // constrain() is registered before dampen() in both builds
}

// softrod_create's checks of the config, in order: the first reason to refuse it, nullptr when there is none.  No HIP
// call and no handle: what is refused here is refused on a host without a device too.
const char* config_why_not(const softrod_config& c) {
    if (c.n_envs < 1 || c.n_elem < 2 || c.n_elem > 2 * kLanes - 2)
        return "need n_envs >= 1 and 2 <= n_elem <= 126";
    if (c.n_elem > kLanes - 1 && c.math_mode != SOFTROD_MATH_FAST)
        return "rods longer than 63 elements (two per lane) exist for SOFTROD_MATH_FAST only";
    if (c.n_substeps < 0 || !(c.dt > 0.0))
        return "need n_substeps >= 0 and dt > 0";
    if (c.math_mode != SOFTROD_MATH_LIBM && c.math_mode != SOFTROD_MATH_FAST)
        return "unknown math_mode";
    if (c.env_kind < SOFTROD_ENV_NONE || c.env_kind > SOFTROD_ENV_REACH)
        return "unknown env_kind";
    if (c.features & SOFTROD_FEAT_COOMM_MUSCLES) {
        // two slots per lane (64..126 elements): the tapered ArmPush arm's own instantiations only
        const bool two_slot_push = c.features == SOFTROD_FEATURES_ARM_PUSH && c.env_kind == SOFTROD_ENV_ARM_PUSH &&
                                   c.math_mode == SOFTROD_MATH_FAST;
        if (c.n_muscles < 1 || c.n_muscles > SOFTROD_MAX_MUSCLES || c.muscle_fl_degree < 0 ||
            c.muscle_fl_degree >= SOFTROD_MAX_FL_COEF || (c.n_elem > kLanes - 1 && !two_slot_push) ||
            ((c.features & SOFTROD_FEAT_OCTO_HEAD) && c.env_kind != SOFTROD_ENV_ARM_PULL_WEIGHT && !mocto_kind(c.env_kind)))
            return "COOMM muscles: 1 <= n_muscles <= 4, 0 <= muscle_fl_degree <= 7, one rod of up to 63 elements per env";
        for (int m = 0; m < c.n_muscles; ++m)
            if (c.muscle_kind[m] != SOFTROD_MUSCLE_LONGITUDINAL && c.muscle_kind[m] != SOFTROD_MUSCLE_TRANSVERSE)
                return "muscle_kind: SOFTROD_MUSCLE_LONGITUDINAL or SOFTROD_MUSCLE_TRANSVERSE";
        if ((c.muscle_equiv_load_form | 1) != 1 || (c.muscle_position_current_radius | 1) != 1 ||
            (c.muscle_tm_length_law | 1) != 1)
            return "muscle_equiv_load_form, muscle_position_current_radius, muscle_tm_length_law: 0 or 1";
    }
    if ((c.features & SOFTROD_FEAT_COOMM_MUSCLES) && c.math_mode == SOFTROD_MATH_FAST &&
        !((c.features == SOFTROD_FEATURES_ARM_PUSH && c.env_kind == SOFTROD_ENV_ARM_PUSH) ||
          (c.features == SOFTROD_FEATURES_ARM_PULL_WEIGHT && (c.env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT || mocto_kind(c.env_kind))) ||
          (c.features == kFeaturesMuscleRod && c.env_kind == SOFTROD_ENV_NONE)))
        return "SOFTROD_MATH_FAST compiles the COOMM muscles for SOFTROD_FEATURES_ARM_PUSH with SOFTROD_ENV_ARM_PUSH "
                    "(tapered) and for FIXED_BC | ANALYTICAL_DAMPER | COOMM_MUSCLES with SOFTROD_ENV_NONE (uniform rod); "
                    "use SOFTROD_MATH_LIBM for any other mix";
    if (c.env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT &&
        (c.features != SOFTROD_FEATURES_ARM_PULL_WEIGHT || c.math_mode != SOFTROD_MATH_FAST || c.n_arm != 1 ||
         !(c.head_length > 0.0) || !(c.head_radius > 0.0) || !(c.head_density > 0.0)))
        return "SOFTROD_ENV_ARM_PULL_WEIGHT: SOFTROD_FEATURES_ARM_PULL_WEIGHT, SOFTROD_MATH_FAST, n_arm = 1, "
                                             "head_length / head_radius / head_density > 0";
    if (c.env_kind == SOFTROD_ENV_ARM_PUSH || c.env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT) {
        const unsigned need = SOFTROD_FEAT_COOMM_MUSCLES | SOFTROD_FEAT_SUCKER_CONSTRAINT;
        if ((c.features & need) != need || c.n_muscles < 3 || (c.arm_push_mode != 0 && c.arm_push_mode != 1))
            return "SOFTROD_ENV_ARM_PUSH needs the sucker constraint, three muscle layers and arm_push_mode 0 or 1";
    }
    if (c.damper_protocol != 0 && c.damper_protocol != 1)
        return "damper_protocol: 0 (per unit mass) or 1 (uniform)";
    // The fast kernels expand theta / sin(theta + eps_sin) as (theta / sin theta)(1 - eps_sin cot theta)
    // (eps_sin_factor, softrod_fast.hpp; the bke * rsq(D^2 + two_shift) term of softrod_planar.hpp), which
    // holds while eps_sin << theta_min = sqrt(2 acos_shift), the smallest angle acos(.. - acos_shift)
    // returns.  The reference's values (1e-14 against 1.4e-5) sit nine orders inside; a config outside
    // — acos_shift = 0 with a straight joint sends cot theta to 1e150 and flips the sign of the bending
    // stiffness — is refused here rather than integrated wrongly (the libm kernel evaluates the
    // quotient as written and takes any values).
    if (c.math_mode == SOFTROD_MATH_FAST &&
        !(c.acos_shift > 0.0 && c.eps_sin >= 0.0 && c.eps_sin <= 1.0e-3 * std::sqrt(2.0 * c.acos_shift)))
        return "SOFTROD_MATH_FAST needs acos_shift > 0 and 0 <= eps_sin <= 1e-3 sqrt(2 acos_shift); "
                    "use SOFTROD_MATH_LIBM for other values";
    {
        const bool muscles = (c.features & SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES) != 0;
        if (muscles != (c.env_kind == SOFTROD_ENV_SOFT_ARM))
            return "SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES and SOFTROD_ENV_SOFT_ARM go together";
        if (muscles && (c.math_mode != SOFTROD_MATH_FAST || c.n_ctrl < 1 || c.n_ctrl > 4 ||
                        c.n_spline_pieces < 1 || c.n_spline_pieces > SOFTROD_MAX_SPLINE_PIECES ||
                        c.n_elem - 1 < c.n_ctrl || !(c.max_activation_rate > 0.0)))
            return "spline muscles need SOFTROD_MATH_FAST, 1 <= n_ctrl <= 4, 1 <= n_spline_pieces <= 8, "
                        "max_activation_rate > 0";
    }
    const bool octo = (c.features & SOFTROD_FEAT_OCTO_HEAD) != 0;
    const bool pull = c.env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT;
    const bool mocto = mocto_kind(c.env_kind);
    if (octo != (c.env_kind == SOFTROD_ENV_OCTO_FLAT || pull || mocto))
        return "SOFTROD_FEAT_OCTO_HEAD goes with SOFTROD_ENV_OCTO_FLAT, SOFTROD_ENV_ARM_PULL_WEIGHT "
                                             "or the muscle octopus envs";
    if (mocto) {
        // n_arm * 32 slots = 1 or 4 whole waves, so that every slot of the block belongs to an arm
        if (c.features != SOFTROD_FEATURES_ARM_PULL_WEIGHT || c.math_mode != SOFTROD_MATH_FAST)
            return "the muscle octopus exists for SOFTROD_FEATURES_ARM_PULL_WEIGHT and SOFTROD_MATH_FAST only";
        if (c.n_elem < 16 || c.n_elem > 31 || (c.n_arm != 2 && c.n_arm != 8) || c.n_muscles != 3)
            return "the muscle octopus needs 16 <= n_elem <= 31, n_arm = 2 or 8, three muscle layers";
        const int nk = c.env_kind == SOFTROD_ENV_CRAWL ? 3 : (c.env_kind == SOFTROD_ENV_ARM_TWO ? 9 : 3 * c.n_elem);
        if (c.n_knots != nk || (c.env_kind == SOFTROD_ENV_ARM_TWO && c.n_suckers != 3) ||
            (c.env_kind == SOFTROD_ENV_CRAWL && c.n_suckers != 1) || (c.env_kind == SOFTROD_ENV_REACH && c.n_suckers != 0))
            return "the muscle octopus: n_knots (actions per arm) 3 / 9 / 3 n_elem and n_suckers 1 / 3 / 0 "
                                                 "for CRAWL / ARM_TWO / REACH";
        if (!(c.head_radius > 0.0) || !(c.head_density > 0.0) || !(c.head_length > 0.0))
            return "the muscle octopus needs head_radius, head_density, head_length > 0";
    }
    if (octo && !pull && !mocto) {
        if (c.features != SOFTROD_FEATURES_OCTO_FLAT || c.math_mode != SOFTROD_MATH_FAST)
            return "OctoFlat exists for SOFTROD_FEATURES_OCTO_FLAT and SOFTROD_MATH_FAST only";
        if (c.n_elem > kLanes - 1 || c.n_arm < 1 || c.n_knots < 1 || c.n_knots > c.n_elem ||
            (c.n_elem - 1) * c.n_knots > 2 * kLanes * 7)
            return "OctoFlat needs n_elem <= 63, n_arm >= 1, 1 <= n_knots <= n_elem";
        const int seg = c.n_elem <= 15 ? 16 : (c.n_elem <= 31 ? 32 : 64);
        if (c.n_arm * seg > 8 * kLanes)
            return "OctoFlat: n_arm * slots-per-arm must not exceed 512";
        if (!(c.head_radius > 0.0) || !(c.head_density > 0.0))
            return "OctoFlat needs head_radius > 0 and head_density > 0";
    }
    if (c.features & SOFTROD_FEAT_SUCKER_CONSTRAINT) {
        if ((octo && !pull && !mocto) || c.n_suckers < (mocto ? 0 : 1) || c.n_suckers > SOFTROD_MAX_SUCKERS)
            return "ControllableFixConstraint: 1 <= n_suckers <= 4, not with OctoFlat";
        for (int j = 0; j < c.n_suckers; ++j)
            if (c.sucker_index[j] < 0 || c.sucker_index[j] >= c.n_elem)
                return "ControllableFixConstraint: 0 <= sucker_index < n_elem";
    }
    if ((c.features & SOFTROD_FEAT_LAPLACE_FILTER) && (c.filter_order < 1 || c.n_elem < 3))
        return "LaplaceDissipationFilter needs filter_order >= 1";
    if (c.early_termination != 0 && c.early_termination != 1)
        return "early_termination is 0 or 1";
    if (c.early_termination && c.env_kind != SOFTROD_ENV_ARM_PUSH && c.env_kind != SOFTROD_ENV_ARM_PULL_WEIGHT)
        return "early_termination (ArmPushEnv's Hamiltonian cut-off) exists for SOFTROD_ENV_ARM_PUSH / ARM_PULL_WEIGHT only";
    {
        const unsigned bcs = c.features & (SOFTROD_FEAT_PENDULUM_BC | SOFTROD_FEAT_FIXED_BC |
                                              SOFTROD_FEAT_MOVING_BASE_BC);
        if (bcs & (bcs - 1)) return "at most one boundary condition";
    }
    return nullptr;
}

// The clock after k env.steps from a reset, k = 0..1023, as `self.time = self.do_step(self.simulator, self.time,
// self.time_step)` accumulates it (soft_pendulum.py:183-184): same additions, same order, IEEE doubles -> bit-identical
std::vector<double> clock_table(const softrod_config& c) {
    std::vector<double> tab(1024);
    double t = 0.0;
    const double half = 0.5 * c.dt;
    for (double& at : tab) {
        at = t;
        for (int s = 0; s < c.n_substeps; ++s) {
            if (c.time_two_half_adds) { t = t + half; t = t + half; }
            else t = t + c.dt;
        }
    }
    return tab;
}

// What follows from the config alone: RodParams, slots per lane, waves per env, the reset record, the two-window form.
void shape_handle(softrod_handle* h) {
    const softrod_config* cfg = &h->cfg;
    h->epl = cfg->n_elem > kLanes - 1 ? 2 : 1;
    fill_params(h->cfg, h->P);
    if (is_octo(h)) {
        h->nw = (cfg->n_arm * h->P.seg + kLanes - 1) / kLanes;
        h->init_stride = (size_t)cfg->n_arm * 18 + (is_mocto(h) ? 4 : 2);
    }
    // A/B switches for profiling and tests.  A product library must not change its kernel tier because of a
    // stray environment variable: they are read only when SOFTROD_DEBUG_SWITCHES=1 is set as well
    // (tests/test_gpu_debug_switches.py), and softrod_kernel_tier() reports what was selected.
    const char* dbg = std::getenv("SOFTROD_DEBUG_SWITCHES");
    const bool debug_switches = dbg && dbg[0] == '1';
    auto debug_env = [&](const char* name) -> const char* { return debug_switches ? std::getenv(name) : nullptr; };
    if (const char* one = debug_env("SOFTROD_WINDOW_PAIRED"))              // softrod_window.hpp
        h->window_paired = one[0] != '0';
    {   // two-window form: ArmSingle with the e_z contact, 64..102 elements
        const int halo = kLanes - (cfg->n_elem + 2) / 2;     // the narrower of the two halos
        const char* off = debug_env("SOFTROD_NO_WINDOW");
        if (h->epl == 2 && cfg->features == SOFTROD_FEATURES_ARM_SINGLE && cfg->env_kind == SOFTROD_ENV_ARM_SINGLE &&
            cfg->math_mode == SOFTROD_MATH_FAST && (h->P.features & kFeatPlaneZup) && !(off && off[0] == '1') &&
            halo >= 3 * kWindowRho)
            h->window_refresh = halo / kWindowRho;    // the front (< 3.25 nodes per substep) stays in the halo
        if (const char* r = debug_env("SOFTROD_WINDOW_REFRESH")) if (h->window_refresh > 0) h->window_refresh = std::atoi(r);
    }
}


// Why softrod_copy_envs refuses these arguments (empty: it does not).  Host only; leaves h->is_dst all zero.
std::string copy_envs_why_not(softrod_handle* h, const int32_t* src, const int32_t* dst, int count) {
    const int N = h->cfg.n_envs;
    if (h->q.depth > 0)
        return "copy envs: not on a handle with device-side auto-reset (the pending-reset flags and the staged queue "
               "belong to each env's RNG future)";
    if (count < 0 || count > N) return "copy envs: count " + std::to_string(count) + " is outside 0 .. n_envs = " + std::to_string(N);
    if (count > 0 && (!src || !dst)) return "copy envs: null src or dst";
    for (int i = 0; i < count; ++i)
        for (const int e : {src[i], dst[i]})
            if (e < 0 || e >= N)
                return "copy envs: env index " + std::to_string(e) + " (pair " + std::to_string(i) + ") is outside 0 .. " + std::to_string(N - 1);
    std::string why;
    for (int i = 0; i < count && why.empty(); ++i) {
        if (h->is_dst[dst[i]]) why = "copy envs: env " + std::to_string(dst[i]) + " appears twice in dst";
        h->is_dst[dst[i]] = 1;
    }
    // the kernel reads and writes in place: a row that one pair writes and another reads would depend on scheduling
    for (int i = 0; i < count && why.empty(); ++i)
        if (src[i] != dst[i] && h->is_dst[src[i]])
            why = "copy envs: env " + std::to_string(src[i]) + " is the dst of one pair and the src of another";
    for (int i = 0; i < count; ++i) h->is_dst[dst[i]] = 0;
    return why;
}

// Every per-env array of the handle, as softrod_copy_envs_kernel takes them: the arrays of softrod_state_view (the
// audit of softrod_create's allocation list: everything else it allocates is shared by all envs — spline table,
// action basis, material and muscle tables, clock table, the parameter copies, the scatter ticket — or reset staging)
// and the per-env tables that exist.
CopyTable copy_table(const softrod_handle* h) {
    CopyTable T{};
    T.n_envs = h->cfg.n_envs;
    auto add = [&T](const void* p, size_t comps, size_t row_bytes) {
        if (p) T.a[T.n++] = CopyArray{(unsigned char*)const_cast<void*>(p), (unsigned)comps, (unsigned)row_bytes};
    };
    const StatePtrs& S = h->S;
    const softrod_config& c = h->cfg;
    const size_t W = (size_t)rod_layout(h).lane_stride * sizeof(double);
    const size_t adim = (size_t)softrod_config_action_dim(&c);
    const size_t per = is_mocto(h) ? (size_t)c.n_arm : 1;      // SuckerControllers per env
    add(S.pos, 3, W); add(S.vel, 3, W); add(S.dir, 9, W); add(S.omg, 3, W); add(S.tan, 3, W);
    add(S.kap, 3, W); add(S.rkap, 3, W); add(S.envmem, 1, W); add(S.mact, SOFTROD_MAX_MUSCLES, W);
    add(S.time, 1, sizeof(double)); add(S.ctrl, 4, sizeof(double)); add(S.head, 20, sizeof(double));
    add(S.bc, 12, sizeof(double)); add(S.aux, 8, sizeof(double));
    add(S.prev_action, 1, (adim > 7 ? adim : 7) * sizeof(float));
    add(S.prev_kappa, 1, (size_t)c.n_arm * (size_t)(c.n_elem - 1) * sizeof(float));
    add(S.sucker, SOFTROD_MAX_SUCKERS, per * sizeof(double));
    add(S.sucker_idx, SOFTROD_MAX_SUCKERS, per * sizeof(int));
    add(h->env_mat.dev.get(), 1, sizeof(EnvMaterial));
    add(h->env_contact.dev.get(), 1, sizeof(EnvContact));
    // shaped starts: where the copy's episode started, and its resets' count (fork(copy_rng=False) puts dst's back)
    add(h->rs.index.get(), 1, sizeof(int)); add(h->rs.episode.get(), 1, sizeof(int));
    // planar certificates: a byte vouches for the rows above, so it travels with them (a bank slot keeps its own)
    add(S.planar_cert, 1, sizeof(uint8_t));
    static_assert(kCopyMaxArrays >= 23, "copy_table adds up to 23 arrays");
    return T;
}

// The pinned copy of a per-env table follows the device rows: the next softrod_set_env_* uploads all of it.
template <class Row>
hipError_t copy_table_rows(EnvTable<Row>& T, const int2* pairs, int n) {
    if (!T.dev.get()) return hipSuccess;
    const hipError_t e = T.wait();      // the previous upload has left the staging buffer
    if (e != hipSuccess) return e;
    Row* const host = T.host.get();
    for (int i = 0; i < n; ++i) host[pairs[i].y] = host[pairs[i].x];
    return hipSuccess;
}

// ---- the state bank (softrod_state_bank.hpp) ----
// The bank's side of a batch table: the same arrays in the same order, each at its twin, `slots` rows per component.
// false: an array of the batch has no twin (every call that creates a per-env array after the bank gives it a twin: bank_twin).
bool bank_table(const StateBank& bank, const CopyTable& batch, CopyTable& out) {
    out = batch;
    out.n_envs = bank.slots;
    for (int k = 0; k < batch.n; ++k)
        if (!(out.a[k].base = bank.twin_of(batch.a[k].base))) return false;
    return true;
}

// One set-up call: the twin, zeroed, that a bank of `slots` slots holds for the per-env array at `base` (its `comps`
// and `row_bytes` as copy_table lists them), appended to `out` — the caller's local list, which it moves into the bank
// when it commits.  A failure is reported in the caller's words (SR_SETUP).
int bank_twin(softrod_handle* h, int slots, const void* base, size_t comps, size_t row_bytes, std::vector<StateBank::Twin>& out,
              const char* prefix, bool oom_is_enomem) {
    DeviceBuf<unsigned char> dev;
    SR_SETUP(h, dev.alloc(comps * (size_t)slots * row_bytes, true), prefix, oom_is_enomem);
    out.push_back({base, std::move(dev)});
    return SOFTROD_OK;
}

std::vector<EnvMaterial>& bank_host_rows(StateBank& b, const EnvMaterial*) { return b.mat; }
std::vector<EnvContact>& bank_host_rows(StateBank& b, const EnvContact*) { return b.contact; }

// The pinned copy of a per-env table and the bank's host rows follow the device rows, as copy_table_rows does for
// softrod_copy_envs.  pairs: (env, slot) for a save, (slot, env) for a load.
template <class Row>
hipError_t bank_table_rows(StateBank& bank, EnvTable<Row>& T, const int2* pairs, int n, bool load) {
    if (!T.dev.get()) return hipSuccess;
    std::vector<Row>& rows = bank_host_rows(bank, T.dev.get());
    Row* const host = T.host.get();
    if (!load) {
        for (int i = 0; i < n; ++i) rows[pairs[i].y] = host[pairs[i].x];
        return hipSuccess;
    }
    const hipError_t e = T.wait();      // the previous upload has left the staging buffer
    if (e != hipSuccess) return e;
    for (int i = 0; i < n; ++i) host[pairs[i].y] = rows[pairs[i].x];
    return hipSuccess;
}

// Why softrod_bank_save (load = false) or softrod_bank_load (load = true) refuses these arguments (empty: it does not).
// Host only; leaves bank.seen all zero.  The side written — the slots of a save, the envs of a load — may name an index
// once; the side read may repeat.
std::string bank_why_not(softrod_handle* h, const int32_t* envs, const int32_t* slots, int count, bool load) {
    const std::string what = load ? "bank load: " : "bank save: ";
    StateBank& bank = h->bank;
    const int N = h->cfg.n_envs, K = bank.slots;
    if (!K) return what + "the handle has no state bank (softrod_bank_create)";
    if (h->q.depth > 0)
        return what + "not on a handle with device-side auto-reset (the pending-reset flags and the staged queue "
                      "belong to each env's RNG future)";
    const int limit = load ? N : K;
    if (count < 0 || count > limit)
        return what + "count " + std::to_string(count) + " is outside 0 .. " + (load ? "n_envs = " : "slots = ") + std::to_string(limit);
    if (count > 0 && (!envs || !slots)) return what + "null envs or slots";
    for (int i = 0; i < count; ++i) {
        if (envs[i] < 0 || envs[i] >= N)
            return what + "env index " + std::to_string(envs[i]) + " (pair " + std::to_string(i) + ") is outside 0 .. " + std::to_string(N - 1);
        if (slots[i] < 0 || slots[i] >= K)
            return what + "slot index " + std::to_string(slots[i]) + " (pair " + std::to_string(i) + ") is outside 0 .. " + std::to_string(K - 1);
    }
    if (load)
        for (int i = 0; i < count; ++i)
            if (!bank.filled[slots[i]]) return what + "slot " + std::to_string(slots[i]) + " holds no state";
    const int32_t* written = load ? envs : slots;
    std::string why;
    for (int i = 0; i < count && why.empty(); ++i) {
        if (bank.seen[written[i]])
            why = what + (load ? "env " : "slot ") + std::to_string(written[i]) + " appears twice";
        bank.seen[written[i]] = 1;
    }
    for (int i = 0; i < count; ++i) bank.seen[written[i]] = 0;
    return why;
}

// softrod_bank_save / softrod_bank_load behind their validation: the pairs' upload and the one kernel.
int bank_copy(softrod_handle* h, const int32_t* envs, const int32_t* slots, int count, bool load, void* stream) {
    const std::string why = bank_why_not(h, envs, slots, count, load);
    if (!why.empty()) return fail(h, SOFTROD_EINVAL, why);
    if (count == 0) return SOFTROD_OK;
    StateBank& bank = h->bank;
    CopyTable batch = copy_table(h), twin;
    if (!bank_table(bank, batch, twin))
        return fail(h, SOFTROD_EINVAL, std::string(load ? "bank load" : "bank save") + ": a per-env array of the handle has no twin in the bank");
    SR_ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    SR_HIP(h, bank.pairs.wait());       // the previous call's pairs have left the staging buffer
    int2* const h_pairs = bank.pairs.host.get();
    for (int i = 0; i < count; ++i) h_pairs[i] = load ? make_int2(slots[i], envs[i]) : make_int2(envs[i], slots[i]);
    SR_HIP(h, bank_table_rows(bank, h->env_mat, h_pairs, count, load));
    SR_HIP(h, bank_table_rows(bank, h->env_contact, h_pairs, count, load));
    SR_HIP(h, bank.pairs.send((size_t)count, st));
    hipLaunchKernelGGL(softrod_bank_copy_kernel, dim3((unsigned)count), dim3(kCopyThreads), 0, st,
                       load ? twin : batch, load ? batch : twin, bank.pairs.dev.get());
    SR_HIP(h, hipGetLastError());
    if (load && h->S.planar_cert) h->cert_live = true;      // (a slot's certificate travels with its rows)
    if (!load)
        for (int i = 0; i < count; ++i) bank.filled[slots[i]] = 1;
    return SOFTROD_OK;
}
}  // namespace

extern "C" {

int softrod_abi_version(void) { return SOFTROD_ABI_VERSION; }

#ifndef SOFTROD_SOURCE_HASH
#define SOFTROD_SOURCE_HASH "unhashed"
#endif
const char* softrod_source_hash(void) { return SOFTROD_SOURCE_HASH; }

int softrod_action_dim(int env_kind) {
    return env_kind == SOFTROD_ENV_SOFTPENDULUM3D ? 2 : env_kind == SOFTROD_ENV_ARM_SINGLE ? 7
         : env_kind == SOFTROD_ENV_OCTO_FLAT ? 24 : env_kind == SOFTROD_ENV_SOFT_ARM ? 8
         : (env_kind == SOFTROD_ENV_ARM_PUSH || env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT) ? 2
         : env_kind == SOFTROD_ENV_CRAWL ? 24 : env_kind == SOFTROD_ENV_ARM_TWO ? 18 : env_kind == SOFTROD_ENV_REACH ? 480 : 1;
}
int softrod_obs_dim(int env_kind) {
    return env_kind == SOFTROD_ENV_SOFTPENDULUM3D ? 9 : env_kind == SOFTROD_ENV_ARM_SINGLE ? 25
         : env_kind == SOFTROD_ENV_OCTO_FLAT ? 8 * 56 + 13 : env_kind == SOFTROD_ENV_SOFT_ARM ? 14
         : (env_kind == SOFTROD_ENV_ARM_PUSH || env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT) ? 84
         : env_kind == SOFTROD_ENV_CRAWL ? 8 * 131 : env_kind == SOFTROD_ENV_ARM_TWO ? 2 * 52 : env_kind == SOFTROD_ENV_REACH ? 8 * 189 : 4;
}
int softrod_config_action_dim(const softrod_config* cfg) {
    if (!cfg) return 0;
    if (cfg->env_kind == SOFTROD_ENV_SOFT_ARM) return 2 * cfg->n_ctrl;     // soft_arm_tracking.py:152-157
    if (cfg->env_kind == SOFTROD_ENV_ARM_PUSH || cfg->env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT)
        return cfg->arm_push_mode == 0 ? 1 : 2;                             // arm_push_env.py:100-118
    if (mocto_kind(cfg->env_kind)) return cfg->n_arm * cfg->n_knots;        // crawl_env.py:84-88, arm_two_env.py:84-89, reach_env.py:79-84
    return cfg->env_kind == SOFTROD_ENV_OCTO_FLAT ? cfg->n_arm * cfg->n_knots : softrod_action_dim(cfg->env_kind);
}
int softrod_config_obs_dim(const softrod_config* cfg) {
    if (!cfg) return 0;
    if (cfg->env_kind == SOFTROD_ENV_SOFT_ARM) return 2 * cfg->n_ctrl + 6;  // :158-163
    if (cfg->env_kind == SOFTROD_ENV_ARM_PUSH || cfg->env_kind == SOFTROD_ENV_ARM_PULL_WEIGHT)
        return 2 * (cfg->n_elem + 1) + 2;                                   // arm_push_env.py:104,118-120
    if (mocto_kind(cfg->env_kind)) {
        const int n = cfg->n_elem, na = cfg->n_arm, nk = cfg->n_knots;
        if (cfg->env_kind == SOFTROD_ENV_ARM_TWO) return na * ((n - 1) * 2 + nk + na + 3);          // arm_two_env.py:92-95
        return na * ((n - 1) + (n + 1) * 4 + nk + na + (cfg->env_kind == SOFTROD_ENV_CRAWL ? 17 : 18));   // crawl_env.py:91-101, reach_env.py:87-91
    }
    if (cfg->env_kind != SOFTROD_ENV_OCTO_FLAT) return softrod_obs_dim(cfg->env_kind);
    return cfg->n_arm * ((cfg->n_elem - 1) + 4 * (cfg->n_elem + 1) + cfg->n_knots) + 13;
}
int softrod_aux_dim(int env_kind) { return env_kind == SOFTROD_ENV_SOFTPENDULUM3D ? 1 : 0; }

int softrod_config_softpendulum(softrod_config* cfg, int n_envs) {
    if (!cfg || n_envs < 1) return SOFTROD_EINVAL;
    config_common(cfg, n_envs);
    cfg->features = SOFTROD_FEATURES_SOFTPENDULUM;
    cfg->env_kind = SOFTROD_ENV_SOFTPENDULUM;
    cfg->base_length = 1.0;                             // build.py:23-26
    cfg->base_radius = 0.05;
    cfg->density = 1000.0;                              // build.py:18-22
    cfg->youngs_modulus = 1e6;
    cfg->shear_modulus = 1e6 / (2.0 * (1.0 + 0.5));     // PyElastica default (none passed)
    cfg->gravity[0] = 0.0; cfg->gravity[1] = -9.80665; cfg->gravity[2] = 0.0;  // build.py:87-91
    cfg->damping_constant = 2e-3;                       // build.py:108
    return SOFTROD_OK;
}

int softrod_config_softpendulum3d(softrod_config* cfg, int n_envs) {
    if (!cfg || n_envs < 1) return SOFTROD_EINVAL;
    config_common(cfg, n_envs);
    cfg->features = SOFTROD_FEATURES_SOFTPENDULUM3D;
    cfg->env_kind = SOFTROD_ENV_SOFTPENDULUM3D;
    cfg->filter_order = 7;                              // soft_pendulum_3d/build.py:82-85
    cfg->base_length = 1.0;                             // soft_pendulum_3d/build.py:55-64
    cfg->base_radius = 0.1;
    cfg->density = 4000.0;
    cfg->youngs_modulus = 1e6;
    cfg->shear_modulus = 1e6 / (2.0 * (1.0 + 0.5));
    cfg->gravity[0] = 0.0; cfg->gravity[1] = 0.0; cfg->gravity[2] = -9.80665;  // :73-76
    cfg->damping_constant = 1.0;                        // :77-81
    cfg->base_step = 1e-3;                              // soft_pendulum_3d.py:57
    cfg->base_limit = 0.5;                              // :58
    return SOFTROD_OK;
}

int softrod_config_arm_single(softrod_config* cfg, int n_envs) {
    if (!cfg || n_envs < 1) return SOFTROD_EINVAL;
    config_common(cfg, n_envs);
    cfg->features = SOFTROD_FEATURES_ARM_SINGLE;
    cfg->env_kind = SOFTROD_ENV_ARM_SINGLE;
    cfg->dt = 7.0e-5;                                   // octopus/arm_single_env.py:58
    cfg->n_substeps = (int)(1.0 / (20 * cfg->dt));      // recording_fps = 20 (:59) -> 714 (:77)
    cfg->final_time = 10.0;                             // :57
    const double L0 = 0.35, r0 = 0.35 * 0.02;           // octopus/build.py:46-49
    cfg->base_length = L0;
    cfg->base_radius = r0;
    cfg->density = 1000.0;                              // :30-33
    cfg->youngs_modulus = 1e6;
    cfg->shear_modulus = 1e6 / (2.0 * (1.0 + 0.5));
    const double g = -9.81;                             // :237
    cfg->gravity[0] = 0.0; cfg->gravity[1] = 0.0; cfg->gravity[2] = g;
    cfg->damping_constant = 1e-2;                       // :285
    cfg->plane_origin[0] = 0.0; cfg->plane_origin[1] = 0.0; cfg->plane_origin[2] = -r0;  // :244
    cfg->plane_normal[0] = 0.0; cfg->plane_normal[1] = 0.0; cfg->plane_normal[2] = 1.0;  // :233
    cfg->contact_k = 1e2;                               // :241
    cfg->contact_nu = 1e1;                              // :242
    cfg->slip_velocity_tol = 1e-8;                      // :245
    cfg->surface_tol = 1e-4;
    const double period = 2.0, froude = 0.1;
    const double mu = L0 / (period * period * std::fabs(g) * froude);   // :247
    const double fac[3] = {1.0, 1.5, 2.0};               // forward, backward, sideways (:253-256)
    for (int i = 0; i < 3; ++i) {
        cfg->kinetic_mu[i] = mu * fac[i];
        cfg->static_mu[i] = 2 * (mu * fac[i]);          // :257
    }
    cfg->control_penalty_coeff = 0.001;                 // arm_single_env.py:62
    cfg->target[0] = 1.0; cfg->target[1] = 0.0;         // :165
    cfg->kappa_range[0] = -49.33508476187419; cfg->kappa_range[1] = 49.33545827754751;          // :111
    cfg->kappa_rate_range[0] = -21.063520620377012; cfg->kappa_rate_range[1] = 24.664591289161944;  // :113
    return SOFTROD_OK;
}

int softrod_config_octo_flat(softrod_config* cfg, int n_envs) {
    const int rc = softrod_config_arm_single(cfg, n_envs);   // per-arm constants: build.py:30-49,134-200
    if (rc != SOFTROD_OK) return rc;
    cfg->features = SOFTROD_FEATURES_OCTO_FLAT;
    cfg->env_kind = SOFTROD_ENV_OCTO_FLAT;
    cfg->n_elem = 10;                                    // octopus/flat_env.py:62
    cfg->final_time = 5.0;                               // :58
    cfg->n_substeps = (int)(1.0 / (5 * cfg->dt));        // recording_fps = 5 (:60) -> 2857
    cfg->n_arm = 8;                                      // :61
    cfg->n_knots = 3;                                    // n_action (:63)
    cfg->head_radius = 0.04;                             // octopus/build.py:95-105
    cfg->head_density = 700.0;
    cfg->joint_k = 1e6;                                  // :117-132
    cfg->joint_nu = 1e-3;
    cfg->joint_kt = 1e0;
    cfg->head_center[0] = 0.0; cfg->head_center[1] = 0.0;          // Cylinder(start = (0, 0, -r0), e_z, e_y, 2 r0), :95-105
    cfg->head_center[2] = -cfg->base_radius + 2.0 * cfg->base_radius / 2;
    cfg->head_length = 2.0 * cfg->base_radius;
    cfg->joint_angle0 = 0.0;
    cfg->joint_angle_step = 360 / (double)cfg->n_arm;    // :73-74
    return SOFTROD_OK;
}

int softrod_config_soft_arm(softrod_config* cfg, int n_envs) {
    if (!cfg || n_envs < 1) return fail(nullptr, SOFTROD_EINVAL, "bad argument");
    config_common(cfg, n_envs);
    cfg->features = SOFTROD_FEATURES_SOFT_ARM;
    cfg->env_kind = SOFTROD_ENV_SOFT_ARM;
    cfg->n_elem = 40;                                    // soft_arm/soft_arm_tracking.py:116
    cfg->dt = 2.0e-4;                                    // sim_dt, :117
    cfg->n_substeps = (int)std::rint(0.01 / cfg->dt);    // num_steps_per_update, :118-121
    cfg->final_time = 5.0;                               // max_episode_final_time, :127
    cfg->base_length = 1000.0;                           // :129 (millimetres)
    cfg->base_radius = 50.0;                             // :130
    cfg->density = 1000 * 1e-6;                          // :280
    cfg->youngs_modulus = 2e6;                           // :122
    cfg->shear_modulus = 2e6 / (2.0 * (1.0 + 0.5));      // not passed at :272-283: PyElastica's default
    cfg->damping_constant = 2e6 * 1e-7 * 1;              // :269
    cfg->n_ctrl = 4;                                     // :132
    cfg->n_spline_pieces = 3;                            // 4 + 2 points, not-a-knot
    cfg->muscle_torque_scale = 10 * 50.0 * 2e6;          // alpha, :350
    cfg->max_activation_rate = INFINITY;                 // :143
    cfg->arm_target[0] = cfg->arm_target[1] = cfg->arm_target[2] = 500.0;   // :147
    return SOFTROD_OK;
}

int softrod_config_arm_push(softrod_config* cfg, int n_envs, int mode) {
    if (!cfg || n_envs < 1 || (mode != 0 && mode != 1)) return fail(nullptr, SOFTROD_EINVAL, "bad argument");
    config_common(cfg, n_envs);
    cfg->features = SOFTROD_FEATURES_ARM_PUSH;
    cfg->env_kind = SOFTROD_ENV_ARM_PUSH;
    cfg->arm_push_mode = mode;                           // octopus/arm_push_env.py:90-97
    cfg->n_elem = 40;                                    // :88
    cfg->dt = 5.0e-5;                                    // :67
    cfg->n_substeps = (int)(1.0 / (40 * cfg->dt));       // recording_fps = 40 (:68) -> 500 (:85)
    cfg->final_time = 2.5;                               // :66
    cfg->base_length = 0.2;                              // L0, :160
    cfg->base_radius = 0.012;                            // radius_base, :161 (the taper: softrod_set_radius_profile)
    cfg->density = 700.0;                                // :174
    cfg->youngs_modulus = 1e4;                           // :175
    cfg->shear_modulus = 1e4 / 1.5;                      // :176
    cfg->damping_constant = 0.05 * 2 * 1e2;              // damp_coefficient * 1e2, :166,183
    cfg->n_suckers = 1;                                  // :187-195
    cfg->sucker_index[0] = 0;
    cfg->sucker_reduction_ratio = 1.0;                   // controllable_constraint.py:11
    cfg->damp_before_constrain = 1;                      // _build registers dampen() before constrain() (:180-195)
    cfg->n_muscles = 3;                                  // create_es_muscle_layers, octopus/build.py:295-338
    cfg->muscle_kind[0] = SOFTROD_MUSCLE_LONGITUDINAL;
    cfg->muscle_kind[1] = SOFTROD_MUSCLE_LONGITUDINAL;
    cfg->muscle_kind[2] = SOFTROD_MUSCLE_TRANSVERSE;
    cfg->muscle_fl_degree = 3;                           // Chang et al. 2023: max{3.06 l^3 - 13.64 l^2 + 18.01 l - 6.44, 0}
    cfg->muscle_fl_coef[0] = -6.44; cfg->muscle_fl_coef[1] = 18.01; cfg->muscle_fl_coef[2] = -13.64; cfg->muscle_fl_coef[3] = 3.06;
    cfg->muscle_equiv_load_form = 0;
    cfg->muscle_position_current_radius = 1;
    cfg->muscle_tm_length_law = 0;
    return SOFTROD_OK;
}

int softrod_config_arm_pull_weight(softrod_config* cfg, int n_envs) {
    const int rc = softrod_config_arm_push(cfg, n_envs, 1);      // registered with mode "continuous" (gym_softrobot/__init__.py:48-52)
    if (rc != SOFTROD_OK) return rc;
    cfg->features = SOFTROD_FEATURES_ARM_PULL_WEIGHT;
    cfg->env_kind = SOFTROD_ENV_ARM_PULL_WEIGHT;
    cfg->dt = 2.5e-5;                                    // octopus/arm_push_env.py:518
    cfg->n_substeps = (int)(1.0 / (40 * cfg->dt));       // 1000
    cfg->damping_constant = 0.05 * 2 * 5e2;              // :549
    cfg->sucker_reduction_ratio = 0.9;                   // :591-599
    cfg->n_arm = 1; cfg->n_knots = 1;
    const double rigid_rod_radius = 0.015, radius_base = 0.012;     // :524,554
    cfg->head_radius = rigid_rod_radius;
    cfg->head_density = 700 * 1.0;                       // :565
    cfg->head_length = radius_base * 2;                  // :553
    cfg->head_center[0] = -rigid_rod_radius * 0.9;       // start (:555-558) + direction * length / 2
    cfg->head_center[1] = 0.0;
    cfg->head_center[2] = -2 * radius_base + radius_base * 2 / 2;
    cfg->joint_k = 1e6; cfg->joint_nu = 1e-2; cfg->joint_kt = 1e0;   // :577-589
    cfg->joint_angle0 = 0.0; cfg->joint_angle_step = 0.0;
    return SOFTROD_OK;
}

int softrod_config_muscle_octopus(softrod_config* cfg, int n_envs, int env_kind) {
    if (!cfg || n_envs < 1 || !mocto_kind(env_kind)) return fail(nullptr, SOFTROD_EINVAL, "bad argument");
    const int rc = softrod_config_arm_push(cfg, n_envs, 1);      // the three layers and the recalled COOMM switches
    if (rc != SOFTROD_OK) return rc;
    cfg->features = SOFTROD_FEATURES_ARM_PULL_WEIGHT;
    cfg->env_kind = env_kind;
    cfg->n_elem = 20;                                    // crawl_env.py:65, arm_two_env.py:59, reach_env.py:57
    cfg->dt = 5.0e-5;                                    // :63 / :57 / :55
    cfg->n_substeps = (int)(1.0 / (25 * cfg->dt));       // recording_fps 25 -> 800
    cfg->final_time = env_kind == SOFTROD_ENV_CRAWL ? 10.0 : 5.0;
    // build_muscle_octopus.py:26-47 ARM_MATERIAL / DEFAULT_SCALE_LENGTH / HEAD_PROPERTIES
    cfg->base_length = 0.25;
    cfg->base_radius = 0.013;                            // r0; the arms' radii: linspace(0.013, 0.0042, n) through softrod_set_radius_profile
    cfg->density = 1000.0;
    cfg->youngs_modulus = 1.5e4;
    cfg->shear_modulus = 1.5e4 / (1.0 + 0.5);
    cfg->damping_constant = 0.20 * 1e-2;                 // damping_constant * nu_scale (:101-106)
    cfg->damper_time_step = 7e-5;                        // the dampers' own time_step (:105)
    cfg->n_arm = env_kind == SOFTROD_ENV_ARM_TWO ? 2 : 8;
    cfg->n_knots = env_kind == SOFTROD_ENV_CRAWL ? 3 : (env_kind == SOFTROD_ENV_ARM_TWO ? 9 : 3 * cfg->n_elem);
    cfg->head_radius = 0.04;
    cfg->head_density = 50.0;
    cfg->head_length = 0.013 * 2;                        // Cylinder(start (0, 0, -2 r0), e_z, e_y, 2 r0, head_radius, density) (:108-114)
    cfg->head_center[0] = 0.0; cfg->head_center[1] = 0.0; cfg->head_center[2] = -0.013 * 2 + 0.013 * 2 / 2;
    cfg->head_fixed = env_kind == SOFTROD_ENV_REACH ? 1 : 0;      // OneEndFixedBC on the head (reach_env.py:126-130)
    cfg->joint_k = 1e6; cfg->joint_kt = 1e2; cfg->joint_nu = 1e-3;
    if (env_kind == SOFTROD_ENV_ARM_TWO) {               // build_two_arms (:200-203); three suckers per arm (arm_two_env.py:76-80,126-139)
        cfg->joint_angle0 = 90.0; cfg->joint_angle_step = 180.0;
        cfg->n_suckers = 3;
        for (int j = 0; j < 3; ++j) cfg->sucker_index[j] = cfg->n_elem / (3 * 2) * (2 * j + 1);
    } else {                                             // build_octopus_muscles (:83-86); CrawlEnv: one sucker per arm (crawl_env.py:146-155)
        cfg->joint_angle0 = 45.0 / 2; cfg->joint_angle_step = 45.0;
        cfg->n_suckers = env_kind == SOFTROD_ENV_CRAWL ? 1 : 0;
        cfg->sucker_index[0] = 0;
    }
    cfg->sucker_reduction_ratio = 1.0;
    cfg->damp_before_constrain = 1;                      // the builds dampen(), the envs constrain() afterwards
    return SOFTROD_OK;
}

int softrod_create(const softrod_config* cfg, int device, softrod_handle** out) {
    if (!cfg || !out) return fail(nullptr, SOFTROD_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(softrod_config))
        return fail(nullptr, SOFTROD_EINVAL, "softrod_config.struct_size mismatch");
    if (const char* why = config_why_not(*cfg)) return fail(nullptr, SOFTROD_EINVAL, why);
    int ndev = 0;
    const hipError_t cnt_err = hipGetDeviceCount(&ndev);
    if (cnt_err != hipSuccess || ndev < 1)
        return fail(nullptr, SOFTROD_ENODEV,
                    std::string("no HIP device visible: hipGetDeviceCount -> ") +
                        hipGetErrorString(cnt_err) + ", count " + std::to_string(ndev));
    if (device < 0 || device >= ndev) return fail(nullptr, SOFTROD_EINVAL, "device out of range");
    softrod_handle* h = new (std::nothrow) softrod_handle;
    if (!h) return fail(nullptr, SOFTROD_ENOMEM, "host allocation failed");
    h->cfg = *cfg;
    h->device = device;
    shape_handle(h);
    const bool mocto = is_mocto(h);
    const size_t N = (size_t)cfg->n_envs;
    const size_t adim = (size_t)softrod_config_action_dim(cfg);
    const size_t rowb = N * kLanes * h->epl * h->nw * sizeof(double);
    int rc = SOFTROD_OK;
    // every step of the set-up runs only while the ones before it succeeded; what was made is released with the handle
    auto zeroed = [&](auto& buf, size_t bytes) {        // zero-filled
        if (rc == SOFTROD_OK && buf.alloc(bytes, true) != hipSuccess) rc = buf.get() ? SOFTROD_EHIP : SOFTROD_ENOMEM;
    };
    auto alloc = [&](auto*& p, size_t bytes) {          // into h->owned: the buffer lives as long as the handle
        DeviceBuf<unsigned char> buf;
        zeroed(buf, bytes);
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(buf.get());
        if (buf.get()) h->owned.push_back(std::move(buf));
    };
    auto pinned = [&](auto& buf, size_t bytes) {
        if (rc == SOFTROD_OK && buf.alloc(bytes) != hipSuccess) rc = SOFTROD_ENOMEM;
    };
    auto event = [&](Event& ev) {
        if (rc == SOFTROD_OK && ev.create(hipEventDisableTiming) != hipSuccess) rc = SOFTROD_EHIP;
    };
    auto upload = [&](void* dst, const void* src, size_t bytes) {
        if (rc == SOFTROD_OK && hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = SOFTROD_EHIP;
    };
    DeviceGuard guard_(device);
    if (guard_.err != hipSuccess) rc = SOFTROD_EHIP;
    alloc(h->S.pos, 3 * rowb);
    alloc(h->S.vel, 3 * rowb);
    alloc(h->S.dir, 9 * rowb);
    alloc(h->S.omg, 3 * rowb);
    alloc(h->S.tan, 3 * rowb);
    alloc(h->S.time, N * sizeof(double));
    alloc(h->S.bc, 12 * N * sizeof(double));
    alloc(h->S.ctrl, 4 * N * sizeof(double));
    alloc(h->S.kap, 3 * rowb);
    alloc(h->S.rkap, 3 * rowb);
    alloc(h->S.envmem, rowb);
    alloc(h->S.prev_action, N * (adim > 7 ? adim : 7) * sizeof(float));
    alloc(h->S.head, 20 * N * sizeof(double));
    // planar certificates, all 0 = unknown: for the handles a SoftPendulum planar kernel may step (StepRow.cert)
    if (cfg->math_mode == SOFTROD_MATH_FAST && cfg->features == SOFTROD_FEATURES_SOFTPENDULUM &&
        cfg->env_kind == SOFTROD_ENV_SOFTPENDULUM) {
        alloc(h->S.planar_cert, N + 1);
        const uint8_t on = 1;       // byte N, the switch (softrod_set_planar_certificates)
        if (h->S.planar_cert) upload(h->S.planar_cert + N, &on, 1);
    }
    alloc(h->d_spline, (size_t)(SOFTROD_MAX_SPLINE_PIECES + 1 + SOFTROD_MAX_SPLINE_PIECES * 4 * 4) * sizeof(double));
    h->P.spline = h->d_spline;
    alloc(h->d_ticket, sizeof(unsigned));    // softrod_scatter_rows' arrival counter, zero
    alloc(h->d_params, sizeof(RodParams));
    h->S.params = h->d_params;
    alloc(h->d_state, sizeof(StatePtrs));
    h->S.self = h->d_state;
    if (cfg->n_substeps > 0) {
        const std::vector<double> tab = clock_table(*cfg);
        alloc(h->d_time_tab, tab.size() * sizeof(double));
        upload(h->d_time_tab, tab.data(), tab.size() * sizeof(double));
        h->S.time_tab = h->d_time_tab;
        h->P.tab_len = (int)tab.size();
        h->P.tab_n_sub = cfg->n_substeps;
        h->P.inv_step_time = 1.0 / ((double)cfg->n_substeps * cfg->dt);
    }
    upload(h->d_params, &h->P, sizeof(RodParams));
    const size_t NS = N * (size_t)(mocto ? cfg->n_arm : 1);      // SuckerControllers: per env, per ARM of the muscle octopus
    alloc(h->S.sucker, (size_t)SOFTROD_MAX_SUCKERS * NS * sizeof(double));
    alloc(h->S.sucker_idx, (size_t)SOFTROD_MAX_SUCKERS * NS * sizeof(int));
    // [8][N] row 0: the step's time-limit flag (softrod_state_view.env_aux); the muscle octopus envs' target and xposbefore
    if (cfg->early_termination || mocto) alloc(h->S.aux, (size_t)8 * N * sizeof(double));
    if (mocto) alloc(h->S.prev_kappa, N * (size_t)cfg->n_arm * (size_t)(cfg->n_elem - 1) * sizeof(float));
    {
        std::vector<int> idx((size_t)SOFTROD_MAX_SUCKERS * NS, 0);
        for (int j = 0; j < SOFTROD_MAX_SUCKERS; ++j)
            for (size_t e = 0; e < NS; ++e) idx[(size_t)j * NS + e] = cfg->sucker_index[j];
        upload(h->S.sucker_idx, idx.data(), idx.size() * sizeof(int));
    }
    if (cfg->features & SOFTROD_FEAT_COOMM_MUSCLES) {
        alloc(h->S.mact, (size_t)SOFTROD_MAX_MUSCLES * rowb);
        alloc(h->d_mtab, (size_t)SOFTROD_MAX_MUSCLES * 4 * kLanes * h->epl * sizeof(double));
        h->S.mtab = h->d_mtab;
    }
    if (cfg->features & SOFTROD_FEAT_SUCKER_CONSTRAINT) {
        // the controllers are switched on after finalize (arm_push_env.py:222): effective ratio = the configured one
        std::vector<double> init((size_t)SOFTROD_MAX_SUCKERS * NS, 0.0);
        for (int j = 0; j < cfg->n_suckers; ++j)
            for (size_t e = 0; e < NS; ++e) init[(size_t)j * NS + e] = cfg->sucker_reduction_ratio;
        upload(h->S.sucker, init.data(), init.size() * sizeof(double));
    }
    {   // softrod_render draws every element with its rest radius
        const std::vector<double> radius((size_t)cfg->n_elem, cfg->base_radius);
        alloc(h->d_render_radius, radius.size() * sizeof(double));
        upload(h->d_render_radius, radius.data(), radius.size() * sizeof(double));
    }
    alloc(h->d_basis, (size_t)2 * kLanes * 7 * sizeof(double));
    h->S.basis = h->d_basis;
    zeroed(h->reset.init.dev, N * h->init_stride * sizeof(double));
    zeroed(h->reset.d_mask, N);
    pinned(h->reset.init.host, N * h->init_stride * sizeof(double));
    pinned(h->reset.h_mask, N);
    event(h->reset.init.ev);
    zeroed(h->pairs.dev, N * sizeof(int2));
    pinned(h->pairs.host, N * sizeof(int2));
    event(h->pairs.ev);
    h->is_dst.assign(N, 0);
    upload(h->d_state, &h->S, sizeof(StatePtrs));
    if (rc != SOFTROD_OK) {
        softrod_destroy(h);
        return fail(nullptr, rc, "device allocation failed");
    }
    *out = h;
    return SOFTROD_OK;
}

int softrod_reset_octo(softrod_handle* h, const double* arm_start, const double* arm_direction,
                       const double* target, const uint8_t* mask, void* stream) {
    if (!h || !arm_start || !arm_direction || !target) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!is_flat(h) && !is_mocto(h)) return fail(h, SOFTROD_EINVAL, "softrod_reset_octo is for SOFTROD_ENV_OCTO_FLAT and the muscle octopus envs");
    SR_ON_DEVICE(h);
    SR_HIP(h, h->reset.init.wait());
    const size_t N = (size_t)h->cfg.n_envs, na = (size_t)h->cfg.n_arm, td = octo_target_dim(h);
    double* const h_init = h->reset.init.host.get();
    uint8_t* const h_mask = h->reset.h_mask.get();
    double* tgt = h_init + N * na * 18;
    for (size_t e = 0; e < N; ++e) {
        if (mask) h_mask[e] = mask[e];
        if (mask && !mask[e]) continue;
        octo_record(h, arm_start + 3 * na * e, arm_direction + 3 * na * e, target + td * e, h_init + e * na * 18, tgt + td * e);
    }
    return upload_and_reset(h, (hipStream_t)stream, mask != nullptr);
}

// ---- device-side auto-reset ------------------------------------------------------------------
int softrod_autoreset_enable(softrod_handle* h, int depth) {
    if (!h || depth < 1 || depth > 4096) return fail(h, SOFTROD_EINVAL, "need 1 <= depth <= 4096");
    if (h->q.depth) return fail(h, SOFTROD_EINVAL, "auto-reset is already enabled");
    if (h->cfg.env_kind == SOFTROD_ENV_NONE) return fail(h, SOFTROD_EINVAL, "env_kind NONE has no episodes");
    SR_ON_DEVICE(h);
    arm_setup(h, "softrod_autoreset_enable");
    const size_t N = (size_t)h->cfg.n_envs;
    const size_t qb = (size_t)depth * N * h->init_stride * sizeof(double);
    ResetQueue q;
    SR_SETUP(h, q.ring.dev.alloc(qb));
    SR_SETUP(h, hipMemset(q.ring.dev.get(), 0, qb));
    SR_SETUP(h, q.ring.host.alloc(qb));
    SR_SETUP(h, q.d_consumed.alloc(N * sizeof(int)));
    SR_SETUP(h, q.d_produced.alloc(N * sizeof(int)));
    SR_SETUP(h, q.d_underflow.alloc(sizeof(int)));
    SR_SETUP(h, q.d_flags.alloc(2 * N));
    SR_SETUP(h, hipMemset(q.d_consumed.get(), 0, N * sizeof(int)));
    SR_SETUP(h, hipMemset(q.d_produced.get(), 0, N * sizeof(int)));
    SR_SETUP(h, hipMemset(q.d_underflow.get(), 0, sizeof(int)));
    SR_SETUP(h, hipMemset(q.d_flags.get(), 0, 2 * N));
    SR_SETUP(h, q.h_produced.alloc(N * sizeof(int)));
    std::memset(q.h_produced.get(), 0, N * sizeof(int));
    SR_SETUP(h, q.ring.ev.create(hipEventDisableTiming));
    q.stage_cap = 2 * N;      // pushes of more records than this upload the whole ring instead
    SR_SETUP(h, q.h_stage.alloc(q.stage_cap * h->init_stride * sizeof(double)));
    SR_SETUP(h, q.h_where.alloc(q.stage_cap * sizeof(int2)));
    SR_SETUP(h, q.d_stage.alloc(q.stage_cap * h->init_stride * sizeof(double)));
    SR_SETUP(h, q.d_where.alloc(q.stage_cap * sizeof(int2)));
    SR_SETUP(h, q.h_status.alloc((N + 1) * sizeof(int)));
    SR_SETUP(h, q.ev_status.create(hipEventDisableTiming));
    std::vector<int> seen(N, 0);
    // the device copy of the state pointers is the LAST thing to change: a failure above leaves it
    // (and h->S) exactly as it was, so the handle keeps stepping without auto-reset
    StatePtrs S = h->S;
    S.needs_reset = q.d_flags.get();
    S.skip = q.d_flags.get() + N;
    S.queue = q.ring.dev.get();
    S.q_consumed = q.d_consumed.get();
    S.q_produced = q.d_produced.get();
    S.q_underflow = q.d_underflow.get();
    S.q_depth = depth;
    S.q_record = (int)h->init_stride;
    SR_SETUP(h, hipMemcpy(h->d_state, &S, sizeof(StatePtrs), hipMemcpyHostToDevice));
    h->S = S;
    h->seen_consumed.swap(seen);
    q.depth = depth;
    h->q = std::move(q);
    return SOFTROD_OK;
}

int softrod_autoreset_same_step(softrod_handle* h, int on) {
    if (!h) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!h->q.depth) return fail(h, SOFTROD_EINVAL, "call softrod_autoreset_enable first");
    SR_ON_DEVICE(h);
    if (on && !h->final.obs.get()) {        // zero-filled
        arm_setup(h, "softrod_autoreset_same_step");
        const size_t N = (size_t)h->cfg.n_envs;
        FinalRows rows;
        SR_SETUP(h, rows.obs.alloc(N * (size_t)softrod_config_obs_dim(&h->cfg) * sizeof(float), true));
        SR_SETUP(h, rows.time.alloc(N * sizeof(double), true));
        SR_SETUP(h, rows.aux.alloc(N * sizeof(double), true));
        h->final = std::move(rows);
    }
    h->same_step = on != 0;
    return SOFTROD_OK;
}

int softrod_final_view(softrod_handle* h, float** final_obs, double** final_time, double** final_aux) {
    if (!h || !final_obs || !final_time || !final_aux) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!h->same_step) return fail(h, SOFTROD_EINVAL, "call softrod_autoreset_same_step first");
    *final_obs = h->final.obs.get();
    *final_time = h->final.time.get();
    *final_aux = h->final.aux.get();
    return SOFTROD_OK;
}

namespace {
// Next free record of env e, or nullptr if staging `count` more would overwrite records the
// device may not have consumed yet (as far as the last softrod_queue_status knows).
int queue_begin(softrod_handle* h, const int32_t* counts, int max_count) {
    if (!h->q.depth) return fail(h, SOFTROD_EINVAL, "call softrod_autoreset_enable first");
    if (!counts || max_count < 0) return fail(h, SOFTROD_EINVAL, "bad argument");
    const int N = h->cfg.n_envs;
    const int* const produced = h->q.h_produced.get();
    for (int e = 0; e < N; ++e) {
        if (counts[e] < 0 || counts[e] > max_count) return fail(h, SOFTROD_EINVAL, "counts[e] out of range");
        if (produced[e] + counts[e] - h->seen_consumed[e] > h->q.depth)
            return fail(h, SOFTROD_EINVAL, "reset queue overflow: staged + new records exceed depth");
    }
    SR_HIP(h, h->q.ring.wait());    // previous upload out of the pinned mirror
    return SOFTROD_OK;
}
// the next record of env e: its slot in the pinned mirror, counted as produced and noted for the commit
double* queue_slot(softrod_handle* h, int e) {
    const int k = h->q.h_produced.get()[e]++ % h->q.depth;
    h->pending.push_back(make_int2(e, k));
    return h->q.ring.host.get() + ((size_t)k * (size_t)h->cfg.n_envs + (size_t)e) * h->init_stride;
}
int queue_commit(softrod_handle* h, hipStream_t st) {
    const ResetQueue& q = h->q;
    const size_t N = (size_t)h->cfg.n_envs;
    const size_t M = h->pending.size(), R = h->init_stride;
    if (M > 0 && M <= q.stage_cap) {
        // only the records of this push cross PCIe: compacted copy + a scatter kernel
        for (size_t m = 0; m < M; ++m) {
            const int2 w = h->pending[m];
            std::memcpy(q.h_stage.get() + m * R, q.ring.host.get() + ((size_t)w.y * N + (size_t)w.x) * R, R * sizeof(double));
            q.h_where.get()[m] = w;
        }
        SR_HIP(h, hipMemcpyAsync(q.d_stage.get(), q.h_stage.get(), M * R * sizeof(double), hipMemcpyHostToDevice, st));
        SR_HIP(h, hipMemcpyAsync(q.d_where.get(), q.h_where.get(), M * sizeof(int2), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(softrod_queue_scatter_kernel, dim3((unsigned)M), dim3(kLanes), 0, st, q.ring.dev.get(), q.d_stage.get(),
                           q.d_where.get(), (int)N, (int)R);
        SR_HIP(h, hipGetLastError());
    } else if (M > 0) {
        SR_HIP(h, hipMemcpyAsync(q.ring.dev.get(), q.ring.host.get(), (size_t)q.depth * N * R * sizeof(double),
                                 hipMemcpyHostToDevice, st));
    }
    h->pending.clear();
    SR_HIP(h, hipMemcpyAsync(q.d_produced.get(), q.h_produced.get(), N * sizeof(int), hipMemcpyHostToDevice, st));
    SR_HIP(h, hipEventRecord(q.ring.ev.get(), st));
    return SOFTROD_OK;
}
}  // namespace

int softrod_queue_push(softrod_handle* h, const double* theta0, const int32_t* counts, int max_count,
                       void* stream) {
    if (!h || !theta0) return fail(h, SOFTROD_EINVAL, "null argument");
    if (is_octo(h)) return fail(h, SOFTROD_EINVAL, "rigid-body envs stage resets through softrod_queue_push_octo / _straight");
    SR_ON_DEVICE(h);
    const int rc = queue_begin(h, counts, max_count);
    if (rc != SOFTROD_OK) return rc;
    for (int e = 0; e < h->cfg.n_envs; ++e)
        for (int j = 0; j < counts[e]; ++j)
            theta_record(h, theta0[(size_t)e * max_count + j], queue_slot(h, e));
    return queue_commit(h, (hipStream_t)stream);
}

int softrod_queue_push_straight(softrod_handle* h, const double* start, const double* direction,
                                const double* normal, const int32_t* counts, int max_count, void* stream) {
    if (!h || !start || !direction || !normal) return fail(h, SOFTROD_EINVAL, "null argument");
    if (is_flat(h)) return fail(h, SOFTROD_EINVAL, "OctoFlat stages resets through softrod_queue_push_octo");
    SR_ON_DEVICE(h);
    const int rc = queue_begin(h, counts, max_count);
    if (rc != SOFTROD_OK) return rc;
    for (int e = 0; e < h->cfg.n_envs; ++e)
        for (int j = 0; j < counts[e]; ++j) {
            const size_t k = ((size_t)e * max_count + j) * 3;
            double* rec = queue_slot(h, e);
            straight_record(h, start + k, direction + k, normal + k, rec, rec + 18);
        }
    return queue_commit(h, (hipStream_t)stream);
}

int softrod_queue_push_octo(softrod_handle* h, const double* arm_start, const double* arm_direction,
                            const double* target, const int32_t* counts, int max_count, void* stream) {
    if (!h || !arm_start || !arm_direction || !target) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!is_flat(h) && !is_mocto(h)) return fail(h, SOFTROD_EINVAL, "softrod_queue_push_octo is for SOFTROD_ENV_OCTO_FLAT and the muscle octopus envs");
    SR_ON_DEVICE(h);
    const int rc = queue_begin(h, counts, max_count);
    if (rc != SOFTROD_OK) return rc;
    const size_t na = (size_t)h->cfg.n_arm, td = octo_target_dim(h);
    for (int e = 0; e < h->cfg.n_envs; ++e)
        for (int j = 0; j < counts[e]; ++j) {
            double* rec = queue_slot(h, e);
            const size_t k = (size_t)e * max_count + j;
            octo_record(h, arm_start + 3 * na * k, arm_direction + 3 * na * k, target + td * k, rec, rec + na * 18);
        }
    return queue_commit(h, (hipStream_t)stream);
}

int softrod_queue_status(softrod_handle* h, int32_t* consumed, int32_t* underflow, void* stream) {
    if (!h || !consumed) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!h->q.depth) return fail(h, SOFTROD_EINVAL, "call softrod_autoreset_enable first");
    SR_ON_DEVICE(h);
    const size_t N = (size_t)h->cfg.n_envs;
    int uf = 0;
    SR_HIP(h, hipMemcpyAsync(consumed, h->q.d_consumed.get(), N * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SR_HIP(h, hipMemcpyAsync(&uf, h->q.d_underflow.get(), sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SR_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    for (size_t e = 0; e < N; ++e) h->seen_consumed[e] = consumed[e];
    if (underflow) *underflow = uf;
    return SOFTROD_OK;
}

int softrod_queue_status_begin(softrod_handle* h, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!h->q.depth) return fail(h, SOFTROD_EINVAL, "call softrod_autoreset_enable first");
    SR_ON_DEVICE(h);
    const size_t N = (size_t)h->cfg.n_envs;
    SR_HIP(h, hipMemcpyAsync(h->q.h_status.get(), h->q.d_consumed.get(), N * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SR_HIP(h, hipMemcpyAsync(h->q.h_status.get() + N, h->q.d_underflow.get(), sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SR_HIP(h, hipEventRecord(h->q.ev_status.get(), (hipStream_t)stream));
    h->status_pending = true;
    return SOFTROD_OK;
}

int softrod_queue_status_poll(softrod_handle* h, int wait, int32_t* consumed, int32_t* underflow) {
    if (!h || !consumed) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!h->status_pending) return fail(h, SOFTROD_EINVAL, "no softrod_queue_status_begin outstanding");
    SR_ON_DEVICE(h);
    const hipError_t q = wait ? hipEventSynchronize(h->q.ev_status.get()) : hipEventQuery(h->q.ev_status.get());
    if (q == hipErrorNotReady) return 0;
    if (q != hipSuccess) return fail(h, SOFTROD_EHIP, std::string("queue status event: ") + hipGetErrorString(q));
    const size_t N = (size_t)h->cfg.n_envs;
    const int* const status = h->q.h_status.get();
    for (size_t e = 0; e < N; ++e) { consumed[e] = status[e]; h->seen_consumed[e] = status[e]; }
    if (underflow) *underflow = status[N];
    h->status_pending = false;
    return 1;
}

int softrod_queue_advance(softrod_handle* h, const int32_t* by, void* stream) {
    if (!h || !by) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!h->q.depth) return fail(h, SOFTROD_EINVAL, "call softrod_autoreset_enable first");
    SR_ON_DEVICE(h);
    const int N = h->cfg.n_envs;
    // consumed += by (by < 0: := produced).  The device counters are only ever written by the
    // auto-reset pass, which is stream-ordered with these copies.
    std::vector<int> cons((size_t)N);
    SR_HIP(h, hipMemcpyAsync(cons.data(), h->q.d_consumed.get(), (size_t)N * sizeof(int), hipMemcpyDeviceToHost,
                             (hipStream_t)stream));
    SR_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    const int* const produced = h->q.h_produced.get();
    for (int e = 0; e < N; ++e) {
        int c = by[e] < 0 ? produced[e] : cons[(size_t)e] + by[e];
        if (c > produced[e]) c = produced[e];
        cons[(size_t)e] = c;
        h->seen_consumed[(size_t)e] = c;
    }
    SR_HIP(h, hipMemcpyAsync(h->q.d_consumed.get(), cons.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice,
                             (hipStream_t)stream));
    SR_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    return SOFTROD_OK;
}

int softrod_reset(softrod_handle* h, const double* theta0, const uint8_t* mask, void* stream) {
    if (!h || !theta0) return fail(h, SOFTROD_EINVAL, "null argument");
    if (is_octo(h)) return fail(h, SOFTROD_EINVAL, "rigid-body envs reset through softrod_reset_octo / softrod_reset_straight");
    SR_ON_DEVICE(h);
    SR_HIP(h, h->reset.init.wait());    // previous upload out of the pinned buffers
    const int N = h->cfg.n_envs;
    double* const h_init = h->reset.init.host.get();
    uint8_t* const h_mask = h->reset.h_mask.get();
    for (int e = 0; e < N; ++e) {
        if (mask) h_mask[e] = mask[e];
        if (mask && !mask[e]) continue;
        theta_record(h, theta0[e], h_init + (size_t)e * 18);
    }
    return upload_and_reset(h, (hipStream_t)stream, mask != nullptr);
}

int softrod_reset_straight(softrod_handle* h, const double* start, const double* direction,
                           const double* normal, const uint8_t* mask, void* stream) {
    if (!h || !start || !direction || !normal) return fail(h, SOFTROD_EINVAL, "null argument");
    if (is_flat(h)) return fail(h, SOFTROD_EINVAL, "OctoFlat resets through softrod_reset_octo");
    SR_ON_DEVICE(h);
    SR_HIP(h, h->reset.init.wait());
    const int N = h->cfg.n_envs;
    double* const h_init = h->reset.init.host.get();
    uint8_t* const h_mask = h->reset.h_mask.get();
    double* tgt = h_init + (size_t)N * 18;
    for (int e = 0; e < N; ++e) {
        if (mask) h_mask[e] = mask[e];
        if (mask && !mask[e]) continue;
        straight_record(h, start + 3 * e, direction + 3 * e, normal + 3 * e, h_init + (size_t)e * 18, tgt + 2 * (size_t)e);
    }
    return upload_and_reset(h, (hipStream_t)stream, mask != nullptr);
}

int softrod_set_spline_table(softrod_handle* h, const double* breaks, const double* coef) {
    if (!h || !breaks || !coef) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!(h->cfg.features & SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES))
        return fail(h, SOFTROD_EINVAL, "this handle has no spline muscles");
    const int np = h->cfg.n_spline_pieces, nc = h->cfg.n_ctrl;
    for (int p = 0; p < np; ++p)
        if (!(breaks[p + 1] > breaks[p])) return fail(h, SOFTROD_EINVAL, "breaks must ascend");
    std::vector<double> buf((size_t)SOFTROD_MAX_SPLINE_PIECES + 1 + (size_t)np * nc * 4, 0.0);
    for (int p = 0; p <= np; ++p) buf[p] = breaks[p];
    for (int i = 0; i < np * nc * 4; ++i) buf[SOFTROD_MAX_SPLINE_PIECES + 1 + i] = coef[i];
    SR_ON_DEVICE(h);
    SR_HIP(h, hipMemcpy(h->d_spline, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
    h->spline_set = true;
    return SOFTROD_OK;
}

// CosseratRod.straight_rod's allocation (elastica/rod/factory_function.py allocate(), recalled)
// with base_radius an ARRAY of n_elements radii (octopus/arm_push_env.py:160-179): the rows of
// kernels' per-lane material table.  Mirrors straight_rod() of oracle/softrod_oracle.c.
int softrod_set_radius_profile(softrod_handle* h, const double* radius) {
    if (!h || !radius) return fail(h, SOFTROD_EINVAL, "null argument");
    // two slots per lane: the ArmPush arm only (its two-slot rows of kStepRows)
    const bool two_slot_push = h->epl == 2 && h->cfg.features == SOFTROD_FEATURES_ARM_PUSH &&
                               h->cfg.env_kind == SOFTROD_ENV_ARM_PUSH && h->cfg.math_mode == SOFTROD_MATH_FAST;
    if ((is_octo(h) && !is_pull(h) && !is_mocto(h)) || (h->epl != 1 && !two_slot_push) || h->window_refresh > 0)
        return fail(h, SOFTROD_EINVAL, "tapered rods: one rod of up to 63 elements per env (126 for the ArmPush arm), "
                                       "or the muscle octopus' arms");
    if (h->was_reset) return fail(h, SOFTROD_EINVAL, "softrod_set_radius_profile must precede the first reset");
    const softrod_config& c = h->cfg;
    const int n = c.n_elem;
    for (int k = 0; k < n; ++k)
        if (!(radius[k] > 0.0)) return fail(h, SOFTROD_EINVAL, "radii must be positive");
    SR_ON_DEVICE(h);
    const int W = kLanes * h->epl;
    // the muscle octopus: every arm is this rod, `seg` slots apart — the table is built for one arm's slots and repeated
    const int period = is_mocto(h) ? h->P.seg : W;
    const double ddt = c.damper_time_step > 0.0 ? c.damper_time_step : c.dt;
    std::vector<double> T((size_t)kMatRows * W, 0.0);
    const double rest_len = c.base_length / (double)n;
    std::vector<double> mass((size_t)n + 1, 0.0), bend01((size_t)n), bend2((size_t)n);
    for (int k = 0; k < n; ++k) {
        const double r = radius[k];
        const double A0 = M_PI * r * r;
        const double I1 = A0 * A0 / (4.0 * M_PI), I3 = 2.0 * I1;
        const double J0 = I1 * (c.density * rest_len), J2 = I3 * (c.density * rest_len);
        T[(size_t)kMatJ0 * W + k] = J0; T[(size_t)kMatJ2 * W + k] = J2;
        T[(size_t)kMatInvJ0 * W + k] = 1.0 / J0; T[(size_t)kMatInvJ2 * W + k] = 1.0 / J2;
        T[(size_t)kMatShear01 * W + k] = c.alpha_c * c.shear_modulus * A0;
        T[(size_t)kMatShear2 * W + k] = c.youngs_modulus * A0;
        bend01[(size_t)k] = c.youngs_modulus * I1;
        bend2[(size_t)k] = c.shear_modulus * I3;
        const double volume = M_PI * (r * r) * rest_len;
        mass[(size_t)k] += 0.5 * c.density * volume;
        mass[(size_t)k + 1] += 0.5 * c.density * volume;
        T[(size_t)kMatR0s * W + k] = r * std::sqrt(rest_len);
        T[(size_t)kMatInvR0s * W + k] = 1.0 / (r * std::sqrt(rest_len));
    }
    for (int k = 0; k < n - 1; ++k) {      // rest-length-weighted average onto the Voronoi vertices
        T[(size_t)kMatBend01 * W + k] = (bend01[(size_t)k + 1] * rest_len + bend01[(size_t)k] * rest_len) / (rest_len + rest_len);
        T[(size_t)kMatBend2 * W + k] = (bend2[(size_t)k + 1] * rest_len + bend2[(size_t)k] * rest_len) / (rest_len + rest_len);
    }
    double ms = 0.0;
    for (int k = 0; k <= n; ++k) { T[(size_t)kMatMass * W + k] = mass[(size_t)k]; ms += mass[(size_t)k]; }
    for (int k = n + 1; k < period; ++k) T[(size_t)kMatMass * W + k] = 1.0;     // finite filler past the rod
    for (int k = 0; k < n; ++k) {          // AnalyticalLinearDamper's per-element coefficients
        double me = 0.5 * (mass[(size_t)k + 1] + mass[(size_t)k]);
        if (k == 0) me += 0.5 * mass[0];
        if (k == n - 1) me += 0.5 * mass[(size_t)n];
        const double l0 = c.damper_protocol == 1 ? -c.damping_constant * ddt : -c.damping_constant * ddt * me * T[(size_t)kMatInvJ0 * W + k];
        const double l2 = c.damper_protocol == 1 ? -c.damping_constant * ddt : -c.damping_constant * ddt * me * T[(size_t)kMatInvJ2 * W + k];
        T[(size_t)kMatDampLog0 * W + k] = l0; T[(size_t)kMatDampLog2 * W + k] = l2;
        T[(size_t)kMatDampR0 * W + k] = std::exp(l0); T[(size_t)kMatDampR2 * W + k] = std::exp(l2);
    }
    for (int k = n; k < period; ++k) {      // slots past the last element: harmless finite values
        T[(size_t)kMatInvJ0 * W + k] = 0.0; T[(size_t)kMatInvJ2 * W + k] = 0.0;
        T[(size_t)kMatDampR0 * W + k] = 1.0; T[(size_t)kMatDampR2 * W + k] = 1.0;
        T[(size_t)kMatR0s * W + k] = 1.0; T[(size_t)kMatInvR0s * W + k] = 1.0;
    }
    for (int row = 0; row < kMatRows; ++row)
        for (int k = period; k < W; ++k) T[(size_t)row * W + k] = T[(size_t)row * W + (k % period)];
    // the first call's table is a local until the uploads have succeeded, then joins h->owned; the StatePtrs upload
    // is the last of them and commits
    arm_setup(h, "softrod_set_radius_profile");
    DeviceBuf<unsigned char> table;
    double* mat = h->d_mat;
    if (!mat) {
        h->owned.reserve(h->owned.size() + 1);
        SR_SETUP(h, table.alloc(T.size() * sizeof(double), true));
        mat = (double*)table.get();
    }
    RodParams P = h->P;
    StatePtrs S = h->S;
    S.mat = mat;
    P.mass_total = ms;
    SR_SETUP(h, hipMemcpy(mat, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));
    SR_SETUP(h, hipMemcpy(h->d_render_radius, radius, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    SR_SETUP(h, hipMemcpy(h->d_params, &P, sizeof(RodParams), hipMemcpyHostToDevice));
    SR_SETUP(h, hipMemcpy(h->d_state, &S, sizeof(StatePtrs), hipMemcpyHostToDevice));
    if (table.get()) h->owned.push_back(std::move(table));
    h->d_mat = mat;
    h->P = P;
    h->S = S;
    h->tapered = true;
    return SOFTROD_OK;
}

int softrod_set_env_material(softrod_handle* h, const double* material, const uint8_t* mask, void* stream) {
    if (!h || !material) return fail(h, SOFTROD_EINVAL, "null argument");
    const softrod_config& c = h->cfg;
    const double own[4] = {c.youngs_modulus, c.shear_modulus, c.density, c.damping_constant};
    return set_env_table(h, h->env_mat, &StatePtrs::env_mat, kOptEnvMaterial, "softrod_set_env_material", "per-env material: env ",
                         material, own, mask, stream,
        [](const double* m) -> const char* {
            if (!(std::isfinite(m[0]) && std::isfinite(m[1]) && std::isfinite(m[2]) && std::isfinite(m[3])))
                return " has a non-finite value";
            return m[0] > 0.0 && m[1] > 0.0 && m[2] > 0.0 && m[3] >= 0.0 ? nullptr
                       : " needs E, G, density > 0 and damping constant >= 0";
        },
        [&c](const double* m, EnvMaterial& R) { env_material_row(c, m, R); });
}

int softrod_set_env_contact(softrod_handle* h, const double* contact, const uint8_t* mask, void* stream) {
    if (!h || !contact) return fail(h, SOFTROD_EINVAL, "null argument");
    const softrod_config& c = h->cfg;
    const double own[8] = {c.contact_k, c.contact_nu, c.kinetic_mu[0], c.kinetic_mu[1], c.kinetic_mu[2],
                           c.static_mu[0], c.static_mu[1], c.static_mu[2]};
    return set_env_table(h, h->env_contact, &StatePtrs::env_contact, kOptEnvContact, "softrod_set_env_contact", "per-env contact: env ",
                         contact, own, mask, stream,
        [](const double* v) -> const char* {
            for (int j = 0; j < 8; ++j) {
                if (!std::isfinite(v[j])) return " has a non-finite value";
                if (!(v[j] >= 0.0)) return " needs contact_k, contact_nu and every mu >= 0";
            }
            return nullptr;
        },
        [](const double* v, EnvContact& R) { env_contact_row(v, R); });
}

int softrod_set_muscle_layers(softrod_handle* h, const double* ratio_position, const double* strength) {
    if (!h || !ratio_position || !strength) return fail(h, SOFTROD_EINVAL, "null argument");
    if (!(h->cfg.features & SOFTROD_FEAT_COOMM_MUSCLES)) return fail(h, SOFTROD_EINVAL, "this handle has no COOMM muscles");
    const int n = h->cfg.n_elem, M = h->cfg.n_muscles;
    const int W = kLanes * h->epl;
    std::vector<double> T((size_t)SOFTROD_MAX_MUSCLES * 4 * W, 0.0);
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < n; ++k) {
            for (int i = 0; i < 3; ++i) {
                const double v = ratio_position[((size_t)m * 3 + i) * n + k];
                if (!std::isfinite(v)) return fail(h, SOFTROD_EINVAL, "ratio_position must be finite");
                T[((size_t)m * 4 + i) * W + k] = v;
            }
            const double st = strength[(size_t)m * n + k];
            if (!std::isfinite(st)) return fail(h, SOFTROD_EINVAL, "strength must be finite");
            T[((size_t)m * 4 + 3) * W + k] = st;
        }
    if (is_mocto(h))                        // every arm carries the same layers, `seg` slots apart
        for (int row = 0; row < SOFTROD_MAX_MUSCLES * 4; ++row)
            for (int k = h->P.seg; k < W; ++k) T[(size_t)row * W + k] = T[(size_t)row * W + (k % h->P.seg)];
    SR_ON_DEVICE(h);
    SR_HIP(h, hipMemcpy(h->d_mtab, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));
    h->muscles_set = true;
    return SOFTROD_OK;
}

int softrod_set_action_basis(softrod_handle* h, const double* basis) {
    if (!h || !basis) return fail(h, SOFTROD_EINVAL, "null argument");
    SR_ON_DEVICE(h);
    // SOFTROD_ENV_ARM_TWO: [n_elem][3], apply_X = basis @ activation (arm_two_env.py:237-245)
    if (is_mocto(h) && h->cfg.env_kind != SOFTROD_ENV_ARM_TWO) return fail(h, SOFTROD_EINVAL, "this env interpolates nothing");
    const size_t bytes = is_mocto(h) ? (size_t)h->cfg.n_elem * 3 * sizeof(double)
                                     : (size_t)(h->cfg.n_elem - 1) * (is_octo(h) ? h->cfg.n_knots : 7) * sizeof(double);
    SR_HIP(h, hipMemcpy(h->d_basis, basis, bytes, hipMemcpyHostToDevice));
    h->basis_set = true;
    return SOFTROD_OK;
}

namespace {
// what softrod_step and softrod_step_packed need of the handle before they launch
int step_preconditions(softrod_handle* h) {
    if ((h->cfg.features & SOFTROD_FEAT_REST_KAPPA_ACTION) && !h->basis_set)
        return fail(h, SOFTROD_EINVAL, "softrod_set_action_basis must be called before softrod_step");
    if ((h->cfg.features & SOFTROD_FEAT_SPLINE_MUSCLE_TORQUES) && !h->spline_set)
        return fail(h, SOFTROD_EINVAL, "softrod_set_spline_table must be called before softrod_step");
    if (h->cfg.env_kind == SOFTROD_ENV_NONE)
        return fail(h, SOFTROD_EINVAL, "env_kind NONE has no step epilogue; use softrod_substeps");
    if ((h->cfg.features & SOFTROD_FEAT_COOMM_MUSCLES) && !h->muscles_set)
        return fail(h, SOFTROD_EINVAL, "softrod_set_muscle_layers must be called before softrod_step");
    return SOFTROD_OK;
}
}  // namespace

int softrod_step(softrod_handle* h, const float* actions, float* obs, double* reward,
                 uint8_t* terminated, uint8_t* truncated, double* aux, void* stream) {
    if (!h || !actions || !obs || !reward || !terminated || !truncated)
        return fail(h, SOFTROD_EINVAL, "null argument");
    if (const int rc = step_preconditions(h)) return rc;
    SR_ON_DEVICE(h);
    return launch_step(h, actions, obs, reward, terminated, truncated, aux, h->cfg.n_substeps, 1, 0,
                       (hipStream_t)stream);
}

int softrod_step_packed(softrod_handle* h, const float* actions, float* packed, double* aux, void* stream) {
    if (!h || !actions || !packed) return fail(h, SOFTROD_EINVAL, "null argument");
    if (const int rc = step_preconditions(h)) return rc;
    SR_ON_DEVICE(h);
    return launch_step(h, actions, packed, nullptr, nullptr, nullptr, aux, h->cfg.n_substeps, 1, 1,
                       (hipStream_t)stream);
}

namespace {
struct PeerTable { float* p[SOFTROD_MAX_PEERS]; };
// One thread per 32-bit word of the local rows; every peer's copy of the row block is written from it
// with SYSTEM-scope write-through stores (sc0 sc1: nothing of them stays behind in this GPU's L2).
// tag_word >= 0: when every block's stores have been acknowledged, the LAST block to finish stores
// `tag` into word `tag_word` of every peer buffer (system-scope release) — a reader that finds the tag
// finds the rows (the buffers are uncached / fine-grained on the reader's side, softrod_exchange_alloc).
__global__ void __launch_bounds__(256) softrod_scatter_rows_kernel(const float* __restrict__ packed, PeerTable peers,
                                                                   int n_peers, size_t n_words, size_t offset,
                                                                   long long tag_word, unsigned tag,
                                                                   unsigned* __restrict__ ticket) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) {
        const float v = packed[i];
        for (int q = 0; q < n_peers; ++q)
            __hip_atomic_store(&peers.p[q][offset + i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (tag_word < 0) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");      // system scope
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned arrived = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == gridDim.x - 1) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch (stream-ordered)
            for (int q = 0; q < n_peers; ++q)
                __hip_atomic_store(reinterpret_cast<unsigned*>(peers.p[q]) + tag_word, tag, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
}  // namespace

int softrod_scatter_rows(softrod_handle* h, const float* packed, const uint64_t* peer_buffers, int n_peers,
                         int row_words, int64_t first_row, int64_t tag_word, uint32_t tag, void* stream) {
    if (!h || !packed || !peer_buffers) return fail(h, SOFTROD_EINVAL, "null argument");
    if (n_peers < 1 || n_peers > SOFTROD_MAX_PEERS || row_words < 1 || first_row < 0)
        return fail(h, SOFTROD_EINVAL, "need 1 <= n_peers <= SOFTROD_MAX_PEERS, row_words >= 1, first_row >= 0");
    SR_ON_DEVICE(h);
    PeerTable t{};
    for (int q = 0; q < n_peers; ++q) {
        if (!peer_buffers[q]) return fail(h, SOFTROD_EINVAL, "null peer buffer");
        t.p[q] = reinterpret_cast<float*>(static_cast<uintptr_t>(peer_buffers[q]));
    }
    // h->d_ticket was allocated and zeroed in softrod_create (a lazy hipMemset on the null stream is not
    // ordered before a launch on a non-blocking stream); ONE ticket per handle: tagged scatters of one
    // handle must be stream-ordered with each other (include/softrod.h)
    const size_t n_words = (size_t)h->cfg.n_envs * (size_t)row_words;
    const unsigned blocks = (unsigned)((n_words + 255) / 256);
    hipLaunchKernelGGL(softrod_scatter_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, packed, t,
                       n_peers, n_words, (size_t)first_row * (size_t)row_words, (long long)tag_word, (unsigned)tag,
                       h->d_ticket);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// -- exchange buffers of transport "p2p": memory the OTHER GPUs store into -----------------------
// A GPU's L2 does not snoop a peer's stores into its HBM: rows a peer has written are only certain to
// be what a local kernel reads if the lines cannot sit in the local L2 — so these buffers are UNCACHED
// (hipDeviceMallocUncached; fine-grained where that is refused), not ordinary coarse-grained
// allocations, which are coherent across devices at kernel boundaries of the WRITER only.
int softrod_exchange_alloc(int device, uint64_t bytes, void** dev_ptr, uint8_t* ipc_handle, int* memory_kind) {
    if (!dev_ptr || bytes == 0) return fail(nullptr, SOFTROD_EINVAL, "null argument");
    DeviceGuard guard_(device);
    if (guard_.err != hipSuccess) return fail(nullptr, SOFTROD_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err));
    void* p = nullptr;
    int kind = SOFTROD_EXCHANGE_UNCACHED;
    hipError_t e = hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        kind = SOFTROD_EXCHANGE_FINEGRAINED;
        e = hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocFinegrained);
    }
    if (e != hipSuccess) return fail(nullptr, SOFTROD_EHIP, std::string("hipExtMallocWithFlags: ") + hipGetErrorString(e));
    e = hipMemset(p, 0, (size_t)bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && ipc_handle) {
        hipIpcMemHandle_t hd;
        static_assert(sizeof(hd) == SOFTROD_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
        e = hipIpcGetMemHandle(&hd, p);
        if (e == hipSuccess) std::memcpy(ipc_handle, &hd, sizeof(hd));
    }
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(nullptr, SOFTROD_EHIP, std::string("exchange buffer set-up: ") + hipGetErrorString(e));
    }
    *dev_ptr = p;
    if (memory_kind) *memory_kind = kind;
    return SOFTROD_OK;
}

int softrod_exchange_open(int device, const uint8_t* ipc_handle, int owner_device, void** dev_ptr) {
    if (!ipc_handle || !dev_ptr) return fail(nullptr, SOFTROD_EINVAL, "null argument");
    DeviceGuard guard_(device);
    if (guard_.err != hipSuccess) return fail(nullptr, SOFTROD_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err));
    if (owner_device >= 0 && owner_device != device) {
        int can = 0;
        hipError_t e = hipDeviceCanAccessPeer(&can, device, owner_device);
        if (e != hipSuccess || !can)
            return fail(nullptr, SOFTROD_EHIP, "device " + std::to_string(device) + " cannot access peer " + std::to_string(owner_device));
        e = hipDeviceEnablePeerAccess(owner_device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            return fail(nullptr, SOFTROD_EHIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        (void)hipGetLastError();
    }
    hipIpcMemHandle_t hd;
    std::memcpy(&hd, ipc_handle, sizeof(hd));
    void* p = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(nullptr, SOFTROD_EHIP, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e));
    *dev_ptr = p;
    return SOFTROD_OK;
}

int softrod_exchange_close(int device, void* dev_ptr) {
    if (!dev_ptr) return SOFTROD_OK;
    DeviceGuard guard_(device);
    const hipError_t e = hipIpcCloseMemHandle(dev_ptr);
    return e == hipSuccess ? SOFTROD_OK : fail(nullptr, SOFTROD_EHIP, std::string("hipIpcCloseMemHandle: ") + hipGetErrorString(e));
}

int softrod_exchange_free(int device, void* dev_ptr) {
    if (!dev_ptr) return SOFTROD_OK;
    DeviceGuard guard_(device);
    (void)hipDeviceSynchronize();
    const hipError_t e = hipFree(dev_ptr);
    return e == hipSuccess ? SOFTROD_OK : fail(nullptr, SOFTROD_EHIP, std::string("hipFree: ") + hipGetErrorString(e));
}

int softrod_substeps(softrod_handle* h, const float* actions, int n, void* stream) {
    if (!h || n < 0) return fail(h, SOFTROD_EINVAL, "bad argument");
    if (actions && h->cfg.env_kind != SOFTROD_ENV_SOFTPENDULUM && h->cfg.env_kind != SOFTROD_ENV_NONE)
        return fail(h, SOFTROD_EINVAL, "softrod_substeps takes no actions for this env_kind");
    if ((h->cfg.features & SOFTROD_FEAT_COOMM_MUSCLES) && !h->muscles_set)
        return fail(h, SOFTROD_EINVAL, "softrod_set_muscle_layers must be called before softrod_substeps");
    SR_ON_DEVICE(h);
    return launch_step(h, actions, nullptr, nullptr, nullptr, nullptr, nullptr, n, 0, 0, (hipStream_t)stream);
}

int softrod_observe(softrod_handle* h, const float* prev_action, float* obs, void* stream) {
    if (!h || !obs) return fail(h, SOFTROD_EINVAL, "null argument");
    if (h->cfg.env_kind == SOFTROD_ENV_NONE) return fail(h, SOFTROD_EINVAL, "env_kind NONE has no observation");
    SR_ON_DEVICE(h);
    const dim3 grid((unsigned)h->cfg.n_envs), block(kLanes);
    if (is_mocto(h)) {
        // get_state on the resident state (prev_action: the resident copy); like the reference's it moves ArmTwoEnv's _prev_kappa
        if (prev_action) return fail(h, SOFTROD_EINVAL, "the muscle octopus envs observe with their resident prev_action (pass NULL)");
        hipLaunchKernelGGL(softrod_mocto_epilogue_kernel, grid, dim3(kLanes * h->nw), 0, (hipStream_t)stream, h->P, h->S, obs,
                           nullptr, nullptr, nullptr, 0, 0);
    } else if (observes_as_body(h))
        hipLaunchKernelGGL(softrod_octo_observe_kernel, grid, dim3(kLanes * h->nw), 0, (hipStream_t)stream,
                           h->P, h->S, prev_action, obs);
    else
        hipLaunchKernelGGL(by_epl(h, softrod_observe_kernel<1>, softrod_observe_kernel<2>), grid, block, 0,
                           (hipStream_t)stream, h->P, h->S, nullptr, prev_action, obs, nullptr, 0);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

namespace {
// The read-outs: one wave per rod of the handle's layout (softrod_readout.hpp), or one wave per env, which finds its
// rods itself (the joint read-out, softrod_joint_readout.hpp).
using ReadoutKernel = void (*)(RodParams, StatePtrs, int, int, int, double*);
enum class ReadoutGrid { kPerRod, kPerEnv };
int launch_readout(softrod_handle* h, ReadoutKernel kernel, double* out, void* stream, ReadoutGrid grid = ReadoutGrid::kPerRod) {
    SR_ON_DEVICE(h);
    const RodLayout y = rod_layout(h);
    const int waves = h->cfg.n_envs * (grid == ReadoutGrid::kPerEnv ? 1 : y.rods);
    hipLaunchKernelGGL(kernel, dim3((unsigned)waves), dim3(kLanes), 0, (hipStream_t)stream, h->P, h->S,
                       y.rods, y.lane_stride, y.arm_stride, out);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}
}  // namespace

int softrod_rod_energies(softrod_handle* h, double* out, void* stream) {
    if (!h || !out) return fail(h, SOFTROD_EINVAL, "null argument");
    return launch_readout(h, by_epl(h, softrod_rod_energies_kernel<1>, softrod_rod_energies_kernel<2>), out, stream);
}

int softrod_ground_reaction(softrod_handle* h, double* out, void* stream) {
    if (!h || !out) return fail(h, SOFTROD_EINVAL, "null argument");
    if (const char* why = ground_reaction_why_not(h)) return fail(h, SOFTROD_EINVAL, why);
    // The kernel's own test for an env of several rods is SOFTROD_FEAT_OCTO_HEAD; rod_layout's is OctoFlat or the muscle
    // octopus.  For every handle that gets here the two agree: of the rigid-head envs only OctoFlat is let through.
    return launch_readout(h, softrod_ground_reaction_kernel, out, stream);
}

int softrod_rod_strains(softrod_handle* h, double* out, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "rod strains: null handle");
    if (!out) return fail(h, SOFTROD_EINVAL, "rod strains: null output buffer");
    // every handle's resident rows have rod_layout's form, so there is no refusal list
    return launch_readout(h, by_epl(h, softrod_rod_strains_kernel<1>, softrod_rod_strains_kernel<2>), out, stream);
}

int softrod_muscle_loads(softrod_handle* h, double* out, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "muscle loads: null handle");
    if (!out) return fail(h, SOFTROD_EINVAL, "muscle loads: null output buffer");
    if (!(h->cfg.features & SOFTROD_FEAT_COOMM_MUSCLES)) return fail(h, SOFTROD_EINVAL, "muscle loads: this handle has no COOMM muscles");
    if (!h->muscles_set) return fail(h, SOFTROD_EINVAL, "muscle loads: softrod_set_muscle_layers has not been called");
    return launch_readout(h, by_epl(h, softrod_muscle_loads_kernel<1>, softrod_muscle_loads_kernel<2>), out, stream);
}

int softrod_joint_loads(softrod_handle* h, double* out, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "joint loads: null handle");
    if (!out) return fail(h, SOFTROD_EINVAL, "joint loads: null output buffer");
    if (!(h->cfg.features & SOFTROD_FEAT_OCTO_HEAD)) return fail(h, SOFTROD_EINVAL, "joint loads: this handle has no rigid body");
    return launch_readout(h, softrod_joint_loads_kernel, out, stream, ReadoutGrid::kPerEnv);
}

int softrod_rod_dynamics(softrod_handle* h, double* out, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "rod dynamics: null handle");
    if (!out) return fail(h, SOFTROD_EINVAL, "rod dynamics: null output buffer");
    if (const char* why = rod_dynamics_why_not(h)) return fail(h, SOFTROD_EINVAL, why);
    // The kernel's own test for a joint is SOFTROD_FEAT_OCTO_HEAD and its arm is readout_rod's: rod_layout gives the
    // weight-pulling arm (one rod per env) arm 0, which is the joint's own index there.
    return launch_readout(h, softrod_rod_dynamics_kernel, out, stream);
}

int softrod_copy_envs(softrod_handle* h, const int32_t* src, const int32_t* dst, int count, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "copy envs: null handle");
    const std::string why = copy_envs_why_not(h, src, dst, count);
    if (!why.empty()) return fail(h, SOFTROD_EINVAL, why);
    SR_ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    SR_HIP(h, h->pairs.wait());     // the previous call's pairs have left the staging buffer
    int2* const h_pairs = h->pairs.host.get();
    int n = 0;
    for (int i = 0; i < count; ++i)
        if (src[i] != dst[i]) h_pairs[n++] = make_int2(src[i], dst[i]);
    if (n == 0) return SOFTROD_OK;
    SR_HIP(h, copy_table_rows(h->env_mat, h_pairs, n));
    SR_HIP(h, copy_table_rows(h->env_contact, h_pairs, n));
    SR_HIP(h, h->pairs.send((size_t)n, st));
    hipLaunchKernelGGL(softrod_copy_envs_kernel, dim3((unsigned)n), dim3(kCopyThreads), 0, st, copy_table(h), h->pairs.dev.get());
    SR_HIP(h, hipGetLastError());
    if (h->S.planar_cert) h->cert_live = true;      // (a certificate may have travelled with its rows)
    return SOFTROD_OK;
}

// ---- the state bank (softrod_state_bank.hpp) ----
int softrod_bank_create(softrod_handle* h, int slots) {
    if (!h) return fail(h, SOFTROD_EINVAL, "bank create: null handle");
    if (h->q.depth > 0)
        return fail(h, SOFTROD_EINVAL, "bank create: not on a handle with device-side auto-reset (the pending-reset flags and "
                                       "the staged queue belong to each env's RNG future)");
    if (h->bank.slots)
        return fail(h, SOFTROD_EINVAL, "bank create: the handle already has a state bank of " + std::to_string(h->bank.slots) + " slots");
    if (slots < 1) return fail(h, SOFTROD_EINVAL, "bank create: slots " + std::to_string(slots) + " is not positive");
    SR_ON_DEVICE(h);
    arm_setup(h, "softrod_bank_create");
    StateBank bank;
    bank.slots = slots;
    const size_t most = (size_t)(slots > h->cfg.n_envs ? slots : h->cfg.n_envs);
    const char* const what = "bank create: ";
    const CopyTable T = copy_table(h);      // a twin, zeroed, of every per-env array the handle has
    for (int k = 0; k < T.n; ++k)
        if (const int rc = bank_twin(h, slots, T.a[k].base, T.a[k].comps, T.a[k].row_bytes, bank.twins, what, true)) return rc;
    SR_SETUP(h, bank.pairs.dev.alloc(most * sizeof(int2)), what, true);
    SR_SETUP(h, bank.pairs.host.alloc(most * sizeof(int2)), what, true);
    SR_SETUP(h, bank.pairs.ev.create(hipEventDisableTiming), what, true);
    try {
        bank.filled.assign((size_t)slots, 0);
        bank.seen.assign(most, 0);
        if (h->env_mat.dev.get()) bank.mat.assign((size_t)slots, EnvMaterial{});
        if (h->env_contact.dev.get()) bank.contact.assign((size_t)slots, EnvContact{});
    } catch (const std::bad_alloc&) {
        return fail(h, SOFTROD_ENOMEM, "bank create: out of host memory");
    }
    h->bank = std::move(bank);
    return SOFTROD_OK;
}

int softrod_bank_save(softrod_handle* h, const int32_t* envs, const int32_t* slots, int count, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "bank save: null handle");
    return bank_copy(h, envs, slots, count, false, stream);
}

int softrod_bank_load(softrod_handle* h, const int32_t* slots, const int32_t* envs, int count, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "bank load: null handle");
    return bank_copy(h, envs, slots, count, true, stream);
}

int softrod_bank_info(softrod_handle* h, int32_t* slots, uint64_t* bytes_per_slot, uint8_t* filled) {
    if (!h) return fail(h, SOFTROD_EINVAL, "bank info: null handle");
    if (!slots || !bytes_per_slot) return fail(h, SOFTROD_EINVAL, "bank info: null argument");
    const CopyTable T = copy_table(h);
    uint64_t bytes = 0;
    for (int k = 0; k < T.n; ++k) bytes += (uint64_t)T.a[k].comps * T.a[k].row_bytes;
    *slots = h->bank.slots;
    *bytes_per_slot = bytes;
    if (filled && h->bank.slots) std::memcpy(filled, h->bank.filled.data(), h->bank.filled.size());
    return SOFTROD_OK;
}

// ---- episode statistics (softrod_episode_stats.hpp) ----
int softrod_episode_stats_enable(softrod_handle* h, int ring) {
    if (!h) return fail(h, SOFTROD_EINVAL, "episode stats: null handle");
    if (ring < 0) return fail(h, SOFTROD_EINVAL, "episode stats: ring " + std::to_string(ring) + " is negative");
    SR_ON_DEVICE(h);
    arm_setup(h, "softrod_episode_stats_enable");
    const char* const what = "episode stats: ";
    const size_t N = (size_t)h->cfg.n_envs, K = (size_t)ring;
    DeviceBuf<unsigned char> block;
    EpisodeStats S{};
    if (ring > 0) {
        // one block: [N] arrays first, then the ring, then count, in the order they are taken below
        std::vector<size_t> at;
        if (const int rc = carve_block(h, what, {N * 8, N * 4, N, N * 4, N * 8, N * 4, N * 8, N, K * 8, K * 4, K * 8, K * 4, 8}, block, at))
            return rc;
        SR_SETUP(h, hipDeviceSynchronize(), what, true);
        unsigned char* const b = block.get();
        S.acc_return = (double*)(b + at[0]); S.acc_length = (int*)(b + at[1]);
        S.latch = b + at[2]; S.finished = (int*)(b + at[3]);
        S.ep_r = (double*)(b + at[4]); S.ep_l = (int*)(b + at[5]);
        S.ep_t = (double*)(b + at[6]); S.ep_mask = b + at[7];
        S.ring_r = (double*)(b + at[8]); S.ring_l = (int*)(b + at[9]);
        S.ring_t = (double*)(b + at[10]); S.ring_env = (int*)(b + at[11]);
        S.count = (unsigned long long*)(b + at[12]);
        S.n_envs = h->cfg.n_envs;
        S.ring = ring;
    }
    h->d_stats = std::move(block);      // hipFree of the old block waits for the device: no kernel still writes the old arrays
    h->stats = S;
    return SOFTROD_OK;
}

int softrod_episode_stats_update(softrod_handle* h, const double* reward, const uint8_t* terminated, const uint8_t* truncated,
                                 const double* end_time, int mode, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "episode stats: null handle");
    if (!h->stats.ring) return fail(h, SOFTROD_EINVAL, "episode stats: the feature is off (softrod_episode_stats_enable)");
    if (!reward || !terminated || !truncated) return fail(h, SOFTROD_EINVAL, "episode stats: null reward, terminated or truncated");
    if (mode < 0 || mode > 2) return fail(h, SOFTROD_EINVAL, "episode stats: mode " + std::to_string(mode) + " is outside 0 .. 2");
    SR_ON_DEVICE(h);
    hipLaunchKernelGGL(softrod_episode_stats_kernel, dim3(1), dim3(kStatsThreads), 0, (hipStream_t)stream, h->stats, reward,
                       terminated, truncated, end_time, mode);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

int softrod_episode_stats_reset(softrod_handle* h, const uint8_t* mask, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "episode stats: null handle");
    if (!h->stats.ring) return fail(h, SOFTROD_EINVAL, "episode stats: the feature is off (softrod_episode_stats_enable)");
    SR_ON_DEVICE(h);
    hipLaunchKernelGGL(softrod_episode_stats_clear_kernel, dim3((unsigned)((h->cfg.n_envs + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, h->stats, mask);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

int softrod_episode_stats_view(softrod_handle* h, struct softrod_episode_stats_view* out) {
    if (!h) return fail(h, SOFTROD_EINVAL, "episode stats: null handle");
    if (!out) return fail(h, SOFTROD_EINVAL, "episode stats: null argument");
    if (!h->stats.ring) return fail(h, SOFTROD_EINVAL, "episode stats: the feature is off (softrod_episode_stats_enable)");
    const EpisodeStats& S = h->stats;
    out->acc_return = S.acc_return; out->acc_length = S.acc_length; out->latch = S.latch; out->finished = S.finished;
    out->ep_r = S.ep_r; out->ep_l = S.ep_l; out->ep_t = S.ep_t; out->ep_mask = S.ep_mask;
    out->ring_r = S.ring_r; out->ring_l = S.ring_l; out->ring_t = S.ring_t; out->ring_env = S.ring_env;
    out->count = (uint64_t*)S.count;
    out->n_envs = S.n_envs;
    out->ring = S.ring;
    return SOFTROD_OK;
}

// ---- observation and reward normalisation (softrod_normalize.hpp) ----
namespace {
const char* const kNormOff = "normalize: the feature is off (softrod_normalize_enable)";
int norm_refuse(softrod_handle* h, const char* what, double v, const char* why) {
    char buf[96];
    snprintf(buf, sizeof buf, "normalize: %s %g %s", what, v, why);
    return fail(h, SOFTROD_EINVAL, buf);
}
// the records as the host writes them: [4][D + 1] rows mean, var, count, inv_std
void norm_records(std::vector<double>& rec, size_t W, const double* mean, const double* var, const double* count,
                  const double* ret, double epsilon) {
    rec.resize(4 * W);
    for (size_t d = 0; d < W; ++d) {
        const bool last = d + 1 == W;
        const double m = mean ? (last ? ret[0] : mean[d]) : 0.0, v = mean ? (last ? ret[1] : var[d]) : 1.0,
                     c = mean ? (last ? ret[2] : count[d]) : 1e-4;
        rec[d] = m; rec[W + d] = v; rec[2 * W + d] = c; rec[3 * W + d] = 1.0 / std::sqrt(v + epsilon);
    }
}
}  // namespace

int softrod_normalize_enable(softrod_handle* h, int obs_on, int reward_on, double gamma, double clip_obs, double clip_reward,
                             double epsilon) {
    const bool on = obs_on || reward_on;
    if (on && !(gamma >= 0.0 && gamma <= 1.0)) return norm_refuse(h, "gamma", gamma, "is outside [0, 1]");
    if (on && !(clip_obs > 0.0)) return norm_refuse(h, "clip_obs", clip_obs, "is not positive");
    if (on && !(clip_reward > 0.0)) return norm_refuse(h, "clip_reward", clip_reward, "is not positive");
    if (on && !(epsilon > 0.0)) return norm_refuse(h, "epsilon", epsilon, "is not positive");
    if (!h) return fail(h, SOFTROD_EINVAL, "normalize: null handle");
    SR_ON_DEVICE(h);
    arm_setup(h, "softrod_normalize_enable");
    const char* const what = "normalize: ";
    const size_t N = (size_t)h->cfg.n_envs, D = (size_t)softrod_config_obs_dim(&h->cfg), W = D + 1;
    DeviceBuf<unsigned char> block;
    NormState S{};
    if (on) {
        std::vector<double> rec;
        norm_records(rec, W, nullptr, nullptr, nullptr, nullptr, epsilon);
        // one block, in the order its arrays are taken below
        std::vector<size_t> at;
        if (const int rc = carve_block(h, what, {4 * W * 8, N * 8, N, N * D * 4, N * D * 4, N * 8}, block, at)) return rc;
        unsigned char* const b = block.get();
        SR_SETUP(h, hipMemcpy(b + at[0], rec.data(), rec.size() * 8, hipMemcpyHostToDevice), what, true);
        SR_SETUP(h, hipDeviceSynchronize(), what, true);
        S.rec = (double*)(b + at[0]); S.ret = (double*)(b + at[1]); S.latch = b + at[2];
        S.norm_obs = (float*)(b + at[3]); S.norm_final_obs = (float*)(b + at[4]);
        S.norm_reward = (double*)(b + at[5]);
        S.n_envs = (int)N; S.obs_dim = (int)D;
        S.obs_on = obs_on ? 1 : 0; S.reward_on = reward_on ? 1 : 0;
        S.gamma = gamma; S.clip_obs = clip_obs; S.clip_reward = clip_reward; S.epsilon = epsilon;
    }
    h->d_norm = std::move(block);       // hipFree of the old block waits for the device: no kernel still writes the old arrays
    h->norm = S;
    return SOFTROD_OK;
}

int softrod_normalize_step(softrod_handle* h, const float* obs, const double* reward, const uint8_t* terminated,
                           const uint8_t* truncated, const float* final_obs, int mode, int update, void* stream) {
    if (mode < 0 || mode > 2) return fail(h, SOFTROD_EINVAL, "normalize: mode " + std::to_string(mode) + " is outside 0 .. 2");
    if (!obs || !reward || !terminated || !truncated) return fail(h, SOFTROD_EINVAL, "normalize: null obs, reward, terminated or truncated");
    if (final_obs && mode != 2) return fail(h, SOFTROD_EINVAL, "normalize: final_obs needs mode 2");
    if (!h) return fail(h, SOFTROD_EINVAL, "normalize: null handle");
    if (!h->norm.rec) return fail(h, SOFTROD_EINVAL, kNormOff);
    SR_ON_DEVICE(h);
    const NormState& S = h->norm;
    if (update) {
        const int tiles = S.obs_on ? (S.obs_dim + kNormTile - 1) / kNormTile : 0;
        hipLaunchKernelGGL(softrod_normalize_stats_kernel, dim3((unsigned)(tiles + S.reward_on)), dim3(kNormThreads), 0,
                           (hipStream_t)stream, S, tiles, obs, mode == 0 ? (const uint8_t*)S.latch : nullptr, false,
                           S.reward_on ? reward : nullptr);
        SR_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(softrod_normalize_rows_kernel, dim3((unsigned)((S.n_envs + kNormRowWaves - 1) / kNormRowWaves)),
                       dim3(kNormRowWaves * 64), 0, (hipStream_t)stream, S, obs, reward, terminated, truncated, final_obs, mode,
                       update ? 1 : 0);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

int softrod_normalize_reset(softrod_handle* h, const float* obs, const uint8_t* mask, int update, void* stream) {
    if (!obs) return fail(h, SOFTROD_EINVAL, "normalize: null obs");
    if (!h) return fail(h, SOFTROD_EINVAL, "normalize: null handle");
    if (!h->norm.rec) return fail(h, SOFTROD_EINVAL, kNormOff);
    SR_ON_DEVICE(h);
    const NormState& S = h->norm;
    if (update && S.obs_on) {
        const int tiles = (S.obs_dim + kNormTile - 1) / kNormTile;
        hipLaunchKernelGGL(softrod_normalize_stats_kernel, dim3((unsigned)tiles), dim3(kNormThreads), 0, (hipStream_t)stream, S,
                           tiles, obs, mask, true, (const double*)nullptr);
        SR_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(softrod_normalize_reset_kernel, dim3((unsigned)((S.n_envs + kNormRowWaves - 1) / kNormRowWaves)),
                       dim3(kNormRowWaves * 64), 0, (hipStream_t)stream, S, obs, mask);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

int softrod_normalize_view(softrod_handle* h, struct softrod_normalize_view* out) {
    if (!out) return fail(h, SOFTROD_EINVAL, "normalize: null argument");
    if (!h) return fail(h, SOFTROD_EINVAL, "normalize: null handle");
    if (!h->norm.rec) return fail(h, SOFTROD_EINVAL, kNormOff);
    const NormState& S = h->norm;
    const size_t D = (size_t)S.obs_dim, W = D + 1;
    out->obs_mean = S.rec; out->obs_var = S.rec + W; out->obs_count = S.rec + 2 * W; out->obs_inv_std = S.rec + 3 * W;
    out->ret_mean = S.rec + D; out->ret_var = S.rec + W + D; out->ret_count = S.rec + 2 * W + D;
    out->ret_inv_std = S.rec + 3 * W + D;
    out->ret = S.ret; out->latch = S.latch;
    out->norm_obs = S.norm_obs; out->norm_final_obs = S.norm_final_obs; out->norm_reward = S.norm_reward;
    out->n_envs = S.n_envs; out->obs_dim = S.obs_dim; out->obs_on = S.obs_on; out->reward_on = S.reward_on;
    out->gamma = S.gamma; out->clip_obs = S.clip_obs; out->clip_reward = S.clip_reward; out->epsilon = S.epsilon;
    return SOFTROD_OK;
}

int softrod_normalize_load(softrod_handle* h, const double* obs_mean, const double* obs_var, const double* obs_count,
                           const double* ret_mean, const double* ret_var, const double* ret_count, void* stream) {
    if (!obs_mean || !obs_var || !obs_count || !ret_mean || !ret_var || !ret_count)
        return fail(h, SOFTROD_EINVAL, "normalize: null argument");
    if (!h) return fail(h, SOFTROD_EINVAL, "normalize: null handle");
    if (!h->norm.rec) return fail(h, SOFTROD_EINVAL, kNormOff);
    SR_ON_DEVICE(h);
    const NormState& S = h->norm;
    const double ret[3] = {*ret_mean, *ret_var, *ret_count};
    std::vector<double> rec;
    norm_records(rec, (size_t)S.obs_dim + 1, obs_mean, obs_var, obs_count, ret, S.epsilon);
    SR_HIP(h, hipMemcpyAsync(S.rec, rec.data(), rec.size() * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
    SR_HIP(h, hipStreamSynchronize((hipStream_t)stream));       // `rec` dies with this call
    return SOFTROD_OK;
}

namespace {
// The env's target, where its kind has one: the point softrod_render draws (render.py draws the same) and
// softrod_rod_clearance measures to.
EnvTarget env_target(const softrod_handle* h) {
    const softrod_config& c = h->cfg;
    const size_t N = (size_t)c.n_envs;
    EnvTarget T{};
    switch (c.env_kind) {
        case SOFTROD_ENV_ARM_SINGLE: T.kind = 1; T.constant[0] = c.target[0]; T.constant[1] = c.target[1]; break;
        case SOFTROD_ENV_OCTO_FLAT: T.kind = 2; T.rows = h->S.head + 18 * N; T.dims = 2; break;
        case SOFTROD_ENV_CRAWL: case SOFTROD_ENV_ARM_TWO: T.kind = 2; T.rows = h->S.aux; T.dims = 2; break;
        case SOFTROD_ENV_REACH: T.kind = 2; T.rows = h->S.aux; T.dims = 3; break;
        case SOFTROD_ENV_SOFT_ARM: T.kind = 2; T.rows = h->S.ctrl + N; T.dims = 3; break;
        default: break;
    }
    return T;
}
}  // namespace

// ---- softrod_render (softrod_render.hpp) ----
int softrod_camera_default(const softrod_config* cfg, softrod_camera* cam) {
    if (!cfg || !cam) return fail(nullptr, SOFTROD_EINVAL, "render: null argument");
    std::memset(cam, 0, sizeof(*cam));
    cam->struct_size = (uint32_t)sizeof(softrod_camera);
    cam->width = 84;
    cam->height = 84;
    const double L = cfg->base_length;
    if (cfg->env_kind == SOFTROD_ENV_SOFTPENDULUM3D || cfg->env_kind == SOFTROD_ENV_SOFT_ARM) {
        // a fixed oblique view from (+x, -y, +z); the reset rod stands on the origin along z (SoftPendulum3D) or y
        cam->right[0] = 0.8; cam->right[1] = 0.6; cam->right[2] = 0.0;
        cam->up[0] = -0.36; cam->up[1] = 0.48; cam->up[2] = 0.8;
        cam->center[cfg->env_kind == SOFTROD_ENV_SOFT_ARM ? 1 : 2] = 0.5 * L;
        cam->half_width = 0.75 * L;
    } else {
        // the pendulum's plane seen along -z, the ground plane seen from above: x right, y up
        cam->right[0] = 1.0;
        cam->up[1] = 1.0;
        if (cfg->features & SOFTROD_FEAT_OCTO_HEAD) {
            cam->follow = 1;
            cam->half_width = 1.1 * (cfg->head_radius + L);
        } else {
            cam->half_width = 1.1 * L;
        }
    }
    cam->target_radius = 0.05 * L;
    cam->light[0] = -0.48; cam->light[1] = 0.6; cam->light[2] = 0.64;
    cam->ambient = 0.35;
    return SOFTROD_OK;
}

int softrod_camera_check(const softrod_camera* cam) {
    if (!cam) return fail(nullptr, SOFTROD_EINVAL, "render: null camera");
    if (cam->struct_size != sizeof(softrod_camera)) return fail(nullptr, SOFTROD_EINVAL, "render: softrod_camera.struct_size mismatch");
    if (cam->width < 1 || cam->width > 1024 || cam->height < 1 || cam->height > 1024)
        return fail(nullptr, SOFTROD_EINVAL, "render: width and height must be 1 .. 1024");
    const double* fields[] = {cam->center, cam->right, cam->up, cam->light};
    bool finite = std::isfinite(cam->half_width) && std::isfinite(cam->target_radius) && std::isfinite(cam->ambient);
    for (const double* f : fields)
        for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(f[i]);
    if (!finite) return fail(nullptr, SOFTROD_EINVAL, "render: a camera field is not finite");
    if (!(cam->half_width > 0.0)) return fail(nullptr, SOFTROD_EINVAL, "render: half_width must be positive");
    auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
    const double tol = 1e-6;
    if (std::fabs(std::sqrt(dot(cam->right, cam->right)) - 1.0) > tol || std::fabs(std::sqrt(dot(cam->up, cam->up)) - 1.0) > tol)
        return fail(nullptr, SOFTROD_EINVAL, "render: right and up must be unit vectors (to 1e-6)");
    if (std::fabs(dot(cam->right, cam->up)) > tol) return fail(nullptr, SOFTROD_EINVAL, "render: right and up must be orthogonal (to 1e-6)");
    if (std::fabs(std::sqrt(dot(cam->light, cam->light)) - 1.0) > tol)
        return fail(nullptr, SOFTROD_EINVAL, "render: light must be a unit vector (to 1e-6)");
    if (cam->ambient < 0.0 || cam->ambient > 1.0) return fail(nullptr, SOFTROD_EINVAL, "render: ambient must be in [0, 1]");
    if (cam->target_radius < 0.0) return fail(nullptr, SOFTROD_EINVAL, "render: target_radius must not be negative");
    if (cam->follow != 0 && cam->follow != 1) return fail(nullptr, SOFTROD_EINVAL, "render: follow must be 0 or 1");
    return SOFTROD_OK;
}

int softrod_render(softrod_handle* h, const softrod_camera* cam, uint8_t* rgb, float* depth, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "render: null handle");
    if (!cam) return fail(h, SOFTROD_EINVAL, "render: null camera");
    if (!rgb) return fail(h, SOFTROD_EINVAL, "render: null rgb buffer");
    if (softrod_camera_check(cam) != SOFTROD_OK) return fail(h, SOFTROD_EINVAL, g_err);
    const softrod_config& c = h->cfg;
    const RodLayout y = rod_layout(h);
    RenderScene sc{};
    sc.pos = h->S.pos;
    sc.head = is_octo(h) ? h->S.head : nullptr;
    sc.radius = h->d_render_radius;
    sc.head_radius = (float)c.head_radius;
    sc.n_envs = c.n_envs; sc.n_elem = c.n_elem; sc.rods = y.rods; sc.lane_stride = y.lane_stride; sc.arm_stride = y.arm_stride;
    sc.target = env_target(h);
    sc.n_prims = y.rods * c.n_elem + (sc.head ? 1 : 0) + (sc.target.kind ? 1 : 0);
    if (sc.n_prims > kRenderMaxPrims)
        return fail(h, SOFTROD_EINVAL, "render: more than " + std::to_string(kRenderMaxPrims) + " primitives per env");
    RenderCamera rc{};
    for (int i = 0; i < 3; ++i) {
        rc.c[i] = cam->center[i]; rc.a[i] = cam->right[i]; rc.b[i] = cam->up[i];
        rc.light[i] = (float)cam->light[i];
    }
    rc.n[0] = rc.a[1] * rc.b[2] - rc.a[2] * rc.b[1];
    rc.n[1] = rc.a[2] * rc.b[0] - rc.a[0] * rc.b[2];
    rc.n[2] = rc.a[0] * rc.b[1] - rc.a[1] * rc.b[0];
    rc.half_width = (float)cam->half_width; rc.target_radius = (float)cam->target_radius; rc.ambient = (float)cam->ambient;
    rc.width = cam->width; rc.height = cam->height; rc.follow = cam->follow;
    const int tiles_x = (cam->width + kRenderTileW - 1) / kRenderTileW, tiles_y = (cam->height + kRenderTileH - 1) / kRenderTileH;
    // a lane's 12 RGB bytes as three 32-bit stores, its four depths as one float4: whole groups of four pixels, aligned buffers
    if ((size_t)c.n_envs * (size_t)tiles_x * (size_t)tiles_y > (size_t)INT32_MAX)
        return fail(h, SOFTROD_EINVAL, "render: n_envs x tiles exceeds the grid (render a smaller frame)");
    const int wide = cam->width % kRenderPx == 0 && ((uintptr_t)rgb & 3u) == 0 && ((uintptr_t)depth & 15u) == 0;
    SR_ON_DEVICE(h);
    hipLaunchKernelGGL(softrod_render_kernel, dim3((unsigned)(c.n_envs * tiles_x * tiles_y)), dim3(kRenderThreads),
                       render_lds_bytes(sc.n_prims), (hipStream_t)stream, sc, rc, rgb, depth, tiles_x, tiles_y, wide);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// ---- softrod_rod_clearance (softrod_clearance.hpp) ----
int softrod_rod_clearance(softrod_handle* h, int self_gap, double* out, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "rod clearance: null handle");
    if (!out) return fail(h, SOFTROD_EINVAL, "rod clearance: null output buffer");
    if (self_gap < 2 || self_gap > 126) return fail(h, SOFTROD_EINVAL, "rod clearance: self_gap must be 2 .. 126");
    // every handle's resident rows have rod_layout's form, so there is no refusal list
    const softrod_config& c = h->cfg;
    const RodLayout y = rod_layout(h);
    const size_t waves = (size_t)c.n_envs * (size_t)(y.rods * (y.rods + 1) / 2 + y.rods);    // pairs a <= b, then the targets
    if (waves > (size_t)INT32_MAX) return fail(h, SOFTROD_EINVAL, "rod clearance: n_envs x record pairs exceeds the grid");
    SR_ON_DEVICE(h);
    hipLaunchKernelGGL(by_epl(h, softrod_rod_clearance_kernel<1>, softrod_rod_clearance_kernel<2>), dim3((unsigned)waves),
                       dim3(kLanes), 0, (hipStream_t)stream, h->S.pos, h->d_render_radius, env_target(h), c.n_envs, c.n_elem,
                       y.rods, y.lane_stride, y.arm_stride, self_gap, out);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// ---- softrod_set_rod_shape (softrod_shape.hpp) ----
int softrod_set_rod_shape(softrod_handle* h, const double* kappa, const double* sigma, const double* velocity,
                          const double* omega, const uint8_t* mask, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "set rod shape: null handle");
    // every handle's resident rows have rod_layout's form, so there is no refusal list
    SR_ON_DEVICE(h);
    if (const int rc = clear_planar_certs(h, (hipStream_t)stream)) return rc;
    const RodLayout y = rod_layout(h);
    const RodShapeArgs args{kappa, sigma, velocity, omega, mask, nullptr};
    hipLaunchKernelGGL(by_epl(h, softrod_rod_shape_kernel<1>, softrod_rod_shape_kernel<2>), dim3((unsigned)(h->cfg.n_envs * y.rods)),
                       dim3(kLanes), 0, (hipStream_t)stream, h->P, h->S, y.rods, y.lane_stride, y.arm_stride, args);
    SR_HIP(h, hipGetLastError());
    return SOFTROD_OK;
}

// ---- softrod_set_reset_shapes (softrod_reset_shapes.hpp) ----
uint32_t softrod_reset_shape_index(uint64_t seed, uint32_t env, uint32_t episode, uint32_t count) {
    return count ? reset_shape_index(seed, env, episode, count) : 0u;
}

int softrod_set_reset_shapes(softrod_handle* h, int count, const double* kappa, const double* sigma, const double* velocity,
                             const double* omega, uint64_t seed, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "set reset shapes: null handle");
    if (count < 0) return fail(h, SOFTROD_EINVAL, "set reset shapes: negative count");
    SR_ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)h->cfg.n_envs;
    const int n = h->cfg.n_elem;
    const size_t rows = (size_t)count * (size_t)rod_layout(h).rods * 3;
    const size_t width[4] = {(size_t)(n - 1), (size_t)n, (size_t)(n + 1), (size_t)n};
    const double* given[4] = {kappa, sigma, velocity, omega};
    arm_setup(h, "softrod_set_reset_shapes");
    const char* const what = "set reset shapes: ";
    ResetShapes& rs = h->rs;
    StateBank& bank = h->bank;
    // the new pool first: a failed call leaves the handle with the pool it had
    DeviceBuf<double> fresh[4];
    for (int f = 0; f < 4; ++f) {
        if (!count || !given[f]) continue;
        const size_t bytes = rows * width[f] * sizeof(double);
        SR_SETUP(h, fresh[f].alloc(bytes), what, false);
        SR_SETUP(h, hipMemcpyAsync(fresh[f].get(), given[f], bytes, hipMemcpyDeviceToDevice, st), what, false);
    }
    // the first pool of a handle: its three rows, zero-filled, and the bank's twins of the two that travel with an env
    // (no twins, no rows: copy_table must not list arrays the bank cannot follow)
    ResetShapes first;
    std::vector<StateBank::Twin> twins;
    if (count && !rs.index.get()) {
        SR_SETUP(h, first.index.alloc(N * sizeof(int), true), what, false);
        SR_SETUP(h, first.episode.alloc(N * sizeof(int), true), what, false);
        SR_SETUP(h, first.picked.alloc(N, true), what, false);
        if (bank.slots) {
            const char* const what_bank = "set reset shapes: state bank: ";
            if (const int rc = bank_twin(h, bank.slots, first.index.get(), 1, sizeof(int), twins, what_bank, false)) return rc;
            if (const int rc = bank_twin(h, bank.slots, first.episode.get(), 1, sizeof(int), twins, what_bank, false)) return rc;
            bank.twins.reserve(bank.twins.size() + 2);
        }
    }
    // a new pool starts a new sequence of starts: no env has a shaped start yet, every ordinal is zero
    int* const index = first.index.get() ? first.index.get() : rs.index.get();
    int* const episode = first.index.get() ? first.episode.get() : rs.episode.get();
    if (index) {
        SR_SETUP(h, hipMemsetAsync(index, 0xFF, N * sizeof(int), st));       // -1
        SR_SETUP(h, hipMemsetAsync(episode, 0, N * sizeof(int), st));
        if (bank.slots) {           // and so does every slot: it loads as its env would be now
            const size_t K = (size_t)bank.slots;
            SR_SETUP(h, hipMemsetAsync(twins.empty() ? bank.twin_of(index) : twins[0].dev.get(), 0xFF, K * sizeof(int), st));
            SR_SETUP(h, hipMemsetAsync(twins.empty() ? bank.twin_of(episode) : twins[1].dev.get(), 0, K * sizeof(int), st));
        }
    }
    // nothing below can fail
    if (first.index.get()) {
        rs.index = std::move(first.index);
        rs.episode = std::move(first.episode);
        rs.picked = std::move(first.picked);
        for (StateBank::Twin& t : twins) bank.twins.push_back(std::move(t));
    }
    // hipFree waits for the device: kernels still reading the old pool have finished
    for (int f = 0; f < 4; ++f) rs.field[f] = std::move(fresh[f]);
    rs.count = count;
    rs.seed = seed;
    return SOFTROD_OK;
}

int softrod_apply_reset_shapes(softrod_handle* h, const uint8_t* mask, void* stream) {
    if (!h) return fail(h, SOFTROD_EINVAL, "apply reset shapes: null handle");
    if (!h->rs.count) return fail(h, SOFTROD_EINVAL, "apply reset shapes: no pool is set (softrod_set_reset_shapes)");
    SR_ON_DEVICE(h);
    if (const int rc = clear_planar_certs(h, (hipStream_t)stream)) return rc;
    return launch_reset_shapes(h, kPickMask, mask, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
}

int softrod_reset_shapes_view(softrod_handle* h, int32_t** index, int32_t** episode) {
    if (!h) return fail(h, SOFTROD_EINVAL, "reset shapes view: null handle");
    if (!index || !episode) return fail(h, SOFTROD_EINVAL, "reset shapes view: null argument");
    if (!h->rs.count) return fail(h, SOFTROD_EINVAL, "reset shapes view: no pool is set (softrod_set_reset_shapes)");
    *index = h->rs.index.get();
    *episode = h->rs.episode.get();
    return SOFTROD_OK;
}

int softrod_state_view_get(softrod_handle* h, softrod_state_view* out) {
    if (!h || !out) return fail(h, SOFTROD_EINVAL, "null argument");
    // The pointers handed out may be written at any later time, on any stream: from here on the handle's step kernels
    // prove planarity at every launch again (softrod_set_planar_certificates alone switches the certificates back on).
    if (h->S.planar_cert && h->cert_on)
        if (const int rc = softrod_set_planar_certificates(h, 0)) return rc;
    out->n_envs = h->cfg.n_envs;
    out->n_elem = h->cfg.n_elem;
    const RodLayout y = rod_layout(h);
    out->lane_stride = y.lane_stride;
    out->arm_stride = y.arm_stride;
    out->position = h->S.pos;
    out->velocity = h->S.vel;
    out->director = h->S.dir;
    out->omega = h->S.omg;
    out->tangents = h->S.tan;
    out->time = h->S.time;
    out->control = h->S.ctrl;
    out->kappa = h->S.kap;
    out->rest_kappa = h->S.rkap;
    out->env_memory = h->S.envmem;
    out->prev_action = h->S.prev_action;
    out->head = h->S.head;
    out->bc_targets = h->S.bc;
    out->sucker_ratio = h->S.sucker;
    out->muscle_activation = h->S.mact;
    out->sucker_index = h->S.sucker_idx;
    out->material = h->d_mat;
    out->env_aux = h->S.aux;
    out->prev_kappa = h->S.prev_kappa;
    return SOFTROD_OK;
}

int softrod_set_planar_certificates(softrod_handle* h, int on) {
    if (!h) return fail(h, SOFTROD_EINVAL, "set planar certificates: null handle");
    if (!h->S.planar_cert) return SOFTROD_OK;       // nothing to switch: no kernel of this handle knows certificates
    SR_ON_DEVICE(h);
    // The switch is byte n_envs of the array, which the kernels read at every launch — a captured graph's too.  Behind
    // everything the device still has in flight: a launch enqueued under the old setting neither reads the new one
    // nor writes a certificate after the clear.
    SR_HIP(h, hipDeviceSynchronize());
    std::vector<uint8_t> bytes((size_t)h->cfg.n_envs + 1, 0);
    bytes.back() = on ? 1 : 0;
    SR_HIP(h, hipMemcpy(h->S.planar_cert, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    h->cert_live = false;
    h->cert_on = on != 0;
    return SOFTROD_OK;
}

int softrod_planar_certificates(softrod_handle* h, uint8_t* out, void* stream) {
    if (!h || !out) return fail(h, SOFTROD_EINVAL, "planar certificates: null argument");
    SR_ON_DEVICE(h);
    const size_t N = (size_t)h->cfg.n_envs;
    if (!h->S.planar_cert) SR_HIP(h, hipMemsetAsync(out, 0, N, (hipStream_t)stream));
    else SR_HIP(h, hipMemcpyAsync(out, h->S.planar_cert, N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SOFTROD_OK;
}

int softrod_set_timing(softrod_handle* h, int n_launches) {
    if (!h || n_launches < 0 || n_launches > (1 << 20)) return fail(h, SOFTROD_EINVAL, "bad argument");
    SR_ON_DEVICE(h);
    arm_setup(h, "softrod_set_timing");
    const size_t want = (size_t)n_launches, have = h->ev_start.size();
    std::vector<Event> start(want > have ? want - have : 0), stop(start.size());     // the pairs a longer ring adds
    for (size_t i = 0; i < start.size(); ++i) {
        SR_SETUP(h, start[i].create(hipEventDefault));
        SR_SETUP(h, stop[i].create(hipEventDefault));
    }
    h->ev_start.reserve(want);
    h->ev_stop.reserve(want);
    h->ev_start.resize(want < have ? want : have);      // a shorter ring drops its last pairs
    h->ev_stop.resize(h->ev_start.size());
    for (size_t i = 0; i < start.size(); ++i) {
        h->ev_start.push_back(std::move(start[i]));
        h->ev_stop.push_back(std::move(stop[i]));
    }
    h->timed = 0;
    return SOFTROD_OK;
}

int softrod_kernel_times_ms(softrod_handle* h, float* out_ms, int cap, int* count) {
    if (!h || !out_ms || !count || cap < 0) return fail(h, SOFTROD_EINVAL, "bad argument");
    SR_ON_DEVICE(h);
    const int n = h->timed < cap ? h->timed : cap;
    for (int i = 0; i < n; ++i) {
        SR_HIP(h, hipEventSynchronize(h->ev_stop[i].get()));
        SR_HIP(h, hipEventElapsedTime(out_ms + i, h->ev_start[i].get(), h->ev_stop[i].get()));
    }
    *count = n;
    return SOFTROD_OK;
}

int softrod_last_kernel_ms(softrod_handle* h, float* ms) {
    if (!h || !ms) return fail(h, SOFTROD_EINVAL, "null argument");
    if (h->timed < 1) return fail(h, SOFTROD_EINVAL, "timing not enabled or no timed launch yet");
    SR_ON_DEVICE(h);
    SR_HIP(h, hipEventSynchronize(h->ev_stop[h->timed - 1].get()));
    SR_HIP(h, hipEventElapsedTime(ms, h->ev_start[h->timed - 1].get(), h->ev_stop[h->timed - 1].get()));
    return SOFTROD_OK;
}

const char* softrod_last_error(softrod_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

// What select_step chooses for env.step (epilogue = 1), by its row's label.
const char* softrod_kernel_tier(softrod_handle* h) {
    if (!h) return "";
    const StepChoice c = select_step(h);
    std::string t = c.row ? c.row->label : std::string("none: ") + c.why;
    auto fill = [&t](const char* token, const std::string& with) {
        const size_t at = t.find(token);
        if (at != std::string::npos) t.replace(at, std::strlen(token), with);
    };
    fill("{waves}", std::to_string(h->nw) + (h->nw == 1 ? " wave" : " waves"));
    fill("{refresh}", std::to_string(h->window_refresh));
    if (c.row && c.row->windowed)
        if (const StepRow* after = select_step(h, 0).row) t += std::string(" + ") + after->label + " epilogue";
    if (h->env_mat.dev.get()) t += ",env material";
    if (h->env_contact.dev.get()) t += ",env contact";
    h->tier = t;
    return h->tier.c_str();
}

int softrod_destroy(softrod_handle* h) {
    if (!h) return SOFTROD_OK;
    DeviceGuard guard_(h->device);
    (void)hipDeviceSynchronize();
    delete h;       // every resource is a member that releases itself (softrod_owned.hpp)
    return SOFTROD_OK;
}

}  // extern "C"

#ifdef SOFTROD_PHASE_CLOCKS
// diagnostic build only: the phase stamps of the last step launch (tools/phase_clocks.py)
extern "C" int softrod_debug_phase_clocks(unsigned long long* out, int n_rods) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(softrod::g_phase_clock), (size_t)n_rods * 8 * sizeof(unsigned long long));
}
#endif
