// softrod_reset_shapes.hpp — shaped episode starts under every reset (softrod_set_reset_shapes).
//
// softrod_set_rod_shape shapes an env once; the staged records of device-side auto-reset are straight rods, so the shape
// is gone at the first automatic reset.  Here the handle keeps a resident POOL of start shapes — the four fields of
// softrod_set_rod_shape with a leading entry axis [count] — and every reset of an env, by hand or by either auto-reset
// pass, is followed by the shape of one entry of it.  Upstream has no counterpart: its builds call
// CosseratRod.straight_rod only (soft_pendulum/build.py:54-61 and the other build files).
//
// One cold pass of three small kernels, launched only while a pool is set:
//   softrod_reset_shapes_pick_kernel     one thread per env: did this call restart the env?  If so draw its entry
//                                        index = reset_shape_index(seed, e, episode[e], count), record it in index[e],
//                                        count the reset in episode[e] and mark the env in `picked`
//   softrod_rod_shape_kernel             softrod_shape.hpp itself, with mask = picked and pool_index = index: the same
//                                        statements as softrod_set_rod_shape, hence the same bits
//   softrod_reset_shapes_observe_kernel  (softrod_apply_reset_shapes leaves this one to the caller's softrod_observe)
//   / _octo_observe_kernel               the picked envs' observation rows again, from the shaped state, with the
//                                        statements of softrod_observe_kernel / softrod_octo_observe_kernel / the muscle
//                                        octopus' get_state, into the dense or the packed row; SoftPendulum3D's aux tilt
//                                        follows as in the auto-reset passes; ArmTwoEnv's _prev_kappa moves as in any
//                                        get_state
// WHICH ENVS A CALL RESTARTED is read from what the auto-reset passes leave behind, so no step kernel and no auto-reset
// kernel changes:
//   kPickMask      softrod_apply_reset_shapes: the caller's mask (the host-driven reset paths)
//   kPickSkipped   NEXT_STEP, between softrod_autoreset_kernel and the step: `skip` is set exactly for the envs the pass
//                  restarted (the step's epilogue clears it); an env that found no staged record has it clear
//   kPickFinished  SAME_STEP, behind softrod_autoreset_same_step_kernel: terminated | truncated of this call (the step
//                  writes both for every env: `skip` is never set in this mode) with needs_reset clear again — the
//                  restart clears the flag, an env that found no staged record keeps it
// A manual reset in a device mode never sets `skip` and leaves no flags of a finished step: it is shaped by
// softrod_apply_reset_shapes alone.  New buffers travel as kernel arguments: StatePtrs and RodParams keep their fields.
#pragma once

namespace softrod {

// The pool entry of env `env`'s reset number `episode` (include/softrod.h softrod_reset_shape_index): fixed integer
// arithmetic mod 2^64, the same on the host and on the device.
__host__ __device__ inline unsigned long long reset_shape_mix(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__host__ __device__ inline unsigned reset_shape_index(unsigned long long seed, unsigned env, unsigned episode, unsigned count) {
    const unsigned long long a = reset_shape_mix(seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)env + 1ull));
    return (unsigned)(reset_shape_mix(a + (unsigned long long)episode) % (unsigned long long)count);
}

enum : int { kPickMask = 0, kPickSkipped = 1, kPickFinished = 2 };
constexpr int kPickThreads = 256;

struct ResetShapesPick {
    int* index;               // [n_envs] the entry each env's current episode started from (-1: no shaped start yet)
    int* episode;             // [n_envs] resets counted so far = the next reset's ordinal
    uint8_t* picked;          // [n_envs] out: 1 for the envs this pass shapes, 0 for the others
    unsigned long long seed;
    int count;                // entries of the pool (>= 1)
    int mode;                 // kPick*
    const uint8_t* mask;      // kPickMask: [n_envs] or nullptr (every env)
    const uint8_t* terminated;   // kPickFinished, dense outputs: [n_envs] each
    const uint8_t* truncated;
    const float* packed;      // kPickFinished, step_packed rows (then terminated / truncated are nullptr): the flags
    int od;                   //   are bytes 0 and 1 of word od + (od & 1) + 2 of a row (out_row, emit_scalars)
};

__global__ void __launch_bounds__(kPickThreads)
softrod_reset_shapes_pick_kernel(const RodParams P, const StatePtrs S, const ResetShapesPick A) {
    const int e = blockIdx.x * kPickThreads + threadIdx.x;
    if (e >= P.n_envs) return;
    bool pick;
    if (A.mode == kPickMask) pick = !A.mask || A.mask[e] != 0;
    else if (A.mode == kPickSkipped) pick = S.skip[e] != 0;
    else {
        bool done;
        if (A.packed) {
            const float* row = A.packed + (size_t)e * (size_t)(A.od + (A.od & 1) + 4);
            done = (__float_as_int(row[A.od + (A.od & 1) + 2]) & 0x0101) != 0;
        } else
            done = (A.terminated[e] | A.truncated[e]) != 0;
        pick = done && !S.needs_reset[e];
    }
    A.picked[e] = pick ? 1 : 0;
    if (!pick) return;
    const int j = A.episode[e];
    A.index[e] = (int)reset_shape_index(A.seed, (unsigned)e, (unsigned)j, (unsigned)A.count);
    A.episode[e] = j + 1;
}

// The picked envs' observation rows from the resident state: softrod_observe_kernel's statements (prev_action: the
// resident copy), into the dense or the packed row.  One 64-lane block per env, the single-rod envs and the muscle arm
// with a weight, as softrod_observe launches them.
template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_reset_shapes_observe_kernel(const RodParams P, const StatePtrs S, const uint8_t* __restrict__ picked,
                                    float* __restrict__ obs, double* __restrict__ aux, const int pack) {
    const int rod = blockIdx.x;
    if (!picked[rod]) return;                    // block-uniform
    const int lane = threadIdx.x;
    const size_t N = (size_t)P.n_envs;
    LaneN<EPL> L;
    load_lane<EPL, kRuntimeFeatures>(S, N, rod, lane, L);
    EnvAction A;
#pragma unroll
    for (int i = 0; i < 7; ++i) A.a[i] = 0.0f;
    A.force = 0.0;
    A.mu_set = false;
    ConstN<EPL> C;
    const EnvMaterial E = env_material_rt(P, S, rod);
    if (S.mat) build_const_m<kRuntimeFeatures, EPL, true>(P, E, lane, A, C, S.mat);
    else build_const_m<kRuntimeFeatures, EPL>(P, E, lane, A, C);
    const int adim = (P.env_kind == SOFTROD_ENV_SOFTPENDULUM3D) ? 2
                   : (P.env_kind == SOFTROD_ENV_ARM_SINGLE) ? 7 : (P.env_kind == SOFTROD_ENV_SOFT_ARM) ? 0
                   : is_push_env(P.env_kind) ? (P.push_mode == 0 ? 1 : 2) : 1;
    float pa[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < adim; ++i) pa[i] = S.prev_action[7 * (size_t)rod + i];
    const int od = env_obs_dim(P);
    float* o = out_row(obs, rod, od, pack);
    env_observe_n<kRuntimeEnv, EPL>(P, S, N, rod, lane, C, L, pa, o);
    // the tilt the auto-reset passes report for a restarted env (lane 0 wrote o[8] itself)
    if (lane == 0 && aux && P.env_kind == SOFTROD_ENV_SOFTPENDULUM3D) aux[rod] = (double)o[8];
}

// The same for the envs of several arms: softrod_octo_observe_kernel's statements (OctoFlat / OctoFlatLite), or
// get_state of the muscle octopus envs as softrod_mocto_epilogue_kernel runs it without scalars.  One workgroup of
// kLanes * nw threads per env.
__global__ void __launch_bounds__(1024)
softrod_reset_shapes_octo_observe_kernel(const RodParams P, const StatePtrs S, const uint8_t* __restrict__ picked,
                                         float* __restrict__ obs, const int pack) {
    const int env = blockIdx.x;
    if (!picked[env]) return;                    // block-uniform; no barrier below
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = blockDim.x >> 6;
    const size_t N = (size_t)P.n_envs, NR = N * (size_t)nw;
    HeadState H;
    double tgt[2];
    load_head(S, N, env, H, tgt);
    if (is_mocto_env(P.env_kind)) {
        const size_t m = ((size_t)env * nw + wave) * kLanes + lane;
        double x[3], v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { x[c] = S.pos[c * NR * kLanes + m]; v[c] = S.vel[c * NR * kLanes + m]; }
        const double kap0 = S.kap[m];
        mocto_write_obs(P, S, env, tid, x, v, kap0, H, out_row(obs, env, mocto_obs_dim(P), pack));
    } else {
        LaneN<1> L;
        load_lane<1, kRuntimeFeatures>(S, NR, env * nw + wave, lane, L);
        const int adim = P.n_arm * P.n_action;
        octo_write_obs(P, tid, L, H, tgt, S.prev_action + (size_t)env * adim, out_row(obs, env, octo_obs_dim(P), pack));
    }
}

}  // namespace softrod
