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
//   softrod_observe_kernel               (softrod_apply_reset_shapes leaves this one to the caller's softrod_observe)
//   / softrod_reset_shapes_octo_observe_kernel
//                                        the picked envs' observation rows again, from the shaped state and the resident
//                                        prev_action, into the dense or the packed row: softrod_observe's own one-rod
//                                        kernel with `picked` set (SoftPendulum3D's aux tilt follows as in the auto-reset
//                                        passes), or observe_body, the auto-reset passes' call, for the envs of several
//                                        arms (ArmTwoEnv's _prev_kappa moves as in any get_state)
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

// The picked envs' observation rows from the resident state, for the envs of several arms (OctoFlat / OctoFlatLite and
// the muscle octopus envs): one workgroup of kLanes * nw threads per env, as softrod_octo_observe_kernel.
__global__ void __launch_bounds__(1024)
softrod_reset_shapes_octo_observe_kernel(const RodParams P, const StatePtrs S, const uint8_t* __restrict__ picked,
                                         float* __restrict__ obs, const int pack) {
    const int env = blockIdx.x;
    if (!picked[env]) return;                    // block-uniform; no barrier below
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = blockDim.x >> 6;
    const size_t N = (size_t)P.n_envs, NR = N * (size_t)nw;
    LaneN<1> L;
    load_lane<1, kRuntimeFeatures>(S, NR, env * nw + wave, lane, L);
    HeadState H;
    double tgt[2];
    load_head(S, N, env, H, tgt);
    observe_body(P, S, env, tid, L, H, tgt, S.prev_action, obs, pack);
}

}  // namespace softrod
