// Same-step device auto-reset (softrod_autoreset_same_step; Gymnasium-1.x AutoresetMode.SAME_STEP).
//
// The NEXT_STEP passes (softrod_autoreset_kernel, softrod_octo_autoreset_kernel) run IN FRONT of a step: an env that
// finished at call t restarts at call t + 1 instead of stepping.  The two kernels here run BEHIND everything an
// env.step enqueues: an env whose step just ended its episode hands its terminal observation, clock and aux value out
// through the `final_*` buffers, consumes its next staged reset record, restarts, and has the new episode's first
// observation in its obs row when the call returns.  reward / terminated / truncated stay the finished step's own;
// `skip` is never set, so the next call steps the fresh episode with that call's action and no env ever idles.
//
// Cold path: the queue arithmetic, the reset and the observation are the calls the NEXT_STEP passes make
// (staged_record, record_target, reset_rod + observe_rod, octo_reset_env + observe_body), so both modes, a manual
// masked reset and the host-driven mode give the same bits.  The new buffers are kernel arguments: StatePtrs and RodParams
// keep their fields, and no step kernel knows this mode exists.
//
// An env that finds no staged record stays finished: its obs row keeps the final observation (final_obs holds the
// same row), needs_reset stays set, q_underflow counts it; the next call steps the finished episode again and goes on
// reporting truncated / terminated, as under NEXT_STEP.
#pragma once

namespace softrod {

// One 64-lane block per env: SoftPendulum, SoftPendulum3D, OctoArmSingle, SoftArmTracking, OctoArmPush, one or two
// slots per lane.  final_obs [N][obs_dim] is dense whatever `pack` is; final_time [N]; final_aux [N] (SoftPendulum3D's
// tilt, written only where the step wrote `aux`).
template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_autoreset_same_step_kernel(const RodParams P, const StatePtrs S, float* __restrict__ obs,
                                   double* __restrict__ aux, const int pack, float* __restrict__ final_obs,
                                   double* __restrict__ final_time, double* __restrict__ final_aux) {
    const int rod = blockIdx.x;
    const int lane = threadIdx.x;
    if (!S.needs_reset[rod]) return;           // (block-uniform: nothing below has written the flag yet)
    const size_t N = (size_t)P.n_envs;
    const int od = env_obs_dim(P);
    float* o = out_row(obs, rod, od, pack);
    const bool tilt = aux && P.env_kind == SOFTROD_ENV_SOFTPENDULUM3D;
    for (int i = lane; i < od; i += kLanes) final_obs[(size_t)od * rod + i] = o[i];
    if (lane == 0) {
        final_time[rod] = S.time[rod];
        if (tilt) final_aux[rod] = aux[rod];
    }
    const int k = S.q_consumed[rod];
    const double* in = staged_record(S, N, rod, k);
    if (!in) return;
    __syncthreads();                           // the finished row has been read before any lane overwrites it
    LaneN<EPL> L;
    reset_rod<EPL>(P, S, N, rod, lane, in, L); // (clears needs_reset and the clock)
    float pa[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) pa[i] = S.prev_action[7 * (size_t)rod + i];     // (after reset_rod cleared SoftPendulum3D's)
    observe_rod<EPL>(P, S, N, rod, lane, L, pa, obs, pack, aux);
    if (lane == 0) S.q_consumed[rod] = k + 1;
}

// One workgroup of kLanes * nw threads per env: OctoFlat / OctoFlatLite, OctoArmPullWeight and the muscle octopus envs
// (the record is softrod_octo_autoreset_kernel's: [n_arm][18] arm frames, then the target).  octo_reset_env's thread 0
// clears needs_reset, so every thread reads the flag and the counter before the first barrier and nothing is written
// to either until after it.
__global__ void __launch_bounds__(1024)
softrod_octo_autoreset_same_step_kernel(const RodParams P, const StatePtrs S, float* __restrict__ obs, const int pack,
                                        float* __restrict__ final_obs, double* __restrict__ final_time) {
    const int env = blockIdx.x;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const bool finished = S.needs_reset[env] != 0;
    const int k = S.q_consumed[env];
    const size_t N = (size_t)P.n_envs;
    const int od = body_obs_dim(P);
    float* o = out_row(obs, env, od, pack);
    if (finished) {
        for (int i = tid; i < od; i += nt) final_obs[(size_t)od * env + i] = o[i];
        if (tid == 0) final_time[env] = S.time[env];
    }
    __syncthreads();                           // every thread has read needs_reset / q_consumed and its part of the row
    if (!finished) return;
    const double* in = staged_record(S, N, env, k);
    if (!in) return;
    double tgt[4];
    record_target(P, in, tgt);
    LaneN<1> L;
    HeadState H;
    octo_reset_env(P, S, env, in, tgt, L, H);
    if (is_mocto_env(P.env_kind)) __syncthreads();     // thread 0's target rows are there (get_state reads them)
    observe_body(P, S, env, tid, L, H, tgt, S.prev_action, obs, pack);
    if (tid == 0) S.q_consumed[env] = k + 1;
}

}  // namespace softrod
