// softrod_readout.hpp — what the per-rod read-out kernels share, and the first of them.
//
// The read-outs are cold kernels beside the step kernels: softrod_rod_energies_kernel (here),
// softrod_rod_strains_kernel (softrod_strains.hpp), softrod_ground_reaction_kernel (softrod_reaction.hpp),
// softrod_muscle_loads_kernel (softrod_muscle_readout.hpp), softrod_rod_dynamics_kernel (softrod_dynamics_readout.hpp)
// and softrod_joint_loads_kernel (softrod_joint_readout.hpp).  The first five run one wave per rod — env
// blockIdx.x / rods, arm blockIdx.x % rods, its slots arm * arm_stride .. arm * arm_stride + n_elem of the env's row
// (`lane_stride` wide: the layouts of softrod_state_view) — so every rod's sums are a plain wave reduction; the joint
// loads run one wave per env, one arm per lane.  Slots past the rod are never read.
//
// readout_rod is that addressing; readout_load fills the wave's LaneN<EPL> from the resident rows and the
// boundary-condition targets as the energies, the strains and the muscle loads take them.  The ground reaction and
// the rod dynamics take only the addressing: their load is rod_literal_load's (softrod_literal.hpp), masked per element
// and Voronoi vertex, which also clears kappa and the tangents.
//
// WHO CALLS WHAT of the literal force evaluation (softrod_literal.hpp):
//   ground reaction   rod_literal_load, rod_literal_internal, rod_literal_joint, rod_literal_contact
//   rod dynamics      the last three of these and muscle_law_literal<1>; the masked load in its own words
//                     (softrod_dynamics_readout.hpp says why)
//   muscle loads      muscle_law_literal<EPL> on rod_strain_config_n's configuration (softrod_strains.hpp)
//   joint loads       joint_load_literal
//   energies, strains none: rod_energies_m and its restatement in softrod_strains.hpp (the early-termination step
//                     kernels inline the original)
#pragma once

namespace softrod {

// (N and W travel with the rod: with both formed inside readout_load the two-slot strains kernel compiles to 136
// VGPRs, with them here to the 134 it had.)
struct ReadoutRod {
    int rod, env, arm;     // blockIdx.x; its env; its arm within the env
    size_t N, W, base;     // envs; the width of an env's row; the rod's slot 0 within one component of the rows
};
__device__ __forceinline__ ReadoutRod readout_rod(const RodParams& P, int rods, int lane_stride, int arm_stride) {
    ReadoutRod R;
    R.N = (size_t)P.n_envs;
    R.W = (size_t)lane_stride;
    R.rod = blockIdx.x;
    R.env = R.rod / rods;
    R.arm = R.rod - R.env * rods;
    R.base = (size_t)R.env * R.W + (size_t)R.arm * (size_t)arm_stride;
    return R;
}

// x, v, omega, Q (and rest_kappa with SOFTROD_FEAT_REST_KAPPA_ACTION) of slots 0..n_elem, zero past the rod;
// B: the env's boundary-condition targets, the base position of SOFTROD_FEAT_MOVING_BASE_BC from its controls.
// Returns whether the rod has a boundary condition (B is loaded only then).
template <int EPL>
__device__ __forceinline__ bool readout_load(const RodParams& P, const StatePtrs& S, const ReadoutRod& R,
                                             int lane, LaneN<EPL>& L, BcTargets& B) {
    const bool rk = (P.features & SOFTROD_FEAT_REST_KAPPA_ACTION) != 0;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) { L.x[s][c] = L.v[s][c] = L.w[s][c] = L.rk[s][c] = 0.0; }
#pragma unroll
        for (int c = 0; c < 9; ++c) L.Q[s][c] = 0.0;
        if (j <= P.n_elem) {
            const size_t i = R.base + (size_t)j;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                L.x[s][c] = S.pos[c * R.N * R.W + i];
                L.v[s][c] = S.vel[c * R.N * R.W + i];
                L.w[s][c] = S.omg[c * R.N * R.W + i];
                if (rk) L.rk[s][c] = S.rkap[c * R.N * R.W + i];
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) L.Q[s][c] = S.dir[c * R.N * R.W + i];
        }
    }
    const bool bc = (P.features & (SOFTROD_FEAT_PENDULUM_BC | SOFTROD_FEAT_FIXED_BC | SOFTROD_FEAT_MOVING_BASE_BC)) != 0;
    if (bc) {
        load_bc(S, R.N, R.env, B);
        if (P.features & SOFTROD_FEAT_MOVING_BASE_BC) { B.pos[0] = S.ctrl[R.env]; B.pos[1] = S.ctrl[R.N + R.env]; }
    }
    return bc;
}

// softrod_rod_energies.  out: [n_envs][rods][4].
template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_rod_energies_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                            const int arm_stride, double* __restrict__ out) {
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    const int lane = threadIdx.x;
    LaneN<EPL> L;
    BcTargets B;
    const bool bc = readout_load<EPL>(P, S, R, lane, L, B);
    double E[4];
    rod_energies_m<EPL>(P, env_material_rt(P, S, R.env), S.mat, B, bc, lane, L, S.time[R.env], E);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(size_t)R.rod * 4 + i] = E[i];
    }
}

}  // namespace softrod
