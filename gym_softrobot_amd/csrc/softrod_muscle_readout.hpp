// softrod_muscle_readout.hpp — softrod_muscle_loads: what ApplyMuscles computes in every substep and returns none
// of (arm_push_env.py:197-212 over the layers of octopus/build.py:295-338) — every COOMM layer's force and length,
// the muscle internal force and couple, and the equivalent external loads they become — for every rod of every
// env, on the device.  PARITY UNPINNED, like softrod_muscle.hpp whose law this restates: COOMM is not on disk.
//
// A cold kernel beside the step kernels, of softrod_rod_strains_kernel's shape, addressing and load
// (softrod_readout.hpp: one wave per rod) — slot j = lane * EPL + s holds node j, element j and Voronoi vertex j.
// Neighbours come through shift_prev / shift_next only; no LDS, no atomics, no array indexed at run time.
//
// THE INSTANT is softrod_rod_strains': rod_strain_config_n (softrod_strains.hpp) rebuilds the configuration of the
// last force evaluation, or takes the state as it stands for an env whose time is 0.
// THE ACTIVATIONS are the resident rows StatePtrs.mact as they stand, read per element: after a step, what the last
// set_action wrote.  For an env whose time is not 0 rows 14-19 are therefore the loads the last substep's force
// evaluation added, to rounding — with ONE exception: the FAST OctoArmPush stepper in continuous mode applies
// element 0's value of the activation rows of layers 0 and 1 to every element (EnvAction.mu), while this kernel reads
// every element; the two agree only where those rows are uniform over the elements (what set_action itself writes).
//
// THE ARITHMETIC is muscle_law_literal<EPL>'s (softrod_literal.hpp), CALLED here as softrod_rod_dynamics_kernel calls
// it: the law in its literal form — FASTM = false: sqrt and IEEE division, no floating-point contraction — for
// handles of either math mode.  muscle_loads_n (softrod_muscle.hpp), inlined into the muscle step kernels, is the
// step kernels' text of the same law and stays untouched.  This kernel owns the instant and forms the
// law's inputs as libm_dynamic_step forms them (softrod_kernels.hpp), at the compiler's default contraction as
// softrod_strains.hpp's helpers are.  tests/test_gpu_muscle_loads.py holds this kernel to the NumPy twin
// diagnostics.muscle_loads_host, tests/test_muscle_loads.py that twin to the oracle's transcription.  Unlike the
// step kernels the law does NOT skip a layer whose amplitude is zero in the whole wave: the length rows are
// defined whatever the activation is.
//
// out: [n_envs][rods][20][n_elem + 1] —
//   rows 0-3    layer force F_m = activation strength max(fl(l_m), 0)                       n_elem columns
//   rows 4-7    layer length l_m = |nu_m| (|nu_m|^-1/2: transverse, muscle_tm_law 0)         n_elem
//   rows 8-10   muscle internal force f = sum F_m t_m, material frame                       n_elem
//   rows 11-13  muscle internal couple c_v = 1/2 (c_k + c_{k+1}), c = sum x_m x F_m t_m     n_elem - 1
//   rows 14-16  equivalent external force on the nodes, lab frame                           n_elem + 1
//   rows 17-19  equivalent external couple on the elements, material frame                  n_elem
// Every column past a row's range, and every row of a layer m >= n_muscles, is written as +0.0.
#pragma once

namespace softrod {

constexpr int kMuscleRows = 20;

template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_muscle_loads_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                            const int arm_stride, double* __restrict__ out) {
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    const int lane = threadIdx.x;
    const int n = P.n_elem;
    constexpr size_t TW = (size_t)kLanes * EPL;         // a row of the layer and the taper tables
    LaneN<EPL> L;
    BcTargets B;
    const bool bc = readout_load<EPL>(P, S, R, lane, L, B);     // slots past the rod are never read
    double x[EPL][3], Q[EPL][9], xn[EPL][3], Qn[EPL][9];
    rod_strain_config_n<EPL>(P, B, bc, lane, L, S.time[R.env], x, Q, xn, Qn);

    // ---- the inputs of the law, as libm_dynamic_step forms them: l, e, Q t, kappa, 1 / eps^3 ----
    double len[EPL], e[EPL], qt[EPL][3], kv[EPL][3];
    bool elem_valid[EPL], vor_valid[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        elem_valid[s] = j < n;
        vor_valid[s] = j < n - 1;
        len[s] = 0.0;
        e[s] = 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) qt[s][c] = kv[s][c] = 0.0;
        if (elem_valid[s]) {
            const double d0 = xn[s][0] - x[s][0], d1 = xn[s][1] - x[s][1], d2 = xn[s][2] - x[s][2];
            len[s] = sqrt(d0 * d0 + d1 * d1 + d2 * d2) + P.eps_length;
            const double t0 = d0 / len[s], t1 = d1 / len[s], t2 = d2 / len[s];
            e[s] = len[s] / P.rest_len;
            qt[s][0] = Q[s][0] * t0 + Q[s][1] * t1 + Q[s][2] * t2;
            qt[s][1] = Q[s][3] * t0 + Q[s][4] * t1 + Q[s][5] * t2;
            qt[s][2] = Q[s][6] * t0 + Q[s][7] * t1 + Q[s][8] * t2;
        }
        if (vor_valid[s]) slot_kappa(P, Q[s], Qn[s], kv[s]);
    }
    double lenn[EPL], e3v[EPL];
    shift_next<EPL>(len, lenn);                         // l_{k+1}: every lane takes part
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double vd = 0.5 * (lenn[s] + len[s]) / P.rest_vor;
        e3v[s] = vor_valid[s] ? 1.0 / (vd * vd * vd) : 1.0;
    }

    // ---- the law: softrod_literal.hpp's, every layer evaluated ----
    double r0s[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s)
        r0s[s] = (S.mat && elem_valid[s]) ? S.mat[(size_t)kMatR0s * TW + lane * EPL + s] : P.r0_sqrt_rest_len;
    MuscleLiteral<EPL> U;
    muscle_law_literal<EPL>(P, S, R.N, R.W, R.base, lane, Q, e, len, qt, kv, e3v, elem_valid, vor_valid, r0s, U);

    double* o = out + (size_t)R.rod * kMuscleRows * (size_t)(n + 1);
    const size_t nc = (size_t)(n + 1);
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        if (j <= n) {                                   // the n + 1 columns of every row, +0.0 past the row's range
#pragma unroll
            for (int m = 0; m < SOFTROD_MAX_MUSCLES; ++m) {
                o[(size_t)m * nc + j] = U.F[s][m];
                o[(size_t)(4 + m) * nc + j] = U.l[s][m];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[(size_t)(8 + c) * nc + j] = elem_valid[s] ? U.f[s][c] : 0.0;
                o[(size_t)(11 + c) * nc + j] = U.cv[s][c];
                o[(size_t)(14 + c) * nc + j] = U.fx[s][c];
                o[(size_t)(17 + c) * nc + j] = elem_valid[s] ? U.tq[s][c] : 0.0;
            }
        }
    }
}

}  // namespace softrod
