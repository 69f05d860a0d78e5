// softrod_strains.hpp — softrod_rod_strains: the strains RodCallBack records once per env.step
// (utils/custom_elastica/callback_func.py:23-41: sigma, kappa, dilatation, voronoi_dilatation) and the passive
// elastic loads they stand for, for every rod of every env, on the device.
//
// A cold kernel beside the step kernels, of softrod_rod_energies_kernel's shape, addressing and load
// (softrod_readout.hpp: one wave per rod) — slot j = lane * EPL + s holds node j,
// element j and Voronoi vertex j, for one- and two-slot rods alike.  Neighbours come through shift_next (DPP wave
// shifts; the out-of-range lane reads 0); no LDS, no atomics, no array indexed at run time.
//
// THE INSTANT and the statements are rod_energies_m's (softrod_kernels.hpp): rod_strain_config_n rebuilds the
// configuration of the last force evaluation (x - dt/2 v, R(dt/2 omega)^T Q, then constrain_values; the state as
// it stands for an env whose time is 0), slot_sigma and slot_kappa form the strains, slot_shear and slot_bend pick
// the stiffness from RodParams, the env's EnvMaterial row or the tapered rod's table.  They are rod_energies_m's
// lines WRITTEN AGAIN here, not shared with it: rod_energies_m is inlined into the early-termination step
// kernels, and calling these functions from it changed those kernels' register allocation.  Change one and
// change the other; tests/test_gpu_rod_strains.py holds 1/2 sum sigma . n l^ and 1/2 sum (kappa - kappa^) . m D^
// of this buffer to the shear and bending energies of softrod_rod_energies at rtol 1e-12.  Floating-point
// contraction is left as rod_energies_m has it (the compiler's default).
//
// out: [n_envs][rods][14][n_elem] —
//   rows 0-2   sigma                       rows 8-10   n = S sigma
//   rows 3-5   kappa (not reduced by kappa^)  rows 11-13  m = B (kappa - kappa^)
//   row  6     dilatation e = l / l^      (kappa^ only with SOFTROD_FEAT_REST_KAPPA_ACTION)
//   row  7     voronoi dilatation (l_k + l_{k+1}) / (2 D^)
// Rows 3-5, 7 and 11-13 live on the n_elem - 1 Voronoi vertices: their last column is written as 0.
#pragma once

namespace softrod {

constexpr int kStrainRows = 14;

// rod_energies_m's statements again, piece by piece (softrod_kernels.hpp; see the note above).
// rod_strain_config_n: the configuration the strains are taken at — mid-substep (`time` != 0) or the state as it
// stands, after constrain_values — and its index+1 neighbours.
template <int EPL>
__device__ __forceinline__ void rod_strain_config_n(const RodParams& P, const BcTargets& B, bool bc, int lane,
                                                    const LaneN<EPL>& L, double time, double (&x)[EPL][3],
                                                    double (&Q)[EPL][9], double (&xn)[EPL][3], double (&Qn)[EPL][9]) {
    const bool mid = time != 0.0;
    const double h = P.half_dt;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
#pragma unroll
        for (int c = 0; c < 3; ++c) x[s][c] = mid ? L.x[s][c] - h * L.v[s][c] : L.x[s][c];
        // Q_mid = R^T Q with R the (transposed-Rodrigues) kinematic rotation of diagnostics.half_step_rotation
        const double* w = L.w[s];
        const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        const double ia = 1.0 / (th + P.eps_rot_axis);
        const double a0 = w[0] * ia, a1 = w[1] * ia, a2 = w[2] * ia;
        const double up = sin(th * h), usq = 1.0 - cos(th * h);
        double R[9];
        R[0] = 1.0 - usq * (a1 * a1 + a2 * a2);
        R[4] = 1.0 - usq * (a0 * a0 + a2 * a2);
        R[8] = 1.0 - usq * (a0 * a0 + a1 * a1);
        R[1] = up * a2 + usq * a0 * a1;
        R[3] = -up * a2 + usq * a0 * a1;
        R[2] = -up * a1 + usq * a0 * a2;
        R[6] = up * a1 + usq * a0 * a2;
        R[5] = up * a0 + usq * a1 * a2;
        R[7] = -up * a0 + usq * a1 * a2;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int l = 0; l < 3; ++l)
                Q[s][3 * i + l] = mid ? R[i] * L.Q[s][l] + R[3 + i] * L.Q[s][3 + l] + R[6 + i] * L.Q[s][6 + l]
                                      : L.Q[s][3 * i + l];
    }
    if (mid && bc && lane == 0) {   // constrain_values on node 0 / element 0 (constrain_values_host)
        if (P.features & SOFTROD_FEAT_PENDULUM_BC) {
            x[0][1] = B.pos[1]; x[0][2] = B.pos[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) { Q[0][j] = B.Q[j]; Q[0][6 + j] = B.Q[6 + j]; }
        }
        if (P.features & (SOFTROD_FEAT_FIXED_BC | SOFTROD_FEAT_MOVING_BASE_BC)) {
#pragma unroll
            for (int j = 0; j < 3; ++j) x[0][j] = B.pos[j];
#pragma unroll
            for (int j = 0; j < 9; ++j) Q[0][j] = B.Q[j];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], o[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = x[s][c];
        shift_next<EPL>(a, o);
#pragma unroll
        for (int s = 0; s < EPL; ++s) xn[s][c] = o[s];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        double a[EPL], o[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = Q[s][c];
        shift_next<EPL>(a, o);
#pragma unroll
        for (int s = 0; s < EPL; ++s) Qn[s][c] = o[s];
    }
}
// One element (slot j < n_elem): its length l, dilatation e = l / l^ and sigma = e Q t - (0, 0, 1).
__device__ __forceinline__ void slot_sigma(const RodParams& P, const double (&x)[3], const double (&xn)[3],
                                           const double (&Q)[9], double& l, double& e, double (&sg)[3]) {
    const double d0 = xn[0] - x[0], d1 = xn[1] - x[1], d2 = xn[2] - x[2];
    l = sqrt(d0 * d0 + d1 * d1 + d2 * d2) + P.eps_length;
    e = l / P.rest_len;
    const double t0 = d0 / l, t1 = d1 / l, t2 = d2 / l;
    sg[0] = e * (Q[0] * t0 + Q[1] * t1 + Q[2] * t2);
    sg[1] = e * (Q[3] * t0 + Q[4] * t1 + Q[5] * t2);
    sg[2] = e * (Q[6] * t0 + Q[7] * t1 + Q[8] * t2) - 1.0;
}
// One Voronoi vertex (slot j < n_elem - 1): kappa = -log(Q_{k+1} Q_k^T) / D^  (_inv_rotate, as rod_strains), NOT
// reduced by the rest curvature.
__device__ __forceinline__ void slot_kappa(const RodParams& P, const double (&Q)[9], const double (&Qn)[9],
                                           double (&kp)[3]) {
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int l = 0; l < 3; ++l)
            R[3 * i + l] = Qn[3 * i] * Q[3 * l] + Qn[3 * i + 1] * Q[3 * l + 1] + Qn[3 * i + 2] * Q[3 * l + 2];
    const double tr = R[0] + R[4] + R[8];
    const double theta = acos(fmin(fmax(0.5 * tr - 0.5 - P.acos_shift, -1.0), 1.0));
    const double f = -0.5 * theta / sin(theta + P.eps_sin) / P.rest_vor;
    kp[0] = (R[7] - R[5]) * f;
    kp[1] = (R[2] - R[6]) * f;
    kp[2] = (R[3] - R[1]) * f;
}
// The diagonal of slot j's shear matrix S and of its Voronoi vertex's bend matrix B: the tapered rod's table or M.
template <int EPL, class Mat>
__device__ __forceinline__ void slot_shear(const Mat& M, const double* __restrict__ mat, int j, double (&S)[3]) {
    S[0] = mat ? mat[(size_t)kMatShear01 * kLanes * EPL + j] : M.shear[0];
    S[1] = mat ? S[0] : M.shear[1];
    S[2] = mat ? mat[(size_t)kMatShear2 * kLanes * EPL + j] : M.shear[2];
}
template <int EPL, class Mat>
__device__ __forceinline__ void slot_bend(const Mat& M, const double* __restrict__ mat, int j, double (&Bd)[3]) {
    Bd[0] = mat ? mat[(size_t)kMatBend01 * kLanes * EPL + j] : M.bend[0];
    Bd[1] = mat ? Bd[0] : M.bend[1];
    Bd[2] = mat ? mat[(size_t)kMatBend2 * kLanes * EPL + j] : M.bend[2];
}

template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_rod_strains_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                           const int arm_stride, double* __restrict__ out) {
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    const int lane = threadIdx.x;
    const int n = P.n_elem;
    const bool rk = (P.features & SOFTROD_FEAT_REST_KAPPA_ACTION) != 0;
    LaneN<EPL> L;
    BcTargets B;
    const bool bc = readout_load<EPL>(P, S, R, lane, L, B);     // slots past the rod are never read
    const EnvMaterial M = env_material_rt(P, S, R.env);
    double x[EPL][3], Q[EPL][9], xn[EPL][3], Qn[EPL][9];
    rod_strain_config_n<EPL>(P, B, bc, lane, L, S.time[R.env], x, Q, xn, Qn);

    double l[EPL], e[EPL], sg[EPL][3], kp[EPL][3], fn[EPL][3], cm[EPL][3];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        l[s] = e[s] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) sg[s][c] = kp[s][c] = fn[s][c] = cm[s][c] = 0.0;
        if (j < n) {
            double Sd[3];
            slot_shear<EPL>(M, S.mat, j, Sd);
            slot_sigma(P, x[s], xn[s], Q[s], l[s], e[s], sg[s]);
#pragma unroll
            for (int c = 0; c < 3; ++c) fn[s][c] = Sd[c] * sg[s][c];
        }
        if (j < n - 1) {
            double Bd[3];
            slot_bend<EPL>(M, S.mat, j, Bd);
            slot_kappa(P, Q[s], Qn[s], kp[s]);
#pragma unroll
            for (int c = 0; c < 3; ++c) cm[s][c] = Bd[c] * (kp[s][c] - (rk ? L.rk[s][c] : 0.0));
        }
    }
    double ln[EPL];
    shift_next<EPL>(l, ln);                             // l_{k+1}: every lane takes part

    double* o = out + (size_t)R.rod * kStrainRows * (size_t)n;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        if (j < n) {                                    // the n columns of every row, the last Voronoi column as 0
            const double vd = (j < n - 1) ? 0.5 * (l[s] + ln[s]) / P.rest_vor : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[(size_t)c * n + j] = sg[s][c];
                o[(size_t)(3 + c) * n + j] = kp[s][c];
                o[(size_t)(8 + c) * n + j] = fn[s][c];
                o[(size_t)(11 + c) * n + j] = cm[s][c];
            }
            o[(size_t)6 * n + j] = e[s];
            o[(size_t)7 * n + j] = vd;
        }
    }
}

}  // namespace softrod
