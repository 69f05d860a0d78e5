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
// THE ARITHMETIC is muscle_loads_n's (softrod_muscle.hpp) in its literal form — FASTM = false: sqrt and IEEE
// division — for handles of either math mode, and its inputs are formed as libm_dynamic_step forms them
// (softrod_kernels.hpp).  The statements are WRITTEN AGAIN here, not shared: muscle_loads_n is inlined into the
// muscle step kernels, and factoring helpers out of such a function changed those kernels' register allocation
// (DESIGN.md §2).  Change one and change the other; tests/test_gpu_muscle_loads.py holds this kernel to the NumPy
// twin diagnostics.muscle_loads_host, tests/test_muscle_loads.py that twin to the oracle's transcription.  Unlike
// the step kernels this one does NOT skip a layer whose amplitude is zero in the whole wave: the length rows are
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

    // ---- the inputs of muscle_loads_n, as libm_dynamic_step forms them: l, e, Q t, kappa, 1 / eps^3 ----
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

    // ---- muscle_loads_n's statements (FASTM = false), every layer evaluated ----
    double kav[EPL][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], o[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = kv[s][c];
        shift_prev<EPL>(a, o);
#pragma unroll
        for (int s = 0; s < EPL; ++s) kav[s][c] = 0.5 * (kv[s][c] + o[s]);
    }
    double fi[EPL][3], ce[EPL][3], rad[EPL], sh[EPL][3];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        const double ilv = elem_valid[s] ? 1.0 / len[s] : 1.0;
        const double scale = P.muscle_cur_radius ? ilv : P.inv_rest_len;      // r0 sqrt(l_rest / l) = r0s sqrt(1 / l)
        const double r0s = (S.mat && elem_valid[s]) ? S.mat[(size_t)kMatR0s * TW + j] : P.r0_sqrt_rest_len;
        rad[s] = r0s * sqrt(scale);
#pragma unroll
        for (int c = 0; c < 3; ++c) { fi[s][c] = 0.0; ce[s][c] = 0.0; sh[s][c] = e[s] * qt[s][c]; }
    }
    double* o = out + (size_t)R.rod * kMuscleRows * (size_t)(n + 1);
    const size_t nc = (size_t)(n + 1);
#pragma unroll
    for (int m = 0; m < SOFTROD_MAX_MUSCLES; ++m) {
        const bool layer = m < P.n_muscles;
        const bool radial = P.muscle_kind[m] == SOFTROD_MUSCLE_TRANSVERSE && P.muscle_tm_law == 0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            const int j = lane * EPL + s;
            const bool on = layer && elem_valid[s];
            const double* tab = S.mtab + (size_t)m * 4 * TW + j;
            const double act = on ? S.mact[((size_t)m * R.N) * R.W + R.base + (size_t)j] : 0.0;
            const double amp = on ? act * tab[3 * TW] : 0.0;
            const double mr0 = on ? tab[0] : 0.0, mr1 = on ? tab[TW] : 0.0, mr2 = on ? tab[2 * TW] : 0.0;
            const double p0 = rad[s] * mr0, p1 = rad[s] * mr1, p2 = rad[s] * mr2;
            const double n0 = sh[s][0] + (kav[s][1] * p2 - kav[s][2] * p1);
            const double n1 = sh[s][1] + (kav[s][2] * p0 - kav[s][0] * p2);
            const double n2 = sh[s][2] + (kav[s][0] * p1 - kav[s][1] * p0);
            double ss = fma(n2, n2, fma(n1, n1, n0 * n0));
            ss = elem_valid[s] ? ss : 1.0;
            const double nrm = sqrt(ss), rn = 1.0 / nrm;
            double ml = nrm;
            if (radial) ml = 1.0 / sqrt(nrm);
            double w;                                                    // fl(l): compile-time indices only
            if (P.fl_degree == 3) {
                w = fma(fma(fma(P.fl_coef[3], ml, P.fl_coef[2]), ml, P.fl_coef[1]), ml, P.fl_coef[0]);
            } else {
                w = 0.0;
#pragma unroll
                for (int p = SOFTROD_MAX_FL_COEF - 1; p >= 0; --p) w = (p <= P.fl_degree) ? fma(w, ml, P.fl_coef[p]) : w;
            }
            w = (w < 0.0) ? 0.0 : w;
            const double Fm = amp * w * rn;
            const double g0 = Fm * n0, g1 = Fm * n1, g2 = Fm * n2;       // F_m t_m
            fi[s][0] += g0; fi[s][1] += g1; fi[s][2] += g2;
            ce[s][0] += p1 * g2 - p2 * g1;
            ce[s][1] += p2 * g0 - p0 * g2;
            ce[s][2] += p0 * g1 - p1 * g0;
            if (j <= n) {
                o[(size_t)m * nc + j] = on ? amp * w : 0.0;
                o[(size_t)(4 + m) * nc + j] = on ? ml : 0.0;
            }
        }
    }
    const bool pyel = P.muscle_form == 1;
    // F_ext = D^h(Q^T f [/ e])
    double cs[EPL][3], fx[EPL][3];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double sc = pyel ? 1.0 / e[s] : 1.0;
        const double a0 = fma(Q[s][6], fi[s][2], fma(Q[s][3], fi[s][1], Q[s][0] * fi[s][0])) * sc;
        const double a1 = fma(Q[s][7], fi[s][2], fma(Q[s][4], fi[s][1], Q[s][1] * fi[s][0])) * sc;
        const double a2 = fma(Q[s][8], fi[s][2], fma(Q[s][5], fi[s][1], Q[s][2] * fi[s][0])) * sc;
        cs[s][0] = elem_valid[s] ? a0 : 0.0;
        cs[s][1] = elem_valid[s] ? a1 : 0.0;
        cs[s][2] = elem_valid[s] ? a2 : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], p[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = cs[s][c];
        shift_prev<EPL>(a, p);
#pragma unroll
        for (int s = 0; s < EPL; ++s) fx[s][c] = cs[s][c] - p[s];
    }
    // tau_ext = D^h(c_v) + A^h(kappa x c_v D^) + (e Q t) x f l^
    double cn[EPL][3], cv[EPL][3], up[EPL][3], um[EPL][3], tq[EPL][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], p[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = elem_valid[s] ? ce[s][c] : 0.0;
        shift_next<EPL>(a, p);
#pragma unroll
        for (int s = 0; s < EPL; ++s) cn[s][c] = p[s];
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double ef = pyel ? e3v[s] : 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) cv[s][c] = vor_valid[s] ? 0.5 * (ce[s][c] + cn[s][c]) : 0.0;
        const double hd = 0.5 * P.rest_vor * ef;
        const double h3[3] = {(kv[s][1] * cv[s][2] - kv[s][2] * cv[s][1]) * hd,
                              (kv[s][2] * cv[s][0] - kv[s][0] * cv[s][2]) * hd,
                              (kv[s][0] * cv[s][1] - kv[s][1] * cv[s][0]) * hd};
#pragma unroll
        for (int c = 0; c < 3; ++c) { up[s][c] = cv[s][c] * ef + h3[c]; um[s][c] = cv[s][c] * ef - h3[c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], p[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = um[s][c];
        shift_prev<EPL>(a, p);
#pragma unroll
        for (int s = 0; s < EPL; ++s) tq[s][c] = up[s][c] - p[s];
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double g = (pyel ? 1.0 : e[s]) * P.rest_len;
        const double q0 = g * qt[s][0], q1 = g * qt[s][1], q2 = g * qt[s][2];
        tq[s][0] += q1 * fi[s][2] - q2 * fi[s][1];
        tq[s][1] += q2 * fi[s][0] - q0 * fi[s][2];
        tq[s][2] += q0 * fi[s][1] - q1 * fi[s][0];
    }

#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        if (j <= n) {                                   // the n + 1 columns of every row, +0.0 past the row's range
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[(size_t)(8 + c) * nc + j] = elem_valid[s] ? fi[s][c] : 0.0;
                o[(size_t)(11 + c) * nc + j] = cv[s][c];
                o[(size_t)(14 + c) * nc + j] = fx[s][c];
                o[(size_t)(17 + c) * nc + j] = elem_valid[s] ? tq[s][c] : 0.0;
            }
        }
    }
}

}  // namespace softrod
