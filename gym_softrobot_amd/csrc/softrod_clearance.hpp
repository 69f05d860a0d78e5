// softrod_clearance.hpp — softrod_rod_clearance_kernel: how near the rods of an env are to each other, to themselves
// and to the env's target (softrod_rod_clearance).
//
// A cold kernel beside the read-outs: it reads the resident positions, the rest radii (the table softrod_render draws
// with) and the env's target, and writes `out` only.  The definition — the capsules, the closest-point rule and its
// order of operations, the tie rule, what a non-finite rod does — is the contract in include/softrod.h
// (softrod_rod_clearance); this file says how the kernel keeps it.
//
// ONE WAVE (a workgroup of kLanes) per record pair: for every env the rods (rods + 1) / 2 unordered pairs a <= b, in
// the order (0,0) (0,1) .. (0,rods-1) (1,1) .., then one wave per (a, target).  blockIdx.x = env * waves_per_env + w.
//   * Rod a, the ROW rod, lives in registers: element i = lane * EPL + s on slot s of its lane (the read-outs' split:
//     EPL = 2 above 63 elements), as node i and the edge to node i + 1 with |edge|^2 and the element's radius.  The
//     addressing is readout_rod's: slot arm * arm_stride + node of the env's row, `lane_stride` wide.
//   * Rod b's nodes and radii are staged ONCE in LDS (4 x 128 doubles) and read as broadcasts in the j loop, node j + 1
//     of one turn carried as node j of the next.
//   * Every coordinate is taken relative to node 0 of rod a BEFORE any product (a crawling octopus may be metres from
//     the origin, and the products cancel).
//   * A lane keeps its best (gap, i, j) under a strict `<` — j ascends, so the lowest j of equal gaps stays — and, with
//     two slots, the lower i of equal gaps; one lexicographic butterfly over the wave (__shfl_xor on the 64-bit
//     values) then leaves the same winner on every lane whatever the scheduling.  No atomics.
//   * Lane 0 writes record [a][b] and its mirror [b][a] (i <-> j, s <-> t), or [a][rods] for the target.
// NON-FINITE: every node the wave reads is tested with fabs(x) <= DBL_MAX, FALSE for a NaN and for +-inf; one failed
// test on either rod (or on the target, for its column) turns the wave's records into NaN, NaN, -1, -1, NaN, NaN.
// Candidates are compared with `<` only, so a NaN never wins; there is no float-to-int conversion of state.
// Slots past a rod are never read, and no LDS slot past n_elem is read either.
//
// Compiled without floating-point contraction: a product followed by a sum rounds twice, as NumPy does in
// tests/rod_clearance_ref.py, and division and sqrt are IEEE.
#pragma once

#include <float.h>
#include <limits.h>

namespace softrod {

constexpr int kClearanceFields = 6;              // gap, distance, i, j, s, t
constexpr int kClearanceSlots = 2 * kLanes;      // LDS slots per staged row: nodes 0 .. n_elem <= 126

struct ClearanceBest {
    double gap, dist, s, t;
    int i, j;
};

__device__ __forceinline__ bool clearance_finite(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN and +-inf
__device__ __forceinline__ double clearance_clamp(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
__device__ __forceinline__ double clearance_dot(const double (&u)[3], const double (&v)[3]) {
#pragma clang fp contract(off)
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
}
// (gap, i, j) in lexicographic order; false whenever x.gap is a NaN
__device__ __forceinline__ bool clearance_less(const ClearanceBest& x, const ClearanceBest& y) {
    return x.gap < y.gap || (x.gap == y.gap && (x.i < y.i || (x.i == y.i && x.j < y.j)));
}

// The clamped closest points of the segments P1 + s d1 and P2 + t d2 (include/softrod.h, "The segment-segment rule"):
// a = |d1|^2, e = |d2|^2.  -> the distance between them.
__device__ __forceinline__ double clearance_segments(const double (&P1)[3], const double (&d1)[3], double a,
                                                     const double (&P2)[3], const double (&d2)[3], double e,
                                                     double& s, double& t) {
#pragma clang fp contract(off)
    const double r[3] = {P1[0] - P2[0], P1[1] - P2[1], P1[2] - P2[2]};
    const double f = clearance_dot(d2, r), c = clearance_dot(d1, r);
    if (!(a > 0.0) && !(e > 0.0)) {
        s = t = 0.0;
    } else if (!(a > 0.0)) {
        s = 0.0;
        t = clearance_clamp(f / e);
    } else if (!(e > 0.0)) {
        t = 0.0;
        s = clearance_clamp(-c / a);
    } else {
        const double b = clearance_dot(d1, d2);
        const double denom = a * e - b * b;
        s = denom > 0.0 ? clearance_clamp((b * f - c * e) / denom) : 0.0;
        t = (b * s + f) / e;
        if (t < 0.0) {
            t = 0.0;
            s = clearance_clamp(-c / a);
        } else if (t > 1.0) {
            t = 1.0;
            s = clearance_clamp((b - c) / a);
        }
    }
    const double w[3] = {(P1[0] + d1[0] * s) - (P2[0] + d2[0] * t), (P1[1] + d1[1] * s) - (P2[1] + d2[1] * t),
                         (P1[2] + d1[2] * s) - (P2[2] + d2[2] * t)};
    return sqrt(clearance_dot(w, w));
}

// out: [n_envs][rods][rods + 1][6]
template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_rod_clearance_kernel(const double* __restrict__ pos, const double* __restrict__ radius, const EnvTarget T,
                             const int n_envs, const int n_elem, const int rods, const int lane_stride,
                             const int arm_stride, const int self_gap, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double rod_b[4][kClearanceSlots];          // x, y, z relative to node 0 of rod a; the radii
    const int lane = threadIdx.x;
    const int pairs = rods * (rods + 1) / 2, per_env = pairs + rods;
    const int env = blockIdx.x / per_env, w = blockIdx.x - env * per_env;
    const bool to_target = w >= pairs;
    int a = 0, b = rods;
    if (to_target) {
        a = w - pairs;
    } else {
        int rem = w;
        while (rem >= rods - a) { rem -= rods - a; ++a; }
        b = a + rem;
    }
    const bool self = a == b;
    const size_t N = (size_t)n_envs, W = (size_t)lane_stride, comp = N * W;
    const size_t base_a = (size_t)env * W + (size_t)a * (size_t)arm_stride;

    // rod a: node 0, then this lane's elements relative to it
    double O[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) { O[c] = pos[(size_t)c * comp + base_a]; ok = ok && clearance_finite(O[c]); }
    double P1[EPL][3], d1[EPL][3], aa[EPL], ri[EPL];
    bool valid[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int i = lane * EPL + s;
        valid[s] = i < n_elem;
        aa[s] = ri[s] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) P1[s][c] = d1[s][c] = 0.0;
        if (valid[s]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double x0 = pos[(size_t)c * comp + base_a + (size_t)i], x1 = pos[(size_t)c * comp + base_a + (size_t)i + 1];
                ok = ok && clearance_finite(x0) && clearance_finite(x1);
                P1[s][c] = x0 - O[c];
                d1[s][c] = (x1 - O[c]) - P1[s][c];
            }
            aa[s] = clearance_dot(d1[s], d1[s]);
            ri[s] = radius[i];
        }
    }

    ClearanceBest best;
    best.gap = best.dist = INFINITY;
    best.s = best.t = 0.0;
    best.i = best.j = INT_MAX;
    bool have_target = true;

    if (to_target) {
        have_target = T.kind != 0;                                             // (wave-uniform)
        if (have_target) {
            double X[3];
            env_target_point(T, N, env, X);
#pragma unroll
            for (int c = 0; c < 3; ++c) { ok = ok && clearance_finite(X[c]); X[c] -= O[c]; }
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
                if (valid[s]) {
                    const double u[3] = {X[0] - P1[s][0], X[1] - P1[s][1], X[2] - P1[s][2]};
                    const double p = aa[s] > 0.0 ? clearance_clamp(clearance_dot(u, d1[s]) / aa[s]) : 0.0;
                    const double g[3] = {X[0] - (P1[s][0] + d1[s][0] * p), X[1] - (P1[s][1] + d1[s][1] * p),
                                         X[2] - (P1[s][2] + d1[s][2] * p)};
                    const double dist = sqrt(clearance_dot(g, g));
                    ClearanceBest cand;
                    cand.gap = dist - ri[s]; cand.dist = dist; cand.s = p; cand.t = 0.0; cand.i = lane * EPL + s; cand.j = -1;
                    if (clearance_less(cand, best)) best = cand;
                }
            }
        }
    } else {
        // rod b into LDS, relative to node 0 of rod a
        const size_t base_b = (size_t)env * W + (size_t)b * (size_t)arm_stride;
        for (int k = lane; k <= n_elem; k += kLanes) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double x = pos[(size_t)c * comp + base_b + (size_t)k];
                ok = ok && clearance_finite(x);
                rod_b[c][k] = x - O[c];
            }
            if (k < n_elem) rod_b[3][k] = radius[k];
        }
        __syncthreads();
        const int j0 = self ? self_gap : 0;
        double B0[3] = {0.0, 0.0, 0.0};
        if (j0 < n_elem) { B0[0] = rod_b[0][j0]; B0[1] = rod_b[1][j0]; B0[2] = rod_b[2][j0]; }
        for (int j = j0; j < n_elem; ++j) {
            const double B1[3] = {rod_b[0][j + 1], rod_b[1][j + 1], rod_b[2][j + 1]};
            const double d2[3] = {B1[0] - B0[0], B1[1] - B0[1], B1[2] - B0[2]};
            const double e = clearance_dot(d2, d2);
            const double rj = rod_b[3][j];
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
                const int i = lane * EPL + s;
                if (valid[s] && (!self || j - i >= self_gap)) {
                    ClearanceBest cand;
                    cand.dist = clearance_segments(P1[s], d1[s], aa[s], B0, d2, e, cand.s, cand.t);
                    cand.gap = cand.dist - ri[s] - rj;
                    cand.i = i; cand.j = j;
                    if (clearance_less(cand, best)) best = cand;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) B0[c] = B1[c];
        }
    }

    // the wave's winner, on every lane
    ok = __all(ok);
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
        ClearanceBest o;
        o.gap = __shfl_xor(best.gap, m); o.dist = __shfl_xor(best.dist, m);
        o.s = __shfl_xor(best.s, m); o.t = __shfl_xor(best.t, m);
        o.i = __shfl_xor(best.i, m); o.j = __shfl_xor(best.j, m);
        if (clearance_less(o, best)) best = o;
    }

    if (lane == 0) {
        const bool found = best.i != INT_MAX;
        double rec[kClearanceFields] = {INFINITY, INFINITY, -1.0, -1.0, 0.0, 0.0};
        if (found) {
            rec[0] = best.gap; rec[1] = best.dist; rec[2] = (double)best.i; rec[3] = (double)best.j;
            rec[4] = best.s; rec[5] = best.t;
        }
        if (!ok && have_target) {
            const double nan = __builtin_nan("");
            rec[0] = rec[1] = rec[4] = rec[5] = nan;
            rec[2] = rec[3] = -1.0;
        }
        const size_t row = (size_t)(rods + 1) * kClearanceFields;
        double* o = out + ((size_t)env * (size_t)rods + (size_t)a) * row + (size_t)b * kClearanceFields;
#pragma unroll
        for (int q = 0; q < kClearanceFields; ++q) o[q] = rec[q];
        if (!to_target && !self) {
            double* m = out + ((size_t)env * (size_t)rods + (size_t)b) * row + (size_t)a * kClearanceFields;
            m[0] = rec[0]; m[1] = rec[1]; m[2] = rec[3]; m[3] = rec[2]; m[4] = rec[5]; m[5] = rec[4];
        }
    }
}

}  // namespace softrod
