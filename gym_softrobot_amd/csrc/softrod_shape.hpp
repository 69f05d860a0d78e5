// softrod_shape.hpp — softrod_rod_shape_kernel: rebuild resident rods from strain fields (softrod_set_rod_shape).
//
// A cold kernel that WRITES a rod's configuration between a reset and the first step, where the read-outs only read
// it: the inverse of softrod_rod_strains_kernel (softrod_strains.hpp).  Upstream has no counterpart: its builds call
// CosseratRod.straight_rod only (soft_pendulum/build.py:54-61 and the other build files).
//
// One wave per rod with the read-outs' grid and addressing (readout_rod, softrod_readout.hpp) — slot j = lane * EPL + s
// holds node j, element j and Voronoi vertex j — so the packed arms of OctoFlat and the muscle octopus need nothing
// special.  The rod keeps its base pose (node 0's position, element 0's directors: the boundary-condition targets, the
// head joints and the pendulum / moving-base constraints stay consistent) and everything else follows from
//     Q_{k+1} = exp([-kappa_k D^]x) Q_k            kappa in the material frame, NOT reduced by rest curvature: the
//                                                  inverse of slot_kappa, kappa = -log(Q_{k+1} Q_k^T) / D^
//     x_{k+1} = x_k + l^ Q_k^T (sigma_k + e3)
// Per slot the exact rotation (Rodrigues with libm sin / cos, a series below |kappa D^|^2 = 1e-6); the product along
// the rod is an inclusive wave scan of 3x3 matrices — a local compose of the lane's EPL slots, six doubling steps
// across the 64 lanes (__shfl_up: ds_bpermute, the plainest movement of a double by a variable distance), a local
// apply — seeded with the base directors in slot 0 and the identity in slots past the rod; the nodes are the same
// scan of 3-vector sums, added to the base node.  The order is fixed: a repeated call is bitwise repeatable.
//
// What reset derives from the shape is derived again, by reset's own calls: the tangent rows (unit_tangents), the kappa
// rows (slot_kappa: what a force evaluation at this state caches), OctoArmSingle's prev_com_state in ctrl[0..1]
// (no_action_const + com_xy_n).  Velocity and omega are written as given.
// A wave writes only its own rod's node slots 1..n_elem (position), 0..n_elem (velocity), element slots 1..n_elem - 1
// (directors), 0..n_elem - 1 (omega, tangents) and Voronoi slots 0..n_elem - 2 (kappa): slot 0 of position and
// directors, the ghost slots between packed arms and every other array stay as they are.  A NULL field is zero.
// No LDS, no atomics, no array indexed at run time.  Values are not validated: a NaN spoils its own rod only.
//
// The same kernel shapes the starts of softrod_set_reset_shapes (softrod_reset_shapes.hpp): there the fields are a pool
// with a leading entry axis and RodShapeArgs::pool_index names each env's entry.  Only the row a rod reads differs, so a
// pool start and softrod_set_rod_shape with that entry's fields run the same statements and give the same bits.
#pragma once

namespace softrod {

struct RodShapeArgs {
    const double* kappa;      // [n_envs][rods][3][n_elem - 1], or nullptr
    const double* sigma;      // [n_envs][rods][3][n_elem], or nullptr
    const double* velocity;   // [n_envs][rods][3][n_elem + 1] lab frame, or nullptr
    const double* omega;      // [n_envs][rods][3][n_elem] material frame, or nullptr
    const uint8_t* mask;      // [n_envs], or nullptr: every env
    const int* pool_index;    // [n_envs], or nullptr.  Set (softrod_set_reset_shapes): the four fields are a pool
                              // [count][rods][3][..] and env e reads entry pool_index[e] of it instead of row e
};

// C = A B (row-major 3x3; rows of a director matrix are d1, d2, d3)
__device__ __forceinline__ void shape_mul(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int l = 0; l < 3; ++l)
            C[3 * i + l] = A[3 * i] * B[l] + A[3 * i + 1] * B[3 + l] + A[3 * i + 2] * B[6 + l];
}
// exp([v]x) = I + a [v]x + b [v]x^2, a = sin(th) / th, b = (1 - cos(th)) / th^2, th = |v|
__device__ __forceinline__ void shape_rotation(const double (&v)[3], double (&R)[9]) {
    const double t = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    double a, b;
    if (t < 1.0e-6) {           // the series: the next terms are t^3 / 5040 and t^3 / 40320
        a = 1.0 - t * (1.0 / 6.0) + t * t * (1.0 / 120.0);
        b = 0.5 - t * (1.0 / 24.0) + t * t * (1.0 / 720.0);
    } else {
        const double th = sqrt(t);
        a = sin(th) / th;
        b = (1.0 - cos(th)) / t;
    }
    const double d = 1.0 - b * t;
    R[0] = d + b * v[0] * v[0];
    R[4] = d + b * v[1] * v[1];
    R[8] = d + b * v[2] * v[2];
    R[1] = b * v[0] * v[1] - a * v[2];
    R[3] = b * v[0] * v[1] + a * v[2];
    R[2] = b * v[0] * v[2] + a * v[1];
    R[6] = b * v[0] * v[2] - a * v[1];
    R[5] = b * v[1] * v[2] - a * v[0];
    R[7] = b * v[1] * v[2] + a * v[0];
}

template <int EPL>
__global__ void __launch_bounds__(kLanes)
softrod_rod_shape_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                         const int arm_stride, const RodShapeArgs A) {
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    if (A.mask && !A.mask[R.env]) return;            // wave-uniform
    const int lane = threadIdx.x;
    const int n = P.n_elem;
    const size_t NW = R.N * R.W;
    // the row of the fields this rod reads: its own, or its arm's row of the env's pool entry
    const size_t rod = A.pool_index ? (size_t)A.pool_index[R.env] * (size_t)rods + (size_t)R.arm : (size_t)R.rod;
    if (lane == 0 && S.planar_cert) S.planar_cert[R.env] = 0;      // the shape need not lie in the plane

    // ---- the per-slot factors: the base directors in slot 0, exp([-kappa D^]x) of vertex j - 1 in slot j, identity past the rod
    double M[EPL][9];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
#pragma unroll
        for (int c = 0; c < 9; ++c) M[s][c] = (c == 0 || c == 4 || c == 8) ? 1.0 : 0.0;
        if (j == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) M[s][c] = S.dir[c * NW + R.base];
        } else if (j < n) {
            double v[3] = {0.0, 0.0, 0.0};
            if (A.kappa) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = -A.kappa[(rod * 3 + c) * (size_t)(n - 1) + (size_t)(j - 1)] * P.rest_vor;
            }
            shape_rotation(v, M[s]);
        }
    }
    // ---- inclusive scan of the products: local compose, six doubling steps, local apply
    double Q[EPL][9];
    {
        double T[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) T[c] = M[0][c];
#pragma unroll
        for (int s = 1; s < EPL; ++s) {
            double U[9];
            shape_mul(M[s], T, U);
#pragma unroll
            for (int c = 0; c < 9; ++c) T[c] = U[c];
        }
#pragma unroll
        for (int d = 1; d < kLanes; d <<= 1) {
            double O[9], U[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) O[c] = __shfl_up(T[c], d);
            shape_mul(T, O, U);
#pragma unroll
            for (int c = 0; c < 9; ++c) T[c] = (lane >= d) ? U[c] : T[c];
        }
        double E[9];                                  // the product of every earlier lane
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const double up = __shfl_up(T[c], 1);
            E[c] = (lane >= 1) ? up : ((c == 0 || c == 4 || c == 8) ? 1.0 : 0.0);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) Q[0][c] = M[0][c];            // the base directors themselves
        } else {
            shape_mul(M[0], E, Q[0]);
        }
#pragma unroll
        for (int s = 1; s < EPL; ++s) shape_mul(M[s], Q[s - 1], Q[s]);
    }
    // ---- the edges l^ Q_k^T (sigma_k + e3) of elements j < n (zero past the rod), and their inclusive scan
    double x[EPL][3];
    {
        double e[EPL][3];
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            const int j = lane * EPL + s;
            double sg[3] = {0.0, 0.0, 0.0};
            if (A.sigma && j < n) {
#pragma unroll
                for (int c = 0; c < 3; ++c) sg[c] = A.sigma[(rod * 3 + c) * (size_t)n + (size_t)j];
            }
            sg[2] += 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                e[s][c] = (j < n) ? P.rest_len * (Q[s][c] * sg[0] + Q[s][3 + c] * sg[1] + Q[s][6 + c] * sg[2]) : 0.0;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double t = e[0][c];
#pragma unroll
            for (int s = 1; s < EPL; ++s) t += e[s][c];
#pragma unroll
            for (int d = 1; d < kLanes; d <<= 1) {
                const double o = __shfl_up(t, d);
                t = (lane >= d) ? t + o : t;
            }
            const double up = __shfl_up(t, 1);
            double run = (lane >= 1) ? up : 0.0;      // the sum of every earlier lane's edges
            const double x0 = S.pos[c * NW + R.base];
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
                x[s][c] = x0 + run;
                run += e[s][c];
            }
        }
    }
    // ---- what reset derives from the shape: tangents, kappa (slot_kappa)
    double tg[EPL][3], kp[EPL][3];
    unit_tangents<EPL>(P, x, tg);
    {
        double Qn[EPL][9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            double a[EPL], o[EPL];
#pragma unroll
            for (int s = 0; s < EPL; ++s) a[s] = Q[s][c];
            shift_next<EPL>(a, o);
#pragma unroll
            for (int s = 0; s < EPL; ++s) Qn[s][c] = o[s];
        }
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) kp[s][c] = 0.0;
            if (lane * EPL + s < n - 1) slot_kappa(P, Q[s], Qn[s], kp[s]);
        }
    }
    // ---- store: only this rod's slots, never slot 0 of position and directors
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int j = lane * EPL + s;
        const size_t i = R.base + (size_t)j;
        if (j <= n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (j >= 1) S.pos[c * NW + i] = x[s][c];
                S.vel[c * NW + i] = A.velocity ? A.velocity[(rod * 3 + c) * (size_t)(n + 1) + (size_t)j] : 0.0;
            }
        }
        if (j < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                S.omg[c * NW + i] = A.omega ? A.omega[(rod * 3 + c) * (size_t)n + (size_t)j] : 0.0;
                S.tan[c * NW + i] = tg[s][c];
            }
            if (j >= 1) {
#pragma unroll
                for (int c = 0; c < 9; ++c) S.dir[c * NW + i] = Q[s][c];
            }
        }
        if (j < n - 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) S.kap[c * NW + i] = kp[s][c];
            // OctoArmSingle's prev_kappa_state = deepcopy(rod.kappa[0]) (arm_single_env.py:173)
            if (P.env_kind == SOFTROD_ENV_ARM_SINGLE) S.envmem[i] = kp[s][0];
        }
    }
    // ---- OctoArmSingle's prev_com_state (arm_single_env.py:174), as reset_rod recomputes it
    if (P.env_kind == SOFTROD_ENV_ARM_SINGLE) {
        LaneN<EPL> L;
#pragma unroll
        for (int s = 0; s < EPL; ++s)
#pragma unroll
            for (int c = 0; c < 3; ++c) L.x[s][c] = x[s][c];
        ConstN<EPL> C;
        no_action_const<EPL>(P, S, R.env, lane, C);
        double com[2];
        com_xy_n<EPL>(P, C, lane, L, com);
        if (lane == 0) {
            S.ctrl[(size_t)0 * R.N + R.env] = com[0];
            S.ctrl[(size_t)1 * R.N + R.env] = com[1];
        }
    }
}

}  // namespace softrod
