// softrod_dynamics_readout.hpp — softrod_rod_dynamics: the two sides of the rods' equation of motion, what PyElastica
// keeps on every rod as internal_forces / internal_torques, external_forces / external_torques and, after
// update_accelerations, acceleration_collection / alpha_collection — for every rod of every env, evaluated ONCE on
// the resident state.  The other read-outs return one contribution each; this one returns the sum.
//
// A cold kernel beside the step kernels, with softrod_ground_reaction_kernel's addressing (readout_rod,
// softrod_readout.hpp: one wave per rod, its slots at offset arm * arm_stride of the env's row) — node k, element k
// and Voronoi vertex k on lane k.  Every branch around a call that shifts across lanes is wave-uniform (a feature bit
// or a config switch), so all 64 lanes take part in every shift.
//
// THE INSTANT is softrod_ground_reaction's: one fresh force evaluation at x, v, Q, omega, rest_kappa as they stand in
// memory — no half kinematic step, no constrain_values.  It is NOT the value the last substep applied.  Constraints,
// the analytical damper, the Laplace filter and the suckers act on values and rates, not on loads: they do not
// enter (update_accelerations, before constrain_rates).
//
// THE ORDER is the substep's own: internal forces and torques (CosseratRod._compute_internal_forces / _torques),
// then FixedJoint2Rigid on node 0 / element 0 (SOFTROD_FEAT_OCTO_HEAD), then the forcing group — gravity, the point
// force (which ASSIGNS component x of node 0), the tip force, the COOMM layers' equivalent loads — and the plane
// contact, in the order contact_before_forcing says.
//
// CALLED, not copied: the whole evaluation is softrod_literal.hpp's, the one literal text beside the step kernels'
// own — rod_literal_internal, rod_literal_joint (joint_load_literal), rod_literal_contact (plane_contact_n<1, false,
// false> of softrod_contact.hpp: the literal fp64 law, for handles of either math mode) and muscle_law_literal<1> —
// as softrod_ground_reaction_kernel and softrod_muscle_loads_kernel call it.  This file keeps the order in which the
// loads are gathered, the forcing terms that are its own, and the rows it stores.
// WRITTEN AGAIN here, the one second text among the read-outs: the masked load, rod_literal_load's statements.  They
// hold no arithmetic, but plane_contact_n is compiled at the compiler's default contraction and which of its products
// are fused follows the code around it: with the load taken through the function this kernel's contact share came
// out differently rounded on every sliding-contact case (measured; with every other part shared it does not move).
// Change one and change the other.
//
// THE ACTION-BORNE INPUTS are read from the resident state.  The point force is (double)prev_action[7 env], what
// the step prologue applies, and 0.0 for an env whose time is 0: a fresh simulator has no point force until the
// first set_action, while _prev_action survives reset.  The muscle activations are the rows StatePtrs.mact as they
// stand, read per element, and the law is evaluated on the strains of THIS state (softrod_muscle_loads rebuilds
// the configuration of the last force evaluation instead; the two instants coincide for an env whose time is 0).
//
// Compiled without floating-point contraction, as everything it calls is, so that a product followed by a sum
// rounds twice, as NumPy does in oracle/softrod_oracle_np.py; the fma calls of the muscle law are muscle_loads_n's own.
//
// out: [n_envs][rods][18][n_elem + 1] —
//   rows 0-2    internal force on the nodes, lab frame                      n_elem + 1 columns
//   rows 3-5    internal torque on the elements, material frame             n_elem
//   rows 6-8    external force on the nodes, lab frame                      n_elem + 1
//   rows 9-11   external torque on the elements, material frame             n_elem
//   rows 12-14  acceleration (internal + external force) / mass             n_elem + 1
//   rows 15-17  angular acceleration J^-1 (internal + external torque) e    n_elem
// Column n_elem of the per-element rows is written as +0.0.
#pragma once

namespace softrod {

constexpr int kDynamicsRows = 18;

// The contact law on f_int + f_ext, t_int + t_ext as they stand when it runs, added to the external loads.
__device__ __forceinline__ void rod_dynamics_contact(const RodParams& P, const StatePtrs& S, int env, int lane,
                                                     const RodLiteral& X, double (&fe)[3], double (&te)[3]) {
#pragma clang fp contract(off)
    const double F[3] = {X.f[0] + fe[0], X.f[1] + fe[1], X.f[2] + fe[2]};
    const double T[3] = {X.t[0] + te[0], X.t[1] + te[1], X.t[2] + te[2]};
    double fc[3], dt[3];
    rod_literal_contact(P, S, env, lane, X, F, T, fc, dt);
#pragma unroll
    for (int c = 0; c < 3; ++c) { fe[c] += fc[c]; te[c] += X.elem_valid ? dt[c] : 0.0; }
}

__global__ void __launch_bounds__(kLanes)
softrod_rod_dynamics_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                            const int arm_stride, double* __restrict__ out) {
#pragma clang fp contract(off)
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    const int lane = threadIdx.x;
    const int n = P.n_elem;
    const bool node_valid = lane <= n, has_elem = lane < n, vor_valid = lane < n - 1;
    const size_t N = R.N, W = R.W;
    const int env = R.env;
    const bool rk = (P.features & SOFTROD_FEAT_REST_KAPPA_ACTION) != 0;
    LaneN<1> L;
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.x[0][c] = L.v[0][c] = L.w[0][c] = L.rk[0][c] = L.kap[0][c] = L.t[0][c] = 0.0; }
#pragma unroll
    for (int c = 0; c < 9; ++c) L.Q[0][c] = 0.0;
    if (node_valid) {                                  // slots past the rod are never read: n + 1 nodes, n elements,
        const size_t i = R.base + (size_t)lane;        // n - 1 Voronoi vertices; the rest stay zero
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            L.x[0][c] = S.pos[c * N * W + i];
            L.v[0][c] = S.vel[c * N * W + i];
            if (has_elem) L.w[0][c] = S.omg[c * N * W + i];
            if (rk && vor_valid) L.rk[0][c] = S.rkap[c * N * W + i];
        }
        if (has_elem) {
#pragma unroll
            for (int c = 0; c < 9; ++c) L.Q[0][c] = S.dir[c * N * W + i];
        }
    }
    LibmMat M;
    const EnvMaterial EM = env_material_rt(P, S, env);
    libm_material(P, EM, S.mat, lane, M);
    double mass = (lane == 0 || lane == n) ? 0.5 * EM.mass_node : EM.mass_node;
    if (S.mat) mass = S.mat[kMatMass * kLanes + lane];
    mass = node_valid ? mass : 0.0;

    RodLiteral X;
    rod_literal_internal(P, lane, L, M, mass, X);
    const bool elem_valid = X.elem_valid;

    // ---- external loads, first the joint: FixedJoint2Rigid on node 0 / element 0 ----
    double fe[3] = {0.0, 0.0, 0.0}, te[3] = {0.0, 0.0, 0.0};
    if (P.features & SOFTROD_FEAT_OCTO_HEAD) {
        double jf[3], jt[3];
        rod_literal_joint(P, S, R.N, R.env, R.arm, lane, X, jf, jt);
#pragma unroll
        for (int c = 0; c < 3; ++c) { fe[c] -= jf[c]; te[c] += jt[c]; }
    }

    const bool has_contact = (P.features & SOFTROD_FEAT_PLANE_CONTACT_ANISO) != 0;
    if (has_contact && P.contact_before_forcing) rod_dynamics_contact(P, S, R.env, lane, X, fe, te);

    // ---- the forcing group, in registration order ----
    if (P.features & SOFTROD_FEAT_GRAVITY) {
#pragma unroll
        for (int c = 0; c < 3; ++c) fe[c] += P.gravity[c] * X.mass;
    }
    if (P.features & SOFTROD_FEAT_POINT_FORCE_NODE0_X) {
        const double pf = (S.time[R.env] == 0.0) ? 0.0 : (double)S.prev_action[7 * (size_t)R.env];
        fe[0] = (lane == 0) ? pf : fe[0];
    }
    if (P.features & SOFTROD_FEAT_TIP_FORCE) {
        const bool tip = (lane == n);
#pragma unroll
        for (int c = 0; c < 3; ++c) fe[c] += tip ? P.tip_force[c] : 0.0;
    }
    if (P.features & SOFTROD_FEAT_COOMM_MUSCLES) {
        // the law on the strains of THIS state: rod_literal_internal's e, l, Q t, kappa and 1 / eps^3
        const bool ev[1] = {elem_valid}, vv[1] = {X.vor_valid};
        const double r0s[1] = {X.M.r0s};
        MuscleLiteral<1> U;
        muscle_law_literal<1>(P, S, R.N, R.W, R.base, lane, X.L.Q, X.e, X.len, X.qt, X.kap, X.e3, ev, vv, r0s, U);
#pragma unroll
        for (int c = 0; c < 3; ++c) { fe[c] += U.fx[0][c]; te[c] += elem_valid ? U.tq[0][c] : 0.0; }
    }
    if (has_contact && !P.contact_before_forcing) rod_dynamics_contact(P, S, R.env, lane, X, fe, te);

    if (X.node_valid) {
        const size_t nc = (size_t)(n + 1);
        double* o = out + (size_t)R.rod * kDynamicsRows * nc + (size_t)lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[(size_t)c * nc] = X.f[c];
            o[(size_t)(3 + c) * nc] = X.t[c];
            o[(size_t)(6 + c) * nc] = fe[c];
            o[(size_t)(9 + c) * nc] = elem_valid ? te[c] : 0.0;
            o[(size_t)(12 + c) * nc] = (X.f[c] + fe[c]) / X.mass;
            o[(size_t)(15 + c) * nc] = elem_valid ? (X.M.invJ[c] * (X.t[c] + te[c])) * X.e[0] : 0.0;
        }
    }
}

}  // namespace softrod
