// softrod_reaction.hpp — softrod_ground_reaction: what RodPlaneContactWithAnisotropicFriction adds to
// external_forces / external_torques of every rod of every env, evaluated ONCE on the resident state.
//
// A cold kernel beside the step kernels, with softrod_rod_energies_kernel's addressing (readout_rod,
// softrod_readout.hpp: one wave per rod; for OctoFlat the rod's slots are row env * nw + wave at slot
// offset arm * seg) — node k, element k and Voronoi vertex k on lane k.
//
// THE INSTANT: one fresh force evaluation at x, v, Q, omega, rest_kappa as they stand in memory — no
// half kinematic step, no constrain_values.  The evaluation is softrod_literal.hpp's, CALLED here as
// softrod_rod_dynamics_kernel calls it: the masked load (rod_literal_load), the internal forces and
// torques (rod_literal_internal), FixedJoint2Rigid on node 0 / element 0 (rod_literal_joint, OctoFlat)
// and the contact law (rod_literal_contact: plane_contact_n<1, false, false>, for handles of either
// math mode).  This file keeps the ORDER, the substep's own: the joint first, its torque added to the
// total the contact sees; then gravity and the tip force, before the contact unless
// contact_before_forcing says otherwise.  Compiled without floating-point contraction, as everything
// it calls is.
//
// out: [n_envs][rods][6][n_elem + 1] — rows 0-2 the lab-frame force the contact added to each node,
// rows 3-5 the material-frame torque it added to each element (column n_elem: 0).
#pragma once

namespace softrod {

__global__ void __launch_bounds__(kLanes)
softrod_ground_reaction_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                               const int arm_stride, double* __restrict__ out) {
#pragma clang fp contract(off)
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    const int lane = threadIdx.x;
    const int n = P.n_elem;
    LaneN<1> L;
    LibmMat M;
    double mass;
    rod_literal_load(P, S, R.N, R.W, R.base, R.env, lane, L, M, mass);
    RodLiteral X;
    rod_literal_internal(P, lane, L, M, mass, X);

    // ---- external loads before the contact: the joint (OctoFlat), whose torque goes straight into the total, then
    // the forcing group unless the contact precedes it ----
    double fe[3] = {0.0, 0.0, 0.0}, tq[3] = {X.t[0], X.t[1], X.t[2]};
    if (P.features & SOFTROD_FEAT_OCTO_HEAD) {
        double jf[3], jt[3];
        rod_literal_joint(P, S, R.N, R.env, R.arm, lane, X, jf, jt);
#pragma unroll
        for (int c = 0; c < 3; ++c) { fe[c] -= jf[c]; tq[c] += jt[c]; }
    }
    if (!P.contact_before_forcing) {
        if (P.features & SOFTROD_FEAT_GRAVITY) {
#pragma unroll
            for (int c = 0; c < 3; ++c) fe[c] += P.gravity[c] * X.mass;
        }
        if (P.features & SOFTROD_FEAT_TIP_FORCE) {
            const bool tip = (lane == n);
#pragma unroll
            for (int c = 0; c < 3; ++c) fe[c] += tip ? P.tip_force[c] : 0.0;
        }
    }

    // ---- the contact law on f_int + f_ext, t_int + t_ext ----
    const double F[3] = {X.f[0] + fe[0], X.f[1] + fe[1], X.f[2] + fe[2]};
    double fc[3], dt[3];
    rod_literal_contact(P, S, R.env, lane, X, F, tq, fc, dt);

    if (X.node_valid) {
        double* o = out + (size_t)R.rod * 6 * (size_t)(n + 1) + (size_t)lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[(size_t)c * (n + 1)] = fc[c];
            o[(size_t)(3 + c) * (n + 1)] = X.elem_valid ? dt[c] : 0.0;
        }
    }
}

}  // namespace softrod
