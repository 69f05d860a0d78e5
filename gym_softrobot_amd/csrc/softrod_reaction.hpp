// softrod_reaction.hpp — softrod_ground_reaction: what RodPlaneContactWithAnisotropicFriction adds to
// external_forces / external_torques of every rod of every env, evaluated ONCE on the resident state.
//
// A cold kernel beside the step kernels, with softrod_rod_energies_kernel's addressing (readout_rod,
// softrod_readout.hpp: one wave per rod; for OctoFlat the rod's slots are row env * nw + wave at slot
// offset arm * seg) — node k, element k and Voronoi vertex k on lane k.  The load is its own: masked
// per element and Voronoi vertex.
// Neighbours come through the DPP shifts from_next / from_prev with their end rules (lane 63 / lane 0
// read 0); no LDS, no atomics, no array indexed at run time.
//
// THE INSTANT: one fresh force evaluation at x, v, Q, omega, rest_kappa as they stand in memory — no
// half kinematic step, no constrain_values.  Internal forces and torques from that state
// (CosseratRod._compute_internal_forces / _torques, written as the LIBM step writes them), then the
// external loads in the substep's own order: FixedJoint2Rigid on node 0 / element 0 first (OctoFlat),
// then the forcing group and the contact in the order contact_before_forcing says.  The contact law is
// plane_contact_n<1, false, false> of softrod_contact.hpp: the literal fp64 instantiation the LIBM step
// calls (any plane normal, IEEE divisions and sqrt), for handles of either math mode.  Everything else
// in this file is compiled without floating-point contraction, so that a product followed by a sum
// rounds twice, as NumPy does in oracle/softrod_oracle_np.py.
//
// out: [n_envs][rods][6][n_elem + 1] — rows 0-2 the lab-frame force the contact added to each node,
// rows 3-5 the material-frame torque it added to each element (column n_elem: 0).
#pragma once

namespace softrod {

// FixedJoint2Rigid.apply_forces / apply_torques (joint.py:47-219) of arm `arm` on its node 0 and element 0,
// literally (softrod_octo.hpp's joints() is the fused fast-math form): fj the force taken from node 0, tj the
// lab-frame torque given to element 0.  x0, v0: node 0; x1: node 1.
__device__ __forceinline__ void joint_load_literal(const RodParams& P, const HeadState& H, int arm,
                                                   const double (&x0)[3], const double (&v0)[3],
                                                   const double (&x1)[3], double (&fj)[3], double (&tj)[3]) {
#pragma clang fp contract(off)
    const double th = (P.joint_angle0 + P.joint_angle_step * (double)arm) / 180.0 * M_PI;
    const double ct = cos(th), st = sin(th);
    const double b0 = H.Q[3], b1 = H.Q[4], b2 = H.Q[5];          // the head's binormal
    const double dir[3] = {-(ct * b0 - st * b1), -(st * b0 + ct * b1), -b2};
    double pos[3] = {H.x[0], H.x[1], 0.0};
    double dv[3], d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pos[i] = pos[i] + dir[i] * P.head_radius;
        dv[i] = x0[i] - pos[i];
        d2 += dv[i] * dv[i];
    }
    const double dist = sqrt(d2);
    const bool apart = !(dist <= 2.220446049250313e-16 * 1e4);
    double rel = 0.0, nv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        nv[i] = apart ? dv[i] / dist : 0.0;
        rel += (v0[i] - H.v[i]) * nv[i];
    }
    double link[3], force[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        fj[i] = P.joint_k * dv[i] + -P.joint_nu * (rel * nv[i]);
        link[i] = x1[i] - x0[i];
        force[i] = -P.joint_kt * (x1[i] - (pos[i] + P.rest_len * dir[i]));
    }
    tj[0] = link[1] * force[2] - link[2] * force[1];
    tj[1] = link[2] * force[0] - link[0] * force[2];
    tj[2] = link[0] * force[1] - link[1] * force[0];
}

__global__ void __launch_bounds__(kLanes)
softrod_ground_reaction_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                               const int arm_stride, double* __restrict__ out) {
#pragma clang fp contract(off)
    const ReadoutRod R = readout_rod(P, rods, lane_stride, arm_stride);
    const int rod = R.rod, env = R.env, arm = R.arm;
    const int lane = threadIdx.x;
    const int n = P.n_elem;
    const size_t N = (size_t)P.n_envs, W = (size_t)lane_stride;
    const bool node_valid = lane <= n, elem_valid = lane < n, vor_valid = lane < n - 1;
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
            if (elem_valid) L.w[0][c] = S.omg[c * N * W + i];
            if (rk && vor_valid) L.rk[0][c] = S.rkap[c * N * W + i];
        }
        if (elem_valid) {
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

    // ---- geometry: lengths, tangents, dilatation ----
    const double xn0 = from_next(L.x[0][0]), xn1 = from_next(L.x[0][1]), xn2 = from_next(L.x[0][2]);
    const double d0 = xn0 - L.x[0][0], d1 = xn1 - L.x[0][1], d2 = xn2 - L.x[0][2];
    double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2) + P.eps_length;
    len = elem_valid ? len : P.rest_len;               // finite geometry on the lanes that hold no element
    L.t[0][0] = d0 / len; L.t[0][1] = d1 / len; L.t[0][2] = d2 / len;
    const double e = len / P.rest_len;

    // ---- shear/stretch: sigma = e Q t - z ; n = S sigma ; internal force: difference of Q^T n / e ----
    const double qt0 = L.Q[0][0] * L.t[0][0] + L.Q[0][1] * L.t[0][1] + L.Q[0][2] * L.t[0][2];
    const double qt1 = L.Q[0][3] * L.t[0][0] + L.Q[0][4] * L.t[0][1] + L.Q[0][5] * L.t[0][2];
    const double qt2 = L.Q[0][6] * L.t[0][0] + L.Q[0][7] * L.t[0][1] + L.Q[0][8] * L.t[0][2];
    const double n0 = M.shear[0] * (e * qt0);
    const double n1 = M.shear[1] * (e * qt1);
    const double n2 = M.shear[2] * (e * qt2 - 1.0);
    double cs0 = (L.Q[0][0] * n0 + L.Q[0][3] * n1 + L.Q[0][6] * n2) / e;
    double cs1 = (L.Q[0][1] * n0 + L.Q[0][4] * n1 + L.Q[0][7] * n2) / e;
    double cs2 = (L.Q[0][2] * n0 + L.Q[0][5] * n1 + L.Q[0][8] * n2) / e;
    cs0 = elem_valid ? cs0 : 0.0;
    cs1 = elem_valid ? cs1 : 0.0;
    cs2 = elem_valid ? cs2 : 0.0;
    const double f0 = cs0 - from_prev(cs0);
    const double f1 = cs1 - from_prev(cs1);
    const double f2 = cs2 - from_prev(cs2);

    // ---- bend/twist: kappa = -log(Q_{k+1} Q_k^T) / D ; couples ----
    double Qn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Qn[i] = from_next(L.Q[0][i]);
    const double len_n = from_next(len);
#define SR_ROWDOT(i, j) (Qn[3 * (i)] * L.Q[0][3 * (j)] + Qn[3 * (i) + 1] * L.Q[0][3 * (j) + 1] + \
                         Qn[3 * (i) + 2] * L.Q[0][3 * (j) + 2])
    const double vec0 = SR_ROWDOT(2, 1) - SR_ROWDOT(1, 2);
    const double vec1 = SR_ROWDOT(0, 2) - SR_ROWDOT(2, 0);
    const double vec2 = SR_ROWDOT(1, 0) - SR_ROWDOT(0, 1);
    const double trace = vor_valid ? (SR_ROWDOT(0, 0) + SR_ROWDOT(1, 1)) + SR_ROWDOT(2, 2) : 3.0;
#undef SR_ROWDOT
    const double theta = acos(0.5 * trace - 0.5 - P.acos_shift);
    const double fk = (-0.5 * theta / sin(theta + P.eps_sin)) / P.rest_vor;
    const double k0 = vec0 * fk, k1 = vec1 * fk, k2 = vec2 * fk;
    const double m0 = M.bend[0] * (k0 - L.rk[0][0]), m1 = M.bend[1] * (k1 - L.rk[0][1]),
                 m2 = M.bend[2] * (k2 - L.rk[0][2]);
    const double vd = 0.5 * (len_n + len) / P.rest_vor;
    const double e3 = 1.0 / (vd * vd * vd);
    double c20 = m0 * e3, c21 = m1 * e3, c22 = m2 * e3;
    const double dv3 = P.rest_vor * e3;
    double c30 = (k1 * m2 - k2 * m1) * dv3;
    double c31 = (k2 * m0 - k0 * m2) * dv3;
    double c32 = (k0 * m1 - k1 * m0) * dv3;
    c20 = vor_valid ? c20 : 0.0; c21 = vor_valid ? c21 : 0.0; c22 = vor_valid ? c22 : 0.0;
    c30 = vor_valid ? c30 : 0.0; c31 = vor_valid ? c31 : 0.0; c32 = vor_valid ? c32 : 0.0;
    double tq0 = (c20 - from_prev(c20)) + 0.5 * (c30 + from_prev(c30));
    double tq1 = (c21 - from_prev(c21)) + 0.5 * (c31 + from_prev(c31));
    double tq2 = (c22 - from_prev(c22)) + 0.5 * (c32 + from_prev(c32));
    tq0 += (qt1 * n2 - qt2 * n1) * P.rest_len;
    tq1 += (qt2 * n0 - qt0 * n2) * P.rest_len;
    tq2 += (qt0 * n1 - qt1 * n0) * P.rest_len;

    // ---- transport (J w / e) x w and unsteady dilatation (J w / e) (de/dt) / e ----
    const double vn0 = from_next(L.v[0][0]), vn1 = from_next(L.v[0][1]), vn2 = from_next(L.v[0][2]);
    const double rv = (L.x[0][0] * L.v[0][0] + L.x[0][1] * L.v[0][1]) + L.x[0][2] * L.v[0][2];
    const double rvn = (xn0 * vn0 + xn1 * vn1) + xn2 * vn2;
    const double rp1v = (xn0 * L.v[0][0] + xn1 * L.v[0][1]) + xn2 * L.v[0][2];
    const double rvp1 = (L.x[0][0] * vn0 + L.x[0][1] * vn1) + L.x[0][2] * vn2;
    const double dil_rate = (rv + rvn - rvp1 - rp1v) / len / P.rest_len;
    const double jw0 = M.J[0] * L.w[0][0] / e, jw1 = M.J[1] * L.w[0][1] / e, jw2 = M.J[2] * L.w[0][2] / e;
    tq0 += jw1 * L.w[0][2] - jw2 * L.w[0][1];
    tq1 += jw2 * L.w[0][0] - jw0 * L.w[0][2];
    tq2 += jw0 * L.w[0][1] - jw1 * L.w[0][0];
    tq0 += jw0 * dil_rate / e; tq1 += jw1 * dil_rate / e; tq2 += jw2 * dil_rate / e;
    tq0 = elem_valid ? tq0 : 0.0; tq1 = elem_valid ? tq1 : 0.0; tq2 = elem_valid ? tq2 : 0.0;

    // ---- external loads before the contact: the joint (OctoFlat), then the forcing group unless the
    // contact precedes it ----
    double fe0 = 0.0, fe1 = 0.0, fe2 = 0.0;
    if (P.features & SOFTROD_FEAT_OCTO_HEAD) {
        HeadState H;
        double tgt[2];
        load_head(S, N, env, H, tgt);
        const double x0[3] = {L.x[0][0], L.x[0][1], L.x[0][2]}, v0[3] = {L.v[0][0], L.v[0][1], L.v[0][2]};
        const double x1[3] = {xn0, xn1, xn2};
        double fj[3], tj[3];
        joint_load_literal(P, H, arm, x0, v0, x1, fj, tj);
        const bool first = lane == 0;                  // lane 0 holds node 0, node 1 next to it
        fe0 -= first ? fj[0] : 0.0; fe1 -= first ? fj[1] : 0.0; fe2 -= first ? fj[2] : 0.0;
        const double* Q = L.Q[0];
        tq0 += first ? (Q[0] * tj[0] + Q[1] * tj[1]) + Q[2] * tj[2] : 0.0;
        tq1 += first ? (Q[3] * tj[0] + Q[4] * tj[1]) + Q[5] * tj[2] : 0.0;
        tq2 += first ? (Q[6] * tj[0] + Q[7] * tj[1]) + Q[8] * tj[2] : 0.0;
    }
    if (!P.contact_before_forcing) {
        if (P.features & SOFTROD_FEAT_GRAVITY) {
            fe0 += P.gravity[0] * mass; fe1 += P.gravity[1] * mass; fe2 += P.gravity[2] * mass;
        }
        if (P.features & SOFTROD_FEAT_TIP_FORCE) {
            const bool tip = (lane == n);
            fe0 += tip ? P.tip_force[0] : 0.0;
            fe1 += tip ? P.tip_force[1] : 0.0;
            fe2 += tip ? P.tip_force[2] : 0.0;
        }
    }

    // ---- the contact law on f_int + f_ext, t_int + t_ext ----
    RodParams Pc = P;
    Pc.seg = 0;                                        // this wave holds ONE rod from lane 0: a slot's index is its lane
    ContactParams CP = contact_params_row(Pc, env_contact_rt(P, S, env));
    CP.r0_sqrt_rest_len = M.r0s;
    CP.inv_r0_sqrt_rest_len = 1.0 / M.r0s;
    ConstN<1> CK;
    CK.mass[0] = mass;
    CK.mass_next[0] = (lane + 1 <= n) ? M.mass_next : 0.0;
    CK.inv_mass_pair[0] = 1.0 / (mass + M.mass_next);
    const double xn[1][3] = {{xn0, xn1, xn2}}, vn[1][3] = {{vn0, vn1, vn2}};
    const double len1[1] = {len};
    const double F[1][3] = {{node_valid ? f0 + fe0 : 0.0, node_valid ? f1 + fe1 : 0.0, node_valid ? f2 + fe2 : 0.0}};
    double tq[1][3] = {{tq0, tq1, tq2}}, fc[1][3];
    plane_contact_n<1, false, false>(CP, Pc, lane, CK, L, xn, vn, len1, F, tq, fc);

    if (node_valid) {
        double* o = out + (size_t)rod * 6 * (size_t)(n + 1) + (size_t)lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * (n + 1)] = fc[0][c];
        o[(size_t)3 * (n + 1)] = elem_valid ? tq[0][0] - tq0 : 0.0;
        o[(size_t)4 * (n + 1)] = elem_valid ? tq[0][1] - tq1 : 0.0;
        o[(size_t)5 * (n + 1)] = elem_valid ? tq[0][2] - tq2 : 0.0;
    }
}

}  // namespace softrod
