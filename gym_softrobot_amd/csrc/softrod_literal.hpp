// softrod_literal.hpp — the literal fp64 force evaluation that the cold read-out kernels share.
//
// Every law of the substep has at most TWO texts in this directory: the step kernels' tuned text (libm_dynamic_step,
// muscle_loads_n, joints(): inlined into step kernels, where factoring helpers out changed the register allocation,
// DESIGN.md §2 — left untouched) and ONE literal text, here, which every read-out that needs the law calls
// (softrod_readout.hpp lists who calls what).  No step kernel inlines any of these functions.  Node k, element k and
// Voronoi vertex k sit on lane k (slot lane * EPL + s in the muscle law); neighbours come through the DPP shifts with
// their end rules (lane 63 / lane 0 read 0), every shift outside any per-lane select so that all 64 lanes take part;
// no LDS, no atomics, no array indexed at run time.
//
// EVERY function here is compiled WITHOUT floating-point contraction, so that a product followed by a sum rounds
// twice, as NumPy does in oracle/softrod_oracle_np.py and in the twins of gym_softrobot_amd/diagnostics.py; the
// explicit fma calls of the muscle law are muscle_loads_n's own and stay.  That includes the muscle law as
// softrod_muscle_loads_kernel calls it, whose own text of the law was compiled at the compiler's default contraction:
// merging it here moved that read-out by rounding, towards its contract-off twin diagnostics.muscle_loads_host.
// The one callee that is NOT contract-off is plane_contact_n: see rod_literal_contact.
#pragma once

namespace softrod {

// FixedJoint2Rigid.apply_forces / apply_torques (joint.py:47-219) of arm `arm` on its node 0 and element 0,
// literally (softrod_octo.hpp's joints() is the fused fast-math form).  x0, v0: node 0; x1: node 1.
struct JointLoad {
    double f[3], t[3];     // the force taken from node 0; the lab-frame torque given to element 0
    double gap[3], dist;   // end_distance_vector: node 0 minus its connection point; end_distance
};
__device__ __forceinline__ JointLoad joint_load_literal(const RodParams& P, const HeadState& H, int arm,
                                                        const double (&x0)[3], const double (&v0)[3],
                                                        const double (&x1)[3]) {
#pragma clang fp contract(off)
    JointLoad J;
    const double th = (P.joint_angle0 + P.joint_angle_step * (double)arm) / 180.0 * M_PI;
    const double ct = cos(th), st = sin(th);
    const double b0 = H.Q[3], b1 = H.Q[4], b2 = H.Q[5];          // the head's binormal
    const double dir[3] = {-(ct * b0 - st * b1), -(st * b0 + ct * b1), -b2};
    double pos[3] = {H.x[0], H.x[1], 0.0};
    double (&dv)[3] = J.gap;
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pos[i] = pos[i] + dir[i] * P.head_radius;
        dv[i] = x0[i] - pos[i];
        d2 += dv[i] * dv[i];
    }
    const double dist = sqrt(d2);
    J.dist = dist;
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
        J.f[i] = P.joint_k * dv[i] + -P.joint_nu * (rel * nv[i]);
        link[i] = x1[i] - x0[i];
        force[i] = -P.joint_kt * (x1[i] - (pos[i] + P.rest_len * dir[i]));
    }
    J.t[0] = link[1] * force[2] - link[2] * force[1];
    J.t[1] = link[2] * force[0] - link[0] * force[2];
    J.t[2] = link[0] * force[1] - link[1] * force[0];
    return J;
}

// One rod on one wave, LaneN<1>: the state as loaded and what one fresh force evaluation at it leaves.
struct RodLiteral {
    bool node_valid, elem_valid, vor_valid;
    LaneN<1> L;
    LibmMat M;
    double mass;                                // this lane's node, 0 past the rod
    // (one slot per lane, shaped as plane_contact_n<1> and muscle_law_literal<1> take them)
    double xn[1][3], vn[1][3], len[1];          // node k + 1; the element's length (rest_len on a lane without one)
    double e[1], qt[1][3];                      // dilatation; Q t
    double kap[1][3], e3[1];                    // kappa, 0 past the last Voronoi vertex; 1 / eps^3, not masked
    double f[3], t[3];                          // internal force on the node, lab frame; internal torque on the
};                                              // element, material frame: both 0 past their range

// x, v of the n + 1 nodes, omega, Q of the n elements, rest_kappa (SOFTROD_FEAT_REST_KAPPA_ACTION) of the n - 1
// Voronoi vertices of the rod whose slot 0 is `base` in one component of the rows (N envs, rows W wide): slots past
// the rod are never read and stay zero, as kappa and the tangents do.  Then the material of this lane and its mass
// (0 past the rod).  softrod_rod_dynamics_kernel holds these statements a second time (it says why).
__device__ __forceinline__ void rod_literal_load(const RodParams& P, const StatePtrs& S, size_t N, size_t W,
                                                 size_t base, int env, int lane, LaneN<1>& L, LibmMat& M, double& mass) {
#pragma clang fp contract(off)
    const int n = P.n_elem;
    const bool node_valid = lane <= n, elem_valid = lane < n, vor_valid = lane < n - 1;
    const bool rk = (P.features & SOFTROD_FEAT_REST_KAPPA_ACTION) != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.x[0][c] = L.v[0][c] = L.w[0][c] = L.rk[0][c] = L.kap[0][c] = L.t[0][c] = 0.0; }
#pragma unroll
    for (int c = 0; c < 9; ++c) L.Q[0][c] = 0.0;
    if (node_valid) {
        const size_t i = base + (size_t)lane;
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
    const EnvMaterial EM = env_material_rt(P, S, env);
    libm_material(P, EM, S.mat, lane, M);
    mass = (lane == 0 || lane == n) ? 0.5 * EM.mass_node : EM.mass_node;
    if (S.mat) mass = S.mat[kMatMass * kLanes + lane];
    mass = node_valid ? mass : 0.0;
}

// CosseratRod._compute_internal_forces / _torques on the loaded state, written as the LIBM step writes them
// (libm_dynamic_step, softrod_kernels.hpp: the step kernels' text of the same law) on the state, material and
// mass as loaded.  Fills X: the validity flags, its copy of the state with the tangents, and the results.
__device__ __forceinline__ void rod_literal_internal(const RodParams& P, int lane, const LaneN<1>& L0, const LibmMat& M0,
                                                     double mass, RodLiteral& X) {
#pragma clang fp contract(off)
    const int n = P.n_elem;
    X.node_valid = lane <= n; X.elem_valid = lane < n; X.vor_valid = lane < n - 1;
    X.L = L0; X.M = M0; X.mass = mass;
    LaneN<1>& L = X.L;
    const LibmMat& M = X.M;
    const bool elem_valid = X.elem_valid, vor_valid = X.vor_valid;

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
    X.f[0] = cs0 - from_prev(cs0);
    X.f[1] = cs1 - from_prev(cs1);
    X.f[2] = cs2 - from_prev(cs2);

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
    const double k0 = vor_valid ? vec0 * fk : 0.0, k1 = vor_valid ? vec1 * fk : 0.0, k2 = vor_valid ? vec2 * fk : 0.0;
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
    double ti0 = (c20 - from_prev(c20)) + 0.5 * (c30 + from_prev(c30));
    double ti1 = (c21 - from_prev(c21)) + 0.5 * (c31 + from_prev(c31));
    double ti2 = (c22 - from_prev(c22)) + 0.5 * (c32 + from_prev(c32));
    ti0 += (qt1 * n2 - qt2 * n1) * P.rest_len;
    ti1 += (qt2 * n0 - qt0 * n2) * P.rest_len;
    ti2 += (qt0 * n1 - qt1 * n0) * P.rest_len;

    // ---- transport (J w / e) x w and unsteady dilatation (J w / e) (de/dt) / e ----
    const double vn0 = from_next(L.v[0][0]), vn1 = from_next(L.v[0][1]), vn2 = from_next(L.v[0][2]);
    const double rv = (L.x[0][0] * L.v[0][0] + L.x[0][1] * L.v[0][1]) + L.x[0][2] * L.v[0][2];
    const double rvn = (xn0 * vn0 + xn1 * vn1) + xn2 * vn2;
    const double rp1v = (xn0 * L.v[0][0] + xn1 * L.v[0][1]) + xn2 * L.v[0][2];
    const double rvp1 = (L.x[0][0] * vn0 + L.x[0][1] * vn1) + L.x[0][2] * vn2;
    const double dil_rate = (rv + rvn - rvp1 - rp1v) / len / P.rest_len;
    const double jw0 = M.J[0] * L.w[0][0] / e, jw1 = M.J[1] * L.w[0][1] / e, jw2 = M.J[2] * L.w[0][2] / e;
    ti0 += jw1 * L.w[0][2] - jw2 * L.w[0][1];
    ti1 += jw2 * L.w[0][0] - jw0 * L.w[0][2];
    ti2 += jw0 * L.w[0][1] - jw1 * L.w[0][0];
    ti0 += jw0 * dil_rate / e; ti1 += jw1 * dil_rate / e; ti2 += jw2 * dil_rate / e;
    X.t[0] = elem_valid ? ti0 : 0.0; X.t[1] = elem_valid ? ti1 : 0.0; X.t[2] = elem_valid ? ti2 : 0.0;

    X.xn[0][0] = xn0; X.xn[0][1] = xn1; X.xn[0][2] = xn2;
    X.vn[0][0] = vn0; X.vn[0][1] = vn1; X.vn[0][2] = vn2;
    X.len[0] = len;
    X.e[0] = e;
    X.qt[0][0] = qt0; X.qt[0][1] = qt1; X.qt[0][2] = qt2;
    X.kap[0][0] = k0; X.kap[0][1] = k1; X.kap[0][2] = k2;
    X.e3[0] = e3;
}

// FixedJoint2Rigid of arm `arm` (SOFTROD_FEAT_OCTO_HEAD) from the body's stored state: jf the force it takes from the
// node, jt the torque it gives the element in the material frame — lane 0's, +0.0 on every other lane.  The caller
// subtracts jf from its external force and adds jt to the torque it keeps.
__device__ __forceinline__ void rod_literal_joint(const RodParams& P, const StatePtrs& S, size_t N, int env, int arm,
                                                  int lane, const RodLiteral& X, double (&jf)[3], double (&jt)[3]) {
#pragma clang fp contract(off)
    HeadState H;
    double tgt[2];
    load_head(S, N, env, H, tgt);
    const LaneN<1>& L = X.L;
    const double x0[3] = {L.x[0][0], L.x[0][1], L.x[0][2]}, v0[3] = {L.v[0][0], L.v[0][1], L.v[0][2]};
    const double x1[3] = {X.xn[0][0], X.xn[0][1], X.xn[0][2]};
    const JointLoad J = joint_load_literal(P, H, arm, x0, v0, x1);
    const bool first = lane == 0;                      // lane 0 holds node 0, node 1 next to it
    const double* Q = L.Q[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        jf[c] = first ? J.f[c] : 0.0;
        jt[c] = first ? (Q[3 * c] * J.t[0] + Q[3 * c + 1] * J.t[1]) + Q[3 * c + 2] * J.t[2] : 0.0;
    }
}

// The contact law on F = f_int + f_ext and T = t_int + t_ext AS THEY STAND when it runs: plane_contact_n<1, false,
// false> of softrod_contact.hpp, the literal fp64 instantiation the LIBM step calls (any plane normal, IEEE divisions
// and sqrt), for handles of either math mode, with the env's contact row and this rod's material.  fc: the force it
// adds to the node.  The law adds its torque to the total in place, so its share dt is taken as the total's movement;
// the caller masks dt by elem_valid where it consumes it.
// plane_contact_n itself is the step kernels' text, compiled at the compiler's DEFAULT contraction: which of its
// products become fused multiply-adds follows the kernel it is inlined into.  tools/readout_ab.py holds a change of
// these kernels to the bytes of the build before it.
__device__ __forceinline__ void rod_literal_contact(const RodParams& P, const StatePtrs& S, int env, int lane,
                                                    const RodLiteral& X, const double (&F)[3], const double (&T)[3],
                                                    double (&fc)[3], double (&dt)[3]) {
#pragma clang fp contract(off)
    const int n = P.n_elem;
    RodParams Pc = P;
    Pc.seg = 0;                                        // this wave holds ONE rod from lane 0: a slot's index is its lane
    ContactParams CP = contact_params_row(Pc, env_contact_rt(P, S, env));
    CP.r0_sqrt_rest_len = X.M.r0s;
    CP.inv_r0_sqrt_rest_len = 1.0 / X.M.r0s;
    ConstN<1> CK;
    CK.mass[0] = X.mass;
    CK.mass_next[0] = (lane + 1 <= n) ? X.M.mass_next : 0.0;
    CK.inv_mass_pair[0] = 1.0 / (X.mass + X.M.mass_next);
    const double F1[1][3] = {{X.node_valid ? F[0] : 0.0, X.node_valid ? F[1] : 0.0, X.node_valid ? F[2] : 0.0}};
    double tq[1][3] = {{T[0], T[1], T[2]}}, fc1[1][3];
    plane_contact_n<1, false, false>(CP, Pc, lane, CK, X.L, X.xn, X.vn, X.len, F1, tq, fc1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        fc[c] = fc1[0][c];
        dt[c] = tq[0][c] - T[c];
    }
}

// The COOMM muscle law in its literal form (muscle_loads_n of softrod_muscle.hpp is the step kernels' text; FASTM =
// false here), every layer evaluated whatever its activation: slot j = lane * EPL + s of the rod whose slot 0 is
// `base` in the activation rows StatePtrs.mact (N envs, rows W wide), read per element as they stand.
// The caller owns the instant and forms the inputs as libm_dynamic_step forms them: Q, e, l, Q t, kappa (0 past the
// last Voronoi vertex), 1 / eps^3, the validity flags and r0 sqrt(l_rest) per slot.
template <int EPL>
struct MuscleLiteral {           // every index is a compile-time one
    double F[EPL][SOFTROD_MAX_MUSCLES], l[EPL][SOFTROD_MAX_MUSCLES];   // layer force F_m and length l_m, 0 where the layer or the slot is off
    double f[EPL][3], cv[EPL][3];    // muscle internal force (not masked); couple c_v on the Voronoi vertices, masked
    double fx[EPL][3], tq[EPL][3];   // equivalent external force on the node; couple on the element (not masked)
};
template <int EPL>
__device__ __forceinline__ void muscle_law_literal(const RodParams& P, const StatePtrs& S, size_t N, size_t W,
                                                   size_t base, int lane, const double (&Q)[EPL][9],
                                                   const double (&e)[EPL], const double (&len)[EPL],
                                                   const double (&qt)[EPL][3], const double (&kv)[EPL][3],
                                                   const double (&e3v)[EPL], const bool (&elem_valid)[EPL],
                                                   const bool (&vor_valid)[EPL], const double (&r0s)[EPL],
                                                   MuscleLiteral<EPL>& O) {
#pragma clang fp contract(off)
    constexpr size_t TW = (size_t)kLanes * EPL;         // a row of the layer tables
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
    double ce[EPL][3], rad[EPL], sh[EPL][3];
    double (&fi)[EPL][3] = O.f;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double ilv = elem_valid[s] ? 1.0 / len[s] : 1.0;
        const double scale = P.muscle_cur_radius ? ilv : P.inv_rest_len;      // r0 sqrt(l_rest / l) = r0s sqrt(1 / l)
        rad[s] = r0s[s] * sqrt(scale);
#pragma unroll
        for (int c = 0; c < 3; ++c) { fi[s][c] = 0.0; ce[s][c] = 0.0; sh[s][c] = e[s] * qt[s][c]; }
    }
#pragma unroll
    for (int m = 0; m < SOFTROD_MAX_MUSCLES; ++m) {
        const bool layer = m < P.n_muscles;
        const bool radial = P.muscle_kind[m] == SOFTROD_MUSCLE_TRANSVERSE && P.muscle_tm_law == 0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            const int j = lane * EPL + s;
            const bool on = layer && elem_valid[s];
            const double* tab = S.mtab + (size_t)m * 4 * TW + j;
            const double act = on ? S.mact[((size_t)m * N) * W + base + (size_t)j] : 0.0;
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
            O.F[s][m] = on ? amp * w : 0.0;
            O.l[s][m] = on ? ml : 0.0;
        }
    }
    const bool pyel = P.muscle_form == 1;
    // F_ext = D^h(Q^T f [/ e])
    double cs[EPL][3];
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
        for (int s = 0; s < EPL; ++s) O.fx[s][c] = cs[s][c] - p[s];
    }
    // tau_ext = D^h(c_v) + A^h(kappa x c_v D^) + (e Q t) x f l^
    double cn[EPL][3], up[EPL][3], um[EPL][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], p[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = elem_valid[s] ? ce[s][c] : 0.0;
        shift_next<EPL>(a, p);      // every lane takes part: inside the select's arm below the shift would run with
#pragma unroll
        for (int s = 0; s < EPL; ++s) cn[s][c] = p[s];      // the last element's lane switched off
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double ef = pyel ? e3v[s] : 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) O.cv[s][c] = vor_valid[s] ? 0.5 * (ce[s][c] + cn[s][c]) : 0.0;
        const double (&cv)[3] = O.cv[s];
        const double hd = 0.5 * P.rest_vor * ef;
        const double h3[3] = {(kv[s][1] * cv[2] - kv[s][2] * cv[1]) * hd,
                              (kv[s][2] * cv[0] - kv[s][0] * cv[2]) * hd,
                              (kv[s][0] * cv[1] - kv[s][1] * cv[0]) * hd};
#pragma unroll
        for (int c = 0; c < 3; ++c) { up[s][c] = cv[c] * ef + h3[c]; um[s][c] = cv[c] * ef - h3[c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a[EPL], p[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) a[s] = um[s][c];
        shift_prev<EPL>(a, p);
#pragma unroll
        for (int s = 0; s < EPL; ++s) O.tq[s][c] = up[s][c] - p[s];
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const double g = (pyel ? 1.0 : e[s]) * P.rest_len;
        const double q0 = g * qt[s][0], q1 = g * qt[s][1], q2 = g * qt[s][2];
        O.tq[s][0] += q1 * fi[s][2] - q2 * fi[s][1];
        O.tq[s][1] += q2 * fi[s][0] - q0 * fi[s][2];
        O.tq[s][2] += q0 * fi[s][1] - q1 * fi[s][0];
    }
}

}  // namespace softrod
