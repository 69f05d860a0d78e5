// softrod_dynamics_readout.hpp — softrod_rod_dynamics: the two sides of the rods' equation of motion, what PyElastica
// keeps on every rod as internal_forces / internal_torques, external_forces / external_torques and, after
// update_accelerations, acceleration_collection / alpha_collection — for every rod of every env, evaluated ONCE on
// the resident state.  The other read-outs return one contribution each; this one returns the sum.
//
// A cold kernel beside the step kernels, with softrod_ground_reaction_kernel's addressing and load (readout_rod,
// softrod_readout.hpp: one wave per rod, its slots at offset arm * arm_stride of the env's row) — node k, element k
// and Voronoi vertex k on lane k, the load masked per node, element and Voronoi vertex so that slots past the rod are
// never read.  Neighbours come through the DPP shifts from_next / from_prev with their end rules (lane 63 / lane 0
// read 0); no LDS, no atomics, no array indexed at run time.  Every branch around a shift is wave-uniform (a feature
// bit or a config switch), so all 64 lanes take part in every shift.
//
// THE INSTANT is softrod_ground_reaction's: one fresh force evaluation at x, v, Q, omega, rest_kappa as they stand in
// memory — no half kinematic step, no constrain_values.  It is NOT the value the last substep applied.  Constraints,
// the analytical damper, the Laplace filter and the suckers act on values and rates, not on loads: they do not
// enter (update_accelerations, before constrain_rates).
//
// THE ORDER is the substep's own: internal forces and torques (CosseratRod._compute_internal_forces / _torques,
// written as the LIBM step writes them), then FixedJoint2Rigid on node 0 / element 0 (SOFTROD_FEAT_OCTO_HEAD), then
// the forcing group — gravity, the point force (which ASSIGNS component x of node 0), the tip force, the COOMM
// layers' equivalent loads — and the plane contact, in the order contact_before_forcing says.
//
// CALLED, not copied: joint_load_literal (softrod_reaction.hpp), plane_contact_n<1, false, false>
// (softrod_contact.hpp: the literal fp64 law, for handles of either math mode), load_head, env_material_rt,
// env_contact_rt, libm_material, contact_params_row.  WRITTEN AGAIN here: the internal force and torque statements
// (softrod_reaction.hpp holds the other copy; libm_dynamic_step, inlined into a step kernel, the original) and the
// muscle law in its literal form, FASTM = false (muscle_loads_n of softrod_muscle.hpp the original,
// softrod_muscle_readout.hpp the other copy) — factoring helpers out of a function that a step kernel inlines changed
// that kernel's register allocation.  Change one and change the others.
//
// THE ACTION-BORNE INPUTS are read from the resident state.  The point force is (double)prev_action[7 env], what
// the step prologue applies, and 0.0 for an env whose time is 0: a fresh simulator has no point force until the
// first set_action, while _prev_action survives reset.  The muscle activations are the rows StatePtrs.mact as they
// stand, read per element, and the law is evaluated on the strains of THIS state (softrod_muscle_loads rebuilds
// the configuration of the last force evaluation instead; the two instants coincide for an env whose time is 0).
//
// Everything in this file is compiled without floating-point contraction, so that a product followed by a sum rounds
// twice, as NumPy does in oracle/softrod_oracle_np.py; the fma calls of the muscle law are muscle_loads_n's own.
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

__global__ void __launch_bounds__(kLanes)
softrod_rod_dynamics_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
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
    ti0 = elem_valid ? ti0 : 0.0; ti1 = elem_valid ? ti1 : 0.0; ti2 = elem_valid ? ti2 : 0.0;

    // ---- external loads, first the joint: FixedJoint2Rigid on node 0 / element 0 ----
    double fe0 = 0.0, fe1 = 0.0, fe2 = 0.0, te0 = 0.0, te1 = 0.0, te2 = 0.0;
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
        te0 += first ? (Q[0] * tj[0] + Q[1] * tj[1]) + Q[2] * tj[2] : 0.0;
        te1 += first ? (Q[3] * tj[0] + Q[4] * tj[1]) + Q[5] * tj[2] : 0.0;
        te2 += first ? (Q[6] * tj[0] + Q[7] * tj[1]) + Q[8] * tj[2] : 0.0;
    }

    // ---- the contact law on f_int + f_ext, t_int + t_ext as they stand when it runs; it adds its torque to the
    // total in place, so its share is taken as the total's movement, as softrod_ground_reaction does ----
    const bool has_contact = (P.features & SOFTROD_FEAT_PLANE_CONTACT_ANISO) != 0;
    auto contact = [&]() {
#pragma clang fp contract(off)
        RodParams Pc = P;
        Pc.seg = 0;                                    // this wave holds ONE rod from lane 0: a slot's index is its lane
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
        const double s0 = ti0 + te0, s1 = ti1 + te1, s2 = ti2 + te2;
        double tq[1][3] = {{s0, s1, s2}}, fc[1][3];
        plane_contact_n<1, false, false>(CP, Pc, lane, CK, L, xn, vn, len1, F, tq, fc);
        fe0 += fc[0][0]; fe1 += fc[0][1]; fe2 += fc[0][2];
        te0 += elem_valid ? tq[0][0] - s0 : 0.0;
        te1 += elem_valid ? tq[0][1] - s1 : 0.0;
        te2 += elem_valid ? tq[0][2] - s2 : 0.0;
    };
    if (has_contact && P.contact_before_forcing) contact();

    // ---- the forcing group, in registration order ----
    if (P.features & SOFTROD_FEAT_GRAVITY) {
        fe0 += P.gravity[0] * mass; fe1 += P.gravity[1] * mass; fe2 += P.gravity[2] * mass;
    }
    if (P.features & SOFTROD_FEAT_POINT_FORCE_NODE0_X) {
        const double pf = (S.time[env] == 0.0) ? 0.0 : (double)S.prev_action[7 * (size_t)env];
        fe0 = (lane == 0) ? pf : fe0;
    }
    if (P.features & SOFTROD_FEAT_TIP_FORCE) {
        const bool tip = (lane == n);
        fe0 += tip ? P.tip_force[0] : 0.0;
        fe1 += tip ? P.tip_force[1] : 0.0;
        fe2 += tip ? P.tip_force[2] : 0.0;
    }
    if (P.features & SOFTROD_FEAT_COOMM_MUSCLES) {
        // muscle_loads_n's statements (FASTM = false) at one slot per lane, every layer evaluated, its inputs formed
        // as libm_dynamic_step forms them: e, 1 / l, Q t, kappa (0 past the last Voronoi vertex), 1 / eps^3
        const double kav0 = 0.5 * (k0 + from_prev(k0)), kav1 = 0.5 * (k1 + from_prev(k1)),
                     kav2 = 0.5 * (k2 + from_prev(k2));
        const double ilv = elem_valid ? 1.0 / len : 1.0;
        const double scale = P.muscle_cur_radius ? ilv : P.inv_rest_len;      // r0 sqrt(l_rest / l) = r0s sqrt(1 / l)
        const double rad = M.r0s * sqrt(scale);
        const double sh0 = e * qt0, sh1 = e * qt1, sh2 = e * qt2;
        double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0, ce0 = 0.0, ce1 = 0.0, ce2 = 0.0;
#pragma unroll
        for (int m = 0; m < SOFTROD_MAX_MUSCLES; ++m) {
            const bool on = m < P.n_muscles && elem_valid;
            const bool radial = P.muscle_kind[m] == SOFTROD_MUSCLE_TRANSVERSE && P.muscle_tm_law == 0;
            const double* tab = S.mtab + (size_t)m * 4 * kLanes + lane;
            const double act = on ? S.mact[((size_t)m * N) * W + R.base + (size_t)lane] : 0.0;
            const double amp = on ? act * tab[3 * kLanes] : 0.0;
            const double mr0 = on ? tab[0] : 0.0, mr1 = on ? tab[kLanes] : 0.0, mr2 = on ? tab[2 * kLanes] : 0.0;
            const double p0 = rad * mr0, p1 = rad * mr1, p2 = rad * mr2;
            const double s0 = sh0 + (kav1 * p2 - kav2 * p1);
            const double s1 = sh1 + (kav2 * p0 - kav0 * p2);
            const double s2 = sh2 + (kav0 * p1 - kav1 * p0);
            double ss = fma(s2, s2, fma(s1, s1, s0 * s0));
            ss = elem_valid ? ss : 1.0;
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
            const double g0 = Fm * s0, g1 = Fm * s1, g2 = Fm * s2;       // F_m t_m
            fi0 += g0; fi1 += g1; fi2 += g2;
            ce0 += p1 * g2 - p2 * g1;
            ce1 += p2 * g0 - p0 * g2;
            ce2 += p0 * g1 - p1 * g0;
        }
        const bool pyel = P.muscle_form == 1;
        // F_ext += D^h(Q^T f [/ e])
        const double* Q = L.Q[0];
        const double sc = pyel ? 1.0 / e : 1.0;
        double a0 = fma(Q[6], fi2, fma(Q[3], fi1, Q[0] * fi0)) * sc;
        double a1 = fma(Q[7], fi2, fma(Q[4], fi1, Q[1] * fi0)) * sc;
        double a2 = fma(Q[8], fi2, fma(Q[5], fi1, Q[2] * fi0)) * sc;
        a0 = elem_valid ? a0 : 0.0; a1 = elem_valid ? a1 : 0.0; a2 = elem_valid ? a2 : 0.0;
        fe0 += a0 - from_prev(a0); fe1 += a1 - from_prev(a1); fe2 += a2 - from_prev(a2);
        // tau_ext += D^h(c_v) + A^h(kappa x c_v D^) + (e Q t) x f l^
        ce0 = elem_valid ? ce0 : 0.0; ce1 = elem_valid ? ce1 : 0.0; ce2 = elem_valid ? ce2 : 0.0;
        const double ef = pyel ? e3 : 1.0;
        const double cn0 = from_next(ce0), cn1 = from_next(ce1), cn2 = from_next(ce2);   // every lane takes part: a
        const double cv0 = vor_valid ? 0.5 * (ce0 + cn0) : 0.0;                          // shift inside the select's arm
        const double cv1 = vor_valid ? 0.5 * (ce1 + cn1) : 0.0;                          // would run with the last
        const double cv2 = vor_valid ? 0.5 * (ce2 + cn2) : 0.0;                          // element's lane switched off
        const double hd = 0.5 * P.rest_vor * ef;
        const double h0 = (k1 * cv2 - k2 * cv1) * hd, h1 = (k2 * cv0 - k0 * cv2) * hd, h2 = (k0 * cv1 - k1 * cv0) * hd;
        const double um0 = cv0 * ef - h0, um1 = cv1 * ef - h1, um2 = cv2 * ef - h2;
        double tm0 = (cv0 * ef + h0) - from_prev(um0);
        double tm1 = (cv1 * ef + h1) - from_prev(um1);
        double tm2 = (cv2 * ef + h2) - from_prev(um2);
        const double g = (pyel ? 1.0 : e) * P.rest_len;
        const double q0 = g * qt0, q1 = g * qt1, q2 = g * qt2;
        tm0 += q1 * fi2 - q2 * fi1;
        tm1 += q2 * fi0 - q0 * fi2;
        tm2 += q0 * fi1 - q1 * fi0;
        te0 += elem_valid ? tm0 : 0.0; te1 += elem_valid ? tm1 : 0.0; te2 += elem_valid ? tm2 : 0.0;
    }
    if (has_contact && !P.contact_before_forcing) contact();

    if (node_valid) {
        const size_t nc = (size_t)(n + 1);
        double* o = out + (size_t)rod * kDynamicsRows * nc + (size_t)lane;
        o[0 * nc] = f0; o[1 * nc] = f1; o[2 * nc] = f2;
        o[3 * nc] = ti0; o[4 * nc] = ti1; o[5 * nc] = ti2;
        o[6 * nc] = fe0; o[7 * nc] = fe1; o[8 * nc] = fe2;
        o[9 * nc] = elem_valid ? te0 : 0.0; o[10 * nc] = elem_valid ? te1 : 0.0; o[11 * nc] = elem_valid ? te2 : 0.0;
        o[12 * nc] = (f0 + fe0) / mass; o[13 * nc] = (f1 + fe1) / mass; o[14 * nc] = (f2 + fe2) / mass;
        o[15 * nc] = elem_valid ? (M.invJ[0] * (ti0 + te0)) * e : 0.0;
        o[16 * nc] = elem_valid ? (M.invJ[1] * (ti1 + te1)) * e : 0.0;
        o[17 * nc] = elem_valid ? (M.invJ[2] * (ti2 + te2)) * e : 0.0;
    }
}

}  // namespace softrod
