// softrod_joint_readout.hpp — softrod_joint_loads: what FixedJoint2Rigid computes in every substep and returns none
// of (utils/custom_elastica/joint.py:47-219: _apply_forces returns contact_force and apply_forces drops it) — the
// force and the restoring torque every arm's joint exchanges with the rigid body, the gap it acts on, and what the
// body makes of their sum: the net load and the acceleration an IMU on the body would read — on the device.
//
// A cold kernel beside the step kernels.  Unlike the per-rod read-outs (softrod_readout.hpp: one wave per rod) it
// runs ONE WAVE PER ENV, grid n_envs: lane a < rods owns arm a and gathers node 0, node 1 and element 0's directors
// of that arm from the env's rows at arm * arm_stride (readout_rod's addressing: an env's row is `lane_stride` wide),
// the body comes through load_head.  Lanes >= rods read nothing and store nothing.  No LDS, no atomics, no scratch.
//
// THE INSTANT is softrod_ground_reaction's: ONE evaluation at x, v, Q of the arms and of the body as they stand in
// memory — no half kinematic step, no constrain_values.  It is not the value the last substep applied.
//
// THE ARITHMETIC is joint_load_literal's (softrod_literal.hpp): the literal fp64 form of the law, which no step
// kernel inlines, the one rod_literal_joint calls for the ground reaction and the rod dynamics.  Force, torque and
// the gap they act on (end_distance_vector, end_distance) come from that ONE computation, as they do in the NumPy
// twin tests/test_gpu_joint_loads.py holds them to.  Everything in this file is compiled without floating-point
// contraction, so that a product followed by a sum rounds twice, as NumPy does in diagnostics.joint_loads_host and
// oracle/softrod_oracle_np.py.
//
// THE NET ROW is formed in a fixed loop a = 0 .. rods - 1 that reads lane a's values with a wave shuffle and adds
// them left to right to +0.0: the order of the reference's loop over its connections (head.f_ext += ...), the same
// in every lane and in every run.  The body's rates follow NumpyCylinder.dynamic / BodyBoundaryCondition
// .compute_constrain_rates: a = f / m with a_z held at +0.0; alpha = (+0.0, +0.0, invJ_3 t_3) — the gyroscopic term
// (J w) x w vanishes identically for a body whose omega is held to (0, 0, w_3) and whose J is diagonal.  With
// head_fixed (OneEndFixedBC on the body, OctoReach) all six are +0.0; the loads are still reported.
//
// out: [n_envs][rods + 1][16] —
//   row a < rods, the joint of arm a:
//     0-2    contact_force: added to the body's external_forces, lab frame
//     3-5    -Q_body torque: added to the body's external_torques, body frame
//     6-8    -contact_force: added to the arm's node 0 (the exact negation of 0-2)
//     9-11   Q_arm[.., 0] torque: added to the arm's element 0, that element's material frame
//     12-14  end_distance_vector: node 0 minus its connection point
//     15     end_distance
//   row rods, the body:
//     0-2    net force: columns 0-2 summed over the arms in arm order
//     3-5    net torque: columns 3-5 summed the same way
//     6-8    linear acceleration            9-11   angular acceleration, body frame            12-15  +0.0
#pragma once

namespace softrod {

constexpr int kJointCols = 16;

__global__ void __launch_bounds__(kLanes)
softrod_joint_loads_kernel(const RodParams P, const StatePtrs S, const int rods, const int lane_stride,
                           const int arm_stride, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int env = blockIdx.x;
    const int arm = threadIdx.x;
    const size_t N = (size_t)P.n_envs, W = (size_t)lane_stride;
    const bool owns = arm < rods;
    double x0[3] = {0.0, 0.0, 0.0}, v0[3] = {0.0, 0.0, 0.0}, x1[3] = {0.0, 0.0, 0.0};
    double Q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (owns) {                                        // slots of other arms and past the env's row are never read
        const size_t i = (size_t)env * W + (size_t)arm * (size_t)arm_stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x0[c] = S.pos[c * N * W + i];
            x1[c] = S.pos[c * N * W + i + 1];
            v0[c] = S.vel[c * N * W + i];
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) Q[c] = S.dir[c * N * W + i];
    }
    HeadState H;
    double tgt[2];
    load_head(S, N, env, H, tgt);

    // Lanes >= rods run the law on zeros: finite values that no shuffle below reads and no store writes; every lane
    // has to reach the shuffle loop.
    const JointLoad J = joint_load_literal(P, H, arm, x0, v0, x1);
    const double (&fj)[3] = J.f, (&tj)[3] = J.t;

    double bt[3], at[3];                               // the torque in the body's frame, negated, and in element 0's
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        bt[i] = -((H.Q[3 * i] * tj[0] + H.Q[3 * i + 1] * tj[1]) + H.Q[3 * i + 2] * tj[2]);
        at[i] = (Q[3 * i] * tj[0] + Q[3 * i + 1] * tj[1]) + Q[3 * i + 2] * tj[2];
    }

    // the body's row: every lane forms the same sums in the same order
    double nf[3] = {0.0, 0.0, 0.0}, nt[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < rods; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nf[c] += __shfl(fj[c], a);
            nt[c] += __shfl(bt[c], a);
        }
    }

    double* o = out + ((size_t)env * (size_t)(rods + 1) + (size_t)arm) * kJointCols;
    if (owns) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = fj[c];
            o[3 + c] = bt[c];
            o[6 + c] = -fj[c];
            o[9 + c] = at[c];
            o[12 + c] = J.gap[c];
        }
        o[15] = J.dist;
    }
    if (arm == 0) {
        double* b = out + ((size_t)env * (size_t)(rods + 1) + (size_t)rods) * kJointCols;
        const bool held = P.head_fixed != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { b[c] = nf[c]; b[3 + c] = nt[c]; }
        b[6] = held ? 0.0 : nf[0] / P.head_mass;
        b[7] = held ? 0.0 : nf[1] / P.head_mass;
        b[8] = 0.0;
        b[9] = 0.0;
        b[10] = 0.0;
        b[11] = held ? 0.0 : P.head_invJ[2] * nt[2];
#pragma unroll
        for (int c = 12; c < 16; ++c) b[c] = 0.0;
    }
}

}  // namespace softrod
