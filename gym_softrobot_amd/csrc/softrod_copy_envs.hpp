// softrod_copy_envs.hpp — softrod_copy_envs_kernel: fork resident envs on the device (softrod_copy_envs).
//
// A cold kernel that EDITS the resident state between two steps, where the read-outs only read it: env dst becomes a
// bitwise copy of env src in every array that holds something per env.  It is a gather copy and nothing else: no
// arithmetic, no LDS, no atomics, no cross-lane traffic.
//
// The arrays travel as a small table in the kernel arguments (CopyTable), built by the host from the handle's
// pointers at every call, so that a per-env table allocated later (softrod_set_env_material / _contact) is seen.
// Every per-env array of the handle has one form, [comps][n_envs][row_bytes]: env e of component c starts at
//     base + (c * n_envs + e) * row_bytes
// i.e. the env stride is row_bytes and the component stride n_envs * row_bytes.  The rows of `lane_stride` doubles
// (position ... muscle_activation) have row_bytes = 512 or more; the columns [comps][n_envs] (time, control, head,
// bc_targets, env_aux) are the same form with row_bytes = 8; prev_action and prev_kappa have one component of a few
// floats; the muscle octopus's sucker rows [4][n_envs * n_arm] have row_bytes = n_arm entries; a per-env table is one
// component of sizeof(Row).
//
// One workgroup of kCopyThreads lanes per (src, dst) pair walks the table.  An array whose row_bytes is a multiple of
// 16 moves as 16-byte units, lane i of the workgroup at unit i of the env's comps * row_bytes / 16: within a row the
// lanes' addresses are consecutive, so a wave's access is 1 KiB contiguous for the 512-byte rows (two rows per wave),
// the widest there is.  Every base is a hipMalloc allocation (256-byte aligned), so those units are 16-byte aligned.
// The other arrays (8-byte columns, 28-byte prev_action rows, ...) are a few dozen bytes per env and move as 4-byte
// words, by the first lanes; a row that is no multiple of 4 bytes (the planar certificates: one byte per env, copied
// with the rows they vouch for) moves byte by byte.
//
// The host guarantees (softrod_copy_envs validates before it enqueues anything): every index is inside 0 .. n_envs - 1,
// no env is written twice, no env that is written is read by another pair, and no pair has src == dst — so the pairs'
// workgroups touch disjoint destination rows and read rows nobody writes: the result does not depend on scheduling.
#pragma once

namespace softrod {

constexpr int kCopyThreads = 256;
constexpr int kCopyMaxArrays = 24;

struct CopyArray {
    unsigned char* base;   // component 0 of env 0
    unsigned comps;        // components
    unsigned row_bytes;    // bytes of one env in one component (the env stride)
};
struct CopyTable {
    int n, n_envs;
    CopyArray a[kCopyMaxArrays];
};

// pairs: [gridDim.x] (src, dst)
__global__ void __launch_bounds__(kCopyThreads)
softrod_copy_envs_kernel(const CopyTable T, const int2* __restrict__ pairs) {
    const int2 p = pairs[blockIdx.x];
    const size_t N = (size_t)T.n_envs, src = (size_t)p.x, dst = (size_t)p.y;
    for (int k = 0; k < T.n; ++k) {
        const CopyArray A = T.a[k];
        const size_t comp_stride = N * (size_t)A.row_bytes;
        const unsigned char* from = A.base + src * (size_t)A.row_bytes;
        unsigned char* to = A.base + dst * (size_t)A.row_bytes;
        if ((A.row_bytes & 15u) == 0) {
            const unsigned per = A.row_bytes >> 4, total = A.comps * per;
            for (unsigned i = threadIdx.x; i < total; i += kCopyThreads) {
                const unsigned c = i / per, u = i - c * per;
                const size_t off = (size_t)c * comp_stride + ((size_t)u << 4);
                *reinterpret_cast<uint4*>(to + off) = *reinterpret_cast<const uint4*>(from + off);
            }
        } else if ((A.row_bytes & 3u) == 0) {
            const unsigned per = A.row_bytes >> 2, total = A.comps * per;
            for (unsigned i = threadIdx.x; i < total; i += kCopyThreads) {
                const unsigned c = i / per, u = i - c * per;
                const size_t off = (size_t)c * comp_stride + ((size_t)u << 2);
                *reinterpret_cast<unsigned*>(to + off) = *reinterpret_cast<const unsigned*>(from + off);
            }
        } else {
            const unsigned per = A.row_bytes, total = A.comps * per;
            for (unsigned i = threadIdx.x; i < total; i += kCopyThreads) {
                const unsigned c = i / per, u = i - c * per;
                const size_t off = (size_t)c * comp_stride + (size_t)u;
                to[off] = from[off];
            }
        }
    }
}

}  // namespace softrod
