// softrod_state_bank.hpp — softrod_bank_copy_kernel: save env states into off-batch slots and load them back
// (softrod_bank_save / softrod_bank_load).
//
// A state bank is a second set of the handle's per-env arrays with `slots` rows where the batch has n_envs: one slot
// holds everything softrod_copy_envs copies for one env.  The step and reset kernels never see it.  This cold kernel is
// softrod_copy_envs_kernel with the two sides in different allocations: a gather copy and nothing else — no
// arithmetic, no LDS, no atomics, no cross-lane traffic.
//
// The two sides travel as two CopyTables (softrod_copy_envs.hpp) in the kernel arguments.  The host derives the bank's
// table from the batch's (copy_table), so the two list the same arrays in the same order with equal `comps` and
// `row_bytes`; only `base` and `n_envs` — the component stride in rows — differ.  Row r of component c of an array
// starts at
//     base + (c * n_envs + r) * row_bytes
// on its own side.  One kernel serves both directions: a save has From = batch, To = bank and pairs (env, slot); a load
// has From = bank, To = batch and pairs (slot, env).
//
// One workgroup of kCopyThreads lanes per (from, to) pair walks the table, exactly as softrod_copy_envs_kernel does: an
// array whose row_bytes is a multiple of 16 moves as 16-byte units, lane i of the workgroup at unit i of the row's
// comps * row_bytes / 16, so a wave's access is 1 KiB contiguous for the 512-byte rows (two rows per wave); every base
// on either side is a hipMalloc allocation (256-byte aligned), so those units are 16-byte aligned.  The other arrays
// (8-byte columns, 28-byte prev_action rows, ...) move as 4-byte words, by the first lanes.
//
// The host guarantees (softrod_bank_save / _load validate before they enqueue anything): every `from` index is inside
// From.n_envs, every `to` index inside To.n_envs, and no `to` index appears twice.  The two sides never alias, so the
// pairs' workgroups write disjoint rows and read rows nobody writes: the result does not depend on scheduling.
#pragma once

#include "softrod_copy_envs.hpp"

namespace softrod {

// pairs: [gridDim.x] (row of From, row of To)
__global__ void __launch_bounds__(kCopyThreads)
softrod_bank_copy_kernel(const CopyTable From, const CopyTable To, const int2* __restrict__ pairs) {
    const int2 p = pairs[blockIdx.x];
    const size_t src = (size_t)p.x, dst = (size_t)p.y;
    for (int k = 0; k < From.n; ++k) {
        const CopyArray A = From.a[k];
        const unsigned char* to_base = To.a[k].base;
        const size_t row = (size_t)A.row_bytes;
        const size_t from_stride = (size_t)From.n_envs * row, to_stride = (size_t)To.n_envs * row;
        const unsigned char* from = A.base + src * row;
        unsigned char* to = const_cast<unsigned char*>(to_base) + dst * row;
        if ((A.row_bytes & 15u) == 0) {
            const unsigned per = A.row_bytes >> 4, total = A.comps * per;
            for (unsigned i = threadIdx.x; i < total; i += kCopyThreads) {
                const unsigned c = i / per, u = i - c * per;
                const size_t in = ((size_t)u << 4);
                *reinterpret_cast<uint4*>(to + (size_t)c * to_stride + in) =
                    *reinterpret_cast<const uint4*>(from + (size_t)c * from_stride + in);
            }
        } else if ((A.row_bytes & 3u) == 0) {
            const unsigned per = A.row_bytes >> 2, total = A.comps * per;
            for (unsigned i = threadIdx.x; i < total; i += kCopyThreads) {
                const unsigned c = i / per, u = i - c * per;
                const size_t in = ((size_t)u << 2);
                *reinterpret_cast<unsigned*>(to + (size_t)c * to_stride + in) =
                    *reinterpret_cast<const unsigned*>(from + (size_t)c * from_stride + in);
            }
        } else {      // the planar certificates: one byte per env
            const unsigned per = A.row_bytes, total = A.comps * per;
            for (unsigned i = threadIdx.x; i < total; i += kCopyThreads) {
                const unsigned c = i / per, u = i - c * per;
                to[(size_t)c * to_stride + u] = from[(size_t)c * from_stride + u];
            }
        }
    }
}

}  // namespace softrod
