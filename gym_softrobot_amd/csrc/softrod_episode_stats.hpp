// softrod_episode_stats.hpp — softrod_episode_stats_kernel / softrod_episode_stats_clear_kernel: the return and length of
// every episode that ends, kept on the device (softrod_episode_stats_update / _reset, include/softrod.h).
//
// What every RL run plots is the return and length of the episodes that just ended.  In the device reset modes the
// host never sees which env finished on which call, so the bookkeeping lives here: per-env accumulators, this call's
// info rows (Gymnasium's infos["episode"] / infos["_episode"]) and a ring of the last K finished episodes of the batch.
// One cold kernel behind the step; no step kernel knows about it.
//
// Arrays (EpisodeStats; N envs, ring length K), all zero when the feature is switched on:
//     acc_return f64[N], acc_length i32[N]   the running episode of every env
//     latch u8[N]                            the env finished on an earlier call and has not started a new episode
//     finished i32[N]                        episodes ended per env since enabling
//     ep_r f64[N], ep_l i32[N], ep_t f64[N], ep_mask u8[N]
//                                            this call's info rows: return, length, end time where ep_mask, else zero
//     ring_r f64[K], ring_l i32[K], ring_t f64[K], ring_env i32[K]
//                                            the last K finished episodes; episode number c (0-based, batch-wide) is in
//                                            slot c % K
//     count u64[1]                           episodes finished by the whole batch since enabling
//
// One update per env.step, for env e (mode 0 manual reset, 1 NEXT_STEP auto-reset, 2 SAME_STEP auto-reset):
//     if latch[e]:                           rows of e = 0; mode 1: latch[e] = 0 (this call was the env's reset call:
//                                            reward 0, no step of any episode); mode 0: stays latched until the clear
//     else: acc_return[e] += reward[e]; acc_length[e] += 1
//           if terminated[e] | truncated[e]: rows of e = (acc_return, acc_length, end_time[e], 1); ring push;
//                                            finished[e] += 1; accumulators = 0; latch[e] = (mode != 2)
//           else:                            rows of e = 0
// The latch is Gymnasium's prev_dones: in the host-driven NEXT_STEP mode the backend steps a finished env once more
// and the env layer discards that step; the latch makes the kernel discard it too.
//
// THE RING PUSH IS DETERMINISTIC: within one call the finished envs push in ascending env index.  The env of rank r
// among this call's F finished envs writes slot (count + r) % K; when F > K only ranks >= F - K write — K consecutive
// episode numbers, so no two envs write one slot, and the ring holds what F sequential pushes would have left.
// count += F once, at the end.
//
// LAUNCH SHAPE: ONE workgroup of 1024 threads (16 waves) walks the envs in chunks of 1024, in two passes.  Pass A counts
// F: a 64-bit __ballot per wave and chunk, __popcll, the 16 wave totals through LDS.  Pass B does the update: an env's
// rank is the popcount of its wave's ballot below its lane, plus the lower waves' totals of the chunk (LDS), plus a
// running base carried from chunk to chunk.  No atomics and no waiting between workgroups: a look-back scan over many
// workgroups would be faster at very large N, but a spin loop is not worth a hang on a shared machine.  The cost grows
// with ceil(N / 1024): at 4096 envs four chunks per pass.  Env e is handled by the same thread in both passes, and
// only that thread touches its rows, so pass B sees latch[e] as pass A did.  Nothing is indexed at run time but the
// ring slot, which is < K by the modulo; every other index is e < N.  The kernel only enqueues work — no allocation,
// synchronisation or host read — so it is capturable.
//
// A return is a sequence of f64 adds in call order and nothing else here is floating-point arithmetic: the NumPy twin
// (tests/episode_stats_ref.py) reproduces every array bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace softrod {

constexpr int kStatsThreads = 1024;     // one workgroup: 16 waves of 64
constexpr int kStatsWaves = kStatsThreads / 64;

struct EpisodeStats {
    double* acc_return;
    int* acc_length;
    uint8_t* latch;
    int* finished;
    double* ep_r;
    int* ep_l;
    double* ep_t;
    uint8_t* ep_mask;
    double* ring_r;
    int* ring_l;
    double* ring_t;
    int* ring_env;
    unsigned long long* count;
    int n_envs;
    int ring;
};

// end_time: [N] or nullptr (t = 0).  Launch: <<<1, kStatsThreads>>>.
__global__ void __launch_bounds__(kStatsThreads)
softrod_episode_stats_kernel(const EpisodeStats S, const double* __restrict__ reward, const uint8_t* __restrict__ terminated,
                             const uint8_t* __restrict__ truncated, const double* __restrict__ end_time, const int mode) {
    __shared__ int s_wave[kStatsWaves];             // pass A: every wave's total; pass B: this chunk's wave totals
    __shared__ int s_total;                         // F
    __shared__ unsigned long long s_count;          // count before this call
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = S.n_envs, K = S.ring;

    // ---- pass A: F = the envs that end an episode on this call ----
    int wave_sum = 0;                               // wave-uniform
    for (int base = 0; base < N; base += kStatsThreads) {
        const int e = base + tid;
        const bool fin = e < N && !S.latch[e] && ((terminated[e] | truncated[e]) != 0);
        wave_sum += __popcll(__ballot(fin));
    }
    if (lane == 0) s_wave[wave] = wave_sum;
    __syncthreads();
    if (tid == 0) {
        int f = 0;
        for (int w = 0; w < kStatsWaves; ++w) f += s_wave[w];
        s_total = f;
        s_count = S.count[0];
    }
    __syncthreads();
    const int F = s_total;
    const unsigned long long count = s_count;
    const int first = F > K ? F - K : 0;            // the lowest rank that still has a slot

    // ---- pass B: the update, ranks in ascending env index ----
    int chunk_base = 0;                             // finished envs in the chunks before this one
    for (int base = 0; base < N; base += kStatsThreads) {
        const int e = base + tid;
        const bool live = e < N;
        const bool latched = live && S.latch[e] != 0;
        const bool fin = live && !latched && ((terminated[e] | truncated[e]) != 0);
        const unsigned long long votes = __ballot(fin);
        __syncthreads();                            // the previous chunk's totals have been read
        if (lane == 0) s_wave[wave] = __popcll(votes);
        __syncthreads();
        int below = 0, total = 0;
        for (int w = 0; w < kStatsWaves; ++w) {
            const int t = s_wave[w];
            below += w < wave ? t : 0;
            total += t;
        }
        if (live) {
            double r = 0.0, t = 0.0;
            int l = 0;
            if (latched) {
                if (mode == 1) S.latch[e] = 0;
            } else {
                const double ret = S.acc_return[e] + reward[e];
                const int len = S.acc_length[e] + 1;
                if (fin) {
                    r = ret;
                    l = len;
                    t = end_time ? end_time[e] : 0.0;
                    const int rank = chunk_base + below + __popcll(votes & ((1ull << lane) - 1ull));
                    if (rank >= first) {
                        const int slot = (int)((count + (unsigned long long)rank) % (unsigned long long)K);
                        S.ring_r[slot] = r;
                        S.ring_l[slot] = l;
                        S.ring_t[slot] = t;
                        S.ring_env[slot] = e;
                    }
                    S.finished[e] += 1;
                    S.acc_return[e] = 0.0;
                    S.acc_length[e] = 0;
                    if (mode != 2) S.latch[e] = 1;
                } else {
                    S.acc_return[e] = ret;
                    S.acc_length[e] = len;
                }
            }
            S.ep_r[e] = r;
            S.ep_l[e] = l;
            S.ep_t[e] = t;
            S.ep_mask[e] = fin ? 1 : 0;
        }
        chunk_base += total;
    }
    if (tid == 0) S.count[0] = count + (unsigned long long)F;
}

// The masked clear (softrod_episode_stats_reset): accumulators, latch and info rows of the envs with mask != 0 (nullptr:
// every env) become zero — a manual reset discards a partial episode.  The ring, `finished` and `count` stay.
__global__ void __launch_bounds__(256)
softrod_episode_stats_clear_kernel(const EpisodeStats S, const uint8_t* __restrict__ mask) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= S.n_envs || (mask && !mask[e])) return;
    S.acc_return[e] = 0.0;
    S.acc_length[e] = 0;
    S.latch[e] = 0;
    S.ep_r[e] = 0.0;
    S.ep_l[e] = 0;
    S.ep_t[e] = 0.0;
    S.ep_mask[e] = 0;
}

}  // namespace softrod
