// softrod_normalize.hpp — softrod_normalize_stats_kernel / softrod_normalize_rows_kernel / softrod_normalize_reset_kernel:
// running normalisation of observations and rewards, kept on the device (softrod_normalize_*, include/softrod.h).
//
// What Gymnasium's NormalizeObservation / NormalizeReward and Stable-Baselines3's VecNormalize do for host envs: a
// RunningMeanStd record per observation column and one for the discounted return, the observations centred and scaled
// by them, the rewards scaled by the return's deviation.  Cold kernels behind the step; no step kernel knows about them.
//
// Arrays (NormState; N envs, D observation columns), one device block:
//     rec f64[4][D + 1]      the records: rows mean, var, count, inv_std; columns 0 .. D-1 the observation columns, column
//                            D the discounted return.  A record starts at (0, 1, 1e-4, 1 / sqrt(1 + epsilon))
//     ret f64[N]             the discounted return of every env's running episode; zero at the start
//     latch u8[N]            the env finished on an earlier call and has not started a new episode (the meaning it has in
//                            softrod_episode_stats.hpp); zero at the start
//     norm_obs f32[N][D], norm_final_obs f32[N][D], norm_reward f64[N]     the outputs
//
// ONE UPDATE OF A COLUMN from the values x_e, e = 0 .. N-1, with weights c_e = the row is counted and x_e is finite:
//     n  = sum c_e                       (n == 0: the column keeps its record)
//     S  = osum(c_e ? (double)x_e : +0.0);  bm = S / n
//     Q  = osum(c_e ? ((double)x_e - bm) * ((double)x_e - bm) : +0.0);  bv = Q / n
//     delta = bm - mean;  tot = count + n
//     mean' = mean + (delta * n) / tot
//     M2    = ((var * count) + (bv * n)) + ((((delta * delta) * count) * n) / tot)
//     var'  = M2 / tot;  count' = tot;  inv_std' = 1.0 / sqrt(var' + epsilon)
// THE FIXED ORDER osum, the same for every N and D: partial p, p = 0 .. 15, adds the rows e = p, p + 16, p + 32, ... in
// ascending e, starting from +0.0; the 16 partials are then added in ascending p, starting from +0.0.  Every operation is
// one IEEE f64 rounding (fp contract off; f64 division and sqrt are correctly rounded on gfx950), so the NumPy twin
// (tests/normalize_ref.py) reproduces every array bit for bit.
//
// ONE STEP CALL (mode 0 manual reset, 1 NEXT_STEP, 2 SAME_STEP), with the latch as the call found it:
//     an unlatched env is reward-counted: ret = (ret * gamma) + reward; the return column is updated over the unlatched
//         envs with a finite ret; then, where terminated | truncated, ret = 0 and latch = (mode != 2)
//     a latched env keeps its ret; in mode 1 its latch clears (this was its reset call), in modes 0 and 2 it stays
//     observation rows counted: mode 0 the unlatched envs, modes 1 and 2 every env
//     norm_obs[e][d] = (float) clamp(((double)obs[e][d] - mean'[d]) * inv_std'[d], -clip_obs, +clip_obs)
//     norm_final_obs: the same of final_obs, for the rows of the envs that finished on this call (unlatched and
//         terminated | truncated); the other rows keep their contents; never counted
//     norm_reward[e] = clamp(reward[e] * inv_std'[D], -clip_reward, +clip_reward): no mean is subtracted
//     a NaN gives the canonical quiet NaN (0x7fc00000, 0x7ff8000000000000), +-inf clamps to +-clip
//     update == 0 (evaluation): nothing is counted, ret and latch stay; the outputs are still written
// ONE RESET CALL: the observation rows of the masked envs are counted (no mask: all); their ret and latch become zero
// (whatever `update` says: a reset starts an episode); every row of norm_obs is written.
//
// LAUNCH SHAPES.  At most two launches per call, no atomics, no waiting between workgroups.
//   softrod_normalize_stats_kernel (only with update != 0): one workgroup of 1024 threads per tile of 64 observation
//     columns, lane <-> column, so a wave reads one 256-byte row segment coalesced; the 16 waves are the 16 partials.
//     The kernel is bound by the latency of its row loads, not by their bytes, so a wave loads 32 of its rows before it
//     adds them, in order: 32 loads in flight per wave, ceil(N / 512) round trips per pass.  Two passes over the tile,
//     sums then squared deviations (the second finds the tile in the L2); the partials meet in LDS (20 KiB)
//     and every thread adds them in ascending p.  ONE MORE WORKGROUP of the same launch owns the return: it updates ret
//     of the unlatched envs, __syncthreads() makes those stores visible to its own waves, and the same two passes run
//     over ret as the one column: there lane l of a wave fetches the wave's row 64 k + l, and the 64 values are added in
//     ascending row order through v_readlane.  No other workgroup of the launch reads ret, and none writes the latch.
//   softrod_normalize_rows_kernel / softrod_normalize_reset_kernel: one wave per env row.  The wave reads the env's
//     latch and flags once, writes the row of norm_obs (and of norm_final_obs where the env finished), and lane 0 then
//     writes norm_reward, zeroes ret and moves the latch.  Only this wave touches the env's latch in the launch, and it
//     has read it before it writes it.
// Every index is e < N or d < D (d == D: the return's record); nothing private is indexed at run time (the 32-row
// batches are fully unrolled).  The kernels only enqueue work — no allocation, synchronisation or host read — so they
// are capturable.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace softrod {

constexpr int kNormWaves = 16;                      // the partials of osum
constexpr int kNormThreads = kNormWaves * 64;
constexpr int kNormTile = 64;                       // observation columns per workgroup
constexpr int kNormBatch = 32;                      // rows a wave loads before it adds them
constexpr int kNormRowWaves = 4;                    // env rows per workgroup of the row kernels

struct NormState {
    double* rec;                // [4][D + 1]: mean, var, count, inv_std
    double* ret;
    uint8_t* latch;
    float* norm_obs;
    float* norm_final_obs;
    double* norm_reward;
    int n_envs;
    int obs_dim;
    int obs_on;
    int reward_on;
    double gamma, clip_obs, clip_reward, epsilon;
};

__device__ __forceinline__ bool norm_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool norm_finite(double x) {
    return ((unsigned)__double2hiint(x) & 0x7ff00000u) != 0x7ff00000u;
}

struct NormPartials {           // the workgroup's LDS: every wave's partial of every column of the tile
    double sum[kNormWaves][kNormTile];
    double sq[kNormWaves][kNormTile];
    int n[kNormWaves][kNormTile];
};

// One wave's partial of one pass over an observation column: the rows e = wave, wave + 16, ... in ascending order,
// 32 loaded before they are added.  first pass: acc += c_e ? x_e : +0.0 and n += c_e; second: acc += c_e ? (x_e - bm)^2
// : +0.0.  A row is counted where `flag` is nullptr or (flag[e] != 0) == flag_set.  A row past N adds +0.0: a sum
// that starts at +0.0 is never -0.0, so it stays as it is.
template <bool second, bool flagged>
__device__ __forceinline__ void norm_tile_partial(const float* __restrict__ obs, const uint8_t* flag, const bool flag_set,
                                                  const int col, const bool live, const int N, const int D,
                                                  const double bm, double& acc, int& n) {
#pragma clang fp contract(off)
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);     // wave-uniform: row addresses are scalar
    const size_t at = (size_t)(live ? col : D - 1);     // an idle lane and a row past N load a valid element and drop it:
    for (int e0 = wave; e0 < N; e0 += kNormWaves * kNormBatch) {       // no branch, so nothing waits between the loads
        float x[kNormBatch];                        // floats wait in half the registers; widened when they are added
        uint8_t f[kNormBatch];
#pragma unroll
        for (int u = 0; u < kNormBatch; ++u) {
            const int e = e0 + kNormWaves * u, ec = e < N ? e : N - 1;
            x[u] = obs[(size_t)ec * (size_t)D + at];
            f[u] = flagged ? flag[ec] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < kNormBatch; ++u) {
            const bool counted = !flagged || ((f[u] != 0) == flag_set);
            const bool ok = live && (e0 + kNormWaves * u < N) && counted && norm_finite(x[u]);
            const double dev = (double)x[u] - bm;
            acc += ok ? (second ? dev * dev : (double)x[u]) : 0.0;
            n += ok ? 1 : 0;
        }
    }
}

// The same partial over the one column ret, counted where the latch is clear.  The column has work for one lane only, so
// the other 63 fetch for it: lane l loads the wave's row number 64 k + l (e = wave + 16 (64 k + l)), and the 64 values
// are then added in ascending e, read lane by lane (v_readlane: the lane index is a constant of the unrolled loop).
// Every lane ends with the same sum.
template <bool second>
__device__ __forceinline__ void norm_ret_partial(const double* ret, const uint8_t* latch, const int N, const double bm,
                                                 double& acc, int& n) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    for (int base = wave; base < N; base += kNormWaves * 64) {
        const int e = base + kNormWaves * lane;
        double v = 0.0;
        bool ok = false;
        if (e < N) {
            v = ret[e];
            ok = !latch[e] && norm_finite(v);
        }
        const double dev = v - bm;
        const double term = ok ? (second ? dev * dev : v) : 0.0;
        n += __popcll(__ballot(ok));
        const int lo = __double2loint(term), hi = __double2hiint(term);
#pragma unroll
        for (int u = 0; u < 64; ++u)
            acc += __hiloint2double(__builtin_amdgcn_readlane(hi, u), __builtin_amdgcn_readlane(lo, u));
    }
}

// One update of record `slot` of S.rec.  partial(second, bm, acc, n), `second` a std::bool_constant, adds this wave's partial of the column this lane
// owns.  Called by every thread of the workgroup; `live` lanes own a column, the others carry zeros.
template <class Partial>
__device__ __forceinline__ void norm_column_update(const NormState& S, NormPartials& L, const int slot, const bool live,
                                                   Partial partial) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    double sum = 0.0;
    int n = 0;
    partial(std::false_type{}, 0.0, sum, n);
    L.sum[wave][lane] = sum;
    L.n[wave][lane] = n;
    __syncthreads();
    double total = 0.0;
    int count = 0;
#pragma unroll
    for (int p = 0; p < kNormWaves; ++p) {
        total += L.sum[p][lane];
        count += L.n[p][lane];
    }
    const double dn = (double)count;
    const double bm = total / dn;                   // NaN where count == 0: that column keeps its record
    double sq = 0.0;
    int again = 0;
    partial(std::true_type{}, bm, sq, again);
    L.sq[wave][lane] = sq;
    __syncthreads();
    if (wave != 0 || !live || count == 0) return;
    double q = 0.0;
#pragma unroll
    for (int p = 0; p < kNormWaves; ++p) q += L.sq[p][lane];
    const double bv = q / dn;
    const size_t W = (size_t)S.obs_dim + 1;
    const double mean = S.rec[slot], var = S.rec[W + slot], cnt = S.rec[2 * W + slot];
    const double delta = bm - mean, tot = cnt + dn;
    const double m2 = ((var * cnt) + (bv * dn)) + ((((delta * delta) * cnt) * dn) / tot);
    const double var1 = m2 / tot;
    S.rec[slot] = mean + (delta * dn) / tot;
    S.rec[W + slot] = var1;
    S.rec[2 * W + slot] = tot;
    S.rec[3 * W + slot] = 1.0 / sqrt(var1 + S.epsilon);
}

// The statistics of one call.  Launch: <<<tiles + (reward ? 1 : 0), kNormThreads>>>, tiles = ceil(D / 64) or 0.
// Workgroups 0 .. tiles-1 update the observation columns from `obs` [N][D]; a row is counted where `flag` is nullptr or
// (flag[e] != 0) == flag_set (a step in mode 0: the latch, clear; a masked reset: the mask, set).  With `reward` the
// last workgroup updates ret of the unlatched envs and the return's record.
__global__ void __launch_bounds__(kNormThreads)
softrod_normalize_stats_kernel(const NormState S, const int tiles, const float* __restrict__ obs,
                               const uint8_t* flag, const bool flag_set, const double* __restrict__ reward) {
#pragma clang fp contract(off)
    __shared__ NormPartials L;
    const int lane = (int)threadIdx.x & 63;
    const int N = S.n_envs, D = S.obs_dim;
    if ((int)blockIdx.x < tiles) {
        const int col = (int)blockIdx.x * kNormTile + lane;
        const bool live = col < D;
        norm_column_update(S, L, live ? col : 0, live, [&](auto second, const double bm, double& acc, int& n) {
            if (flag) norm_tile_partial<decltype(second)::value, true>(obs, flag, flag_set, col, live, N, D, bm, acc, n);
            else norm_tile_partial<decltype(second)::value, false>(obs, flag, flag_set, col, live, N, D, bm, acc, n);
        });
        return;
    }
    // the return: ret of the unlatched envs first, then the column over what this workgroup has just written
    double* const ret = S.ret;
    const uint8_t* const latch = S.latch;
    for (int e = (int)threadIdx.x; e < N; e += kNormThreads)
        if (!latch[e]) ret[e] = (ret[e] * S.gamma) + reward[e];
    __syncthreads();
    norm_column_update(S, L, D, lane == 0, [&](auto second, const double bm, double& acc, int& n) {
        norm_ret_partial<decltype(second)::value>(ret, latch, N, bm, acc, n);
    });
}

__device__ __forceinline__ float norm_obs_value(const float x, const double mean, const double inv_std, const double clip) {
#pragma clang fp contract(off)
    const double v = ((double)x - mean) * inv_std;
    if (v != v) return __uint_as_float(0x7fc00000u);
    return (float)(v < -clip ? -clip : (v > clip ? clip : v));
}

// One wave per env row: norm_obs, the finished envs' norm_final_obs rows, norm_reward, and with `update` the end of the
// row rules (ret = 0 and the latch).  `final_obs` may be nullptr.  Launch: <<<ceil(N / 4), 256>>>.
__global__ void __launch_bounds__(kNormRowWaves * 64)
softrod_normalize_rows_kernel(const NormState S, const float* __restrict__ obs, const double* __restrict__ reward,
                              const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated,
                              const float* __restrict__ final_obs, const int mode, const int update) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * kNormRowWaves + ((int)threadIdx.x >> 6);
    const int D = S.obs_dim;
    if (e >= S.n_envs) return;
    const size_t W = (size_t)D + 1;
    const bool latched = S.latch[e] != 0;
    const bool finished = !latched && ((terminated[e] | truncated[e]) != 0);
    if (S.obs_on) {
        const size_t at = (size_t)e * (size_t)D;
        for (int d = lane; d < D; d += 64) {
            const double mean = S.rec[d], inv_std = S.rec[3 * W + d];
            S.norm_obs[at + d] = norm_obs_value(obs[at + d], mean, inv_std, S.clip_obs);
            if (final_obs && finished) S.norm_final_obs[at + d] = norm_obs_value(final_obs[at + d], mean, inv_std, S.clip_obs);
        }
    }
    if (lane != 0) return;
    if (S.reward_on) {
        const double v = reward[e] * S.rec[3 * W + D], c = S.clip_reward;
        S.norm_reward[e] = v != v ? __longlong_as_double(0x7ff8000000000000ll) : (v < -c ? -c : (v > c ? c : v));
    }
    if (!update) return;
    if (latched) {
        if (mode == 1) S.latch[e] = 0;
    } else if (finished) {
        S.ret[e] = 0.0;
        S.latch[e] = mode != 2 ? 1 : 0;
    }
}

// The reset call's rows: every row of norm_obs; ret and latch of the masked envs (nullptr: all) become zero.
// Launch: <<<ceil(N / 4), 256>>>.
__global__ void __launch_bounds__(kNormRowWaves * 64)
softrod_normalize_reset_kernel(const NormState S, const float* __restrict__ obs, const uint8_t* __restrict__ mask) {
    const int lane = (int)threadIdx.x & 63;
    const int e = (int)blockIdx.x * kNormRowWaves + ((int)threadIdx.x >> 6);
    const int D = S.obs_dim;
    if (e >= S.n_envs) return;
    if (S.obs_on) {
        const size_t W = (size_t)D + 1, at = (size_t)e * (size_t)D;
        for (int d = lane; d < D; d += 64)
            S.norm_obs[at + d] = norm_obs_value(obs[at + d], S.rec[d], S.rec[3 * W + d], S.clip_obs);
    }
    if (lane == 0 && (!mask || mask[e])) {
        S.ret[e] = 0.0;
        S.latch[e] = 0;
    }
}

}  // namespace softrod
