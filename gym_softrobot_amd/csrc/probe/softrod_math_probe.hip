// softrod_math_probe.hip — the SOFTROD_MATH_FAST device primitives, one at a time, on plain arrays.
//
// A test-only library (variants/libsoftrod_math_probe.so, `make probe`): it includes the shipped headers
// unchanged and is NOT one of the shipped library's sources (a subdirectory, a .hip suffix), so
// libsoftrod_hip.so and its source hash do not know it exists.  tests/test_gpu_math_primitives.py compares
// what it returns with 50-digit references.
//
// One element-wise kernel per form, in blocks of 64 threads: a wave is exactly 64 consecutive inputs, which
// is what the primitives' wave-uniform range checks see.  The lanes behind the n-th input (n need not be a
// multiple of 64) repeat the last input and store nothing, so they never change the tier a wave takes.
#include "../softrod_kernels.hpp"

namespace {
using namespace softrod;

enum Which : int {
    kFastRcp = 0,
    kFastRsqrt = 1,
    kSeedRcp = 2,           // __builtin_amdgcn_rcp, for the record
    kSeedRsq = 3,           // __builtin_amdgcn_rsq, for the record
    kSincCoscLean = 4,      // sinc_cosc<true>(a) -> out0 = sinc, out1 = cosc
    kSincCoscPlain = 5,     // sinc_cosc<false>
    kSeries6 = 6,           // theta_over_sin_series<6>(a)
    kSeries12 = 7,
    kSeries20 = 8,
    kThetaOverSin = 9,      // theta_over_sin<false>(a, valid)
    kThetaOverSinBatched = 10,
    kEpsSinFactor = 11,     // eps_sin_factor(a, b)
    kExpPair = 12,          // exp_pair(a, b, valid) -> out0, out1
    kExpWidePair = 13,      // exp_wide_pair(a, b)
    kExpOne = 14,           // exp_one<1>(K, a), K from planar_build_const
    kPlanarRotation = 15,   // planar_kinematic_n<1> on c = 1, s = 0, wz = a -> out0 = c, out1 = s
    kWhichCount = 16
};

// the planar loop's constants as planar_build_const makes them, from a rod whose every scale is 1
__device__ __forceinline__ void unit_planar_const(int lane, ConstN<1>& C, PlanarC<1>& K) {
    RodParams P{};
    P.n_elem = kLanes - 1;
    P.dt = 1.0; P.half_dt = 0.5;
    P.rest_len = 1.0; P.inv_rest_len = 1.0;
    P.rest_vor = 1.0; P.inv_rest_vor = 1.0;
    P.J[0] = P.J[1] = P.J[2] = 1.0;
    P.damp_t = 1.0;
    P.eps_length = 1.0e-14; P.acos_shift = 1.0e-10; P.eps_sin = 1.0e-14;
    P.two_acos_shift = 2.0e-10; P.neg_eps_sin = -1.0e-14;
    C = ConstN<1>{};
    C.hx[0] = 1.0; C.hq[0] = 1.0;
    planar_build_const<1>(P, C, lane, K);
}

template <int W>
__global__ void __launch_bounds__(kLanes)
probe_kernel(const double* __restrict__ a, const double* __restrict__ b, const unsigned char* __restrict__ valid,
             double* __restrict__ out0, double* __restrict__ out1, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    const size_t j = i < n ? i : n - 1;        // (n >= 1: the entry point returns before a launch of nothing)
    const double x = a[j];
    const double x2 = b ? b[j] : 0.0;
    const bool ok = valid ? valid[j] != 0 : true;
    double r0 = 0.0, r1 = 0.0;
    if constexpr (W == kFastRcp) r0 = fast_rcp(x);
    else if constexpr (W == kFastRsqrt) r0 = fast_rsqrt(x);
    else if constexpr (W == kSeedRcp) r0 = __builtin_amdgcn_rcp(x);
    else if constexpr (W == kSeedRsq) r0 = __builtin_amdgcn_rsq(x);
    else if constexpr (W == kSincCoscLean) sinc_cosc<true>(x, r0, r1);
    else if constexpr (W == kSincCoscPlain) sinc_cosc<false>(x, r0, r1);
    else if constexpr (W == kSeries6) r0 = theta_over_sin_series<6>(x);
    else if constexpr (W == kSeries12) r0 = theta_over_sin_series<12>(x);
    else if constexpr (W == kSeries20) r0 = theta_over_sin_series<20>(x);
    else if constexpr (W == kThetaOverSin) r0 = theta_over_sin<false>(x, ok);
    else if constexpr (W == kThetaOverSinBatched) r0 = theta_over_sin<true>(x, ok);
    else if constexpr (W == kEpsSinFactor) r0 = eps_sin_factor(x, x2);
    else if constexpr (W == kExpPair) exp_pair(x, x2, ok, r0, r1);
    else if constexpr (W == kExpWidePair) exp_wide_pair(x, x2, r0, r1);
    else if constexpr (W == kExpOne) {
        ConstN<1> C;
        PlanarC<1> K;
        unit_planar_const((int)threadIdx.x, C, K);
        r0 = exp_one<1>(K, x);
    } else if constexpr (W == kPlanarRotation) {
        ConstN<1> C;
        PlanarC<1> K;
        unit_planar_const((int)threadIdx.x, C, K);
        PlanarN<1> Z{};
        Z.c[0] = 1.0; Z.s[0] = 0.0; Z.s2 = 1.0;
        Z.wz[0] = x;
        planar_kinematic_n<1>(1.0, K.hq_dt, C, K, Z);     // h = dt = 1, hq = 1: the element turns by wz
        r0 = Z.c[0]; r1 = Z.s[0];
    }
    if (i < n) {
        out0[i] = r0;
        if (out1) out1[i] = r1;
    }
}

template <int W>
int launch(const double* a, const double* b, const unsigned char* valid, double* out0, double* out1, size_t n,
           hipStream_t stream) {
    const unsigned blocks = (unsigned)((n + kLanes - 1) / kLanes);
    hipLaunchKernelGGL(probe_kernel<W>, dim3(blocks), dim3(kLanes), 0, stream, a, b, valid, out0, out1, n);
    return (int)hipGetLastError();
}

template <int W = 0>
int dispatch(int which, const double* a, const double* b, const unsigned char* valid, double* out0, double* out1,
             size_t n, hipStream_t stream) {
    if constexpr (W < kWhichCount) {
        if (which == W) return launch<W>(a, b, valid, out0, out1, n, stream);
        return dispatch<W + 1>(which, a, b, valid, out0, out1, n, stream);
    } else {
        return -1;
    }
}
}  // namespace

// a, out0: n doubles on the device; b, valid, out1: n entries or null (b reads as 0, valid as all set).
// Returns 0, a hipError_t of the launch, or -1 for an unknown form / a missing array / more than 2^20 inputs.
extern "C" __attribute__((visibility("default")))
int softrod_math_probe(int which, const double* a, const double* b, const unsigned char* valid, double* out0,
                       double* out1, size_t n, void* stream) {
    if (which < 0 || which >= kWhichCount || !a || !out0 || n > ((size_t)1 << 20)) return -1;
    if (n == 0) return 0;
    return dispatch(which, a, b, valid, out0, out1, n, (hipStream_t)stream);
}

extern "C" __attribute__((visibility("default"))) int softrod_math_probe_forms(void) { return kWhichCount; }
