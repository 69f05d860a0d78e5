// softrod_dyn_probe.hip — ONE force evaluation and rate update of the FAST step kernels alone, on plain arrays: dynamic_n
// (softrod_fast.hpp: shear/stretch stress, the bend/twist log map, Voronoi couples, kappa x B kappa, shear couple,
// transport, unsteady dilatation, rate update, fused damper) and planar_dynamic_n (softrod_planar.hpp: the same substep
// of the SoftPendulum rod with the zeros removed).
//
// A test-only library (variants/libsoftrod_dyn_probe.so, `make probe`), the third of its kind after
// softrod_math_probe.hip and softrod_rod_probe.hip: it includes the shipped headers unchanged and is NOT one of the
// shipped library's sources, so libsoftrod_hip.so and its source hash do not know it exists.
// tests/test_gpu_dyn_probe.py compares what it returns with 50-digit references (tests/dyn_probe_ref.py).
//
// One wave of 64 threads is one rod, one block per rod; slot j = lane * EPL + s of rod r is entry r * 64 * EPL + j of
// every array, components innermost.  The inputs hold all 64 * EPL slots of a rod, the ones behind it included (they are
// what the neighbour shifts and the sanitizer see); the outputs are stored for the rod's own nodes / elements /
// vertices only.  ConstN comes from the shipped build_const (PlanarC from planar_build_const), so the folded constants
// cf, ca, cw, s, b, bd (cfy, cwl, bk, bke, xl, jr) are the shipped ones.
#include "../softrod_kernels.hpp"

namespace {
using namespace softrod;

// (softrod_capi.hip's name for the compiled mask of the 100-element arm benchmark)
constexpr unsigned kArmSingleZup = SOFTROD_FEATURES_ARM_SINGLE | kFeatPlaneZup;

enum DynForm : int {
    kRuntime1 = 0,      // dynamic_n<kRuntimeFeatures, 1>, the mask from the parameter block
    kRuntime2 = 1,      // <kRuntimeFeatures, 2>
    kRuntimeTaper1 = 2, // <kRuntimeFeatures, 1, true>
    kArm1 = 3,          // <kArmSingleZup, 1>
    kArm2 = 4,          // <kArmSingleZup, 2>
    kArmTaper1 = 5,     // <kArmSingleZup, 1, true>
    kDynForms = 6
};

// the host parameter block, in doubles
enum Par : int {
    kDt = 0, kRestLen, kInvRestLen, kRestVor, kInvRestVor,
    kJ, kInvJ = kJ + 3, kShear = kInvJ + 3, kBend = kShear + 3, kMassNode = kBend + 3,
    kGravity, kDampT = kGravity + 3, kDampR, kDampLogR = kDampR + 3,
    kEpsLength = kDampLogR + 3, kAcosShift, kEpsSin, kFeatures,
    kPlaneOrigin, kPlaneNormal = kPlaneOrigin + 3, kContactK = kPlaneNormal + 3, kContactNu, kSlipTol, kSurfaceTol,
    kKinMu, kStatMu = kKinMu + 3, kR0SqrtRestLen = kStatMu + 3, kPointForce, kParams
};

RodParams rod_params(const double* par, int n_rods, int n_elem, unsigned features) {
    RodParams P{};
    P.n_envs = n_rods;
    P.n_elem = n_elem;
    P.features = features;
    P.dt = par[kDt]; P.half_dt = 0.5 * par[kDt];
    P.rest_len = par[kRestLen]; P.inv_rest_len = par[kInvRestLen];
    P.rest_vor = par[kRestVor]; P.inv_rest_vor = par[kInvRestVor];
    for (int c = 0; c < 3; ++c) {
        P.J[c] = par[kJ + c]; P.invJ[c] = par[kInvJ + c];
        P.shear[c] = par[kShear + c]; P.bend[c] = par[kBend + c];
        P.gravity[c] = par[kGravity + c];
        P.damp_r[c] = par[kDampR + c]; P.damp_logr[c] = par[kDampLogR + c];
        P.plane_origin[c] = par[kPlaneOrigin + c]; P.plane_normal[c] = par[kPlaneNormal + c];
        P.kin_mu[c] = par[kKinMu + c]; P.stat_mu[c] = par[kStatMu + c];
    }
    P.mass_node = par[kMassNode];
    P.mass_total = par[kMassNode] * n_elem;
    P.damp_t = par[kDampT];
    P.eps_length = par[kEpsLength]; P.acos_shift = par[kAcosShift]; P.eps_sin = par[kEpsSin];
    P.two_acos_shift = 2.0 * par[kAcosShift] + 1.0e-200;      // (fill_params' operations)
    P.neg_eps_sin = -par[kEpsSin];
    P.contact_k = par[kContactK]; P.contact_nu = par[kContactNu];
    P.slip_tol = par[kSlipTol]; P.surface_tol = par[kSurfaceTol];
    P.r0_sqrt_rest_len = par[kR0SqrtRestLen];
    return P;
}

struct DynArrays {
    const double *x, *v, *Q, *w, *rk, *mat;
    double *v_out, *w_out, *t_out, *kap_out;
};

template <unsigned F, int EPL, bool TAPER>
__global__ void __launch_bounds__(kLanes) dynamic_kernel(RodParams P, double force, DynArrays a) {
    constexpr size_t W = (size_t)kLanes * EPL;
    const int lane = (int)threadIdx.x;
    const size_t base = (size_t)blockIdx.x * W + (size_t)lane * EPL;
    const int n = P.n_elem;
    LaneN<EPL> L{};
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            L.x[s][c] = a.x[3 * j + c]; L.v[s][c] = a.v[3 * j + c];
            L.w[s][c] = a.w[3 * j + c]; L.rk[s][c] = a.rk[3 * j + c];
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) L.Q[s][c] = a.Q[9 * j + c];
    }
    // as at the entry of the contact kernels; the shipped kernels of the other masks do not run it (softrod_fast.hpp), so
    // what this probe shows about the slots behind the rod holds for rods that have passed it
    sanitize_unused_slots<EPL>(P, lane, L);
    ConstN<EPL> C{};
    EnvAction A{};
    A.force = force;                                     // (read under SOFTROD_FEAT_POINT_FORCE_NODE0_X only)
    build_const<F, EPL, TAPER>(P, lane, A, C, a.mat);
    BcTargets B{};                                       // no BC, sucker or Laplace feature in these forms
    RodParams Pk = P;
    if (!has<F>(P, SOFTROD_FEAT_ANALYTICAL_DAMPER)) Pk.damp_t = 1.0;
    dynamic_n<F, EPL, TAPER>(Pk, C, B, lane, L);
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
        const int idx = lane * EPL + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (idx <= n) a.v_out[3 * j + c] = L.v[s][c];
            if (idx < n) { a.w_out[3 * j + c] = L.w[s][c]; a.t_out[3 * j + c] = L.t[s][c]; }
            if (idx < n - 1) a.kap_out[3 * j + c] = L.kap[s][c];
        }
    }
}

template <unsigned F, int EPL, bool TAPER>
int launch_dynamic(const RodParams& P, double force, const DynArrays& a, int n_rods, hipStream_t stream) {
    hipLaunchKernelGGL((dynamic_kernel<F, EPL, TAPER>), dim3((unsigned)n_rods), dim3(kLanes), 0, stream, P, force, a);
    return (int)hipGetLastError();
}

struct PlanarArrays {
    const double *x, *v, *c, *s, *wz, *dl, *d, *dv;
    double *v_out, *wz_out, *t_out, *dv_out;
};

template <int EPL>
__global__ void __launch_bounds__(kLanes) planar_kernel(RodParams P, double s2, double force, PlanarArrays a) {
    constexpr size_t W = (size_t)kLanes * EPL;
    const int lane = (int)threadIdx.x;
    const size_t base = (size_t)blockIdx.x * W + (size_t)lane * EPL;
    const int n = P.n_elem;
    ConstN<EPL> C{};
    EnvAction A{};
    A.force = force;
    build_const<SOFTROD_FEATURES_SOFTPENDULUM, EPL>(P, lane, A, C);
    PlanarC<EPL> K;
    planar_build_const<EPL>(P, C, lane, K);
    PlanarN<EPL> Z;
    Z.s2 = s2;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            Z.x[s][c] = a.x[2 * j + c]; Z.v[s][c] = a.v[2 * j + c];
            Z.d[s][c] = a.d[2 * j + c]; Z.dv[s][c] = a.dv[2 * j + c];
            Z.t[s][c] = 0.0;
        }
        Z.c[s] = a.c[j]; Z.s[s] = a.s[j]; Z.wz[s] = a.wz[j]; Z.dl[s] = a.dl[j];
    }
    planar_sanitize_unused<EPL>(P, lane, Z);             // as planar_from_lane leaves the state
    planar_dynamic_n<EPL>(P, C, K, lane, Z);
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
        const int idx = lane * EPL + s;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (idx <= n) a.v_out[2 * j + c] = Z.v[s][c];
            if (idx < n) { a.t_out[2 * j + c] = Z.t[s][c]; a.dv_out[2 * j + c] = Z.dv[s][c]; }
        }
        if (idx < n) a.wz_out[j] = Z.wz[s];
    }
}

constexpr int kMaxRods = 1024;
}  // namespace

// form: a DynForm.  par: kParams (50) doubles ON THE HOST, in the order of enum Par — dt, rest_len, 1 / rest_len,
// rest_vor, 1 / rest_vor, J, 1 / J, shear, bend (3 each), the interior node mass, gravity (3), exp(-nu dt), damp_r (3),
// damp_logr (3), eps_length, acos_shift, eps_sin, the run-time feature mask (as a double; the compiled forms ignore it),
// plane origin, plane normal, contact k, nu, slip_tol, surface_tol, kinetic mu, static mu (3 each), r0 sqrt(l_rest),
// the point force on node 0 (EnvAction.force).  Device arrays of n_rods * 64 * EPL slots: x, v (nodes), w
// (elements), rk (vertices) with 3 components, Q with 9.  mat: the tapered forms' material table [16 rows][64 * EPL] in
// build_const_m's layout, shared by all rods (else ignored).  Outputs: v (slots 0 .. n_elem), w and t (0 .. n_elem - 1),
// kap (0 .. n_elem - 2); the other slots are not written.
// Returns 0, the launch's hipError_t, or -1 for bad arguments: an unknown form, a missing array, n_rods outside
// 1 .. 1024, n_elem < 2, a rod that does not fit (n_elem + 1 > 64 * EPL), a z-up form with another normal.
extern "C" __attribute__((visibility("default")))
int softrod_dyn_probe_dynamic(int form, int n_rods, int n_elem, const double* par, const double* x, const double* v,
                              const double* Q, const double* w, const double* rk, const double* mat, double* v_out,
                              double* w_out, double* t_out, double* kap_out, void* stream) {
    if (form < 0 || form >= kDynForms || !par || !x || !v || !Q || !w || !rk || !v_out || !w_out || !t_out || !kap_out ||
        n_rods < 1 || n_rods > kMaxRods)
        return -1;
    const int epl = (form == kRuntime2 || form == kArm2) ? 2 : 1;
    const bool taper = (form == kRuntimeTaper1 || form == kArmTaper1), arm = form >= kArm1;
    if (n_elem < 2 || n_elem + 1 > kLanes * epl) return -1;
    if (taper && !mat) return -1;
    const unsigned features = arm ? kArmSingleZup : (unsigned)par[kFeatures];
    const RodParams P = rod_params(par, n_rods, n_elem, features);
    if (arm && !(P.plane_normal[0] == 0.0 && P.plane_normal[1] == 0.0 && P.plane_normal[2] == 1.0)) return -1;
    const DynArrays a{x, v, Q, w, rk, mat, v_out, w_out, t_out, kap_out};
    hipStream_t st = (hipStream_t)stream;
    switch (form) {
        case kRuntime1: return launch_dynamic<kRuntimeFeatures, 1, false>(P, par[kPointForce], a, n_rods, st);
        case kRuntime2: return launch_dynamic<kRuntimeFeatures, 2, false>(P, par[kPointForce], a, n_rods, st);
        case kRuntimeTaper1: return launch_dynamic<kRuntimeFeatures, 1, true>(P, par[kPointForce], a, n_rods, st);
        case kArm1: return launch_dynamic<kArmSingleZup, 1, false>(P, par[kPointForce], a, n_rods, st);
        case kArm2: return launch_dynamic<kArmSingleZup, 2, false>(P, par[kPointForce], a, n_rods, st);
        default: return launch_dynamic<kArmSingleZup, 1, true>(P, par[kPointForce], a, n_rods, st);
    }
}

// build_const<SOFTROD_FEATURES_SOFTPENDULUM, epl>, planar_build_const<epl>, one planar_dynamic_n<epl>.  par as above.
// Device arrays of n_rods * 64 * epl slots: x, v (nodes), d, dv (elements) with 2 components, c, s, wz (elements), dl
// (vertices) with one; s2 = +-1.  Outputs: v (slots 0 .. n_elem), wz, t, dv (0 .. n_elem - 1).
// Returns 0, the launch's hipError_t, or -1 for bad arguments (as above; epl other than 1 or 2).
extern "C" __attribute__((visibility("default")))
int softrod_dyn_probe_planar(int epl, int n_rods, int n_elem, const double* par, const double* x, const double* v,
                             const double* c, const double* s, const double* wz, const double* dl, const double* d,
                             const double* dv, double s2, double* v_out, double* wz_out, double* t_out, double* dv_out,
                             void* stream) {
    if ((epl != 1 && epl != 2) || !par || !x || !v || !c || !s || !wz || !dl || !d || !dv || !v_out || !wz_out || !t_out ||
        !dv_out || n_rods < 1 || n_rods > kMaxRods)
        return -1;
    if (n_elem < 2 || n_elem + 1 > kLanes * epl) return -1;
    const RodParams P = rod_params(par, n_rods, n_elem, SOFTROD_FEATURES_SOFTPENDULUM);
    const PlanarArrays a{x, v, c, s, wz, dl, d, dv, v_out, wz_out, t_out, dv_out};
    hipStream_t st = (hipStream_t)stream;
    if (epl == 1)
        hipLaunchKernelGGL(planar_kernel<1>, dim3((unsigned)n_rods), dim3(kLanes), 0, st, P, s2, par[kPointForce], a);
    else
        hipLaunchKernelGGL(planar_kernel<2>, dim3((unsigned)n_rods), dim3(kLanes), 0, st, P, s2, par[kPointForce], a);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int softrod_dyn_probe_forms(void) { return kDynForms; }
extern "C" __attribute__((visibility("default"))) int softrod_dyn_probe_params(void) { return kParams; }
