// softrod_rod_probe.hip — two per-element blocks of the 3-D step kernels alone, on plain arrays: the rod-plane contact
// law plane_contact_n (softrod_contact.hpp) and the kinematic step kinematic_n (softrod_fast.hpp).
//
// A test-only library (variants/libsoftrod_rod_probe.so, `make probe`), like softrod_math_probe.hip one level down: it
// includes the shipped headers unchanged and is NOT one of the shipped library's sources, so libsoftrod_hip.so and its
// source hash do not know it exists.  tests/test_gpu_rod_probe.py compares what it returns with 50-digit references
// (tests/rod_probe_ref.py).
//
// One wave of 64 threads is one rod, one block per rod; slot j = lane * EPL + s of rod r is entry r * 64 * EPL + j of
// every array, components innermost.  The inputs hold all 64 * EPL slots of a rod, the ones behind it included (they are
// what the neighbour shifts and the sanitizer see); the outputs are stored for the rod's own nodes / elements only.
#include "../softrod_kernels.hpp"

namespace {
using namespace softrod;

enum ContactForm : int {
    kZup1 = 0,          // plane_contact_n<1, true, true, false>
    kZup2 = 1,          // <2, true, true, false>
    kZupTaper1 = 2,     // <1, true, true, true>
    kZupTaper2 = 3,     // <2, true, true, true>
    kPlane1 = 4,        // <1, false, true, false>
    kPlane2 = 5,        // <2, false, true, false>
    kLiteral1 = 6,      // <1, false, false, false>: the literal law, for comparison
    kContactForms = 7
};

// the law's scalar parameters, by value (wave-uniform: scalar registers, like RodParams in the step kernels)
struct ContactScalars {
    double k, nu, slip_tol, surface_tol;
    double kin_mu[3], stat_mu[3];
    double origin[3], normal[3];
    double r0_sqrt_rest_len;
    int n_elem;
};

struct ContactArrays {
    const double *x, *v, *Q, *w, *t, *len, *F, *tq, *mass, *r0s;
    double *fc, *tq_out;
};

template <int EPL, bool ZUP, bool FM, bool TAPER>
__global__ void __launch_bounds__(kLanes) contact_kernel(ContactScalars cs, ContactArrays a) {
    constexpr size_t W = (size_t)kLanes * EPL;
    const int lane = (int)threadIdx.x;
    const size_t base = (size_t)blockIdx.x * W + (size_t)lane * EPL;
    const int n = cs.n_elem;
    RodParams P{};
    P.n_envs = (int)gridDim.x;
    P.n_elem = n;
    P.contact_k = cs.k; P.contact_nu = cs.nu; P.slip_tol = cs.slip_tol; P.surface_tol = cs.surface_tol;
    P.r0_sqrt_rest_len = cs.r0_sqrt_rest_len;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        P.kin_mu[c] = cs.kin_mu[c]; P.stat_mu[c] = cs.stat_mu[c];
        P.plane_origin[c] = cs.origin[c]; P.plane_normal[c] = cs.normal[c];
    }
    const ContactParams CP = contact_params(P);          // the shipped means and half differences

    LaneN<EPL> L{};
    ConstN<EPL> K{};
    double len[EPL], F[EPL][3], tq[EPL][3], fc[EPL][3];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
        const int idx = slot_local(P, lane * EPL + s);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            L.x[s][c] = a.x[3 * j + c]; L.v[s][c] = a.v[3 * j + c];
            L.w[s][c] = a.w[3 * j + c]; L.t[s][c] = a.t[3 * j + c];
            F[s][c] = a.F[3 * j + c]; tq[s][c] = a.tq[3 * j + c];
            fc[s][c] = 0.0;
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) L.Q[s][c] = a.Q[9 * j + c];
        len[s] = a.len[j];
        // the mass fields as build_const_m forms them: zeros past the rod's end, 1 / (m_k + m_{k+1}) finite there
        const double mass = (idx <= n) ? a.mass[j] : 1.0;
        const double mass_next = (idx + 1 <= n) ? a.mass[j + 1] : 1.0;
        K.mass[s] = (idx <= n) ? mass : 0.0;
        K.mass_next[s] = (idx + 1 <= n) ? mass_next : 0.0;
        K.inv_mass_pair[s] = 1.0 / (mass + mass_next);
        if constexpr (TAPER) {
            K.r0s[s] = a.r0s[j];
            K.ir0s[s] = 1.0 / a.r0s[j];
        } else {
            K.r0s[s] = P.r0_sqrt_rest_len;
            K.ir0s[s] = 1.0 / P.r0_sqrt_rest_len;
        }
    }
    sanitize_unused_slots<EPL>(P, lane, L);              // the law's documented precondition (kernel entry)
    double xn[EPL][3], vn[EPL][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {                        // next-node position / velocity, as dynamic_n forms them
        double p[EPL], o[EPL], pv[EPL], ov[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) { p[s] = L.x[s][c]; pv[s] = L.v[s][c]; }
        shift_next<EPL>(p, o);
        shift_next<EPL>(pv, ov);
#pragma unroll
        for (int s = 0; s < EPL; ++s) { xn[s][c] = o[s]; vn[s][c] = ov[s]; }
    }
    plane_contact_n<EPL, ZUP, FM, TAPER>(CP, P, lane, K, L, xn, vn, len, F, tq, fc);
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
        const int idx = slot_local(P, lane * EPL + s);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (idx <= n) a.fc[3 * j + c] = fc[s][c];
            if (idx < n) a.tq_out[3 * j + c] = tq[s][c];
        }
    }
}

template <int EPL, bool ZUP, bool FM, bool TAPER>
int launch_contact(const ContactScalars& cs, const ContactArrays& a, int n_rods, hipStream_t stream) {
    hipLaunchKernelGGL((contact_kernel<EPL, ZUP, FM, TAPER>), dim3((unsigned)n_rods), dim3(kLanes), 0, stream, cs, a);
    return (int)hipGetLastError();
}

template <int EPL>
__global__ void __launch_bounds__(kLanes)
kinematic_kernel(double h, const double* __restrict__ x, const double* __restrict__ v, const double* __restrict__ Q,
                 const double* __restrict__ w, const double* __restrict__ hx, const double* __restrict__ hq,
                 double* __restrict__ x_out, double* __restrict__ Q_out) {
    constexpr size_t W = (size_t)kLanes * EPL;
    const size_t base = (size_t)blockIdx.x * W + (size_t)threadIdx.x * EPL;
    LaneN<EPL> L{};
    ConstN<EPL> C{};
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            L.x[s][c] = x[3 * j + c]; L.v[s][c] = v[3 * j + c]; L.w[s][c] = w[3 * j + c];
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) L.Q[s][c] = Q[9 * j + c];
        C.hx[s] = hx[j];
        C.hq[s] = hq[j];
    }
    kinematic_n<EPL>(h, C, L);
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const size_t j = base + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) x_out[3 * j + c] = L.x[s][c];
#pragma unroll
        for (int c = 0; c < 9; ++c) Q_out[9 * j + c] = L.Q[s][c];
    }
}

constexpr int kMaxRods = 1024;
}  // namespace

// form: a ContactForm.  par: 17 doubles ON THE HOST — k, nu, slip_tol, surface_tol, kinetic mu
// (forward, backward, sideways), static mu, plane origin, plane normal, r0 sqrt(l_rest) of a uniform rod.  Device arrays
// of n_rods * 64 * EPL slots: x, v, F (nodes), w, t, tq (elements) with 3 components, Q with 9, len, mass, r0s (tapered
// forms only; else ignored) with one.  fc: the contact force per node (slots 0 .. n_elem); tq_out: tq with the law's
// torque added, per element (slots 0 .. n_elem - 1); the other slots are not written.
// Returns 0, the launch's hipError_t, or -1 for bad arguments: an unknown form, a missing array, n_rods outside
// 1 .. 1024, a rod that does not fit (n_elem + 1 > 64 * EPL) or has no element, a z-up form with another normal.
extern "C" __attribute__((visibility("default")))
int softrod_rod_probe_contact(int form, int n_rods, int n_elem, const double* par, const double* x, const double* v,
                              const double* Q, const double* w, const double* t, const double* len, const double* F,
                              const double* tq, const double* mass, const double* r0s, double* fc, double* tq_out,
                              void* stream) {
    if (form < 0 || form >= kContactForms || !par || !x || !v || !Q || !w || !t || !len || !F || !tq || !mass || !fc ||
        !tq_out || n_rods < 1 || n_rods > kMaxRods)
        return -1;
    const int epl = (form == kZup2 || form == kZupTaper2 || form == kPlane2) ? 2 : 1;
    const bool zup = form <= kZupTaper2, taper = (form == kZupTaper1 || form == kZupTaper2);
    if (n_elem < 1 || n_elem + 1 > kLanes * epl) return -1;
    if (taper && !r0s) return -1;
    ContactScalars cs;
    cs.k = par[0]; cs.nu = par[1]; cs.slip_tol = par[2]; cs.surface_tol = par[3];
    for (int c = 0; c < 3; ++c) {
        cs.kin_mu[c] = par[4 + c]; cs.stat_mu[c] = par[7 + c];
        cs.origin[c] = par[10 + c]; cs.normal[c] = par[13 + c];
    }
    cs.r0_sqrt_rest_len = par[16];
    cs.n_elem = n_elem;
    if (zup && !(cs.normal[0] == 0.0 && cs.normal[1] == 0.0 && cs.normal[2] == 1.0)) return -1;
    const ContactArrays a{x, v, Q, w, t, len, F, tq, mass, r0s, fc, tq_out};
    hipStream_t st = (hipStream_t)stream;
    switch (form) {
        case kZup1: return launch_contact<1, true, true, false>(cs, a, n_rods, st);
        case kZup2: return launch_contact<2, true, true, false>(cs, a, n_rods, st);
        case kZupTaper1: return launch_contact<1, true, true, true>(cs, a, n_rods, st);
        case kZupTaper2: return launch_contact<2, true, true, true>(cs, a, n_rods, st);
        case kPlane1: return launch_contact<1, false, true, false>(cs, a, n_rods, st);
        case kPlane2: return launch_contact<2, false, true, false>(cs, a, n_rods, st);
        default: return launch_contact<1, false, false, false>(cs, a, n_rods, st);
    }
}

// kinematic_n<epl>(h, C, L) with C.hx / C.hq from the arrays: n_waves * 64 * epl slots each of x, v, w (3 components),
// Q (9), hx, hq (1); every slot's x and Q are stored.  Returns 0, the launch's hipError_t, or -1 for bad arguments.
extern "C" __attribute__((visibility("default")))
int softrod_rod_probe_kinematic(int epl, int n_waves, double h, const double* x, const double* v, const double* Q,
                                const double* w, const double* hx, const double* hq, double* x_out, double* Q_out,
                                void* stream) {
    if ((epl != 1 && epl != 2) || n_waves < 1 || n_waves > kMaxRods || !x || !v || !Q || !w || !hx || !hq || !x_out ||
        !Q_out)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    if (epl == 1)
        hipLaunchKernelGGL(kinematic_kernel<1>, dim3((unsigned)n_waves), dim3(kLanes), 0, st, h, x, v, Q, w, hx, hq,
                           x_out, Q_out);
    else
        hipLaunchKernelGGL(kinematic_kernel<2>, dim3((unsigned)n_waves), dim3(kLanes), 0, st, h, x, v, Q, w, hx, hq,
                           x_out, Q_out);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int softrod_rod_probe_forms(void) { return kContactForms; }
