"""fast_rsqrt (softrod_kernels.hpp) takes its third-order correction in five fp64 operations behind the v_rsq_f64 seed
instead of six: the two halvings of

    e  = fma(-(0.5 x) r, r, 0.5);   r' = fma(r, e fma(1.5, e, 1.0), r)

are folded into constants,

    E  = fma(-(x r), r, 1.0);       r' = fma(r, E fma(E, 0.375, 0.5), r)       (E = 2 e, fma(E, 0.375, 0.5) = fma(1.5, e, 1.0) / 2)

Scaling by a power of two commutes with rounding while nothing is subnormal, so the result is the same BITS.  This test
holds that: a stand-alone C++ program (host compiler, -ffp-contract=off, std::fma) evaluates both forms from the SAME
seed — the correctly rounded 1/sqrt(x), and that seed perturbed by up to 2^-20 relative, well past the hardware seed's
2^-23 — and demands zero differing bit patterns.

Inputs: x log-uniform over [1e-20, 1e6] (the planar loop's range: |d|^2 is clamped from below at 1e-20), the clamp value
itself, every power of two from 2^-66 to 2^20, and log-uniform over [1e-300, 1e300] (the contact law and the rigid head
clamp at 1e-300).  The one place where the two forms can part is a SUBNORMAL x (0.5 x rounds there, x r does not):
below 2.2e-308, which no caller reaches behind its clamp.

fast_rcp (three operations), the Horner polynomials of sinc_cosc / exp_pair / exp_one and theta_over_sin's series hold
no power-of-two scaling to fold; nothing else was rewritten.
"""
import shutil
import subprocess

import pytest

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static double old_form(double x, double r) {
    const double e = std::fma(-(0.5 * x) * r, r, 0.5);
    return std::fma(r, e * std::fma(1.5, e, 1.0), r);
}
static double new_form(double x, double r) {
    const double E = std::fma(-(x * r), r, 1.0);
    return std::fma(r, E * std::fma(E, 0.375, 0.5), r);
}
static uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {            // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uniform01() { return (double)(next_u64() >> 11) * 0x1.0p-53; }

static long checked = 0, differing = 0;
static void check_seed(double x, double r) {
    const double a = old_form(x, r), b = new_form(x, r);
    ++checked;
    if (bits(a) != bits(b)) {
        if (differing < 10) std::printf("x = %a  seed = %a: old %a  new %a\n", x, r, a, b);
        ++differing;
    }
}
static void check(double x) {
    const double exact = (double)(1.0L / sqrtl((long double)x));
    check_seed(x, exact);
    // the hardware seed is good to 2^-23; up to 2^-20 either way here, at fixed and at random sizes
    const double fixed[] = {0x1.0p-20, -0x1.0p-20, 0x1.0p-23, -0x1.0p-23, 0x1.0p-30, -0x1.0p-30, 0x1.0p-52, -0x1.0p-52};
    for (double d : fixed) check_seed(x, exact * (1.0 + d));
    for (int i = 0; i < 3; ++i) check_seed(x, exact * (1.0 + (2.0 * uniform01() - 1.0) * 0x1.0p-20));
    check_seed(x, std::nextafter(exact, 0.0));
    check_seed(x, std::nextafter(exact, 2.0 * exact));
}

int main() {
    const long n = 1000000;
    for (long i = 0; i < n; ++i) check(std::pow(10.0, -20.0 + 26.0 * uniform01()));          // [1e-20, 1e6]
    for (long i = 0; i < n / 4; ++i) check(std::pow(10.0, -300.0 + 600.0 * uniform01()));    // [1e-300, 1e300]
    check(1.0e-20);
    check(1.0e-300);
    check(1.0e6);
    for (int k = -66; k <= 20; ++k) {
        const double p = std::ldexp(1.0, k);
        check(p);
        check(std::nextafter(p, 0.0));
        check(std::nextafter(p, 2.0 * p));
    }
    std::printf("checked %ld (x, seed) pairs, %ld differing bit patterns\n", checked, differing);
    return differing == 0 ? 0 : 1;
}
"""


def test_five_operation_rsqrt_correction_is_bit_identical(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "rsqrt_rewrite.cpp", tmp_path / "rsqrt_rewrite"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), str(src)], check=True)
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "0 differing bit patterns" in p.stdout
