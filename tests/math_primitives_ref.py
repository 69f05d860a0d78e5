"""References, inputs and budgets for the SOFTROD_MATH_FAST device primitives (softrod_kernels.hpp fast_rcp / fast_rsqrt,
softrod_fast.hpp sinc_cosc / theta_over_sin / eps_sin_factor / exp_pair / exp_wide_pair, softrod_planar.hpp exp_one and
the planar rotation), shared by tests/test_math_primitives.py (CPU) and tests/test_gpu_math_primitives.py (the device,
through csrc/probe/softrod_math_probe.hip).

Three things live here:

  * the references: each operation in mpmath at 50 digits, evaluated at the fp64 input exactly as given;
  * a NumPy fp64 transcription of each primitive's operation sequence, wave by wave (64 consecutive inputs share the
    range checks, like on the device), every fma written as a product and a sum — two roundings, so a budget the
    transcription meets is one the device's single-rounding fma can meet.  fast_rcp / fast_rsqrt are the exception:
    their residual 1 - x r is a cancellation that only exists with an fma, so they take an exactly rounded one
    (rational arithmetic), from an emulated 24-bit seed here and from the device's own seed in the GPU test.
    `single_rounding()` runs every transcription that way: the device's sequence operation by operation, which the
    GPU test compares bit for bit;
  * the cases: inputs in waves of 64 from one tier each, with the thresholds' neighbours and the tier's upper edge,
    at most 4096 values a case, and the budget each value is held to.

BUDGETS.  1 ulp = 2^-52 relative to the reference (absolute where stated).  They come from the arithmetic:

  fast_rcp, fast_rsqrt    1 ulp: third-order correction of a seed good to 2^-20 leaves 2^-60 before the last rounding
  theta_over_sin_series   2 ulp: last fma 1/2, the Horner chain below it y/(1-y)/2, the remainder c_K y^K/(1-y) —
                          0.37 ulp (8.3e-17) at the first tier's edge, 0.02 and 0.035 at the other two
  theta_over_sin beyond   4 ulp: two refined 1/sqrt (1 ulp each), their product, the series, the last product
  sinc_cosc in range      1 ulp: last fma 1/2, chain t/12, remainder t^4/9! < 3e-18
  sinc_cosc k quarterings absolute 2 (k + 2) ulp on both outputs: each double-angle step adds at most two roundings
                          of values <= 1 to an error it does not amplify (|d sin 2p| <= 2 |d sin p| is paid for by
                          sinc = sin / th halving with it)
  eps_sin_factor          2^-22 |ref - 1| + 1 ulp: the raw seed by design
  exp_pair, exp_wide_pair 2 ulp: last fma 1/2 (1/2 to 0.72 relative for results below 1), chain |x|/2, argument
                          reduction 1/8, remainder
  exp_one, k halvings     2^k ulp: each squaring doubles the relative error
  planar rotation         absolute 2 ulp on cos and sin in range, 2 (k + 2) beyond (up to a = 10, k = 9: cos = 1 - cosc t
                          carries cosc's error times t, and the two-rounding transcription reaches 22.02 of 22
                          there; in single-rounding fmas, and on the device, it is 18.9)

EDGE BIAS.  In three tiers the polynomial's LAST term is itself below those budgets — the series were cut where the
remainder drops under a rounding: c_11 y^11 = 0.49 ulp at y = 0.04, c_19 y^19 = 0.20 ulp at 0.15, x^8/8! = 0.73 ulp at
|x| = 0.04.  No bound on the LARGEST error can see such a term go: the last rounding alone is half an ulp either way.
But a missing term is systematic where a rounding is not.  So these tiers carry 512 values in the top 2 % of their
range, and the MEAN signed error over them is held to

    what the truncation legitimately leaves there (c_K y^K/(1-y): 0.02 and 0.035 ulp; x^9/9!: 0.004) + 0.1 ulp.

The 0.1: 512 last roundings, each uniform over +-1/2 ulp, have a mean of standard deviation 0.29/sqrt(512) = 0.013; the
roundings below the last reach the result through a factor |x| <= 0.15 and are as unbiased.  0.1 is eight deviations;
the dropped terms shift the mean by 0.44, 0.17 and 0.67.  (`Case.bias_edge`, `Case.bias_budget`, edge_bias().)
"""
from __future__ import annotations

import contextlib
import functools
from dataclasses import dataclass, field
from fractions import Fraction

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50
ULP = 2.0 ** -52
WAVE = 64
MAX_VALUES = 4096

# probe form ids (csrc/probe/softrod_math_probe.hip, enum Which)
FAST_RCP, FAST_RSQRT, SEED_RCP, SEED_RSQ = 0, 1, 2, 3
SINC_LEAN, SINC_PLAIN = 4, 5
SERIES6, SERIES12, SERIES20 = 6, 7, 8
THETA, THETA_BATCHED = 9, 10
EPS_SIN, EXP_PAIR, EXP_WIDE, EXP_ONE, PLANAR = 11, 12, 13, 14, 15
N_FORMS = 16

THETA_EDGES = (2.5e-3, 0.04, 0.15)     # theta_over_sin's tiers: y < edge
SINC_EDGE = 1.0e-3                     # sinc_cosc / the planar rotation: t < edge
EXP_EDGES = (1.0e-3, 0.04)             # exp_pair: max |x| < edge;  exp_one: the first only
EPS = 1.0e-14                          # softrod_config.eps_sin


# ---------------------------------------------------------------------------------------------------------------
# references, 50 digits
# ---------------------------------------------------------------------------------------------------------------
def _mpf(v):
    return MP.mpf(float(v))


def ref_rcp(x):
    return [1 / _mpf(v) for v in x]


def ref_rsqrt(x):
    return [1 / MP.sqrt(_mpf(v)) for v in x]


def ref_theta_over_sin(y):
    """theta / sin(theta) with y = sin^2(theta / 2): asin(sqrt y) / (sqrt y sqrt(1 - y))."""
    out = []
    for v in y:
        v = _mpf(v)
        if v == 0:
            out.append(MP.mpf(1))
        else:
            s = MP.sqrt(v)
            out.append(MP.asin(s) / (s * MP.sqrt(1 - v)))
    return out


def ref_sinc_cosc(t):
    """sin(th) / th and (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2 from t = th^2."""
    sc, cc = [], []
    for v in t:
        v = _mpf(v)
        if v == 0:
            sc.append(MP.mpf(1))
            cc.append(MP.mpf(1) / 2)
        else:
            th = MP.sqrt(v)
            sc.append(MP.sin(th) / th)
            cc.append(2 * MP.sin(th / 2) ** 2 / v)
    return sc, cc


def ref_eps_sin_factor(y, eps):
    """1 - d cot(theta), cot(theta) = (1 - 2 y) / (2 sqrt(y (1 - y)))."""
    out = []
    for v, d in zip(y, eps):
        v, d = _mpf(v), _mpf(d)
        out.append(1 - d * (1 - 2 * v) / (2 * MP.sqrt(v * (1 - v))))
    return out


def ref_exp(x):
    return [MP.exp(_mpf(v)) for v in x]


def ref_cos_sin(a):
    return [MP.cos(_mpf(v)) for v in a], [MP.sin(_mpf(v)) for v in a]


def err_ulps(got, ref, absolute=False):
    """|got - ref| in units of 2^-52 (times |ref| unless absolute), per element; inf where got is not finite."""
    out = np.empty(len(ref))
    for i, (g, r) in enumerate(zip(got, ref)):
        if not np.isfinite(g):
            out[i] = np.inf
            continue
        e = abs(_mpf(g) - r)
        out[i] = float(e / ULP) if absolute else float(e / abs(r) / ULP)
    return out


def signed_err_ulps(got, ref):
    return np.array([float((_mpf(g) - r) / abs(r) / ULP) for g, r in zip(got, ref)])


# ---------------------------------------------------------------------------------------------------------------
# NumPy transcriptions
# ---------------------------------------------------------------------------------------------------------------
def fma_plain(a, b, c):
    return a * b + c


def fma_exact(a, b, c):
    """a b + c with ONE rounding (rationals; float() of a Fraction rounds to nearest even).  Finite inputs."""
    a, b, c = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(c, float))
    out = np.empty(a.shape)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


FMA = fma_plain      # what the transcriptions' Horner chains and double-angle steps use (see single_rounding)


@contextlib.contextmanager
def single_rounding():
    """The transcriptions with the device's single-rounding fma (rationals: slow, for a thousand values)."""
    global FMA
    FMA = fma_exact
    try:
        yield
    finally:
        FMA = fma_plain


def seed24(v):
    """v rounded to 24 significant bits: a stand-in for the v_rcp_f64 / v_rsq_f64 seeds (good to 2^-23)."""
    m, e = np.frexp(v)
    return np.ldexp(np.round(m * 2.0 ** 24) / 2.0 ** 24, e)


def _mutate(coefs, tag, mut):
    """mut = (tag, 'drop_last') | (tag, 'scale', index, factor) | (tag, 'replace', index, value); index counts from
    the highest-degree coefficient, the order the Horner chain takes them in."""
    coefs = list(coefs)
    if mut is None or mut[0] != tag:
        return coefs
    if mut[1] == "drop_last":
        return coefs[1:]
    if mut[1] == "scale":
        coefs[mut[2]] *= mut[3]
        return coefs
    if mut[1] == "replace":
        coefs[mut[2]] = mut[3]
        return coefs
    raise ValueError(mut)


def horner(coefs, x, tag=None, mut=None):
    """((c0 x + c1) x + c2) ... : the device's chain of fmas, each as a product and a sum."""
    c = _mutate(coefs, tag, mut)
    p = np.full_like(x, c[0])
    for ck in c[1:]:
        p = FMA(p, x, ck)
    return p


def _waves(*arrays):
    """Pads to a multiple of 64 with the last element (what the probe's idle lanes hold) -> (n, [(waves, 64) ...])."""
    n = len(arrays[0])
    pad = (-n) % WAVE
    out = []
    for a in arrays:
        a = np.asarray(a)
        if pad:
            a = np.concatenate([a, np.repeat(a[-1:], pad)])
        out.append(a.reshape(-1, WAVE).copy())
    return n, out


def t_fast_rcp(x, seed=None, fma=fma_exact, mut=None):
    x = np.asarray(x, float)
    r = seed24(1.0 / x) if seed is None else seed
    e = fma(-x, r, 1.0)
    corr = e if (mut and mut[0] == "rcp") else fma(e, e, e)
    return fma(r, corr, r)


def t_fast_rsqrt(x, seed=None, fma=fma_exact, mut=None):
    x = np.asarray(x, float)
    r = seed24(1.0 / np.sqrt(x)) if seed is None else seed
    E = fma(-(x * r), r, 1.0)
    g = 0.5 if (mut and mut[0] == "rsqrt") else fma(E, 0.375, 0.5)
    return fma(r, E * g, r)


SINC_S = (-1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0)
SINC_C = (-1.0 / 40320.0, 1.0 / 720.0, -1.0 / 24.0, 0.5)


def sinc_quarterings(t_wave):
    """k of sinc_cosc for one wave (0: in range)."""
    with np.errstate(invalid="ignore"):
        t = np.array(t_wave, float)
        k = 0
        while np.any(t >= SINC_EDGE) and k < 16:
            t *= 0.25
            k += 1
    return k


def t_sinc_cosc(t, mut=None):
    n, (T,) = _waves(np.asarray(t, float))
    sc, cc = np.empty_like(T), np.empty_like(T)
    with np.errstate(all="ignore"):
        for w in range(len(T)):
            tw = T[w]
            if not np.any(tw >= SINC_EDGE):
                sc[w] = horner(SINC_S, tw, "sinc.sc", mut)
                cc[w] = horner(SINC_C, tw, "sinc.cc", mut)
                continue
            k = 0
            while np.any(tw >= SINC_EDGE) and k < 16:
                tw = tw * 0.25
                k += 1
            s = horner(SINC_S, tw, "sinc.sc.cold", mut)
            c_ = horner(SINC_C, tw, "sinc.cc.cold", mut)
            for _ in range(k):
                c = FMA(-c_, tw, 1.0)
                c_ = 0.5 * s * s
                s = s * c
                tw = tw * 4.0
            sc[w], cc[w] = s, c_
    return sc.ravel()[:n], cc.ravel()[:n]


@functools.lru_cache(maxsize=None)
def series_coefs(K):
    """c_k = (2k)!!/(2k+1)!! by the header's recurrence, highest degree first, c_0 = 1 last."""
    c = [1.0]
    for k in range(1, K):
        c.append(c[k - 1] * float(2 * k) / float(2 * k + 1))
    return tuple(reversed(c))


def t_series(K, y, mut=None):
    return horner(series_coefs(K), np.asarray(y, float), f"series{K}", mut)


def theta_tier(y_wave, valid_wave):
    """0, 1, 2: the series of 6, 12, 20 terms; 3: the half-angle steps."""
    with np.errstate(invalid="ignore"):
        for tier, edge in enumerate(THETA_EDGES):
            if not np.any(~(y_wave < edge) & valid_wave):
                return tier
    return 3


def t_theta_over_sin(y, valid=None, mut=None):
    y = np.asarray(y, float)
    valid = np.ones(len(y), bool) if valid is None else np.asarray(valid).astype(bool)
    n, (Y, V) = _waves(y, valid)
    out = np.empty_like(Y)
    with np.errstate(all="ignore"):
        for w in range(len(Y)):
            tier = theta_tier(Y[w], V[w])
            if tier < 3:
                out[w] = t_series((6, 12, 20)[tier], Y[w], mut)
                continue
            om0 = np.fmax(1.0 - Y[w], 1.0e-300)
            r0 = t_fast_rsqrt(om0, fma=FMA)
            y1 = FMA(-0.5 * om0, r0, 0.5)
            om1 = 1.0 - y1
            r1 = t_fast_rsqrt(om1, fma=FMA)
            y2 = FMA(-0.5 * om1, r1, 0.5)
            out[w] = t_series(20, y2, mut) * (r0 * r1)
    return out.ravel()[:n]


def t_eps_sin_factor(y, eps):
    y, eps = np.asarray(y, float), np.asarray(eps, float)
    rho = seed24(1.0 / np.sqrt(np.fmax(-y * y + y, 1.0e-300)))
    return (y * eps + (-0.5 * eps)) * rho + 1.0


C_EXP_T1 = (1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0)
C_EXP_T2 = (1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0)
C_EXP_WIDE = (1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
            1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0)
LOG2E, LN2_HI, LN2_LO = 1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10


def exp_wide_reduced(x):
    """(n, r) of exp_wide_pair: x = n ln 2 + r."""
    x = np.asarray(x, float)
    n = np.rint(x * LOG2E)
    r = FMA(-n, LN2_HI, x)
    return n, FMA(-n, LN2_LO, r)


def t_exp_wide(x, mut=None):
    with np.errstate(all="ignore"):
        n, r = exp_wide_reduced(x)
        p = horner(C_EXP_WIDE, r, "exp.wide", mut)
        return np.ldexp(p, np.fmin(np.fmax(n, -1100.0), 1100.0).astype(int))


def exp_pair_tier(x0_wave, x2_wave, valid_wave):
    with np.errstate(invalid="ignore"):
        m = np.fmax(np.abs(x0_wave), np.abs(x2_wave))
        for tier, edge in enumerate(EXP_EDGES):
            if not np.any(~(m < edge) & valid_wave):
                return tier
    return 2


def t_exp_pair(x0, x2, valid=None, mut=None):
    x0, x2 = np.asarray(x0, float), np.asarray(x2, float)
    valid = np.ones(len(x0), bool) if valid is None else np.asarray(valid).astype(bool)
    n, (X0, X2, V) = _waves(x0, x2, valid)
    e0, e2 = np.empty_like(X0), np.empty_like(X2)
    with np.errstate(all="ignore"):
        for w in range(len(X0)):
            tier = exp_pair_tier(X0[w], X2[w], V[w])
            for X, e in ((X0, e0), (X2, e2)):
                if tier == 0:
                    e[w] = horner(C_EXP_T1, X[w], "exp.t1", mut)
                elif tier == 1:
                    e[w] = horner(C_EXP_T2, X[w], "exp.t2", mut)
                else:
                    e[w] = t_exp_wide(X[w], mut)
    return e0.ravel()[:n], e2.ravel()[:n]


def exp_one_halvings(x_wave):
    with np.errstate(invalid="ignore"):
        x = np.array(x_wave, float)
        k = 0
        while np.any(~(np.abs(x) < EXP_EDGES[0])) and k < 24:
            x *= 0.5
            k += 1
    return k


def t_exp_one(x, mut=None):
    n, (X,) = _waves(np.asarray(x, float))
    out = np.empty_like(X)
    with np.errstate(all="ignore"):
        for w in range(len(X)):
            xw = X[w]
            if not np.any(~(np.abs(xw) < EXP_EDGES[0])):
                out[w] = horner(C_EXP_T1, xw, "exp_one.in", mut)
                continue
            k = 0
            while np.any(~(np.abs(xw) < EXP_EDGES[0])) and k < 24:
                xw = xw * 0.5
                k += 1
            e = horner(C_EXP_T1, xw, "exp_one.cold", mut)
            for _ in range(k):
                e = e * e
            out[w] = e
    return out.ravel()[:n]


PLANAR_S = (-1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0)       # K.s3, K.s2, K.s1
PLANAR_C = (-1.0 / 720.0, 1.0 / 24.0, -0.5, 1.0)              # K.c3, K.c2: the cosine itself


def t_planar_rotation(a, mut=None):
    """planar_kinematic_n on (c, s) = (1, 0), hq h = 1: (cos a, sin a) the way the loop forms them."""
    a = np.asarray(a, float)
    n, (A,) = _waves(a)
    c, s = np.empty_like(A), np.empty_like(A)
    with np.errstate(all="ignore"):
        for w in range(len(A)):
            t = A[w] * A[w]
            if not np.any(t >= SINC_EDGE):
                sc = horner(PLANAR_S, t, "planar.sin", mut)
                cs = horner(PLANAR_C, t, "planar.cos", mut)
            else:
                sc, cc = t_sinc_cosc(t, mut)
                cs = FMA(-cc, t, 1.0)
            sn = sc * A[w]
            c[w] = FMA(-sn, 0.0, cs * 1.0)
            s[w] = FMA(cs, 0.0, sn * 1.0)
    return c.ravel()[:n], s.ravel()[:n]


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    forms: tuple                 # probe forms that take this case (variants of one operation: bit-identical)
    a: np.ndarray
    b: np.ndarray | None = None
    valid: np.ndarray | None = None
    tiers: np.ndarray | None = None      # per wave: the tier / trip count the wave is meant to take
    check: np.ndarray | None = None      # lanes held to the budget (all, unless some are sacrificed)
    budget: np.ndarray | None = None     # per element, ulps
    absolute: bool = False
    bias_edge: float | None = None       # the tier's upper edge: |input| in [0.98 edge, edge) enters the mean signed error
    bias_budget: float | None = None     # |mean signed error| there, ulps
    assert_values: bool = True           # False: the launch must return, nothing else
    note: str = ""
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        n = len(self.a)
        assert n <= MAX_VALUES, (self.name, n)
        if self.check is None:
            self.check = np.ones(n, bool)


def _rng(name):
    return np.random.default_rng(abs(hash_name(name)) % (2 ** 32))


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 61 - 1)
    return h


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def up(x):
    return np.nextafter(x, np.inf)


def down(x):
    return np.nextafter(x, -np.inf)


def tier_values(rng, lo, hi, n_waves, floor, edge_in=False, dense_top=0):
    """n_waves * 64 values of the tier [lo, hi): log-uniform (from `floor` if lo = 0), `dense_top` of them in the
    top 2 % of the tier, and in the first wave the lower edge with its upper neighbour, the largest value below the
    upper edge — and the upper edge itself where the form is called without a range check (edge_in)."""
    n = n_waves * WAVE
    v = log_uniform(rng, max(lo, floor), hi, n)
    v = np.minimum(v, down(hi))
    if dense_top:
        v[WAVE:WAVE + dense_top] = np.minimum(rng.uniform(0.98 * hi, hi, dense_top), down(hi))
    v[0] = lo
    v[1] = up(lo)
    v[2] = down(hi)
    v[3] = down(down(hi))
    if edge_in:
        v[4] = hi
        v[5] = up(hi)
    return v


def _series_remainder(K, y):
    """c_K y^K / (1 - y) in ulps: what the truncated series leaves out."""
    cK = series_coefs(K + 1)[0]
    return cK * y ** K / (1.0 - y) / ULP


# |mean signed error| over the top 2 % of the tier: the legitimate truncation there + 0.1 ulp (module docstring)
_BIAS = {
    "series12": _series_remainder(12, 0.04) + 0.1,
    "series20": _series_remainder(20, 0.15) + 0.1,
    "exp.t2": 0.04 ** 9 / 362880.0 / ULP + 0.1,
}


def _theta_cases():
    cases = []
    both = (THETA, THETA_BATCHED)
    lows = (0.0,) + THETA_EDGES
    for tier in range(3):
        K = (6, 12, 20)[tier]
        lo, hi = lows[tier], THETA_EDGES[tier]
        rng = _rng(f"theta{tier}")
        # the series on its own: the tier's range with the upper edge itself
        v = tier_values(rng, lo, hi, 24, 1.0e-12, edge_in=True, dense_top=512)
        bias = {"bias_edge": hi, "bias_budget": _BIAS[f"series{K}"]} if f"series{K}" in _BIAS else {}
        cases.append(Case(f"series{K}", ((SERIES6, SERIES12, SERIES20)[tier],), v, budget=np.full(len(v), 2.0),
                          **bias))
        # through the range checks: every wave inside the tier
        v = tier_values(rng, lo, hi, 24, 1.0e-12, dense_top=512)
        cases.append(Case(f"theta_over_sin/tier{tier + 1}", both, v, tiers=np.full(24, tier),
                          budget=np.full(len(v), 2.0), **bias))
    rng = _rng("theta3")
    v = tier_values(rng, 0.15, 0.999, 32, 0.15)
    v[4] = 0.999
    cases.append(Case("theta_over_sin/beyond", both, v, tiers=np.full(32, 3), budget=np.full(len(v), 4.0)))
    # towards theta = pi: a dozen points
    v = np.full(WAVE, 0.5)
    v[:12] = [1.0 - 10.0 ** -j for j in range(1, 13)]
    chk = np.zeros(WAVE, bool)
    chk[:12] = True
    cases.append(Case("theta_over_sin/near_one", both, v, tiers=np.full(1, 3), check=chk,
                      note="finite, positive, within 100 x the transcription's own error"))
    # one lane blown up (y = 0.99): the others stay inside the last tier's budget
    v = np.concatenate([tier_values(rng, lows[t], THETA_EDGES[t], 4, 1.0e-12) for t in range(3)])
    chk = np.ones(len(v), bool)
    for w in range(len(v) // WAVE):
        lane = int(rng.integers(0, WAVE))
        v[w * WAVE + lane] = 0.99
        chk[w * WAVE + lane] = False
    cases.append(Case("theta_over_sin/mixed", both, v, tiers=np.full(len(v) // WAVE, 3), check=chk,
                      budget=np.full(len(v), 4.0)))
    return cases


def _sinc_cases():
    cases = []
    both = (SINC_LEAN, SINC_PLAIN)
    rng = _rng("sinc")
    v = tier_values(rng, 0.0, SINC_EDGE, 32, 1.0e-30)
    cases.append(Case("sinc_cosc/in_range", both, v, tiers=np.zeros(32, int), budget=np.full(len(v), 1.0)))
    # k quarterings, k = 1 .. 13 (t <= 6e4): two waves each — every lane in the top bracket, and lanes from all
    # over [1e-6, bracket) under one lane at the top
    v, tiers = [], []
    for k in range(1, 14):
        lo, hi = SINC_EDGE * 4.0 ** (k - 1), min(SINC_EDGE * 4.0 ** k, 6.0e4)
        w1 = np.minimum(log_uniform(rng, lo, hi, WAVE), down(hi))
        w1[0] = lo
        w1[1] = down(hi) if k < 13 else hi
        w2 = log_uniform(rng, 1.0e-6, hi, WAVE)
        w2 = np.minimum(w2, down(hi))
        w2[int(rng.integers(0, WAVE))] = up(lo)
        v += [w1, w2]
        tiers += [k, k]
    v, tiers = np.concatenate(v), np.array(tiers)
    cases.append(Case("sinc_cosc/quartered", both, v, tiers=tiers, budget=np.repeat(2.0 * (tiers + 2), WAVE),
                      absolute=True))
    # one lane at t = 1e4 (k = 12) over in-range lanes
    v = tier_values(rng, 0.0, SINC_EDGE, 4, 1.0e-30)
    chk = np.ones(len(v), bool)
    for w in range(4):
        lane = int(rng.integers(6, WAVE))
        v[w * WAVE + lane] = 1.0e4
        chk[w * WAVE + lane] = False
    cases.append(Case("sinc_cosc/mixed", both, v, tiers=np.full(4, 12), check=chk,
                      budget=np.full(len(v), 2.0 * 14), absolute=True))
    v = np.full(3 * WAVE, 1.0e-4)
    v[0:8] = [4.3e6, 1.0e8, 1.0e30, 1.0e300, np.inf, 4.3e6, 5.0e6, 1.0e-5]
    v[WAVE] = np.nan
    v[2 * WAVE] = np.inf
    v[2 * WAVE + 1] = np.nan
    cases.append(Case("sinc_cosc/non_finite", both, v, assert_values=False))
    return cases


def _signed(rng, v):
    return v * rng.choice([-1.0, 1.0], len(v))


def _exp_cases():
    cases = []
    rng = _rng("exp")
    lows = (0.0,) + EXP_EDGES
    for tier in range(2):
        lo, hi = lows[tier], EXP_EDGES[tier]
        a = tier_values(rng, lo, hi, 24, 1.0e-20, dense_top=512)
        b = tier_values(rng, lo, hi, 24, 1.0e-20, dense_top=512)[::-1].copy()
        a, b = _signed(rng, a), _signed(rng, b)
        a[6], b[6] = -down(hi), down(hi)
        tag = ("exp.t1", "exp.t2")[tier]
        bias = {"bias_edge": hi, "bias_budget": _BIAS[tag]} if tag in _BIAS else {}
        cases.append(Case(f"exp_pair/tier{tier + 1}", (EXP_PAIR,), a, b=b, tiers=np.full(24, tier),
                          budget=np.full(len(a), 2.0), **bias))
    a = _signed(rng, tier_values(rng, 0.04, 700.0, 32, 0.04))
    b = _signed(rng, log_uniform(rng, 1.0e-6, 700.0, len(a)))
    a[4], a[5], b[4], b[5] = 700.0, -700.0, -700.0, 700.0
    cases.append(Case("exp_pair/beyond", (EXP_PAIR,), a, b=b, tiers=np.full(32, 2), budget=np.full(len(a), 2.0)))
    # exp_wide_pair itself, over everything it may be handed: |x| <= 700, dense where |r| is largest (odd
    # multiples of ln 2 / 2: the polynomial's edge)
    a = _signed(rng, log_uniform(rng, 1.0e-6, 700.0, 48 * WAVE))
    b = _signed(rng, log_uniform(rng, 1.0e-6, 700.0, 48 * WAVE))
    odd = (2.0 * rng.integers(-1000, 1000, 16 * WAVE) + 1.0) * (np.log(2.0) / 2.0)
    b[:16 * WAVE] = odd * (1.0 + rng.uniform(-1.0, 1.0, len(odd)) * 1.0e-3 / np.maximum(np.abs(odd), 1.0))
    a[0:6] = [0.0, 700.0, -700.0, 1.0e-3, 0.04, -0.04]
    cases.append(Case("exp_wide_pair", (EXP_WIDE,), a, b=b, budget=np.full(len(a), 2.0)))
    # one lane at x0 = -300 over first-tier lanes: the wave takes exp_wide_pair
    a = _signed(rng, tier_values(rng, 0.0, 1.0e-3, 4, 1.0e-20))
    b = _signed(rng, tier_values(rng, 0.0, 1.0e-3, 4, 1.0e-20))
    chk = np.ones(len(a), bool)
    for w in range(4):
        lane = int(rng.integers(6, WAVE))
        a[w * WAVE + lane] = -300.0
        chk[w * WAVE + lane] = False
    cases.append(Case("exp_pair/mixed", (EXP_PAIR,), a, b=b, tiers=np.full(4, 2), check=chk,
                      budget=np.full(len(a), 2.0)))
    return cases


def _exp_one_cases():
    cases = []
    rng = _rng("exp_one")
    a = _signed(rng, tier_values(rng, 0.0, 1.0e-3, 32, 1.0e-20))
    a[6], a[7] = -down(1.0e-3), down(1.0e-3)
    cases.append(Case("exp_one/in_range", (EXP_ONE,), a, tiers=np.zeros(32, int), budget=np.full(len(a), 2.0)))
    v, tiers = [], []
    for k in range(1, 21):
        lo, hi = 1.0e-3 * 2.0 ** (k - 1), min(1.0e-3 * 2.0 ** k, 700.0)
        w1 = np.minimum(log_uniform(rng, lo, hi, WAVE), down(hi))
        w1[0] = lo
        w1[1] = down(hi) if k < 20 else hi
        w2 = np.minimum(log_uniform(rng, 1.0e-6, hi, WAVE), down(hi))
        w2[int(rng.integers(0, WAVE))] = up(lo)
        v += [-w1, -w2]
        tiers += [k, k]
    v, tiers = np.concatenate(v), np.array(tiers)
    cases.append(Case("exp_one/halved", (EXP_ONE,), v, tiers=tiers, budget=np.repeat(2.0 ** tiers, WAVE)))
    a = -tier_values(rng, 0.0, 1.0e-3, 4, 1.0e-20)
    chk = np.ones(len(a), bool)
    for w in range(4):
        lane = int(rng.integers(6, WAVE))
        a[w * WAVE + lane] = -300.0
        chk[w * WAVE + lane] = False
    cases.append(Case("exp_one/mixed", (EXP_ONE,), a, tiers=np.full(4, 19), check=chk,
                      budget=np.full(len(a), 2.0 ** 19)))
    return cases


def _planar_cases():
    cases = []
    rng = _rng("planar")
    edge = np.sqrt(SINC_EDGE)
    while edge * edge >= SINC_EDGE:          # the largest a with a^2 < 1e-3 as the device squares it
        edge = down(edge)
    a = _signed(rng, np.minimum(log_uniform(rng, 1.0e-12, edge, 32 * WAVE), edge))
    a[0:4] = [0.0, edge, -edge, down(edge)]
    cases.append(Case("planar_rotation/in_range", (PLANAR,), a, tiers=np.zeros(32, int),
                      budget=np.full(len(a), 2.0), absolute=True))
    v, tiers = [], []
    for k in range(1, 10):
        lo, hi = np.sqrt(SINC_EDGE * 4.0 ** (k - 1)), min(np.sqrt(SINC_EDGE * 4.0 ** k), 10.0)
        lo, hi = up(up(lo)), down(down(hi))          # (the square must land in the bracket)
        w1 = np.clip(log_uniform(rng, lo, hi, WAVE), lo, hi)
        w1[0], w1[1] = lo, hi
        w2 = np.minimum(log_uniform(rng, 1.0e-6, hi, WAVE), hi)
        w2[int(rng.integers(0, WAVE))] = lo
        v += [_signed(rng, w1), _signed(rng, w2)]
        tiers += [k, k]
    v, tiers = np.concatenate(v), np.array(tiers)
    v[-WAVE + 1] = 10.0
    cases.append(Case("planar_rotation/quartered", (PLANAR,), v, tiers=tiers,
                      budget=np.repeat(2.0 * (tiers + 2), WAVE), absolute=True))
    a = _signed(rng, np.minimum(log_uniform(rng, 1.0e-12, edge, 4 * WAVE), edge))
    chk = np.ones(len(a), bool)
    for w in range(4):
        lane = int(rng.integers(0, WAVE))
        a[w * WAVE + lane] = 10.0
        chk[w * WAVE + lane] = False
    cases.append(Case("planar_rotation/mixed", (PLANAR,), a, tiers=np.full(4, 9), check=chk,
                      budget=np.full(len(a), 2.0 * 11), absolute=True))
    return cases


def _rcp_inputs(rng):
    v = [log_uniform(rng, 1.0e-300, 1.0e300, 2048), log_uniform(rng, 1.0e-20, 1.0e6, 1024)]
    p = np.ldexp(1.0, np.arange(-996, 997, 12))
    v += [p, up(p), down(p), np.array([1.0e-20, 1.0e-300, 1.0e300, up(1.0e-300), down(1.0e300)])]
    return np.concatenate(v)


def _rcp_cases():
    x = _rcp_inputs(_rng("rcp"))
    one = np.full(len(x), 1.0)
    return [Case("fast_rcp", (FAST_RCP,), x, budget=one, extra={"seed": SEED_RCP}),
            Case("fast_rsqrt", (FAST_RSQRT,), x, budget=one, extra={"seed": SEED_RSQ}),
            Case("seed_rcp", (SEED_RCP,), x, budget=one * 2.0 ** 32, note="2^-20 relative"),
            Case("seed_rsq", (SEED_RSQ,), x, budget=one * 2.0 ** 32, note="2^-20 relative")]


def _eps_sin_cases():
    rng = _rng("eps_sin")
    y = log_uniform(rng, 1.0e-11, 0.999, MAX_VALUES)
    y[0:4] = [1.0e-11, 0.999, 0.5, up(0.5)]
    return [Case("eps_sin_factor", (EPS_SIN,), y, b=np.full(len(y), EPS),
                 note="|got - ref| <= 2^-22 |ref - 1| + 1 ulp")]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for c in (_rcp_cases() + _theta_cases() + _sinc_cases() + _eps_sin_cases() + _exp_cases() + _exp_one_cases()
              + _planar_cases()):
        assert c.name not in out
        out[c.name] = c
    return out


def family(case):
    return case.name.split("/")[0]


def wave_tiers(case):
    """The tier / trip count each wave of the case takes, by the device's own wave-uniform checks."""
    fam = family(case)
    valid = np.ones(len(case.a), bool) if case.valid is None else case.valid.astype(bool)
    if fam == "theta_over_sin":
        _, (Y, V) = _waves(case.a, valid)
        return np.array([theta_tier(y, v) for y, v in zip(Y, V)])
    if fam == "sinc_cosc":
        _, (T,) = _waves(case.a)
        return np.array([sinc_quarterings(t) for t in T])
    if fam == "planar_rotation":
        _, (A,) = _waves(case.a)
        return np.array([sinc_quarterings(a * a) for a in A])
    if fam == "exp_pair":
        _, (X0, X2, V) = _waves(case.a, case.b, valid)
        return np.array([exp_pair_tier(a, b, v) for a, b, v in zip(X0, X2, V)])
    if fam == "exp_one":
        _, (X,) = _waves(case.a)
        return np.array([exp_one_halvings(x) for x in X])
    raise KeyError(fam)


def transcribe(case, mut=None):
    """The transcription's outputs for a case: a tuple of one or two arrays."""
    fam = family(case)
    if fam == "fast_rcp":
        return (t_fast_rcp(case.a, mut=mut),)
    if fam == "fast_rsqrt":
        return (t_fast_rsqrt(case.a, mut=mut),)
    if fam == "seed_rcp":
        return (seed24(1.0 / case.a),)
    if fam == "seed_rsq":
        return (seed24(1.0 / np.sqrt(case.a)),)
    if fam.startswith("series"):
        return (t_series(int(fam[6:]), case.a, mut),)
    if fam == "theta_over_sin":
        return (t_theta_over_sin(case.a, case.valid, mut),)
    if fam == "sinc_cosc":
        return t_sinc_cosc(case.a, mut)
    if fam == "eps_sin_factor":
        return (t_eps_sin_factor(case.a, case.b),)
    if fam == "exp_pair":
        return t_exp_pair(case.a, case.b, case.valid, mut)
    if fam == "exp_wide_pair":
        return t_exp_wide(case.a, mut), t_exp_wide(case.b, mut)
    if fam == "exp_one":
        return (t_exp_one(case.a, mut),)
    if fam == "planar_rotation":
        return t_planar_rotation(case.a, mut)
    raise KeyError(fam)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The 50-digit reference of a case, once per process: a tuple of one or two lists of mpf."""
    case = cases()[name]
    fam = family(case)
    if not case.assert_values:
        return None
    if fam in ("fast_rcp", "seed_rcp"):
        return (ref_rcp(case.a),)
    if fam in ("fast_rsqrt", "seed_rsq"):
        return (ref_rsqrt(case.a),)
    if fam.startswith("series") or fam == "theta_over_sin":
        return (ref_theta_over_sin(case.a),)
    if fam == "sinc_cosc":
        return ref_sinc_cosc(case.a)
    if fam == "eps_sin_factor":
        return (ref_eps_sin_factor(case.a, case.b),)
    if fam in ("exp_pair", "exp_wide_pair"):
        return ref_exp(case.a), ref_exp(case.b)
    if fam == "exp_one":
        return (ref_exp(case.a),)
    if fam == "planar_rotation":
        return ref_cos_sin(case.a)
    raise KeyError(fam)


def errors(case, outputs):
    """Per output: |outputs - reference| in ulps (relative, or absolute for the case's kind), all lanes."""
    return [err_ulps(o, r, case.absolute) for o, r in zip(outputs, reference(case.name))]


def edge_bias(case, outputs):
    """Per output: the mean signed relative error (ulps) over the inputs in the top 2 % of the case's tier."""
    out = []
    for x, o, r in zip((case.a, case.b), outputs, reference(case.name)):
        m = (np.abs(x) >= 0.98 * case.bias_edge) & (np.abs(x) < case.bias_edge)
        assert m.sum() >= 512, (case.name, int(m.sum()))
        idx = np.flatnonzero(m)
        out.append(float(np.mean(signed_err_ulps(o[idx], [r[i] for i in idx]))))
    return out


def eps_sin_excess(case, got):
    """|got - ref| - 2^-22 |ref - 1|, in ulps of the reference: the budget is 1."""
    out = np.empty(len(got))
    for i, (g, r) in enumerate(zip(got, reference(case.name)[0])):
        out[i] = float((abs(_mpf(g) - r) - abs(r - 1) * 2.0 ** -22) / abs(r) / ULP) if np.isfinite(g) else np.inf
    return out
