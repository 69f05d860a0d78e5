"""Cases, references and budgets for ONE force evaluation and rate update of the FAST step kernels, run alone through
csrc/probe/softrod_dyn_probe.hip: dynamic_n (softrod_fast.hpp) and planar_dynamic_n (softrod_planar.hpp).  Shared by
tests/test_dyn_probe.py (CPU) and tests/test_gpu_dyn_probe.py.

REFERENCE L, the literal law.  literal_law() is one scalar transcription of oracle/softrod_oracle_np.py's _shear_stress,
_kappa, _forces_and_torques, forcing (gravity, the point force), dynamic and dampen, generic over the number type.  In
Python floats it is tied to the NumPy twin at 1e-12 of the rod's largest force / torque component; in mpmath at 50 digits it
is the reference for dynamic_n.  It takes what the device takes — the fp64 state and the fp64 material constants (masses,
stiffnesses, J, 1 / J, log c_r) — and forms cf, ca, cw and c_r^e from them at 50 digits, so the device, the float run and
the twin differ from it by rounding alone.  (The dilatation rate is written d . (v+ - v) / (l l^), the twin's expanded four
dot products being the same number; c_r^e is exp(e log c_r) with log c_r the fp64 input both the device and the twin get.)

REFERENCE P, the planar substep as softrod_planar.hpp documents it: kappa = s2 D (1 + acos_shift / 3)
(1 - eps_sin / sqrt(D^2 + 2 acos_shift)) / D^ from the carried angle, edges from the carried d, the dilatation rate from the
carried dv, the damper c_r^e, node 0's v_y pinned (force coefficient zero).  planar_gap() holds P against L at 50 digits:
that is the only place where the header's two modelling claims are held; the device is held to P by rounding alone.

RODS.  Crafted, not random walks: per joint the relative rotation angle, its axis, per element the stretch, the tilt of
the tangent from d3 are drawn from lists (THETAS, AXES, STRETCHES, TILTS) independently — rod r starts each list at another
entry, so that the end elements walk through every entry — and one rod of every case has exact zeros in every velocity and
rate (v_out = cf f + ca then shows the forces alone).  `hot` rods keep every joint and element inside the first tier of
theta_over_sin and exp_pair; `one_theta` / `one_stretch` are hot rods with ONE joint at theta = 2 / ONE element at e = 2
that drag the wave into the cold tier.

BUDGETS, measured on the reference side — never on the device.  Errors are in units of 2^-52 x a scale built from the
50-digit intermediates BEFORE cancellation:
  node velocity  |damp_t v| + cf max |stress of the two adjoining elements| + |ca|      (stress: S max(|Q t|, 1 / e))
  element rate   c_r^e (|w| + cw e max(couple of either vertex, kappa x B kappa term, shear couple, transport,
                 dilatation)); the couple scale is B / D^ / vd^3 x max(1, |vec|), not B |kappa|: R - R^T carries an
                 absolute 1e-16 whatever theta is
  t              1
  kap            1 / D^ x max(1, theta / sin theta)
Baseline, per case and output: the worse of two roundings of the literal law, the float run of L and the NumPy twin (planar:
the float runs of P and of L, each against its own 50-digit run).  The device is held to 4 x baseline, floor 8 — the rule
and the two reasons of tests/rod_probe_ref.py (fast_rcp / fast_rsqrt are good to 1 ulp where division and sqrt round to
half; the FAST form associates the same sums differently).
"""
from __future__ import annotations

import functools
import json
import math
from dataclasses import dataclass
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from oracle import softrod_oracle_np as O
from tests import math_primitives_ref as M
from tests import rod_probe_ref as R

MP = M.MP
ULP = M.ULP
WAVE = 64
ROOT = Path(__file__).resolve().parents[1]

# feature bits (include/softrod.h) and the probe's forms (enum DynForm)
GRAVITY, POINT_FORCE, PENDULUM_BC, DAMPER, CONTACT, REST_KAPPA, PLANE_ZUP = 1, 2, 4, 8, 256, 512, 1 << 30
ARM_SINGLE = GRAVITY | CONTACT | DAMPER | REST_KAPPA
SOFTPENDULUM = GRAVITY | POINT_FORCE | PENDULUM_BC | DAMPER
MASKS = {"damper": DAMPER, "damper+gravity": DAMPER | GRAVITY, "damper+rest_kappa": DAMPER | REST_KAPPA}
RT1, RT2, RT_TAPER1, ARM1, ARM2, ARM_TAPER1 = range(6)
N_FORMS, N_PARAMS = 6, 50
FORM_NAMES = {RT1: "<runtime,1>", RT2: "<runtime,2>", RT_TAPER1: "<runtime,1,taper>", ARM1: "<ArmSingleZup,1>",
              ARM2: "<ArmSingleZup,2>", ARM_TAPER1: "<ArmSingleZup,1,taper>"}
FORM_EPL = {RT1: 1, RT2: 2, RT_TAPER1: 1, ARM1: 1, ARM2: 2, ARM_TAPER1: 1}
FORM_TAPER = {RT1: False, RT2: False, RT_TAPER1: True, ARM1: False, ARM2: False, ARM_TAPER1: True}
MAT_ROWS = 16      # SOFTROD_MATERIAL_ROWS; the rows' order is enum MatRow (softrod_kernels.hpp)

THETAS = (0.0, 1e-9, 1e-5, 1e-3, 0.05, 0.0999, 0.1001, 0.3, 0.6, 1.0, 2.0, 3.0)     # (0.6: the 20-term tier, 0.04 <= y < 0.15)
HOT_THETAS = (0.0, 1e-9, 1e-5, 1e-3, 0.05)
AXES = ("d3", "d1", "generic")
STRETCHES = (0.5, 0.9, 1.0 - 1e-9, 1.0, 1.0 + 1e-9, 1.1, 2.0)
HOT_STRETCHES = (1.0 - 1e-9, 1.0, 1.0 + 1e-9)
TILTS = (0.0, 1e-8, 0.01, 0.3)
PLANAR_DL = (0.0, 1e-9, -1e-9, 1e-5, -1e-5, 0.05, -0.05, 0.3, -0.3, 1.5, -1.5)

MUTATIONS = ("couple_e2", "voronoi_no_half", "kxbk_sign", "swap_gj_ei", "lever_rest_len", "transport_no_e",
             "dilatation_il", "no_acos_shift", "no_eps_sin", "no_eps_length", "damper_e1", "wrong_neighbour",
             "no_rest_kappa", "planar_no_shift_third", "planar_old_dv")
PLANAR_ONLY = ("planar_no_shift_third", "planar_old_dv")


@dataclass(frozen=True)
class Arith:
    num: object
    sqrt: object
    acos: object
    sin: object
    exp: object


FLOAT = Arith(float, math.sqrt, math.acos, math.sin, math.exp)
MPF = Arith(lambda v: MP.mpf(v), MP.sqrt, MP.acos, MP.sin, MP.exp)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _amax(a):
    return max(abs(c) for c in a)


# ---------------------------------------------------------------------------------------------------------------
# materials: what fill_params / softrod_set_radius_profile derive, as the fp64 numbers the device gets
# ---------------------------------------------------------------------------------------------------------------
def material(n, kind="arm", taper=False, features=DAMPER, damping=None):
    """kind 'arm': a soft arm of 2 cm elements (log c_r = -0.057, the octopus arm's); 'pendulum': SoftPendulum-v0's rod with
    2 cm elements.  taper: the radius falls 10:1 along the rod (per-element constants, CosseratRod.straight_rod's)."""
    if kind == "arm":
        dt, rest_len, r0, rho, E = 2.0e-5, 0.02, 0.012, 1000.0, 1.0e6
        nu = 0.057 / (dt * 4.0 / (r0 * r0)) if damping is None else damping
        gravity = (0.0, 0.0, -9.80665)
    else:
        dt, rest_len, r0, rho, E = 1.0e-4, 0.02, 0.05, 1000.0, 1.0e6
        nu = 2.0e-3 if damping is None else damping
        gravity = (0.0, -9.80665, 0.0)
    G, alpha_c = E / (2.0 * (1.0 + 0.5)), 27.0 / 28.0
    radius = r0 * np.linspace(1.0, 0.1, n) if taper else np.full(n, r0)
    A0 = np.pi * radius * radius
    I1 = A0 * A0 / (4.0 * np.pi)
    J0, J2 = I1 * (rho * rest_len), 2.0 * I1 * (rho * rest_len)
    volume = np.pi * (radius * radius) * rest_len
    m = SimpleNamespace(n=n, kind=kind, taper=taper, features=features, dt=dt, rest_len=rest_len,
                        inv_rest_len=1.0 / rest_len, rest_vor=0.5 * (rest_len + rest_len), eps_length=1e-14,
                        acos_shift=1e-10, eps_sin=1e-14, gravity=gravity, point_force=0.0)
    m.inv_rest_vor = 1.0 / m.rest_vor
    m.mass_node = float(rho * volume[0])
    if taper:
        m.mass = np.zeros(n + 1)
        m.mass[:-1] += 0.5 * rho * volume
        m.mass[1:] += 0.5 * rho * volume
        me = 0.5 * (m.mass[1:] + m.mass[:-1])
        me[0] += 0.5 * m.mass[0]
        me[-1] += 0.5 * m.mass[-1]
    else:           # build_const_m's own: the interior node mass, halved at the two ends
        m.mass = np.full(n + 1, m.mass_node)
        m.mass[0] = m.mass[-1] = 0.5 * m.mass_node
        me = np.full(n, m.mass_node)
    m.J0, m.J2, m.invJ0, m.invJ2 = J0, J2, 1.0 / J0, 1.0 / J2
    m.shear01, m.shear2 = alpha_c * G * A0, E * A0
    b01, b2 = E * I1, G * 2.0 * I1
    m.bend01, m.bend2 = 0.5 * (b01[1:] + b01[:-1]), 0.5 * (b2[1:] + b2[:-1])
    m.damp_t = math.exp(-nu * dt)
    m.dlog0, m.dlog2 = -nu * dt * me * m.invJ0, -nu * dt * me * m.invJ2
    m.dr0, m.dr2 = np.exp(m.dlog0), np.exp(m.dlog2)
    m.r0s = radius * math.sqrt(rest_len)
    m.contact = R._par(R.E_Z, R.MU_OCTOPUS, r0=float(m.r0s[0]) / math.sqrt(rest_len))
    return m


def with_features(m, features):
    out = SimpleNamespace(**vars(m))
    out.features = features
    return out


def params(m):
    """The probe's host parameter block (enum Par of softrod_dyn_probe.hip)."""
    c = m.contact
    p = [m.dt, m.rest_len, m.inv_rest_len, m.rest_vor, m.inv_rest_vor,
         m.J0[0], m.J0[0], m.J2[0], m.invJ0[0], m.invJ0[0], m.invJ2[0], m.shear01[0], m.shear01[0], m.shear2[0],
         m.bend01[0], m.bend01[0], m.bend2[0], m.mass_node, *m.gravity, m.damp_t, m.dr0[0], m.dr0[0], m.dr2[0],
         m.dlog0[0], m.dlog0[0], m.dlog2[0], m.eps_length, m.acos_shift, m.eps_sin, float(m.features),
         *c.origin, *c.normal, c.k, c.nu, c.slip_tol, c.surface_tol, *c.kin_mu, *c.stat_mu, float(m.r0s[0]),
         m.point_force]
    assert len(p) == N_PARAMS
    return [float(v) for v in p]


def material_table(m, epl):
    """build_const_m's table of a tapered rod: [MAT_ROWS][64 epl], element / node / vertex k in slot k; 1 behind."""
    W, n = WAVE * epl, m.n
    t = np.ones((MAT_ROWS, W))
    t[0, :n + 1] = m.mass
    for row, a in ((1, m.shear01), (2, m.shear2), (5, m.J0), (6, m.J2), (7, m.invJ0), (8, m.invJ2), (9, m.dlog0),
                   (10, m.dlog2), (11, m.dr0), (12, m.dr2), (13, m.r0s), (14, 1.0 / m.r0s)):
        t[row, :n] = a
    t[3, :n - 1], t[4, :n - 1] = m.bend01, m.bend2
    return t


# ---------------------------------------------------------------------------------------------------------------
# L: the literal law, generic over the number type
# ---------------------------------------------------------------------------------------------------------------
def literal_law(rod, A=FLOAT, mut=(), features=None):
    """-> namespace v (n + 1, 3), w, t (n, 3), kap (n - 1, 3) as nested lists of A's numbers, info (magnitudes of the
    intermediates, for the scales and the tier counts).  rod: n, x, v (n + 1, 3), Q (n, 9) row-major (row i = d_{i+1}),
    w (n, 3), rk (n - 1, 3), mat.  mut: names from MUTATIONS (the CPU test's teeth)."""
    num, sqrt = A.num, A.sqrt
    m, n = rod.mat, rod.n
    feat = m.features if features is None else features
    zero, one, half = num(0.0), num(1.0), num(0.5)

    def vecs(a):
        return [[num(c) for c in row] for row in a]

    def arr(a):
        return [num(c) for c in a]

    x, v, Q, w = vecs(rod.x), vecs(rod.v), vecs(rod.Q), vecs(rod.w)
    use_rk = (feat & REST_KAPPA) and "no_rest_kappa" not in mut
    rk = vecs(rod.rk) if use_rk else [[zero] * 3 for _ in range(n - 1)]
    rest_len, rest_vor, dt = num(m.rest_len), num(m.rest_vor), num(m.dt)
    eps_len = zero if "no_eps_length" in mut else num(m.eps_length)
    shift = zero if "no_acos_shift" in mut else num(m.acos_shift)
    eps_sin = zero if "no_eps_sin" in mut else num(m.eps_sin)
    mass, s01, s2 = arr(m.mass), arr(m.shear01), arr(m.shear2)
    b01, b2 = arr(m.bend01), arr(m.bend2)
    if "swap_gj_ei" in mut:
        b01, b2 = b2, b01
    J = [[num(a), num(a), num(b)] for a, b in zip(m.J0, m.J2)]
    invJ = [[num(a), num(a), num(b)] for a, b in zip(m.invJ0, m.invJ2)]
    dlog = [[num(a), num(a), num(b)] for a, b in zip(m.dlog0, m.dlog2)]
    info = SimpleNamespace(e=[], stress=[], shear_couple=[], transport=[], dilatation=[], couple=[], kxbk=[], theta=[],
                           y=[], tos=[], damper=[], x0=[], x2=[])

    # _shear_stress
    d, ln, tang, e, qt, nint, cs = [], [], [], [], [], [], []
    for k in range(n):
        dk = [x[k + 1][i] - x[k][i] for i in range(3)]
        lk = sqrt(_dot(dk, dk)) + eps_len
        tk = [c / lk for c in dk]
        ek = lk / rest_len
        q = [_dot(Q[k][3 * i:3 * i + 3], tk) for i in range(3)]
        sigma = [ek * q[0], ek * q[1], ek * q[2] - one]
        nk = [s01[k] * sigma[0], s01[k] * sigma[1], s2[k] * sigma[2]]
        ck = [(Q[k][i] * nk[0] + Q[k][3 + i] * nk[1] + Q[k][6 + i] * nk[2]) / ek for i in range(3)]
        d.append(dk); ln.append(lk); tang.append(tk); e.append(ek); qt.append(q); nint.append(nk); cs.append(ck)
        info.e.append(ek)
        info.stress.append(max(s01[k] * abs(q[0]), s01[k] * abs(q[1]), s2[k] * max(abs(q[2]), one / ek)))

    def cs_at(k):
        return cs[k] if 0 <= k < n else [zero] * 3

    if "wrong_neighbour" in mut:
        f_int = [[cs_at(k)[i] - cs_at(k + 1)[i] for i in range(3)] for k in range(n + 1)]
    else:
        f_int = [[cs_at(k)[i] - cs_at(k - 1)[i] for i in range(3)] for k in range(n + 1)]

    # _kappa and the Voronoi couples
    kap, c2, c3 = [], [], []
    for j in range(n - 1):
        Rm = [[sum(Q[j + 1][3 * a + c] * Q[j][3 * b + c] for c in range(3)) for b in range(3)] for a in range(3)]
        vec = [Rm[2][1] - Rm[1][2], Rm[0][2] - Rm[2][0], Rm[1][0] - Rm[0][1]]
        trace = Rm[0][0] + Rm[1][1] + Rm[2][2]
        arg = half * trace - half - shift
        if "no_acos_shift" in mut:           # (the mutated law alone can leave arccos' domain, or meet 0 / 0)
            arg = min(arg, one)
        theta = A.acos(arg)
        g = -half * theta / A.sin(theta + eps_sin)
        kj = [c * g / rest_vor for c in vec]
        bend = [b01[j], b01[j], b2[j]]
        mint = [bend[i] * (kj[i] - rk[j][i]) for i in range(3)]
        vdil = (ln[j + 1] + ln[j]) / rest_vor * (one if "voronoi_no_half" in mut else half)
        e3 = one / (vdil * vdil) if "couple_e2" in mut else one / (vdil * vdil * vdil)
        kxm = _cross(kj, mint)
        if "kxbk_sign" in mut:
            kxm = [-c for c in kxm]
        kap.append(kj)
        c2.append([c * e3 for c in mint])
        c3.append([c * rest_vor * e3 for c in kxm])
        info.theta.append(theta)
        info.y.append(num(0.75) + half * num(m.acos_shift) - num(0.25) * trace)
        info.tos.append(abs(theta / A.sin(theta)) if theta != 0 else one)
        info.couple.append(max(bend) / rest_vor * e3 * max(one, _amax(vec)))
        info.kxbk.append(half * _amax(c3[-1]))

    def at(a, j):
        return a[j] if 0 <= j < n - 1 else [zero] * 3

    v_new, w_new = [], []
    g = arr(m.gravity)
    for k in range(n + 1):
        fe = [g[i] * mass[k] for i in range(3)] if feat & GRAVITY else [zero] * 3
        if (feat & POINT_FORCE) and k == 0:
            fe[0] = num(m.point_force)
        vk = [v[k][i] + dt * ((f_int[k][i] + fe[i]) / mass[k]) for i in range(3)]
        if (feat & PENDULUM_BC) and k == 0:
            vk[1] = vk[2] = zero
        if feat & DAMPER:
            vk = [c * num(m.damp_t) for c in vk]
        v_new.append(vk)
    for k in range(n):
        c2d = [at(c2, k)[i] - at(c2, k - 1)[i] for i in range(3)]
        c3d = [half * (at(c3, k)[i] + at(c3, k - 1)[i]) for i in range(3)]
        lever = rest_len / e[k] if "lever_rest_len" in mut else rest_len
        ssc = [c * lever for c in _cross(qt[k], nint[k])]
        jwe = [J[k][i] * w[k][i] / (one if "transport_no_e" in mut else e[k]) for i in range(3)]
        lt = _cross(jwe, w[k])
        dv = [v[k + 1][i] - v[k][i] for i in range(3)]
        dil_rate = _dot(d[k], dv) / rest_len / (one if "dilatation_il" in mut else ln[k])
        ud = [c * dil_rate / e[k] for c in jwe]
        t_int = [c2d[i] + c3d[i] + ssc[i] + lt[i] + ud[i] for i in range(3)]
        wk = [w[k][i] + dt * (invJ[k][i] * t_int[i]) * e[k] for i in range(3)]
        if (feat & PENDULUM_BC) and k == 0:
            wk[0] = wk[2] = zero
        ex = one if "damper_e1" in mut else e[k]
        damp = [A.exp(dlog[k][i] * ex) for i in range(3)] if feat & DAMPER else [one] * 3
        w_new.append([wk[i] * damp[i] for i in range(3)])
        npk = [s01[k] * abs(qt[k][0]), s01[k] * abs(qt[k][1]), s2[k] * max(abs(qt[k][2]), one / e[k])]
        info.shear_couple.append(ln[k] * _amax(qt[k]) * max(npk))
        info.transport.append(_amax(jwe) * _amax(w[k]))
        info.dilatation.append(_amax(ud))
        info.damper.append(max(damp))
        info.x0.append((e[k] - one) * dlog[k][0])
        info.x2.append((e[k] - one) * dlog[k][2])
    return SimpleNamespace(v=v_new, w=w_new, t=tang, kap=kap, info=info)


def twin(rod, features=None):
    """The same evaluation by oracle/softrod_oracle_np.py's whole-array kernels -> namespace of numpy arrays v, w, t,
    kap, and the rod's internal force / torque (for the 1e-12 tie)."""
    m, n = rod.mat, rod.n
    feat = m.features if features is None else features
    o = object.__new__(O.NumpyRod)
    o.cfg = SimpleNamespace(eps_length=m.eps_length, acos_shift=m.acos_shift, eps_sin=m.eps_sin, features=feat,
                            gravity=m.gravity, tip_force=(0.0, 0.0, 0.0), damp_before_constrain=0, dt=m.dt)
    o.n = n
    o.x, o.v = np.array(rod.x, float).T.copy(), np.array(rod.v, float).T.copy()
    o.Q = np.array(rod.Q, float).reshape(n, 3, 3).transpose(1, 2, 0).copy()
    o.w = np.array(rod.w, float).T.copy()
    o.rest_len, o.rest_vor = np.full(n, m.rest_len), np.full(n - 1, m.rest_vor)
    o.volume = np.ones(n)
    o.shear = np.array([m.shear01, m.shear01, m.shear2])
    o.bend = np.array([m.bend01, m.bend01, m.bend2])
    o.J, o.invJ = np.array([m.J0, m.J0, m.J2]), np.array([m.invJ0, m.invJ0, m.invJ2])
    o.mass = np.array(m.mass, float)
    o.rest_sigma = np.zeros((3, n))
    o.rest_kappa = np.array(rod.rk, float).T.copy() if feat & REST_KAPPA else np.zeros((3, n - 1))
    o.f_ext, o.t_ext = np.zeros((3, n + 1)), np.zeros((3, n))
    o.damp_t = m.damp_t
    o.damp_r = np.exp(np.array([m.dlog0, m.dlog0, m.dlog2]))
    o.point_force = m.point_force
    o.fixed_pos, o.fixed_dir = o.x[:, 0].copy(), o.Q[:, :, 0].copy()
    o._forces_and_torques()
    o.forcing()
    o.dynamic(m.dt)
    o.rates_operators()
    return SimpleNamespace(v=o.v.T.copy(), w=o.w.T.copy(), t=o.tang.T.copy(), kap=o.kappa.T.copy(),
                           f_int=o.f_int.T.copy(), t_int=o.t_int.T.copy())


# ---------------------------------------------------------------------------------------------------------------
# P: the planar substep as softrod_planar.hpp documents it
# ---------------------------------------------------------------------------------------------------------------
def planar_law(rod, A=FLOAT, mut=()):
    """-> namespace v (n + 1, 2), wz (n), t (n, 2), dv (n, 2), up (n - 1: the Voronoi couples), info.  rod: n, v (n + 1, 2),
    c, s, wz (n), dl (n - 1), d, dv (n, 2), s2, mat (entries may already be A's numbers)."""
    num, sqrt = A.num, A.sqrt
    m, n = rod.mat, rod.n
    zero, one, half = num(0.0), num(1.0), num(0.5)
    v = [[num(c) for c in row] for row in rod.v]
    d = [[num(c) for c in row] for row in rod.d]
    dv = [[num(c) for c in row] for row in rod.dv]
    c, s, wz, dl = ([num(a) for a in b] for b in (rod.c, rod.s, rod.wz, rod.dl))
    rest_len, rest_vor, dt, damp_t = num(m.rest_len), num(m.rest_vor), num(m.dt), num(m.damp_t)
    eps_len = zero if "no_eps_length" in mut else num(m.eps_length)
    shift = zero if "no_acos_shift" in mut else num(m.acos_shift)
    eps_sin = zero if "no_eps_sin" in mut else num(m.eps_sin)
    third = zero if ("planar_no_shift_third" in mut or "no_acos_shift" in mut) else num(m.acos_shift) / num(3.0)
    info = SimpleNamespace(e=[], stress=[], shear_couple=[], dilatation=[], couple=[], damper=[], x0=[])
    ln, tang, e, qt, npl, cs = [], [], [], [], [], []
    for k in range(n):
        lk = sqrt(d[k][0] * d[k][0] + d[k][1] * d[k][1]) + eps_len
        tk = [d[k][0] / lk, d[k][1] / lk]
        ek = lk / rest_len
        q0, q2 = c[k] * tk[1] - s[k] * tk[0], s[k] * tk[1] + c[k] * tk[0]
        n0, n2 = num(m.shear01[k]) * q0, num(m.shear2[k]) * (q2 - one / ek)
        ln.append(lk); tang.append(tk); e.append(ek); qt.append((q0, q2)); npl.append((n0, n2))
        cs.append([c[k] * n2 - s[k] * n0, s[k] * n2 + c[k] * n0])
        info.e.append(ek)
        info.stress.append(max(num(m.shear01[k]) * abs(q0), num(m.shear2[k]) * max(abs(q2), one / ek)))
    up = []
    for j in range(n - 1):
        D = dl[j]
        kappa = D * (one + third) * (one - eps_sin / sqrt(D * D + num(2.0) * shift)) / rest_vor if (eps_sin != 0) else \
            D * (one + third) / rest_vor
        vd = (ln[j + 1] + ln[j]) / rest_vor * (one if "voronoi_no_half" in mut else half)
        e3 = one / (vd * vd) if "couple_e2" in mut else one / (vd * vd * vd)
        up.append(num(m.bend01[j]) * kappa * e3)
        info.couple.append(num(m.bend01[j]) / rest_vor * e3 * max(one, abs(D)))
    v_new, wz_new = [], []
    g = [num(a) for a in m.gravity]
    for k in range(n + 1):
        mass = num(m.mass[k])
        cf = damp_t * dt / mass
        fe = [g[0] * mass, g[1] * mass]
        if k == 0:
            fe[0] = num(m.point_force)
        csk = cs[k] if k < n else [zero, zero]
        csp = cs[k - 1] if k >= 1 else [zero, zero]
        vk = [damp_t * v[k][i] + cf * (csk[i] - csp[i]) + cf * fe[i] for i in range(2)]
        if k == 0:
            vk[1] = damp_t * v[0][1]            # the pinned component: its force coefficient is zero
        v_new.append(vk)
    for k in range(n):
        q0, q2 = qt[k]
        n0, n2 = npl[k]
        lever = rest_len if "lever_rest_len" in mut else ln[k]
        tq = (up[k] if k < n - 1 else zero) - (up[k - 1] if k >= 1 else zero) + lever * (q2 * n0 - q0 * n2)
        tdv = tang[k][0] * dv[k][0] + tang[k][1] * dv[k][1]
        il = one if "dilatation_il" in mut else one / ln[k]
        dil = num(m.J0[k]) * rest_len / ln[k] * il * tdv * wz[k]
        tq = tq + dil
        ex = one if "damper_e1" in mut else e[k]
        damp = A.exp(num(m.dlog0[k]) * ex)
        wz_new.append((wz[k] + dt * num(m.invJ0[k]) * e[k] * tq) * damp)
        info.shear_couple.append(ln[k] * max(abs(q0), abs(q2)) * max(num(m.shear01[k]) * abs(q0),
                                                                       num(m.shear2[k]) * max(abs(q2), one / e[k])))
        info.dilatation.append(abs(dil))
        info.damper.append(damp)
        info.x0.append(num(m.dlog0[k]) * e[k])
    src = v if "planar_old_dv" in mut else v_new
    dv_new = [[src[k + 1][i] - src[k][i] for i in range(2)] for k in range(n)]
    return SimpleNamespace(v=v_new, wz=wz_new, t=tang, dv=dv_new, up=up, info=info)


def planar_to_3d(rod, exact=False):
    """The 3-D state of a planar rod: d1 = (-s2 s, s2 c, 0), d2 = (0, 0, s2), d3 = (c, s, 0), omega = (0, s2 wz, 0), the
    pendulum's mask.  exact: c, s are taken as the rod holds them (50-digit numbers of planar_exact)."""
    n, s2 = rod.n, rod.s2
    z = 0.0
    Q = [[-s2 * rod.s[k], s2 * rod.c[k], z, z, z, s2, rod.c[k], rod.s[k], z] for k in range(n)]
    out = SimpleNamespace(n=n, mat=rod.mat, kind=rod.kind, x=[[p[0], p[1], z] for p in rod.x], v=[[p[0], p[1], z] for p in rod.v], Q=Q,
                          w=[[z, s2 * rod.wz[k], z] for k in range(n)], rk=[[z] * 3 for _ in range(n - 1)])
    if not exact:
        for k in ("x", "v", "Q", "w", "rk"):
            setattr(out, k, np.array(getattr(out, k), float))
    return out


def planar_exact(rod):
    """The planar rod with (c, s) = (cos, sin) of the fp64 director's angle at 50 digits and D recomputed from them: the
    state on which the header's claims are exact statements (planar_gap)."""
    phi = [MP.atan2(MP.mpf(float(s)), MP.mpf(float(c))) for c, s in zip(rod.c, rod.s)]
    out = SimpleNamespace(**vars(rod))
    out.c, out.s = [MP.cos(p) for p in phi], [MP.sin(p) for p in phi]
    out.dl = []
    for k in range(rod.n - 1):
        D = phi[k + 1] - phi[k]
        D = D - 2 * MP.pi * MP.nint(D / (2 * MP.pi))
        out.dl.append(D)
    return out


def planar_gap(rod):
    """P against L at 50 digits on planar_exact(rod) -> per vertex (relative couple difference, D), and the largest
    relative difference of everything else (v, t; the rate less what the couples explain)."""
    ex = planar_exact(rod)
    p = planar_law(ex, MPF)
    l3 = planar_to_3d(ex, exact=True)
    lref = literal_law(l3, MPF, features=SOFTPENDULUM)
    m, n, s2 = rod.mat, rod.n, rod.s2
    # L's couple about d2 (= s2 e_z) per vertex, from its kappa: B kappa / vd^3
    couples = []
    for j in range(n - 1):
        ln0 = MP.sqrt(sum(MP.mpf(float(c)) ** 2 for c in rod.d[j])) + MP.mpf(m.eps_length)
        ln1 = MP.sqrt(sum(MP.mpf(float(c)) ** 2 for c in rod.d[j + 1])) + MP.mpf(m.eps_length)
        vd = (ln0 + ln1) / (2 * MP.mpf(m.rest_vor))
        cl = s2 * MP.mpf(float(m.bend01[j])) * lref.kap[j][1] / vd ** 3
        D = ex.dl[j]
        rel = abs(cl - p.up[j]) / abs(p.up[j]) if p.up[j] != 0 else abs(cl)
        couples.append((rel, D, abs(cl - p.up[j])))
    other = MP.mpf(0)
    for k in range(n + 1):
        for i in range(2):
            other = max(other, abs(lref.v[k][i] - p.v[k][i]) / max(abs(p.v[k][i]), MP.mpf(1e-300)))
        other = max(other, abs(lref.v[k][2]))
    for k in range(n):
        for i in range(2):
            other = max(other, abs(lref.t[k][i] - p.t[k][i]))
        explained = sum(c[2] for j, c in enumerate(couples) if j in (k - 1, k))
        cw = MP.mpf(m.dt) * MP.mpf(float(m.invJ0[k])) * p.info.e[k] * p.info.damper[k]
        rest = abs(s2 * lref.w[k][1] - p.wz[k]) - cw * explained
        other = max(other, rest / max(abs(p.wz[k]), MP.mpf(1e-300)), abs(lref.w[k][0]), abs(lref.w[k][2]))
    return couples, other


# ---------------------------------------------------------------------------------------------------------------
# crafted rods
# ---------------------------------------------------------------------------------------------------------------
def _rot(axis, theta):
    """Rotation matrix (mpmath) about the unit axis by theta, right-handed."""
    a = [MP.mpf(c) for c in axis]
    nrm = MP.sqrt(sum(c * c for c in a))
    a = [c / nrm for c in a]
    cth, sth = MP.cos(MP.mpf(theta)), MP.sin(MP.mpf(theta))
    K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    return [[(cth if i == j else 0) + sth * K[i][j] + (1 - cth) * a[i] * a[j] for j in range(3)] for i in range(3)]


def _matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


_AXIS = {"d3": (0.0, 0.0, 1.0), "d1": (1.0, 0.0, 0.0), "generic": (0.36, -0.48, 0.8)}


def make_rod(name, n, mat, r, kind="walk", lift=0.0):
    """Rod r of a case.  kind: 'walk' (every list, generic rates), 'zeros' (the same, v = w = 0), 'hot', 'hot_zeros',
    'one_theta', 'one_stretch' (see the module's docstring)."""
    rng = np.random.default_rng(M.hash_name(f"dyn/{name}/{r}"))
    hot = kind in ("hot", "hot_zeros", "one_theta", "one_stretch")
    thetas, stretches = (HOT_THETAS, HOT_STRETCHES) if hot else (THETAS, STRETCHES)
    tilts = TILTS[:2] if hot else TILTS
    Q0 = _matmul(_rot((0.3, 0.5, -0.7), 0.4 + 0.37 * r), [[MP.mpf(int(i == j)) for j in range(3)] for i in range(3)])
    Qs_mp, Qs = [Q0], [np.array([[float(c) for c in row] for row in Q0])]
    for j in range(n - 1):
        th = thetas[(j + r) % len(thetas)]
        if kind == "one_theta" and j == (n - 1) // 2:
            th = 2.0
        if th == 0.0:
            Qs_mp.append(Qs_mp[-1])
            Qs.append(Qs[-1].copy())                   # identical directors, bit for bit
            continue
        ax = _AXIS[AXES[(j + r // 2) % 3]]
        # relative rotation E about an axis given in the material frame: Q+ = E Q, so Q+ Q^T = E and vec = 2 sin(theta) axis
        Qn = _matmul(_rot(ax, th), [[MP.mpf(c) for c in row] for row in Qs[-1]])
        Qs_mp.append(Qn)
        Qs.append(np.array([[float(c) for c in row] for row in Qn]))
    x = np.zeros((n + 1, 3))
    x[0] = (0.1, -0.2, 0.3 + lift)
    for k in range(n):
        e = stretches[(k + 2 * r) % len(stretches)]
        if kind == "one_stretch" and k == n // 2:
            e = 2.0
        tilt = tilts[(k + r) % len(tilts)]
        phi = 0.7 * k + r
        d1, d2, d3 = Qs[k]
        direction = math.cos(tilt) * d3 + math.sin(tilt) * (math.cos(phi) * d1 + math.sin(phi) * d2)
        x[k + 1] = x[k] + (e * mat.rest_len) * direction
    if kind in ("zeros", "hot_zeros"):
        v, w = np.zeros((n + 1, 3)), np.zeros((n, 3))
    else:
        v, w = 0.1 * rng.normal(size=(n + 1, 3)), 5.0 * rng.normal(size=(n, 3))
    rk = 3.0 * rng.normal(size=(n - 1, 3))
    return SimpleNamespace(n=n, mat=mat, kind=kind, x=x, v=v, Q=np.array([q.ravel() for q in Qs]), w=w, rk=rk)


@dataclass(frozen=True)
class DynCase:
    name: str
    n: int
    epl: int          # the slot count the case is made for (its size class); forms of other slot counts may run it too
    taper: bool
    lifted: bool
    rods: tuple
    mat: object


GROUPS = ("walk", "hot", "dragged")


def _kinds(n, group):
    """The rods of a case: one case per size and tier group, so that a budget is the budget of the tier taken."""
    if group == "walk":
        return ["walk"] * (12 if n <= 5 else 3) + ["zeros"]
    if group == "hot":
        return ["hot", "hot", "hot_zeros"]
    return ["one_theta", "one_stretch"]


SIZES = ((1, False, (2, 5, 63)), (2, False, (5, 64, 101, 126, 127)), (1, True, (5, 63)))
# 127 elements fill the two-slot wave (node 127 in the last slot); the probe's own bound admits them, the shipped rows stop
# at 126 (config_why_not), which is kept beside it.


@functools.lru_cache(maxsize=None)
def dyn_cases():
    cases = {}
    for epl, taper, sizes in SIZES:
        for n in sizes:
            for group in GROUPS:
                for lifted in (False, True):
                    name = f"{'taper' if taper else 'epl%d' % epl}/n{n}/{group}" + ("/lifted" if lifted else "")
                    mat = material(n, "arm", taper)
                    rods = tuple(make_rod(name, n, mat, r, kind, lift=1.0 if lifted else 0.0)
                                 for r, kind in enumerate(_kinds(n, group)))
                    cases[name] = DynCase(name, n, epl, taper, lifted, rods, mat)
    # the same planar states through the 3-D form (SoftPendulum's mask less its BC)
    for pname in FROM_PLANAR:
        pc = planar_cases()[pname]
        cases["from-" + pname] = DynCase("from-" + pname, pc.n, pc.epl, False, False,
                                         tuple(planar_to_3d(rod) for rod in pc.rods), pc.mat)
    return cases


FROM_PLANAR = ("planar1/n5/walk/s2+", "planar1/n63/hot/s2-", "planar2/n64/walk/s2-")
PENDULUM_FREE = GRAVITY | POINT_FORCE | DAMPER


def case_masks(case):
    if case.name.startswith("from-"):
        return ["pendulum"]
    return ["arm"] if case.lifted else list(MASKS)


def case_forms(case):
    """(form, mask name) pairs of a case: the run-time forms under the three masks on the rods near the origin, the
    compiled arm mask (and the run-time form with the same mask) on the lifted ones."""
    if case.name.startswith("from-"):
        return [(RT1 if case.epl == 1 else RT2, "pendulum")]
    if case.taper:
        rt, arm = [RT_TAPER1], [ARM_TAPER1]
    elif case.epl == 1:
        rt, arm = [RT1] + ([RT2] if case.n in (5, 63) else []), [ARM1] + ([ARM2] if case.n in (5, 63) else [])
    else:
        rt, arm = [RT2] + ([RT1] if case.n == 5 else []), [ARM2] + ([ARM1] if case.n == 5 else [])
    if case.lifted:
        return [(f, "arm") for f in arm] + [(rt[0], "arm")]
    return [(f, k) for f in rt for k in MASKS]


def mask_features(mask):
    if mask == "pendulum":
        return PENDULUM_FREE
    return ARM_SINGLE | PLANE_ZUP if mask == "arm" else MASKS[mask]


def _np(a):
    return np.array([[float(c) for c in row] for row in a], float)


def dyn_scales(rod, ref, features):
    """(node (n + 1), element (n), tangent (n), kappa (n - 1)) scales from the 50-digit run."""
    m, n, I = rod.mat, rod.n, ref.info
    f = lambda a: np.array([float(c) for c in a])
    stress, e, damper = f(I.stress), f(I.e), f(I.damper)
    cf = m.damp_t * m.dt / np.asarray(m.mass)
    adj = np.maximum(np.concatenate([stress, [0.0]]), np.concatenate([[0.0], stress]))
    ca = cf * np.abs(np.asarray(m.mass)) * max(abs(g) for g in m.gravity) if features & GRAVITY else 0.0 * cf
    if features & POINT_FORCE:
        ca[0] = max(ca[0], cf[0] * abs(m.point_force))
    node = m.damp_t * np.abs(rod.v).max(axis=1) + cf * adj + ca
    couple, kxbk = f(I.couple), f(I.kxbk)
    pad = lambda a: np.maximum(np.concatenate([a, [0.0]]), np.concatenate([[0.0], a]))
    term = np.max([pad(couple), pad(kxbk), f(I.shear_couple), f(I.transport), f(I.dilatation)], axis=0)
    elem = damper * (np.abs(rod.w).max(axis=1) + m.dt * np.asarray(m.invJ0) * e * term)
    kap = m.inv_rest_vor * np.maximum(1.0, f(I.tos))
    return node, elem, np.ones(n), kap


def _err(got, ref, scale):
    """max over the components of |got - ref| / (2^-52 scale), per slot; the difference at 50 digits."""
    out = np.zeros(len(ref))
    for k, (g, r) in enumerate(zip(got, ref)):
        out[k] = max(float(abs(MP.mpf(float(a)) - b)) for a, b in zip(np.atleast_1d(g), r)) / (ULP * scale[k])
    return out


def dyn_errors(rod, ref, scales, out):
    """out: namespace / dict with v, w, t, kap (arrays or nested lists of floats) -> errors per output, budget units."""
    get = (lambda k: out[k]) if isinstance(out, dict) else (lambda k: getattr(out, k))
    return {k: _err(get(k), getattr(ref, k), s) for k, s in zip(("v", "w", "t", "kap"), scales)}


OUTPUTS = ("v", "w", "t", "kap")


@functools.lru_cache(maxsize=None)
def dyn_reference(name, mask):
    """Per rod of the case: (50-digit run, scales)."""
    case, feat = dyn_cases()[name], mask_features(mask)
    out = []
    for rod in case.rods:
        ref = literal_law(rod, MPF, features=feat)
        out.append((ref, dyn_scales(rod, ref, feat)))
    return out


@functools.lru_cache(maxsize=None)
def dyn_budget(name, mask):
    """{output: {"baseline", "budget"}}: the worse of the float run and the NumPy twin over the case's rods; 4 x, floor 8."""
    case, feat = dyn_cases()[name], mask_features(mask)
    base = {k: 0.0 for k in OUTPUTS}
    for rod, (ref, scales) in zip(case.rods, dyn_reference(name, mask)):
        for run in (literal_law(rod, FLOAT, features=feat), twin(rod, feat)):
            for k, e in dyn_errors(rod, ref, scales, run).items():
                base[k] = max(base[k], float(e.max()) if len(e) else 0.0)
    return {k: {"baseline": b, "budget": max(8.0, 4.0 * b)} for k, b in base.items()}


def contact_is_zero(rod):
    """rod_probe_ref.contact_law on the lifted rod's state: the reference contact force and torque are exactly zero."""
    m, n = rod.mat, rod.n
    ref = literal_law(rod, FLOAT, features=ARM_SINGLE)
    d = rod.x[1:] - rod.x[:-1]
    ln = np.sqrt((d * d).sum(axis=1)) + m.eps_length
    tw = twin(rod, ARM_SINGLE)
    F = tw.f_int + np.asarray(m.gravity)[None, :] * np.asarray(m.mass)[:, None]
    crod = SimpleNamespace(n=n, par=m.contact, x=rod.x, v=rod.v, F=F, tq=tw.t_int, w=rod.w, t=_np(ref.t), Q=rod.Q, len=ln,
                           r0s=m.r0s, mass=m.mass, l_rest=m.rest_len)
    fc, dt, _ = R.contact_law(crod, R.FLOAT)
    return all(c == 0.0 for row in fc for c in row) and all(c == 0.0 for row in dt for c in row)


def tiers(rod, ref):
    """From the 50-digit run: the wave's theta_over_sin tier (0..3) and exp_pair tier (0..2), the tiers the single joints
    / elements fall in."""
    I = ref.info
    y = np.array([float(c) for c in I.y])
    x0, x2 = np.array([float(c) for c in I.x0]), np.array([float(c) for c in I.x2])
    joint = {int(np.searchsorted(M.THETA_EDGES, v, side="right")) for v in y}
    elem = {int(np.searchsorted(M.EXP_EDGES, max(abs(a), abs(b)), side="right")) for a, b in zip(x0, x2)}
    return (M.theta_tier(y, np.ones(len(y), bool)), M.exp_pair_tier(x0, x2, np.ones(len(x0), bool)), joint, elem)


# ---------------------------------------------------------------------------------------------------------------
# planar rods
# ---------------------------------------------------------------------------------------------------------------
GRID = 2.0 ** -40      # edge vectors and positions on this grid: x[k + 1] - x[k] == d exactly in fp64
VGRID = 2.0 ** -30     # velocities on this one: dv == v[k + 1] - v[k] exactly


def make_planar_rod(name, n, mat, r, kind="walk", s2=1.0):
    rng = np.random.default_rng(M.hash_name(f"planar/{name}/{r}"))
    hot = kind in ("hot", "hot_zeros")
    stretches = HOT_STRETCHES if hot else STRETCHES
    tilts = TILTS[:2] if hot else TILTS
    dls = PLANAR_DL[:5] if hot else PLANAR_DL
    dl = np.array([dls[(j + 3 * r) % len(dls)] for j in range(n - 1)])
    phi = np.concatenate([[0.3 + 0.41 * r], 0.3 + 0.41 * r + np.cumsum(dl)])
    c = np.array([float(MP.cos(MP.mpf(p))) for p in phi])
    s = np.array([float(MP.sin(MP.mpf(p))) for p in phi])
    d = np.zeros((n, 2))
    for k in range(n):
        e = stretches[(k + 2 * r) % len(stretches)]
        a = phi[k] + tilts[(k + r) % len(tilts)] * (1 if k % 2 else -1)
        d[k] = np.round(e * mat.rest_len * np.array([math.cos(a), math.sin(a)]) / GRID) * GRID
    x = np.zeros((n + 1, 2))
    x[0] = (np.round(0.25 / GRID) * GRID, 0.0)
    for k in range(n):
        x[k + 1] = x[k] + d[k]
    assert np.array_equal(x[1:] - x[:-1], d)
    if kind in ("zeros", "hot_zeros"):
        v, wz = np.zeros((n + 1, 2)), np.zeros(n)
    else:
        v, wz = np.round(0.1 * rng.normal(size=(n + 1, 2)) / VGRID) * VGRID, 5.0 * rng.normal(size=n)
    v[0, 1] = 0.0                      # the pendulum constraint's invariant
    dv = v[1:] - v[:-1]
    return SimpleNamespace(n=n, mat=mat, kind=kind, x=x, v=v, c=c, s=s, wz=wz, dl=dl, d=d, dv=dv, s2=s2)


@dataclass(frozen=True)
class PlanarCase:
    name: str
    n: int
    epl: int
    rods: tuple
    mat: object
    s2: float
    halvings: int      # exp_one's loop trips for this case's wave (0: the polynomial's range)


PLANAR_SIZES = ((1, (2, 5, 63)), (2, (64, 127)))
STRONG_DAMPING = 2.0e-2      # ten times SoftPendulum's: xl len leaves exp_one's polynomial range


@functools.lru_cache(maxsize=None)
def planar_cases():
    cases = {}
    for epl, sizes in PLANAR_SIZES:
        for n in sizes:
            for s2 in (1.0, -1.0):
                for group in ("walk", "hot"):
                    name = f"planar{epl}/n{n}/{group}/s2{'+' if s2 > 0 else '-'}"
                    mat = material(n, "pendulum", features=SOFTPENDULUM)
                    mat.point_force = 7.25
                    kinds = ["walk"] * (11 if n <= 5 else 3) + ["zeros"] if group == "walk" else ["hot", "hot", "hot_zeros"]
                    rods = tuple(make_planar_rod(name, n, mat, r, k, s2) for r, k in enumerate(kinds))
                    cases[name] = PlanarCase(name, n, epl, rods, mat, s2, 0)
    mat = material(5, "pendulum", features=SOFTPENDULUM, damping=STRONG_DAMPING)
    mat.point_force = -3.5
    rods = tuple(make_planar_rod("planar1/n5/damped", 5, mat, r, "walk", 1.0) for r in range(4))
    x = np.concatenate([np.asarray(rods[0].mat.dlog0) * np.sqrt((rod.d ** 2).sum(axis=1)) / mat.rest_len for rod in rods])
    cases["planar1/n5/damped"] = PlanarCase("planar1/n5/damped", 5, 1, rods, mat, 1.0, M.exp_one_halvings(x))
    return cases


def planar_scales(rod, ref):
    """(node, rate, tangent, dv) scales from P's 50-digit run."""
    m, n, I = rod.mat, rod.n, ref.info
    f = lambda a: np.array([float(c) for c in a])
    stress, e, damper = f(I.stress), f(I.e), f(I.damper)
    cf = m.damp_t * m.dt / np.asarray(m.mass)
    adj = np.maximum(np.concatenate([stress, [0.0]]), np.concatenate([[0.0], stress]))
    fe = np.abs(np.asarray(m.mass)) * max(abs(g) for g in m.gravity)
    fe[0] = max(fe[0], abs(m.point_force))
    node = m.damp_t * np.abs(rod.v).max(axis=1) + cf * adj + cf * fe
    couple = f(I.couple)
    pad = lambda a: np.maximum(np.concatenate([a, [0.0]]), np.concatenate([[0.0], a])) if len(a) else np.zeros(1)
    term = np.max([pad(couple), f(I.shear_couple), f(I.dilatation)], axis=0)
    rate = damper * (np.abs(rod.wz) + m.dt * np.asarray(m.invJ0) * e * term)
    return node, rate, np.ones(n), np.maximum(node[1:], node[:-1])


PLANAR_OUTPUTS = ("v", "wz", "t", "dv")


def planar_errors(ref, scales, out):
    get = (lambda k: out[k]) if isinstance(out, dict) else (lambda k: getattr(out, k))
    res = {}
    for k, s in zip(PLANAR_OUTPUTS, scales):
        r = getattr(ref, k)
        if k == "wz":
            r = [[c] for c in r]
        res[k] = _err(get(k), r, s)
    return res


@functools.lru_cache(maxsize=None)
def planar_reference(name):
    return [(ref, planar_scales(rod, ref)) for rod in planar_cases()[name].rods
            for ref in (planar_law(rod, MPF),)]


def literal_as_planar(rod, A):
    """L on the planar rod's 3-D state, read back as P's outputs."""
    l3 = planar_to_3d(rod)
    ref = literal_law(l3, A, features=SOFTPENDULUM)
    v = [row[:2] for row in ref.v]
    return SimpleNamespace(v=v, wz=[rod.s2 * row[1] for row in ref.w], t=[row[:2] for row in ref.t],
                           dv=[[v[k + 1][i] - v[k][i] for i in range(2)] for k in range(rod.n)])


@functools.lru_cache(maxsize=None)
def exp_one_recorded():
    """profiles/math_primitives_error.json: exp_one's measured error (2^-52) by loop trips."""
    rec = json.loads((ROOT / "profiles" / "math_primitives_error.json").read_text())
    rows = rec["records"] if isinstance(rec, dict) and "records" in rec else rec
    for row in _walk(rows):
        if isinstance(row, dict) and row.get("case") == "exp_one/halved" and "device_by_trips" in row:
            return {int(k): float(v) for k, v in row["device_by_trips"].items()}
    raise KeyError("exp_one/halved")


def _walk(o):
    if isinstance(o, dict):
        yield o
        for v in o.values():
            yield from _walk(v)
    elif isinstance(o, list):
        for v in o:
            yield from _walk(v)


@functools.lru_cache(maxsize=None)
def planar_budget(name):
    """Baseline: the float runs of P and of L, each against its own 50-digit run, in P's scales; 4 x, floor 8; the rate
    of a case outside exp_one's polynomial range gets exp_one's recorded error at its trip count on top."""
    case = planar_cases()[name]
    base = {k: 0.0 for k in PLANAR_OUTPUTS}
    for rod, (ref, scales) in zip(case.rods, planar_reference(name)):
        runs = ((planar_law(rod, FLOAT), ref), (literal_as_planar(rod, FLOAT), literal_as_planar(rod, MPF)))
        for run, own in runs:
            for k, e in planar_errors(own, scales, run).items():
                base[k] = max(base[k], float(e.max()))
    out = {k: {"baseline": b, "budget": max(8.0, 4.0 * b)} for k, b in base.items()}
    if case.halvings:
        out["wz"]["exp_one"] = exp_one_recorded()[case.halvings]
        out["wz"]["budget"] += out["wz"]["exp_one"]
    return out


# ---------------------------------------------------------------------------------------------------------------
# the probe's arrays
# ---------------------------------------------------------------------------------------------------------------
BEHIND = ("clean", "poison", "continued")
_BAD = np.array([np.nan, np.inf, -np.inf, 1.0e300, -1.0e300])


def dyn_layout(case, epl, behind="clean", seed=5):
    """The case's rods as the probe's arrays (rods, 64 epl, components).  behind: what the slots behind each rod hold in
    x, v (past node n) and Q, w, rk (past element n - 1): zeros, NaN / +-inf / +-1e300, or a finite continuation.  The
    finite continuation of rk starts one slot earlier, at vertex slot n - 1, the one vertex slot behind the rod whose
    value meets a valid output (b01 = 0 times (kappa - rk) in the last element's couple); the poison does not: nothing
    masks that slot, and a step in sanitize_unused_slots that would costs the per-env contact + material kernel a
    register its uniform twin does not need (tests/test_env_contact.py holds the two alike) — DESIGN.md section 3."""
    W, n, rods = WAVE * epl, case.n, case.rods
    rng = np.random.default_rng(seed)
    a = {k: np.zeros((len(rods), W, c)) for k, c in (("x", 3), ("v", 3), ("Q", 9), ("w", 3), ("rk", 3))}
    for r, rod in enumerate(rods):
        a["x"][r, :n + 1], a["v"][r, :n + 1] = rod.x, rod.v
        a["Q"][r, :n], a["w"][r, :n], a["rk"][r, :n - 1] = rod.Q, rod.w, rod.rk
        nodes, elems = W - (n + 1), W - n
        if behind == "poison":
            a["x"][r, n + 1:], a["v"][r, n + 1:] = rng.choice(_BAD, (nodes, 3)), rng.choice(_BAD, (nodes, 3))
            a["Q"][r, n:], a["w"][r, n:], a["rk"][r, n:] = (rng.choice(_BAD, (elems, c)) for c in (9, 3, 3))
        elif behind == "continued":
            step = rod.x[n] - rod.x[n - 1]
            a["x"][r, n + 1:] = rod.x[n] + np.arange(1, nodes + 1)[:, None] * step
            a["v"][r, n + 1:] = rng.normal(size=(nodes, 3)) * 1e-3
            a["Q"][r, n:] = np.stack([R._random_rotation(rng).ravel() for _ in range(elems)]) if elems else 0.0
            a["w"][r, n:], a["rk"][r, n - 1:] = rng.normal(size=(elems, 3)), rng.normal(size=(elems + 1, 3))   # (finite: from n - 1)
    return a


def planar_layout(case, behind="clean", seed=5):
    """The same for the planar probe: fillings in x, v past node n, in c, s, wz past element n - 1 and in dl past vertex
    n - 2 (slot n - 1: bk = 0 times dl there goes into the last element's couple) — and in d, dv past element n - 1 too, which
    the step kernel forms from x and v behind the rod."""
    W, n, rods = WAVE * case.epl, case.n, case.rods
    rng = np.random.default_rng(seed)
    a = {k: np.zeros((len(rods), W, c)) for k, c in (("x", 2), ("v", 2), ("c", 1), ("s", 1), ("wz", 1), ("dl", 1),
                                                    ("d", 2), ("dv", 2))}
    for r, rod in enumerate(rods):
        a["x"][r, :n + 1], a["v"][r, :n + 1] = rod.x, rod.v
        a["d"][r, :n], a["dv"][r, :n] = rod.d, rod.dv
        for k in ("c", "s", "wz"):
            a[k][r, :n, 0] = getattr(rod, k)
        a["dl"][r, :n - 1, 0] = rod.dl
        nodes, elems = W - (n + 1), W - n
        if behind == "poison":
            a["x"][r, n + 1:], a["v"][r, n + 1:] = rng.choice(_BAD, (nodes, 2)), rng.choice(_BAD, (nodes, 2))
            for k in ("c", "s", "wz"):
                a[k][r, n:] = rng.choice(_BAD, (elems, 1))
            a["dl"][r, n - 1:] = rng.choice(_BAD, (elems + 1, 1))
            a["d"][r, n:], a["dv"][r, n:] = rng.choice(_BAD, (elems, 2)), rng.choice(_BAD, (elems, 2))
        elif behind == "continued":
            a["x"][r, n + 1:] = rod.x[n] + np.arange(1, nodes + 1)[:, None] * rod.d[n - 1]
            a["v"][r, n + 1:] = rng.normal(size=(nodes, 2)) * 1e-3
            ang = rng.uniform(-3.0, 3.0, elems)
            a["c"][r, n:, 0], a["s"][r, n:, 0] = np.cos(ang), np.sin(ang)
            a["wz"][r, n:, 0], a["dl"][r, n - 1:, 0] = rng.normal(size=elems), rng.normal(size=elems + 1) * 0.1
            a["d"][r, n:] = rod.d[n - 1]
            a["dv"][r, n:] = rng.normal(size=(elems, 2)) * 1e-3
    return a


# argument checks of the two entry points: (what, overrides) — the GPU test drives them, the CPU test holds the list
BAD_DYNAMIC = (("unknown form", {"form": N_FORMS}), ("negative form", {"form": -1}), ("no rods", {"n_rods": 0}),
               ("too many rods", {"n_rods": 1025}), ("one element", {"n_elem": 1}),
               ("65 nodes in 64 lanes", {"form": RT1, "n_elem": 64}), ("129 nodes in 128 slots", {"form": RT2, "n_elem": 128}),
               ("no parameters", {"par": None}), ("no x", {"x": None}), ("no Q", {"Q": None}), ("no rk", {"rk": None}),
               ("no v_out", {"v_out": None}), ("no kap_out", {"kap_out": None}),
               ("tapered form without a table", {"form": RT_TAPER1, "mat": None}))
BAD_PLANAR = (("epl 3", {"epl": 3}), ("epl 0", {"epl": 0}), ("no rods", {"n_rods": 0}), ("too many rods", {"n_rods": 1025}),
              ("one element", {"n_elem": 1}), ("65 nodes in 64 lanes", {"epl": 1, "n_elem": 64}),
              ("129 nodes in 128 slots", {"epl": 2, "n_elem": 128}), ("no parameters", {"par": None}),
              ("no c", {"c": None}), ("no dl", {"dl": None}), ("no dv", {"dv": None}), ("no wz_out", {"wz_out": None}))
