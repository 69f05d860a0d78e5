"""Cases, references and budgets for two per-element blocks of the 3-D FAST step kernels, evaluated alone through
csrc/probe/softrod_rod_probe.hip: the rod-plane contact law plane_contact_n (softrod_contact.hpp) and the kinematic
step kinematic_n (softrod_fast.hpp).  Shared by tests/test_rod_probe.py (CPU) and tests/test_gpu_rod_probe.py.

THE CONTACT LAW.  contact_law() is one scalar transcription of PyElastica's RodPlaneContactWithAnisotropicFriction, with
the structure of oracle/softrod_oracle_np.py (rod_plane_contact + rod_plane_contact_with_anisotropic_friction: selects,
masks, sign()-picked coefficients, divisions, the rolling direction as a cross product) and generic over the number
type.  In Python floats it is tied to the NumPy twin at 1e-12; in mpmath at 50 digits it is the reference.  It takes
the law's own arguments as the device gets them (t, len, r0 sqrt(l_rest) are inputs, not recomputed), so the device,
the float run and the twin differ from the reference by rounding alone.

The rods are crafted: every branch quantity of every element is placed — gap, sign of the normal force, axial speed,
rolling slip, axial push against its cap, no-slip rolling force against its cap — from lists that hold both signs,
exact zeros of both signs, the exact multiples 1.0, 1.3, 1.7, 2.0 of slip_velocity_tol and values far on either side,
drawn independently per element.  Node fields are shared by two elements, so nodes come in runs of two with the same
value: the element inside a run gets the run's value exactly, the one between two runs a blend (a value inside the
range).  The law is continuous across every threshold but one, so no element is excused: the one discontinuity, the
surface_tol cut, is approached to surface_tol (1 +- 1e-6) and no closer, and the CPU test verifies that the 50-digit
run and the float run take the same side for every element (the info records' `off`).

CONTACT BUDGET, measured on the reference side.  Per element the force scale is the largest of |any element force the
law forms| (50-digit intermediates), k (|dist| + radius) and nu |element velocity|; a node takes the larger scale of
its two elements; the torque scale is radius x force scale + max |tq in|.  Errors are in units of 2^-52 x scale.  The
float transcription and the NumPy twin — two roundings of the literal law, neither the code under test — give the
case's baselines (the larger maximum, for the force and for the torque separately); the FAST forms are held to 4 x baseline (x 2: fast_rcp / fast_rsqrt are good to
1 ulp where division and sqrt round to half; x 2: the FM form associates the same sums differently), floor 8; the
literal instantiation <1, false, false> to 2 x baseline, floor 8.

THE KINEMATIC STEP.  Reference: x + h hx v and R(h hq w) Q in mpmath with the exact product h hq w and the fp64 Q as
given (a rotation only to rounding), R in the kernel's (PyElastica's) sign convention.  Budgets, derived: positions
1 ulp of the result; Q, absolute in 2^-52: 3 in range (R's diagonal one rounding at magnitude 1, off-diagonals 0.03
relative ulps, each new entry a three-term fma chain of magnitudes <= 1: 1.5; together <= 2, held at 3); 2 (k + 3)
after k quarterings (sinc_cosc's 2 (k + 2), one more for the product with Q).  kin_budgets() applies the fall-back
rule: where the exactly rounded-fma transcription itself misses 2 (k + 3) the device is held to that transcription's
measured maximum + 2 instead, and the record says so.
t_kinematic() is kinematic_n's sequence with sinc_cosc<true, true>: behind the quartering tier the pair (sin, cos) is put
back on the unit circle to first order (t_sinc_cosc_on_circle), which is what keeps Q Q^T - I from growing faster than
the entries' error.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from tests import math_primitives_ref as M

MP = M.MP
ULP = M.ULP
WAVE = 64
MAX_WAVES = 16

# contact forms of the probe (enum ContactForm)
ZUP1, ZUP2, ZUP_TAPER1, ZUP_TAPER2, PLANE1, PLANE2, LITERAL1 = range(7)
N_FORMS = 7
FORM_NAMES = {ZUP1: "<1,zup,fm>", ZUP2: "<2,zup,fm>", ZUP_TAPER1: "<1,zup,fm,taper>", ZUP_TAPER2: "<2,zup,fm,taper>",
              PLANE1: "<1,plane,fm>", PLANE2: "<2,plane,fm>", LITERAL1: "<1,plane,literal>"}
FORM_EPL = {ZUP1: 1, ZUP2: 2, ZUP_TAPER1: 1, ZUP_TAPER2: 2, PLANE1: 1, PLANE2: 2, LITERAL1: 1}

K_CONTACT, NU_CONTACT, SLIP_TOL, SURFACE_TOL = 1.0e2, 1.0e1, 1.0e-8, 1.0e-4
_MU = 0.35 / (2.0 * 2.0 * 9.81 * 0.1)            # the octopus': L0 / (period^2 g froude)
MU_OCTOPUS = ((_MU, 1.5 * _MU, 2.0 * _MU), (2 * _MU, 2 * (1.5 * _MU), 2 * (2.0 * _MU)))     # backward > forward
MU_FORWARD = ((1.7 * _MU, 0.6 * _MU, 1.2 * _MU), (3.1 * _MU, 1.4 * _MU, 2.2 * _MU))        # forward > backward
L_REST = 0.02

MUTATIONS = ("swap_kinetic", "swap_static", "swap_end_weights", "half_end_nodes", "roll_negated", "third_half",
             "tax_once", "rest_radius", "ramp_3x", "damping_sign", "static_cap_kinetic", "one_radius", "arm_plus")


# ---------------------------------------------------------------------------------------------------------------
# the literal law, generic over the number type
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Arith:
    num: object
    sqrt: object


FLOAT = Arith(float, math.sqrt)
MPF = Arith(lambda v: MP.mpf(v), MP.sqrt)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sign(x):
    return (x > 0) - (x < 0)


def contact_law(rod, A=FLOAT, mut=()):
    """-> (fc[n + 1][3], torque added [n][3], info[n]).  rod: x, v, F (n + 1, 3); tq, w, t (n, 3); Q (n, 9) row-major;
    len, r0s (n); mass (n + 1); l_rest; par.  mut: names from MUTATIONS (the CPU test's teeth)."""
    num, sqrt = A.num, A.sqrt
    n, par = rod.n, rod.par
    half, one, zero, eps = num(0.5), num(1.0), num(0.0), num(1e-14)
    nrm = [num(c) for c in par.normal]
    org = [num(c) for c in par.origin]
    k, nu, slip_tol, surface_tol = num(par.k), num(par.nu), num(par.slip_tol), num(par.surface_tol)
    kin = [num(c) for c in par.kin_mu]
    stat = [num(c) for c in par.stat_mu]
    if "swap_kinetic" in mut:
        kin = [kin[1], kin[0], kin[2]]
    if "swap_static" in mut:
        stat = [stat[1], stat[0], stat[2]]
    cap_mu = kin if "static_cap_kinetic" in mut else stat

    def vecs(a):
        return [[num(c) for c in row] for row in a]

    x, v, F, tq, w, tang, Q = (vecs(a) for a in (rod.x, rod.v, rod.F, rod.tq, rod.w, rod.t, rod.Q))
    length = [num(c) for c in rod.len]
    mass = [num(c) for c in rod.mass]
    radius = []
    for e in range(n):
        r0s = num(rod.r0s[0 if "one_radius" in mut else e])
        radius.append(r0s / sqrt(num(rod.l_rest) if "rest_radius" in mut else length[e]))
    fext = [[zero] * 3 for _ in range(n + 1)]
    text = [[zero] * 3 for _ in range(n)]

    def node_to_element(f):                    # node_to_element_mass_or_force: the rod's two end nodes in full
        out = [[half * (f[e][i] + f[e + 1][i]) for i in range(3)] for e in range(n)]
        if "half_end_nodes" not in mut:
            first, last = (1, n - 1) if "swap_end_weights" in mut else (0, n)
            for i in range(3):
                out[0][i] = out[0][i] + half * f[first][i]
                out[n - 1][i] = out[n - 1][i] + half * f[last][i]
        return out

    def to_nodes(e, f):
        for i in range(3):
            fext[e][i] = fext[e][i] + half * f[i]
            fext[e + 1][i] = fext[e + 1][i] + half * f[i]

    def slipping(vec):                          # find_slipping_elements
        mag = sqrt(_dot(vec, vec))
        if abs(mag) > slip_tol:
            q = mag / slip_tol - one
            if "ramp_3x" in mut:
                q = q * half
            return abs(one - min(one, q))
        return one

    def q_mul(e, a):                            # Q a
        return [Q[e][3 * i] * a[0] + Q[e][3 * i + 1] * a[1] + Q[e][3 * i + 2] * a[2] for i in range(3)]

    def qt_mul(e, a):                           # Q^T a
        return [Q[e][i] * a[0] + Q[e][3 + i] * a[1] + Q[e][6 + i] * a[2] for i in range(3)]

    info = [SimpleNamespace() for _ in range(n)]
    # ---- rod_plane_contact ----
    total = node_to_element([[F[j][i] + fext[j][i] for i in range(3)] for j in range(n + 1)])
    mag, no_contact, elem_v = [], [], []
    for e in range(n):
        along = _dot(nrm, total[e])
        response = [-(nrm[i] * along) for i in range(3)]
        if along > 0:
            response = [zero] * 3
        ex = [half * (x[e + 1][i] + x[e][i]) for i in range(3)]
        dist = _dot(nrm, [ex[i] - org[i] for i in range(3)])
        gap = dist - radius[e]
        pen = min(gap, zero)
        elastic = [-k * (nrm[i] * pen) for i in range(3)]
        ev = [(mass[e + 1] * v[e + 1][i] + mass[e] * v[e][i]) / (mass[e + 1] + mass[e]) for i in range(3)]
        vn = _dot(nrm, ev)
        damping = [(nu if "damping_sign" in mut else -nu) * (nrm[i] * vn) for i in range(3)]
        tr = [response[i] + elastic[i] + damping[i] for i in range(3)]
        off = gap > surface_tol
        if off:
            response, tr = [zero] * 3, [zero] * 3
        to_nodes(e, tr)
        mag.append(sqrt(_dot(response, response)))
        no_contact.append(off)
        elem_v.append(ev)
        I = info[e]
        I.gap, I.off, I.along, I.radius = gap, off, along, radius[e]
        I.forces = [total[e], tr]
        I.floor = max(k * (abs(dist) + radius[e]), nu * sqrt(_dot(ev, ev)))
    # ---- anisotropic friction: kinetic ----
    axial, rolling, slip_ax, slip_ro, arms = [], [], [], [], []
    for e in range(n):
        I = info[e]
        tn = _dot(nrm, tang[e])
        in_plane = [tang[e][i] - nrm[i] * tn for i in range(3)]
        d = sqrt(_dot(in_plane, in_plane)) + eps
        ax = [c / d for c in in_plane]
        ev = elem_v[e]
        vam = _dot(ev, ax)
        v_axial = [vam * c for c in ax]
        sgn = _sign(vam)
        mu_k = half * (kin[0] * (1 + sgn) + kin[1] * (1 - sgn))
        sa = slipping(v_axial)
        ro = _cross(ax, nrm)
        if "roll_negated" in mut:
            ro = [-c for c in ro]
        arm = [-(c * radius[e]) for c in nrm]
        v_roll = _dot(ev, ro)
        spin = qt_mul(e, _cross(w[e], q_mul(e, arm)))
        srm = v_roll + _dot(spin, ro)
        slip_roll = [srm * c for c in ro]
        sr = slipping(slip_roll)
        unit = [slip_roll[i] + v_axial[i] for i in range(3)]
        um = sqrt(_dot([c + eps for c in unit], [c + eps for c in unit]))
        unit = [c / um for c in unit]
        c_ax = (one - sa) * mu_k * mag[e] * _dot(unit, ax)
        f = [-(c_ax * c) for c in ax]
        if no_contact[e]:
            f = [zero] * 3
        to_nodes(e, f)
        c_ro = (one - sr) * kin[2] * mag[e] * _dot(unit, ro)
        g = [-(c_ro * c) for c in ro]
        if no_contact[e]:
            g = [zero] * 3
        to_nodes(e, g)
        tarm = [-c for c in arm] if "arm_plus" in mut else arm
        dt = q_mul(e, _cross(tarm, g))
        text[e] = [text[e][i] + dt[i] for i in range(3)]
        axial.append(ax); rolling.append(ro); slip_ax.append(sa); slip_ro.append(sr); arms.append(tarm)
        I.forces += [f, g]
        I.slip_ax_arg = sqrt(_dot(v_axial, v_axial)) / slip_tol
        I.slip_ro_arg = sqrt(_dot(slip_roll, slip_roll)) / slip_tol
        I.vam, I.srm = vam, srm
    # ---- static ----
    total = node_to_element([[F[j][i] + fext[j][i] for i in range(3)] for j in range(n + 1)])
    for e in range(n):
        I = info[e]
        ax, ro = axial[e], rolling[e]
        push = _dot(total[e], ax)
        psgn = _sign(push)
        mu_s = half * (cap_mu[0] * (1 + psgn) + cap_mu[1] * (1 - psgn))
        fmax = slip_ax[e] * mu_s * mag[e]
        c_ax = min(abs(push), fmax) * psgn
        f = [-(c_ax * c) for c in ax]
        if no_contact[e]:
            f = [zero] * 3
        I.push, I.push_cap = push, fmax
        torques = qt_mul(e, [tq[e][i] + text[e][i] for i in range(3)])
        t_axial = _dot(torques, ax)
        f_roll = _dot(total[e], ro)
        noslip = -((radius[e] * f_roll - (1 if "tax_once" in mut else 2) * t_axial)
                   / (2 if "third_half" in mut else 3) / radius[e])
        fmax = slip_ro[e] * cap_mu[2] * mag[e]
        c_ro = min(abs(noslip), fmax) * _sign(noslip)
        g = [c_ro * c for c in ro]
        if no_contact[e]:
            g = [zero] * 3
        I.noslip, I.noslip_cap = noslip, fmax
        I.forces += [total[e], f, g]
        info[e].static = (f, g)
    for e in range(n):                          # (after every element has read the totals of round 1)
        f, g = info[e].static
        to_nodes(e, f)
        to_nodes(e, g)
        dt = q_mul(e, _cross(arms[e], g))
        text[e] = [text[e][i] + dt[i] for i in range(3)]
        I = info[e]
        I.fscale = max(I.floor, max(abs(c) for vec in I.forces for c in vec))
        I.tscale = I.radius * I.fscale + max(abs(c) for c in tq[e])
    return fext, text, info


def twin_rod(rod):
    """The rod as oracle/softrod_oracle_np.py's functions take it."""
    n = rod.n
    return SimpleNamespace(n=n, x=rod.x.T.copy(), v=rod.v.T.copy(), mass=rod.mass.copy(), tang=rod.t.T.copy(),
                           radius=rod.r0s / np.sqrt(rod.len), Q=np.transpose(rod.Q.reshape(n, 3, 3), (1, 2, 0)).copy(),
                           w=rod.w.T.copy(), f_int=rod.F.T.copy(), f_ext=np.zeros((3, n + 1)),
                           t_int=rod.tq.T.copy(), t_ext=np.zeros((3, n)))


def twin_law(rod):
    """The NumPy twin's function on the same arguments -> (fc (n + 1, 3), torque added (n, 3))."""
    from oracle.softrod_oracle_np import rod_plane_contact_with_anisotropic_friction

    r, p = twin_rod(rod), rod.par
    rod_plane_contact_with_anisotropic_friction(r, np.array(p.origin), np.array(p.normal), p.surface_tol, p.slip_tol,
                                                p.k, p.nu, np.array(p.kin_mu), np.array(p.stat_mu))
    return r.f_ext.T.copy(), r.t_ext.T.copy()


# ---------------------------------------------------------------------------------------------------------------
# crafted rods
# ---------------------------------------------------------------------------------------------------------------
# gap = dist - radius: penetrating, on either side of 0, inside surface_tol, at the cut's two sides, off the plane
GAPS = (-3.0e-4, -2.0e-5, -1.0e-9, 1.0e-9, 4.0e-5, SURFACE_TOL * (1 - 1e-6), SURFACE_TOL * (1 + 1e-6), 2.5e-4, 6.0e-4)
# multiples of slip_velocity_tol for the axial speed and the rolling slip: zeros of both signs, below, the ramp's ends
# and two points inside it (exact multiples), above, far above — both signs
SLIPS = (0.0, -0.0, 0.4, -0.4, 1.0, -1.0, 1.3, -1.3, 1.7, -1.7, 2.0, -2.0, 3.0, -3.0, 50.0, -50.0, 3.0e4, -3.0e4)
F_NORMAL = (-1.0e-2, 1.0e-2, -1.0e-3, 1.0e-3, -1.0e-5, 1.0e-5, -3.0e-3, 0.0, -0.0)
F_PLANE = (0.0, -0.0, 1.0e-8, -1.0e-8, 1.0e-6, -1.0e-6, 3.0e-5, -3.0e-5, 3.0e-4, -3.0e-4, 3.0e-3, -3.0e-3, 1.0e-2, -1.0e-2)
TORQUES = (0.0, -0.0, 1.0e-9, -1.0e-9, 1.0e-7, -1.0e-7, 1.0e-6, -1.0e-6, 1.0e-5, -1.0e-5, 1.0e-4, -1.0e-4)
V_NORMAL = (0.0, 1.0e-5, -1.0e-5, 1.0e-4, -1.0e-4, 1.0e-3, -1.0e-3)
SPIN_MODES = ("zero", "negative zero", "about the tangent", "shared", "opposed", "generic")


def _frame(normal):
    nrm = np.asarray(normal, float)
    if nrm[0] == 0.0 and nrm[1] == 0.0:
        return np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    e1 = np.cross(nrm, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(nrm, e1)


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_rod(rng, n, par, taper, sel):
    """One crafted rod.  sel: an integer that walks the first and the last element (and so the node in front of the
    slot behind the rod) through every list, so that over a family's rods the ends see every regime."""
    nrm = np.asarray(par.normal, float)
    origin = np.asarray(par.origin, float)
    e1, e2 = _frame(nrm)
    calls = [0]

    def pick(seq, e):
        if e != 0 and e != n - 1:
            return seq[rng.integers(len(seq))]
        calls[0] += 1                           # (each draw of an end element from another place of its list)
        return seq[(sel * (7 if e == 0 else 5) + 3 * calls[0] + sel // len(seq)) % len(seq)]

    r0 = 1.2e-2 * 10.0 ** (-np.arange(n) / max(n - 1, 1)) if taper else np.full(n, par.r0s_uniform / math.sqrt(L_REST))
    r0s = r0 * math.sqrt(L_REST) if taper else np.full(n, par.r0s_uniform)
    length = L_REST * (1.0 + rng.uniform(-0.06, 0.06, n))
    heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.uniform(-0.15, 0.15, n))
    # gaps in runs of two elements: the node heights z_{k+1} = 2 h_k - z_k then stay within a radius of the plane
    gap = np.empty(n)
    for e in range(0, n, 2):
        gap[e:e + 2] = pick(GAPS, e)
    gap[n - 1] = pick(GAPS, n - 1)
    ln = length.copy()
    for _ in range(4):                          # radius depends on len, len on the heights: a fixed point in two rounds
        h = r0s / np.sqrt(ln) + gap
        z = np.empty(n + 1)
        z[0] = h[0]
        for e in range(n):
            z[e + 1] = 2.0 * h[e] - z[e]
        dz = np.diff(z)
        assert np.all(np.abs(dz) < 0.8 * length)
        step = np.sqrt(length ** 2 - dz ** 2)
        a = np.concatenate([[0.0], np.cumsum(step * np.cos(heading))])
        b = np.concatenate([[0.0], np.cumsum(step * np.sin(heading))])
        x = origin + a[:, None] * e1 + b[:, None] * e2 + z[:, None] * nrm
        d = np.diff(x, axis=0)
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    t = d / ln[:, None]
    radius = r0s / np.sqrt(ln)
    in_plane = t - np.outer(t @ nrm, nrm)
    ipn = np.linalg.norm(in_plane, axis=1)
    ax = in_plane / ipn[:, None]
    ro = np.cross(ax, nrm)
    # node velocities in runs of two (nodes 2j, 2j + 1; the last two nodes too): the run's element gets them exactly
    v = np.empty((n + 1, 3))
    for j in range(0, n + 1, 2):
        e = min(j, n - 1)
        v[j:j + 2] = (pick(SLIPS, e) * SLIP_TOL) * ax[e] + (pick(SLIPS, e) * SLIP_TOL) * ro[e] + pick(V_NORMAL, e) * nrm
    e = n - 1
    v[n - 1:] = (pick(SLIPS, e) * SLIP_TOL) * ax[e] + (pick(SLIPS, e) * SLIP_TOL) * ro[e] + pick(V_NORMAL, e) * nrm
    # nodal forces in runs of two, one node later (nodes 2j - 1, 2j); the first and the last two nodes are runs
    F = np.empty((n + 1, 3))
    for j in range(-1, n + 1, 2):
        e = min(max(j, 0), n - 1)
        F[max(j, 0):j + 2] = pick(F_NORMAL, e) * nrm + pick(F_PLANE, e) * ax[e] + pick(F_PLANE, e) * ro[e]
    F[:2] = pick(F_NORMAL, 0) * nrm + pick(F_PLANE, 0) * ax[0] + pick(F_PLANE, 0) * ro[0]
    F[n - 1:] = pick(F_NORMAL, n - 1) * nrm + pick(F_PLANE, n - 1) * ax[n - 1] + pick(F_PLANE, n - 1) * ro[n - 1]
    Q = np.empty((n, 9))
    w = np.empty((n, 3))
    tq = np.empty((n, 3))
    m_elem = 1000.0 * np.pi * r0 ** 2 * L_REST
    mass = np.concatenate([[0.5 * m_elem[0]], 0.5 * (m_elem[1:] + m_elem[:-1]), [0.5 * m_elem[-1]]])
    for e in range(n):
        q = np.eye(3) if rng.integers(8) == 0 else _random_rotation(rng)
        Q[e] = q.ravel()
        mode = pick(SPIN_MODES, e)
        v_roll = ((mass[e + 1] * v[e + 1] + mass[e] * v[e]) / (mass[e + 1] + mass[e])) @ ro[e]
        target = pick(SLIPS, e) * SLIP_TOL
        if mode == "zero":
            w[e] = 0.0
        elif mode == "negative zero":
            w[e] = -0.0
        elif mode == "generic":
            w[e] = rng.normal(size=3) * 10.0 ** rng.uniform(-6, -2)
        else:                                   # a spin about the tangent moves the contact point by -omega r |in-plane t|
            want = {"about the tangent": target, "shared": target - v_roll, "opposed": -1.7 * target}[mode]
            w[e] = q @ ((-want / (radius[e] * ipn[e])) * t[e])
        tau = pick(TORQUES, e)
        other = rng.normal(size=3) * abs(tau) * 0.5
        tq[e] = q @ (tau * ax[e] + other) if tau != 0.0 else np.full(3, tau)
    return SimpleNamespace(n=n, par=par, x=x, v=v, F=F, tq=tq, Q=Q, w=w, t=t, len=ln, mass=mass, r0s=r0s,
                           l_rest=L_REST, taper=taper)


@dataclass
class ContactCase:
    name: str
    n: int
    forms: tuple
    par: SimpleNamespace
    rods: list = field(default_factory=list)


def _par(normal, mu, r0=6.0e-3):
    nrm = np.asarray(normal, float)
    return SimpleNamespace(k=K_CONTACT, nu=NU_CONTACT, slip_tol=SLIP_TOL, surface_tol=SURFACE_TOL, kin_mu=mu[0],
                           stat_mu=mu[1], origin=(0.013, -0.007, -0.0061), normal=tuple(float(c) for c in nrm),
                           r0s_uniform=r0 * math.sqrt(L_REST))


_GENERIC = np.array([0.36, -0.48, 0.8])          # a unit vector with three non-zero components (0.1296 + 0.2304 + 0.64)
E_Z, TILTED = (0.0, 0.0, 1.0), (0.6, 0.0, 0.8)
# name: (n, normal, taper, mu, r0, rods, forms)
_CONTACT = {
    "ez/n2": (2, E_Z, False, MU_OCTOPUS, 6.0e-3, 16, (ZUP1, PLANE1, LITERAL1)),
    "ez/n5": (5, E_Z, False, MU_FORWARD, 7.0e-3, 16, (ZUP1, ZUP2, PLANE1, PLANE2, LITERAL1)),
    "ez/n63": (63, E_Z, False, MU_OCTOPUS, 1.2e-2, 2, (ZUP1, PLANE1, LITERAL1)),
    "ez/n64": (64, E_Z, False, MU_FORWARD, 1.0e-3, 2, (ZUP2, PLANE2)),
    "ez/n101": (101, E_Z, False, MU_OCTOPUS, 3.0e-3, 2, (ZUP2, PLANE2)),
    "ez/n126": (126, E_Z, False, MU_FORWARD, 7.0e-3, 2, (ZUP2, PLANE2)),
    "taper/n5": (5, E_Z, True, MU_OCTOPUS, None, 16, (ZUP_TAPER1, ZUP_TAPER2)),
    "taper/n63": (63, E_Z, True, MU_FORWARD, None, 2, (ZUP_TAPER1, ZUP_TAPER2)),
    "taper/n101": (101, E_Z, True, MU_OCTOPUS, None, 2, (ZUP_TAPER2,)),
    "tilted/n5": (5, TILTED, False, MU_OCTOPUS, 6.0e-3, 8, (PLANE1, PLANE2, LITERAL1)),
    "tilted/n63": (63, TILTED, False, MU_FORWARD, 4.0e-3, 2, (PLANE1, LITERAL1)),
    "generic/n5": (5, _GENERIC, False, MU_FORWARD, 5.0e-3, 8, (PLANE1, PLANE2, LITERAL1)),
    "generic/n126": (126, _GENERIC, False, MU_OCTOPUS, 2.0e-3, 2, (PLANE2,)),
}


def make_zero_rod(rng, n, par, negative):
    """A rod at rest lying flat on the plane: v = 0 and w = 0 exactly (of either sign), nodal forces along the normal
    only, no torque — so the axial speed, the rolling slip, the push and the no-slip force are exact zeros, of both
    signs over the family (the zero's sign follows `negative` and the quadrant the tangent points into) — and the
    nodes' common height is moved ulp by ulp until the middle element's gap, as fp64 forms it, is EXACTLY 0.  The
    other elements' lengths differ in the last bits, so their gaps are zero or an ulp of the radius to either side."""
    z0 = -0.0 if negative else 0.0
    length = np.full(n, L_REST)
    heading = rng.uniform(0, 2 * np.pi)
    a = np.concatenate([[0.0], np.cumsum(length * math.cos(heading))])
    b = np.concatenate([[0.0], np.cumsum(length * math.sin(heading))])
    origin = np.asarray(par.origin, float)
    r0s = np.full(n, par.r0s_uniform)
    mid = n // 2

    def build(z):
        x = origin + np.stack([a, b, np.full(n + 1, z)], axis=1)
        d = np.diff(x, axis=0)
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        gap = 0.5 * (x[mid + 1, 2] + x[mid, 2]) - origin[2] - r0s[mid] / math.sqrt(ln[mid])
        return x, d, ln, gap

    z = par.r0s_uniform / math.sqrt(L_REST)
    for _ in range(200):
        x, d, ln, gap = build(z)
        if gap == 0.0:
            break
        z = math.nextafter(z, -math.inf if gap > 0 else math.inf)
    assert gap == 0.0
    t = d / ln[:, None]
    m_elem = 1000.0 * np.pi * (par.r0s_uniform / math.sqrt(L_REST)) ** 2 * L_REST
    mass = np.concatenate([[0.5 * m_elem], np.full(n - 1, m_elem), [0.5 * m_elem]])
    F = np.full((n + 1, 3), z0)
    F[:, 2] = -rng.choice([1.0e-2, 1.0e-3, 1.0e-5], n + 1)
    Q = np.stack([_random_rotation(rng).ravel() for _ in range(n)])
    return SimpleNamespace(n=n, par=par, x=x, v=np.full((n + 1, 3), z0), F=F, tq=np.full((n, 3), z0), Q=Q,
                           w=np.full((n, 3), z0), t=t, len=ln, mass=mass, r0s=r0s, l_rest=L_REST, taper=False)


ZERO_CASE = "ez/zeros"


@functools.lru_cache(maxsize=None)
def contact_cases():
    out = {}
    sel = 0
    for name, (n, normal, taper, mu, r0, rods, forms) in _CONTACT.items():
        par = _par(normal, mu, r0 if r0 else 1.2e-2)
        case = ContactCase(name, n, forms, par)
        rng = np.random.default_rng(M.hash_name("rod-probe/" + name))
        for _ in range(rods):
            case.rods.append(make_rod(rng, n, par, taper, sel))
            sel += 1
        out[name] = case
    par = _par(E_Z, MU_OCTOPUS, 6.0e-3)
    case = ContactCase(ZERO_CASE, 5, (ZUP1, ZUP2, PLANE1, PLANE2, LITERAL1), par)
    rng = np.random.default_rng(M.hash_name("rod-probe/" + ZERO_CASE))
    case.rods = [make_zero_rod(rng, 5, par, negative=bool(i % 2)) for i in range(8)]
    out[ZERO_CASE] = case
    return out


@functools.lru_cache(maxsize=None)
def contact_reference(name):
    """[(fc, torque, info)] per rod of the case, at 50 digits."""
    return [contact_law(rod, MPF) for rod in contact_cases()[name].rods]


def contact_errors(ref, fc, dt):
    """(force error per node, torque error per element) in units of 2^-52 x the reference side's scale; the largest
    component.  fc (n + 1, 3), dt (n, 3): fp64 results; the torque as the ADDED torque (see added_torque)."""
    rfc, rdt, info = ref
    n = len(info)
    ef, et = np.empty(n + 1), np.empty(n)
    for j in range(n + 1):
        scale = max(info[e].fscale for e in (j - 1, j) if 0 <= e < n)
        ef[j] = float(max(abs(MP.mpf(float(fc[j][i])) - rfc[j][i]) for i in range(3)) / scale / ULP) \
            if np.all(np.isfinite(fc[j])) else np.inf
    for e in range(n):
        et[e] = float(max(abs(dt[e][i] - rdt[e][i]) for i in range(3)) / info[e].tscale / ULP)
    return ef, et


def contact_scales(ref):
    """(force scale per node (n + 1,), torque scale per element (n,)) of one rod's reference, as floats."""
    info = ref[2]
    n = len(info)
    node = [max(info[e].fscale for e in (j - 1, j) if 0 <= e < n) for j in range(n + 1)]
    return np.array([float(s) for s in node]), np.array([float(I.tscale) for I in info])


def added_torque(tq_in, tq_out):
    """tq_out - tq_in exactly (50 digits): the probe returns the element's torque with the law's share added."""
    return [[MP.mpf(float(o)) - MP.mpf(float(i)) if np.isfinite(o) else MP.inf for i, o in zip(ri, ro)]
            for ri, ro in zip(tq_in, tq_out)]


def float_law(rod, mut=()):
    fc, dt, info = contact_law(rod, FLOAT, mut)
    return np.array(fc, float), np.array(dt, float), info


def _mp_rows(a):
    return [[MP.mpf(float(c)) for c in row] for row in a]


@functools.lru_cache(maxsize=None)
def contact_budget(name):
    """{'force': {...}, 'torque': {...}}, each {'float', 'twin': the two roundings' maxima against the reference,
    'baseline': the larger, 'budget': 4 x baseline (floor 8), 'literal_budget': 2 x baseline (floor 8)}: the force and
    the torque are each held to their own baseline."""
    case = contact_cases()[name]
    worst = {"force": [0.0, 0.0], "torque": [0.0, 0.0]}
    for rod, ref in zip(case.rods, contact_reference(name)):
        fc, dt, _ = float_law(rod)
        tf, tt = twin_law(rod)
        for i, (f, t) in enumerate(((fc, dt), (tf, tt))):
            ef, et = contact_errors(ref, f, _mp_rows(t))
            worst["force"][i] = max(worst["force"][i], float(ef.max()))
            worst["torque"][i] = max(worst["torque"][i], float(et.max()))
    return {q: {"float": fl, "twin": tw, "baseline": max(fl, tw), "budget": max(8.0, 4.0 * max(fl, tw)),
                "literal_budget": max(8.0, 2.0 * max(fl, tw))} for q, (fl, tw) in worst.items()}


def regimes(info):
    """Which branch each element of one evaluation takes, as a dict of per-element labels."""
    def ramp(a):
        return "static" if a <= 1 else ("ramp" if a < 2 else "kinetic")

    def cap(f, c):                              # (a cap of zero — off the plane, lifting, or sliding — binds nothing)
        return "zero" if f == 0 else ("no cap" if c == 0 else ("capped" if abs(f) > c else "free"))

    return {
        "gap": ["penetrating" if I.gap < 0 else ("off" if I.off else "inside") for I in info],
        "normal force": ["pressing" if I.along < 0 else ("lifting" if I.along > 0 else "zero") for I in info],
        "axial speed": [("forward" if I.vam > 0 else "backward" if I.vam < 0 else "zero") for I in info],
        "axial slip": [ramp(I.slip_ax_arg) for I in info],
        "rolling slip": [ramp(I.slip_ro_arg) for I in info],
        "push": [cap(I.push, I.push_cap) for I in info],
        "no-slip": [cap(I.noslip, I.noslip_cap) for I in info],
    }


ALL_REGIMES = {"gap": {"penetrating", "inside", "off"}, "normal force": {"pressing", "lifting"},
               "axial speed": {"forward", "backward"}, "axial slip": {"static", "ramp", "kinetic"},
               "rolling slip": {"static", "ramp", "kinetic"}, "push": {"capped", "free"}, "no-slip": {"capped", "free"}}


# ---------------------------------------------------------------------------------------------------------------
# the kinematic step
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class KinCase:
    name: str
    epl: int
    h: float
    x: np.ndarray       # (slots, 3)
    v: np.ndarray
    Q: np.ndarray       # (slots, 9)
    w: np.ndarray
    hx: np.ndarray      # (slots,)
    hq: np.ndarray

    @property
    def waves(self):
        return len(self.hx) // (WAVE * self.epl)


def kin_trips(case):
    """k of sinc_cosc per slot (the trip count of the call its lane's slot s makes with the other 63 lanes)."""
    a = (case.h * case.hq)[:, None] * case.w
    t = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]).reshape(-1, WAVE, case.epl)
    k = np.empty(t.shape, int)
    for wv in range(t.shape[0]):
        for s in range(case.epl):
            k[wv, :, s] = M.sinc_quarterings(t[wv, :, s])
    return k.ravel()


def t_sinc_cosc_on_circle(t):
    """sinc_cosc<true, true> as kinematic_n calls it: M.t_sinc_cosc's sequence, and in a wave that was quartered the
    pair put back on the unit circle, d = sin^2 + cos^2 - 1 = t (sc^2 - 2 cc + cc^2 t) removed to first order."""
    fma = lambda a, b, c: M.FMA(a, b, c)
    sc, cc = M.t_sinc_cosc(t)
    n, (T, S, C) = M._waves(np.asarray(t, float), sc, cc)
    with np.errstate(all="ignore"):
        for w in range(len(T)):
            if M.sinc_quarterings(T[w]) == 0:
                continue
            tw, s, c_ = T[w], S[w], C[w]
            e = fma(s, s, fma(c_ * tw, c_, -2.0 * c_))
            cos = fma(-c_, tw, 1.0)
            C[w] = fma(0.5 * e, cos, c_)
            S[w] = fma(-(0.5 * tw) * e, s, s)
    return S.ravel()[:n], C.ravel()[:n]


def t_kinematic(case):
    """kinematic_n's operation sequence in NumPy, wave by wave; fmas as M.FMA (two roundings, or exactly rounded
    under M.single_rounding()).  -> (x (slots, 3), Q (slots, 9))."""
    fma = lambda a, b, c: M.FMA(a, b, c)
    h = case.h
    hp = h * case.hx
    x = np.stack([fma(hp, case.v[:, i], case.x[:, i]) for i in range(3)], axis=1)
    hh = h * case.hq
    a0, a1, a2 = hh * case.w[:, 0], hh * case.w[:, 1], hh * case.w[:, 2]
    q0, q1, q2 = a0 * a0, a1 * a1, a2 * a2
    t = (q0 + q1 + q2).reshape(-1, WAVE, case.epl)
    sc, cc = np.empty(t.shape), np.empty(t.shape)
    for s in range(case.epl):
        o = t_sinc_cosc_on_circle(t[:, :, s].ravel())
        sc[:, :, s], cc[:, :, s] = o[0].reshape(-1, WAVE), o[1].reshape(-1, WAVE)
    sc, cc = sc.ravel(), cc.ravel()
    s0, s1, s2 = sc * a0, sc * a1, sc * a2
    ca0, ca1 = cc * a0, cc * a1
    c01, c02, c12 = ca0 * a1, ca0 * a2, ca1 * a2
    R0, R4, R8 = fma(-cc, q1 + q2, 1.0), fma(-cc, q0 + q2, 1.0), fma(-cc, q0 + q1, 1.0)
    R1, R3 = c01 + s2, c01 - s2
    R2, R6 = c02 - s1, c02 + s1
    R5, R7 = c12 + s0, c12 - s0
    Q = np.empty_like(case.Q)
    for j in range(3):
        b0, b1, b2 = case.Q[:, j], case.Q[:, 3 + j], case.Q[:, 6 + j]
        p0, p1, p2 = fma(R1, b1, R0 * b0), fma(R4, b1, R3 * b0), fma(R7, b1, R6 * b0)
        Q[:, j] = fma(R2, b2, p0)
        Q[:, 3 + j] = fma(R5, b2, p1)
        Q[:, 6 + j] = fma(R8, b2, p2)
    return x, Q


def _rotations(rng, n):
    return np.stack([_random_rotation(rng).ravel() for _ in range(n)])


def _with_angle(rng, mag, h, axis=None):
    """w (n, 3) with |h w| = mag (to rounding), in random directions or along the given axes."""
    n = len(mag)
    if axis is None:
        axis = rng.normal(size=(n, 3))
        axis /= np.linalg.norm(axis, axis=1)[:, None]
    return axis * (np.asarray(mag) / h)[:, None]


def _kin(name, rng, epl, h, mag, axis=None, hx=None, hq=None):
    n = len(mag)
    assert n % (WAVE * epl) == 0 and n // (WAVE * epl) <= MAX_WAVES
    return KinCase(name, epl, h, rng.uniform(-0.3, 0.3, (n, 3)), rng.normal(size=(n, 3)), _rotations(rng, n),
                   _with_angle(rng, mag, h, axis), np.ones(n) if hx is None else hx, np.ones(n) if hq is None else hq)


KIN_EDGE = math.sqrt(M.SINC_EDGE)      # |a| at the in-range edge t = 1e-3


def _tier_magnitudes(rng, k, n):
    """|a| of n lanes whose wave takes k quarterings: log-spread over the tier, the first lane near its top."""
    lo = KIN_EDGE * 2.0 ** (k - 1)
    hi = min(KIN_EDGE * 2.0 ** k, 10.0) * (1 - 1e-6)
    mag = np.exp(rng.uniform(math.log(lo * (1 + 1e-6)), math.log(hi), n))
    mag[0] = hi
    return mag


@functools.lru_cache(maxsize=None)
def kin_cases():
    out = {}
    h = 2.5e-4 * 1.0009765625

    def add(case):
        out[case.name] = case

    rng = np.random.default_rng(M.hash_name("rod-probe/kinematic"))
    mag = np.exp(rng.uniform(math.log(1e-12), math.log(KIN_EDGE * (1 - 1e-6)), 4 * WAVE))
    mag[::WAVE] = KIN_EDGE * (1 - 1e-6)
    add(_kin("in_range", rng, 1, h, mag))
    below = KIN_EDGE * (1 - 10.0 ** -rng.uniform(3, 9, WAVE))             # a whole wave just under the edge: in range
    above = np.where(np.arange(WAVE) % 2 == 0, KIN_EDGE * (1 + 10.0 ** -rng.uniform(3, 9, WAVE)), below)
    add(_kin("edge", rng, 1, h, np.concatenate([below, above])))          # one lane in two just over it: k = 1
    axes = np.tile(np.vstack([np.eye(3), -np.eye(3), np.zeros((2, 3))]), (8, 1))
    amag = np.exp(rng.uniform(math.log(1e-9), math.log(KIN_EDGE * 0.99), WAVE))
    case = _kin("axis_aligned_and_zero", rng, 1, h, amag, axis=axes)
    case.w[7::8] = -0.0
    add(case)
    add(_kin("quartered", rng, 1, h, np.concatenate([_tier_magnitudes(rng, k, WAVE) for k in range(1, 10)])))
    mixed = np.exp(rng.uniform(math.log(1e-9), math.log(KIN_EDGE * 0.99), 2 * WAVE))
    mixed[17] = 100.0
    mixed[WAVE + 63] = 100.0
    add(_kin("mixed", rng, 1, h, mixed))
    # EPL 2: slot 0 of every lane in one regime, slot 1 in another (the two calls of sinc_cosc take different tiers)
    two = np.empty((3, WAVE, 2))
    two[0, :, 0] = np.exp(rng.uniform(math.log(1e-9), math.log(KIN_EDGE * 0.99), WAVE))
    two[0, :, 1] = _tier_magnitudes(rng, 3, WAVE)
    two[1, :, 0] = _tier_magnitudes(rng, 9, WAVE)
    two[1, :, 1] = np.exp(rng.uniform(math.log(1e-12), math.log(KIN_EDGE * 0.99), WAVE))
    two[2, :, 0] = _tier_magnitudes(rng, 1, WAVE)
    two[2, :, 1] = _tier_magnitudes(rng, 6, WAVE)
    add(_kin("two_slots", rng, 2, h, two.ravel()))
    # held slots: hq = 0 / hx = 0 on every other slot, in an in-range wave, a quartered one and a blown-up one
    held = np.concatenate([np.exp(rng.uniform(math.log(1e-6), math.log(KIN_EDGE * 0.99), WAVE)),
                           _tier_magnitudes(rng, 5, WAVE), _tier_magnitudes(rng, 2, WAVE)])
    held[2 * WAVE + 5] = 100.0
    n = len(held)
    hq = np.where(np.arange(n) % 2 == 0, 0.0, 1.0)
    hx = np.where(np.arange(n) % 3 == 0, 0.0, 1.0)
    add(_kin("held", rng, 1, h, held, hx=hx, hq=hq))
    return out


@functools.lru_cache(maxsize=None)
def kin_reference(name):
    """(x[slots][3], Q[slots][9]) at 50 digits: x + h hx v and R(h hq w) Q in the kernel's sign convention
    (R01 = cosc a0 a1 + sinc a2: PyElastica's _get_rotation_matrix, the transpose of the textbook's)."""
    case = kin_cases()[name]
    mp = MP.mpf
    xs, Qs = [], []
    for j in range(len(case.hx)):
        hp = mp(case.h) * mp(float(case.hx[j]))
        xs.append([mp(float(case.x[j, i])) + hp * mp(float(case.v[j, i])) for i in range(3)])
        hh = mp(case.h) * mp(float(case.hq[j]))
        a = [hh * mp(float(case.w[j, i])) for i in range(3)]
        t = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
        if t == 0:
            sc, cc = mp(1), mp(1) / 2
        else:
            th = MP.sqrt(t)
            sc, cc = MP.sin(th) / th, 2 * MP.sin(th / 2) ** 2 / t
        R = [[cc * a[i] * a[m] for m in range(3)] for i in range(3)]
        for i in range(3):
            R[i][i] = 1 - cc * (t - a[i] * a[i])
        R[0][1] += sc * a[2]; R[1][0] -= sc * a[2]
        R[0][2] -= sc * a[1]; R[2][0] += sc * a[1]
        R[1][2] += sc * a[0]; R[2][1] -= sc * a[0]
        q = [mp(float(c)) for c in case.Q[j]]
        Qs.append([sum(R[i][m] * q[3 * m + c] for m in range(3)) for i in range(3) for c in range(3)])
    return xs, Qs


def kin_errors(name, x, Q):
    """(position error in ulps of the result, Q error in absolute ulps), each the largest component per slot."""
    rx, rq = kin_reference(name)
    ex, eq = np.empty(len(rx)), np.empty(len(rx))
    for j in range(len(rx)):
        if not (np.all(np.isfinite(x[j])) and np.all(np.isfinite(Q[j]))):
            ex[j] = eq[j] = np.inf
            continue
        ex[j] = float(max(abs(MP.mpf(float(x[j, i])) - rx[j][i]) / abs(rx[j][i]) for i in range(3)) / ULP)
        eq[j] = float(max(abs(MP.mpf(float(Q[j, i])) - rq[j][i]) for i in range(9)) / ULP)
    return ex, eq


def derived_q_budget(k):
    return 3.0 if k == 0 else 2.0 * (k + 3)


@functools.lru_cache(maxsize=None)
def kin_budgets():
    """{k: {'derived', 'plain', 'fma', 'budget', 'note'}} over every case: the two transcriptions' maxima per trip
    count and the budget the device is held to — the derived one, or (the fall-back rule) the exactly rounded-fma
    transcription's maximum + 2 where that transcription itself misses the derived bound."""
    per_k = {}
    for name, case in kin_cases().items():
        k = kin_trips(case)
        with np.errstate(all="ignore"):
            plain = kin_errors(name, *t_kinematic(case))[1]
            with M.single_rounding():
                fused = kin_errors(name, *t_kinematic(case))[1]
        for kk in np.unique(k):
            d = per_k.setdefault(int(kk), {"derived": derived_q_budget(int(kk)), "plain": 0.0, "fma": 0.0})
            d["plain"] = max(d["plain"], float(plain[k == kk].max()))
            d["fma"] = max(d["fma"], float(fused[k == kk].max()))
    for kk, d in per_k.items():
        if d["fma"] <= d["derived"]:
            d["budget"], d["note"] = d["derived"], "derived"
        else:
            d["budget"] = d["fma"] + 2.0
            d["note"] = "fall-back: the exactly rounded-fma transcription itself misses the derived bound"
    return per_k


def kin_q_budget(case):
    """The Q budget per slot: that of the tier its wave takes."""
    b = kin_budgets()
    return np.array([b[int(k)]["budget"] for k in kin_trips(case)])


def orthogonality_defect(Q):
    """max |Q Q^T - I| per slot in units of 2^-52 (extended precision)."""
    q = np.asarray(Q, np.longdouble).reshape(-1, 3, 3)
    d = np.einsum("nij,nkj->nik", q, q) - np.eye(3, dtype=np.longdouble)
    return np.asarray(np.abs(d).reshape(len(q), -1).max(axis=1) / ULP, float)
