"""The single-interaction catalogue of the single-precision kernels: ONE leaf, ONE hit, every field of the records it leaves, held
to a bound that follows from float rounding and from the conditioning of the problem itself.

Every form is one leaf at ORIGIN = (30, 20, -10), turned by POSE (a dense M, large coordinates), met by an AIMED fan of N_RAYS =
130 rays (two waves and two lanes): a ray is built backwards from a target point P on the surface, an angle of incidence and an
azimuth, so its hit lies where the fan put it — inside the aperture by the margin of the target region, at an incidence clear of
the critical angle — and not where a random direction happens to land.  A lens group is built and posed as a group and its front
face taken out of it: the scene is that leaf alone, the child of the hit meets nothing.  Not part of scenes.SCENES.

    FORMS, NAMES                  the catalogue: name -> Form (builder, fan, ray fields, expectations, N)
    leaf(oa, name)                the posed leaf;  rays(name): the host rays, float32 values widened to double
    reference(name)               (compiled scene, rays, K, Bound) from the oracle alone, cached
    bound(scene, rays, K, N)      THE bound: the oracle's records and a tolerance per record and field
    compare(bnd, rays, got)       a trace in the reference's order against a Bound: the list of violations and the worst ratios

THE BOUND.  |x - x*| <= N (u S + D) per record and field, u = 2^-24:
  x*  the oracle on the float32 inputs widened to double (the values the device reads);
  S   the largest magnitude that enters the field's arithmetic: hit point and segment 0's `length`: max(|ray origin|_inf,
      |leaf origin|_inf, t); direction: 1; n and intensity: the value; pathlength: |pl_in| + t n; q: |q_in + t|;
  D   the conditioning: the largest change of the oracle's OWN value of that field over RUNS = 8 seeded runs with every component
      of o and d, the wavelength and q moved by +-1 ulp of float32 (the method of oracle.q_tolerance).  A ray whose surface
      sequence, number of children or total-reflection decision changes in one of those runs is EXCLUDED;
  N   the number of roundings on the longest dependency chain from the loaded ray to the stored field, counted in
      trace_core.h (test_leaf / hit_leaf, surf_normal, material_index, interact) and written down below — never measured.

COUNTING RULES.  One per float operation whose result is rounded (a fused multiply-add is one; -ffp-contract=on fuses a * b + c
inside an expression, and where the source leaves that open the unfused count is taken); one for a scene constant that is not a
float (M, a radius, an index, 1 / f ...) where the chain starts at it.  v_rcp_f32, v_rsq_f32 and v_sqrt_f32: no document in
this repository states their error (the source calls them "1 ulp"), so each counts as TWO roundings (HW).  A binary operation
continues the LONGER of its operands' chains.  A Newton step that squares the error of its start (rsqrt_t's, polish_root's
accepted step) ends the chain that led to the start: what remains are the roundings of the step itself; polish_root's
termination, |step| <= 2.4e-7 |t| = 4 u |t|, counts as four.  N_CAP = 64: a count above it is NOT used — the field is held to 64
and the form is named in OVER_CAP (DESIGN.md section 5 reports them).

THE CHAINS (the numbers are computed by _chains() from these steps, so the text and the table cannot drift apart):
  frames    r = o - g: 1; M^T r (product, two fused steps): 3 -> LOC_O = 4.  M^T d: the rounded M entry 1 + 3 -> LOC_D = 4.
            a direction out: |v|^2 3, rsqrt_t 3 (-0.5 x y, the fused step, the product; the estimate's error is squared away),
            v * inv 1, M v 3 -> NORM_LAB = 10.  a point out: M P 3, + g 1 -> LAB_O = 4.
  the input direction is a unit vector only to one rounding, and the oracle renormalises it: t, and what is built on t, carries
            one more (IN_NORM = 1).
  planar    t = s * rcp(ld_x): max(LOC_O, LOC_D + HW) + 1 = 7; P = fma(t, ld, lo): 8.
  sphere    tca 3 on max(LOC_O, LOC_D) = 7; c = o + tca d: 8; disc = R^2 - |c|^2: 3 + 1 = 12; sqrt: 14; t = tca -+ hc: 15; P: 16;
            normal P * rcp(R): 17.
  searched  (cylinder, 3-D polygon, aspheres: ten samples, then polish_root)  the last Newton step from a start whose error it
            squares: P = o + t d on LOC_O: 5; g; dg; t - g * rcp(dg); + 4 for the termination.  cylinder g = Px^2 + Py^2 - R^2: 8,
            dg: 7, rcp 9, step 10 -> t = 14.  3-D polygon g = n . (P - v0): 9, dg 7 -> t = 14.  conic / exact asphere: r^2 7,
            1 - p6 r^2 8, sqrt 10, 1 + 11, rcp 13, product 14, the polynomial's sums 16, x + F 17; dg 15, rcp 17, step 18 -> t = 22.
            series asphere: r = sqrt(r^2) 9, the Clenshaw argument 11, 2 per coefficient after the first and 2 for the last line
            (CLENSHAW(n) = 2 n) -> F; x + F; dg one more, its division by r one more, + dx; rcp; step; + 4.
  normals   plane: exact.  polygon: the record's rounded normal, 1.  cylinder: P * rcp(R), P + 1.  asphere: r = sqrt(Py^2 + Pz^2):
            P + 2 + HW; s = sag_d1(r) analytic: r^2 1, (1 + k) r^2 1, * rcp(R^2) 1, 1 - 1, sqrt HW, R sq 1, rcp HW, r * 1, + polynomial
            1 -> r + 11 (the exact form is one shorter); series: r + 2 + CLENSHAW(n).  ay = s * (Py * rcp(r)): 1; 1 + ay^2 + az^2: 2;
            rsqrt_t 3; ay * inv 1 -> s + 7.
  dn        3 on max(LOC_D, normal).
  mirror    d - 2 dn n (fused): dn + 1, then NORM_LAB.  passing on: LOC_D, then NORM_LAB.  I * r: the rounded coefficient and the
            product: 2.  q = q_in + t: t + IN_NORM + 1; pathlength = pl + t n: t + IN_NORM + 2 (taken unfused).
  lens      d - P / f (fused): max(LOC_D, P) + 1, then NORM_LAB.  q1 / (1 - q1 / f): br = 1 - q1r jf: q + 1; |b|^2 2; rcp HW; the
            quotient 1 -> q + 6.  n and pathlength are the input's: 1.
  index     constant: 1.  Sellmeier: wl * unit 2 (the rounded unit), * rcp(1e-6) on max(2, 1 + HW): 4, squared 5, - C 6, B p p 8,
            two sums 10, um^2 * num 11; the denominator 8, rcp 10; the quotient 12; 1 + 13; sqrt 15.  series: x 2, 2x - (lo + hi) 3,
            * rcp(hi - lo) 5, CLENSHAW(n).
  Snell     ratio = nin * rcp(nout): index + HW + 1.  si = sqrt(1 - ci^2): dn + 1 + HW; st = ratio * si: max + 1; ct = sqrt(1 - st^2):
            + 1 + HW; ratio (d - dn n) + ct n: ct + 2; then NORM_LAB.  reflected (total or partial): as the mirror.
            q at a flat face: q1 * rcp(ratio): max(q, ratio + HW) + 1; reflected: q1.  at a curved face: Cc = (nin - nout) * rcp(ROC
            nout): max(index + 1, ROC + 1) + HW + 1; br = Cc q1r + ratio: max(Cc, q, ratio) + 1; |b|^2 2, rcp HW, quotient 1 -> br + 5;
            reflected: Cr = 2 rcp(ROC): ROC + HW, then the same.  ROC of a cap: the rounded radius, 1.  of an asphere: c = sag_d2(r):
            the cube of sq 2 past sq, R^3 sq^3 1, rcp HW, product 1, two sums 2 -> r + 4 + HW + 8 (series: r + 2 + CLENSHAW(n));
            w = 1 + s^2: s + 1; w sqrt(w): HW + 1; * rcp(c): max(w + 3, c + HW) + 1.
"""
import functools
from collections import namedtuple

import numpy as np

import form_scenes
from optable_amd import abi, shapes
from optable_amd import workloads as W
from optable_amd.components import BLOCK, LENS, MIRROR, REFRACT, ROC_ASPHERE, ROC_CONST, ROC_INF

U = 2.0**-24
ORIGIN = (30.0, 20.0, -10.0)
N_RAYS = 130
RUNS = 8
N_CAP = 64
HW = 2  # v_rcp_f32, v_rsq_f32, v_sqrt_f32: no document here states their error; two roundings each
REAL_FIELDS = abi.SEG_FIELDS
GROUPS = {"ox": "o", "oy": "o", "oz": "o", "dx": "d", "dy": "d", "dz": "d", "length": "length", "intensity": "intensity",
          "q_re": "q", "q_im": "q", "n": "n", "pathlength": "pathlength"}
# the input ray beyond origin and direction: not round numbers, q with a real part of the size of its imaginary part
Q_IN = -40.0 + 25.0j
I_IN, PL_IN = 0.8, 12.5
DISPERSION_NM = (400.0, 780.0, 1100.0)
CAUCHY_NM = (450.0, 633.0, 850.0)  # inside the fitted range of the flint (materials.WAVELENGTH_RANGE)


def POSE(c):
    return c.RotZ(0.7).RotY(-0.4).RotX(0.3)


# -- N: the chains of the docstring as arithmetic -------------------------------------------------------------------------------
LOC_O, LOC_D, NORM_LAB, LAB_O, IN_NORM, TERMINATION = 4, 4, 10, 4, 1, 4


def CLENSHAW(n):
    return 2 * n


SELLMEIER = 15


def _series_index(n):
    return 5 + CLENSHAW(n)


def _hit(kind, n_series=0):
    """(t, P, normal): chain lengths to the hit distance, the local hit point and the normal's components"""
    if kind == "planar":
        t = max(LOC_O, LOC_D + HW) + 1
        return t, t + 1, 0
    if kind == "polygon":
        t = max(LOC_O, LOC_D + HW) + 1
        return t, t + 1, 1
    if kind == "sphere":
        t = max(LOC_O, LOC_D) + 3 + 1 + 3 + 1 + HW + 1
        return t, t + 1, t + 2
    if kind == "cylinder":
        t = max(LOC_O + 1 + 3, LOC_O + 1 + 2 + HW) + 1 + TERMINATION
        return t, t + 1, t + 2
    if kind == "polygon3d":
        t = max(LOC_O + 1 + 1 + 3, LOC_D + 3 + HW) + 1 + TERMINATION
        return t, t + 1, 1
    if kind in ("asphere", "asphere_exact"):
        g = LOC_O + 1 + 2 + 1 + HW + 1 + HW + 1 + 2 + 1
        t = max(g, 15 + HW) + 1 + TERMINATION
        r = t + 1 + 2 + HW
        s = r + (11 if kind == "asphere" else 10)
        return t, t + 1, s + 7
    if kind == "asphere_series":
        r0 = LOC_O + 1 + 2 + HW
        F = r0 + 2 + CLENSHAW(n_series)
        t = max(F + 1, F + 3 + HW) + 1 + TERMINATION
        r = t + 1 + 2 + HW
        s = r + 2 + CLENSHAW(n_series)
        return t, t + 1, s + 7
    raise KeyError(kind)


def _roc(kind, hit, n_series=0):
    """chain length to ROC"""
    t, P, nrm = hit
    if kind == "sphere":
        return 1
    r, s = P + 2 + HW, nrm - 7
    c = r + 4 + HW + 8 if kind != "asphere_series" else r + 2 + CLENSHAW(n_series)
    return max(s + 1 + HW + 1, c + HW) + 1


def _chains(kind, inter, index=1, n_series=0):
    """N per field group for one form.  kind: the hit (see _hit); inter: "mirror" | "pass" | "lens" | "lens_noq" | "block" |
    "refract" | "reflect" (the reflected ray of an interface: total reflection, a coat, the partial reflection) | a tuple of
    those for a hit that emits more than one kind of child (the maximum per field is taken); index: the chain of the interface's
    dispersive index (1: constants)."""
    if isinstance(inter, tuple):
        parts = [_chains(kind, i, index, n_series) for i in inter]
        return {k: max(p[k] for p in parts) for k in parts[0]}
    hit = _hit(kind, n_series)
    t, P, nrm = hit
    q1 = t + IN_NORM + 1
    N = {"o": P + LAB_O, "length": t + IN_NORM, "intensity": 2, "n": 1, "pathlength": t + IN_NORM + 2, "q": q1, "d": 1}
    dn = max(LOC_D, nrm) + 3
    if inter == "block":
        return N
    if inter in ("mirror", "reflect"):
        N["d"] = dn + 1 + NORM_LAB
        if inter == "reflect" and kind != "planar":  # q_r through Cr = 2 / ROC
            N["q"] = max(_roc(kind, hit, n_series) + HW, q1) + 1 + 5
    elif inter == "pass":
        N["d"] = LOC_D + NORM_LAB
    elif inter in ("lens", "lens_noq"):
        N["d"] = max(LOC_D, P) + 1 + NORM_LAB
        N["q"] = q1 + 6 if inter == "lens" else 1
        N["pathlength"] = 1
    elif inter == "refract":
        ratio = index + HW + 1
        si = dn + 1 + HW
        ct = max(ratio, si) + 1 + 1 + HW
        N["d"] = ct + 2 + NORM_LAB
        N["n"] = index
        if kind == "planar":
            N["q"] = max(q1, ratio + HW) + 1
        else:
            Cc = max(index + 1, _roc(kind, hit, n_series) + 1) + HW + 1
            N["q"] = max(Cc, q1, ratio) + 1 + 5
    else:
        raise KeyError(inter)
    return N


# -- the catalogue ----------------------------------------------------------------------------------------------------------------
Form = namedtuple("Form", "name group build fan n_in has_q wavelengths_nm chain expect planar_const")
# fan: dict(target=..., side=+1 (the ray arrives on the side the normal points to: dn < 0) | -1, incidence=(lo, hi) degrees,
#           distance=(lo, hi) from the ray origin to the hit)
# expect: dict(shape, interaction, roc_kind, preset, children, n_changes (per child), shares (intensity of each child / I_IN), dn_sign)
FORMS = {}
OVER_CAP = {}  # name -> {field group: counted N} where the count exceeds N_CAP


def _add(name, group, build, fan, chain, expect, n_in=1.0, has_q=True, wavelengths_nm=None, planar_const=False):
    FORMS[name] = Form(name, group, build, fan, n_in, has_q, wavelengths_nm, chain, expect, planar_const)


_DISC = dict(target=("disc", 0.9))
_ENTER, _LEAVE, _TIR = (5.0, 60.0), (5.0, 35.0), (48.0, 70.0)  # n = 1.5: sin(critical) = 2/3, 41.8 degrees; st <= 0.87 and >= 1.11


def _front_face(group):
    return POSE(group).components[0]


def _mirror(r, t):
    return lambda oa: POSE(oa.Mirror(ORIGIN, radius=1.0, reflectivity=r, transmission=t))


for _n, _r, _t, _inter, _shares in (("mirror_reflecting", 1.0, 0.0, "mirror", (1.0,)), ("mirror_splitting", 0.7, 0.3, ("mirror", "pass"), (0.7, 0.3)),
                                     ("mirror_passing", 0.0, 1.0, "pass", (1.0,))):
    _add(_n, "mirrors", _mirror(_r, _t), dict(_DISC, side=+1, incidence=(3.0, 50.0)), ("planar", _inter),
         dict(shape=shapes.CIRCLE, interaction=MIRROR, roc_kind=ROC_INF, preset="FA", children=len(_shares), n_changes=(False,) * len(_shares),
              shares=_shares, dn_sign=-1), planar_const=True)
for _n, _f, _q in (("lens_converging", 7.5, True), ("lens_diverging", -7.5, True), ("lens_converging_no_q", 7.5, False), ("lens_diverging_no_q", -7.5, False)):
    _add(_n, "thin lenses", (lambda f: lambda oa: POSE(oa.Lens(ORIGIN, focal_length=f, radius=1.0, transmission=0.95)))(_f),
         dict(_DISC, side=+1, incidence=(3.0, 30.0)), ("planar", "lens" if _q else "lens_noq"),
         dict(shape=shapes.CIRCLE, interaction=LENS, roc_kind=ROC_INF, preset="FA", children=1, n_changes=(False,), shares=(0.95,), dn_sign=-1),
         has_q=_q, planar_const=True)
_add("block", "mirrors", lambda oa: POSE(oa.Block(ORIGIN, width=2.0, height=2.0)), dict(target=("rect", 0.9, 0.9), side=+1, incidence=(3.0, 50.0)),
     ("planar", "block"), dict(shape=shapes.RECT, interaction=BLOCK, roc_kind=ROC_INF, preset="FA", children=0, n_changes=(), shares=(), dn_sign=-1),
     planar_const=True)


def _flat(n2=1.5, r=0.0, t=1.0):
    return lambda oa: POSE(oa.CircleRefractive(ORIGIN, radius=1.0, n1=1.0, n2=n2(oa) if callable(n2) else n2, reflectivity=r, transmission=t))


_FLAT = dict(shape=shapes.CIRCLE, interaction=REFRACT, roc_kind=ROC_INF, preset="FB")
_add("flat_entering", "flat interface", _flat(), dict(_DISC, side=+1, incidence=_ENTER), ("planar", "refract"),
     dict(_FLAT, children=1, n_changes=(True,), shares=(1.0,), dn_sign=-1), planar_const=True)
_add("flat_leaving", "flat interface", _flat(), dict(_DISC, side=-1, incidence=_LEAVE), ("planar", "refract"),
     dict(_FLAT, children=1, n_changes=(True,), shares=(1.0,), dn_sign=+1), n_in=1.5, planar_const=True)
_add("flat_total_reflection", "flat interface", _flat(), dict(_DISC, side=-1, incidence=_TIR), ("planar", "reflect"),
     dict(_FLAT, children=1, n_changes=(False,), shares=(1.0,), dn_sign=+1), n_in=1.5, planar_const=True)
_add("flat_splitting", "flat interface", _flat(r=0.1, t=0.9), dict(_DISC, side=-1, incidence=_LEAVE), ("planar", ("refract", "reflect")),
     dict(_FLAT, children=2, n_changes=(True, False), shares=(0.9, 0.1), dn_sign=+1), n_in=1.5, planar_const=True)
_add("flat_total_reflection_splitting", "flat interface", _flat(r=0.1, t=0.9), dict(_DISC, side=-1, incidence=_TIR), ("planar", "reflect"),
     dict(_FLAT, children=2, n_changes=(False, False), shares=(1.0, 0.1), dn_sign=+1), n_in=1.5, planar_const=True)

from optable_amd import materials as _materials  # noqa: E402

for _g in _materials._GLASSES:
    _add("dispersion_" + _g[len("Glass_"):], "dispersion", _flat(n2=(lambda g: lambda oa: getattr(oa, g)())(_g)), dict(_DISC, side=+1, incidence=_ENTER),
         ("planar", "refract", SELLMEIER), dict(_FLAT, children=1, n_changes=(True,), shares=(1.0,), dn_sign=-1), wavelengths_nm=DISPERSION_NM)
_add("dispersion_two_term_at_one_micron", "dispersion",
     _flat(n2=lambda oa: oa.SellmeierMaterial("two-term", [1.03961212, 0.231792344], [0.00600069867, 0.0200179144])),
     dict(_DISC, side=+1, incidence=_ENTER), ("planar", "refract", SELLMEIER), dict(_FLAT, children=1, n_changes=(True,), shares=(1.0,), dn_sign=-1),
     wavelengths_nm=(1000.0,))
CAUCHY_TERMS = 58  # coefficients of the series the compiler fits to the flint over its default range (asserted by the CPU tests)
_add("dispersion_cauchy_callable", "dispersion", _flat(n2=lambda oa: oa.Material("cauchy flint", n=lambda wl_m: 1.6 + 8e-15 / wl_m**2)),
     dict(_DISC, side=+1, incidence=_ENTER), ("planar", "refract", _series_index(CAUCHY_TERMS)),
     dict(_FLAT, preset="FM", children=1, n_changes=(True,), shares=(1.0,), dn_sign=-1), wavelengths_nm=CAUCHY_NM)

CAP_R, CAP_H = 8.0, 1.0
_CAP_ANGLE = 0.85 * float(np.arcsin(form_scenes.cap_half_width(CAP_R, CAP_H) / CAP_R))


def _cap(n2, r=0.0, t=1.0):
    return lambda oa: POSE(oa.SphereRefractive(ORIGIN, radius=CAP_R, height=CAP_H, n1=1.0, n2=oa.Glass_NBK7() if n2 == "NBK7" else n2, reflectivity=r, transmission=t))


_SPH = dict(shape=shapes.SPHERE, interaction=REFRACT, roc_kind=ROC_CONST, preset="FE")
for _tag, _n2, _idx in (("constant", 1.5, 1), ("NBK7", "NBK7", SELLMEIER)):
    _add(f"sphere_outside_{_tag}", "spherical caps", _cap(_n2), dict(target=("sphere", CAP_R, _CAP_ANGLE), side=+1, incidence=(3.0, 40.0)),
         ("sphere", "refract", _idx), dict(_SPH, children=1, n_changes=(True,), shares=(1.0,), dn_sign=-1))
    _add(f"sphere_inside_{_tag}", "spherical caps", _cap(_n2), dict(target=("sphere", CAP_R, _CAP_ANGLE), side=-1, incidence=(3.0, 33.0), distance=(3.0, 8.0)),
         ("sphere", "refract", _idx), dict(_SPH, children=1, n_changes=(True,), shares=(1.0,), dn_sign=+1), n_in=1.5)
    _add(f"sphere_coated_{_tag}", "spherical caps", _cap(_n2, r=1.0, t=0.0), dict(target=("sphere", CAP_R, _CAP_ANGLE), side=+1, incidence=(3.0, 40.0)),
         ("sphere", "reflect", _idx), dict(_SPH, children=1, n_changes=(False,), shares=(1.0,), dn_sign=-1))

SERIES_TERMS = 11  # coefficients of the series of g24's sag_front on this aperture (asserted by the CPU tests)
_SAG_FRONT = lambda r: 0.5 * (np.cosh(0.3 * r) - 1.0) + 1e-3 * r**4  # noqa: E731 - scenes.g24_callables
_ASPH = dict(interaction=REFRACT, roc_kind=ROC_ASPHERE, children=1, n_changes=(True,), shares=(1.0,), dn_sign=-1)
for _k in ("parabola", "all_terms"):
    _add(f"asphere_{_k}", "aspheres", (lambda k: lambda oa: _front_face(oa.ASphericParametricLens(ORIGIN, CT=0.6, diameter=2.4, n=1.5, **form_scenes.ASPHERES[k])))(_k),
         dict(target=("asphere", 1.2, 0.85), side=+1, incidence=(3.0, 35.0)), ("asphere", "refract"), dict(_ASPH, shape=shapes.ASPHERE_PARAM, preset="FE"))
_add("asphere_exact", "aspheres", lambda oa: _front_face(oa.ASphericExactSphericalLens(ORIGIN, CT=0.6, diameter=2.4, **form_scenes.EXACT["exact_long"])),
     dict(target=("asphere", 1.2, 0.85), side=+1, incidence=(3.0, 35.0)), ("asphere_exact", "refract"), dict(_ASPH, shape=shapes.ASPHERE_EXACT, preset="FE"))
_add("asphere_series", "aspheres", lambda oa: _front_face(oa.ASphericLens(ORIGIN, CT=0.7, f_asphere_1=_SAG_FRONT, f_asphere_2=None, diameter=2.6, n=1.5)),
     dict(target=("asphere", 1.3, 0.85), side=+1, incidence=(3.0, 35.0)), ("asphere_series", "refract", 1, SERIES_TERMS),
     dict(_ASPH, shape=shapes.ASPHERE_CHEB, preset="FM"))

CYL_R, CYL_ARC = 1.5, (-np.pi / 4, np.pi / 4)  # an arc: the ray reflected inside leaves through the open side


def _cyl(oa):
    return POSE(oa.CylMirror(ORIGIN, radius=CYL_R, height=2.0, theta_range=CYL_ARC))


_CYL = dict(shape=shapes.CYLINDER, interaction=MIRROR, roc_kind=ROC_INF, preset="FM", children=1, n_changes=(False,), shares=(1.0,))
_add("cylinder_inside", "cylinder", _cyl, dict(target=("cylinder", CYL_R, 0.6, 0.8), side=-1, incidence=(3.0, 35.0), distance=(0.5, 2.0)), ("cylinder", "mirror"),
     dict(_CYL, dn_sign=+1))
_add("cylinder_convex", "cylinder", _cyl, dict(target=("cylinder", CYL_R, 0.6, 0.8), side=+1, incidence=(3.0, 35.0)), ("cylinder", "mirror"), dict(_CYL, dn_sign=-1))


def _polygon(name):
    def build(oa):
        m = oa.BaseMirror(ORIGIN)
        normal = form_scenes.polygon_normal(name)
        verts = form_scenes.polygon_vertices(name)
        m.surface = oa.Polygon(verts) if normal is None else oa.Polygon(verts, normal=normal)
        return POSE(m)
    return build


_POLY = dict(interaction=MIRROR, roc_kind=ROC_INF, children=1, n_changes=(False,), shares=(1.0,), dn_sign=-1)
_add("polygon_planar", "polygons", _polygon("poly_concave"), dict(target=("polygon", "poly_concave"), side=+1, incidence=(3.0, 50.0)), ("polygon", "mirror"),
     dict(_POLY, shape=shapes.POLYGON2D, preset="FE"), planar_const=True)
_add("polygon_tilted_3d", "polygons", _polygon("poly3d_tilted"), dict(target=("polygon", "poly3d_tilted"), side=+1, incidence=(3.0, 50.0)),
     ("polygon3d", "mirror"), dict(_POLY, shape=shapes.POLYGON3D, preset="FM"))

NAMES = list(FORMS)
BRANCHING = tuple(n for n, f in FORMS.items() if f.expect["children"] > 1)


def counted_N(name):
    """The N of a form per field group as counted (before the cap)."""
    return _chains(*FORMS[name].chain)


def N_of(name):
    """The N a form is held to: the count, at most N_CAP (a form with a count above it: OVER_CAP)."""
    counted = counted_N(name)
    over = {k: v for k, v in counted.items() if v > N_CAP}
    if over:
        OVER_CAP[name] = over
    return {k: min(v, N_CAP) for k, v in counted.items()}


def max_trace_num(name):
    """K = 2: the hit and its child; a hit with two children needs a third pop of the queue to record the second."""
    return 3 if name in BRANCHING else 2


# -- the leaf, its preset and its rays ----------------------------------------------------------------------------------------------
def leaf(oa, name):
    return FORMS[name].build(oa)


@functools.lru_cache(maxsize=None)
def table(name):
    """the OpticalTable that holds the form's leaf and nothing else"""
    import optable_amd as oa

    tab = oa.OpticalTable()
    tab.add_components([leaf(oa, name)])
    return tab


@functools.lru_cache(maxsize=None)
def compiled(name):
    return table(name).compile()


def preset(scene):
    """The feature preset the library picks for a scene, restated from its rule (scene_features and tables.h): FA mirrors and thin
    lenses, FB + interfaces, FE + polygon apertures and curved surfaces, FM + cylinders, tilted polygons and series."""
    need = set()
    for nd in scene.nodes[: scene.n_nodes]:
        if nd.kind != abi.NODE_LEAF:
            continue
        if nd.shape in (shapes.POLYGON2D, shapes.CSG):
            need.add("POLY")
        if nd.shape not in (shapes.CIRCLE, shapes.RECT, shapes.POLYGON2D, shapes.CSG):
            need.add("CURVED")
        if nd.shape in (shapes.ASPHERE_CHEB, shapes.IMPLICIT_CHEB, shapes.POLYGON3D, shapes.CYLINDER):
            need.add("MISC")
        if nd.shape == shapes.POLYGON3D:
            need.add("POLY")
        if nd.interaction == REFRACT:
            need.add("REFRACT")
    if any(m.kind == abi.MAT_CHEB for m in scene.materials[: scene.n_materials]):
        need.add("MISC")
    if "MISC" in need:
        return "FM"
    if need & {"POLY", "CURVED"}:
        return "FE"
    return "FB" if "REFRACT" in need else "FA"


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _targets(rng, spec, n):
    """(P, normal) in the leaf frame: n target points on the surface, inside the aperture by the margin of the region drawn from"""
    kind = spec[0]
    phi = rng.uniform(-np.pi, np.pi, n)
    if kind == "disc":
        r = spec[1] * np.sqrt(rng.uniform(0, 1, n))
        return np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], 1), np.tile([1.0, 0.0, 0.0], (n, 1))
    if kind == "rect":
        return np.stack([np.zeros(n), rng.uniform(-spec[1], spec[1], n), rng.uniform(-spec[2], spec[2], n)], 1), np.tile([1.0, 0.0, 0.0], (n, 1))
    if kind == "sphere":
        R, amax = spec[1], spec[2]
        a = amax * np.sqrt(rng.uniform(0, 1, n))
        nrm = np.stack([np.cos(a), np.sin(a) * np.cos(phi), np.sin(a) * np.sin(phi)], 1)
        return R * nrm, nrm
    if kind == "cylinder":
        R, th, z = spec[1], rng.uniform(-spec[2], spec[2], n), rng.uniform(-spec[3], spec[3], n)
        nrm = np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1)
        return np.stack([R * nrm[:, 0], R * nrm[:, 1], z], 1), nrm
    if kind == "polygon":  # inside a triangle of the tiling, drawn towards its centroid: >= a fifth of its inradius from every edge
        pieces = np.stack(form_scenes.polygon_pieces(spec[1]))
        tri = pieces[rng.integers(0, len(pieces), n)]
        w = 0.8 * rng.dirichlet([1.0, 1.0, 1.0], n) + 0.2 / 3.0
        yz = np.einsum("nk,nkc->nc", w, tri)
        p = form_scenes.POLYGONS[spec[1]]
        if "place" not in p:
            return np.stack([np.zeros(n), yz[:, 0], yz[:, 1]], 1), np.tile([1.0, 0.0, 0.0], (n, 1))
        return form_scenes._place(p["place"], yz), np.tile(form_scenes.polygon_normal(spec[1]), (n, 1))
    raise KeyError(kind)


def _asphere_targets(rng, F, radius, share, n):
    phi = rng.uniform(-np.pi, np.pi, n)
    r = share * radius * np.sqrt(rng.uniform(0.01, 1, n))
    h = 1e-6
    slope = (F(r + h) - F(r - h)) / (2 * h)
    P = np.stack([-F(r), r * np.cos(phi), r * np.sin(phi)], 1)
    return P, _unit(np.stack([np.ones(n), slope * np.cos(phi), slope * np.sin(phi)], 1))


def f32(x):
    """float32 values widened to double: what the device reads"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _rays(name, seed):
    import optable_amd as oa

    form = FORMS[name]
    comp = leaf(oa, name)
    M, g = np.asarray(comp.transform_matrix, dtype=float), np.asarray(comp.origin, dtype=float)
    rng = np.random.default_rng([seed, NAMES.index(name)])
    fan, n = form.fan, N_RAYS
    if fan["target"][0] == "asphere":
        P, nrm = _asphere_targets(rng, comp.surface.f_asphere, fan["target"][1], fan["target"][2], n)
    else:
        P, nrm = _targets(rng, fan["target"], n)
    inc = np.radians(rng.uniform(*fan["incidence"], n))
    psi = rng.uniform(-np.pi, np.pi, n)
    helper = np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    e1 = _unit(np.cross(nrm, helper))
    e2 = np.cross(nrm, e1)
    d = -fan["side"] * np.cos(inc)[:, None] * nrm + np.sin(inc)[:, None] * (np.cos(psi)[:, None] * e1 + np.sin(psi)[:, None] * e2)
    s = rng.uniform(*fan.get("distance", (4.0, 9.0)), n)
    o = P - s[:, None] * d
    o, d = o @ M.T + g, _unit(d @ M.T)
    wl = np.asarray(form.wavelengths_nm or (W.WL / 1e-7,), dtype=float) * 1e-7  # model units: 1e-2 m
    copies = len(wl)
    rays = {"ox": o[:, 0], "oy": o[:, 1], "oz": o[:, 2], "dx": d[:, 0], "dy": d[:, 1], "dz": d[:, 2]}
    rays = {k: np.tile(f32(v), copies) for k, v in rays.items()}
    total = n * copies
    rays["wavelength"] = f32(np.repeat(wl, n))
    rays["q_re"] = np.full(total, f32(Q_IN.real) if form.has_q else 0.0)
    rays["q_im"] = np.full(total, f32(Q_IN.imag) if form.has_q else 0.0)
    rays["intensity"] = np.full(total, f32(I_IN))
    rays["n"] = np.full(total, f32(form.n_in))
    rays["pathlength"] = np.full(total, f32(PL_IN))
    rays["id"] = np.arange(total, dtype=np.int32)
    rays["flags"] = np.full(total, abi.RAY_HAS_Q if form.has_q else 0, dtype=np.int32)
    for v in rays.values():
        v.setflags(write=False)
    return rays


def rays(name, seed=0):
    """The host rays of a form (abi.RAY_FIELDS, id, flags): float32 values widened to double, read-only.  Wavelength-multiplexed
    forms: the fan once per wavelength, wavelength-major (RayBatch.multiplexed_in_wavelength's order)."""
    return _rays(name, seed)


def subset(rays_, index):
    out = {k: np.ascontiguousarray(v[index]) for k, v in rays_.items()}
    out["id"] = np.arange(len(out["ox"]), dtype=np.int32)
    return out


def device_batch(rays_, device="cuda"):
    """The fp32 RayBatch of host rays: their very bit patterns (nothing is normalised or rounded again)."""
    from optable_amd.batch import RayBatch

    has_q = bool(rays_["flags"][0] & abi.RAY_HAS_Q)
    return RayBatch.from_arrays(np.stack([rays_["ox"], rays_["oy"], rays_["oz"]], 1), np.stack([rays_["dx"], rays_["dy"], rays_["dz"]], 1),
                                wavelength=rays_["wavelength"], intensity=rays_["intensity"], q=(rays_["q_re"] + 1j * rays_["q_im"]) if has_q else None,
                                n_index=rays_["n"], pathlength=rays_["pathlength"], precision="f32", device=device, normalize=False)


# -- the bound ---------------------------------------------------------------------------------------------------------------------
Bound = namedtuple("Bound", "ref tol excluded first N")
# ref: the oracle's records (reference order); tol: {field: [records]} (segment 0: only `length` is used — the rest is compared bit
# for bit with the input); excluded: [input rays] bool; first: [records] bool, segment 0 of its ray; N: per field group


def _moved(rays_, rng):
    """every component of o and d, the wavelength and q one ulp of float32 up or down, the sign drawn per ray and component"""
    out = dict(rays_)
    fields = ["ox", "oy", "oz", "dx", "dy", "dz", "wavelength"] + (["q_re", "q_im"] if rays_["flags"][0] & abi.RAY_HAS_Q else [])
    for f in fields:
        x = rays_[f].astype(np.float32)
        up = rng.integers(0, 2, len(x)).astype(bool)
        out[f] = np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float64)
    return out


def _signature(trace, n):
    """per input ray: the surfaces of its records in order, and for every child whether it kept its parent's index (the
    total-reflection decision shows there and in the number of children)"""
    sig = [[] for _ in range(n)]
    parent_n = {}
    for ray, surf, idx in zip(trace["ray"].tolist(), trace["surface"].tolist(), trace["n"].tolist()):
        if ray not in parent_n:
            parent_n[ray] = idx
            sig[ray].append(surf)
        else:
            sig[ray].append((surf, idx == parent_n[ray]))
    return sig


def bound(scene, rays_, K, N, seed=0):
    """The oracle's records of `rays_` (float32 values widened to double) through `scene` and the tolerance of every record and
    field, N (u S + D), from the oracle alone (module docstring).  Returns a Bound."""
    from oracle import oracle as orc

    n = len(rays_["ox"])
    ref = orc.trace(scene, rays_, max_trace_num=K)
    ray = np.asarray(ref["ray"])
    sig = _signature(ref, n)
    excluded = np.zeros(n, dtype=bool)
    spread = {f: np.zeros(len(ray)) for f in REAL_FIELDS}
    rng = np.random.default_rng([seed, 0xF32])
    for _ in range(RUNS):
        alt = orc.trace(scene, _moved(rays_, rng), max_trace_num=K)
        alt_sig = _signature(alt, n)
        changed = np.array([a != b for a, b in zip(sig, alt_sig)])
        excluded |= changed
        keep_ref, keep_alt = ~changed[ray], ~changed[np.asarray(alt["ray"])]
        for f in REAL_FIELDS:
            a, b = np.asarray(ref[f])[keep_ref], np.asarray(alt[f])[keep_alt]
            with np.errstate(invalid="ignore"):
                diff = np.where(np.isfinite(a) & np.isfinite(b), np.abs(a - b), 0.0)
            spread[f][keep_ref] = np.maximum(spread[f][keep_ref], diff)
    first = np.r_[True, ray[1:] != ray[:-1]]
    # per record: the input ray's fields and the length t of its segment 0
    t0 = np.asarray(ref["length"])[first]
    seg0_ray = ray[first]
    t = np.full(n, np.inf)
    t[seg0_ray] = t0
    t = t[ray]
    leaf_origin = max(max(abs(x) for x in nd.origin[:]) for nd in scene.nodes[: scene.n_nodes])
    o_in = np.maximum.reduce([np.abs(rays_[f]) for f in ("ox", "oy", "oz")])[ray]
    with np.errstate(invalid="ignore"):
        S = {"o": np.maximum.reduce([o_in, np.full(len(ray), leaf_origin), np.where(np.isfinite(t), t, 0.0)]),
             "d": np.ones(len(ray)),
             "n": np.abs(ref["n"]), "intensity": np.abs(ref["intensity"]),
             "pathlength": np.abs(rays_["pathlength"][ray]) + np.where(np.isfinite(t), t, 0.0) * rays_["n"][ray],
             "q": np.hypot(rays_["q_re"][ray] + np.where(np.isfinite(t), t, 0.0), rays_["q_im"][ray])}
    S["length"] = S["o"]
    tol = {}
    for f in REAL_FIELDS:
        grp = GROUPS[f]
        tol[f] = N[grp] * (U * S[grp] + spread[f])
        tol[f][excluded[ray]] = np.inf
    return Bound(ref, tol, excluded, first, dict(N))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(compiled scene, host rays, K, Bound) of a form: computed once, shared by every test, never written to."""
    scene, r, K = compiled(name), rays(name), max_trace_num(name)
    return scene, r, K, bound(scene, r, K, N_of(name))


def _bits32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).view(np.int32)


def compare(bnd, rays_, got, only_rays=None):
    """A trace `got` (dict of abi.SEG_FIELDS, `ray`, `surface` in the reference's order; float32 widened or double) against a
    Bound.  Every ray that is not excluded: the same records in the same order, `ray` and `surface` equal; segment 0's o, d,
    intensity, q, n and pathlength the input's float32 bit patterns; segment 0's finite `length` and every field of the later
    records inside their tolerance; `length` infinite exactly where the oracle's is.  only_rays: {ray index of `got`: ray index of
    the bound} for a trace of a subset.  Returns (violations: list of strings, worst: {field: largest error / tolerance})."""
    ref, bad, worst = bnd.ref, [], {}
    ref_ray, got_ray = np.asarray(ref["ray"]), np.asarray(got["ray"])
    if only_rays is not None:
        lut = np.full(int(got_ray.max()) + 1 if len(got_ray) else 1, -1)
        for a, b in only_rays.items():
            lut[a] = b
        got_ray = lut[got_ray]
        sel = np.isin(ref_ray, list(only_rays.values()))
    else:
        sel = np.ones(len(ref_ray), dtype=bool)
    if len(got_ray) and (got_ray.min() < 0 or got_ray.max() >= len(bnd.excluded)):
        return [f"records: of rays {int(got_ray.min())} .. {int(got_ray.max())}, which the batch does not hold"], worst
    sel &= ~bnd.excluded[ref_ray]
    gsel = ~bnd.excluded[got_ray]
    if sel.sum() != gsel.sum() or not np.array_equal(ref_ray[sel], got_ray[gsel]):
        return [f"records: {int(gsel.sum())} of rays in another order or number than the oracle's {int(sel.sum())}"], worst
    rr = ref_ray[sel]
    surf_ref, surf_got = np.asarray(ref["surface"])[sel], np.asarray(got["surface"])[gsel]
    if not np.array_equal(surf_ref, surf_got):
        k = np.flatnonzero(surf_ref != surf_got)
        bad.append(f"surface: {len(k)} records differ, first ray {int(rr[k[0]])}: {int(surf_got[k[0]])} for {int(surf_ref[k[0]])}")
    first = bnd.first[sel]
    for f in REAL_FIELDS:
        x, want, tol = np.asarray(got[f], dtype=np.float64)[gsel], np.asarray(ref[f], dtype=np.float64)[sel], bnd.tol[f][sel]
        if f == "length":
            inf = np.isinf(want)
            if not np.array_equal(x[inf], want[inf]):
                bad.append("length: not infinite where the oracle's is")
            check = ~inf
        else:
            src = rays_["n" if f == "n" else f]
            exact = _bits32(x[first]) == _bits32(src[rr[first]])
            if not exact.all():
                bad.append(f"{f}: segment 0 of {int((~exact).sum())} rays is not the input's bit pattern, first ray {int(rr[first][np.flatnonzero(~exact)[0]])}")
            check = ~first
        with np.errstate(invalid="ignore"):
            err = np.abs(x[check] - want[check])
            ratio = err / tol[check]
        ok = err <= tol[check]  # (a NaN fails)
        worst[f] = float(np.nanmax(ratio)) if len(ratio) else 0.0
        if not ok.all():
            k = np.flatnonzero(~ok)
            j = k[np.argmax(np.where(np.isnan(ratio[k]), np.inf, ratio[k]))]
            bad.append(f"{f}: {len(k)} records outside N (u S + D), N = {bnd.N[GROUPS[f]]}; worst ray {int(rr[check][j])}: {x[check][j]!r} for {want[check][j]!r}, "
                       f"error {err[j]:.3e} = {ratio[j]:.2f} x its bound {tol[check][j]:.3e}")
    return bad, worst
