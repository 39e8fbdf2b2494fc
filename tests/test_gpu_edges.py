"""GPU: rays aimed at decision boundaries, every kernel family, against the oracle.

Random rays rarely come within 1e-9 of an aperture edge, so the differential fuzz tests say little about the rays that
decide between two surfaces.  Here every ray is marginal on purpose: for each aperture family (circle, rectangle,
polygon, cylinder theta end, sphere cap, asphere, boolean aperture), for total internal reflection at the critical
angle and for two mirrors through one line (a tie), rays start at signed offsets of 1e-3 .. 1e-12 scene units from the
decision; so do rays at the decisions of a spherical cap's root search (the rim and the local box of a cap deeper than a
hemisphere, a tangent line, a chord as long as the scan's sample step, a hit at the t = 100 cut) and at a reflex vertex and
a vertex level of a concave polygon.  The oracle confirms which side each ray is on.  They are traced in fp64 and fp32, by the default call and
by the forced lane-per-ray and rolling-list kernels in the slots, tiled and append layouts, in batches that are not
multiples of 64 with the marginal rays in the last partial wave:
  - fp64 rays whose offset is above the fp64 floor match the oracle exactly (sequence; fields within 1e-9),
  - fp32 rays whose offset is at least 1e-4 take the oracle's sequence,
  - every other ray is explained by the divergence audit (optable_amd.fp32_audit)."""
import numpy as np
import pytest

import optable_amd as oa
import scenes
from optable_amd import abi
from optable_amd.batch import RayBatch
from optable_amd.engine import get_engine
from optable_amd.fp32_audit import FLOOR, assert_explained, audit_traces

pytestmark = pytest.mark.gpu
OFFSETS = np.array([s * m for m in (1e-3, 1e-6, 1e-9, 1e-12) for s in (1, -1)])
Q = 1j * np.pi * scenes.W0**2 / scenes.WL
K = 8
# (OPT_KERNEL, layout): the default call, and each kernel family forced, in every layout it writes (the append list is
# written by the rolling-list kernel only)
LAUNCHES = [(None, "auto"), (1, "slots"), (1, "tiled"), (2, "slots"), (2, "append")]


def _rim_rays(offsets, at, step, d):
    """Rays that start at `at` + offset * `step` (unit `step`, across the decision), all with direction d."""
    at, step, d = (np.asarray(v, float) for v in (at, step, d))
    o = at[None, :] + offsets[:, None] * step[None, :]
    return o, np.tile(d, (len(o), 1))


def _family(name):
    """Components, marginal rays (o, d, offset) and a filler ray far from any decision."""
    back = oa.Mirror([9, 0, 0], radius=4.0)  # catches the rays that miss the boundary leaf
    if name == "circle":
        comps = [oa.Mirror([5, 0, 0], radius=1.0), back]
        phi = np.repeat([0.0, 0.7, 2.0, -2.6], len(OFFSETS))
        r = 1.0 + np.tile(OFFSETS, 4)
        o = np.stack([np.zeros_like(r), r * np.cos(phi), r * np.sin(phi)], 1)
        d = np.tile([1.0, 0, 0], (len(o), 1))
        return comps, o, d, np.tile(OFFSETS, 4), ([0, 0.3, 0.1], [1, 0, 0])
    if name == "rectangle":
        comps = [oa.SquareMirror([5, 0, 0], width=1.6, height=1.2), back]
        o1, d1 = _rim_rays(OFFSETS, [0, 0.8, 0.2], [0, 1, 0], [1, 0, 0])
        o2, d2 = _rim_rays(OFFSETS, [0, -0.3, -0.6], [0, 0, -1], [1, 0, 0])
        return comps, np.r_[o1, o2], np.r_[d1, d2], np.r_[OFFSETS, OFFSETS], ([0, 0.1, 0.1], [1, 0, 0])
    if name == "polygon":
        tri = oa.BaseMirror([5, 0, 0])
        tri.surface = oa.Polygon(np.array([[-1.0, -1.0], [1.0, -1.0], [0.0, 1.0]]))
        nrm = np.array([0, 2, 1]) / np.sqrt(5)
        at = np.array([0, 0.5, 0.0]) + 1e-9 / np.sqrt(5) * nrm  # |cross| <= 1e-9 counts as inside (surfaces.py:534-558)
        o1, d1 = _rim_rays(OFFSETS, at, nrm, [1, 0, 0])
        o2, d2 = _rim_rays(OFFSETS, [0, 0.0, -1.0 - 1e-9 / 2], [0, 0, -1], [1, 0, 0])  # the base edge, length 2
        return [tri, back], np.r_[o1, o2], np.r_[d1, d2], np.r_[OFFSETS, OFFSETS], ([0, 0, -0.2], [1, 0, 0])
    if name == "cylinder":
        cyl = oa.CylMirror([0, 0, 0], radius=1.2, height=2.0, theta_range=(np.pi / 2, np.pi))
        o1, d1 = _rim_rays(OFFSETS, [0, 5, 0.3], [1, 0, 0], [0, -1, 0])  # theta = pi/2 -/+ x / R: outside for x > 0
        o2, d2 = _rim_rays(OFFSETS, [-0.8, 5, 1.0], [0, 0, 1], [0, -1, 0])  # the z = +height/2 rim
        return [cyl], np.r_[o1, o2], np.r_[d1, d2], np.r_[OFFSETS, OFFSETS], ([-0.5, 5, 0], [0, -1, 0])
    if name == "sphere_cap":
        cap = oa.SphereRefractive([0, 0, 0], radius=5.0, height=2.0, n1=1.0, n2=1.0, reflectivity=1.0, transmission=0.0)
        # rim: x = R - h = 3, r = 4; rays along +x at r = 4 + offset
        o, d = _rim_rays(OFFSETS, [-6, 4.0, 0], [0, 1, 0], [1, 0, 0])
        return [cap], o, d, OFFSETS, ([-6, 1.0, 0.5], [1, 0, 0])
    if name == "asphere":
        bowl = oa.BaseRefraciveSurface(origin=[0, 0, 0], n1=1.0, n2=1.0, surface=oa.ASphere(3.0, oa.sag_parametric(1.0, -1.0)),
                                       reflectivity=1.0, transmission=0.0)
        o, d = _rim_rays(OFFSETS, [-8, 0, 3.0], [0, 0, 1], [1, 0, 0])
        return [bowl, oa.Mirror([-9, 0, 0], radius=6.0)], o, d, OFFSETS, ([-8, 1.0, 0.5], [1, 0, 0])
    if name == "boolean":
        plate = oa.Block([5, 0, 0], hole=oa.Circle(0.5), width=2, height=2)
        o, d = _rim_rays(OFFSETS, [0, 0.5, 0], [0, 1, 0], [1, 0, 0])
        return [plate, back], o, d, OFFSETS, ([0, 0.1, 0.1], [1, 0, 0])
    if name == "tir":
        face = oa.BaseRefraciveSurface([0, 0, 0], n1=1.5, n2=1.0, surface=oa.Rectangle(4, 4))
        s = 1 / 1.5 + OFFSETS  # sin of the incidence angle: the critical angle + offset (inside the n1 = 1.5 side)
        d = np.stack([-np.sqrt(1 - s * s), s, np.zeros_like(s)], 1)
        o = -d / np.sqrt(1 - s[:, None] ** 2)  # start at x = 1, reach the face at its centre
        return [face, oa.Mirror([3, 0, 0], radius=5.0)], o, d, OFFSETS, ([1, -0.5, 0], [-1, 0.5, 0])
    if name == "tie":
        comps = [oa.Mirror([5, 0, 0], radius=1.0), oa.Mirror([5, 0, 0], radius=1.0).RotZ(0.1)]
        o, d = _rim_rays(OFFSETS, [0, 0, 0.3], [0, 1, 0], [1, 0, 0])
        return comps, o, d, OFFSETS, ([0, 0.5, 0], [1, 0, 0])
    if name.startswith("sphere_") and name != "sphere_t100":
        # a reflective cap deeper than a hemisphere: x in [R - h, R] = [-1.2, 2]; its local box has the half-width a = 1.6 < R
        R, h = DEEP_CAP
        cap = oa.SphereRefractive([0, 0, 0], radius=R, height=h, n1=1.0, n2=1.0, reflectivity=1.0, transmission=0.0)
        a = cap.surface.get_bbox_local()[3]
        eps = 1e-9  # the reference's EPS: the search interval is the box crossing widened by it at both ends
        if name == "sphere_deep_rim":  # along +x at r = a + offset, on the diagonal (inside the box): the first root has x = -sqrt(R^2 - r^2),
            # on the cap for r >= a; below that the ray enters through the mouth and meets the crown from inside
            u = np.array([0, 1, 1]) / np.sqrt(2)
            o, d = _rim_rays(OFFSETS, np.array([-6.0, 0, 0]) + a * u, u, [1, 0, 0])
        elif name == "sphere_box_face":  # along +x at y = a + offset, z = 0.5: the belly (x = -1.09) is searched from inside the box only
            o, d = _rim_rays(OFFSETS, [-6, a, 0.5], [0, 1, 0], [1, 0, 0])
        elif name == "sphere_tangent":  # along +y, at R + offset from the centre; from y = -a / 2 the point of contact is sample 3 of the
            # scan (0, a / 6, .., 1.5 a), so a chord of any length has its roots in two intervals
            u = np.array([0.8, 0, 0.6])
            o, d = _rim_rays(OFFSETS, R * u + [0, -a / 2, 0], u, [0, 1, 0])
        elif name == "sphere_chord":  # along +y across the whole box, the chord centred in the middle interval: found iff chord > step
            step = (2 * a + 2 * eps) / 9
            x = np.sqrt(R * R - ((step + OFFSETS) / 2) ** 2)
            o = np.stack([x, np.full_like(x, -5.0), np.zeros_like(x)], 1)
            d = np.tile([0.0, 1.0, 0.0], (len(o), 1))
        else:
            raise KeyError(name)
        return [cap], o, d, OFFSETS, ([-6, 0.3, 0.2], [1, 0, 0])
    if name == "sphere_t100":  # a hit at t = 100 + offset (the search ends at min(t2, 100) + EPS): the crown at x = 0, centre at x = -R
        R = T100_X - 100.0
        cap = oa.SphereRefractive([-R, 0, 0], radius=R, height=0.5, n1=1.0, n2=1.0, reflectivity=1.0, transmission=0.0)
        x_hit = -R + np.sqrt(R * R - 0.25)
        o, d = _rim_rays(OFFSETS, [x_hit + 100.0 + 1e-9, 0.5, 0], [1, 0, 0], [-1, 0, 0])
        return [cap, oa.Mirror([-3, 0, 0], radius=4.0)], o, d, OFFSETS, ([50, 0.1, 0.2], [-1, 0, 0])
    if name.startswith("polygon_"):
        stop = oa.BaseMirror([5, 0, 0])
        if name == "polygon_concave_vertex":  # the reflex vertex (0, -0.2) of the arrow, along its bisector +z; |cross| <= 1e-9 counts as
            # inside (surfaces.py:534-558): 0.9 * depth for the two edges that meet there
            stop.surface = oa.Polygon(np.array([(0.0, 1.0), (-0.9, -0.8), (0.0, -0.2), (0.9, -0.8)]))
            o, d = _rim_rays(OFFSETS, [0, 0.0, -0.2 - 1e-9 / 0.9], [0, 0, 1], [1, 0, 0])
        elif name == "polygon_level_vertex":  # the edge y = -0.25 of an L, from outside (+) to inside: the even-odd test casts its ray
            # along +z, i.e. along that edge and through the vertex (-0.25, 1) at its end; the edge has the length 1.25
            stop.surface = oa.Polygon(np.array([(-0.75, -1.0), (0.75, -1.0), (0.75, -0.25), (-0.25, -0.25), (-0.25, 1.0), (-0.75, 1.0)]))
            o, d = _rim_rays(OFFSETS, [0, -0.25 + 1e-9 / 1.25, 0.3], [0, 1, 0], [1, 0, 0])
        else:
            raise KeyError(name)
        return [stop, back], o, d, OFFSETS, ([0, -0.5, -0.6], [1, 0, 0])
    raise KeyError(name)


DEEP_CAP = (2.0, 3.2)
T100_X = 120.0  # sphere_t100: the largest coordinate of the decision, the ray's start in the frame of the cap (its centre)
FAMILIES = ["circle", "rectangle", "polygon", "cylinder", "sphere_cap", "asphere", "boolean", "tir", "tie",
            "sphere_deep_rim", "sphere_box_face", "sphere_tangent", "sphere_chord", "sphere_t100", "polygon_concave_vertex", "polygon_level_vertex"]
# fp32, "clear of the decision": 1e-4, or 16 ulp_f32(X) where the decision involves a coordinate or distance X so large that
# this is more: an offset below a few ulp of X does not survive the rounding of the ray to single precision (t = 100 is
# the difference of two coordinates of that size, each rounded to ulp / 2, and the root adds a few more)
FP32_SCALE = {"sphere_t100": T100_X}


def fp32_clear(family):
    return max(1e-4, 16.0 * float(np.spacing(np.float32(FP32_SCALE.get(family, 1.0)))))


def _batch(o, d, off, filler, n):
    """n rays: filler rays first, the marginal rays last (the last one alone in the final partial wave when n % 64 == 1)."""
    m = min(len(o), n)
    fo, fd = (np.tile(np.asarray(v, float), (n - m, 1)) for v in filler)
    oo, dd = np.r_[fo, o[-m:]], np.r_[fd, d[-m:]]
    offs = np.r_[np.full(n - m, np.inf), off[-m:]]
    return oo, dd, offs


def _trace(table, o, d, prec, kernel, layout):
    eng = get_engine()
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=Q, precision=prec)
    if kernel is None:
        return table.trace_batch(batch, max_segments=K), eng.last_launch()
    eng.set_option(abi.OPT_KERNEL, kernel)
    try:
        segs = table.trace_batch(batch, max_segments=K, layout=layout)
        info = eng.last_launch()
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
    assert info["kernel"] == kernel, (kernel, layout, info)
    assert segs.layout == layout, (segs.layout, layout)
    return segs, info


def _rays_of(x, rays):
    keep = np.isin(x["ray"], rays)
    return {k: (v[keep] if k in abi.SEG_FIELDS + ("ray", "surface") else v) for k, v in x.items()}


@pytest.mark.parametrize("family", FAMILIES)
def test_marginal_rays_on_every_kernel(family, oracle):
    comps, o, d, off, filler = _family(family)
    table = oa.OpticalTable()
    table.add_components(comps)
    scene = table.compile()
    # the construction really straddles the decision: the oracle sends the +1e-3 and -1e-3 rays different ways
    host = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=Q, device="cpu").to_host()
    ref0 = oracle.trace(scene, host, max_trace_num=K)
    seq = lambda x, i: tuple(x["surface"][x["ray"] == i].tolist())
    plus, minus = ({seq(ref0, int(i)) for i in np.flatnonzero(sg * off > 0)} for sg in (1, -1))
    assert not plus & minus, (family, plus, minus)
    for n in (1, 63, 65, 4097):
        oo, dd, offs = _batch(o, d, off, filler, n)
        host = RayBatch.from_arrays(oo, dd, wavelength=scenes.WL, q=Q, device="cpu").to_host()
        ref = oracle.trace(scene, host, max_trace_num=K)
        for prec in ("f64", "f32"):
            for kernel, layout in LAUNCHES if n != 1 else LAUNCHES[:2]:
                segs, info = _trace(table, oo, dd, prec, kernel, layout)
                got = segs.to_host(reference_order=True)
                where = f"{family} n={n} {prec} kernel={kernel} layout={layout} launch={info}"
                tol = 1e-9 if prec == "f64" else 2e-3
                rep = audit_traces(scene, ref, got, prec=prec, tol=tol, rays=host)
                try:
                    assert_explained(rep)
                except AssertionError as e:
                    raise AssertionError(f"{where}\n{e}") from None
                # rays clear of the decision take the oracle's path exactly
                clear = np.abs(offs) > (FLOOR["f64"] if prec == "f64" else fp32_clear(family) - 1e-12)
                bad = [int(r) for r in rep["ray"] if clear[r]]
                assert not bad, (where, bad, offs[bad])
                if prec == "f64":  # ... and its fields to 1e-9
                    rays = np.flatnonzero(clear)
                    a, b = _rays_of(got, rays), _rays_of(ref, rays)
                    np.testing.assert_array_equal(a["ray"], b["ray"], err_msg=where)
                    np.testing.assert_array_equal(a["surface"], b["surface"], err_msg=where)
                    for f in ("ox", "oy", "oz", "dx", "dy", "dz", "length", "intensity", "pathlength"):
                        np.testing.assert_allclose(a[f], b[f], rtol=1e-9, atol=1e-9, err_msg=f"{where} {f}")
