"""The surface-form catalogue: one small scene per FORM of a shape the trace kernels branch on — every conic and polynomial
variant of the parametric asphere (both orientations, the exact plano-convex sag, reflective bowls that a ray meets more
than once), the arcs of the built-in cylinder wall, boolean apertures with a union, a polygon operand and nested
programs, spherical caps from shallow to nearly full (both orientations, a full sphere that is never hit, mirror-coated
bowls, rays that start inside the ball, chords as short as the scan's sample step, a cap beyond the t = 100 cut of the
search, a deep cap in a group) and polygons (concave, clockwise, self-overlapping, with edges along the cast ray of the
even-odd test, and as 3-D polygons on either in-plane basis, with a derived normal, in a coordinate plane).  Written against
a namespace `ns` like tests/scenes.py, so the same builder runs on the reference (tools/make_golden.py records
`scene(ns, name)` into tests/golden/g30-g35) and on this package.  NOT part of
scenes.SCENES: the existing parametrised tests and g28_adapter.npz stay as they are.

    NAMES, FAMILY[name]          every form and the fixture file it is recorded in
    components(ns, name, split)  the scene; split=True: the form's interface splits every ray (reflectivity 0.3), planar
                                 forms and 3-D polygons get a GlassSlab(reflectivity=0.2) in front instead
    fan(name, n, seed)           the batch ray fan of the form: (origins, directions)
    scene(ns, name)              the object-API scene of the fixtures (<= 40 Ray objects of the same fan, cap <= 12)
    form_leaves(scene, name)     indices of the leaves that carry the form under test
    curved_scene, curved_scene_deep_caps, curved_deep_case   random curved scenes whose parts are drawn from the catalogue
    named(form)                  a context in which every failure names the form
"""
import contextlib

import numpy as np

from optable_amd.workloads import WL, W0


@contextlib.contextmanager
def named(form):
    """Every failure names the form."""
    try:
        yield
    except AssertionError as exc:
        raise AssertionError(f"surface form {form!r}: {exc}") from exc


# -- aspheres: ASphericParametricLens([4, 0.1, 0], CT=0.6, diameter=2.4, n=1.5, **form), as built and turned by RotZ(pi) ------
ASPHERES = {
    "sphere": dict(R=8, kappa=0),
    "oblate": dict(R=8, kappa=0.6),
    "prolate": dict(R=8, kappa=-0.5),
    "parabola": dict(R=8, kappa=-1),                                   # the control: the only form the other suites build
    "hyperbola": dict(R=8, kappa=-2.5),
    "negative_R": dict(R=-8, kappa=-0.5),                              # the DN_CONVEX_NEG side of the classifier
    "all_terms": dict(R=8, kappa=-0.5, a4=2e-3, a6=-1e-3, a8=5e-4),
    "wavy": dict(R=1e6, kappa=0, a4=5e-3, a6=0, a8=-1e-3),             # F'' changes sign at r ~ 1.02: no convexity flag
    "strong": dict(R=3, kappa=2),                                      # radicand 0.04 at the corner of the local box
    "beyond_domain": dict(R=3, kappa=4),                               # NaN inside the local box: no flag, full scan
    "edge": dict(R=2.2, kappa=1.6),
}
# forms whose sag is real on the whole local box (r up to radius * sqrt 2): what the random curved scenes draw from
IN_DOMAIN = ("sphere", "oblate", "prolate", "parabola", "hyperbola", "negative_R", "all_terms", "wavy", "strong")
EXACT = {"exact_long": dict(EFL=6.0, n=1.5), "exact_short": dict(EFL=3.0, n=1.8)}
# reflective bowls ASphere(radius, sag_parametric(R, kappa)): deep enough that a ray meets the same surface again
BOWLS = {
    "bowl_oblate": dict(radius=1.5, R=2.0, kappa=0.6, side=-1),       # radicand < 0 beyond r = 1.58, inside the local box: NaN
                                                                       # samples next to negative ones on the way out of the bowl
    "bowl_hyperbola": dict(radius=2.0, R=0.3, kappa=-2.5, side=-1),
    "bowl_negative_R": dict(radius=2.2, R=-2.0, kappa=-0.5, side=+1),   # opens towards +x: the rays come from there
}
# -- cylinders: CylMirror([5, 0, 0], radius=1.5, height=2.0, theta_range=arc) ------------------------------------------------
CYLINDERS = {
    "cyl_full_turn": dict(arc=None, rot=0.0),
    "cyl_across_zero": dict(arc=(-np.pi / 4, np.pi / 4), rot=0.0),
    "cyl_ends_at_minus_pi": dict(arc=(-np.pi, -np.pi / 2), rot=0.0),
    "cyl_wide_rotated": dict(arc=(-3 * np.pi / 4, 3 * np.pi / 4), rot=0.3),
}
TRIANGLE = [(-0.6, -0.5), (0.7, -0.4), (0.1, 0.8)]
# -- boolean apertures on a BaseMirror([5, 0, 0]), a back mirror behind it: (aperture builder, half extents of the fan) --------
APERTURES = {
    "csg_union": (lambda ns: ns.Rectangle(1, 2.2).union(ns.Circle(0.8)), (0.85, 1.15)),
    "csg_nested": (lambda ns: ns.Rectangle(2, 2).subtract(ns.Circle(0.5)).union(ns.Rectangle(0.2, 3)), (1.05, 1.2)),
    "csg_polygon": (lambda ns: ns.Rectangle(2.4, 2).subtract(ns.Polygon(TRIANGLE)), (1.3, 1.1)),
    "csg_island": (lambda ns: ns.Circle(1.3).subtract(ns.Rectangle(1, 1).subtract(ns.Circle(0.3))), (1.2, 1.2)),
    "csg_deeper": (lambda ns: ns.Circle(1.3).subtract(ns.Rectangle(1, 1).subtract(ns.Circle(0.3).subtract(ns.Rectangle(0.25, 0.15)))),
                   (1.2, 1.2)),
}

# -- spherical caps: SphereRefractive([0, 0, 0], R, h, n1=1, n2=1.5), the crown at local x = +R, the cap x in [R - h, R].  The local
# box of a cap has the half-width a = sqrt(R^2 - (R - h)^2) in y and z: a cap deeper than a hemisphere (h > R) has a < R and its
# belly lies OUTSIDE the box that clips the root search.  `fan`: "disc" rays from +x onto the crown (as built) or into the mouth
# (turned), disc radius `spread` * a; "mouth" rays from -x into a reflective cap; the other fans are the form's own.
CAPS = {
    "shallow": dict(R=5.0, h=0.5, spread=0.93),        # the control: the only kind of cap the other suites build (h < R)
    "hemisphere": dict(R=2.0, h=2.0, spread=1.04),     # h == R: the first cap on the x-bound side of the upload's choice
    "deep": dict(R=2.0, h=3.2, spread=1.15),           # a = 1.6 < R: rays beyond the box's faces see no belly
    "nearly_full": dict(R=2.0, h=3.9, spread=1.15),    # a = 0.62
}
# Catch mirrors (`catch`): "both" sides where the rays stay near the axis; a strongly curved refracting cap that a ray meets
# again after a catch mirror is met near the critical angle or grazing by some rays, whose further path then amplifies a
# last-digit difference 1e4-fold: no trace defines it to 1e-9 (tests/test_surface_forms_cpu.py bounds the amplification of
# every fan).  So as built the hemisphere and the deep cap are crossed once; turned, with the mouth towards the rays, they
# have the mirror behind the crown only, and the turned hemisphere a narrower fan.
_CATCH = {"sph_shallow": "both", "sph_shallow_turned": "both", "sph_nearly_full": "both", "sph_nearly_full_turned": "both", "sph_full": "both",
          "sph_hemisphere": None, "sph_deep": None, "sph_hemisphere_turned": "behind", "sph_deep_turned": "behind"}
SPHERES = {
    **{f"sph_{k}{t}": dict(c, fan="disc", turned=bool(t)) for k, c in CAPS.items() for t in ("", "_turned")},
    # height 2 R, the documented default (height=None itself raises in the reference's constructor and in this package's):
    # a = 0, a local box of zero width, which no ray of the fan crosses: the full sphere is NEVER hit
    "sph_full": dict(R=2.0, h=4.0, spread=0.93, fan="disc", never_hit=True),
    # mirror-coated caps (n2 = 1 like n1: with glass behind the coat, total reflection would add a second child and make the
    # trace a ray tree): every further hit is on the same leaf, on its concave side
    "sph_bowl_hemisphere": dict(R=2.0, h=2.0, spread=0.82, fan="mouth", mirror=True),  # (rays nearer the rim go round it grazing)
    "sph_bowl_deep": dict(R=2.0, h=3.2, spread=0.93, fan="mouth", mirror=True),
    "sph_inside": dict(R=2.0, h=3.2, fan="inside", mirror=True),       # rays that start inside the ball (g < 0 at the first sample)
    "sph_chords": dict(R=2.0, h=2.0, fan="chords", mirror=True),       # short chords through the crown: the same-interval rule
    "sph_far": dict(R=30.0, h=0.5, fan="far"),                         # the crown 85 - 115 from the ray origins: the t = 100 cut
    "sph_in_group": dict(R=2.0, h=3.2, spread=1.15, fan="disc", group=True),
}
SPHERES["sph_hemisphere_turned"]["spread"] = 0.85
for _k, _v in _CATCH.items():
    SPHERES[_k]["catch"] = _v
NEVER_HIT = tuple(k for k, s in SPHERES.items() if s.get("never_hit"))
CHORD_DELTAS = ((0.003, 0.0105), (0.0145, 0.06))  # sph_chords: R - (distance of the ray to the y axis of the cap), missing / hitting
FAR_DISTANCES = ((100.7, 115.0), (85.0, 99.3))    # sph_far: crown to ray origin, beyond / before the cut


def chord_threshold(R, crossing):
    """delta* of a ray that crosses the local box of a cap over the length `crossing`, symmetric about its closest approach
    to the centre, at the distance R - delta from it: the chord 2 sqrt(R^2 - (R - delta)^2) equals the sample step
    crossing / 9 of the ten-point scan.  A shorter chord lies inside the middle sample interval: no sign change, no hit."""
    return R - np.sqrt(R * R - (crossing / 9.0) ** 2 / 4.0)


# -- polygons on a BaseMirror([5, 0, 0]), a back mirror behind it.  verts: (y, z); pieces: index triples of triangles that
# tile the inside (where interior rays are aimed); place: how the (y, z) plane is put into the leaf frame -------------------
_STAR = [(1.1 * np.cos(np.pi / 2 + 0.8 * np.pi * k), 1.1 * np.sin(np.pi / 2 + 0.8 * np.pi * k)) for k in range(5)]  # drawing order
_STAR_IN = 1.1 * np.sin(np.pi / 10) / np.sin(0.7 * np.pi)  # radius of the doubly covered pentagon: a hole by the even-odd rule
_ARROW = [(0.0, 1.0), (-0.9, -0.8), (0.0, -0.2), (0.9, -0.8)]  # reflex vertex: index 2
_ELL = [(-0.75, -1.0), (0.75, -1.0), (0.75, -0.25), (-0.25, -0.25), (-0.25, 1.0), (-0.75, 1.0)]  # reflex vertex: index 3; dyadic levels
_FAN2 = [(2, 3, 0), (2, 0, 1)]
POLYGONS = {
    "poly_concave": dict(verts=_ARROW, pieces=_FAN2),
    "poly_clockwise": dict(verts=[(0.0, 1.0), (0.95, 0.3), (0.6, -0.8), (-0.6, -0.8), (-0.95, 0.3)], pieces=[(0, 1, 2), (0, 2, 3), (0, 3, 4)]),
    "poly_star": dict(verts=_STAR, pieces="tips"),
    "poly_level_vertices": dict(verts=_ELL, pieces=[(3, 4, 5), (3, 5, 0), (3, 0, 1), (3, 1, 2)], levels=True),
    "poly3d_near_x": dict(verts=_ARROW, pieces=_FAN2, place=("z", 0.12), normal=True),   # n.x = 0.9928 > 0.99: the basis built on y
    "poly3d_tilted": dict(verts=_ARROW, pieces=_FAN2, place=("z", 0.6), normal=True),    # n.x = 0.825: the basis built on x
    "poly3d_derived_normal": dict(verts=_ELL, pieces=[(3, 4, 5), (3, 5, 0), (3, 0, 1), (3, 1, 2)], place=("y", 0.4), normal=False),
    "poly3d_axis_plane": dict(verts=_ARROW, pieces=_FAN2, place=("xz", 0.0), normal=True),  # the plane y = 0: a local box of zero thickness
}
EDGE_BAND = 0.15  # polygon fans: half of the targets lie within this distance of an edge, on both sides of it

LENSES = [f"asph_{k}{t}" for k in ASPHERES for t in ("", "_turned")] + list(EXACT)
FAMILY = {**{n: "g31_aspheres_turned" if n.endswith("_turned") else "g30_aspheres" for n in LENSES},
          **{n: "g31_aspheres_turned" for n in BOWLS},  # (the turned lenses and the bowls: one file of all aspheres would be the largest fixture)
          **{n: "g32_cylinders" for n in CYLINDERS}, **{n: "g33_apertures" for n in APERTURES},
          **{n: "g34_spheres" for n in SPHERES}, **{n: "g35_polygons" for n in POLYGONS}}  # (appended: fan() seeds by position)
NAMES = list(FAMILY)
FAMILIES = sorted(set(FAMILY.values()))
PLANAR = tuple(APERTURES) + tuple(POLYGONS)  # the forms whose splitting variant is a slab in front
CAP = {"g30_aspheres": 12, "g31_aspheres_turned": 12, "g32_cylinders": 10, "g33_apertures": 10,     # max_trace_num of the fixtures
       "g34_spheres": 12, "g35_polygons": 10}
N_RAYS = {"g30_aspheres": 24, "g31_aspheres_turned": 24, "g32_cylinders": 40, "g33_apertures": 40,  # Ray objects per fixture scene
          "g34_spheres": 24, "g35_polygons": 40}
# the leaf kinds under test, per family (a catch mirror is a Circle in every family)
LEAF_KINDS = {"g34_spheres": ("Sphere",), "g35_polygons": ("Polygon",)}


def _sag_parametric(ns, R, kappa, a4=0.0, a6=0.0, a8=0.0):
    """The conic + even polynomial sag: this package's own (it carries its device form); for a namespace without one a
    closure over (R, kappa, a4, a6, a8), which is how the reference writes it and what optable_amd.adapter recognises."""
    if hasattr(ns, "sag_parametric"):
        return ns.sag_parametric(R, kappa, a4, a6, a8)

    def F(r):
        return r**2 / (R * (1 + np.sqrt(1 - (1 + kappa) * (r**2) / (R**2)))) + a4 * r**4 + a6 * r**6 + a8 * r**8

    return F


def cap_half_width(R, h):
    """Half-width in y and z of the local box of a cap (surfaces.py:292, 328-336)."""
    return float(np.sqrt(max(R * R - (R - h) ** 2, 0.0)))


def polygon_vertices(name):
    """The vertices a polygon form is built from: (N, 2) in the component plane, or (N, 3) placed in the leaf frame."""
    p = POLYGONS[name]
    v = np.asarray(p["verts"], dtype=float)
    if "place" not in p:
        return v
    return _place(p["place"], v)


def _place(place, yz):
    """(y, z) points of the polygon's plane as leaf-frame points: turned about z or y by an angle, or laid into y = 0."""
    axis, ang = place
    yz = np.asarray(yz, dtype=float)
    y, z, c, s = yz[:, 0], yz[:, 1], np.cos(ang), np.sin(ang)
    if axis == "z":
        return np.stack([-s * y, c * y, z], 1)
    if axis == "y":
        return np.stack([s * z, y, c * z], 1)
    return np.stack([-y, np.zeros_like(y), z], 1)  # "xz": normal (0, 1, 0) exactly


def polygon_normal(name):
    """The normal given to the constructor (None: 2-D vertices, or left to the constructor to derive)."""
    p = POLYGONS[name]
    if not p.get("normal"):
        return None
    axis, ang = p["place"]
    return {"z": (np.cos(ang), np.sin(ang), 0.0), "y": (np.cos(ang), 0.0, -np.sin(ang)), "xz": (0.0, 1.0, 0.0)}[axis]


def _sphere_components(ns, name, split):
    s = SPHERES[name]
    if split:
        coat = dict(n2=1.5, reflectivity=0.3, transmission=0.7)
    else:
        coat = dict(n2=1.0, reflectivity=1, transmission=0) if s.get("mirror") else dict(n2=1.5)
    cap = ns.SphereRefractive([0, 0, 0], radius=s["R"], height=s["h"], n1=1.0, **coat)
    if s["fan"] in ("mouth", "inside", "chords"):  # nothing else in the scene: every hit after the first is on the same leaf
        return [cap]
    if s["fan"] == "far":
        return [cap, ns.Mirror([s["R"] - 4.0, 0, 0], radius=6.0).RotZ(0.02)]
    if s.get("group"):  # the lab box of the leaf, and of its group, are those of the local box: the belly sticks out of both
        group = ns.ComponentGroup([0, 0, 0])
        group.add_component(cap.RotZ(np.pi))
        group.add_component(ns.Mirror([-7, 0, 0], radius=3.0))
        return [group.RotZ(0.1)]
    if s.get("turned"):
        cap = cap.RotZ(np.pi)
    behind, front = ns.Mirror([-7, 0, 0], radius=3.0).RotZ(0.02), ns.Mirror([9, 0, 0], radius=3.0).RotZ(np.pi + 0.02)
    return [cap] + {"both": [behind, front], "behind": [behind], None: []}[s["catch"]]


def _polygon_components(ns, name, split):
    p = POLYGONS[name]
    stop = ns.BaseMirror([5, 0, 0])
    normal = polygon_normal(name)
    stop.surface = ns.Polygon(polygon_vertices(name)) if normal is None else ns.Polygon(polygon_vertices(name), normal=normal)
    along_y = p.get("place", ("", 0))[0] == "xz"
    back = ns.Mirror([5, 3, 0], radius=3.0).RotZ(-np.pi / 2 + 0.03) if along_y else ns.Mirror([8, 0, 0], radius=3.0).RotZ(np.pi + 0.03)
    comps = [stop, back]
    if split:
        slab = ns.GlassSlab([5, -3, 0] if along_y else [2, 0, 0], width=4, height=4, thickness=0.4, n1=1, n2=1.5, reflectivity=0.2, transmission=0.8)
        comps.insert(0, slab.RotZ(np.pi / 2) if along_y else slab)
    return comps


def components(ns, name, split=False):
    if name in SPHERES:
        return _sphere_components(ns, name, split)
    if name in POLYGONS:
        return _polygon_components(ns, name, split)
    face = dict(reflectivity=0.3, transmission=0.7) if split else {}
    if name in LENSES:
        if name in EXACT:
            lens = ns.ASphericExactSphericalLens([4, 0.1, 0], CT=0.6, diameter=2.4, **EXACT[name], **face)
        else:
            key = name[len("asph_"):]
            turned = key.endswith("_turned")
            lens = ns.ASphericParametricLens([4, 0.1, 0], CT=0.6, diameter=2.4, n=1.5, **ASPHERES[key[:-len("_turned")] if turned else key], **face)
            if turned:
                lens = lens.RotZ(np.pi)
        return [lens, ns.Mirror([9, 0, 0], radius=3.0).RotZ(np.pi + 0.02)]
    if name in BOWLS:
        b = BOWLS[name]
        refl = dict(reflectivity=0.3, transmission=0.7) if split else dict(reflectivity=1, transmission=0)
        return [ns.BaseRefraciveSurface(origin=[0, 0, 0], n1=1.0, n2=1.0, surface=ns.ASphere(b["radius"], _sag_parametric(ns, b["R"], b["kappa"])), **refl)]
    if name in CYLINDERS:
        c = CYLINDERS[name]
        kw = {} if c["arc"] is None else dict(theta_range=c["arc"])
        cyl = ns.CylMirror([5, 0, 0], radius=1.5, height=2.0, **kw, **face)
        return [cyl.RotZ(c["rot"]) if c["rot"] else cyl]
    build, _ = APERTURES[name]
    stop = ns.BaseMirror([5, 0, 0])
    stop.surface = build(ns)
    comps = [stop, ns.Mirror([8, 0, 0], radius=3.0).RotZ(np.pi + 0.03)]
    if split:
        comps.insert(0, ns.GlassSlab([2, 0, 0], width=4, height=4, thickness=0.4, n1=1, n2=1.5, reflectivity=0.2, transmission=0.8))
    return comps


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _disc(rng, n, radius):
    r, phi = radius * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(-np.pi, np.pi, n)
    return r * np.cos(phi), r * np.sin(phi)


def _sphere_fan(rng, name, n):
    s = SPHERES[name]
    R, kind = s["R"], s["fan"]
    if kind in ("disc", "mouth"):  # along the axis and a little off it: onto the crown / into the mouth
        side = -1.0 if kind == "mouth" else 1.0
        y, z = _disc(rng, n, s["spread"] * (cap_half_width(R, s["h"]) or R))
        o = np.stack([np.full(n, 6.0 * side), y, z], 1)
        d = np.stack([np.full(n, -side), rng.uniform(-0.04, 0.04, n), rng.uniform(-0.04, 0.04, n)], 1)
    elif kind == "inside":  # from a ball of radius 0.9 about the centre, up to 55 degrees off the axis towards the crown (every
        # direction alike would send six rays in ten at the belly outside the local box or out of the mouth)
        o = _unit(rng.normal(size=(n, 3))) * (0.9 * np.cbrt(rng.uniform(0, 1, n)))[:, None]
        d = np.stack([np.ones(n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)], 1)
    elif kind == "chords":  # exactly along y, at R - delta from the cap's y axis: delta on both sides of chord_threshold(R, 2 R)
        miss = np.arange(n) % 3 == 0
        delta = np.where(miss, rng.uniform(*CHORD_DELTAS[0], n), rng.uniform(*CHORD_DELTAS[1], n))
        phi = rng.uniform(-0.3, 0.3, n)
        o = np.stack([(R - delta) * np.cos(phi), rng.uniform(-6.0, -4.0, n), (R - delta) * np.sin(phi)], 1)
        d = np.tile([0.0, 1.0, 0.0], (n, 1))
    else:  # "far": towards the crown from 85 - 115 away, one ray in three from beyond the cut
        beyond = np.arange(n) % 3 == 0
        dist = np.where(beyond, rng.uniform(*FAR_DISTANCES[0], n), rng.uniform(*FAR_DISTANCES[1], n))
        y, z = _disc(rng, n, 2.0)
        o = np.stack([R + dist, y, z], 1)
        d = np.stack([-np.ones(n), rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n)], 1)
    return o, _unit(d)


def polygon_pieces(name):
    """Triangles (3, 2) that tile the inside of a polygon form (the five tips of the pentagram: its centre is a hole)."""
    p = POLYGONS[name]
    v = np.asarray(p["verts"], dtype=float)
    if p["pieces"] != "tips":
        return [v[list(t)] for t in p["pieces"]]
    ang = lambda k: np.pi / 2 + 0.4 * np.pi * k
    inner = lambda k: _STAR_IN * np.array([np.cos(ang(k) + 0.2 * np.pi), np.sin(ang(k) + 0.2 * np.pi)])
    return [np.array([1.1 * np.array([np.cos(ang(k)), np.sin(ang(k))]), inner(k - 1), inner(k)]) for k in range(5)]


def _polygon_fan(rng, name, n):
    """Tight to the polygon: every ray is aimed at a target in the polygon's plane, half of them inside a triangle of its
    tiling, half within EDGE_BAND of a random point of a random edge, on either side of it."""
    p = POLYGONS[name]
    v = np.asarray(p["verts"], dtype=float)
    pieces = polygon_pieces(name)
    tri = np.stack(pieces)[rng.integers(0, len(pieces), n)]
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    inner = np.einsum("nk,nkc->nc", w, tri)
    e = rng.integers(0, len(v), n)
    a, b = v[e], v[(e + 1) % len(v)]
    along = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
    band = a + rng.uniform(0, 1, n)[:, None] * (b - a) + rng.uniform(-EDGE_BAND, EDGE_BAND, n)[:, None] * np.stack([-along[:, 1], along[:, 0]], 1)
    target = np.where((np.arange(n) % 2 == 0)[:, None], inner, band)
    tilt = np.stack([rng.uniform(-0.03, 0.03, n), rng.uniform(-0.02, 0.02, n)], 1)
    if p.get("levels"):  # one ray in eight exactly at the level of a vertex (dyadic), straight on: py == y1 in poly_inside
        lv = np.arange(n) % 8 == 5
        target[lv, 0] = rng.choice(np.unique(v[:, 0]), int(lv.sum()))
        tilt[lv] = 0.0
    if "place" not in p:
        T = np.stack([np.full(n, 5.0), target[:, 0], target[:, 1]], 1)
    else:
        T = np.array([5.0, 0.0, 0.0]) + _place(p["place"], target)
    if p.get("place", ("", 0))[0] == "xz":  # rays along +y from y = -5
        d = _unit(np.stack([tilt[:, 0], np.ones(n), tilt[:, 1]], 1))
        return T - d * ((T[:, 1] + 5.0) / d[:, 1])[:, None], d
    d = _unit(np.stack([np.ones(n), tilt[:, 0], tilt[:, 1]], 1))
    return T - d * (T[:, 0] / d[:, 0])[:, None], d


def fan(name, n, seed=0):
    """(origins, unit directions) of the form's ray fan: rays that meet the form, well inside its aperture for the most part."""
    rng = np.random.default_rng([seed, NAMES.index(name)])
    if name in SPHERES:
        return _sphere_fan(rng, name, n)
    if name in POLYGONS:
        return _polygon_fan(rng, name, n)
    if name in LENSES:  # a disc inside the lens aperture (radius 1.2 about y = 0.1), a small angular spread
        y, z = _disc(rng, n, 1.0)
        o = np.stack([np.zeros(n), 0.1 + y, z], 1)
        d = np.stack([np.ones(n), rng.uniform(-0.03, 0.03, n), rng.uniform(-0.02, 0.02, n)], 1)
    elif name in BOWLS:  # into the bowl, along its axis and a little off it
        b = BOWLS[name]
        y, z = _disc(rng, n, 0.93 * b["radius"])
        o = np.stack([np.full(n, 6.0 * b["side"]), y, z], 1)
        d = np.stack([np.full(n, -1.0 * b["side"]), rng.uniform(-0.04, 0.04, n), rng.uniform(-0.04, 0.04, n)], 1)
    elif name in CYLINDERS:  # three in four from inside the wall towards the arc, one in four from outside onto its convex side
        c = CYLINDERS[name]
        lo, hi = (-np.pi, np.pi) if c["arc"] is None else c["arc"]
        mid, half = 0.5 * (lo + hi) + c["rot"], 0.5 * (hi - lo)
        phi = mid + rng.uniform(-0.8, 0.8, n) * half
        inside = np.arange(n) % 4 != 3
        u = np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], 1)
        jitter = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.7, 0.7, n)], 1)
        o = np.where(inside[:, None], [5.0, 0.0, 0.0] + jitter, [5.0, 0.0, 0.0] + 3.5 * u + 0.25 * jitter)
        tilt = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.08, 0.08, n)], 1)
        d = np.where(inside[:, None], u, -u) + tilt
    else:  # a box around the aperture
        hy, hz = APERTURES[name][1]
        o = np.stack([np.zeros(n), rng.uniform(-hy, hy, n), rng.uniform(-hz, hz, n)], 1)
        d = np.stack([np.ones(n), rng.uniform(-0.03, 0.03, n), rng.uniform(-0.02, 0.02, n)], 1)
    return o, _unit(d)


def scene(ns, name):
    """The fixture scene: the form with a few Ray objects of its fan (Gaussian q, explicit ids), capped."""
    fam = FAMILY[name]
    o, d = fan(name, N_RAYS[fam], seed=1)
    rays = [ns.Ray(o[i], d[i], wavelength=WL, w0=W0, id=i) for i in range(len(o))]
    return dict(components=components(ns, name), monitors=[], rays=rays, limit={"max_trace_num": CAP[fam]})


def form_leaves(compiled, name=None):
    """Leaf indices of the surfaces under test in a compiled catalogue scene: the aspheres, cylinder walls, boolean apertures;
    for a form `name` of a later family the leaf kinds of that family (LEAF_KINDS)."""
    kinds = LEAF_KINDS.get(FAMILY.get(name), ("ASphere", "Cylinder", "BooleanPlane"))
    return [k for k, leaf in enumerate(compiled.leaves) if type(leaf.surface).__name__ in kinds]


def sub_fixture(gold, name):
    """The arrays of one form out of a family fixture (keys `<form>/<key>`), as a fixture of the single-scene format."""
    return {k[len(name) + 1:]: v for k, v in gold.items() if k.startswith(name + "/")}


def curved_scene(oa, rng):
    """test_gpu_pool._curved_scene (random scenes of the curved-surface preset) with its asphere lens drawn from the in-domain
    catalogue forms (their own R and kappa) instead of the single kappa = -1."""
    comps = []
    for _ in range(int(rng.integers(4, 10))):
        pos = [rng.uniform(2, 26), rng.uniform(-4, 4), rng.uniform(-0.5, 0.5)]
        ang = rng.uniform(-np.pi, np.pi)
        kind = int(rng.integers(0, 7))
        if kind == 0:
            c = oa.Mirror(pos, radius=rng.uniform(0.5, 1.5)).RotZ(ang)
        elif kind == 1:
            c = oa.GlassSlab(pos, width=2, height=2, thickness=rng.uniform(0.2, 0.8), n1=1, n2=rng.uniform(1.3, 1.8)).RotZ(0.4 * ang)
        elif kind == 2:
            c = oa.BiConvexLens(pos, CT=0.5, R1=rng.uniform(6, 15), R2=-rng.uniform(6, 15), diameter=2.4, n=1.52).RotZ(0.2 * ang)
        elif kind == 3:
            c = oa.SquareMirror(pos, width=1.6, height=1.2).RotZ(ang).RotY(rng.uniform(-0.2, 0.2))
        elif kind == 4:
            c = oa.SphereRefractive(pos, radius=rng.uniform(4.0, 9.0), height=1.0, n1=1.0, n2=1.5).RotZ(0.2 * ang)
        elif kind == 5:
            form = IN_DOMAIN[int(rng.integers(0, len(IN_DOMAIN)))]
            c = oa.ASphericParametricLens(pos, CT=0.6, diameter=2.4, n=1.5, **ASPHERES[form]).RotZ(0.15 * ang)
        else:
            c = oa.MMA(origin=pos, N=(5, 6), pitch=0.4, roc=rng.uniform(15, 40), n=1.5, thickness=0.1, reflectivity=1,
                       transmission=0).RotZ(np.pi + 0.3 * ang)
        comps.append(c)
    comps.append(oa.BiConvexLens([28, 0, 0], CT=0.5, R1=9.0, R2=-9.0, diameter=9.0, n=1.5))  # (every scene has a curved surface)
    return comps


DEEP_COAT = dict(n1=1.0, n2=1.5)
# Seeds of the random scenes below.  A ball of glass of radius ~1 that rays meet at every angle sends a few rays in ten thousand
# through a refraction near the critical angle, whose further path and q no trace defines to 1e-9 (the reference's own roots
# carry brentq's 2e-12).  These are the first three seeds whose scene amplifies a displaced ray start at most 400-fold on
# every one of its rays, measured with the oracle alone (tests/test_surface_forms_cpu.py asserts it).
DEEP_SEEDS = (2, 3, 7)
DEEP_CAPS = ((1.0, 1.0), (1.2, 1.2), (1.0, 1.6), (1.1, 1.9), (0.9, 1.7))  # (R, h): hemispheres and caps deeper than one


def curved_scene_deep_caps(oa, rng):
    """curved_scene with its SphereRefractive parts drawn from DEEP_CAPS, as built or turned round (the mouth towards the rays),
    and one of them in every scene, in the middle of the fan."""
    comps = []
    for _ in range(int(rng.integers(4, 10))):
        pos = [rng.uniform(2, 26), rng.uniform(-4, 4), rng.uniform(-0.5, 0.5)]
        ang = rng.uniform(-np.pi, np.pi)
        kind = int(rng.integers(0, 7))
        if kind == 0:
            c = oa.Mirror(pos, radius=rng.uniform(0.5, 1.5)).RotZ(ang)
        elif kind == 1:
            c = oa.GlassSlab(pos, width=2, height=2, thickness=rng.uniform(0.2, 0.8), n1=1, n2=rng.uniform(1.3, 1.8)).RotZ(0.4 * ang)
        elif kind == 2:
            c = oa.BiConvexLens(pos, CT=0.5, R1=rng.uniform(6, 15), R2=-rng.uniform(6, 15), diameter=2.4, n=1.52).RotZ(0.2 * ang)
        elif kind == 3:
            c = oa.SquareMirror(pos, width=1.6, height=1.2).RotZ(ang).RotY(rng.uniform(-0.2, 0.2))
        elif kind in (4, 5):
            R, h = DEEP_CAPS[int(rng.integers(0, len(DEEP_CAPS)))]
            c = oa.SphereRefractive(pos, radius=R, height=h, **DEEP_COAT).RotZ(ang)
        else:
            form = IN_DOMAIN[int(rng.integers(0, len(IN_DOMAIN)))]
            c = oa.ASphericParametricLens(pos, CT=0.6, diameter=2.4, n=1.5, **ASPHERES[form]).RotZ(0.15 * ang)
        comps.append(c)
    for x, y, turn in ((5.0, -2.0, np.pi), (5.5, 2.0, 0.3)):  # (every scene has deep caps where the rays are)
        R, h = DEEP_CAPS[int(rng.integers(0, len(DEEP_CAPS)))]
        comps.append(oa.SphereRefractive([x, y, 0.0], radius=R, height=h, **DEEP_COAT).RotZ(turn))
    comps.append(oa.BiConvexLens([28, 0, 0], CT=0.5, R1=9.0, R2=-9.0, diameter=9.0, n=1.5))  # (every scene has a curved surface)
    return comps


def curved_deep_case(oa, seed, n):
    """(components, origins, directions) of random deep-cap scene `seed` and its ray fan (the fan of the other random curved scenes)."""
    rng = np.random.default_rng(7400 + seed)
    comps = curved_scene_deep_caps(oa, rng)
    o = np.stack([np.zeros(n), rng.uniform(-4, 4, n), rng.uniform(-0.4, 0.4, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.15, 0.15, n), rng.uniform(-0.03, 0.03, n)], 1)
    return comps, o, d
