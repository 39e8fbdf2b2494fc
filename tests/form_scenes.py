"""The surface-form catalogue: one small scene per FORM of a shape the trace kernels branch on — every conic and polynomial
variant of the parametric asphere (both orientations, the exact plano-convex sag, reflective bowls that a ray meets more
than once), the arcs of the built-in cylinder wall, and boolean apertures with a union, a polygon operand and nested
programs.  Written against a namespace `ns` like tests/scenes.py, so the same builder runs on the reference
(tools/make_golden.py records `scene(ns, name)` into tests/golden/g30-g33) and on this package.  NOT part of
scenes.SCENES: the existing parametrised tests and g28_adapter.npz stay as they are.

    NAMES, FAMILY[name]          every form and the fixture file it is recorded in
    components(ns, name, split)  the scene; split=True: the form's interface splits every ray (reflectivity 0.3), planar
                                 forms get a GlassSlab(reflectivity=0.2) in front instead
    fan(name, n, seed)           the batch ray fan of the form: (origins, directions)
    scene(ns, name)              the object-API scene of the fixtures (<= 40 Ray objects of the same fan, cap <= 12)
    form_leaves(scene)           indices of the leaves that carry the form under test
"""
import numpy as np

from optable_amd.workloads import WL, W0

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

LENSES = [f"asph_{k}{t}" for k in ASPHERES for t in ("", "_turned")] + list(EXACT)
FAMILY = {**{n: "g31_aspheres_turned" if n.endswith("_turned") else "g30_aspheres" for n in LENSES},
          **{n: "g31_aspheres_turned" for n in BOWLS},  # (the turned lenses and the bowls: one file of all aspheres would be the largest fixture)
          **{n: "g32_cylinders" for n in CYLINDERS}, **{n: "g33_apertures" for n in APERTURES}}
NAMES = list(FAMILY)
FAMILIES = sorted(set(FAMILY.values()))
PLANAR = tuple(APERTURES)
CAP = {"g30_aspheres": 12, "g31_aspheres_turned": 12, "g32_cylinders": 10, "g33_apertures": 10}     # max_trace_num of the fixtures
N_RAYS = {"g30_aspheres": 24, "g31_aspheres_turned": 24, "g32_cylinders": 40, "g33_apertures": 40}  # Ray objects per fixture scene


def _sag_parametric(ns, R, kappa, a4=0.0, a6=0.0, a8=0.0):
    """The conic + even polynomial sag: this package's own (it carries its device form); for a namespace without one a
    closure over (R, kappa, a4, a6, a8), which is how the reference writes it and what optable_amd.adapter recognises."""
    if hasattr(ns, "sag_parametric"):
        return ns.sag_parametric(R, kappa, a4, a6, a8)

    def F(r):
        return r**2 / (R * (1 + np.sqrt(1 - (1 + kappa) * (r**2) / (R**2)))) + a4 * r**4 + a6 * r**6 + a8 * r**8

    return F


def components(ns, name, split=False):
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


def fan(name, n, seed=0):
    """(origins, unit directions) of the form's ray fan: rays that meet the form, well inside its aperture for the most part."""
    rng = np.random.default_rng([seed, NAMES.index(name)])
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


def form_leaves(compiled):
    """Leaf indices of the surfaces under test in a compiled catalogue scene: the aspheres, cylinder walls, boolean apertures."""
    kinds = ("ASphere", "Cylinder", "BooleanPlane")
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
