"""Audit of a single-precision trace against the double-precision trace of the same rays.

Single precision cannot promise the fp64 surface sequence for every ray over 20-50 bounces: a ray that grazes an
aperture edge flips between hit and miss at 6e-8 relative, and every bounce amplifies the difference.  What it can
promise is that rays leave the fp64 path only THERE: `audit` finds, for every ray whose sequences differ, the first
segment that ends on different leaves and measures how far the two hit points lie from the aperture edge of their
leaves, in the leaf frame (circle / sphere cap / asphere: |r - radius|; rectangle: distance to the nearest side).

`audit_traces` is the general form, for any two traces of the same rays (fp64 against fp64, fp32 against fp64, ray trees
included): it reads them in the reference's order, checks everything before the first difference, and names a cause
for the difference with a margin measured in the fp64 trace (see its docstring).  `assert_explained` fails with a
table of every ray it cannot explain.
"""
import json
import os

import numpy as np


def _edge_margin(comp, P):
    """Distance of lab point P (on or near the leaf's surface) to the leaf's aperture edge; inf when the shape has
    no simple edge description (polygons, booleans: not audited)."""
    surf = comp.surface
    M = np.asarray(comp.transform_matrix, dtype=float)
    loc = M.T @ (np.asarray(P, dtype=float) - np.asarray(comp.origin, dtype=float))
    kind = type(surf).__name__
    if kind == "Circle":
        return abs(np.linalg.norm(loc) - surf.radius)
    if kind == "Rectangle":
        return min(abs(surf.width / 2 - abs(loc[1])), abs(surf.height / 2 - abs(loc[2])))
    if kind == "Sphere":  # cap of height h: aperture radius sqrt(R^2 - (R-h)^2) around the x axis
        a = np.sqrt(max(surf.radius**2 - (surf.radius - surf.height) ** 2, 0.0))
        return abs(np.hypot(loc[1], loc[2]) - a)
    if kind == "ASphere":
        return abs(np.hypot(loc[1], loc[2]) - surf.radius)
    if kind in ("Polygon", "Cylinder"):
        return _boundary_distance(surf, loc)
    return np.inf


def audit(scene, s64, s32, K):
    """s64 / s32: SegmentBatch of the same rays (any layout of the non-branching trace).  Returns arrays over the diverged rays:
    ray, kstar (first differing segment), leaf64 / leaf32 (leaf ids, -1 = escaped), margin (smallest edge margin of
    the hit points involved), pos_err (|origin64 - origin32| of segment kstar: how far apart the two traces were
    when they disagreed), plus `same` (bool per ray)."""
    s64, s32 = s64.as_kray_slots(K), s32.as_kray_slots(K)  # (whatever layout the traces were written in)
    n = s64.n_rays
    c64, c32 = np.abs(s64.count.cpu().numpy()), np.abs(s32.count.cpu().numpy())
    def f(s, name):
        with np.errstate(invalid="ignore"):  # unused slots are uninitialised memory; they are masked by the counts
            return s.field(name).cpu().numpy().reshape(K, n).astype(np.float64)

    surf64 = s64.surface.cpu().numpy().reshape(K, n)
    surf32 = s32.surface.cpu().numpy().reshape(K, n)
    O64 = np.stack([f(s64, "ox"), f(s64, "oy"), f(s64, "oz")], axis=-1)
    O32 = np.stack([f(s32, "ox"), f(s32, "oy"), f(s32, "oz")], axis=-1)
    valid = np.arange(K)[:, None] < np.minimum(c64, c32)[None, :]
    differ = (surf64 != surf32) & valid
    same = (c64 == c32) & ~differ.any(axis=0)
    rays = np.nonzero(~same)[0]
    L64, L32 = f(s64, "length"), f(s32, "length")
    out = {k: [] for k in ("ray", "kstar", "leaf64", "leaf32", "margin", "pos_err", "start_margin", "len64", "len32")}
    for i in rays:
        ks = int(np.argmax(differ[:, i])) if differ[:, i].any() else int(min(c64[i], c32[i])) - 1
        a, b = int(surf64[ks, i]), int(surf32[ks, i])
        margins = []
        # a trace names the point where it hit by the origin of its NEXT segment
        if a >= 0 and ks + 1 < c64[i]:
            margins.append(_edge_margin(scene.leaves[a], O64[ks + 1, i]))
            if b >= 0:  # ... and where was that point relative to the leaf the other precision chose?
                margins.append(_edge_margin(scene.leaves[b], O64[ks + 1, i]))
        if b >= 0 and ks + 1 < c32[i]:
            margins.append(_edge_margin(scene.leaves[b], O32[ks + 1, i]))
            if a >= 0:
                margins.append(_edge_margin(scene.leaves[a], O32[ks + 1, i]))
        out["ray"].append(i)
        out["kstar"].append(ks)
        out["leaf64"].append(a)
        out["leaf32"].append(b)
        out["margin"].append(min(margins) if margins else np.inf)
        out["pos_err"].append(float(np.linalg.norm(O64[ks, i] - O32[ks, i])))
        # where the deciding segment STARTS: a start near an edge of the leaf it leaves (a prism corner, the rim of a
        # lens) is where the next face lies within the self-hit guard (1e-9 in fp64, 1e-5 in fp32: DESIGN.md §5)
        prev = int(surf64[ks - 1, i]) if ks > 0 else -1
        out["start_margin"].append(_edge_margin(scene.leaves[prev], O64[ks, i]) if prev >= 0 else np.inf)
        out["len64"].append(float(L64[ks, i]))
        out["len32"].append(float(L32[ks, i]))
    rep = {k: np.array(v) for k, v in out.items()}
    rep["same"] = same
    return rep


# ---------------------------------------------------------------------------------------------------------------------
# General divergence audit
#
# A ray is EXPLAINED when the decision at which its two traces part is marginal in the fp64 trace: its margin (a
# distance for `edge`, `tie`, `guard`, `escape` and the root-search causes `box`, `scan`, `cut`, `graze` of a spherical
# cap; |1 - sin^2 theta_t| for `tir`) is at most C * delta + FLOOR[prec],
# where delta = |dO| + L |dD| is how far apart the two traces already were where they parted.
#
# C: a start moved by dO and a direction turned by dD move the hit point by |dO| + L |dD| along the surface, times
#    1 / cos(incidence) at most; 10 covers incidence up to 84 degrees.  (Beyond that a hit is a graze, which the edge
#    and tie margins see anyway.)
# FLOOR["f64"] = 1e-10: what two correct fp64 traces may disagree on at the decision itself, at scene scale ~30.  The
#    oracle polishes non-planar roots with Brent (xtol 2e-12 in t), the device with Newton to 4.4e-16 relative; the
#    hit point then carries ~30 x 2.2e-16 x a few operations of rounding (~1e-14).  1e-10 is the Brent tolerance
#    times 50, and leaves the ulp-level terms 4 orders of magnitude of room.
# FLOOR["f32"] = 1e-4: fp32 rounds a coordinate of ~30 to 2e-6 and a 20-50 bounce path piles that up to ~1e-4; the
#    fp32 self-hit guard is 1e-5 (trace_core.h).  It is the EDGE / SHORT bound tests/test_gpu_fp32_*.py used before.
C_DELTA = 10.0
FLOOR = {"f64": 1e-10, "f32": 1e-4}
GUARD = {"f64": 1e-9, "f32": 1e-5}  # self-hit guard: trace_core.h Num<T>::eps_t (the oracle: EPS_T)
GUARD_FACTOR = 10.0  # `guard` explains a deciding segment shorter than this many guards ...
CAUSES = ("edge", "tie", "tir", "guard", "escape", "box", "scan", "cut", "graze")
_MIRROR, _REFRACT = 0, 1  # OT_INT_* (include/optable_hip.h)
_MAT_CONST, _MAT_SELLMEIER, _MAT_CHEB = 0, 1, 2


def _rect_boundary(u, v, hu, hv):
    """Distance of (u, v) to the boundary of the rectangle |u| <= hu, |v| <= hv (hu = inf: no boundary along u)."""
    du, dv = abs(u) - hu, abs(v) - hv
    if du <= 0 and dv <= 0:
        return min(-du, -dv)
    return float(np.hypot(max(du, 0.0), max(dv, 0.0)))


def _segment_distance(p, a, b):
    ab = b - a
    t = np.clip(np.dot(p - a, ab) / max(np.dot(ab, ab), 1e-300), 0.0, 1.0)
    return float(np.linalg.norm(p - (a + t * ab)))


def _boundary_distance(surf, loc):
    """Distance, in the leaf frame, of the local point `loc` to the edge of the aperture of `surf`, measured along the
    surface (closed forms; a ring probe of `within_boundary` for any other aperture)."""
    kind = type(surf).__name__
    y, z = loc[1], loc[2]
    if kind == "Circle":
        return abs(np.linalg.norm(loc) - surf.radius)  # the reference's 3-norm test (surfaces.py:144-145)
    if kind == "Rectangle":
        return _rect_boundary(y, z, surf.width / 2, surf.height / 2)
    if kind == "Sphere":  # the rim circle x = R - h, r = a
        a = np.sqrt(max(surf.radius**2 - (surf.radius - surf.height) ** 2, 0.0))
        return float(np.hypot(loc[0] - (surf.radius - surf.height), np.hypot(y, z) - a))
    if kind == "ASphere":
        return abs(np.hypot(y, z) - surf.radius)
    if kind == "Polygon":  # nearest edge segment; the reference counts |cross| <= 1e-9 as on the edge (surfaces.py:534-558),
        p = surf._project_to_2d(np.asarray(loc, dtype=float)[None, :])[0]  # which moves the decision outwards by 1e-9 / |edge|
        v = surf._verts2d
        e = [(_segment_distance(p, v[i], v[(i + 1) % len(v)]), surf._tol / np.linalg.norm(v[(i + 1) % len(v)] - v[i])) for i in range(len(v))]
        d, shift = min(e)
        inside = False
        for i in range(len(v)):  # even-odd test without the tolerance
            (x1, y1), (x2, y2) = v[i], v[(i + 1) % len(v)]
            if (y1 > p[1]) != (y2 > p[1]) and x1 + (p[1] - y1) * (x2 - x1) / (y2 - y1) >= p[0]:
                inside = not inside
        return abs((-d if inside else d) - shift)
    if kind == "Cylinder":  # (arc length, z) rectangle: theta-range ends as arc length, the +-height/2 rims
        rho = np.hypot(loc[0], loc[1])
        t0, t1 = surf.theta_range
        hz = surf.height / 2
        if t1 - t0 >= 2 * np.pi - 1e-12:
            return abs(abs(z) - hz)
        th = np.arctan2(loc[1], loc[0])
        mid, half = 0.5 * (t0 + t1), 0.5 * (t1 - t0)
        return _rect_boundary(rho * (th - mid), z, rho * half, hz)
    return _probe_boundary(surf, loc)


PROBE_RADII = 1e-14 * 2.0 ** np.arange(0, 50)  # 1e-14 .. 5.6: the generic probe's ladder (factor 2)


def _probe_boundary(surf, loc):
    """Any aperture (BooleanPlane, user surfaces): the smallest radius of the ladder at which `within_boundary` on a ring
    of 16 points around `loc`, in the plane tangent to the surface, disagrees with its value at `loc`."""
    loc = np.asarray(loc, dtype=float)
    nrm = np.asarray(surf.normal(loc), dtype=float)
    nrm = nrm / np.linalg.norm(nrm)
    e1 = np.cross(nrm, [0.0, 0.0, 1.0] if abs(nrm[2]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    inside = bool(surf.within_boundary(loc))
    phi = np.linspace(0, 2 * np.pi, 16, endpoint=False)
    ring = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    for r in PROBE_RADII:
        for p in loc + r * ring:
            if bool(surf.within_boundary(p)) != inside:
                return float(r)
    return np.inf


class _Leaves:
    """Leaf frames, surfaces and materials of a CompiledScene, as the tracers read them (node table)."""

    def __init__(self, scene, wavelength=None):
        self.scene = scene
        nodes = scene.node_table()
        self.node = {}
        for k in range(scene.n_nodes):
            if int(nodes["kind"][k]) == 1:  # OT_NODE_LEAF
                self.node[int(nodes["leaf_id"][k])] = k
        self.nodes = nodes
        self.wavelength = wavelength
        # most children a hit on the leaf can have: mirror (reflected) + (transmitted), refraction 1 (refracted or
        # totally reflected) + (reflected), thin lens 1, block 0
        self.fanout = np.zeros(max(self.node, default=-1) + 1, dtype=np.int64)
        for leaf, k in self.node.items():
            inter, r, t = int(nodes["interaction"][k]), nodes["reflectivity"][k] > 0, nodes["transmission"][k] > 0
            self.fanout[leaf] = {_MIRROR: int(r) + int(t), _REFRACT: 1 + int(r), 2: 1}.get(inter, 0)

    def local(self, leaf, P):
        nd = self.nodes[self.node[leaf]]
        M = np.asarray(nd["M"], dtype=float).reshape(3, 3)
        return M.T @ (np.asarray(P, dtype=float) - np.asarray(nd["origin"], dtype=float)), M

    def surface(self, leaf):
        return self.scene.leaves[leaf].surface

    def edge(self, leaf, P):
        """Distance of lab point P to the rim of the leaf: off the surface (|f|) and to the aperture edge, combined."""
        if leaf < 0 or not np.all(np.isfinite(P)):
            return np.inf
        loc, _ = self.local(leaf, P)
        surf = self.surface(leaf)
        return float(np.hypot(abs(float(surf.f(loc))), _boundary_distance(surf, loc)))

    def on_surface(self, leaf, P):
        """How far lab point P is from being a hit on the leaf: |f| if inside the aperture, else also its edge distance."""
        loc, _ = self.local(leaf, P)
        surf = self.surface(leaf)
        off = abs(float(surf.f(loc)))
        return off if surf.within_boundary(loc) else float(np.hypot(off, _boundary_distance(surf, loc)))

    def search_margins(self, leaf, O, D, P):
        """The decisions of the root search of a spherical cap (trace_core.h hit_leaf, optical_component.py:206-233) that are no
        aperture edge, for the lab ray (O, D) and a hit point P on it, each with its margin in scene units, measured on
        that ray (the fp64 trace's):
          box    distance of P to the nearest face of the leaf's local box: the search runs over the ray's crossing of the
                 box only, and a cap deeper than a hemisphere has its belly outside it;
          scan   the ten samples of the crossing: distance of a root to the nearest sample (a root that changes its sample
                 interval changes which intervals show a sign change; two roots in one interval show none) and
                 |chord - step|;
          cut    |t - 100| of the nearest root (|t1 - 100| when the whole crossing lies beyond): the search ends at t = 100;
          graze  |R - distance of the line to the centre|: whether there are roots at all.
        {} for any other leaf."""
        surf = self.surface(leaf) if leaf >= 0 else None
        if type(surf).__name__ != "Sphere" or not (np.all(np.isfinite(O)) and np.all(np.isfinite(D))):
            return {}
        nd = self.nodes[self.node[leaf]]
        o, M = self.local(leaf, O)
        d = M.T @ np.asarray(D, dtype=float)
        d = d / np.linalg.norm(d)
        box = np.asarray(nd["lbox"], dtype=float).reshape(3, 2)
        out = {}
        if P is not None and np.all(np.isfinite(P)):
            loc, _ = self.local(leaf, P)
            out["box"] = float(np.min(np.abs(loc[:, None] - box)))
        R = float(surf.radius)
        tca = -float(o @ d)
        c2 = float(np.sum((o + tca * d) ** 2))
        out["graze"] = abs(R - np.sqrt(c2))
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (box[:, 0] - o) / d, (box[:, 1] - o) / d
        ta, tb = np.where(np.isnan(ta), -np.inf, ta), np.where(np.isnan(tb), np.inf, tb)
        t1, t2 = float(np.max(np.minimum(ta, tb))), float(np.min(np.maximum(ta, tb)))
        eps = GUARD["f64"]
        if c2 >= R * R or t2 + eps < t1:
            return out
        half = np.sqrt(R * R - c2)
        roots = np.array([tca - half, tca + half])
        if max(t1, 0.0) > 100.0:
            out["cut"] = max(t1, 0.0) - 100.0
            return out
        a, b = max(t1, 0.0) - eps, min(t2, 100.0) + eps
        samples = a + (b - a) / 9.0 * np.arange(10)
        near = np.abs(roots[:, None] - samples[None, :])
        if t2 > 100.0:
            out["cut"] = float(np.min(near[:, -1]))
            near = near[:, :-1]
        out["scan"] = float(min(np.min(near), abs(2 * half - (b - a) / 9.0)))
        return out

    def _index(self, mat, wl_m):
        m = self.scene.materials[mat]
        if m.kind == _MAT_CONST:
            return m.n
        if m.kind == _MAT_CHEB:
            rec = np.ctypeslib.as_array(self.scene.aux)[int(m.n):]
            n, lo, hi = int(rec[0]), rec[1], rec[2]
            w = min(max(wl_m, lo), hi)
            return float(np.polynomial.chebyshev.chebval((2 * w - (lo + hi)) / (hi - lo), rec[3:3 + n]))
        um2 = (wl_m / 1e-6) ** 2
        return float(np.sqrt(1 + sum(m.B[k] * um2 / (um2 - m.C[k]) for k in range(3))))

    def tir_margin(self, leaf, P, D, ray):
        """|1 - sin^2 theta_t| of a ray arriving along D at lab point P of a refracting leaf (inf for any other leaf)."""
        nd = self.nodes[self.node[leaf]]
        if leaf < 0 or int(nd["interaction"]) != _REFRACT or not np.all(np.isfinite(P)):
            return np.inf
        loc, M = self.local(leaf, P)
        d = M.T @ np.asarray(D, dtype=float)
        d /= np.linalg.norm(d)
        nrm = np.asarray(self.surface(leaf).normal(loc), dtype=float)
        nrm = nrm / np.linalg.norm(nrm)
        mats = (int(nd["mat1"]), int(nd["mat2"]))
        if all(self.scene.materials[m].kind == _MAT_CONST for m in mats):
            wl_m = 0.0
        elif self.wavelength is None:
            return np.inf
        else:
            wl_m = float(np.broadcast_to(self.wavelength, (ray + 1,))[ray]) * self.scene.unit
        n1, n2 = (self._index(m, wl_m) for m in mats)
        dn = float(np.clip(d @ nrm, -1, 1))
        nin, nout = (n1, n2) if dn < 0 else (n2, n1)
        return abs(1.0 - (nin / nout) ** 2 * (1 - dn * dn))


def _tree_bounds(x, n):
    ray = np.asarray(x["ray"], dtype=np.int64)
    if len(ray) and np.any(np.diff(ray) < 0):
        raise ValueError("trace is not in the reference's order (input ray major)")
    return np.searchsorted(ray, np.arange(n + 1))


def _children(x, lo, hi, tol, fanout):
    """Child count of every record of one tree (FIFO order): the children of a record are the next unclaimed records
    that start where it ended, at most as many as its leaf can emit (a short child segment puts the grandchild's start
    there too)."""
    O = np.stack([x["ox"][lo:hi], x["oy"][lo:hi], x["oz"][lo:hi]], 1).astype(np.float64)
    D = np.stack([x["dx"][lo:hi], x["dy"][lo:hi], x["dz"][lo:hi]], 1).astype(np.float64)
    L = np.asarray(x["length"][lo:hi], dtype=np.float64)
    S = np.asarray(x["surface"][lo:hi])
    nk, nxt, parent = np.zeros(hi - lo, dtype=np.int64), 1, np.full(hi - lo, -1, dtype=np.int64)
    for i in range(hi - lo):
        if S[i] < 0 or not np.isfinite(L[i]):
            continue
        P = O[i] + L[i] * D[i]
        while nxt < hi - lo and nk[i] < fanout[S[i]] and np.linalg.norm(O[nxt] - P) <= tol * (1 + np.linalg.norm(P)):
            parent[nxt] = i
            nk[i] += 1
            nxt += 1
    return nk, parent


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    same_inf = ~np.isfinite(a) & ~np.isfinite(b) & (a == b)
    return bool(np.all(same_inf | (fin & (np.abs(a - b) <= tol * (1 + np.abs(a))))))


def audit_traces(scene, ref, got, prec="f64", tol=None, rays=None):
    """Every ray (tree) on which two traces of the same input rays differ, explained or not.

    ref: the fp64 trace (the oracle's, or the device's fp64 trace when `got` is fp32); got: the trace audited.  Both are
    host dicts in the reference's order (input ray major, FIFO within a tree) as `SegmentBatch.to_host(reference_order
    =True)` and `oracle.trace` return them.  prec: precision of `got` ("f64": FLOOR 1e-10, "f32": 1e-4).  tol: the
    site's field tolerance (default 1e-9 in fp64, 2e-3 in fp32); every record before the first difference must agree to
    it in origin, direction and length (|a - b| <= tol (1 + |a|)), and the first differing record in origin and
    direction.  rays: the input rays' host dict (their wavelengths are what `tir` needs in dispersive glass).

    Returns a dict of arrays over the diverged rays: ray, kstar (first differing record of the tree, FIFO order), leaf_ref
    / leaf_got (surfaces there; -1 escaped, -2 dead), cause ("edge", "tie", "tir", "guard", "escape", and for a spherical cap
    the decisions of its root search, "box", "scan", "cut", "graze": _Leaves.search_margins; "prefix" when an earlier record disagrees, "missing" when a record is absent, "unexplained" otherwise), margin, delta, bound
    (C_DELTA * delta + FLOOR[prec]) and explained; plus `same` (bool per input ray) and `n_rays`."""
    if tol is None:
        tol = 1e-9 if prec == "f64" else 2e-3
    floor = FLOOR[prec]
    n = int(max(np.max(ref["ray"], initial=-1), np.max(got["ray"], initial=-1), -1 if rays is None else len(rays["ox"]) - 1)) + 1
    leaves = _Leaves(scene, None if rays is None else np.asarray(rays["wavelength"], dtype=np.float64))
    ba, bb = _tree_bounds(ref, n), _tree_bounds(got, n)
    ca, cb = np.diff(ba), np.diff(bb)
    # same surface sequence: per record of `ref`, the record of `got` at the same place in its tree
    sa, sb = np.asarray(ref["surface"]), np.asarray(got["surface"])
    ra = np.asarray(ref["ray"], dtype=np.int64)
    eq = ca[ra] == cb[ra]
    j = np.where(eq, bb[ra] + np.arange(len(ra)) - ba[ra], 0)
    bad_rec = ~eq
    bad_rec[eq] = sa[eq] != sb[j[eq]]
    same = ca == cb
    same[np.unique(ra[bad_rec])] = False
    out = {k: [] for k in ("ray", "kstar", "leaf_ref", "leaf_got", "cause", "margin", "delta", "bound", "explained")}
    fields = lambda x, lo, hi: (np.stack([x["ox"][lo:hi], x["oy"][lo:hi], x["oz"][lo:hi]], 1).astype(np.float64),
                                np.stack([x["dx"][lo:hi], x["dy"][lo:hi], x["dz"][lo:hi]], 1).astype(np.float64),
                                np.asarray(x["length"][lo:hi], dtype=np.float64), np.asarray(x["surface"][lo:hi]))
    link = 1e-6 if prec == "f64" else 1e-4  # how close a child starts to where its parent ended (relative)
    for r in np.flatnonzero(~same):
        Oa, Da, La, Sa = fields(ref, ba[r], ba[r + 1])
        Ob, Db, Lb, Sb = fields(got, bb[r], bb[r + 1])
        nka, par = _children(ref, ba[r], ba[r + 1], link, leaves.fanout)
        nkb, _ = _children(got, bb[r], bb[r + 1], link, leaves.fanout)
        cause, k, margin, delta = "unexplained", 0, np.inf, np.inf
        for k in range(max(len(Sa), len(Sb))):
            if k >= len(Sa) or k >= len(Sb):
                cause = "missing"
                break
            if not (_close(Oa[k], Ob[k], tol)):
                cause = "prefix"
                break
            L = max([x for x in (La[k], Lb[k]) if np.isfinite(x)], default=0.0)
            delta = float(np.linalg.norm(Oa[k] - Ob[k]) + L * np.linalg.norm(Da[k] - Db[k]))
            if not _close(Da[k], Db[k], tol):
                p = int(par[k])
                if p < 0:
                    cause = "prefix"
                    break
                # same start, another direction: the parent's hit had another outcome (refracted / totally reflected)
                k = p
                Pa = Oa[p] + La[p] * Da[p]
                cause, margin = "tir", leaves.tir_margin(int(Sa[p]), Pa, Da[p], r)
                delta = float(np.linalg.norm(Oa[p] - Ob[p]) + La[p] * np.linalg.norm(Da[p] - Db[p]))
                break
            if Sa[k] != Sb[k] or nka[k] != nkb[k]:
                a, b = int(Sa[k]), int(Sb[k])
                Pa = Oa[k] + La[k] * Da[k] if a >= 0 else None
                Pb = Oa[k] + Lb[k] * Da[k] if b >= 0 else None  # where `got` hit, on the fp64 ray
                cand = {}
                if a == b:
                    if a >= 0:
                        cand["tir"] = leaves.tir_margin(a, Pa, Da[k], r)
                elif a >= 0 and b >= 0:
                    cand["edge"] = min(leaves.edge(a, Pa), leaves.edge(b, Pb))
                    cand["tie"] = max(abs(La[k] - Lb[k]), leaves.on_surface(b, Pb), leaves.on_surface(a, Pa))
                elif (a >= 0) != (b >= 0) and min(a, b) == -1:
                    cand["escape"] = leaves.edge(a, Pa) if a >= 0 else leaves.edge(b, Pb)
                if a != b and max(a, b) >= 0:
                    short = min(x for x in (La[k], Lb[k]) if np.isfinite(x))
                    cand["guard"] = max(short - GUARD_FACTOR * GUARD[prec], 0.0)
                if a != b:
                    for leaf, P in ((a, Pa), (b, Pb)):
                        for c, m in leaves.search_margins(leaf, Oa[k], Da[k], P).items():
                            cand[c] = min(cand.get(c, np.inf), m)
                if cand:
                    cause = min(cand, key=lambda c: cand[c])
                    margin = float(cand[cause])
                break
            if not (_close(La[k], Lb[k], tol)):
                # the same leaf at another root (a cap met on its far side where the other trace met the near one)
                cand = {}
                for L in (La[k], Lb[k]):
                    for c, m in leaves.search_margins(int(Sa[k]), Oa[k], Da[k], Oa[k] + L * Da[k] if np.isfinite(L) else None).items():
                        cand[c] = min(cand.get(c, np.inf), m)
                cand.pop("graze", None)  # (both traces found roots)
                cause = min(cand, key=lambda c: cand[c]) if cand else "prefix"
                margin = float(cand[cause]) if cand else np.inf
                break
        bound = C_DELTA * delta + floor if np.isfinite(delta) else floor
        ok = cause in CAUSES and margin <= bound
        out["ray"].append(int(r))
        out["kstar"].append(int(k))
        out["leaf_ref"].append(int(Sa[k]) if k < len(Sa) else -9)
        out["leaf_got"].append(int(Sb[k]) if k < len(Sb) else -9)
        out["cause"].append(cause if (ok or cause in ("prefix", "missing")) else "unexplained:" + cause)
        out["margin"].append(float(margin))
        out["delta"].append(float(delta))
        out["bound"].append(float(bound))
        out["explained"].append(bool(ok))
    rep = {k: np.array(v) for k, v in out.items()}
    rep["explained"] = rep["explained"].astype(bool)
    rep["same"] = same
    rep["n_rays"] = n
    rep["scene"] = scene
    return rep


def cause_counts(rep):
    """{cause: number of diverged rays} (unexplained rays under "unexplained:<nearest cause>", "prefix" or "missing")."""
    causes, counts = np.unique(rep["cause"], return_counts=True) if len(rep["cause"]) else ([], [])
    return {str(c): int(k) for c, k in zip(causes, counts)}


def table(rep, rows=None, limit=40):
    """A readable table of (some of) the diverged rays."""
    rows = range(len(rep["ray"])) if rows is None else rows
    leaves = rep["scene"].leaves
    kind = lambda s: type(leaves[s].surface).__name__ if 0 <= s < len(leaves) and leaves[s] is not None else {-1: "escape", -2: "dead", -9: "-"}.get(s, "?")
    lines = [f"{'ray':>7} {'kstar':>5} {'leaf_ref':>16} {'leaf_got':>16} {'cause':>20} {'margin':>10} {'delta':>10} {'bound':>10}"]
    for i in list(rows)[:limit]:
        a, b = int(rep["leaf_ref"][i]), int(rep["leaf_got"][i])
        lines.append(f"{rep['ray'][i]:>7} {rep['kstar'][i]:>5} {f'{a} {kind(a)}':>16} {f'{b} {kind(b)}':>16} {rep['cause'][i]:>20} "
                     f"{rep['margin'][i]:>10.3g} {rep['delta'][i]:>10.3g} {rep['bound'][i]:>10.3g}")
    return "\n".join(lines)


def assert_explained(rep):
    """Fails, with a table of the offenders, when any diverged ray is not explained.  With OT_AUDIT_LOG set, first appends
    one JSON line (the running test, rays, diverged rays per cause) to that file: how campaigns record the counts."""
    log = os.environ.get("OT_AUDIT_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", ""), "rays": int(rep["n_rays"]),
                                "causes": cause_counts(rep)}) + "\n")
    bad = np.flatnonzero(~rep["explained"]) if len(rep["ray"]) else []
    if len(bad):
        raise AssertionError(f"{len(bad)} of {rep['n_rays']} rays diverge without a marginal cause "
                             f"(all diverged: {cause_counts(rep)}):\n" + table(rep, bad))
