"""CPU: the divergence audit (optable_amd.fp32_audit.audit_traces) bites.

The differential tests of the device let a small share of rays take another surface sequence than the oracle (a ray
within an ulp of an aperture edge may fall to either side) and compare fields on the other rays only.  The audit
asks, for every such ray, whether the two traces agreed up to where they parted and whether the decision there was
marginal.  Here, without a GPU: the oracle against itself diverges nowhere; pairs of oracle traces from inputs a few
ulps apart across a decision are explained under the right cause; and traces mutated the way a kernel bug would
mutate them — each of which the old allowance accepts — are flagged."""
import numpy as np
import pytest

import optable_amd as oa
import scenes
from optable_amd import abi
from optable_amd.batch import RayBatch
from optable_amd.fp32_audit import assert_explained, audit_traces, cause_counts
from test_gpu_fuzz import random_branching_scene, random_scene

Q = 1j * np.pi * scenes.W0**2 / scenes.WL


def _host(o, d, wavelength=scenes.WL):
    return RayBatch.from_arrays(np.asarray(o, float), np.asarray(d, float), wavelength=wavelength, q=Q, device="cpu").to_host()


def _trace(oracle, comps, o, d, K=12):
    table = oa.OpticalTable()
    table.add_components(comps)
    scene = table.compile()
    host = _host(o, d)
    return scene, host, oracle.trace(scene, host, max_trace_num=K)


def old_allowance(ref, got, n, frac=0.002, tol=1e-9):
    """The contract the differential tests kept before the audit: at most `frac` of the rays take another surface
    sequence; every field agrees to `tol` on the other rays."""
    seq = lambda x: [tuple(x["surface"][x["ray"] == i].tolist()) for i in range(n)]
    same = np.array([a == b for a, b in zip(seq(ref), seq(got))])
    if (~same).mean() > frac:
        return False
    kr, kg = same[ref["ray"]], same[got["ray"]]
    return all(np.allclose(got[f][kg], ref[f][kr], rtol=tol, atol=tol) for f in abi.SEG_FIELDS)


def _fuzz(oracle, seed=0, branching=False):
    rng = np.random.default_rng((2000 if branching else 1000) + seed)
    comps = (random_branching_scene if branching else random_scene)(oa, rng)
    n = 1500 if branching else 3000
    s = 3 if branching else 4
    o = np.stack([np.zeros(n), rng.uniform(-s, s, n), rng.uniform(-0.4, 0.4, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.15, 0.15, n), rng.uniform(-0.03, 0.03, n)], 1)
    scene, host, ref = _trace(oracle, comps, o, d, K=14 if branching else 12)
    return scene, host, ref, n


def _copy(x):
    return {k: np.array(v, copy=True) for k, v in x.items()}


def _take(x, keep):
    return {k: (v[keep] if k in abi.SEG_FIELDS + ("ray", "surface") else v) for k, v in x.items()}


@pytest.mark.parametrize("branching", [False, True])
def test_oracle_against_itself(oracle, branching):
    scene, host, ref, n = _fuzz(oracle, 0, branching)
    rep = audit_traces(scene, ref, _copy(ref), rays=host)
    assert rep["same"].all() and len(rep["ray"]) == 0
    again = oracle.trace(scene, host, max_trace_num=14 if branching else 12)
    assert audit_traces(scene, ref, again, rays=host)["same"].all()


# ------------------------------------------------------------------------------------------------- marginal rays
EPS = 1e-14  # scene units: a few ulps of a coordinate of order 1 either side of the decision


def _marginal(oracle, comps, o, d, step, cause, prec="f64", eps=EPS):
    """Two oracle traces of a ray moved by -eps / +eps along `step`: they must part, and the audit must name `cause`."""
    o, d, step = (np.asarray(v, float) for v in (o, d, step))
    scene, host, a = _trace(oracle, comps, [o - eps * step], [d])
    _, _, b = _trace(oracle, comps, [o + eps * step], [d])
    rep = audit_traces(scene, a, b, prec=prec, rays=host)
    assert len(rep["ray"]) == 1, "the two rays did not part: the construction missed the decision"
    assert rep["cause"][0] == cause, (rep["cause"], rep["margin"])
    assert rep["explained"].all()
    assert rep["margin"][0] <= 100 * eps
    return rep


def test_marginal_circle_rim(oracle):
    _marginal(oracle, [oa.Mirror([5, 0, 0], radius=1.0)], [0, 1.0, 0], [1, 0, 0], [0, 1, 0], "escape")


def test_marginal_rectangle_side(oracle):
    comps = [oa.SquareMirror([5, 0, 0], width=1.6, height=1.2), oa.Mirror([9, 0, 0], radius=3.0)]
    _marginal(oracle, comps, [0, 0.8, 0.1], [1, 0, 0], [0, 1, 0], "edge")


def test_marginal_polygon_edge(oracle):
    tri = oa.BaseMirror([5, 0, 0])
    tri.surface = oa.Polygon(np.array([[-1.0, -1.0], [1.0, -1.0], [0.0, 1.0]]))
    comps = [tri, oa.Mirror([9, 0, 0], radius=3.0)]
    # the edge from (y, z) = (1, -1) to (0, 1) crosses z = 0 at y = 0.5, outward normal (2, 1) / sqrt(5); points within
    # |cross| <= 1e-9 of it count as inside (surfaces.py:534-558): the decision lies 1e-9 / sqrt(5) outside the edge
    nrm = np.array([0, 2, 1]) / np.sqrt(5)
    _marginal(oracle, comps, np.array([0, 0.5, 0.0]) + 1e-9 / np.sqrt(5) * nrm, [1, 0, 0], nrm, "edge")


def test_marginal_cylinder_theta_end(oracle):
    cyl = oa.CylMirror([0, 0, 0], radius=1.2, height=2.0, theta_range=(np.pi / 2, np.pi))
    # travelling -y at x ~ 0: hits theta = pi/2 -/+ x / R, just inside or just outside the range
    _marginal(oracle, [cyl], [0, 5, 0.2], [0, -1, 0], [1, 0, 0], "escape")


def test_marginal_tir_at_the_critical_angle(oracle):
    face = oa.BaseRefraciveSurface([0, 0, 0], n1=1.5, n2=1.0, surface=oa.Rectangle(4, 4))
    back = oa.Mirror([3, 0, 0], radius=5.0)  # where the totally reflected ray goes; the refracted one grazes the face
    s = 1 / 1.5  # sin of the critical angle; the ray travels -x inside the n1 = 1.5 side
    d = [-np.sqrt(1 - s * s), s, 0]
    o = -1.0 / np.sqrt(1 - s * s) * np.asarray(d)  # reaches the face at its centre (from x = 1: clear of `back`)
    # the decision is the angle: tilt the direction by +-EPS instead of moving the start
    scene, host, a = _trace(oracle, [face, back], [o], [[d[0] - EPS * s, d[1] + EPS * np.sqrt(1 - s * s), 0]])
    _, _, b = _trace(oracle, [face, back], [o], [[d[0] + EPS * s, d[1] - EPS * np.sqrt(1 - s * s), 0]])
    assert np.sign(a["dx"][1]) != np.sign(b["dx"][1])  # one refracted (-x), one totally reflected (+x)
    rep = audit_traces(scene, a, b, rays=host)
    assert list(rep["cause"]) == ["tir"] and rep["explained"].all() and rep["kstar"][0] == 0, rep


def test_marginal_tie_of_two_crossing_mirrors(oracle):
    """The g21 situation made marginal: two mirrors through the same line; a ray at the line hits both at one t."""
    comps = [oa.Mirror([5, 0, 0], radius=1.0), oa.Mirror([5, 0, 0], radius=1.0).RotZ(0.1)]
    _marginal(oracle, comps, [0, 0, 0.3], [1, 0, 0], [0, 1, 0], "tie")


# the decisions of a spherical cap's root search that are no aperture edge (fp32_audit._Leaves.search_margins)
def _deep_cap():
    cap = oa.SphereRefractive([0, 0, 0], radius=2.0, height=3.2, n1=1.0, n2=1.0, reflectivity=1.0, transmission=0.0)
    return cap, cap.surface.get_bbox_local()[3]  # its local box has the half-width a = 1.6 < R: the belly is outside


def test_marginal_local_box_face_of_a_deep_cap(oracle):
    cap, a = _deep_cap()  # along +x at y = a -/+: inside the box the belly at x = -1.09 is found, outside nothing is searched
    rep = _marginal(oracle, [cap], [-6, a, 0.5], [1, 0, 0], [0, 1, 0], "box")
    assert {int(rep["leaf_ref"][0]), int(rep["leaf_got"][0])} == {0, -1}


def test_marginal_chord_as_long_as_the_sample_step(oracle):
    cap, a = _deep_cap()  # along +y across the box: the chord is centred in the middle sample interval, found iff longer than it
    step = (2 * a + 2e-9) / 9
    _marginal(oracle, [cap], [np.sqrt(4.0 - (step / 2) ** 2), -5, 0], [0, 1, 0], [1, 0, 0], "scan")


def test_marginal_hit_at_the_cut_of_the_search(oracle):
    R = 20.0  # the crown at x = 0; a hit at t = 100 + EPS, where the search ends; the mirror behind catches what the cut lets pass
    cap = oa.SphereRefractive([-R, 0, 0], radius=R, height=0.5, n1=1.0, n2=1.0, reflectivity=1.0, transmission=0.0)
    x_hit = -R + np.sqrt(R * R - 0.25)
    rep = _marginal(oracle, [cap, oa.Mirror([-3, 0, 0], radius=4.0)], [x_hit + 100.0 + 1e-9, 0.5, 0], [-1, 0, 0], [1, 0, 0], "cut", eps=1e-12)
    assert {int(rep["leaf_ref"][0]), int(rep["leaf_got"][0])} == {0, 1}


def test_marginal_tangent_line(oracle):
    cap, a = _deep_cap()  # along +y from y = -a / 2: the point of contact is the scan's sample 3, so any chord shows two sign changes
    u = np.array([0.8, 0, 0.6])
    _marginal(oracle, [cap], 2.0 * u + [0, -a / 2, 0], [0, 1, 0], u, "graze")


def test_a_cap_hit_far_from_the_decisions_of_its_search_is_not_explained(oracle):
    """A hit dropped by a kernel bug, in the middle of the box, of a sample interval and of the search: none of the new causes
    excuses it."""
    cap, a = _deep_cap()
    scene, host, ref = _trace(oracle, [cap], [[6, 0.31, 0.2]], [[-1, 0.013, 0.007]])
    assert ref["surface"][0] == 0
    got = _take(ref, np.arange(len(ref["ray"])) == 0)
    got["surface"][0], got["length"][0] = -1, np.inf
    rep = audit_traces(scene, ref, got, rays=host)
    assert len(rep["ray"]) == 1 and not rep["explained"][0] and rep["margin"][0] > 1e-3, rep


def test_exact_tie_is_not_a_divergence(oracle):
    comps = [oa.Mirror([5, 0, 0], radius=1.0, reflectivity=0.25), oa.Mirror([5, 0, 0], radius=1.0, reflectivity=0.75)]
    scene, host, a = _trace(oracle, comps, [[0, 0.1, 0]], [[1, 0, 0]])
    _, _, b = _trace(oracle, comps, [[0, 0.1, 0]], [[1, 0, 0]])
    assert audit_traces(scene, a, b, rays=host)["same"].all()


# ------------------------------------------------------------------------------------------------- mutations
def _flagged(scene, ref, got, host, n, tol=1e-9):
    assert old_allowance(ref, got, n, tol=tol), "the old allowance already catches this mutation"
    rep = audit_traces(scene, ref, got, rays=host)
    assert len(rep["ray"]) >= 1 and not rep["explained"].all(), rep
    with pytest.raises(AssertionError, match="without a marginal cause"):
        assert_explained(rep)
    return rep


def test_mutation_drop_every_record_of_the_last_ray(oracle):
    scene, host, ref, n = _fuzz(oracle)
    got = _take(ref, ref["ray"] != n - 1)
    rep = _flagged(scene, ref, got, host, n)
    assert list(rep["ray"]) == [n - 1] and rep["cause"][0] == "missing"


def test_mutation_swap_two_rays(oracle):
    scene, host, ref, n = _fuzz(oracle)
    counts = np.bincount(ref["ray"], minlength=n)
    seq = lambda i: tuple(ref["surface"][ref["ray"] == i])
    a = int(np.flatnonzero(counts >= 3)[0])
    b = next(i for i in np.flatnonzero(counts >= 3) if seq(i) != seq(a))
    groups = [np.flatnonzero(ref["ray"] == i) for i in range(n)]
    groups[a], groups[b] = groups[b], groups[a]
    order = np.concatenate(groups)
    got = {k: ref[k][order] for k in abi.SEG_FIELDS + ("surface",)}
    got["ray"] = np.repeat(np.arange(n), [len(g) for g in groups]).astype(ref["ray"].dtype)
    rep = _flagged(scene, ref, got, host, n)
    assert sorted(rep["ray"]) == sorted([a, b]) and set(rep["cause"]) == {"prefix"}


def test_mutation_move_a_mid_path_origin(oracle):
    """A ray that legitimately diverges (across the rim of a mirror) among 2999 that do not; its records before the
    divergence are never compared by the old allowance: moving one by 1e-6 passes it."""
    comps = [oa.Mirror([4, 0, 0], radius=3.0).RotZ(np.pi), oa.Mirror([-3, 0, 0], radius=1.0)]
    n = 3000
    rng = np.random.default_rng(3)
    o = np.stack([np.zeros(n), rng.uniform(-0.9, 0.9, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.tile([1.0, 0, 0], (n, 1))
    o[-1] = [0, 1.0 - 1e-14, 0]  # sent back by the first mirror onto the rim of the second one (|y| = 1)
    scene, host, ref = _trace(oracle, comps, o, d)
    o[-1, 1] = 1.0 + 1e-14
    _, _, got = _trace(oracle, comps, o, d)
    rep = audit_traces(scene, ref, got, rays=host)
    assert list(rep["ray"]) == [n - 1] and rep["explained"].all() and rep["kstar"][0] >= 1, (rep["cause"], rep["kstar"])
    i = np.flatnonzero(got["ray"] == n - 1)[rep["kstar"][0]]  # the start of the record where the traces part
    got["oy"][i] += 1e-6
    rep = _flagged(scene, ref, got, host, n)
    assert list(rep["cause"]) == ["prefix"]


def test_mutation_remove_a_rays_last_segment(oracle):
    scene, host, ref, n = _fuzz(oracle)
    counts = np.bincount(ref["ray"], minlength=n)
    r = int(np.flatnonzero(counts >= 3)[5])
    last = np.flatnonzero(ref["ray"] == r)[-1]
    got = _take(ref, np.arange(len(ref["ray"])) != last)
    rep = _flagged(scene, ref, got, host, n)
    assert list(rep["ray"]) == [r] and not rep["explained"][0]  # (a hit without its child)


def test_mutation_relabel_a_surface_far_from_any_edge(oracle):
    scene, host, ref, n = _fuzz(oracle)
    got = _copy(ref)
    from optable_amd.fp32_audit import _Leaves
    lv = _Leaves(scene)
    for i in np.flatnonzero(ref["surface"] >= 0):
        P = np.array([ref["ox"][i], ref["oy"][i], ref["oz"][i]]) + ref["length"][i] * np.array([ref["dx"][i], ref["dy"][i], ref["dz"][i]])
        s = int(ref["surface"][i])
        if lv.edge(s, P) > 0.1:
            break
    got["surface"][i] = (s + 1) % scene.n_leaves
    rep = _flagged(scene, ref, got, host, n)
    assert list(rep["ray"]) == [ref["ray"][i]] and rep["cause"][0].startswith("unexplained"), rep["cause"]


def test_mutation_drop_one_child_of_a_tree(oracle):
    scene, host, ref, n = _fuzz(oracle, 0, branching=True)
    counts = np.bincount(ref["ray"], minlength=n)
    r = int(np.argmax(counts))
    recs = np.flatnonzero(ref["ray"] == r)
    assert len(recs) >= 4
    got = _take(ref, np.arange(len(ref["ray"])) != recs[2])
    rep = _flagged(scene, ref, got, host, n)
    assert list(rep["ray"]) == [r], rep["cause"]
    assert not rep["explained"][0]


def test_report_counts_causes(oracle):
    comps = [oa.Mirror([5, 0, 0], radius=1.0)]
    scene, host, a = _trace(oracle, comps, [[0, 1.0 - EPS, 0], [0, 0.2, 0]], [[1, 0, 0]] * 2)
    _, _, b = _trace(oracle, comps, [[0, 1.0 + EPS, 0], [0, 0.2, 0]], [[1, 0, 0]] * 2)
    rep = audit_traces(scene, a, b, rays=host)
    assert cause_counts(rep) == {"escape": 1}
    assert_explained(rep)
