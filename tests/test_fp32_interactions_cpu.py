"""CPU: the single-interaction catalogue (tests/fp32_interactions.py) checked on the oracle alone — every form is one leaf of
the expected kind, its fan meets it clear of every decision, reaches the branch of trace_core.h it is named for, and loses at most
1 % of its rays to the exclusion rule (none on the planar forms with constant indices) — and the comparator checked without a
device: the oracle's own records rounded to float32 pass every bound, an error of 256 u in one field does not, and neither do
three defects a flat 2e-3 cannot see."""
import numpy as np
import pytest

import form_scenes
import fp32_interactions as fi
from optable_amd import abi, shapes
from optable_amd.components import REFRACT

FORMS_WITH_CHILDREN = [n for n in fi.NAMES if fi.FORMS[n].expect["children"] > 0]


def _copy(ref):
    got = {f: np.array(ref[f], dtype=np.float64) for f in abi.SEG_FIELDS}
    got["ray"], got["surface"] = np.array(ref["ray"]), np.array(ref["surface"])
    return got


def _local_hits(name):
    """(P, d, t, hit) of every input ray in the leaf frame, from the oracle's segment 0"""
    import optable_amd as oa

    scene, rays, K, bnd = fi.reference(name)
    comp = fi.leaf(oa, name)
    M, g = np.asarray(comp.transform_matrix, dtype=float), np.asarray(comp.origin, dtype=float)
    ref = bnd.ref
    first = bnd.first
    assert np.array_equal(np.asarray(ref["ray"])[first], np.arange(len(rays["ox"])))  # one segment 0 per input ray, in order
    t = np.asarray(ref["length"])[first]
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    hit = np.asarray(ref["surface"])[first] == 0
    P = (o + np.where(hit, t, 0.0)[:, None] * d - g) @ M
    return comp, P, d @ M, t, hit


def _normal(name, comp, P):
    target = fi.FORMS[name].fan["target"]
    if target[0] in ("disc", "rect"):
        return np.tile([1.0, 0.0, 0.0], (len(P), 1))
    if target[0] == "polygon":
        nrm = form_scenes.polygon_normal(target[1])
        return np.tile([1.0, 0.0, 0.0] if nrm is None else nrm, (len(P), 1))
    return np.stack([comp.surface.normal(p) for p in P])


def _distance_to_edges(P, verts):
    best = np.full(len(P), np.inf)
    for a, b in zip(verts, np.roll(verts, -1, axis=0)):
        ab = b - a
        s = np.clip(((P - a) @ ab) / (ab @ ab), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(P - (a + s[:, None] * ab), axis=1))
    return best


def _aperture_margin(name, P):
    target = fi.FORMS[name].fan["target"]
    rho = np.hypot(P[:, 1], P[:, 2])
    if target[0] == "disc":
        return 1.0 - rho
    if target[0] == "rect":
        return np.minimum(1.0 - np.abs(P[:, 1]), 1.0 - np.abs(P[:, 2]))
    if target[0] == "sphere":
        return form_scenes.cap_half_width(fi.CAP_R, fi.CAP_H) - rho
    if target[0] == "asphere":
        return target[1] - rho
    if target[0] == "cylinder":
        return np.minimum(fi.CYL_R * (fi.CYL_ARC[1] - np.abs(np.arctan2(P[:, 1], P[:, 0]))), 1.0 - np.abs(P[:, 2]))
    verts = form_scenes.polygon_vertices(target[1])
    if verts.shape[1] == 2:
        verts = np.stack([np.zeros(len(verts)), verts[:, 0], verts[:, 1]], 1)
    return _distance_to_edges(P, verts)


@pytest.mark.parametrize("name", fi.NAMES)
def test_form_compiles_to_one_leaf_of_its_kind(name):
    scene = fi.compiled(name)
    e = fi.FORMS[name].expect
    assert scene.n_nodes == 1 and scene.n_leaves == 1
    nd = scene.nodes[0]
    assert nd.kind == abi.NODE_LEAF and not nd.flags & abi.NODE_CHECK_AABB and nd.max_interact_count < 0
    assert (nd.shape, nd.interaction, nd.roc_kind) == (e["shape"], e["interaction"], e["roc_kind"])
    assert fi.preset(scene) == e["preset"]
    # what the leaf can emit: a mirror coat on an interface may add the totally reflected ray (none of this fan's is)
    assert scene.max_children == e["children"] + ("coated" in name) and scene.always_branches == (name in fi.BRANCHING)
    assert tuple(nd.origin[:]) == fi.ORIGIN and np.count_nonzero(np.abs(np.array(nd.M[:])) < 0.01) == 0  # a dense M, large coordinates
    # the series whose length enters N
    if name == "dispersion_cauchy_callable":
        m = scene.materials[nd.mat2]
        assert m.kind == abi.MAT_CHEB and int(scene.aux[int(m.n)]) == fi.CAUCHY_TERMS
    if name == "asphere_series":
        assert int(scene.aux[nd.aux]) == fi.SERIES_TERMS


@pytest.mark.parametrize("name", fi.NAMES)
def test_fan_meets_its_form_clear_of_every_decision(name, oracle):
    form = fi.FORMS[name]
    scene, rays, K, bnd = fi.reference(name)
    n = len(rays["ox"])
    assert n == fi.N_RAYS * len(form.wavelengths_nm or (0,))
    comp, P, d, t, hit = _local_hits(name)
    assert hit.mean() >= 0.6, hit.mean()  # (the catalogue's floor; the aimed fans meet their form with every ray)
    assert _aperture_margin(name, P[hit]).min() >= 1e-3
    dn = np.einsum("nk,nk->n", d[hit], _normal(name, comp, P[hit]))
    assert np.all(np.sign(dn) == form.expect["dn_sign"]), "the fan arrives on the other side"
    if comp.__class__.__name__ != "Lens" and scene.nodes[0].interaction == REFRACT:
        wl_m = rays["wavelength"][hit] * scene.unit
        n1, n2 = np.array([comp._n1(w) for w in wl_m]), np.array([comp._n2(w) for w in wl_m])
        st = np.where(dn < 0, n1 / n2, n2 / n1) * np.sqrt(1 - dn * dn)
        assert np.abs(st - 1).min() >= 1e-3, "a refraction within 1e-3 of the critical angle"
        total = st >= 1
        assert total.all() if "total_reflection" in name else not total.any()
    for f in ("ox", "oy", "oz", "dx", "dy", "dz", "wavelength", "q_re", "q_im", "intensity", "n", "pathlength"):
        assert np.array_equal(rays[f], fi.f32(rays[f])), f  # what the device reads


@pytest.mark.parametrize("name", fi.NAMES)
def test_form_reaches_its_branch(name, oracle):
    """From the oracle's records: the number of children, n changed or kept, the intensity shares; every child leaves the scene."""
    form = fi.FORMS[name]
    scene, rays, K, bnd = fi.reference(name)
    ref, e = bnd.ref, form.expect
    ray, first = np.asarray(ref["ray"]), bnd.first
    hit = np.asarray(ref["surface"])[first] == 0
    count = np.bincount(ray, minlength=len(rays["ox"]))
    assert np.all(count[hit] == 1 + e["children"])
    later = ~first
    assert np.all(np.asarray(ref["surface"])[later] == -1) and np.all(np.isinf(np.asarray(ref["length"])[later]))
    k_in_ray = np.arange(len(ray)) - np.flatnonzero(first)[np.cumsum(first) - 1]
    for child in range(e["children"]):
        m = k_in_ray == child + 1
        assert m.sum() == hit.sum()
        n_in = rays["n"][ray[m]]
        changed = np.asarray(ref["n"])[m] != n_in
        assert changed.all() if e["n_changes"][child] else not changed.any(), (child, "n")
        np.testing.assert_allclose(np.asarray(ref["intensity"])[m], e["shares"][child] * rays["intensity"][ray[m]], rtol=1e-12)
    if form.has_q:
        assert np.all(np.hypot(ref["q_re"], ref["q_im"]) > 1.0)
    else:  # has_q false: q stays what it was
        assert not np.any(ref["q_re"]) and not np.any(ref["q_im"]) and not np.any(rays["flags"] & abi.RAY_HAS_Q)
    if name.startswith("lens"):
        m = later
        inv_f = 1.0 / scene.nodes[0].focal_length
        assert (inv_f > 0) == ("converging" in name)
        assert np.array_equal(np.asarray(ref["pathlength"])[m], rays["pathlength"][ray[m]])  # the thin lens advances neither
        if form.has_q:
            assert np.all(np.asarray(ref["q_im"])[m] != rays["q_im"][ray[m]])  # the cdiv branch
    if name == "mirror_passing":  # the ray goes on: its direction, q and pathlength advanced by t
        t = np.asarray(ref["length"])[first][ray[later]]
        d_in = np.stack([rays[f][ray[later]] for f in ("dx", "dy", "dz")], 1)
        np.testing.assert_allclose(np.stack([np.asarray(ref[f])[later] for f in ("dx", "dy", "dz")], 1), d_in / np.linalg.norm(d_in, axis=1, keepdims=True), atol=1e-15)
        np.testing.assert_allclose(np.asarray(ref["q_re"])[later], rays["q_re"][ray[later]] + t, rtol=1e-14)
        np.testing.assert_allclose(np.asarray(ref["pathlength"])[later], rays["pathlength"][ray[later]] + t * rays["n"][ray[later]], rtol=1e-14)


@pytest.mark.parametrize("name", fi.NAMES)
def test_excluded_share(name, oracle):
    scene, rays, K, bnd = fi.reference(name)
    share = bnd.excluded.mean()
    assert share <= 0.01, share
    if fi.FORMS[name].planar_const:
        assert not bnd.excluded.any()


def test_the_planar_constant_forms_are_the_ones_meant():
    for name, form in fi.FORMS.items():
        nd = fi.compiled(name).nodes[0]
        planar = nd.shape in (shapes.CIRCLE, shapes.RECT, shapes.POLYGON2D)
        const = all(m.kind == abi.MAT_CONST for m in fi.compiled(name).materials[: fi.compiled(name).n_materials])
        assert form.planar_const == (planar and const), name


def test_every_N_is_counted_and_capped():
    for name in fi.NAMES:
        counted, held = fi.counted_N(name), fi.N_of(name)
        assert set(counted) == set(fi.GROUPS.values())
        assert all(1 <= held[k] <= fi.N_CAP and held[k] == min(counted[k], fi.N_CAP) for k in counted), (name, counted)
    # the forms whose count exceeds the cap (DESIGN.md section 5 names them): the long series of the Cauchy flint and what is
    # built on an asphere's normal
    assert sorted(fi.OVER_CAP) == ["asphere_all_terms", "asphere_exact", "asphere_parabola", "asphere_series", "dispersion_cauchy_callable"]
    assert all(set(v) <= {"d", "q", "n"} for v in fi.OVER_CAP.values())


# -- the comparator, without a device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fi.NAMES)
def test_oracle_rounded_to_float_passes_every_bound(name, oracle):
    """No bound lies below what a float can hold."""
    scene, rays, K, bnd = fi.reference(name)
    got = _copy(bnd.ref)
    for f in abi.SEG_FIELDS:
        got[f] = fi.f32(got[f])
    bad, worst = fi.compare(bnd, rays, got)
    assert not bad, bad
    assert max(worst.values()) <= 0.5  # half an ulp of the value is u |x| <= u S, and N >= 1 ... 2 where a product is rounded
    for f in abi.SEG_FIELDS:
        assert np.all(bnd.tol[f][~bnd.first] >= fi.U * np.abs(np.asarray(bnd.ref[f])[~bnd.first]) * (1 - 1e-12)) or f == "length"


@pytest.mark.parametrize("field", abi.SEG_FIELDS)
def test_an_error_of_256_u_in_one_field_fails(field, oracle):
    """A relative error of 256 u in one field of the oracle's own records: in the child records (for `length`: in segment 0, the
    children's is infinite).  The bound is absolute in S, so a form can miss the error only where the field is small against S
    (the y component of a direction along x, the length 1 of a ray that starts inside a cylinder at coordinates of 30): exactly
    where 256 u |x| lies inside N (u S + D) on every record, and on fewer than half of the forms."""
    caught, forms = 0, 0
    for name in fi.NAMES:
        scene, rays, K, bnd = fi.reference(name)
        m = bnd.first if field == "length" else ~bnd.first
        m = m & ~bnd.excluded[np.asarray(bnd.ref["ray"])] & np.isfinite(np.asarray(bnd.ref[field]))
        x = np.asarray(bnd.ref[field], dtype=np.float64)
        if not m.any() or not np.any(x[m]):
            continue
        forms += 1
        got = _copy(bnd.ref)
        got[field][m] = x[m] * (1 + 256 * fi.U)
        bad, worst = fi.compare(bnd, rays, got)
        detectable = np.any(np.abs(x[m]) * 256 * fi.U > bnd.tol[field][m] * (1 + 1e-9))
        assert bool(bad) == bool(detectable), (name, field, bad)
        assert all(b.startswith(field + ":") for b in bad), bad  # ... and no other field is blamed
        caught += bool(bad)
    assert forms >= 30 and caught > forms / 2, (field, caught, forms)


def test_another_surface_fails(oracle):
    for name in fi.NAMES:
        scene, rays, K, bnd = fi.reference(name)
        got = _copy(bnd.ref)
        got["surface"][0] += 1
        bad, _ = fi.compare(bnd, rays, got)
        assert len(bad) == 1 and bad[0].startswith("surface:"), (name, bad)
        got = _copy(bnd.ref)
        got["ray"][-1] += 1
        assert fi.compare(bnd, rays, got)[0], name
        got = {k: v[:-1] for k, v in _copy(bnd.ref).items()}  # a record short
        assert fi.compare(bnd, rays, got)[0], name


def test_a_segment_0_that_is_not_the_input_fails(oracle):
    scene, rays, K, bnd = fi.reference("mirror_reflecting")
    for f in ("ox", "dz", "intensity", "q_im", "n", "pathlength"):
        got = _copy(bnd.ref)
        k = np.flatnonzero(bnd.first)[7]
        got[f][k] = np.nextafter(np.float32(got[f][k]), np.float32(np.inf))  # one ulp of float32
        bad, _ = fi.compare(bnd, rays, got)
        assert len(bad) == 1 and bad[0].startswith(f + ": segment 0"), (f, bad)


@pytest.mark.parametrize("name", FORMS_WITH_CHILDREN)
def test_defect_child_direction_not_renormalised(name, oracle):
    """a child direction scaled by 1 + 1e-5: what a missing renormalisation leaves"""
    scene, rays, K, bnd = fi.reference(name)
    got = _copy(bnd.ref)
    for f in ("dx", "dy", "dz"):
        got[f][~bnd.first] *= 1 + 1e-5
    bad, _ = fi.compare(bnd, rays, got)
    assert bad and all(b[:2] in ("dx", "dy", "dz") for b in bad), bad


@pytest.mark.parametrize("name", ["sphere_inside_constant", "sphere_inside_NBK7"])
def test_defect_q_t_with_the_roc_of_the_other_side(name, oracle):
    """q_t on the inside of a cap formed with +ROC where the ray sees -ROC (optical_component.py:640-660)"""
    import optable_amd as oa

    scene, rays, K, bnd = fi.reference(name)
    comp = fi.leaf(oa, name)
    ref, later = bnd.ref, ~bnd.first
    ray = np.asarray(ref["ray"])[later]
    t = np.asarray(ref["length"])[bnd.first][ray]
    q1 = rays["q_re"][ray] + t + 1j * rays["q_im"][ray]
    wl_m = rays["wavelength"][ray] * scene.unit
    nin, nout = np.array([comp._n2(w) for w in wl_m]), np.array([comp._n1(w) for w in wl_m])
    q_t = {sign: q1 / ((nin - nout) / (sign * fi.CAP_R * nout) * q1 + nin / nout) for sign in (-1.0, +1.0)}
    np.testing.assert_allclose(q_t[-1.0], np.asarray(ref["q_re"])[later] + 1j * np.asarray(ref["q_im"])[later], rtol=1e-12)  # the restatement is the oracle's
    for sign, fails in ((-1.0, False), (+1.0, True)):
        got = _copy(ref)
        got["q_re"][later], got["q_im"][later] = q_t[sign].real, q_t[sign].imag
        bad, _ = fi.compare(bnd, rays, got)
        assert bool(bad) == fails, bad
        assert all(b.startswith("q_") for b in bad)


@pytest.mark.parametrize("name", [n for n in fi.NAMES if fi.FORMS[n].n_in != 1.0])
def test_defect_pathlength_advanced_by_t_in_glass(name, oracle):
    """pathlength + t where the ray runs in glass: + t * n is the optical path"""
    scene, rays, K, bnd = fi.reference(name)
    ref, later = bnd.ref, ~bnd.first
    ray = np.asarray(ref["ray"])[later]
    t = np.asarray(ref["length"])[bnd.first][ray]
    for index, fails in ((rays["n"][ray], False), (1.0, True)):
        got = _copy(ref)
        got["pathlength"][later] = rays["pathlength"][ray] + t * index
        bad, _ = fi.compare(bnd, rays, got)
        assert bool(bad) == fails, bad
        assert all(b.startswith("pathlength:") for b in bad)


def test_a_subset_is_compared_with_its_own_rays(oracle):
    """one ray of a fan, traced alone (the n = 1 launches of the GPU tests): ray 0 of the trace is ray `i` of the bound"""
    name = "flat_splitting"
    scene, rays, K, bnd = fi.reference(name)
    i = 77
    alone = oracle.trace(scene, fi.subset(rays, [i]), max_trace_num=K)
    bad, worst = fi.compare(bnd, rays, alone, only_rays={0: i})
    assert not bad and max(worst.values()) == 0.0
    bad, _ = fi.compare(bnd, rays, alone, only_rays={0: i + 1})
    assert bad
