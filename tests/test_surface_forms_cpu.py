"""CPU: the surface-form catalogue (tests/form_scenes.py: every conic / polynomial asphere form in both orientations, exact
sags, reflective bowls, the arcs of the cylinder wall, boolean apertures with unions, polygons and nested programs, spherical
caps from shallow to full, polygons of every form).  The
oracle reproduces what the reference recorded for every form (tests/golden/g30-g35, tools/make_golden.py forms_fixture), this
package's constructors build the reference's geometry, the reference's own objects compile to the same device tables where
they can be imported, and each form's batch ray fan is a fair test: it meets the form, does not sit on edges and, through a
strongly curved cap, does not amplify a last-digit difference beyond what the reference's own roots define."""
import numpy as np
import pytest

import form_scenes as FS
import helpers
import optable_amd as oa
from optable_amd import abi
from optable_amd.batch import RayBatch
from test_adapter_reference import live_ref  # noqa: F401  (the fixture: the reference package where it can be imported)

Q = 1j * np.pi * FS.W0**2 / FS.WL


@pytest.fixture(scope="module")
def gold():
    return {fam: helpers.golden(fam) for fam in FS.FAMILIES}


def _table(name):
    sc = FS.scene(oa, name)
    table = oa.OpticalTable()
    table.add_components(sc["components"])
    return table, sc


def _fan_trace(oracle, name, n=600, K=12):
    table = oa.OpticalTable()
    table.add_components(FS.components(oa, name))
    scene = table.compile()
    o, d = FS.fan(name, n)
    host = RayBatch.from_arrays(o, d, wavelength=FS.WL, q=Q, device="cpu").to_host()
    return scene, o, d, oracle.trace(scene, host, max_trace_num=K)


def test_catalogue_covers_what_it_says(oracle):
    assert len(FS.NAMES) == len(set(FS.NAMES)) == (2 * len(FS.ASPHERES) + len(FS.EXACT) + len(FS.BOWLS) + len(FS.CYLINDERS) + len(FS.APERTURES)
                                                    + len(FS.SPHERES) + len(FS.POLYGONS))
    assert FS.NAMES.index("sph_shallow") == 2 * len(FS.ASPHERES) + len(FS.EXACT) + len(FS.BOWLS) + len(FS.CYLINDERS) + len(FS.APERTURES)  # appended
    forms = FS.ASPHERES
    assert forms["parabola"]["kappa"] == -1 and all(f["kappa"] != -1 for k, f in forms.items() if k != "parabola")
    assert forms["negative_R"]["R"] < 0 and forms["all_terms"]["a8"] != 0
    corner2 = 2 * 1.2**2  # r^2 at the corner of the local box of a lens of diameter 2.4
    radicand = {k: 1 - (1 + f["kappa"]) * corner2 / f["R"] ** 2 for k, f in forms.items()}
    assert radicand["strong"] == pytest.approx(0.04) and radicand["beyond_domain"] < 0 and radicand["edge"] < 0
    assert all(radicand[k] > 0 for k in FS.IN_DOMAIN)
    # boolean programs: a union, a polygon operand, stacks deeper than two
    progs = {k: build(oa).lower().aux for k, (build, _) in FS.APERTURES.items()}
    assert float(oa.shapes.CSG_OR) in progs["csg_union"] and len(progs["csg_polygon"]) > 13 + 2 * len(FS.TRIANGLE)
    assert progs["csg_island"][0] == 5 and progs["csg_deeper"][0] == 7  # tokens: three / four operands on the stack at once
    # spherical caps: which side of the upload's choice (height < R: radial bound, else the x bound), and the local box
    sph = FS.SPHERES
    assert sph["sph_shallow"]["h"] < sph["sph_shallow"]["R"] and sph["sph_hemisphere"]["h"] == sph["sph_hemisphere"]["R"]
    for k in ("sph_deep", "sph_deep_turned", "sph_nearly_full", "sph_bowl_deep", "sph_inside", "sph_in_group"):
        R, h = sph[k]["R"], sph[k]["h"]
        box = oa.Sphere(R, h).get_bbox_local()
        assert h > R and 0 < box[3] == -box[2] == box[5] < R and box[0] == R - h < 0, k  # the belly |y| in (a, R] is outside the box
    assert oa.Sphere(2.0, 4.0).get_bbox_local()[2:] == (0.0, 0.0, 0.0, 0.0) and sph["sph_full"]["h"] == 2 * sph["sph_full"]["R"]
    with pytest.raises(TypeError):  # the default height cannot be asked for by leaving it out (surfaces.py:292)
        oa.Sphere(2.0)
    # sph_chords: a ray along y crosses the box of the hemisphere over w = 2 R (+ 2 EPS); its chord is centred in the crossing,
    # i.e. in the middle one of the nine sample intervals, and is found iff it is longer than the interval: delta > delta*
    R = sph["sph_chords"]["R"]
    dstar = FS.chord_threshold(R, 2 * R + 2e-9)
    assert FS.CHORD_DELTAS[0][1] < dstar < FS.CHORD_DELTAS[1][0] and dstar == pytest.approx(0.012384, abs=1e-6)
    scene, o, d, tr = _fan_trace(oracle, "sph_chords")
    delta = R - np.hypot(o[:, 0], o[:, 2])
    hit = np.zeros(len(o), bool)
    hit[tr["ray"][tr["surface"] == 0]] = True
    assert (delta < dstar).sum() > 100 and (delta > dstar).sum() > 100
    np.testing.assert_array_equal(hit, delta > dstar)  # (every one of these lines meets the sphere: delta > 0)
    # sph_far: the first segment ends on the cap before the cut and on the mirror behind it beyond, and both occur
    scene, o, d, tr = _fan_trace(oracle, "sph_far")
    first = tr["surface"][np.searchsorted(tr["ray"], np.arange(len(o)))]
    crown = sph["sph_far"]["R"]
    t_plane = (o[:, 0] - crown) / -d[:, 0]  # where the ray enters the local box; the crown's sag adds < 0.07 to it
    assert set(first.tolist()) == {0, 1} and np.all(t_plane[first == 0] < 100 - 0.07) and np.all(t_plane[first == 1] > 100)
    # bowls: rays that meet the same leaf three times and more
    for k in ("sph_bowl_hemisphere", "sph_bowl_deep"):
        scene, o, d, tr = _fan_trace(oracle, k)
        assert (np.bincount(tr["ray"][tr["surface"] == 0], minlength=len(o)) >= 3).mean() > 0.05, k
    # sph_inside: every ray starts inside the ball and inside its local box
    o, _ = FS.fan("sph_inside", 600)
    assert np.all(np.linalg.norm(o, axis=1) < 0.9 + 1e-12)
    # sph_in_group: the cap is a child of a group
    nodes = oa.compile_scene(FS.components(oa, "sph_in_group")).node_table()
    assert (nodes["kind"] == abi.NODE_GROUP).sum() == 1
    # polygons
    poly = {k: oa.Polygon(FS.polygon_vertices(k), normal=FS.polygon_normal(k)) for k in FS.POLYGONS}
    area = {k: 0.5 * float(np.sum(p._verts2d[:, 0] * np.roll(p._verts2d[:, 1], -1) - np.roll(p._verts2d[:, 0], -1) * p._verts2d[:, 1]))
            for k, p in poly.items()}
    assert area["poly_clockwise"] < -1.0 and area["poly_concave"] > 0.5
    c = np.zeros(3)
    assert not poly["poly_star"].within_boundary(c) and poly["poly_star"].within_boundary(np.array([0.0, 0.0, 0.8]))  # centre: a hole; a tip
    assert not poly["poly_concave"].within_boundary(np.array([0.0, 0.0, -0.5])) and poly["poly_concave"].within_boundary(np.array([0.0, 0.0, 0.3]))
    for k in FS.POLYGONS:  # the fan's interior triangles are inside, whatever the vertex order
        for tri in FS.polygon_pieces(k):
            p3 = np.array([0.0, *tri.mean(0)]) if "place" not in FS.POLYGONS[k] else FS._place(FS.POLYGONS[k]["place"], tri.mean(0)[None])[0]
            assert poly[k].within_boundary(p3), k
    ell = poly["poly_level_vertices"]._verts2d  # horizontal edges in the frame the even-odd test casts its ray in, and vertices at dyadic levels
    assert sum(ell[i, 1] == ell[(i + 1) % len(ell), 1] for i in range(len(ell))) == 3
    o, d = FS.fan("poly_level_vertices", 600)
    assert np.isin(o[:, 1], np.unique(np.asarray(FS.POLYGONS["poly_level_vertices"]["verts"])[:, 0])).sum() >= 600 // 8
    near = poly["poly3d_near_x"]  # |n.x| > 0.99: the in-plane basis is built on y, u = n x (0, 1, 0), not on x
    assert 0.99 < abs(near._normal[0]) < 1.0 and near._normal[1] != 0.0
    np.testing.assert_allclose(near._basis[0], np.cross(near._normal, [0.0, 1.0, 0.0]) / np.linalg.norm(np.cross(near._normal, [0.0, 1.0, 0.0])), atol=1e-15)
    assert abs(poly["poly3d_tilted"]._normal[0]) < 0.99
    v3 = FS.polygon_vertices("poly3d_derived_normal")
    assert FS.polygon_normal("poly3d_derived_normal") is None and not np.allclose(v3[:, 0], 0.0)
    want = np.cross(v3[2] - v3[0], v3[1] - v3[0])
    np.testing.assert_allclose(poly["poly3d_derived_normal"]._normal, want / np.linalg.norm(want), atol=1e-15)
    flat = poly["poly3d_axis_plane"]
    assert tuple(flat._normal) == (0.0, 1.0, 0.0) and flat.get_bbox_local()[2:4] == (0.0, 0.0) and not flat.planar
    assert all(not poly[k].planar for k in FS.POLYGONS if k.startswith("poly3d")) and all(poly[k].planar for k in FS.POLYGONS if not k.startswith("poly3d"))


@pytest.mark.parametrize("name", FS.NAMES)
def test_form_geometry_matches_reference(name, gold):
    table, _ = _table(name)
    g = FS.sub_fixture(gold[FS.FAMILY[name]], name)
    nodes = table.compile().node_table()
    leaves, groups = nodes[nodes["kind"] == abi.NODE_LEAF], nodes[nodes["kind"] == abi.NODE_GROUP]
    with FS.named(name):
        assert len(leaves) == len(g["leaf_origin"])
        np.testing.assert_allclose(leaves["origin"], g["leaf_origin"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(leaves["M"].reshape(-1, 3, 3), g["leaf_M"], rtol=0, atol=1e-12)
        in_group = g["leaf_in_group"]
        np.testing.assert_allclose(leaves["aabb"][in_group], g["leaf_bbox"][in_group], rtol=0, atol=1e-12)
        np.testing.assert_allclose(groups["aabb"].reshape(-1, 6), g["group_bbox"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", FS.NAMES)
def test_oracle_reproduces_form_fixture(name, gold, oracle):
    table, sc = _table(name)
    g = FS.sub_fixture(gold[FS.FAMILY[name]], name)
    host, n_classes = helpers.pack_host(sc["rays"])
    assert len(sc["rays"]) <= 40 and 0 < int(g["limit"][0]) <= 12
    with FS.named(name):
        np.testing.assert_allclose(np.stack([host["ox"], host["oy"], host["oz"]], 1), g["in_origin"], atol=1e-15)
        np.testing.assert_allclose(np.stack([host["dx"], host["dy"], host["dz"]], 1), g["in_direction"], atol=1e-15)
        got = oracle.trace(table.compile(), host, max_trace_num=int(g["limit"][0]), n_classes=n_classes)
        helpers.assert_segments_match(got, g, g["in_has_q"])
        hit_form = np.isin(got["surface"], FS.form_leaves(table.compile(), name))
        if name in FS.NEVER_HIT:  # a local box of zero width: what the reference recorded is a trace that never meets the form
            assert hit_form.sum() == 0
        else:
            assert hit_form.sum() >= len(sc["rays"]) // 2  # the recorded rays do meet the form


@pytest.mark.parametrize("name", FS.NAMES)
def test_reference_objects_of_a_form_compile_to_the_same_tables(name, live_ref):  # noqa: F811
    """The live branch of tests/test_adapter_reference.py for the catalogue: the reference's closures (sags, boolean apertures)
    are read back into the very tables this package's own classes lower to."""
    if live_ref is None:
        pytest.skip("needs the reference package's own classes, which are not part of the repository")
    mine = helpers.scene_tables(oa.compile_scene(FS.components(oa, name)))
    with FS.named(name):
        helpers.assert_same_tables(helpers.scene_tables(oa.compile_scene(FS.components(live_ref, name))), mine)


def _sequences(trace, n):
    seq = [[] for _ in range(n)]
    for ray, surf in zip(trace["ray"].tolist(), trace["surface"].tolist()):
        seq[ray].append(surf)
    return seq


@pytest.mark.parametrize("name", FS.NAMES)
def test_form_fan_meets_the_form_and_survives_float32_rounding(name, oracle):
    """The batch fan the GPU tests trace (4,099 rays, K = 12), with the oracle alone: at most 0.05 % of the rays change their
    surface sequence when the inputs are rounded to float32 and back (a fan that sits on edges would turn the fp32 tests into
    edge-case counts), and at least 60 % of the rays interact with the form under test."""
    n, K = 4099, 12
    table = oa.OpticalTable()
    table.add_components(FS.components(oa, name))
    scene = table.compile()
    o, d = FS.fan(name, n)
    host = RayBatch.from_arrays(o, d, wavelength=FS.WL, q=Q, device="cpu").to_host()
    rounded = dict(host)
    for f in ("ox", "oy", "oz", "dx", "dy", "dz"):
        rounded[f] = np.asarray(host[f], dtype=np.float64).astype(np.float32).astype(np.float64)
    a = _sequences(oracle.trace(scene, host, max_trace_num=K), n)
    b = _sequences(oracle.trace(scene, rounded, max_trace_num=K), n)
    changed = sum(x != y for x, y in zip(a, b))
    form = set(FS.form_leaves(scene, name))
    assert form, name
    meets = np.mean([bool(form.intersection(s)) for s in a])
    print(f"{name}: {changed} of {n} rays change their sequence under float32 rounding, {meets:.1%} meet the form")
    with FS.named(name):
        assert changed <= 0.0005 * n, f"{changed} of {n} rays change their surface sequence"
        if name in FS.NEVER_HIT:
            assert meets == 0.0, f"{meets:.1%} of the rays meet a form that no ray can meet"
        else:
            assert meets >= 0.60, f"only {meets:.1%} of the rays interact with the form"
        if name in FS.BOWLS or name.startswith("sph_bowl"):  # what the bowls are for: the same surface met again
            assert np.mean([sum(s in form for s in q) >= 2 for q in a]) > 0.2


def _legs(trace, n):
    bounds = np.searchsorted(trace["ray"], np.arange(n + 1))
    return bounds, [trace["surface"][bounds[i]:bounds[i + 1]] for i in range(n)]


def amplification(oracle, scene, o, d, K, h=1e-8):
    """The largest factor by which a displacement h of a ray's start (along x, y, z in turn) grows in any later segment's
    origin or direction, and in q relative to |q| + 1, over the rays that keep their surface sequence; with the oracle alone."""
    n = len(o)
    trace = lambda oo: oracle.trace(scene, RayBatch.from_arrays(oo, d, wavelength=FS.WL, q=Q, device="cpu").to_host(), max_trace_num=K)
    ref = trace(o)
    ba, sa = _legs(ref, n)
    worst, worst_q, kept = 0.0, 0.0, n
    for e in np.eye(3):
        alt = trace(o + h * e)
        bb, sb = _legs(alt, n)
        same = [i for i in range(n) if np.array_equal(sa[i], sb[i])]
        kept = min(kept, len(same))
        ia = np.concatenate([np.arange(ba[i] + 1, ba[i + 1]) for i in same])
        ib = np.concatenate([np.arange(bb[i] + 1, bb[i + 1]) for i in same])
        for f in ("ox", "oy", "oz", "dx", "dy", "dz"):
            worst = max(worst, float(np.abs(ref[f][ia] - alt[f][ib]).max()) / h)
        dq = np.hypot(ref["q_re"][ia] - alt["q_re"][ib], ref["q_im"][ia] - alt["q_im"][ib])
        worst_q = max(worst_q, float((dq / (np.hypot(ref["q_re"][ia], ref["q_im"][ia]) + 1.0)).max()) / h)
    return worst, worst_q, kept


# What the GPU tests compare to 1e-9 must be defined to 1e-9 by the reference's own algorithm.  Its roots carry brentq's
# xtol = 2e-12; a ray that meets a strongly curved refracting cap near the critical angle, or grazing, amplifies such a
# difference without bound.  So no ray of a sphere fan, or of a random deep-cap scene, may amplify a displacement of its
# start more than 400-fold (2e-12 * 400 = 8e-10 < 1e-9; in fp32 a few ulp of 1.2e-7 * 400 stay below the 2e-3 of the fp32 test).
MAX_AMPLIFICATION = 400.0


@pytest.mark.parametrize("name", list(FS.SPHERES))
def test_sphere_fan_is_well_conditioned(name, oracle):
    table = oa.OpticalTable()
    table.add_components(FS.components(oa, name))
    o, d = FS.fan(name, 4099)
    worst, worst_q, kept = amplification(oracle, table.compile(), o, d, 12)
    print(f"{name}: a displacement of a ray's start grows at most {worst:.3g}-fold (q: {worst_q:.3g})")
    assert kept >= 4099 - 2 and worst <= MAX_AMPLIFICATION and worst_q <= MAX_AMPLIFICATION, (name, worst, worst_q, kept)


@pytest.mark.parametrize("seed", FS.DEEP_SEEDS)
def test_random_deep_cap_scene_is_well_conditioned_and_meets_its_caps(seed, oracle):
    n, cap = 8003, 14
    comps, o, d = FS.curved_deep_case(oa, seed, n)
    table = oa.OpticalTable()
    table.add_components(comps)
    scene = table.compile()
    worst, worst_q, kept = amplification(oracle, scene, o, d, cap)
    print(f"random deep-cap scene {seed}: a displacement of a ray's start grows at most {worst:.3g}-fold (q: {worst_q:.3g})")
    assert kept >= n - 8 and worst <= MAX_AMPLIFICATION and worst_q <= MAX_AMPLIFICATION, (seed, worst, worst_q, kept)
    assert scene.max_children == 1
    kinds = {(s.radius, s.height) for s in (leaf.surface for leaf in scene.leaves) if type(s).__name__ == "Sphere"}
    assert kinds & set(FS.DEEP_CAPS) and all(h >= R for R, h in FS.DEEP_CAPS)  # (the other spheres are the faces of the lenses)
