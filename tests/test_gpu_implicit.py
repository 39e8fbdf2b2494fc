"""GPU (MI355X): user-defined implicit surfaces traced as verified 3-D Chebyshev series (OT_SHAPE_IMPLICIT_CHEB) — against the
reference fixture (g29), against the built-in Sphere / Cylinder they reproduce, fp32 against fp64, the lane-per-tree kernel
against the generation loop, the global-image kernel against the LDS one, and the run-time check of ray_tracing."""
import numpy as np
import pytest

import helpers
import implicit_scenes
import optable_amd as oa
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch
from optable_amd.engine import get_engine
from optable_amd.fp32_audit import assert_explained, audit_traces, cause_counts
from optable_amd.scene import SceneError

pytestmark = pytest.mark.gpu
U = implicit_scenes.implicit_surface_classes(oa)
Q = 1j * np.pi * W.W0**2 / W.WL


def _table(comps, implicit=True):
    t = oa.OpticalTable()
    t.implicit_surfaces = implicit
    t.add_components(comps)
    return t


def test_g29_ray_tracing_matches_reference_fixture(capsys):
    from test_gpu_parity import rays_to_segs

    sc = implicit_scenes.g29_implicit_surfaces(oa)
    gold = helpers.golden("g29_implicit_surfaces")
    table = _table(sc["components"])
    out = table.ray_tracing(sc["rays"], perfomance_limit=sc["limit"])
    got = rays_to_segs(out)
    got["ray"] = gold["seg_tree"]
    assert len(out) == len(gold["seg_tree"])
    np.testing.assert_array_equal(got["has_q"], gold["seg_has_q"])
    helpers.assert_segments_match(got, gold, gold["in_has_q"])


def _twins(implicit):
    """A cylinder wall about the lab x axis (a light pipe) and a sphere cap mirror behind it: built-in shapes or their
    implicit twins, one component class."""
    cyl = U["ImplicitCylinder"](2.0, 6.0) if implicit else oa.Cylinder(2.0, 6.0)
    cap = U["ImplicitSphere"](5.0, 0.5) if implicit else oa.Sphere(5.0, 0.5)
    return [U["CurvedMirror"]([0, 0, 0], cyl).RotY(np.pi / 2), U["CurvedMirror"]([0, 0, 0], cap)]


def _twin_rays(n, precision="f64", seed=5):
    rng = np.random.default_rng(seed)
    r, th = 1.8 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    o = np.stack([np.full(n, -2.5), r * np.cos(th), r * np.sin(th)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n)], 1)
    return RayBatch.from_arrays(o, d, wavelength=W.WL, q=Q, precision=precision), o, d


K = 10


def test_implicit_sphere_and_cylinder_equal_the_built_in_shapes():
    builtin, implicit = _table(_twins(False), implicit=False), _table(_twins(True))
    assert {n.shape for n in implicit.compile().nodes[:2]} == {oa.shapes.IMPLICIT_CHEB}
    batch, o, d = _twin_rays(100_000)
    a = builtin.trace_batch(batch, max_segments=K).to_host(reference_order=True)
    b = implicit.trace_batch(batch, max_segments=K).to_host(reference_order=True)
    assert len(a["ray"]) > 3 * 100_000  # the rays bounce along the pipe and off the cap
    rep = audit_traces(builtin.compile(), a, b, prec="f64", tol=1e-9,
                       rays=RayBatch.from_arrays(o, d, wavelength=W.WL, q=Q, device="cpu").to_host())
    print("diverged:", cause_counts(rep))
    assert_explained(rep)  # every ray whose surface sequence differs, explained by a marginal decision


def test_fp32_trace_of_implicit_surfaces_tracks_fp64():
    table = _table(_twins(True))
    b64, o, d = _twin_rays(20_000)
    b32, _, _ = _twin_rays(20_000, "f32")
    s64 = table.trace_batch(b64, max_segments=K).to_host(reference_order=True)
    s32 = table.trace_batch(b32, max_segments=K).to_host(reference_order=True)
    rep = audit_traces(table.compile(), s64, s32, prec="f32", tol=2e-3,
                       rays=RayBatch.from_arrays(o, d, wavelength=W.WL, q=Q, device="cpu").to_host())
    print("diverged:", cause_counts(rep))
    assert_explained(rep)


def _torus_scene():
    torus = U["CurvedMirror"]([6, 0, 0], U["Torus"](10.0, 4.0, 1.5), reflectivity=0.4, transmission=0.6).RotZ(np.pi + 0.02)
    back = oa.Mirror([1, 0, 0], radius=3.0).RotZ(0.01)
    return _table([back, torus]).compile()


def _tree_rays(n, seed=9):
    rng = np.random.default_rng(seed)
    o = np.stack([np.full(n, 2.0), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n)], 1)
    return RayBatch.from_arrays(o, d, wavelength=W.WL, q=Q)


def test_partially_reflecting_torus_trees_equal_the_generation_loop():
    eng = get_engine()
    scene, batch, cap = _torus_scene(), _tree_rays(4096), 12
    eng.upload(scene)
    assert eng.trees_plan("f64", cap)["kernel"]
    trees = eng.trace_trees(batch, cap, layout="append")
    gens = eng.trace_tree(batch, cap)
    a, b = trees.to_host(reference_order=True), gens.to_host(reference_order=True)
    assert len(a["ray"]) > 2 * 4096
    np.testing.assert_array_equal(a["ray"], b["ray"])
    np.testing.assert_array_equal(a["surface"], b["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


def test_global_image_tree_kernel_equals_the_lds_one():
    """OT_OPT_TREES_GLOBAL_IMAGE sends every scene to the kernels for images beyond the LDS.  A scene with implicit surfaces
    must take the one that reads everything from global memory (IMG = 0), not the one that keeps the records in LDS and has
    no implicit-series branch (IMG = 2): the records would differ if it did."""
    eng = get_engine()
    scene, batch, cap = _torus_scene(), _tree_rays(4096), 12
    eng.upload(scene)
    lds = eng.trace_trees(batch, cap, layout="append").to_host(reference_order=True)
    eng.set_option(abi.OPT_TREES_GLOBAL_IMAGE, 1)
    try:
        glob = eng.trace_trees(batch, cap, layout="append").to_host(reference_order=True)
    finally:
        eng.set_option(abi.OPT_TREES_GLOBAL_IMAGE, 0)
    np.testing.assert_array_equal(lds["ray"], glob["ray"])
    np.testing.assert_array_equal(lds["surface"], glob["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_array_equal(lds[f], glob[f], err_msg=f)


def test_ray_tracing_checks_hits_against_the_users_aperture():
    from test_implicit_cpu import _holed

    surf = _holed(U)(10.0, 4.0, 1.5)
    table = _table([U["CurvedMirror"]([6, 0, 0], surf).RotZ(np.pi)])
    ok = table.ray_tracing([oa.Ray([0, -0.5, 0.2], [1, 0, 0], wavelength=W.WL, w0=W.W0)])
    assert len(ok) == 2
    with pytest.raises(SceneError, match="within_boundary"):
        table.ray_tracing([oa.Ray([0, -0.4, 0.3], [1, 0, 0], wavelength=W.WL, w0=W.W0)])  # RotZ(pi): local y = -lab y
