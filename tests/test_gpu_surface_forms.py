"""GPU (MI355X): every surface FORM of the catalogue (tests/form_scenes.py) through the trace kernels.  The kernels branch on
the form of a surface — the paraboloid shortcut against the general conic (square root and division), the two sides of the
convex-start shortcut, sags that are not convex or go NaN inside the local box and must take the full scan, arcs of the
cylinder wall that contain theta = 0 or end at -pi, boolean aperture programs with a union, a polygon operand and a stack
deeper than two, the closed-form root search of a spherical cap with the reference's scan quirks re-created by hand (a cap
deeper than a hemisphere, whose local box clips its belly; a chord inside one sample interval; the t = 100 cut; a start inside
the ball), the even-odd test on concave, clockwise and self-overlapping polygons and the 3-D polygon's two in-plane bases —
and the other suites build one form of each.  Per form: the fp64 default launch against the oracle, lane
per ray against the rolling lists bit for bit in both precisions and in every output layout, a splitting variant as ray
trees against the oracle, the fp32 default launch against the oracle with every diverging ray explained, and the object
API against what the reference recorded (tests/golden/g30-g35).  Only launch options that other suites already set; what
ran is read back from last_launch()."""
import numpy as np
import pytest

import form_scenes as FS
import helpers
import optable_amd as oa
from optable_amd import abi
from optable_amd.batch import RayBatch
from optable_amd.engine import get_engine
from optable_amd.fp32_audit import assert_explained, audit_traces

pytestmark = pytest.mark.gpu
Q = 1j * np.pi * FS.W0**2 / FS.WL
N, K = 4099, 12  # not a multiple of 64, more than one workgroup


_CASES = {}


def _case(name, oracle):
    """(table, compiled scene, origins, directions, host rays, oracle trace) of a form's fan: computed once, shared, read only."""
    if name not in _CASES:
        table = oa.OpticalTable()
        table.add_components(FS.components(oa, name))
        scene = table.compile()
        o, d = FS.fan(name, N)
        host = RayBatch.from_arrays(o, d, wavelength=FS.WL, q=Q, device="cpu").to_host()
        _CASES[name] = (table, scene, o, d, host, oracle.trace(scene, host, max_trace_num=K))
    return _CASES[name]


def _batch(o, d, precision="f64"):
    return RayBatch.from_arrays(o, d, wavelength=FS.WL, q=Q, precision=precision)


def _assert_matches_oracle(oracle, scene, host, ref, got, cap):
    """`ray` and `surface` equal, every field but q to 1e-9, q within oracle.q_tolerance (1e-9 until it has met an asphere)."""
    assert len(got["ray"]) == len(ref["ray"])
    np.testing.assert_array_equal(got["ray"], ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        if f not in ("q_re", "q_im"):
            np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    qtol, clean = oracle.q_tolerance(scene, host, ref, cap)
    qerr = np.hypot(got["q_re"] - ref["q_re"], got["q_im"] - ref["q_im"])
    assert np.all(qerr <= qtol), f"q off by {float((qerr / qtol).max()):.2f} x its tolerance"
    return clean


@pytest.mark.parametrize("name", FS.NAMES)
def test_form_fp64_default_launch_matches_oracle(name, oracle):
    table, scene, o, d, host, ref = _case(name, oracle)
    segs = table.trace_batch(_batch(o, d), max_segments=K, scene=scene)
    got = segs.to_host(reference_order=True)
    with FS.named(name):
        clean = _assert_matches_oracle(oracle, scene, host, ref, got, K)
        assert clean.all() or name in FS.LENSES or name in FS.BOWLS  # without an asphere the bound on q IS 1e-9
        np.testing.assert_array_equal(segs.count.abs().cpu().numpy() >= K, ref["capped"].astype(bool))
        met = np.isin(ref["surface"], FS.form_leaves(scene, name)).sum()
        assert met == 0 if name in FS.NEVER_HIT else met > 0.6 * N  # (a full sphere's local box has no width: never hit)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", FS.NAMES)
def test_form_lane_per_ray_equals_rolling_lists_in_every_layout(name, precision):
    table = oa.OpticalTable()
    table.add_components(FS.components(oa, name))
    scene = table.compile()
    batch = _batch(*FS.fan(name, N), precision=precision)
    eng = get_engine()
    out = {}
    try:
        with FS.named(name):
            eng.set_option(abi.OPT_KERNEL, 1)
            out["lane per ray, slots"] = table.trace_batch(batch, max_segments=K, layout="slots", scene=scene)
            assert eng.last_launch()["kernel"] == 1, eng.last_launch()
            out["lane per ray, tiled"] = table.trace_batch(batch, max_segments=K, layout="tiled", scene=scene)
            info = eng.last_launch()
            assert info["kernel"] == 1 and info["pair_queue"] & 8, info
            eng.set_option(abi.OPT_KERNEL, 2)
            out["rolling lists, slots"] = table.trace_batch(batch, max_segments=K, layout="slots", scene=scene)
            assert eng.last_launch()["kernel"] == 2, eng.last_launch()
            out["rolling lists, append"] = table.trace_batch(batch, max_segments=K, layout="append", scene=scene)
            info = eng.last_launch()
            assert info["kernel"] == 2 and info["pair_queue"] & 4, info
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
    host = {k: v.to_host(reference_order=True) for k, v in out.items()}
    base = host.pop("lane per ray, slots")
    with FS.named(name):
        assert len(base["ray"]) > N
        for variant, got in host.items():
            for f in abi.SEG_FIELDS + ("ray", "surface", "count"):
                np.testing.assert_array_equal(base[f], got[f], err_msg=f"{variant}: {f}")


@pytest.mark.parametrize("name", FS.NAMES)
def test_form_splitting_variant_matches_oracle(name, oracle):
    """The form's interface reflects 0.3 and passes 0.7 of every ray (planar forms: an uncoated glass slab in front): ray trees
    through the generation / lane-per-tree kernels of the form's preset, fp64, against the oracle."""
    n = 1500
    table = oa.OpticalTable()
    table.add_components(FS.components(oa, name, split=True))
    scene = table.compile()
    o, d = FS.fan(name, n)
    batch = _batch(o, d)
    host = batch.to_host()
    got = table.trace_batch(batch, max_segments=K, scene=scene).to_host(reference_order=True)
    ref = oracle.trace(scene, host, max_trace_num=K)
    with FS.named(name):
        assert scene.max_children == 2 and len(ref["ray"]) > 2.5 * n  # (a narrow arc is met once: 3 segments per ray, less the misses)
        _assert_matches_oracle(oracle, scene, host, ref, got, K)


def _sequences(trace, n):
    bounds = np.searchsorted(trace["ray"], np.arange(n + 1))
    return [trace["surface"][bounds[i]:bounds[i + 1]] for i in range(n)], bounds


@pytest.mark.parametrize("name", FS.NAMES)
def test_form_fp32_default_launch_against_oracle(name, oracle):
    """Single precision, the default call: at least 99.9 % of the rays visit exactly the surfaces the oracle's visit, their
    segment starts agree to 2e-3, and EVERY other ray is an explained edge case (fp32_audit).

    (`sph_far` stood at 0.98048 before the sphere branch of hit_leaf put the root at an emitted ray's own start point at 0: after
    a segment of 85 - 100 units that root landed at t = 1.1e-5 .. 1.9e-5, beyond the fp32 guard, and the cap was met twice.)"""
    table, scene, o, d, host, ref = _case(name, oracle)
    got = table.trace_batch(_batch(o, d, "f32"), max_segments=K, scene=scene).to_host(reference_order=True)
    a, ba = _sequences(ref, N)
    b, bb = _sequences(got, N)
    same = np.array([np.array_equal(x, y) for x, y in zip(a, b)])
    print(f"fp32 share {name}: {same.mean():.5f} ({int((~same).sum())} of {N} rays diverge)")
    with FS.named(name):
        assert_explained(audit_traces(scene, ref, got, prec="f32", tol=2e-3, rays=host))
        assert same.mean() > 0.999, f"{int((~same).sum())} of {N} rays diverge (all explained)"
        ia = np.concatenate([np.arange(ba[i], ba[i + 1]) for i in np.flatnonzero(same)])
        ib = np.concatenate([np.arange(bb[i], bb[i + 1]) for i in np.flatnonzero(same)])
        for f in ("ox", "oy", "oz"):
            np.testing.assert_allclose(got[f][ib], ref[f][ia], atol=2e-3, err_msg=f)


@pytest.mark.parametrize("name", FS.NAMES)
def test_form_object_api_matches_reference_fixture(name):
    """Drop-in API on the recorded scenes: OpticalTable.ray_tracing(List[Ray]) returns what the reference returned."""
    from test_gpu_parity import rays_to_segs

    gold = FS.sub_fixture(helpers.golden(FS.FAMILY[name]), name)
    sc = FS.scene(oa, name)
    table = oa.OpticalTable()
    table.add_components(sc["components"])
    out = table.ray_tracing(sc["rays"], perfomance_limit=sc["limit"])
    got = rays_to_segs(out)
    got["ray"] = gold["seg_tree"]  # Ray objects carry no tree index; order is checked field by field
    with FS.named(name):
        assert len(out) == len(gold["seg_tree"])
        np.testing.assert_array_equal(got["has_q"], gold["seg_has_q"])
        helpers.assert_segments_match(got, gold, gold["in_has_q"])


CURVED_SEEDS = (0, 1, 2)


def _curved(seed, n):
    rng = np.random.default_rng(7300 + seed)
    table = oa.OpticalTable()
    table.add_components(FS.curved_scene(oa, rng))
    o = np.stack([np.zeros(n), rng.uniform(-4, 4, n), rng.uniform(-0.4, 0.4, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.15, 0.15, n), rng.uniform(-0.03, 0.03, n)], 1)
    return table, o, d


@pytest.mark.parametrize("seed", CURVED_SEEDS)
def test_block_pool_on_curved_scenes_of_catalogue_forms(seed):
    """test_gpu_pool's random curved scenes with the asphere lenses drawn from the catalogue: the block pool through the
    append layout against the per-wave lists through the slots, fp32, bit for bit."""
    import torch

    n, cap = 8003, 14
    table, o, d = _curved(seed, n)
    batch = _batch(o, d, "f32")
    eng = get_engine()
    eng.upload(table.compile())
    try:  # (engine level: a ray tree that branches is marked in `count` and left to the caller, by both kernels alike)
        eng.set_option(abi.OPT_KERNEL, 2)
        eng.set_option(abi.OPT_BLOCK_POOL, 0)
        lists = eng.trace(batch, cap)
        assert not eng.last_launch()["pair_queue"] & 16
        eng.set_option(abi.OPT_BLOCK_POOL, -1)
        eng.set_option(abi.OPT_APPEND_CHUNK, 64)
        app = eng.trace(batch, cap, layout="append")
        pooled = bool(eng.last_launch()["pair_queue"] & 16)
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
        eng.set_option(abi.OPT_BLOCK_POOL, -1)
        eng.set_option(abi.OPT_APPEND_CHUNK, 512)
    if not pooled:  # (a scene that happens to draw no curved surface but the closing lens can fall into another preset)
        pytest.skip("this scene is outside the preset k_trace_pool is built for")
    assert torch.equal(lists.count, app.count)
    a, b = lists.to_host(reference_order=True), app.to_host(reference_order=True)
    assert len(a["ray"]) == int(lists.count.abs().sum().item())
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"seed {seed}: {f}")


@pytest.mark.parametrize("seed", CURVED_SEEDS)
def test_curved_scenes_of_catalogue_forms_match_oracle(seed, oracle):
    n, cap = 8003, 14
    table, o, d = _curved(seed, n)
    scene = table.compile()
    batch = _batch(o, d)
    host = batch.to_host()
    got = table.trace_batch(batch, max_segments=cap, scene=scene).to_host(reference_order=True)
    ref = oracle.trace(scene, host, max_trace_num=cap)
    with FS.named(f"curved scene {seed}"):
        _assert_matches_oracle(oracle, scene, host, ref, got, cap)


def _assert_block_pool_equals_lists(table, batch, cap, where):
    import torch

    eng = get_engine()
    eng.upload(table.compile())
    try:
        eng.set_option(abi.OPT_KERNEL, 2)
        eng.set_option(abi.OPT_BLOCK_POOL, 0)
        lists = eng.trace(batch, cap)
        assert not eng.last_launch()["pair_queue"] & 16
        eng.set_option(abi.OPT_BLOCK_POOL, -1)
        eng.set_option(abi.OPT_APPEND_CHUNK, 64)
        app = eng.trace(batch, cap, layout="append")
        pooled = bool(eng.last_launch()["pair_queue"] & 16)
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
        eng.set_option(abi.OPT_BLOCK_POOL, -1)
        eng.set_option(abi.OPT_APPEND_CHUNK, 512)
    assert pooled, f"{where}: a scene with deep caps is a scene of the curved-surface preset"
    assert torch.equal(lists.count, app.count)
    a, b = lists.to_host(reference_order=True), app.to_host(reference_order=True)
    assert len(a["ray"]) == int(lists.count.abs().sum().item())
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{where}: {f}")


def _curved_deep(seed, n):
    comps, o, d = FS.curved_deep_case(oa, seed, n)
    table = oa.OpticalTable()
    table.add_components(comps)
    return table, o, d


@pytest.mark.parametrize("seed", FS.DEEP_SEEDS)
def test_block_pool_on_curved_scenes_of_deep_caps(seed):
    """The random curved scenes with their spherical caps drawn from hemispheres and caps deeper than one (the x bound of the
    upload, a belly outside the local box), in both orientations: block pool + append = per-wave lists + slots, fp32, bit for bit."""
    n, cap = 8003, 14
    table, o, d = _curved_deep(seed, n)
    _assert_block_pool_equals_lists(table, _batch(o, d, "f32"), cap, f"seed {seed}")


@pytest.mark.parametrize("seed", FS.DEEP_SEEDS)
def test_curved_scenes_of_deep_caps_match_oracle(seed, oracle):
    n, cap = 8003, 14
    table, o, d = _curved_deep(seed, n)
    scene = table.compile()
    batch = _batch(o, d)
    host = batch.to_host()
    got = table.trace_batch(batch, max_segments=cap, scene=scene).to_host(reference_order=True)
    ref = oracle.trace(scene, host, max_trace_num=cap)
    with FS.named(f"curved scene of deep caps {seed}"):
        caps = [k for k, leaf in enumerate(scene.leaves) if type(leaf.surface).__name__ == "Sphere" and leaf.surface.height >= leaf.surface.radius]
        assert np.isin(ref["surface"], caps).sum() > 0.25 * n  # the deep caps are met
        _assert_matches_oracle(oracle, scene, host, ref, got, cap)
