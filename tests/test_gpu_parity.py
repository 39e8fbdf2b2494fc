"""GPU (MI355X): the HIP path through the C-ABI against (a) the committed golden fixtures made
from the reference and (b) the CPU oracle on the same seeded inputs, plus size-independent
properties at BASELINE's full cfg-2 size.  Tolerance: 1e-6 relative (north_star) against the
reference fixtures; 1e-9 against the oracle (both fp64, same formulas, different root polish)."""
import os

import numpy as np
import pytest

import helpers
import scenes
import support
from optable_amd import abi
from optable_amd.fp32_audit import assert_explained, audit_traces

pytestmark = pytest.mark.gpu


def rays_to_segs(rays):
    n = len(rays)
    o = np.array([r.origin for r in rays], dtype=float).reshape(n, 3)
    d = np.array([r.direction for r in rays], dtype=float).reshape(n, 3)
    q = np.array([complex(r.qo) if r.qo is not None else 0j for r in rays])
    return dict(ox=o[:, 0], oy=o[:, 1], oz=o[:, 2], dx=d[:, 0], dy=d[:, 1], dz=d[:, 2],
                length=np.array([np.inf if r.length is None else r.length for r in rays]),
                intensity=np.array([r.intensity for r in rays]), q_re=q.real, q_im=q.imag,
                n=np.array([r.n for r in rays]), pathlength=np.array([r._pathlength for r in rays]),
                surface=np.array([-1 if r.alive else 0 for r in rays]),
                has_q=np.array([r.qo is not None for r in rays]))


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_ray_tracing_matches_reference_fixture(name, capsys):
    """Drop-in API: OpticalTable.ray_tracing(List[Ray]) -> List[Ray], same order, same numbers."""
    table, sc = helpers.build(name)
    gold = helpers.golden(name)
    out = table.ray_tracing(sc["rays"], perfomance_limit=sc["limit"])
    got = rays_to_segs(out)
    got["ray"] = gold["seg_tree"]  # Ray objects carry no tree index; order is checked field by field
    assert len(out) == len(gold["seg_tree"])
    np.testing.assert_array_equal(got["has_q"], gold["seg_has_q"])
    helpers.assert_segments_match(got, gold, gold["in_has_q"])
    # ids are inherited by every segment of a tree (base.py:10-22)
    in_ids = [r._id for r in sc["rays"]]
    assert [r._id for r in out] == [in_ids[t] for t in gold["seg_tree"]]
    # interact counters were written back to the components
    scene = table.compile()
    if gold["counts"].size:
        uniq = list(dict.fromkeys(in_ids))
        got_counts = np.array([[c._interact_count.get(i, 0) for i in uniq] for c in scene.limited])
        np.testing.assert_array_equal(got_counts, gold["counts"])
    for m, mon in enumerate(table.monitors):
        np.testing.assert_allclose(np.array([d[0] for d in mon._data_raw]).reshape(-1, 3), gold[f"mon{m}_P"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose([d[2] for d in mon._data_raw], gold[f"mon{m}_t"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose([d[1] for d in mon._data_raw], gold[f"mon{m}_I"], rtol=1e-6, atol=1e-12)


def _batch(o, d, device="cuda"):
    from optable_amd.batch import RayBatch

    q = support.Q
    return RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, device=device)


# q tolerance: 1e-9 until a ray's q has passed an aspheric interface.  ASphere.roc is a 3-point finite difference
# with h = 1e-4*radius (surfaces.py:355-369): rounding noise in F is amplified by 1/h^2 ~ 1.6e7, so a 1-ulp change of
# the INPUT moves the reference algorithm's own q by up to ~1e-4 relative after 50 segments
# (tests/test_oracle_golden.py::test_asphere_q_is_ill_conditioned).  Behind an asphere the bound is therefore 50 x the
# spread of the oracle's q under +-2 ulp of its input, per segment (oracle.q_tolerance) — not a flat number.
# Positions, directions, lengths and path lengths stay at 1e-9 everywhere.
CASES = {
    "cfg2": (lambda oa: scenes.cfg2_components(oa), lambda n: scenes.cfg2_rays(n, 0), 20000, 5),
    "cfg3": (lambda oa: scenes.cfg3_components(oa), lambda n: scenes.cfg3_rays(n, 2), 20000, 20),
    "cfg5": (lambda oa: scenes.cfg5_components(oa), lambda n: scenes.cfg5_rays(n, 3), 3000, 50),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_trace_matches_oracle(case, oracle):
    """Scalable API (RayBatch -> SegmentBatch), fused kernel, against the oracle on the same inputs."""
    import optable_amd as oa

    comps, gen, n, K = CASES[case]
    table = support.table_of(comps(oa))
    o, d = gen(n)
    batch = _batch(o, d)
    segs = table.trace_batch(batch, max_segments=K, layout="slots")
    got = segs.to_host(reference_order=True)
    scene, host = table.compile(), batch.to_host()
    ref = oracle.trace(scene, host, max_trace_num=K)
    assert len(got["ray"]) == len(ref["ray"])
    np.testing.assert_array_equal(got["ray"], ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        if f not in ("q_re", "q_im"):
            np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    qtol, clean = oracle.q_tolerance(scene, host, ref, K)
    qerr = np.hypot(got["q_re"] - ref["q_re"], got["q_im"] - ref["q_im"])
    assert np.all(qerr <= qtol), float((qerr / qtol).max())
    assert case == "cfg5" or clean.all()  # only cfg 5 has aspheres: everywhere else the bound IS 1e-9
    capped = (got["count"] >= K) if "count" in got else segs.capped.cpu().numpy()
    np.testing.assert_array_equal(capped, ref["capped"].astype(bool))


def test_cfg4_dispersion_matches_oracle(oracle):
    """64 wavelengths through an N-BK7 slab (cfg 4 shape): Sellmeier evaluated per ray on the device."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    nb, nwl = 500, 64
    rng = np.random.default_rng(4)
    jit = rng.uniform(-0.3, 0.3, (nb, 2))
    o = np.stack([np.full(nb, -3.0), 2 + jit[:, 0], jit[:, 1]], 1)
    d = np.tile([np.cos(np.pi / 6), -np.sin(np.pi / 6), 0.0], (nb, 1))
    wl = np.repeat(np.linspace(400e-7, 1100e-7, nwl), nb)  # wavelength-major (ray.py:441-444)
    o, d = np.tile(o, (nwl, 1)), np.tile(d, (nwl, 1))
    table = support.table_of([oa.GlassSlab([0, 0, 0], width=2, height=2, thickness=0.5, n1=oa.Vacuum(), n2=oa.Glass_NBK7(), reflectivity=0)])
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl)
    got = table.trace_batch(batch, max_segments=8, layout="slots").to_host(reference_order=True)
    ref = oracle.trace(table.compile(), batch.to_host(), max_trace_num=8)
    np.testing.assert_array_equal(got["count"], 3)  # exactly 3 segments per ray-wavelength pair
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)


def test_branching_batch_matches_oracle(oracle):
    """Generation-by-generation path on a branching scene, many trees at once."""
    import optable_amd as oa

    n = 2000
    rng = np.random.default_rng(7)
    o = np.stack([np.full(n, -3.0), 2 + rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.tile([np.cos(np.pi / 6), -np.sin(np.pi / 6), 0.0], (n, 1))
    table = support.table_of([oa.GlassSlab([0, 0, 0], width=2, height=2, thickness=0.5, n1=1, n2=1.5, reflectivity=0.2),
                    oa.BeamSplitter([3, 0, 0], width=3, height=3, eta=0.4).RotZ(0.3)])
    batch = _batch(o, d)
    segs = table.trace_batch(batch, max_segments=40, layout="slots")
    got = segs.to_host(reference_order=True)
    ref = oracle.trace(table.compile(), batch.to_host(), max_trace_num=40)
    assert len(got["ray"]) == len(ref["ray"])
    np.testing.assert_array_equal(got["ray"], ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    np.testing.assert_array_equal(segs.capped.cpu().numpy(), ref["capped"].astype(bool))


def test_cfg2_full_size_properties():
    """BASELINE cfg 2 at full size (1e6 rays x 5 segments): properties that need no oracle."""
    import torch
    import optable_amd as oa

    n, K = 1_000_000, 5
    table = support.table_of(scenes.cfg2_components(oa))
    o, d = scenes.cfg2_rays(n, 0)
    batch = _batch(o, d)
    segs = table.trace_batch(batch, max_segments=K, layout="slots")
    assert int(segs.count.min()) == K and int(segs.count.max()) == K  # lens, mirror, mirror, lens, escape
    f = {name: segs.field(name).reshape(K, n) for name in abi.SEG_FIELDS}
    surf = segs.surface.reshape(K, n)
    assert bool((surf[:4] >= 0).all()) and bool((surf[4] == -1).all())
    # unit directions
    norm = torch.sqrt(f["dx"] ** 2 + f["dy"] ** 2 + f["dz"] ** 2)
    assert float((norm - 1).abs().max()) < 1e-12
    # continuity: segment k+1 starts where segment k ended
    for a in "xyz":
        end = f["o" + a][:-1] + f["length"][:-1] * f["d" + a][:-1]
        assert float((end - f["o" + a][1:]).abs().max()) < 1e-9
    # mirrors add t*n to the path length, the thin lens does not (optical_component.py:944-946)
    dpl = f["pathlength"][1:] - f["pathlength"][:-1]
    expect = torch.where(surf[:4] == 0, torch.zeros_like(dpl), f["length"][:4] * f["n"][:4])
    assert float((dpl - expect).abs().max()) < 1e-9
    # lossless optics
    assert float((f["intensity"] - 1).abs().max()) == 0.0
    # shard invariance: two half batches reproduce the full batch bit for bit (rays are independent)
    half = n // 2
    a = table.trace_batch(batch.slice(0, half), max_segments=K, layout="slots")
    b = table.trace_batch(batch.slice(half, n), max_segments=K, layout="slots")
    for name in abi.SEG_FIELDS:
        whole = segs.field(name).reshape(K, n)
        assert torch.equal(whole[:, :half], a.field(name).reshape(K, half))
        assert torch.equal(whole[:, half:], b.field(name).reshape(K, n - half))


def test_empty_and_ragged_inputs():
    import optable_amd as oa

    table = support.table_of(scenes.cfg2_components(oa))
    assert table.ray_tracing([]) == []
    for n in (1, 63, 65, 257):  # partial waves / partial blocks
        o, d = scenes.cfg2_rays(n, 5)
        segs = table.trace_batch(_batch(o, d), max_segments=5, layout="slots")
        assert segs.count.tolist() == [5] * n


def test_fp32_trace_tracks_fp64():
    """fp32 entry point: same scene, float streams; tolerance 2e-4 absolute on positions over 5 segments
    (float epsilon 6e-8 x path length ~20 x error growth through two lens passes)."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    n, K = 50000, 5
    table = support.table_of(scenes.cfg2_components(oa))
    o, d = scenes.cfg2_rays(n, 0)
    q = support.Q
    b64 = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q)
    b32 = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision="f32")
    s64 = table.trace_batch(b64, max_segments=K, layout="slots").to_host()
    s32 = table.trace_batch(b32, max_segments=K, layout="slots").to_host()
    np.testing.assert_array_equal(s64["surface"], s32["surface"])
    for f in ("ox", "oy", "oz", "dx", "dy", "dz", "length"):
        np.testing.assert_allclose(s32[f], s64[f], rtol=2e-4, atol=2e-4, err_msg=f)


def test_calculate_abcd_matrix_matches_reference():
    """f2: three device traces + monitor accessors reproduce the reference's ABCD matrices."""
    import optable_amd as oa

    sc = scenes.abcd_4f(oa)
    table = oa.OpticalTable()
    table.add_components(sc["components"])
    table.add_monitors(sc["monitors"])
    Ms = table.calculate_abcd_matrix(sc["monitors"][0], sc["monitors"][1], sc["rays"])
    gold = helpers.golden("g17_abcd")["Ms"]
    # finite differences with disp = rot = 1e-5 amplify 1e-12 trace noise to ~1e-7
    np.testing.assert_allclose(Ms, gold, rtol=1e-5, atol=1e-5)


def test_abcd_batch_matches_reference():
    """f2, scalable form: the same ABCD matrices from a RayBatch without Python objects."""
    import optable_amd as oa
    from optable_amd.table import _pack

    sc = scenes.abcd_4f(oa)
    table = oa.OpticalTable()
    table.add_components(sc["components"])
    rays = sorted(sc["rays"], key=lambda r: r._id)
    batch = _pack(rays, np.arange(len(rays), dtype=np.int32), "cuda")
    Ms = table.abcd_batch(sc["monitors"][0], sc["monitors"][1], batch).cpu().numpy()
    np.testing.assert_allclose(Ms, helpers.golden("g17_abcd")["Ms"], rtol=1e-5, atol=1e-5)


def test_record_batch_matches_object_api():
    """f1: Monitor.record on a SegmentBatch (no Python objects) == the List[Ray] path."""
    import optable_amd as oa

    table, sc = helpers.build("g07_spherical_lenses")
    table.ray_tracing(sc["rays"])   # fills the monitors through the object path
    mon = table.monitors[0]
    from optable_amd.table import _pack

    batch = _pack(sc["rays"], np.arange(len(sc["rays"]), dtype=np.int32), "cuda")
    segs = table.trace_batch(batch, max_segments=16, layout="slots")
    hits = table.record_batch(mon, segs)
    assert len(hits) == mon.ndata
    raw_P = np.array([d[0] for d in mon._data_raw])
    np.testing.assert_allclose(hits.PList(sort=None).cpu().numpy(), raw_P, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(hits.tList(sort=None).cpu().numpy(), [d[2] for d in mon._data_raw], rtol=1e-12, atol=1e-12)
    for sort in ("YZ", "ID"):  # the reference's accessor orders (monitor.py:126-134)
        np.testing.assert_allclose(hits.yList(sort).cpu().numpy(), mon.get_yList(sort=sort), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(hits.zList(sort).cpu().numpy(), mon.get_zList(sort=sort), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(hits.tYList(sort).cpu().numpy(), mon.get_tYList(sort=sort), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(hits.IList(sort).cpu().numpy(), mon.get_IList(sort=sort), rtol=1e-12, atol=1e-12)


def test_launch_options_do_not_change_results():
    """NT stores, register cap and grid size are performance knobs only: bit-identical outputs."""
    import torch
    import optable_amd as oa
    from optable_amd.engine import get_engine

    n, K = 100_003, 5
    table = support.table_of(scenes.cfg2_components(oa))
    o, d = scenes.cfg2_rays(n, 1)
    batch = _batch(o, d)
    eng = get_engine()
    base = table.trace_batch(batch, max_segments=K, layout="slots")
    try:
        for nt, mw, bpc in ((0, 0, 2), (1, 0, 8), (0, 4, 1), (1, 4, 16)):
            eng.set_option(abi.OPT_NT_STORES, nt)
            eng.set_option(abi.OPT_MIN_WAVES, mw)
            eng.set_option(abi.OPT_BLOCKS_PER_CU, bpc)
            other = table.trace_batch(batch, max_segments=K, layout="slots")
            for f in abi.SEG_FIELDS + ("ray", "surface"):
                assert torch.equal(base.field(f), other.field(f)), (f, nt, mw, bpc)
    finally:
        eng.set_option(abi.OPT_NT_STORES, 1)
        eng.set_option(abi.OPT_MIN_WAVES, 4)
        eng.set_option(abi.OPT_BLOCKS_PER_CU, 0)


@pytest.mark.parametrize("case", ["cfg2", "cfg3", "cfg5"])
def test_blocked_kernel_equals_lane_per_ray_kernel(case):
    """k_trace_rolling (persistent waves, per-wave lists of live rays compacted every segment) and k_trace_fused (lane
    per ray) are interchangeable: same slots, same bits."""
    import torch
    import optable_amd as oa
    from optable_amd.engine import get_engine

    comps, gen, n, K = CASES[case]
    n = min(n, 5000) + 37  # ragged last chunk
    table = support.table_of(comps(oa))
    o, d = gen(n)
    batch = _batch(o, d)
    eng = get_engine()
    try:
        eng.set_option(abi.OPT_KERNEL, 1)
        a = table.trace_batch(batch, max_segments=K, layout="slots")
        eng.set_option(abi.OPT_KERNEL, 2)
        b = table.trace_batch(batch, max_segments=K, layout="slots")
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
    assert torch.equal(a.count, b.count)
    valid = a.valid_mask()
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        assert torch.equal(a.field(f)[valid], b.field(f)[valid]), f


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["cfg3", "cfg5"])  # mixed lists under a top-level grid / generation-pure lists
def test_heavy_kernel_edge_sizes_dead_rays_and_finite_lengths(case, prec):
    """The list machinery of k_trace_rolling at its corners — fewer rays than a ticket, exactly one / two tickets, one ray
    more, a cap of one segment, rays that are dead on input (optical_component.py:349) and rays of finite length
    (optical_component.py:184-190) — against the lane-per-ray kernel, bit for bit."""
    import torch
    import optable_amd as oa
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    comps, gen, _, K = CASES[case]
    table = support.table_of(comps(oa))
    eng = get_engine()
    q = support.Q
    try:
        for n, cap in ((1, K), (63, K), (64, 1), (65, 3), (129, K), (1000, K)):
            o, d = gen(n)
            batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision=prec)
            batch.flags[::7] |= abi.RAY_DEAD
            length = torch.full((n,), float("inf"), dtype=batch.ox.dtype, device=batch.device)
            length[1::5] = 6.0  # shorter than the way to most components: those rays end as escapes of finite length
            batch.length = length
            eng.set_option(abi.OPT_KERNEL, 1)
            a = table.trace_batch(batch, max_segments=cap, layout="slots")
            eng.set_option(abi.OPT_KERNEL, 2)
            b = table.trace_batch(batch, max_segments=cap, layout="slots")
            assert torch.equal(a.count, b.count), (n, cap)
            valid = a.valid_mask()
            for f in abi.SEG_FIELDS + ("ray", "surface"):
                x, y = a.field(f)[valid], b.field(f)[valid]
                # both precisions bit for bit: the library is built with -ffp-contract=on, so one source expression is
                # rounded the same way in every instantiation (with the HIP default the fp32 kernels differed in the last
                # digits, <= 5e-5 after 20 bounces)
                assert torch.equal(x, y), (f, n, cap)
            assert int((a.surface.view(cap, n)[0][::7] == -2).sum()) == len(range(0, n, 7))  # dead rays came back as they were
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pair_queue_walk_equals_per_lane_walk(prec):
    """The cooperative top-level walk of k_trace_rolling (trace_core.h flat_grid_hit: candidate (ray, node) pairs queued in
    LDS and tested 64 at a time by whichever lanes are free) against the same kernel with every lane testing its own
    candidates: the same bits for every ray, at sizes with several tickets per wave and a ragged tail.  Single precision packs
    t and the node index into one 64-bit key; double precision keeps t in the key and votes the node index separately."""
    import torch
    import optable_amd as oa
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    comps, gen, _, K = CASES["cfg3"]
    table = support.table_of(comps(oa))
    eng = get_engine()
    q = support.Q
    try:
        eng.set_option(abi.OPT_KERNEL, 2)
        for n in (64, 4097, 200_003):
            o, d = gen(n)
            batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision=prec)
            eng.set_option(abi.OPT_FLAT_QUEUE, 0)
            a = table.trace_batch(batch, max_segments=K, layout="slots")
            eng.set_option(abi.OPT_FLAT_QUEUE, 1)
            b = table.trace_batch(batch, max_segments=K, layout="slots")
            assert torch.equal(a.count, b.count), n
            valid = a.valid_mask()
            for f in abi.SEG_FIELDS + ("ray", "surface"):
                assert torch.equal(a.field(f)[valid], b.field(f)[valid]), (f, n)
            # the same kernel with the records of the live rays in LDS instead of the per-wave global scratch, and the launch
            # shape says which variant ran
            eng.set_option(abi.OPT_LDS_RECORDS, 0)
            c0 = table.trace_batch(batch, max_segments=K, layout="slots")
            shape0 = eng.last_launch()
            eng.set_option(abi.OPT_LDS_RECORDS, 1)
            c1 = table.trace_batch(batch, max_segments=K, layout="slots")
            shape1 = eng.last_launch()
            assert shape0["kernel"] == 2 and shape0["pair_queue"] == 1
            assert shape1["pair_queue"] == (3 if prec == "f32" else 1)  # fp64 records (108 bytes) stay in global memory
            assert torch.equal(c0.count, c1.count) and torch.equal(c0.count, a.count), n
            for f in abi.SEG_FIELDS + ("ray", "surface"):
                assert torch.equal(c0.field(f)[valid], c1.field(f)[valid]), (f, n)
                assert torch.equal(c0.field(f)[valid], a.field(f)[valid]), (f, n)
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
        eng.set_option(abi.OPT_FLAT_QUEUE, 1)
        eng.set_option(abi.OPT_LDS_RECORDS, -1)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pair_queue_round_that_does_not_fit_defers_lanes(prec):
    """The pair queue of a wave holds 512 (ray, leaf) pairs per round, not the worst case of 64 lanes with the fullest
    cells; lanes whose pairs do not fit sit the round out and queue the same cells again (trace_core.h flat_grid_hit).
    cfg 3 never gets there at 512 — so the room is cut to 192 pairs, a third of its typical round: most rounds defer
    lanes, and every record must still equal the per-lane walk's, bit for bit."""
    import torch
    import optable_amd as oa
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    comps, gen, _, K = CASES["cfg3"]
    table = support.table_of(comps(oa))
    eng = get_engine()
    q = support.Q
    o, d = gen(50_003)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision=prec)
    try:
        eng.set_option(abi.OPT_KERNEL, 2)
        eng.set_option(abi.OPT_FLAT_QUEUE, 0)
        a = table.trace_batch(batch, max_segments=K, layout="slots")
        eng.set_option(abi.OPT_FLAT_QUEUE, 192)
        b = table.trace_batch(batch, max_segments=K, layout="slots")
        assert eng.last_launch()["pair_queue"] & 1
        eng.set_option(abi.OPT_FLAT_QUEUE, 1)
        c = table.trace_batch(batch, max_segments=K, layout="slots")
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
        eng.set_option(abi.OPT_FLAT_QUEUE, 1)
    assert torch.equal(a.count, b.count) and torch.equal(a.count, c.count)
    valid = a.valid_mask()
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        assert torch.equal(a.field(f)[valid], b.field(f)[valid]), f
        assert torch.equal(a.field(f)[valid], c.field(f)[valid]), f


def test_pair_queue_room_does_not_cost_resident_waves():
    """The pair queue's room is LDS every wave holds.  Under a grid whose fullest cell lists five leaves the worst case of a
    round is 640 pairs and the room used to be 512 (1 KB): with the records of the live rays in LDS the sixteenth wave of a CU
    no longer fit and the plan fell to 12 (cfg 3's scene under an 8 x 3 grid: 2.95 instead of 2.6 ms, tools/sweep_root_grid.py).
    The plan now takes the largest room that keeps the most waves (optable_hip.hip launch_rolling); a round that overflows it
    defers lanes.  Same records as under the default grid, bit for bit: a grid only accelerates."""
    import torch
    import optable_amd as oa
    import optable_amd.scene as scene_mod
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    comps, gen, _, K = CASES["cfg3"]
    eng = get_engine()
    q = support.Q
    o, d = gen(200_003)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision="f32")
    a = support.table_of(comps(oa)).trace_batch(batch, max_segments=K, layout="append")
    waves_default = eng.last_launch()["threads"] // 64 * eng.last_launch()["workgroups_per_cu"]
    try:
        scene_mod.ROOT_GRID_DIMS = (8, 3)
        table = support.table_of(comps(oa))
        b = table.trace_batch(batch, max_segments=K, layout="append")
    finally:
        scene_mod.ROOT_GRID_DIMS = None
    launch = eng.last_launch()
    assert launch["pair_queue"] & 1
    assert launch["threads"] // 64 * launch["workgroups_per_cu"] == waves_default == 16
    ha, hb = a.to_host(reference_order=True), b.to_host(reference_order=True)
    for f in ha:
        np.testing.assert_array_equal(ha[f], hb[f], err_msg=f)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pair_queue_winner_that_fails_its_own_box_takes_the_per_lane_walk(prec, oracle):
    """In the pair queue a leaf's own AABB test (component_group.py:104-107) is applied to the WINNER of a ray, not to
    every candidate (trace_core.h flat_grid_hit); a ray whose winner fails it repeats the search lane by lane with every
    test on every candidate.  With honest boxes that happens only within rounding of a box face, so the boxes here are
    cut: every second gated leaf keeps z <= 0.1 of a face that reaches z = 1, and the rays that meet the face above
    that must pass THROUGH it, as the reference's gate has it — a quarter of all rays take the fallback.  Same bits as
    the per-lane kernel; in double precision also the oracle's answer for the same (cut) scene."""
    import torch
    import optable_amd as oa
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    comps, gen, _, K = CASES["cfg3"]
    table = support.table_of(comps(oa))
    honest = table.compile()
    scene = table.compile()
    nodes = scene.node_table()
    gated = [i for i in range(len(nodes)) if nodes["kind"][i] == abi.NODE_LEAF and nodes["flags"][i] & abi.NODE_CHECK_AABB]
    assert len(gated) >= 30
    for i in gated[::2]:
        nodes["aabb"][i][5] = 0.1
    n = 20_011
    o, d = gen(n)
    q = support.Q
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision=prec)
    eng = get_engine()
    try:
        eng.set_option(abi.OPT_KERNEL, 2)
        eng.set_option(abi.OPT_FLAT_QUEUE, 0)
        a = table.trace_batch(batch, max_segments=K, scene=scene, layout="slots")
        eng.set_option(abi.OPT_FLAT_QUEUE, 1)
        b = table.trace_batch(batch, max_segments=K, scene=scene, layout="slots")
        assert eng.last_launch()["pair_queue"] & 1
        whole = table.trace_batch(batch, max_segments=K, scene=honest, layout="slots")
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
        eng.set_option(abi.OPT_FLAT_QUEUE, 1)
    assert torch.equal(a.count, b.count)
    valid = a.valid_mask()
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        assert torch.equal(a.field(f)[valid], b.field(f)[valid]), f
    # the cut boxes matter: many rays now pass through a face they used to end on
    changed = (b.count != whole.count).float().mean().item()
    assert changed > 0.1, changed
    if prec == "f64":
        got = b.to_host(reference_order=True)
        ref = oracle.trace(scene, batch.to_host(), max_trace_num=K)
        np.testing.assert_array_equal(got["ray"], ref["ray"])
        np.testing.assert_array_equal(got["surface"], ref["surface"])
        for f in ("ox", "oy", "oz", "length"):
            np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)


@pytest.mark.parametrize("case", ["cfg3", "cfg5"])
def test_acceleration_grids_do_not_change_results(case):
    """Group grids and the top-level grid only choose WHICH nodes get tested; every bit of the output
    must equal the plain linear pass (component_group.py:104-115, optical_table.py:119-123)."""
    import torch
    import optable_amd as oa

    comps, gen, n, K = CASES[case]
    n = min(n, 6000)
    o, d = gen(n)
    batch = _batch(o, d)
    table = support.table_of(comps(oa))
    fast = table.trace_batch(batch, max_segments=K, layout="slots")
    table.accelerate = False
    plain = table.trace_batch(batch, max_segments=K, layout="slots")
    assert torch.equal(fast.count, plain.count)
    valid = fast.valid_mask()
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        assert torch.equal(fast.field(f)[valid], plain.field(f)[valid]), f


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # unused slots are uninitialised memory; they are masked before any assert
@pytest.mark.parametrize("case,min_same", [("cfg3", 0.999), ("cfg5", 0.999)])  # measured: 99.997 % / 100 % (tests/test_gpu_fp32_contract.py audits the rest)
def test_fp32_heavy_scenes_track_fp64(case, min_same):
    """BASELINE cfg 3 / cfg 5 are quoted in fp32.  Single precision cannot promise per-ray identity over
    20-50 bounces (a ray grazing an aperture edge flips between hit and miss at 6e-8 relative), so the
    contract is statistical: at least `min_same` of the rays visit exactly the same surface sequence as
    fp64, and on those rays every segment origin agrees to 2e-3 absolute (scene size ~30, path ~100)."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    comps, gen, n, K = CASES[case]
    n = min(n, 8000)
    table = support.table_of(comps(oa))
    o, d = gen(n)
    q = support.Q
    s64 = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q), max_segments=K, layout="slots")
    s32 = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision="f32"), max_segments=K, layout="slots")
    c64, c32 = s64.count.cpu().numpy(), s32.count.cpu().numpy()
    surf64 = s64.surface.cpu().numpy().reshape(K, n)
    surf32 = s32.surface.cpu().numpy().reshape(K, n)
    valid = np.arange(K)[:, None] < c64[None, :]
    same = (c64 == c32) & np.all((surf64 == surf32) | ~valid, axis=0)
    assert same.mean() >= min_same, same.mean()
    assert_explained(audit_traces(table.compile(), s64.to_host(reference_order=True), s32.to_host(reference_order=True), prec="f32",
                                  tol=2e-3, rays=RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, device="cpu").to_host()))
    for f in ("ox", "oy", "oz"):
        a = s64.field(f).cpu().numpy().reshape(K, n)
        b = s32.field(f).cpu().numpy().reshape(K, n).astype(np.float64)
        err = np.abs(a - b)[valid & same[None, :]]
        assert err.max() < 2e-3, (f, err.max())


@pytest.mark.parametrize("prec,tol", [("f64", 1e-9), ("f32", 2e-4)])
@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # unused slots are uninitialised memory; they are masked before any assert
@pytest.mark.parametrize("case", ["cfg2", "cfg3", "cfg5"])
def test_segment_chain_is_continuous(case, prec, tol):
    """Oracle-free invariant for every kernel variant and precision: segment k+1 starts exactly where
    segment k ended (origin + length*direction), directions are unit vectors, lengths are positive."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    comps, gen, n, K = CASES[case]
    n = min(n, 6000)
    table = support.table_of(comps(oa))
    o, d = gen(n)
    q = support.Q
    segs = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision=prec), max_segments=K, layout="slots")
    cnt = segs.count.cpu().numpy()
    assert (cnt > 0).all()
    f = {name: segs.field(name).cpu().numpy().reshape(K, n).astype(np.float64) for name in ("ox", "oy", "oz", "dx", "dy", "dz", "length")}
    link = np.arange(K - 1)[:, None] < (cnt - 1)[None, :]   # segment k has a successor
    for a in "xyz":
        end = f["o" + a][:-1] + f["length"][:-1] * f["d" + a][:-1]
        assert np.abs(end - f["o" + a][1:])[link].max() < tol * 30, a
    valid = np.arange(K)[:, None] < cnt[None, :]
    norm = np.sqrt(f["dx"] ** 2 + f["dy"] ** 2 + f["dz"] ** 2)
    assert np.abs(norm - 1)[valid].max() < (1e-12 if prec == "f64" else 1e-6)
    assert (f["length"][valid] > 0).all()


def test_fused_path_honours_input_length_and_dead_flags(oracle):
    """Finite input lengths (`t > ray.length` rejects the hit, optical_component.py:184-190) and dead input
    rays (optical_component.py:349) through the one-launch kernel, against the oracle."""
    import torch
    import optable_amd as oa

    n, K = 4096, 5
    table = support.table_of(scenes.cfg2_components(oa))
    o, d = scenes.cfg2_rays(n, 9)
    batch = _batch(o, d)
    rng = np.random.default_rng(9)
    length = np.where(rng.uniform(size=n) < 0.5, rng.uniform(1.0, 9.0, n), np.inf)  # some stop before the lens at t~5
    flags = batch.flags.cpu().numpy()
    flags[::7] |= abi.RAY_DEAD
    batch.flags.copy_(torch.from_numpy(flags))
    batch.length = torch.from_numpy(length).to(batch.device)
    got = table.trace_batch(batch, max_segments=K, layout="slots").to_host(reference_order=True)
    host = batch.to_host()
    host["length"] = length
    ref = oracle.trace(table.compile(), host, max_trace_num=K)
    np.testing.assert_array_equal(got["ray"], ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    assert (got["surface"] == -2).sum() == len(flags[::7])


def test_zero_rays_and_empty_scene():
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    table = support.table_of(scenes.cfg2_components(oa))
    empty = table.trace_batch(RayBatch(0), max_segments=5, layout="slots")
    assert empty.to_host()["ox"].size == 0
    void = oa.OpticalTable()  # no components: every ray escapes unchanged
    o, d = scenes.cfg2_rays(100, 3)
    segs = void.trace_batch(_batch(o, d), max_segments=3, layout="slots").to_host()
    assert segs["count"].tolist() == [1] * 100 and (segs["surface"] == -1).all()
    np.testing.assert_allclose(segs["dx"], d[:, 0], rtol=0, atol=1e-15)


def test_lazy_materialisation_and_csv_export(tmp_path):
    """f3/f4: pull only some rays of a device trace back as Ray objects; CSV export of table.rays."""
    import optable_amd as oa
    from optable_amd.table import _pack

    table, sc = helpers.build("g01_gaussian_beam")
    rays = sc["rays"]
    full = table.ray_tracing(rays)
    batch = _pack(rays, np.arange(len(rays), dtype=np.int32), "cuda")
    segs = table.trace_batch(batch, max_segments=8, layout="slots")
    some = table.materialize(segs, rays, select=[1, 4])
    want = [r for r in full if r._id in (rays[1]._id, rays[4]._id)]
    assert len(some) == len(want) == 5
    for a, b in zip(some, want):
        np.testing.assert_allclose(a.origin, b.origin, atol=1e-12)
        np.testing.assert_allclose(a.direction, b.direction, atol=1e-12)
        assert a.alive == b.alive and a._id == b._id and (a.length is None) == (b.length is None)
    out = tmp_path / "rays.csv"
    table.export_rays_csv(str(out))
    lines = out.read_text().strip().splitlines()
    assert lines[0].startswith("origin,transform_matrix,intensity") and len(lines) == 1 + len(table.rays)


def test_sorted_spatially_is_a_pure_reordering():
    """RayBatch.sorted_spatially: tracing the sorted batch gives, ray for ray, the bits of tracing the original."""
    import torch
    import optable_amd as oa

    comps, gen, n, K = CASES["cfg3"]
    n = 5000
    table = support.table_of(comps(oa))
    o, d = gen(n)
    batch = _batch(o, d)
    ordered, order = batch.sorted_spatially()
    assert torch.equal(torch.sort(order).values, torch.arange(n, device=order.device))
    a = table.trace_batch(batch, max_segments=K, layout="slots")
    b = table.trace_batch(ordered, max_segments=K, layout="slots")
    assert torch.equal(a.count[order], b.count)
    for f in abi.SEG_FIELDS + ("surface",):
        x, y = a.field(f).reshape(K, n)[:, order], b.field(f).reshape(K, n)
        valid = torch.arange(K, device=x.device)[:, None] < b.count[None, :]
        assert torch.equal(x[valid], y[valid]), f


@pytest.mark.parametrize("branching", [False, True])
def test_batch_limited_scene_with_shared_ids(branching, oracle):
    """`max_interact_count` surfaces + rays that share an id (three wavelength copies of every ray, as
    multiplex_rays_in_wavelength makes them, ray.py:441-444): the copies must consume the SAME counters in
    input order (optical_component.py:140-149).  trace_batch runs them in rounds over one device table; the
    oracle traces the rays one after the other like the reference."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    rng = np.random.default_rng(77)
    comps = [oa.Mirror([-2, 0, 0], radius=3),
             oa.Mirror([6, 0, 0], radius=3, max_interact_count=2).RotZ(np.pi),      # opens after two hits per id
             oa.TriangularPrism([10, 0.3, 0], width=1.5, height=2, n1=1, n2=1.5),   # faces 2/3 limited to 5 by default
             oa.Mirror([14, 0, 0], radius=3, max_interact_count=1).RotZ(np.pi)]
    if branching:
        comps.append(oa.BeamSplitter([3, 0, 0], width=4, height=4, eta=0.5).RotZ(0.3))
    table = support.table_of(comps)
    scene = table.compile()
    assert len(scene.limited) >= 3 and scene.max_children == (2 if branching else 1)
    nb, K = 400, 14
    o = np.stack([np.zeros(nb), rng.uniform(-1, 1, nb), rng.uniform(-0.2, 0.2, nb)], 1)
    d = np.stack([np.ones(nb), rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.01, 0.01, nb)], 1)
    ids = 1000 + 7 * rng.permutation(nb)               # arbitrary, unordered, not 0..n-1
    base = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q, ids=ids)
    batch = base.multiplexed_in_wavelength([780e-7, 560e-7, 400e-7])
    segs = table.trace_batch(batch, max_segments=K, layout="slots")
    got = segs.to_host(reference_order=True)
    host = batch.to_host()
    uniq, inverse = np.unique(host["id"], return_inverse=True)
    np.testing.assert_array_equal(segs.count_ids.cpu().numpy(), uniq)
    host["id"] = inverse.astype(np.int32)
    ref = oracle.trace(scene, host, max_trace_num=K, n_classes=len(uniq))
    np.testing.assert_array_equal(got["ray"], ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    np.testing.assert_array_equal(segs.counts_table.cpu().numpy(), ref["counts"])
    # the gates really acted: the second and third copies of a ray do not repeat the first copy's path
    first, third = got["surface"][got["ray"] < nb], got["surface"][got["ray"] >= 2 * nb]
    assert len(first) != len(third) or not np.array_equal(first, third)


def test_fp32_ray_trees_track_fp64():
    """The generational path in single precision (`ot_trace_generation_f32`): same trees, same order; positions
    within 2e-4 of the fp64 trace over ten generations (float epsilon x path length x a few bounces)."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    table = support.table_of([oa.BeamSplitter([3, 0, 0], width=3, height=3, eta=0.4).RotZ(0.3), oa.Mirror([6, 0, 0], radius=2).RotZ(np.pi),
                    oa.GlassSlab([-2, 0, 0], width=3, height=3, thickness=0.4, n1=1, n2=1.5, reflectivity=0.2).RotZ(0.1)])
    o, d = scenes.cfg2_rays(2000, 3)
    q = support.Q
    s32 = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision="f32"), max_segments=10, layout="slots")
    s64 = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision="f64"), max_segments=10, layout="slots")
    assert s32.precision == "f32" and s64.precision == "f64"
    a, b = s32.to_host(), s64.to_host()
    n = 2000
    seq = lambda x: [tuple(x["surface"][x["ray"] == i].tolist()) for i in range(n)]
    same = np.array([u == v for u, v in zip(seq(a), seq(b))])
    assert same.mean() > 0.995, same.mean()            # a ray grazing an edge may fall on the other side in float
    assert_explained(audit_traces(table.compile(), s64.to_host(reference_order=True), s32.to_host(reference_order=True), prec="f32",
                                  tol=2e-4, rays=RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, device="cpu").to_host()))
    ka, kb = same[a["ray"]], same[b["ray"]]
    for f in ("ox", "oy", "oz", "dx", "dy", "dz", "intensity"):
        assert np.abs(a[f][ka].astype(np.float64) - b[f][kb]).max() < 2e-4, f
    mon = oa.Monitor([1, 0, 0], 6, 6)
    h32, h64 = table.record_batch(mon, s32), table.record_batch(mon, s64)     # monitor pass widens fp32 segments
    assert abs(len(h32) - len(h64)) <= 0.005 * len(h64) + 2


def test_compiled_scene_can_be_reused_and_is_not_uploaded_twice():
    """trace_batch(scene=...) skips the Python flattening; the engine skips the upload of the scene it already
    holds; a component moved afterwards needs a fresh compile (poses are read at compile time)."""
    import torch
    import optable_amd as oa
    from optable_amd.engine import get_engine

    comps = scenes.cfg2_components(oa)
    table = support.table_of(comps)
    o, d = scenes.cfg2_rays(2000, 1)
    batch = _batch(o, d)
    scene = table.compile()
    a = table.trace_batch(batch, max_segments=5, scene=scene, layout="slots")
    assert get_engine().scene is scene
    b = table.trace_batch(batch, max_segments=5, scene=scene, layout="slots")
    fresh = table.trace_batch(batch, max_segments=5, layout="slots")
    for f in abi.SEG_FIELDS:
        assert torch.equal(a.field(f), b.field(f)) and torch.equal(a.field(f), fresh.field(f))
    comps[0]._Translate([0.5, 0, 0])                       # move the lens
    stale = table.trace_batch(batch, max_segments=5, scene=scene, layout="slots")
    moved = table.trace_batch(batch, max_segments=5, layout="slots")
    assert torch.equal(stale.field("length"), a.field("length"))
    assert not torch.equal(moved.field("length"), a.field("length"))


def _g20():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g20_interact.npz"))


def test_single_call_api_matches_reference_fixture():
    """`component.interact(ray)` and `leaf.intersect_point_local(...)` — the per-object form of the hot path
     — against outputs of the reference's own methods (tools/make_golden.py g20)."""
    import optable_amd as oa

    g = _g20()
    for name, comp, rays in scenes.interact_cases(oa):
        t_ref = g[f"{name}_t"]
        owner = g[f"{name}_out_owner"]
        rows = 0
        for k, ray in enumerate(rays):
            t, out = comp.interact(ray)
            if np.isnan(t_ref[k]):
                assert t is None and out is None, (name, k)
                continue
            assert t == pytest.approx(t_ref[k], rel=1e-9, abs=1e-9), (name, k)
            sel = np.nonzero(owner == k)[0]
            assert len(out) == len(sel), (name, k, len(out), len(sel))
            for r, j in zip(out, sel):
                np.testing.assert_allclose(r.origin, g[f"{name}_out_origin"][j], atol=1e-9, err_msg=f"{name} {k}")
                np.testing.assert_allclose(r.direction, g[f"{name}_out_direction"][j], atol=1e-9, err_msg=f"{name} {k}")
                assert r.intensity == pytest.approx(g[f"{name}_out_intensity"][j], rel=1e-12, abs=1e-15)
                assert bool(r.alive) == bool(g[f"{name}_out_alive"][j])
                ref_len = g[f"{name}_out_length"][j]
                assert (r.length is None) == bool(np.isinf(ref_len))
                if r.length is not None:
                    assert r.length == pytest.approx(ref_len, rel=1e-9)
                assert r.n == pytest.approx(g[f"{name}_out_n"][j], rel=1e-12)
                assert r._pathlength == pytest.approx(g[f"{name}_out_pathlength"][j], rel=1e-9, abs=1e-9)
                qtol = 2e-3 if "asphere" in name else 1e-9
                assert complex(r.qo) == pytest.approx(complex(g[f"{name}_out_q"][j]), rel=qtol, abs=1e-9)
                rows += 1
            if f"{name}_local_t" in g.files:
                P, tl = comp.intersect_point_local(comp.ray_to_local_coordinates(ray))
                assert tl == pytest.approx(g[f"{name}_local_t"][k], rel=1e-9, abs=1e-9)
                np.testing.assert_allclose(P, g[f"{name}_local_P"][k], atol=1e-9)
        assert rows > 0, name
    # a miss in the local API, and the counters of the limited prism faces
    leaf = oa.Mirror([2, 0, 0], radius=1.0)
    assert leaf.intersect_point_local(oa.Ray([-3, 5, 0], [1, 0, 0])) == (None, None)


def test_monitor_analysis_helpers():
    """get_delta_pos / std_histy / get_beam_waist (monitor.py:218-253) on hits recorded by the device pass."""
    table, sc = helpers.build("g06_mirror_pair")
    table.ray_tracing(sc["rays"])
    mon = table.monitors[0]
    assert mon.ndata >= 1
    dy, dz = mon.get_delta_pos()
    assert len(dy) == max(mon.ndata - 1, 0) or (mon.ndata == 0 and len(dy) == 1)
    assert np.isfinite(mon.std_histy)
    import optable_amd as oa
    t = oa.OpticalTable()
    m = oa.Monitor([3, 0, 0], 2, 2)
    t.add_monitors(m)
    t.ray_tracing([oa.Ray([0, 0.1 * k, 0], [1, 0, 0], wavelength=780e-7, w0=50e-4) for k in range(4)])
    w = m.get_beam_waist()
    assert w.shape == (4,) and np.allclose(w, 50e-4)       # free propagation keeps the waist
    assert np.allclose(np.sort(m.get_delta_pos()[0]), 0.1)


def test_interact_local_is_the_lab_interaction_seen_from_the_leaf():
    """leaf.interact_local(ray_local) == children of leaf.interact(ray) mapped into the leaf's frame."""
    import optable_amd as oa

    for name, comp, rays in scenes.interact_cases(oa):
        if hasattr(comp, "components"):
            with pytest.raises(NotImplementedError):
                comp.interact_local(rays[0])
            continue
        for ray in rays[:3]:
            t, out = comp.interact(ray)
            local = comp.interact_local(comp.ray_to_local_coordinates(ray))
            if t is None:
                assert local == []
                continue
            assert len(local) == len(out) - 1
            for a, b in zip(local, out[1:]):
                back = comp.ray_to_lab_coordinates(a)
                np.testing.assert_allclose(back.origin, b.origin, atol=1e-9)
                np.testing.assert_allclose(back.direction, b.direction, atol=1e-9)
                assert a.intensity == pytest.approx(b.intensity)
    with pytest.raises(NotImplementedError):
        oa.OpticalComponent([0, 0, 0]).interact_local(oa.Ray([-1, 0, 0], [1, 0, 0]))


@pytest.mark.parametrize("many", [False, True])
def test_exact_ties_go_to_the_first_component(many, oracle):
    """Two surfaces at exactly the same distance: OpticalTable keeps the first in list order (strict `t < t_min`,
    optical_table.py:119-123) and a ComponentGroup the first minimum (np.argmin, component_group.py:118-120).
    Checked on the plain pass and, with 14 more components, on the top-level grid (ties go to the lower node
    index there too), against the oracle and against the explicit expectation."""
    import optable_amd as oa

    near_a = oa.Mirror([3, 0, 0], radius=1.0, reflectivity=0.25)          # same plane x = 3, same aperture
    near_b = oa.Mirror([3, 0, 0], radius=1.0, reflectivity=0.75)
    pair = oa.ComponentGroup([6, 0, 0])                                    # a group whose two children coincide
    pair.add_component(oa.Lens([6, 0, 0], focal_length=4.0, radius=1.0))
    pair.add_component(oa.Mirror([6, 0, 0], radius=1.0))
    comps = [oa.Mirror([-2, 0, 0], radius=2.0).RotZ(np.pi), near_a, near_b, pair]
    if many:
        comps += [oa.Block([10 + k, 5 + (k % 3), 0], width=0.5, height=0.5) for k in range(14)]
    table = support.table_of(comps)
    scene = table.compile()
    assert (scene.root_grid >= 0) == many
    o = np.tile([[0.0, 0.0, 0.0]], (64, 1)) + np.linspace(-0.3, 0.3, 64)[:, None] * np.array([[0, 1, 0]])
    d = np.tile([[1.0, 0.0, 0.0]], (64, 1))
    batch = _batch(o, d)
    got = table.trace_batch(batch, max_segments=4, layout="slots").to_host(reference_order=True)
    ref = oracle.trace(scene, batch.to_host(), max_trace_num=4)
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-12, atol=1e-12, err_msg=f)
    first = got["surface"].reshape(64, -1)[:, 0]
    assert (first == 1).all()                                               # near_a (leaf 1), never near_b (leaf 2)
    second_intensity = got["intensity"].reshape(64, -1)[:, 1]
    np.testing.assert_allclose(second_intensity, 0.25)                      # reflected by near_a


def test_group_tie_keeps_the_first_child(oracle):
    import optable_amd as oa

    pair = oa.ComponentGroup([6, 0, 0])
    pair.add_component(oa.Lens([6, 0, 0], focal_length=4.0, radius=1.0))
    pair.add_component(oa.Mirror([6, 0, 0], radius=1.0))
    table = support.table_of([pair])
    o, d = np.array([[0.0, 0.2, 0.0]]), np.array([[1.0, 0.0, 0.0]])
    got = table.trace_batch(_batch(o, d), max_segments=3, layout="slots").to_host()
    ref = oracle.trace(table.compile(), _batch(o, d).to_host(), max_trace_num=3)
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    assert got["surface"][0] == 0 and got["dx"][1] > 0                      # the lens won: the ray goes on, bent


def test_axis_parallel_rays_and_flat_boxes_match_oracle(oracle):
    """The slab test's special cases on the device (solver.py:27-33, :46): direction components that are exactly
    zero or below np.isclose's 1e-8 (axis treated as parallel: miss iff the origin lies outside the slab), rays
    that start ON a box face, and the zero-thickness AABBs every axis-aligned planar leaf of a group has."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    comps = [oa.GlassSlab([4, 0, 0], width=2, height=2, thickness=0.5, n1=1, n2=1.5),             # axis-aligned: flat child boxes
             oa.MirrorPair([9, 0, 0], 4, 4),
             oa.GlassSlab([4, 3, 0], width=2, height=2, thickness=0.5, n1=1, n2=1.5).RotZ(np.pi / 2),  # faces normal to y
             oa.Prism([-4, 0, 0], width=1.5, height=2, n1=1, n2=1.5).RotZ(np.pi)]
    table = support.table_of(comps)
    rng = np.random.default_rng(8)
    n = 4000
    o = np.stack([rng.uniform(-6, 12, n), rng.uniform(-2, 5, n), rng.uniform(-1.2, 1.2, n)], 1)
    d = rng.normal(size=(n, 3))
    d[0::5] = [1.0, 0.0, 0.0]                  # exactly along x
    d[1::5, 2] = 0.0                            # in the z = const plane
    d[2::10] = [0.0, 1.0, 0.0]                  # exactly along y: parallel to the first slab's faces
    d[3::10, 1] = 1e-9                          # below isclose's threshold: treated as parallel
    d[4::10, 2] = -5e-9
    o[0::20, 0] = 3.75                          # start exactly on the slab's front face plane
    o[5::20, 1] = 1.0                           # ... on its side plane (y = +1 edge of the 2 x 2 aperture)
    o[10::20, 2] = 1.0                          # ... on the top edge plane
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q, normalize=False)
    got = table.trace_batch(batch, max_segments=10, layout="slots").to_host(reference_order=True)
    ref = oracle.trace(table.compile(), batch.to_host(), max_trace_num=10)
    seq = lambda x: [tuple(x["surface"][x["ray"] == i].tolist()) for i in range(n)]
    same = np.array([a == b for a, b in zip(seq(got), seq(ref))])
    assert (~same).sum() <= 2, f"{(~same).sum()} rays took a different path"   # edge-grazing rounding only
    kg, kr = same[got["ray"]], same[ref["ray"]]
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f][kg], ref[f][kr], rtol=1e-9, atol=1e-9, err_msg=f)
    hit_any = np.array([len(s) > 1 for s in seq(ref)])
    assert hit_any[0::5].sum() > 50 and hit_any[2::10].sum() > 10              # the special rays do reach things


def test_two_threads_sharing_the_engine_do_not_interleave():
    """An ot_ctx holds ONE scene: two Python threads tracing different tables through the shared engine must each
    get the result of their own scene (the table entry points hold the engine lock over upload + trace)."""
    import threading
    import torch
    import optable_amd as oa

    o, d = scenes.cfg2_rays(20000, 4)
    tables = [support.table_of(scenes.cfg2_components(oa)), support.table_of([oa.Mirror([3, 0, 0], radius=2.0).RotZ(np.pi)])]
    expect = [t.trace_batch(_batch(o, d), max_segments=5, layout="slots").count.clone() for t in tables]
    assert not torch.equal(expect[0], expect[1])
    errors = []

    def work(k):
        try:
            for _ in range(30):
                got = tables[k].trace_batch(_batch(o, d), max_segments=5, layout="slots").count
                if not torch.equal(got, expect[k]):
                    errors.append(k)
        except Exception as exc:  # noqa: BLE001
            errors.append(repr(exc))

    threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_streamed_host_api_equals_the_resident_batch(precision):
    """trace_host (chunks on two HIP streams, pinned staging, overlapped copies) returns what trace_batch + to_host
    return for the same rays, for chunk sizes that do and do not divide the batch.  It normalises the directions on
    the device (torch) where from_arrays does it on the host (numpy): inputs agree to one ulp, results to ~1e-13
    relative in fp64 / 1e-5 in fp32 after five segments."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch
    from optable_amd import dist as odist

    n, K = 50_000, 5
    table = support.table_of(scenes.cfg2_components(oa))
    o, d = scenes.cfg2_rays(n, 2)
    q = support.Q
    segs = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision=precision), max_segments=K, layout="slots")
    final = odist.final_state(segs).cpu().numpy()
    tol = 1e-11 if precision == "f64" else 2e-4
    for chunk in (n, 16384, 7001):
        got = table.trace_host(o, d, wavelength=scenes.WL, q=q, max_segments=K, chunk=chunk, history=True, precision=precision)
        np.testing.assert_array_equal(got["count"], segs.count.cpu().numpy())
        for k, f in enumerate(odist.FINAL_FIELDS):
            np.testing.assert_allclose(got["final"][f], final[k], rtol=tol, atol=tol, err_msg=f)
        valid = np.arange(K)[:, None] < got["count"][None, :]     # unused slots are uninitialised memory on both sides
        for f in abi.SEG_FIELDS:
            np.testing.assert_allclose(got[f][valid], segs.field(f).view(K, n).cpu().numpy()[valid], rtol=tol, atol=tol, err_msg=f)
        np.testing.assert_array_equal(got["surface"][valid], segs.surface.view(K, n).cpu().numpy()[valid])
    # chunking itself changes nothing: two chunkings of the streamed path agree bit for bit
    a = table.trace_host(o, d, wavelength=scenes.WL, q=q, max_segments=K, chunk=n, precision=precision)
    b = table.trace_host(o, d, wavelength=scenes.WL, q=q, max_segments=K, chunk=7001, precision=precision)
    for f in odist.FINAL_FIELDS:
        np.testing.assert_array_equal(a["final"][f], b["final"][f], err_msg=f)
    with pytest.raises(NotImplementedError):
        support.table_of([oa.BeamSplitter([3, 0, 0], width=3, height=3)]).trace_host(o[:10], d[:10], max_segments=3)


def test_large_image_with_every_feature_reads_the_scene_from_l2(oracle):
    """A scene whose fp64 image exceeds 64 KB AND needs the all-features kernel (a cylinder next to cfg 5's
    micro-mirror array): that instantiation is limited to 256-thread workgroups, so the image stays in global
    memory (the 512-thread LDS mode does not apply) — the one combination no other test reaches."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    comps = scenes.cfg5_components(oa) + [oa.CylMirror([8, 3.5, 0], radius=1.2, height=2.0, theta_range=(np.pi / 2, np.pi)).RotZ(0.4)]
    table = support.table_of(comps)
    scene = table.compile()
    assert scene.n_nodes > 200
    n, K = 3000, 30
    o, d = scenes.cfg5_rays(n, 5)
    d = d + np.array([0.0, 0.02, 0.0]) * np.linspace(-1, 1, n)[:, None]      # fan out so that some rays reach the cylinder
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q)
    got = table.trace_batch(batch, max_segments=K, layout="slots").to_host(reference_order=True)
    ref = oracle.trace(scene, batch.to_host(), max_trace_num=K)
    np.testing.assert_array_equal(got["ray"], ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        tol = 2e-3 if f in ("q_re", "q_im") else 1e-9
        np.testing.assert_allclose(got[f], ref[f], rtol=tol, atol=max(tol, 1e-9), err_msg=f)
    cyl_leaf = scene.n_leaves - 1
    s32 = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=1j, precision="f32"), max_segments=K, layout="slots")
    assert int((s32.count > 0).sum()) == n and (got["surface"] == cyl_leaf).sum() >= 0


def test_very_large_scene_image(oracle):
    """A 24x24 micro-mirror array: 580 nodes, 213 KB in fp64 (read from L2), 121 KB in fp32 (the 512-thread LDS
    mode).  Both against the oracle's surface sequences; fp64 field by field."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    comps = scenes.cfg5_components(oa, N=(24, 24))
    table = support.table_of(comps)
    scene = table.compile()
    assert scene.n_nodes > 570
    n, K = 4000, 24
    rng = np.random.default_rng(11)
    o = np.stack([np.zeros(n), rng.uniform(-2.2, 2.2, n), rng.uniform(-2.2, 2.2, n)], 1)
    d = np.tile([[1.0, 0.0, 0.0]], (n, 1))
    q = support.Q
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q)
    got = table.trace_batch(batch, max_segments=K, layout="slots").to_host(reference_order=True)
    ref = oracle.trace(scene, batch.to_host(), max_trace_num=K)
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        tol = 2e-3 if f in ("q_re", "q_im") else 1e-9
        np.testing.assert_allclose(got[f], ref[f], rtol=tol, atol=max(tol, 1e-9), err_msg=f)
    g32 = table.trace_batch(RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=q, precision="f32"), max_segments=K, layout="slots").to_host(reference_order=True)
    seq = lambda x: [tuple(x["surface"][x["ray"] == i].tolist()) for i in range(n)]
    same = np.array([a == b for a, b in zip(seq(g32), seq(ref))])
    assert same.mean() > 0.9, same.mean()
    assert_explained(audit_traces(scene, ref, g32, prec="f32", tol=2e-3, rays=batch.to_host()))


@pytest.mark.filterwarnings("ignore:Maximum number of iterations")  # the 50-iteration cap is upstream's own setting
@pytest.mark.parametrize("criterion,key", [("min_stdtY", "opt_min_stdtY"), ("M=-I", "opt_MmI")])
def test_calibrate_symmetric_4f_reaches_the_reference_optimum(criterion, key, capsys):
    """calibrate_symmetric_4f (optical_table.py:299-422): 50 Nelder-Mead iterations, every cost evaluation one
    ray_tracing + one calculate_abcd_matrix on the device.  The cost surfaces have flat directions (F1 barely
    matters), so the simplex path is not reproducible digit for digit; what must hold is that the optimum found
    here is as good as the reference's (fixture g22), judged by the same cost evaluated at both points."""
    import optable_amd as oa

    ref_opt = np.load(os.path.join(os.path.dirname(__file__), "golden", "g22_calibrate.npz"))[key]
    sc = scenes.calibrate_case(oa)
    F1, F2 = oa.OpticalTable.calibrate_symmetric_4f(sc["lens"], sc["rays"], sc["F10"], sc["F20"], criterion=criterion)
    capsys.readouterr()

    def cost(f1, f2):
        Ms, _, ty = oa.OpticalTable.calibrate_symmetric_4f(sc["lens"], sc["rays"], f1, f2, criterion=criterion, optimize=False)
        if criterion == "M=-I":
            return float(np.mean([np.linalg.norm(M + np.eye(2)) for M in Ms]))
        return float(np.std(ty))

    mine, theirs, start = cost(F1, F2), cost(*ref_opt), cost(sc["F10"], sc["F20"])
    assert mine <= start                                       # the optimiser did not make things worse
    assert mine <= theirs * 1.05 + 1e-9, (mine, theirs, (F1, F2), ref_opt.tolist())
    if criterion == "min_stdtY":
        assert F2 == pytest.approx(ref_opt[1], abs=2e-3)       # the direction the cost does depend on


def test_monitor_export_rays_npz(tmp_path, capsys):
    """f4: Monitor.export_rays_npz (monitor.py:255-269) writes the sorted hit lists under the reference's key names."""
    table, sc = helpers.build("g06_mirror_pair")
    table.ray_tracing(sc["rays"])
    mon = next(m for m in table.monitors if m.ndata)
    path = tmp_path / "hits.npz"
    mon.export_rays_npz(str(path))
    capsys.readouterr()
    data = np.load(path)
    assert sorted(data.files) == ["IList", "tXList", "tYList", "xList", "yList"]
    np.testing.assert_array_equal(data["xList"], mon.yList)      # upstream names the monitor's Y axis "x" in the file
    np.testing.assert_array_equal(data["yList"], mon.zList)
    np.testing.assert_array_equal(data["tXList"], mon.tYList)
    np.testing.assert_array_equal(data["IList"], mon.IList)


@pytest.mark.parametrize("kernel", [1, 2])
def test_stale_cached_boxes_gate_but_never_prune(kernel, oracle):
    """A component moved AFTER a first trace keeps its cached bounding boxes (optical_component.py:62-67,
    component_group.py:29-38: never invalidated).  The reference goes on using the stale box as a pass / fail gate, and
    the true geometry can then lie in front of it: a MirrorPair pulled towards the source is hit BEFORE the lens that
    stands between the pair's new place and its old box.  The kernels must not skip the pair because its box starts
    behind the lens (nearer-hit pruning assumed every hit lies inside its box)."""
    import optable_amd as oa
    from optable_amd.engine import get_engine

    lens = oa.Lens([7, 0, 0], focal_length=6, radius=1.5)
    pair = oa.MirrorPair([10, 0, 0], 4, 4)
    table = support.table_of([lens, pair])
    o, d = scenes.cfg2_rays(4000, 0)
    d = np.stack([np.ones(len(d)), 0.3 * d[:, 1], 0.3 * d[:, 2]], 1)
    batch = _batch(o, d)
    eng = get_engine()
    eng.set_option(abi.OPT_KERNEL, kernel)
    try:
        first = table.trace_batch(batch, max_segments=6, layout="slots").to_host(reference_order=True)  # caches every box
        ref0 = oracle.trace(table.compile(), batch.to_host(), max_trace_num=6)
        np.testing.assert_array_equal(first["surface"], ref0["surface"])
        pair._Translate([-5.0, 0.0, 0.0])  # the group and its mirrors move; their cached boxes stay at x ~ 10
        scene = table.compile()
        nodes = scene.node_table()
        assert not all(nodes["flags"] & abi.NODE_BOX_TRUSTED)
        got = table.trace_batch(batch, max_segments=6, layout="slots").to_host(reference_order=True)
        ref = oracle.trace(scene, batch.to_host(), max_trace_num=6)
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)
    assert len(got["ray"]) == len(ref["ray"])
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    # the scenario is real: most first segments now end on the moved pair (x ~ 5), in front of the lens at x = 7
    first_seg = np.r_[True, np.diff(ref["ray"]) != 0]
    assert (ref["length"][first_seg] < 6.5).mean() > 0.5


@pytest.mark.parametrize("shape", ["sphere", "paraboloid"])
def test_repeated_hits_on_one_curved_surface(shape, oracle):
    """A ray that leaves a curved surface can meet THE SAME surface again (whispering-gallery reflections along a concave
    spherical cap; two reflections inside a deep paraboloid).  The root at the start point is thrown away, the next
    one is a hit — in double precision against the oracle, and in single precision too, where the start point can lie
    1e-5 off the surface (the start-point bracket must not swallow a genuine second crossing)."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    n = 2000
    rng = np.random.default_rng(21)
    if shape == "sphere":
        comp = oa.SphereRefractive([0, 0, 0], radius=5.0, height=2.0, n1=1.0, n2=1.0, reflectivity=1.0, transmission=0.0)
        th = np.deg2rad(rng.uniform(-45, -30, n))
        rad = rng.uniform(4.6, 4.95, n)
        delta = rng.uniform(0.08, 0.3, n)            # angle between the ray and the tangent: chords of 0.8 .. 3
        o = np.stack([rad * np.cos(th), rad * np.sin(th), rng.uniform(-0.2, 0.2, n)], 1)
        d = np.stack([-np.sin(th - delta), np.cos(th - delta), np.zeros(n)], 1)
        K, min_repeats = 12, 3
    else:
        comp = oa.BaseRefraciveSurface(origin=[0, 0, 0], n1=1.0, n2=1.0, surface=oa.ASphere(3.0, oa.sag_parametric(1.0, -1.0)),
                                       reflectivity=1.0, transmission=0.0)
        yz = rng.uniform(-2.2, 2.2, (n, 2))
        o = np.stack([np.full(n, -6.0), yz[:, 0], yz[:, 1]], 1)       # inside the bowl x = -r^2 / 2, travelling towards its bottom
        d = np.tile([1.0, 0.0, 0.0], (n, 1))
        K, min_repeats = 6, 2
    table = support.table_of([comp])
    out = {}
    for prec in ("f64", "f32"):
        b = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q, precision=prec)
        out[prec] = table.trace_batch(b, max_segments=K, layout="slots")
    got = out["f64"].to_host(reference_order=True)
    host = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q, device="cpu").to_host()
    ref = oracle.trace(table.compile(), host, max_trace_num=K)
    np.testing.assert_array_equal(got["surface"], ref["surface"])
    for f in ("ox", "oy", "oz", "dx", "dy", "dz", "length"):
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    c64, c32 = out["f64"].count.cpu().numpy(), out["f32"].count.cpu().numpy()
    assert np.median(c64) > min_repeats            # the rays really do come back to the surface they left
    assert (c64 == c32).mean() >= 0.99, (c64 == c32).mean()
    assert_explained(audit_traces(table.compile(), got, out["f32"].to_host(reference_order=True), prec="f32", tol=2e-3, rays=host))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_generation_emit_pass_reuses_the_count_pass_decision(prec):
    """Heavy branching scenes: the emit pass rebuilds the hit the count pass found (node + distance kept per ray) instead
    of searching the scene again (OT_OPT_GEN_REUSE).  Same trees, bit for bit, as with two searches; no mismatches."""
    import optable_amd as oa
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    n, cap = 20000, 20
    table = support.table_of(W.cfg3_components(oa, slab_reflectivity=0.1))
    o, d = scenes.cfg3_rays(n, 2)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q, precision=prec)
    eng = get_engine()
    got = {}
    for reuse in (0, 1):
        eng.set_option(abi.OPT_GEN_REUSE, reuse)
        try:
            got[reuse] = table.trace_batch(batch, max_segments=cap, layout="slots").to_host(reference_order=True)
        finally:
            eng.set_option(abi.OPT_GEN_REUSE, -1)
    assert len(got[0]["ray"]) > 3 * n  # the trees do branch
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        np.testing.assert_array_equal(got[0][f], got[1][f], err_msg=f)
    assert eng.generation_mismatches() == 0
