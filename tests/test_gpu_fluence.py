"""GPU (MI355X): fluence maps — `OpticalTable.fluence_map`, every segment of a SegmentBatch rasterised into a projected view of the
table by k_seg_raster (ot_fluence_map).

Reference, in every comparison: tests/fluence_reference.py (plain numpy, checked against closed forms in tests/test_fluence_cpu.py)
run on the SAME segment records, copied from the device — only the rasteriser is under test.
Counts must be EQUAL, and so must `skipped`.  The fluence of a pixel must agree within
    sum over its pieces of |I| 64 U t_b  +  2 c U sum |I| l          (U = 2^-53, c = the pixel's count)
— derived, not measured: every crossing parameter is (e - o) / dh with e and o exact doubles; the subtraction, the division and
the renormalised dh (three products, two sums, a square root, a reciprocal, a product) give at most 16 U relative error a side, a
piece has two ends, and the two sides are kernel and reference; the second term is the bound of tests/test_gpu_image.py for two
summation orders.  Kernel and reference may round a crossing parameter differently, so every comparison on traced data first
asserts, from the REFERENCE's values, that every positive piece is longer than 1e-9 — some five orders of magnitude above the bound
at table scale, so no piece can change pixel or vanish.  The ROIs' grid lines avoid the scenes' symmetry planes (v from -3.01 to
2.97, not -3 to 3); the CPU oracle's cfg 2 segments give a shortest piece of 6.5e-8 over the views and shapes below.
The pixel rule itself is checked on exact coordinates, lines and their neighbouring doubles included, with no such condition."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from fluence_reference import fluence_reference
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import fluence_plan, get_engine, segment_source
from optable_amd.fluence import fluence_view
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROI = (-1.03, 12.9, -3.01, 2.97, -2.83, 3.07)  # cfg 2: source at the origin, lens at x = 5, mirror pair at x = 10; finite depth in every view


def _reference(records, view, roi, pixels, weight="intensity"):
    o, d, length, intensity = records
    axes, ue, ve, depth, _ = fluence_view(view, roi, pixels)
    return fluence_reference(o, d, length, intensity if weight == "intensity" else None, axes, ue, ve, *depth)


def _assert_map(fm, ref, traced=True):
    counts, fluence, ue, ve = fm.to_host()
    assert counts.dtype == np.int64 and fluence.dtype == np.float64 and counts.shape == fluence.shape == fm.pixels == (len(ue) - 1, len(ve) - 1)
    if traced and len(ref.pieces):
        print(f"  {len(ref.pieces)} pieces, the shortest {ref.pieces.min():.3g}")
        assert ref.pieces.min() > 1e-9  # a condition on the inputs
    np.testing.assert_array_equal(counts, ref.counts)
    assert fm.skipped == ref.skipped
    err = np.abs(fluence - ref.fluence)
    print(f"  {int(ref.counts.sum())} pieces in {int((ref.counts > 0).sum())} pixels, most in one {int(ref.counts.max())}; fluence: largest error "
          f"{err.max():.3g}, bound there {ref.bound.flat[np.argmax(err)]:.3g}")
    excess = err - ref.bound
    assert np.all(excess <= 0), float(excess.max())


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 5,003 rays, 5 segments: (table, {(layout, precision): (segs, records)}), traced on first use."""
    table = support.cfg2_table()
    o, d = scenes.cfg2_rays(5003, 0)
    return table, support.traced(table, lambda precision: support.weighted_batch(o, d, precision), 5, support.host_records)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_precisions_views(case1, layout, precision, monkeypatch):
    table, get = case1
    segs, records = get(layout, precision)
    assert 5003 * 5 - 10 <= len(records[2]) <= 5003 * 5 and fluence_plan(40, 30)["path"] == "lds"

    def refuse(self, *args, **kwargs):
        raise AssertionError("fluence_map converted the batch")

    for view in ("Z", "Y"):
        with monkeypatch.context() as mp:
            mp.setattr(SegmentBatch, "to_slots", refuse)
            mp.setattr(SegmentBatch, "astype", refuse)
            fm = table.fluence_map(segs, view=view, roi=ROI, pixels=(40, 30))
            plain = table.fluence_map(segs, view=view, roi=ROI, pixels=(40, 30), weight="none")
        assert fm.counts.is_cuda and fm.counts.dtype == torch.int64 and fm.fluence.dtype == torch.float64 and fm.view == view
        ref = _reference(records, view, ROI, (40, 30))
        _assert_map(fm, ref)
        assert int((ref.counts > 0).sum()) > 100 and len(ref.pieces) > 10 * len(records[2])  # a real walk: ten pixels a segment and more
        # conservation: with weight 1 the image sums to the clipped length of the segments, nothing twice on a grid line
        ref = _reference(records, view, ROI, (40, 30), weight="none")
        _assert_map(plain, ref)
        assert torch.equal(plain.counts, fm.counts)
        want = _clipped_length(records, view, ROI)
        got = float(plain.fluence.sum(dtype=torch.float64).item())
        print(f"  path length {got:.15g}, Liang-Barsky {want:.15g}, bound {ref.bound.sum():.3g}")
        assert abs(got - want) <= ref.bound.sum()


def _clipped_length(records, view, roi):
    """Summed Liang-Barsky length of the segments inside the box of the roi, with no grid: np.maximum / np.minimum over the slabs."""
    o, d, length, _ = records
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    t0, t1 = np.zeros(len(o)), length.copy()
    for k in range(3):
        lo, hi = roi[2 * k], roi[2 * k + 1]
        moving = d[:, k] != 0.0
        with np.errstate(all="ignore"):
            a, b = (lo - o[:, k]) / d[:, k], (hi - o[:, k]) / d[:, k]
        t0 = np.where(moving, np.maximum(t0, np.minimum(a, b)), t0)
        t1 = np.where(moving, np.minimum(t1, np.maximum(a, b)), np.where((o[:, k] >= lo) & (o[:, k] <= hi), t1, -1.0))
    return float(np.clip(t1 - t0, 0.0, None).sum())


@pytest.mark.parametrize("pixels", [(96, 80), (7, 5), (30, 1), (1, 1)])
def test_shapes(case1, pixels):
    """(96, 80): 7,680 pixels, more than the LDS budget: global atomics.  (7, 5): a transposed or mis-strided image cannot pass.
    (30, 1): one row of pixels along v.  (1, 1): the box."""
    table, get = case1
    segs, records = get("slots", "f64")
    assert fluence_plan(*pixels)["path"] == ("global" if pixels == (96, 80) else "lds")
    for view in ("Z", "X"):
        fm = table.fluence_map(segs, view=view, roi=ROI, pixels=pixels)
        _assert_map(fm, _reference(records, view, ROI, pixels))
    if pixels == (30, 1):
        full = table.fluence_map(segs, view="X", roi=ROI, pixels=(30, 30), weight="none")
        one = table.fluence_map(segs, view="X", roi=ROI, pixels=(30, 1), weight="none")
        assert int(one.counts.sum()) < int(full.counts.sum())  # fewer lines, fewer pieces; the same length
        assert abs(float(one.fluence.sum()) - float(full.fluence.sum())) <= _reference(records, "X", ROI, (30, 30), "none").bound.sum()


# -- exact coordinates ----------------------------------------------------------------------------------------------------------
def _exact_segments():
    """Axis-parallel segments on the grid of the integer lines 0 .. 7 x 0 .. 5: along u and along v, both ways, at rest on every line
    of the other axis and on the doubles next to it, starting and ending on lines (1 -> 4) and inside pixels (0.5 -> 4.5; all
    lengths whole, all pieces multiples of 1 / 2), of no length, unbounded, along the depth, outside, and with a NaN origin."""
    ue, ve = np.arange(8.0), np.arange(6.0)
    o, d, length = [], [], []
    for rest, along, lines, reach in ((1, 0, support.around(ve), 7.0), (0, 1, support.around(ue), 5.0)):
        for x in lines:
            for start, sign, L in ((1.0, 1, 3.0), (4.0, -1, 3.0), (0.5, 1, 4.0), (4.5, -1, 4.0), (2.0, 1, 0.0), (0.5, 1, np.inf), (reach - 0.5, -1, np.inf),
                                   (-2.0, 1, 4.0), (reach, -1, 2.0), (0.0, 1, reach)):
                p, q = np.zeros(3), np.zeros(3)
                p[rest], p[along], q[along] = x, start, sign
                o.append(p), d.append(q), length.append(L)
    for p, q, L in (([0.5, 0.5, 0.0], [0, 0, 1], np.inf), ([6.5, 4.5, 0.5], [0, 0, -1], np.inf), ([3.5, 2.5, -3.0], [0, 0, 2], 3.0),  # along the depth
                    ([3.0, 2.0, 0.0], [0, 0, 1], 1.0),                                                                                  # ... on a corner
                    ([10.0, 10.0, 0.0], [1, 0, 0], 5.0), ([-4.0, 2.5, 0.0], [-1, 0, 0], np.inf), ([3.5, 2.5, 5.0], [1, 0, 0], 2.0),    # outside
                    ([np.nan, 2.5, 0.0], [1, 0, 0], 2.0), ([3.5, 2.5, 0.0], [0, 0, 0], 2.0), ([3.5, 2.5, 0.0], [1, 0, 0], np.nan)):    # no numbers
        o.append(np.array(p, dtype=float)), d.append(np.array(q, dtype=float)), length.append(L)
    return np.array(o), np.array(d), np.array(length)


def test_pixel_rule_on_exact_coordinates():
    """Counts, `skipped` and — with intensities of 0.5 and pieces that are multiples of 1 / 2 — the fluence itself equal the
    reference with NO precondition; inside a finite and inside an infinite depth range."""
    table = oa.OpticalTable()
    o, d, length = _exact_segments()
    segs = support.list_batch(o, d, length, np.full(len(o), 0.5))
    many = support.list_batch(np.tile(o, (7, 1)), np.tile(d, (7, 1)), np.tile(length, 7), np.full(7 * len(o), 0.5))
    assert 7 * len(o) > 2048  # more than one workgroup's slots
    for z1, skipped in ((1.0, 3), (np.inf, 4)):  # the NaN origin, the zero direction, the NaN length; and the ray leaving along z
        roi = (0.0, 7.0, 0.0, 5.0, -1.0, z1)
        fm = table.fluence_map(segs, view="Z", roi=roi, pixels=(7, 5))
        np.testing.assert_array_equal(fm.u_edges, np.arange(8.0))
        np.testing.assert_array_equal(fm.v_edges, np.arange(6.0))
        ref = _reference((o, d, length, np.full(len(o), 0.5)), "Z", roi, (7, 5))
        assert ref.skipped == skipped and ref.counts.sum() > 1000 and (ref.counts > 0).all()
        assert (ref.pieces * 2 == np.round(ref.pieces * 2)).all()
        assert torch.equal(fm.counts.cpu(), torch.from_numpy(ref.counts)) and fm.skipped == ref.skipped
        assert torch.equal(fm.fluence.cpu(), torch.from_numpy(ref.fluence))
        # a segment along a line lies in the upper pixel, the last one closed: row v = 5.0 went to pixel 4, v = 0.0 to pixel 0
        seven = table.fluence_map(many, view="Z", roi=roi, pixels=(7, 5))
        assert torch.equal(seven.counts, 7 * fm.counts) and torch.equal(seven.fluence, 7 * fm.fluence) and seven.skipped == 7 * skipped
    # the other precision and a view whose depth is x: the same rule on the same numbers
    single = support.list_batch(o, d, length, np.full(len(o), 0.5)).astype("f32")
    assert single.precision == "f32"
    roi = (0.0, 7.0, 0.0, 5.0, -1.0, 1.0)
    host = support.host_records(single)
    fm = table.fluence_map(single, view="Z", roi=roi, pixels=(7, 5))
    ref = _reference(host, "Z", roi, (7, 5))
    assert torch.equal(fm.counts.cpu(), torch.from_numpy(ref.counts)) and fm.skipped == ref.skipped == 3
    assert torch.equal(fm.fluence.cpu(), torch.from_numpy(ref.fluence))
    fm = table.fluence_map(segs, view="X", roi=(0.5, 6.5, 0.0, 5.0, -1.0, 1.0), pixels=(5, 2))
    ref = _reference((o, d, length, np.full(len(o), 0.5)), "X", (0.5, 6.5, 0.0, 5.0, -1.0, 1.0), (5, 2))
    assert torch.equal(fm.counts.cpu(), torch.from_numpy(ref.counts)) and fm.skipped == ref.skipped
    assert torch.equal(fm.fluence.cpu(), torch.from_numpy(ref.fluence))


def test_uneven_walks_in_one_wave():
    """512 x 512 pixels (global atomics): one segment along the whole image — 511 + 511 crossings, 1,023 pieces — among 255 that stay
    inside one pixel each."""
    rng = np.random.default_rng(3)
    n = 256
    corner = rng.integers(0, 512, (n, 2)).astype(float)
    o = np.concatenate([corner + rng.uniform(0.3, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, (n, 1))], axis=1)
    phi = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], axis=1)
    length = np.full(n, 0.2)
    o[77], d[77], length[77] = [0.25, 0.3, 0.0], [511.65, 510.9, 0.0], np.hypot(511.65, 510.9)
    intensity = 0.25 + 0.75 * rng.random(n)
    roi = (0.0, 512.0, 0.0, 512.0, -1.0, 1.0)
    assert fluence_plan(512, 512)["path"] == "global"
    fm = oa.OpticalTable().fluence_map(support.list_batch(o, d, length, intensity), view="Z", roi=roi, pixels=512)
    ref = _reference((o, d, length, intensity), "Z", roi, 512)
    assert len(ref.pieces) == 255 + 1023 and ref.skipped == 0
    _assert_map(fm, ref)


class _Maps(support.Sentinel):
    """counts / fluence / skipped of nu x nv pixels for ot_fluence_map, with a guard region on either side of each."""

    def __init__(self, nu, nv):
        super().__init__(guard=64, counts=(torch.int64, (nu, nv)), fluence=(torch.float64, (nu, nv)), skipped=(torch.int64, (1,)))

    def zero_(self):
        self.counts.zero_(), self.fluence.zero_(), self.skipped.zero_()
        return self


def _call(lib, ctx, segs, view, roi, pixels, out, accumulate=0):
    src, n, count, n_rays = segment_source(segs)
    axes, ue, ve, depth, _ = fluence_view(view, roi, pixels)
    dp = C.POINTER(C.c_double)
    return lib.ot_fluence_map(ctx, np.ascontiguousarray(axes).ctypes.data_as(dp), ue.ctypes.data_as(dp), len(ue) - 1, ve.ctypes.data_as(dp), len(ve) - 1,
                              depth[0], depth[1], C.byref(src), segs.field("intensity").data_ptr(), n, None if count is None else count.data_ptr(),
                              n_rays, out.counts.data_ptr(), out.fluence.data_ptr(), out.skipped.data_ptr(), accumulate)


def test_edges_of_the_partition():
    table, eng = support.cfg2_table(), get_engine()
    # one ray, one segment (origin -> lens)
    for layout in ("slots", "tiled", "append"):
        segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(1, 0)), max_segments=1, layout=layout)
        fm = table.fluence_map(segs, view="Z", roi=ROI, pixels=(40, 30))
        ref = _reference(support.host_records(segs), "Z", ROI, (40, 30))
        assert 10 < ref.counts.sum() < 60
        _assert_map(fm, ref)
    # slot counts of 64 k + 1: 65 slots, and 2,049 = one more than a workgroup's 2,048
    for n, K in ((13, 5), (2049, 1)):
        segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(n, 3)), max_segments=K, layout="slots")
        assert segment_source(segs)[1] % 64 == 1
        guarded = _Maps(40, 30).zero_()
        axes, ue, ve, depth, _ = fluence_view("Z", ROI, (40, 30))
        eng.fluence_map(axes, ue, ve, depth, segs, into=(guarded.counts, guarded.fluence, guarded.skipped))
        fm = table.fluence_map(segs, view="Z", roi=ROI, pixels=(40, 30))
        ref = _reference(support.host_records(segs), "Z", ROI, (40, 30))
        _assert_map(fm, ref)
        torch.cuda.synchronize()
        assert guarded.guards_untouched() and torch.equal(guarded.counts, fm.counts) and int(guarded.skipped.item()) == 0
        assert np.all(np.abs(guarded.fluence.cpu().numpy() - ref.fluence) <= ref.bound)
    # ... the same through global atomics, the guards around them
    guarded = _Maps(96, 80).zero_()
    axes, ue, ve, depth, _ = fluence_view("Z", ROI, (96, 80))
    eng.fluence_map(axes, ue, ve, depth, segs, into=(guarded.counts, guarded.fluence, guarded.skipped))
    torch.cuda.synchronize()
    ref = _reference(support.host_records(segs), "Z", ROI, (96, 80))
    assert ref.pieces.min() > 1e-9
    assert guarded.guards_untouched() and np.array_equal(guarded.counts.cpu().numpy(), ref.counts)
    assert np.all(np.abs(guarded.fluence.cpu().numpy() - ref.fluence) <= ref.bound)
    # a list of no segments: a zero map, and through the ABI n_segments = 0 zeroes a pre-filled map
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    fm = table.fluence_map(none, view="Y", roi=ROI, pixels=(7, 5))
    assert fm.pixels == (7, 5) and not fm.counts.any() and not fm.fluence.any() and fm.skipped == 0
    some = SegmentBatch(64, "f64", "cuda")
    some.n_valid = 0
    out = _Maps(7, 5)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, some, "Z", ROI, (7, 5), out) == 0
    torch.cuda.synchronize()
    assert not out.counts.any() and not out.fluence.any() and not out.skipped.any() and out.guards_untouched()
    kept = _Maps(7, 5)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, some, "Z", ROI, (7, 5), kept, accumulate=1) == 0  # ... and adds nothing to one it accumulates into
    torch.cuda.synchronize()
    assert kept.untouched()


def test_accumulation():
    """A map summed over the chunks of a trace: the two halves of a batch with `into=` against the whole batch in one call."""
    table = support.cfg2_table()
    o, d = scenes.cfg2_rays(2049, 3)
    whole = support.weighted_batch(o, d)
    segs = table.trace_batch(whole, max_segments=5, layout="slots")
    ref = _reference(support.host_records(segs), "Z", ROI, (40, 30))
    full = table.fluence_map(segs, view="Z", roi=ROI, pixels=(40, 30))
    _assert_map(full, ref)
    halves = []
    for part in (slice(0, 1024), slice(1024, 2049)):
        b = RayBatch.from_arrays(o[part], d[part], wavelength=scenes.WL, intensity=whole.intensity[part].cpu().numpy(),
                                 q=support.Q, device="cuda")
        halves.append(table.trace_batch(b, max_segments=5, layout="slots"))
    fm = table.fluence_map(halves[0], view="Z", roi=ROI, pixels=(40, 30))
    first = fm.counts.clone()
    assert table.fluence_map(halves[1], view="Z", roi=ROI, pixels=(40, 30), into=fm) is fm
    assert int(first.sum()) < int(fm.counts.sum()) and torch.equal(fm.counts, full.counts) and fm.skipped == 0
    assert np.all(np.abs(fm.fluence.cpu().numpy() - ref.fluence) <= ref.bound)
    # without `into=` a call starts from zero again
    assert torch.equal(table.fluence_map(halves[0], view="Z", roi=ROI, pixels=(40, 30)).counts, first)


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (tests/test_gpu_trees.py): the [k][tree] slots, the dense list with holes
    and the list in generation order."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    roi = (-3.53, 3.47, -3.01, 2.97, -1.03, 1.07)
    eng = get_engine()
    eng.upload(table.compile())
    assert eng.trees_plan("f64", 12)["slots"]
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        records = support.host_records(segs)
        assert len(records[2]) >= 3 * 320
        for view in ("Z", "X"):
            _assert_map(table.fluence_map(segs, view=view, roi=roi, pixels=(40, 30)), _reference(records, view, roi, (40, 30)))


def test_abi_errors(ctx):
    lib, c = ctx
    n, nu, nv = 130, 7, 5
    segs = SegmentBatch(2 * n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    segs.ox.fill_(0.5), segs.oy.fill_(0.5)
    segs.dx.fill_(1.0)
    segs.length.fill_(2.0)
    segs.intensity.fill_(0.5)
    segs.ray.copy_(torch.arange(2 * n, dtype=torch.int32) % n)
    segs.count, segs.n_rays = torch.full((n,), 2, dtype=torch.int32, device="cuda"), n
    out = _Maps(nu, nv)
    src, n_segments, count, n_rays = segment_source(segs)
    assert (n_segments, n_rays) == (2 * n, n)
    good_axes, good_u, good_v = np.eye(3), np.arange(nu + 1.0), np.arange(nv + 1.0)
    dp = C.POINTER(C.c_double)

    def call(ctx_=c, axes=good_axes, ue=good_u, u=nu, ve=good_v, v=nv, w_lo=-1.0, w_hi=1.0, source=src, intensity=segs.intensity.data_ptr(),
             n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(), fluence=out.fluence.data_ptr(),
             skipped=out.skipped.data_ptr(), acc=0):
        as_ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(dp)  # noqa: E731
        return lib.ot_fluence_map(ctx_, as_ptr(axes), as_ptr(ue), u, as_ptr(ve), v, w_lo, w_hi, None if source is None else C.byref(source), intensity,
                                  n_seg, cnt, rays, counts, fluence, skipped, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    def with_value(a, at, value):
        b = np.array(a, dtype=float)
        b.flat[at] = value
        return b

    for null in ("ctx_", "axes", "ue", "ve", "source", "counts", "fluence", "skipped"):
        expect(call(**{null: None}), "NULL")
    no_field = altered()
    no_field.base[3] = None
    expect(call(source=no_field), "NULL field")
    expect(call(source=altered(ray=None)), "NULL field")
    expect(call(u=0), "nu and nv")
    expect(call(v=0), "nu and nv")
    expect(call(u=-2), "nu and nv")
    big_u, big_v = np.arange(4098.0), np.arange(4097.0)
    expect(call(ue=big_u, u=4097, ve=big_v, v=4096), "2^24 pixels")  # one more row than 2^24 pixels
    expect(call(acc=2), "accumulate")
    expect(call(acc=-1), "accumulate")
    expect(call(n_seg=-1), "segment count")
    expect(call(source=altered(capacity=1 << 32), n_seg=1 << 31, cnt=None, rays=0), "segment count")
    expect(call(source=altered(width=2)), "width")
    expect(call(source=altered(width=16)), "width")
    expect(call(source=altered(tile_stride=256)), "tile stride")
    expect(call(n_seg=n_segments + 1, cnt=None, rays=0), "capacity")
    expect(call(rays=0), "multiple of n_rays")            # seg_count without its n_rays
    expect(call(n_seg=n_segments - 1), "multiple of n_rays")
    expect(call(cnt=None), "n_rays without seg_count")
    for at, value in ((0, np.nan), (3, np.inf), (nu, -np.inf), (2, good_u[1]), (2, good_u[4])):  # not finite, equal, decreasing
        expect(call(ue=with_value(good_u, at, value)), "edges")
    for at, value in ((1, np.nan), (3, good_v[2]), (nv, 0.0)):
        expect(call(ve=with_value(good_v, at, value)), "edges")
    expect(call(w_lo=1.0, w_hi=-1.0), "w_lo")
    expect(call(w_lo=np.nan), "w_lo")
    expect(call(w_hi=np.nan), "w_lo")
    expect(call(axes=with_value(good_axes, 1, np.nan)), "axes")
    expect(call(axes=with_value(good_axes, 8, np.inf)), "axes")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good: every one of the 2 n segments runs from (0.5, 0.5) two units along u: pixels (0, 0), (1, 0), (2, 0)
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    ref = np.zeros((nu, nv), dtype=np.int64)
    ref[:3, 0] = 2 * n
    length = np.zeros((nu, nv))
    length[:3, 0] = [0.5, 1.0, 0.5]
    np.testing.assert_array_equal(out.counts.cpu().numpy(), ref)
    np.testing.assert_array_equal(out.fluence.cpu().numpy(), 0.5 * 2 * n * length)
    assert int(out.skipped.item()) == 0
    assert call(acc=1, w_hi=np.inf, intensity=None) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... once more on top, weight 1, no far wall
    np.testing.assert_array_equal(out.counts.cpu().numpy(), 2 * ref)
    np.testing.assert_array_equal(out.fluence.cpu().numpy(), 1.5 * 2 * n * length)
    assert int(out.skipped.item()) == 0 and out.guards_untouched()
