"""GPU (MI355X): detector images — `OpticalTable.image_all` / `image_batch`, the hits of every monitor binned on the device by
the image mode of k_mon_count (ot_monitor_image_many), with no hit list.

Reference, in every comparison: numpy on the hit lists of the verified path,
    np.histogram2d(h.yList(None), h.zList(None), bins=[y_edges, z_edges], weights=h.IList(None))  for h in table.record_all(...).
Counts must be EQUAL.  The intensity of a bin must agree within 2 c 2^-53 sum|w| (c = the bin's count, sum|w| = the reference
sum of the absolute weights of the bin): the first-order bound for two different summation orders of the same c doubles —
derived, not measured.  torch's `P @ axis` and the kernel's dot product may round differently, so every comparison on traced data
first asserts, from the REFERENCE values, that no y or z lies within 1e-9 of a bin edge: a condition on the inputs (the CPU
oracle gives a smallest distance of 3e-7 for the cfg 2 inputs below, all eight monitors, all four bin shapes).
The bin rule itself is checked on exact coordinates, edges and their neighbouring doubles included, with no such condition."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine, image_plan, segment_source
from optable_amd.table import monitor_struct
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

U = 2.0**-53


EMPTY, DROPS, SPREAD = 2, 6, 7


def _reference(h, y_edges, z_edges):
    """(counts, sum w, sum |w|) per bin from the hit list `h`, after asserting that no coordinate is within 1e-9 of an edge."""
    y, z = h.yList(None).double().cpu().numpy(), h.zList(None).double().cpu().numpy()
    w = h.IList(None).double().cpu().numpy()
    if len(y):
        clear = min(np.abs(y[:, None] - y_edges[None, :]).min(), np.abs(z[:, None] - z_edges[None, :]).min())
        print(f"  {len(y)} hits, smallest distance to a bin edge {clear:.3g}")
        assert clear > 1e-9
    counts = np.histogram2d(y, z, bins=[y_edges, z_edges])[0]
    return counts.astype(np.int64), np.histogram2d(y, z, bins=[y_edges, z_edges], weights=w)[0], np.histogram2d(y, z, bins=[y_edges, z_edges], weights=np.abs(w))[0]


def _assert_image(im, h):
    counts, weights, y_edges, z_edges = im.to_host()
    assert im.monitor is h.monitor and counts.dtype == np.int64 and weights.dtype == np.float64
    assert counts.shape == weights.shape == (len(y_edges) - 1, len(z_edges) - 1) == im.bins
    c, w, w_abs = _reference(h, y_edges, z_edges)
    np.testing.assert_array_equal(counts, c)
    excess = np.abs(weights - w) - 2 * c * U * w_abs
    print(f"  {int(c.sum())} in range, most in a bin {int(c.max())}; intensity: largest error {np.abs(weights - w).max():.3g}, bound there "
          f"{(2 * c * U * w_abs).flat[np.argmax(np.abs(weights - w))]:.3g}")
    assert np.all(excess <= 0), float(excess.max())
    return c


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 5,003 rays, 5 segments, eight monitors: (table, monitors, {(layout, precision): (segs, record_all hits)}), traced and
    recorded on first use."""
    table, mons = support.cfg2_table(), support.eight_monitors()
    o, d = scenes.cfg2_rays(5003, 0)
    return table, mons, support.traced(table, lambda precision: support.weighted_batch(o, d, precision), 5, lambda segs: table.record_all(segs, monitors=mons))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_and_precisions(case1, layout, precision, monkeypatch):
    table, mons, get = case1
    segs, hits = get(layout, precision)
    assert image_plan(len(mons), 30, 30)["passes"] > 1  # eight monitors of 30 x 30 are more than one LDS pass holds
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("image_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        images = table.image_all(segs)  # the table's own monitors, in their order, bins=30
    assert len(images) == len(mons) and all(im.monitor is m for im, m in zip(images, mons))
    assert all(im.counts.is_cuda and im.counts.dtype == torch.int64 and im.intensity.dtype == torch.float64 for im in images)
    totals = [int(_assert_image(im, h).sum()) for im, h in zip(images, hits)]
    assert len(hits[EMPTY]) == 0 and totals[EMPTY] == 0 and not images[EMPTY].intensity.any()
    assert 0 < totals[DROPS] < len(hits[DROPS])  # hits outside the image range are dropped
    assert int((images[SPREAD].counts > 0).sum()) > 200
    assert all(t == len(h) for k, (t, h) in enumerate(zip(totals, hits)) if k != DROPS)
    two = table.image_all(segs, monitors=[mons[3], mons[0]])  # ... or those given
    _assert_image(two[0], hits[3])
    _assert_image(two[1], hits[0])
    _assert_image(table.image_batch(mons[SPREAD], segs), hits[SPREAD])


@pytest.mark.parametrize("bins", [(80, 80), (7, 5), (30, 1)])
def test_bin_shapes(case1, bins):
    """(80, 80): 6,400 bins a monitor, more than the LDS budget: global atomics.  (7, 5): a transposed or mis-strided image cannot
    pass.  (30, 1): one column."""
    table, mons, get = case1
    segs, hits = get("slots", "f64")
    assert image_plan(len(mons), *bins)["path"] == ("global" if bins == (80, 80) else "lds")
    images = table.image_all(segs, bins=bins, monitors=mons)
    totals = [int(_assert_image(im, h).sum()) for im, h in zip(images, hits)]
    assert all(im.bins == bins for im in images) and totals[EMPTY] == 0 and 0 < totals[DROPS] < len(hits[DROPS])
    if bins == (30, 1):
        one = table.image_all(segs, bins=30, monitors=mons)
        for a, b in zip(images, one):
            assert torch.equal(a.counts[:, 0], b.counts.sum(dim=1))


def test_more_than_one_group_of_monitors():
    table = support.cfg2_table()
    mons = [oa.Monitor([5.5 + 0.125 * k, 0, 0], 6, 6) for k in range(32)] + [oa.Monitor([5.5, 0, 0], 6, 6)]  # 33: positions 0 and 32 alike
    segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(2003, 0)), max_segments=5, layout="slots")
    assert image_plan(33, 7, 5)["passes"] == 2
    images = table.image_all(segs, bins=(7, 5), monitors=mons)
    hits = table.record_all(segs, monitors=mons)
    assert len(images) == 33 and sum(len(h) > 0 for h in hits) >= 3
    for im, h in zip(images, hits):
        _assert_image(im, h)
    assert int(images[0].counts.sum()) > 0 and torch.equal(images[0].counts, images[32].counts)


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (tests/test_gpu_trees.py): the [k][tree] slots, the dense list with holes
    and the list in generation order."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    eng = get_engine()
    eng.upload(table.compile())
    assert eng.trees_plan("f64", 12)["slots"]
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        hits = table.record_all(segs, monitors=mons)
        assert all(len(h) >= 320 for h in hits)  # every tree crosses each
        for im, h in zip(table.image_all(segs, monitors=mons), hits):
            assert int(_assert_image(im, h).sum()) == len(h)


class _Images(support.Sentinel):
    """counts / weights of M monitors of nby x nbz bins for ot_monitor_image_many, with a guard region on either side."""

    def __init__(self, M, nby, nbz):
        super().__init__(guard=64, counts=(torch.int64, (M, nby, nbz)), weights=(torch.float64, (M, nby, nbz)))


def test_accumulation():
    """A detector summed over the chunks of a trace: the two halves of a batch with `into=` against the whole batch in one call."""
    table = support.cfg2_table()
    o, d = scenes.cfg2_rays(2049, 3)
    whole = support.weighted_batch(o, d)
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 2, 2), oa.Monitor([7.5, 40, 0], 6, 6)]
    segs = table.trace_batch(whole, max_segments=5, layout="slots")
    hits = table.record_all(segs, monitors=mons)
    full = table.image_all(segs, monitors=mons)
    for im, h in zip(full, hits):
        _assert_image(im, h)
    halves = []
    for part in (slice(0, 1024), slice(1024, 2049)):
        b = RayBatch.from_arrays(o[part], d[part], wavelength=scenes.WL, intensity=whole.intensity[part].cpu().numpy(),
                                 q=support.Q, device="cuda")
        halves.append(table.trace_batch(b, max_segments=5, layout="slots"))
    images = table.image_all(halves[0], monitors=mons)
    first = [im.counts.clone() for im in images]
    assert table.image_all(halves[1], monitors=mons, into=images) is not None
    eng, structs = get_engine(), [monitor_struct(m) for m in mons]
    guarded = _Images(len(mons), 30, 30)
    guarded.counts.zero_()
    guarded.weights.zero_()
    axes, edges = support.image_tables(mons, 30, 30)
    for half in halves:
        eng.monitor_image_many(structs, axes, edges, (30, 30), half, into=(guarded.counts, guarded.weights))
    torch.cuda.synchronize()
    assert guarded.guards_untouched()
    for k, (im, ref, h) in enumerate(zip(images, full, hits)):
        assert torch.equal(im.counts, ref.counts) and torch.equal(guarded.counts[k], ref.counts)
        assert int(first[k].sum()) < int(im.counts.sum()) or len(h) == 0
        c, w, w_abs = _reference(h, im.y_edges, im.z_edges)
        for got in (im.intensity, guarded.weights[k]):
            assert np.all(np.abs(got.cpu().numpy() - w) <= 2 * c * U * w_abs)
    # without `into=` a call starts from zero again
    again = table.image_all(halves[0], monitors=mons)
    assert all(torch.equal(a.counts, b) for a, b in zip(again, first))


def _call(lib, ctx, mons, segs, nby, nbz, images, accumulate=0):
    src, n, count, n_rays = segment_source(segs)
    table = (abi.OtMonitor * len(mons))(*[monitor_struct(m) for m in mons])
    axes, edges = support.image_tables(mons, nby, nbz)
    dp = C.POINTER(C.c_double)
    return lib.ot_monitor_image_many(ctx, table, len(mons), axes.ctypes.data_as(dp), edges.ctypes.data_as(dp), nby, nbz, C.byref(src),
                                     segs.field("intensity").data_ptr(), n, None if count is None else count.data_ptr(), n_rays,
                                     images.counts.data_ptr(), images.weights.data_ptr(), accumulate)


def test_edges_of_the_partition():
    table = support.cfg2_table()
    eng = get_engine()
    # one ray, one segment (origin -> lens): the first monitor sees it, the second does not
    mons = [oa.Monitor([2.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 6, 6)]
    for layout in ("slots", "tiled", "append"):
        segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(1, 0)), max_segments=1, layout=layout)
        images = table.image_all(segs, monitors=mons)
        assert (int(images[0].counts.sum()), int(images[1].counts.sum())) == (1, 0)
        for im, h in zip(images, table.record_all(segs, monitors=mons)):
            _assert_image(im, h)
    # slot counts of 64 k + 1: 65 slots, and 2,049 = one more than a workgroup's 2,048
    for n, K in ((13, 5), (2049, 1)):
        segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(n, 3)), max_segments=K, layout="slots")
        assert segment_source(segs)[1] % 64 == 1
        images = table.image_all(segs, monitors=mons)
        assert int(images[0].counts.sum()) >= n  # every ray's first segment, the one in the slot behind the boundary among them
        for im, h in zip(images, table.record_all(segs, monitors=mons)):
            assert int(_assert_image(im, h).sum()) == len(h)
    # a list of no segments: zero images, and through the ABI n_segments = 0 zeroes a pre-filled image
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    for im in table.image_all(none, bins=(7, 5), monitors=mons):
        assert im.bins == (7, 5) and not im.counts.any() and not im.intensity.any()
    some = SegmentBatch(64, "f64", "cuda")
    some.n_valid = 0
    out = _Images(2, 7, 5)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, some, 7, 5, out) == 0
    torch.cuda.synchronize()
    assert not out.counts.any() and not out.weights.any() and out.guards_untouched()
    kept = _Images(2, 7, 5)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, some, 7, 5, kept, accumulate=1) == 0  # ... and adds nothing to one it accumulates into
    torch.cuda.synchronize()
    assert kept.untouched()


def _exact_segments(ys, zs, intensity):
    """A list of len(ys) x len(zs) segments (0, y, z) + t (1, 0, 0) of length 10: the unrotated monitor at x = 5 sees P = (0, y, z)
    exactly."""
    y, z = (a.ravel() for a in np.meshgrid(ys, zs, indexing="ij"))
    return support.list_segments(len(y), oy=y, oz=z, dx=1.0, length=10.0, intensity=intensity), y, z


def test_bin_rule_on_exact_coordinates():
    """Counts equal np.histogram2d with NO clear-of-edges precondition: y and z run over every edge of the 7 and 5 bins of +-1 and
    over the doubles next to each (-1.0 and +1.0 among them: the last bin is closed; their outer neighbours miss the monitor)."""
    table = oa.OpticalTable()
    mon = oa.Monitor([5, 0, 0], 2, 2)
    y_edges, z_edges = np.linspace(-1, 1, 8), np.linspace(-1, 1, 6)
    ys, zs = support.around(y_edges), support.around(z_edges)
    assert -1.0 in ys and 1.0 in ys and len(ys) == 24 and len(zs) == 18
    rng = np.random.default_rng(11)
    segs, y, z = _exact_segments(ys, zs, 0.25 + 0.75 * rng.random(len(ys) * len(zs)))
    assert segs.layout == "list"
    im = table.image_batch(mon, segs, bins=(7, 5))
    np.testing.assert_array_equal(im.y_edges, y_edges)
    np.testing.assert_array_equal(im.z_edges, z_edges)
    counts, weights, _, _ = im.to_host()
    w = segs.intensity.cpu().numpy()
    ref = np.histogram2d(y, z, bins=[y_edges, z_edges])[0].astype(np.int64)
    assert ref.sum() == 22 * 16  # all but the four outer neighbours
    np.testing.assert_array_equal(counts, ref)
    ref_w, ref_abs = np.histogram2d(y, z, bins=[y_edges, z_edges], weights=w)[0], np.histogram2d(y, z, bins=[y_edges, z_edges], weights=np.abs(w))[0]
    assert np.all(np.abs(weights - ref_w) <= 2 * ref * U * ref_abs)
    # ... and the same values many times over, more than one workgroup's slots: 7 x 432 = 3,024
    many, y, z = _exact_segments(np.tile(ys, 7), zs, np.full(7 * len(ys) * len(zs), 0.5))
    im = table.image_batch(mon, many, bins=(7, 5))
    assert torch.equal(im.counts.cpu(), torch.from_numpy(7 * ref)) and torch.equal(im.intensity.cpu(), torch.from_numpy(3.5 * ref))  # (halves add exactly)


def test_abi_errors(ctx):
    lib, c = ctx
    n, nby, nbz = 130, 7, 5
    segs = SegmentBatch(2 * n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    segs.dx.fill_(1.0)
    segs.length.fill_(10.0)
    segs.intensity.fill_(0.5)
    segs.ray.copy_(torch.arange(2 * n, dtype=torch.int32) % n)
    segs.count, segs.n_rays = torch.full((n,), 2, dtype=torch.int32, device="cuda"), n
    m = oa.Monitor([5, 0, 0], 2, 2)
    mon = monitor_struct(m)
    out = _Images(1, nby, nbz)
    src, n_segments, count, n_rays = segment_source(segs)
    assert (n_segments, n_rays) == (2 * n, n)
    good_axes, good_edges = support.image_tables([m], nby, nbz)
    dp = C.POINTER(C.c_double)

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, edges=good_edges, by=nby, bz=nbz, source=src, intensity=segs.intensity.data_ptr(),
             n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(), weights=out.weights.data_ptr(), acc=0):
        return lib.ot_monitor_image_many(ctx_, mons, M, None if axes is None else axes.ctypes.data_as(dp), None if edges is None else edges.ctypes.data_as(dp),
                                         by, bz, None if source is None else C.byref(source), intensity, n_seg, cnt, rays, counts, weights, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    def edges_with(at, value):
        e = good_edges.copy()
        e[0, at] = value
        return e

    def axes_with(at, value):
        a = good_axes.copy()
        a[0, at] = value
        return a

    for null in ("ctx_", "mons", "axes", "edges", "source", "counts", "weights", "intensity"):
        expect(call(**{null: None}), "NULL")
    no_field = altered()
    no_field.base[3] = None
    expect(call(source=no_field), "NULL field")
    expect(call(source=altered(ray=None)), "NULL field")
    expect(call(M=0), "n_monitors")
    expect(call(M=-3), "n_monitors")
    expect(call(by=0), "nby and nbz")
    expect(call(bz=0), "nby and nbz")
    expect(call(by=-2), "nby and nbz")
    expect(call(by=4097, bz=4096), "bins per monitor")  # one more row than 2^24 bins
    expect(call(acc=2), "accumulate")
    expect(call(acc=-1), "accumulate")
    expect(call(n_seg=-1), "segment count")
    expect(call(source=altered(capacity=1 << 32), n_seg=1 << 31, cnt=None, rays=0), "segment count")
    expect(call(source=altered(width=2)), "width")
    expect(call(source=altered(width=16)), "width")
    expect(call(n_seg=n_segments + 1, cnt=None, rays=0), "capacity")
    expect(call(rays=0), "multiple of n_rays")            # seg_count without its n_rays
    expect(call(n_seg=n_segments - 1), "multiple of n_rays")
    expect(call(cnt=None), "n_rays without seg_count")
    for at, value in ((0, np.nan), (3, np.inf), (nby, -np.inf), (2, good_edges[0, 1]), (2, good_edges[0, 4]),  # y: not finite, equal, decreasing
                      (nby + 1, np.nan), (nby + 3, good_edges[0, nby + 2]), (nby + nbz + 1, 0.0)):             # z likewise
        expect(call(edges=edges_with(at, value)), "edges")
    expect(call(axes=axes_with(1, np.nan)), "axes")
    expect(call(axes=axes_with(5, np.inf)), "axes")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good: every one of the 2 n segments crosses x = 5 at P = (0, 0, 0), bin (3, 2) of 7 x 5
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    ref = np.zeros((nby, nbz), dtype=np.int64)
    ref[3, 2] = 2 * n
    np.testing.assert_array_equal(out.counts[0].cpu().numpy(), ref)
    np.testing.assert_array_equal(out.weights[0].cpu().numpy(), 0.5 * ref)
    assert call(acc=1) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    np.testing.assert_array_equal(out.counts[0].cpu().numpy(), 2 * ref)
    np.testing.assert_array_equal(out.weights[0].cpu().numpy(), 1.0 * ref)
    assert out.guards_untouched()
