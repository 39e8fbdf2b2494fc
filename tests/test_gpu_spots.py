"""GPU (MI355X): spot statistics — `OpticalTable.spots_all` / `spots_batch`, the moments of every monitor's hits on the monitor and
on planes displaced along its normal, summed on the device by k_mon_spots (ot_monitor_spots_many) with no hit list, no image and
no floating-point atomic.

Reference, in every comparison: tests/spots_reference.py on the segment records copied from the device — the rule of the header in
numpy, its sums formed with math.fsum.  Every case first asserts, from the REFERENCE, that no decision (plane crossing within the
segment, rectangle) lies within 1e-7 of its boundary: a condition on the inputs, some 1e6 times the rounding of P and t at table
scale.  Counts must then be EQUAL.

Tolerance of the sums: `bound` of the reference, derived in its docstring from the roundings of P (128 U S a coordinate, U = 2^-53,
S the magnitude of the operands over |dx|), of the products (U or 2 U a term) and of a sum of c terms in any order
((c + 2) U sum |term|) — derived, not measured.  Derived quantities (rms radius, best focus) are held to what those bounds allow
(spots_reference.variance_bound), propagated in the test that uses them.

Why `centre` matters (test_weight_none_and_centre): a spot of rms 1e-6 at y = 0.4 has Wyy / W = 0.16 and var_y = 1e-12.  With
centre = 0 the bound of Wyy / W is 2 |y| d = 1e-13 from the coordinates alone, a tenth of the variance: no reference can confirm
the radius to better than percents, whatever the kernel does.  With centre on the spot |y| is 1e-6 and the same d bounds the
variance to 1e-6 of itself."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine, segment_source, spots_plan
from optable_amd.table import monitor_struct
from spots_reference import U, radius_interval, spots_reference, variance_bound
from support import ctx  # noqa: F401  (the fixture)
from wavefront_cases import axes_of

pytestmark = pytest.mark.gpu

OFFSETS = np.array([-0.9, -0.3, 0.0, 0.45, 0.9])


def _reference(records, mon, offsets, weight="intensity", centre=(0.0, 0.0)):
    o, d, length, intensity = records
    s = monitor_struct(mon)
    ref = spots_reference(o, d, length, intensity if weight == "intensity" else None, list(s.M), list(s.origin), s.half_width, s.half_height, axes_of(mon),
                          centre, offsets)
    print(f"  margin {ref.margin:.3g}, hits per plane {ref.counts.min()} .. {ref.counts.max()}")
    assert ref.margin > 1e-7  # a condition on the inputs
    return ref


def _assert_sums(counts, sums, ref, factor=1.0):
    np.testing.assert_array_equal(counts, ref.counts)
    err = np.abs(sums - ref.sums)
    worst = np.argmax(err - factor * ref.bound)
    print(f"  sums: largest error {err.max():.3g}; nearest to its bound {err.flat[worst]:.3g} of {factor * ref.bound.flat[worst]:.3g}")
    assert np.all(err <= factor * ref.bound), float((err - factor * ref.bound).max())
    assert np.all(sums[ref.counts == 0] == 0.0)


def _assert_spots(sp, ref):
    counts, sums, offsets = sp.to_host()
    assert counts.dtype == np.int64 and sums.dtype == np.float64 and counts.shape == (len(offsets),) and sums.shape == (len(offsets), 6)
    assert sp.counts.is_cuda and sp.sums.is_cuda
    _assert_sums(counts, sums, ref)
    radius = sp.rms_radius().cpu().numpy()
    for j in np.nonzero(ref.counts > 0)[0]:
        lo, hi = radius_interval(ref.sums[j], ref.bound[j])
        assert lo <= radius[j] <= hi, (j, lo, radius[j], hi)
    assert np.isnan(radius[ref.counts == 0]).all()


def _monitors():
    return [oa.Monitor([7.5, 0, 0], 6, 6),
            oa.Monitor([7.5, 0, 0], 0.5, 0.5),          # clips the beam
            oa.Monitor([7.5, 40, 0], 6, 6),             # where no segment passes
            oa.Monitor([7.5, 0, 0], 6, 6).RotZ(0.3)]    # planes displaced along a normal that is not x


EMPTY = 2


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 5,003 rays, 5 segments — 25,015 slots: 13 workgroups of 2,048 with a ragged tail — four monitors, five planes:
    (table, monitors, {(layout, precision): (segs, (records, [reference per monitor]))}), traced and reduced on the host on first use."""
    table, mons = support.cfg2_table(), _monitors()
    o, d = scenes.cfg2_rays(5003, 0)

    def derive(segs):
        records = support.host_records(segs)
        return records, [_reference(records, m, OFFSETS) for m in mons]

    return table, mons, support.traced(table, lambda precision: support.weighted_batch(o, d, precision), 5, derive)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_and_precisions(case1, layout, precision, monkeypatch):
    table, mons, get = case1
    segs, (records, refs) = get(layout, precision)
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("spots_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        spots = table.spots_all(segs, offsets=OFFSETS)  # the table's own monitors, in their order
    assert len(spots) == len(mons) and all(sp.monitor is m for sp, m in zip(spots, mons))
    for sp, ref in zip(spots, refs):
        _assert_spots(sp, ref)
    assert refs[0].counts.min() >= 5003 and 0 < refs[1].counts.max() < 5003  # every ray crosses the wide monitor; the small one clips
    assert not spots[EMPTY].counts.any() and not spots[EMPTY].sums.any() and torch.isnan(spots[EMPTY].rms_radius()).all()
    assert torch.isnan(spots[EMPTY].centroid()).all() and spots[EMPTY].best_focus()[0] != spots[EMPTY].best_focus()[0]
    two = table.spots_all(segs, offsets=OFFSETS, monitors=[mons[3], mons[0]])  # ... or those given
    _assert_spots(two[0], refs[3])
    _assert_spots(two[1], refs[0])
    # J = 1, the default: the monitor itself
    one = table.spots_batch(mons[1], segs)
    assert one.offsets.tolist() == [0.0] and int(one.counts[0]) == refs[1].counts[2]
    assert np.all(np.abs(one.sums[0].cpu().numpy() - refs[1].sums[2]) <= refs[1].bound[2])


def test_layouts_agree(case1):
    """Counts equal and sums within twice the tolerance from one layout to the next (each is within one of its own reference)."""
    table, mons, get = case1
    got = {}
    for layout in ("slots", "tiled", "append"):
        segs, (_, refs) = get(layout, "f64")
        got[layout] = [sp.to_host()[:2] for sp in table.spots_all(segs, offsets=OFFSETS, monitors=mons)]
    for layout in ("tiled", "append"):
        for (c0, s0), (c1, s1), ref in zip(got["slots"], got[layout], get("slots", "f64")[1][1]):
            np.testing.assert_array_equal(c0, c1)
            assert np.all(np.abs(s0 - s1) <= 2 * ref.bound)


@pytest.mark.parametrize("n,K", [(130, 3), (1027, 5), (1, 1)])
def test_batch_sizes(n, K):
    """130 x 3 = 390 slots: a partial wave in a partial workgroup; 1,027 x 5 = 5,135: three workgroups, the last one ragged; 1 x 1."""
    table = support.cfg2_table()
    mons = [oa.Monitor([2.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 6, 6)]
    segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(n, 3)), max_segments=K, layout="slots")
    records = support.host_records(segs)
    offsets = [-0.5, 0.0, 0.25]
    spots = table.spots_all(segs, offsets=offsets, monitors=mons)
    for sp, m in zip(spots, mons):
        _assert_spots(sp, _reference(records, m, offsets))
    assert int(spots[0].counts.min()) >= n and (K > 1) == bool(spots[1].counts.any())


def test_more_cells_than_one_group():
    """2 monitors x 200 planes = 400 cells: two launches, the first ending inside the second monitor's planes."""
    table = support.cfg2_table()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([7.0, 0, 0], 5, 5).RotZ(-0.2)]  # (wide: 400 planes of a clipping aperture put some ray on a rim)
    offsets = np.linspace(-0.995, 0.995, 200)
    assert spots_plan(2, 200) == [(0, 256), (256, 144)]
    segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(1003, 5)), max_segments=5, layout="slots")
    records = support.host_records(segs)
    spots = table.spots_all(segs, offsets=offsets, monitors=mons)
    for sp, m in zip(spots, mons):
        _assert_spots(sp, _reference(records, m, offsets))
    assert int(spots[1].counts.min()) > 0


def test_more_cells_than_one_group_streamed():
    """The 400 cells and 1,003 rays above as two chunks of 512 and 491 rays, the second added with `into=`: every launch of the
    second call draws its own ticket, shares the call's partials and adds to what the first call left.  The hits are those of the
    one-call test, so no ray sits on a rim; the bounds are the reference's own for the concatenated records."""
    table = support.cfg2_table()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([7.0, 0, 0], 5, 5).RotZ(-0.2)]
    offsets = np.linspace(-0.995, 0.995, 200)
    assert spots_plan(2, 200) == [(0, 256), (256, 144)]
    o, d = scenes.cfg2_rays(1003, 5)
    whole = support.weighted_batch(o, d)
    chunks = []
    for part in (slice(0, 512), slice(512, 1003)):
        b = RayBatch.from_arrays(o[part], d[part], wavelength=scenes.WL, intensity=whole.intensity[part].cpu().numpy(),
                                 q=support.Q, device="cuda")
        chunks.append(table.trace_batch(b, max_segments=5, layout="slots"))
    records = tuple(np.concatenate(parts) for parts in zip(*(support.host_records(c) for c in chunks)))
    spots = table.spots_all(chunks[0], offsets=offsets, monitors=mons)
    table.spots_all(chunks[1], offsets=offsets, monitors=mons, into=spots)
    for sp, m in zip(spots, mons):
        _assert_spots(sp, _reference(records, m, offsets))
    assert int(spots[1].counts.min()) > 0


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (every hit splits, tests/test_gpu_trees.py): the [k][tree] slots with count[i],
    the dense list with holes and the list in generation order."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    offsets = [-0.2, 0.0, 0.3]
    eng = get_engine()
    eng.upload(table.compile())
    assert eng.trees_plan("f64", 12)["slots"]
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        records = support.host_records(segs)
        for sp, m in zip(table.spots_all(segs, offsets=offsets, monitors=mons), mons):
            ref = _reference(records, m, offsets)
            _assert_spots(sp, ref)
            assert ref.counts.min() >= 320  # every tree crosses each plane


def _torch_moments(h):
    """(count, the six sums) of a `MonitorHits` with torch, on the device."""
    y, z, w = h.yList(None).double(), h.zList(None).double(), h.IList(None).double()
    return len(h), torch.stack([w.sum(), (w * y).sum(), (w * z).sum(), (w * y * y).sum(), (w * z * z).sum(), (w * y * z).sum()]).cpu().numpy()


def test_planes_are_displaced_monitors(case1):
    """Offset 0 is the monitor: the moments of its `record_all` hits.  Offset d is a Monitor built at the displaced pose.  torch sums
    in an order of its own and rounds its own P: twice the tolerance."""
    table, mons, get = case1
    segs, (_, refs) = get("slots", "f64")
    for k in (0, 1, 3):
        mon, ref = mons[k], refs[k]
        normal = np.asarray(mon.transform_matrix, dtype=float)[:, 0]
        assert abs(normal @ mon.tangent_Y) < 1e-15 and abs(normal @ mon.tangent_Z) < 1e-15
        moved = []
        for off in OFFSETS:
            m = oa.Monitor(list(np.asarray(mon.origin, dtype=float) + off * normal), mon.width, mon.height)
            moved.append(m.RotZ(0.3) if k == 3 else m)
            np.testing.assert_allclose(np.asarray(moved[-1].transform_matrix, dtype=float), np.asarray(mon.transform_matrix, dtype=float), atol=1e-16)
        sp = table.spots_batch(mon, segs, offsets=OFFSETS)
        counts, sums, _ = sp.to_host()
        for j, h in enumerate(table.record_all(segs, monitors=moved)):
            c, s = _torch_moments(h)
            assert c == counts[j] == ref.counts[j]
            assert np.all(np.abs(s - sums[j]) <= 2 * ref.bound[j]), (k, j)
        assert moved[2].origin[0] == mon.origin[0]  # offset 0: the monitor's own pose


def test_determinism(case1):
    """The same call twice: the same bits, sums included — also for `into=` twice."""
    table, mons, get = case1
    for layout in ("slots", "append"):
        segs = get(layout, "f64")[0]
        a, b = (table.spots_all(segs, offsets=OFFSETS, monitors=mons) for _ in range(2))
        for x, y in zip(a, b):
            assert torch.equal(x.counts, y.counts) and torch.equal(x.sums, y.sums) and x.sums is not y.sums
        table.spots_all(segs, offsets=OFFSETS, monitors=mons, into=a)
        table.spots_all(segs, offsets=OFFSETS, monitors=mons, into=b)
        for x, y in zip(a, b):
            assert torch.equal(x.counts, y.counts) and torch.equal(x.sums, y.sums)
        assert int(a[0].counts.min()) >= 2 * 5003 and bool((a[0].sums != 0).all())
    many = np.linspace(-0.9, 0.9, 300)  # two launches
    a, b = (table.spots_batch(mons[0], segs, offsets=many) for _ in range(2))
    assert torch.equal(a.counts, b.counts) and torch.equal(a.sums, b.sums)


def test_streaming():
    """Two chunks of a trace with `into=` against the reference of their concatenation."""
    table = support.cfg2_table()
    o, d = scenes.cfg2_rays(2049, 3)
    whole = support.weighted_batch(o, d)
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 0.7, 0.7), oa.Monitor([7.5, 40, 0], 6, 6)]
    halves = []
    for part in (slice(0, 1024), slice(1024, 2049)):
        b = RayBatch.from_arrays(o[part], d[part], wavelength=scenes.WL, intensity=whole.intensity[part].cpu().numpy(),
                                 q=support.Q, device="cuda")
        halves.append(table.trace_batch(b, max_segments=5, layout="slots"))
    records = tuple(np.concatenate(parts) for parts in zip(*(support.host_records(h) for h in halves)))
    spots = table.spots_all(halves[0], offsets=OFFSETS, monitors=mons)
    first = [sp.counts.clone() for sp in spots]
    assert table.spots_all(halves[1], offsets=OFFSETS, monitors=mons, into=spots) is not None
    for sp, m, before in zip(spots, mons, first):
        _assert_spots(sp, _reference(records, m, OFFSETS))
        assert int(before.sum()) < int(sp.counts.sum()) or not sp.counts.any()
    again = table.spots_all(halves[0], offsets=OFFSETS, monitors=mons)  # without `into=` a call starts from zero again
    assert all(torch.equal(a.counts, b) for a, b in zip(again, first))


def test_weight_none_and_centre():
    """3,000 slightly tilted segments (more than a workgroup's 2,048) whose spot on the monitor at x = 5 is 0.4 off axis, rms 1e-6 a
    coordinate.  weight="none": W is the count.  With `centre` on the spot the radius is confirmed to 1e-5 of itself; with centre = 0
    the derived bound is percents of the radius (the module's docstring says why), and all that can be asserted is that bound."""
    rng = np.random.default_rng(17)
    n = 3000
    tilt = np.array([1.0, 1e-6, -2e-6])  # (the spot moves by less than its size from plane to plane: one centre serves all three)
    d = np.tile(tilt / np.sqrt(tilt @ tilt), (n, 1))
    o = np.stack([np.zeros(n), 0.4 + 1e-6 * rng.normal(size=n), 1e-6 * rng.normal(size=n)], axis=1)
    intensity = 0.25 + 0.75 * rng.random(n)
    segs = support.list_batch(o, d, np.full(n, 8.0), intensity)
    records = (o, d, np.full(n, 8.0), intensity)
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 2, 2)
    offsets = [-0.5, 0.0, 0.5]
    plain = table.spots_batch(mon, segs, offsets=offsets, weight="none")
    _assert_spots(plain, _reference(records, mon, offsets, weight="none"))
    assert plain.power().tolist() == [float(n)] * 3 and plain.counts.tolist() == [n] * 3 and plain.weight == "none"
    centre = (0.400005, -0.00001)  # where the bundle's axis meets the monitor
    near = table.spots_batch(mon, segs, offsets=offsets, centre=centre)
    ref = _reference(records, mon, offsets, centre=centre)
    _assert_spots(near, ref)
    radius = near.rms_radius().cpu().numpy()
    for j in range(3):
        lo, hi = radius_interval(ref.sums[j], ref.bound[j])
        print(f"  centre on the spot: radius {radius[j]:.6g} in [{lo:.6g}, {hi:.6g}]")
        assert 1.2e-6 < radius[j] < 1.6e-6 and hi - lo < 1e-5 * radius[j]
    np.testing.assert_allclose(near.centroid().cpu().numpy()[1], [0.4 + 5e-6, -1e-5], atol=1e-7)  # `centre` added back
    far = table.spots_batch(mon, segs, offsets=offsets)
    ref0 = _reference(records, mon, offsets)
    _assert_spots(far, ref0)
    lo, hi = radius_interval(ref0.sums[1], ref0.bound[1])
    assert hi - lo > 1e-2 * radius[1]  # the bound itself: no reference confirms this radius


def test_best_focus_of_a_thin_lens():
    """A collimated bundle through Lens(f = 5) at x = 5 crosses the axis at x = 10.  Monitor at x = 10.3, 25 planes over +-0.6:
    best_focus() is (-0.3, 0).  Tolerance: the three variances the vertex is taken from are each within e of the reference's
    (variance_bound, from the bounds of the sums); with h the spacing, the two slopes are within 2 e / h, the curvature a within
    da = 2 e / h^2, b within db = 4 e / h: the vertex moves by at most db / (2 a') + |b| da / (2 a'^2), a' = a - da, and the
    variance at the vertex by e + |b| db / (2 a') + b^2 da / (4 a'^2); the focus itself is as sharp as the trace's rounding, which
    the bound of P contains."""
    n = 1500
    rng = np.random.default_rng(23)
    r, phi = 0.5 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    o = np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], axis=1)
    batch = RayBatch.from_arrays(o, np.tile([1.0, 0.0, 0.0], (n, 1)), wavelength=scenes.WL, q=support.Q, device="cuda")
    table, mon = oa.OpticalTable(), oa.Monitor([10.3, 0, 0], 2, 2)
    table.add_components([oa.Lens([5, 0, 0], focal_length=5, radius=1.0)])
    segs = table.trace_batch(batch, max_segments=3)
    offsets = np.linspace(-0.6, 0.6, 25)
    sp = table.spots_batch(mon, segs, offsets=offsets)
    ref = _reference(support.host_records(segs), mon, offsets)
    _assert_spots(sp, ref)
    assert (ref.counts == n).all()
    var, e = zip(*(variance_bound(ref.sums[j], ref.bound[j]) for j in range(25)))
    i = int(np.argmin(var))
    assert i == 6 and abs(offsets[i] + 0.3) < 1e-15
    h, e = offsets[1] - offsets[0], max(e[i - 1:i + 2])
    a = (var[i - 1] - 2 * var[i] + var[i + 1]) / (2 * h * h)
    b = (var[i + 1] - var[i - 1]) / (2 * h)
    da, db = 2 * e / h**2, 4 * e / h
    tol_x = db / (2 * (a - da)) + abs(b) * da / (2 * (a - da) ** 2)
    tol_v = e + abs(b) * db / (2 * (a - da)) + b * b * da / (4 * (a - da) ** 2) + var[i]
    x, radius = sp.best_focus()
    print(f"  best focus {x:.12g} (tolerance {tol_x:.3g}), radius {radius:.3g} (tolerance {math.sqrt(tol_v):.3g}); a = {a:.4g}")
    assert tol_x < 1e-6 and abs(x + 0.3) <= tol_x and 0.0 <= radius <= math.sqrt(tol_v)
    # the curve around it is the cone's: radius = |offset + 0.3| / 5 times the rms radius of the pupil about its own centroid
    want = np.abs(offsets + 0.3) * np.sqrt(np.mean(r * r) - o[:, 1].mean() ** 2 - o[:, 2].mean() ** 2) / 5
    np.testing.assert_allclose(sp.rms_radius().cpu().numpy(), want, atol=1e-9)


def test_power_is_the_sum_of_the_image():
    """cfg 2 at small n: `power()` on its monitor against `image_all(...).intensity.sum()`.  Both add the same c weights in orders of
    their own ((c - 1) U sum |w| each), torch then the 900 bins: (2 c + 900) U sum |w|."""
    table = support.cfg2_table()
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(2003, 1)), max_segments=5, layout="slots")
    sp = table.spots_batch(mon, segs)
    im = table.image_batch(mon, segs)
    c = int(sp.counts[0])
    assert c == int(im.counts.sum()) >= 2003
    total = float(im.intensity.sum())
    assert abs(float(sp.power()[0]) - total) <= (2 * c + 900) * U * total


def test_the_example_runs():
    """examples/through_focus.py as a user would run it: 41 planes from one trace, the focus of the f = 5 lens at x = 10."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "through_focus.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "41 planes" in out.stdout and "best focus: offset -0.500000 (x = 10.000000)" in out.stdout, out.stdout


class _Out(support.Sentinel):
    """counts / sums of M monitors x J planes for ot_monitor_spots_many, with a guard region on either side of each."""

    def __init__(self, M, J):
        super().__init__(guard=64, counts=(torch.int64, (M, J)), sums=(torch.float64, (M, J, 6)))


def _call(lib, ctx, mons, segs, offsets, out, accumulate=0, weighted=True):
    src, n, count, n_rays = segment_source(segs)
    table = (abi.OtMonitor * len(mons))(*[monitor_struct(m) for m in mons])
    axes, centre, offsets = np.array([axes_of(m) for m in mons]), np.zeros((len(mons), 2)), np.asarray(offsets, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    return lib.ot_monitor_spots_many(ctx, table, len(mons), axes.ctypes.data_as(dp), centre.ctypes.data_as(dp), offsets.ctypes.data_as(dp), len(offsets),
                                     C.byref(src), segs.field("intensity").data_ptr() if weighted else None, n, None if count is None else count.data_ptr(),
                                     n_rays, out.counts.data_ptr(), out.sums.data_ptr(), accumulate)


def test_no_segments_and_the_guards():
    table, eng = support.cfg2_table(), get_engine()
    mons = [oa.Monitor([2.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 6, 6)]
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    for sp in table.spots_all(none, offsets=[0.0, 0.5], monitors=mons):
        assert not sp.counts.any() and not sp.sums.any() and torch.isnan(sp.rms_radius()).all()
    some = SegmentBatch(64, "f64", "cuda")
    some.n_valid = 0
    out = _Out(2, 3)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, some, [0.0, 0.5, 1.0], out) == 0  # n_segments = 0 zeroes a pre-filled output
    torch.cuda.synchronize()
    assert not out.counts.any() and not out.sums.any() and out.guards_untouched()
    kept = _Out(2, 3)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, some, [0.0, 0.5, 1.0], kept, accumulate=1) == 0  # ... and adds nothing to one it accumulates into
    torch.cuda.synchronize()
    assert kept.untouched()
    # a real batch into guarded outputs, 300 planes (two launches): nothing outside them is written
    segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(257, 2)), max_segments=5, layout="append")
    offsets = np.linspace(-0.9, 0.9, 300)
    wide = _Out(2, 300)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, segs, offsets, wide) == 0
    torch.cuda.synchronize()
    assert wide.guards_untouched()
    records = support.host_records(segs)
    for k, m in enumerate(mons):
        _assert_sums(wide.counts[k].cpu().numpy(), wide.sums[k].cpu().numpy(), _reference(records, m, offsets))


def test_abi_errors(ctx):
    lib, c = ctx
    n, J = 130, 3
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
    out = _Out(1, J)
    src, n_segments, count, n_rays = segment_source(segs)
    assert (n_segments, n_rays) == (2 * n, n)
    good_axes, good_centre, good_offsets = axes_of(m).reshape(1, 6), np.array([[0.25, -0.5]]), np.array([-1.0, 0.0, 6.0])
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, centre=good_centre, offsets=good_offsets, n_off=J, source=src,
             intensity=segs.intensity.data_ptr(), n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(),
             sums=out.sums.data_ptr(), acc=0):
        return lib.ot_monitor_spots_many(ctx_, mons, M, ptr(axes), ptr(centre), ptr(offsets), n_off, None if source is None else C.byref(source), intensity,
                                         n_seg, cnt, rays, counts, sums, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    def with_value(good, at, value):
        a = good.copy()
        a.flat[at] = value
        return a

    for null in ("ctx_", "mons", "axes", "centre", "offsets", "source", "counts", "sums"):
        expect(call(**{null: None}), "NULL")
    no_field = altered()
    no_field.base[3] = None
    expect(call(source=no_field), "NULL field")
    expect(call(source=altered(ray=None)), "NULL field")
    expect(call(M=0), "n_monitors")
    expect(call(M=-3), "n_monitors")
    expect(call(n_off=0), "n_offsets")
    expect(call(n_off=-1), "n_offsets")
    expect(call(M=1 << 10, n_off=(1 << 10) + 1), "2^20")  # (refused before a monitor or an offset is read)
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
    expect(call(axes=with_value(good_axes, 1, np.nan)), "axes")
    expect(call(axes=with_value(good_axes, 5, np.inf)), "axes")
    expect(call(centre=with_value(good_centre, 0, np.nan)), "centre")
    expect(call(centre=with_value(good_centre, 1, -np.inf)), "centre")
    expect(call(offsets=with_value(good_offsets, 2, np.nan)), "offsets")
    expect(call(offsets=with_value(good_offsets, 0, np.inf)), "offsets")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good: every one of the 2 n segments runs from x = 0 to 10 along the axis: it crosses the planes at x = 4
    # and 5 at P = (0, 0, 0), y = -0.25, z = 0.5, and ends before x = 11
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    c2 = 2 * n
    want = np.array([0.5 * c2, -0.125 * c2, 0.25 * c2, 0.03125 * c2, 0.125 * c2, -0.0625 * c2])  # (binary fractions: every sum is exact)
    assert out.counts[0].tolist() == [c2, c2, 0]
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), [want, want, np.zeros(6)])
    assert call(acc=1) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    assert out.counts[0].tolist() == [2 * c2, 2 * c2, 0]
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), [2 * want, 2 * want, np.zeros(6)])
    assert call(intensity=None) == 0 and lib.ot_ctx_synchronize(c) == 0  # intensity = NULL: weight 1
    assert out.counts[0].tolist() == [c2, c2, 0] and out.sums[0, :, 0].tolist() == [float(c2), float(c2), 0.0]
    assert out.guards_untouched()
