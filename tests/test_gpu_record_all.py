"""GPU (MI355X): `OpticalTable.record_all` — Monitor.record on every monitor of a table in one pass over the segments
(ot_monitor_record_many: k_mon_count, a scan, k_mon_emit) — against `record_batch` per monitor (ot_monitor_record_f64, the
path it stands next to) and, in double precision, the C oracle.  Slot sets must be identical; P, t and the accessors agree to
1e-12, the bound tests/test_gpu_parity.py::test_record_batch_matches_object_api holds this pass to.  Identical sets need
inputs with no hit on an edge: every comparison first asserts, from the record_batch values, that no reference hit lies
within 1e-9 of the monitor's half-width or half-height or of the limits on t.
Shapes: 5,003 rays x 5 slots (a ragged last wave, 13 workgroups of 2,048 slots, 391 tiles), 33 monitors (two launches of the
kernels), slot counts of 64 k + 1."""
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
from optable_amd.engine import get_engine, segment_source
from optable_amd.table import monitor_struct
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)
EMPTY = 2  # (its place among support.six_monitors())


def _gather(field, slot):
    return field[slot // 64, slot % 64] if field.dim() == 2 else field[slot]


def _assert_clear_of_edges(ref):
    """No hit of `ref` (a record_batch result) within 1e-9 of an aperture edge or of the limits on t (|t| < 1e-9, t > length)."""
    if len(ref) == 0:
        return
    P, t = ref.P.cpu().numpy(), ref.t.cpu().numpy()
    length = _gather(ref.segs.length, ref.slot).double().cpu().numpy()
    assert np.all(np.abs(np.abs(P[:, 1]) - ref.monitor.width / 2) > 1e-9)
    assert np.all(np.abs(np.abs(P[:, 2]) - ref.monitor.height / 2) > 1e-9)
    assert np.all(t - 1e-9 > 1e-9) and np.all(length - t > 1e-9)  # (the lower limit on t is 1e-9 itself: |t| < 1e-9 is no hit)


def _assert_same_hits(got, ref):
    _assert_clear_of_edges(ref)
    assert len(got) == len(ref)
    assert torch.equal(got.slot, ref.slot)  # identical slots, in the reference's order
    for acc in ("PList", "tList", "yList", "zList", "tYList", "IList", "ray_index"):
        np.testing.assert_allclose(getattr(got, acc)(None).cpu().numpy(), getattr(ref, acc)(None).cpu().numpy(), err_msg=acc, **TOL)
    for sort in ("YZ", "ID"):
        np.testing.assert_allclose(got.yList(sort).cpu().numpy(), ref.yList(sort).cpu().numpy(), err_msg=sort, **TOL)


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 5,003 rays, 5 segments, six monitors: (table, monitors, {(layout, precision): (segs, record_batch per monitor)}),
    traced and recorded on first use."""
    table, mons = support.cfg2_table(), support.six_monitors()
    o, d = scenes.cfg2_rays(5003, 0)
    return table, mons, support.traced(table, lambda precision: support.batch(o, d, precision), 5, lambda segs: [table.record_batch(m, segs) for m in mons])


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_and_precisions(case1, layout, precision):
    table, mons, get = case1
    segs, refs = get(layout, precision)
    table.monitors = []
    table.add_monitors(mons)
    hits = table.record_all(segs)  # the table's own monitors, in their order
    assert len(hits) == len(mons) and all(h.monitor is m for h, m in zip(hits, mons))
    assert sum(len(r) > 0 for r in refs) >= 3 and len(refs[EMPTY]) == 0 and len(hits[EMPTY]) == 0
    assert 0 < len(refs[5]) < len(refs[0])  # the small monitor clips
    for got, ref in zip(hits, refs):
        _assert_same_hits(got, ref)
    two = table.record_all(segs, monitors=[mons[3], mons[0]])  # ... or those given
    _assert_same_hits(two[0], refs[3])
    _assert_same_hits(two[1], refs[0])


def test_no_conversion_copy(case1, monkeypatch):
    table, mons, get = case1
    segs, refs = get("tiled", "f32")

    def refuse(self, *args, **kwargs):
        raise AssertionError("record_all converted the batch")

    monkeypatch.setattr(SegmentBatch, "to_slots", refuse)
    monkeypatch.setattr(SegmentBatch, "astype", refuse)
    hits = table.record_all(segs, monitors=mons)
    for got, ref in zip(hits, refs):  # (the accessors read the tiles in place too)
        _assert_same_hits(got, ref)


def test_more_than_one_chunk_of_monitors():
    table = support.cfg2_table()
    mons = [oa.Monitor([5.5 + 0.125 * k, 0, 0], 6, 6) for k in range(32)] + [oa.Monitor([5.5, 0, 0], 6, 6)]  # 33: positions 0 and 32 alike
    segs = table.trace_batch(support.batch(*scenes.cfg2_rays(2003, 0)), max_segments=5, layout="slots")
    hits = table.record_all(segs, monitors=mons)
    assert len(hits) == 33 and sum(len(h) > 0 for h in hits) >= 3
    for m, got in zip(mons, hits):
        _assert_same_hits(got, table.record_batch(m, segs))
    assert len(hits[0]) > 0 and torch.equal(hits[0].slot, hits[32].slot)
    assert torch.equal(hits[0].P, hits[32].P) and torch.equal(hits[0].t, hits[32].t)


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
        for m, got in zip(mons, hits):
            _assert_same_hits(got, table.record_batch(m, segs))


def test_oracle(case1, oracle):
    table, mons, get = case1
    segs, _ = get("slots", "f64")
    host = segs.to_host(reference_order=True)
    for m, got in zip(mons, table.record_all(segs, monitors=mons)):
        idx, P, t = oracle.monitor_record(monitor_struct(m), host)
        assert len(idx) == len(got)
        np.testing.assert_array_equal(host["ray"][idx], got.ray_index(None).cpu().numpy())
        np.testing.assert_allclose(got.PList(None).cpu().numpy().reshape(-1, 3), P.reshape(-1, 3), **TOL)
        np.testing.assert_allclose(got.tList(None).cpu().numpy(), t, **TOL)


class _Outputs:
    """The output buffers of ot_monitor_record_many for M monitors and `capacity` entries, each with a guard region behind it."""
    GUARD = 64

    def __init__(self, M, capacity):
        self.M, self.capacity = M, capacity
        self.idx = torch.full((capacity + self.GUARD,), -7, dtype=torch.int64, device="cuda")
        self.real = [torch.full((capacity + self.GUARD,), -7.0, dtype=torch.float64, device="cuda") for _ in range(4)]
        self.first = torch.full((M + 1 + self.GUARD,), -7, dtype=torch.int64, device="cuda")
        self.total = torch.full((1 + self.GUARD,), -7, dtype=torch.int64, device="cuda")

    def args(self):
        return (self.capacity, self.first.data_ptr(), self.idx.data_ptr(), *(r.data_ptr() for r in self.real), self.total.data_ptr())

    def guards_untouched(self):
        return (bool((self.idx[self.capacity:] == -7).all()) and all(bool((r[self.capacity:] == -7.0).all()) for r in self.real)
                and bool((self.first[self.M + 1:] == -7).all()) and bool((self.total[1:] == -7).all()))


def _call(lib, ctx, mons, segs, out):
    src, n, count, n_rays = segment_source(segs)
    table = (abi.OtMonitor * len(mons))(*[monitor_struct(m) for m in mons])
    return lib.ot_monitor_record_many(ctx, table, len(mons), C.byref(src), n, None if count is None else count.data_ptr(), n_rays, *out.args())


def test_edges():
    table = support.cfg2_table()
    eng = get_engine()
    # one ray, one segment (origin -> lens): the first monitor sees it, the second does not
    mons = [oa.Monitor([2.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 6, 6)]
    for layout in ("slots", "tiled", "append"):
        segs = table.trace_batch(support.batch(*scenes.cfg2_rays(1, 0)), max_segments=1, layout=layout)
        hits = table.record_all(segs, monitors=mons)
        assert (len(hits[0]), len(hits[1])) == (1, 0)
        for m, got in zip(mons, hits):
            _assert_same_hits(got, table.record_batch(m, segs))
    # slot counts of 64 k + 1: 65 slots, and 2,049 = one more than a workgroup's 2,048
    for n, K in ((13, 5), (2049, 1)):
        segs = table.trace_batch(support.batch(*scenes.cfg2_rays(n, 3)), max_segments=K, layout="slots")
        assert segment_source(segs)[1] % 64 == 1
        mons = [oa.Monitor([2.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 6, 6)]
        hits = table.record_all(segs, monitors=mons)
        assert len(hits[0]) >= n  # every ray's first segment, the one in the slot behind the boundary among them
        for m, got in zip(mons, hits):
            _assert_same_hits(got, table.record_batch(m, segs))
    # a list of no segments: empty hits, and through the ABI `first` all zero
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    assert [len(h) for h in table.record_all(none, monitors=mons)] == [0, 0]
    some = SegmentBatch(64, "f64", "cuda")
    some.n_valid = 0
    out = _Outputs(2, 8)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, some, out) == 0
    assert out.first[:3].tolist() == [0, 0, 0] and int(out.total[0]) == 0 and out.guards_untouched()


def test_capacity(case1):
    table, mons, get = case1
    segs, refs = get("slots", "f64")
    eng = get_engine()
    structs = [monitor_struct(m) for m in mons]
    full = eng.monitor_record_many(structs, segs)
    small = eng.monitor_record_many(structs, segs, capacity=64)  # too small: one retry at the exact total
    counts = [len(r) for r in refs]
    assert sum(counts) > 64
    for (s0, P0, t0), (s1, P1, t1), ref in zip(full, small, refs):
        assert torch.equal(s0, s1) and torch.equal(P0, P1) and torch.equal(t0, t1)
        assert torch.equal(torch.sort(s0).values, torch.sort(ref.slot).values)
    # through the ABI with room for half of the hits: exact totals, nothing written behind the buffers
    out = _Outputs(len(mons), sum(counts) // 2)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, mons, segs, out) == 0
    torch.cuda.synchronize()
    assert int(out.total[0]) == sum(counts)
    assert out.first[:len(mons) + 1].tolist() == [0] + list(np.cumsum(counts))
    assert out.guards_untouched()
    everything = torch.cat([s for s, _, _ in full])
    assert torch.equal(out.idx[:out.capacity], everything[:out.capacity])  # what fits is the front of the full result


def test_abi_errors(ctx):
    lib, c = ctx
    n = 130
    segs = SegmentBatch(2 * n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    segs.dx.fill_(1.0)
    segs.length.fill_(10.0)
    segs.ray.copy_(torch.arange(2 * n, dtype=torch.int32) % n)
    segs.count, segs.n_rays = torch.full((n,), 2, dtype=torch.int32, device="cuda"), n
    mon = monitor_struct(oa.Monitor([5, 0, 0], 2, 2))
    out = _Outputs(1, 2 * n)
    src, n_segments, count, n_rays = segment_source(segs)
    assert (n_segments, n_rays) == (2 * n, n)

    def call(mons=C.byref(mon), M=1, source=src, n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, args=None):
        return lib.ot_monitor_record_many(c, mons, M, None if source is None else C.byref(source), n_seg, cnt, rays, *(args or out.args()))

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    expect(lib.ot_monitor_record_many(None, C.byref(mon), 1, C.byref(src), n_segments, count.data_ptr(), n_rays, *out.args()), "NULL")
    expect(call(mons=None), "NULL")
    expect(call(source=None), "NULL")
    for k in range(1, 8):  # first, hit_index, Px, Py, Pz, t, total
        args = list(out.args())
        args[k] = None
        expect(call(args=args), "NULL")
    no_field = altered()
    no_field.base[3] = None
    expect(call(source=no_field), "NULL field")
    expect(call(source=altered(ray=None)), "NULL field")
    expect(call(M=0), "n_monitors")
    expect(call(M=-3), "n_monitors")
    expect(call(n_seg=-1), "segment count")
    expect(call(source=altered(capacity=1 << 32), n_seg=1 << 31, cnt=None, rays=0), "segment count")
    expect(call(source=altered(width=2)), "width")
    expect(call(source=altered(width=16)), "width")
    expect(call(n_seg=n_segments + 1, cnt=None, rays=0), "capacity")
    expect(call(rays=0), "multiple of n_rays")            # seg_count without its n_rays
    expect(call(n_seg=n_segments - 1), "multiple of n_rays")
    expect(call(cnt=None), "n_rays without seg_count")
    assert out.guards_untouched() and bool((out.idx == -7).all())  # nothing was launched
    # the context is still good: every one of the 2 n segments crosses x = 5
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.first[:2].tolist() == [0, 2 * n] and int(out.total[0]) == 2 * n
    assert out.idx[:2 * n].tolist() == list(range(2 * n)) and out.guards_untouched()
    np.testing.assert_allclose(out.real[3][:2 * n].cpu().numpy(), 5.0, **TOL)
