"""GPU (MI355X): the diffraction PSF per ray group — `OpticalTable.psf_grouped_all` / `psf_grouped_batch`
(ot_monitor_psf_groups_many): the hit list of every monitor split by group on the device, stably, by the two partition passes of
k_mon_psf, and its sum run over the cells (monitor, group).

Reference for cell (m, g), in every comparison: tests/psf_reference.py on the segment records copied from the device with
valid = (ids[ray] == g) — the rays of group g alone.  The rule is tests/test_gpu_psf.py's `_assert_psf`: the reference's margin
asserted on the inputs, counts EQUAL, every sample of the field within the reference's own bound."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
import wavefront_cases as cases
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import PSF_PART_TILE as T, get_engine, psf_groups_plan, segment_source
from optable_amd.psf import psf_grid
from optable_amd.table import monitor_struct
from optable_amd.wavefront import wavefront_reference as reference_tables
from psf_reference import airy, disc_grid, psf_reference
from support import ctx  # noqa: F401  (the fixture)
from test_gpu_psf import STEP, _assert_psf, _batch, _records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = scenes.WL
FAR = dict(direction=(1.0, 0.0, 0.0))  # the collimated beam of cfg 2 at x = 7.5


def _far_monitor():
    return oa.Monitor([7.5, 0, 0], 6, 6)


def _reference(rec, mon, kwargs, step, pixels, valid=None, wavelength=WL, centre=(0.0, 0.0), amplitude="sqrt"):
    kind, _, local = reference_tables(kwargs.get("focus"), kwargs.get("direction"), [mon])
    grid, (ny, nz), _, _ = psf_grid(step, pixels, centre, 1)
    s = monitor_struct(mon)
    ref = psf_reference(rec["o"], rec["d"], rec["length"], rec["intensity"], rec["n"], rec["pathlength"], rec["ray"], list(s.M), list(s.origin), s.half_width,
                        s.half_height, cases.axes_of(mon), kind, local[0], grid[0], ny, nz, wavelength, ("sqrt", "linear", "unit").index(amplitude),
                        valid=valid)
    assert ref.margin > cases.MARGIN  # a condition on the inputs
    return ref


def _ids_of(rec, ids, G):
    """The group of every record: ids[ray], -1 where the ray has no entry or the id is no group."""
    ids, ray = np.asarray(ids, dtype=np.int64), rec["ray"]
    known = (ray >= 0) & (ray < len(ids))
    g = np.where(known, ids[np.clip(ray, 0, len(ids) - 1)], -1)
    return np.where((g >= 0) & (g < G), g, -1)


def _assert_groups(p, rec, mon, kwargs, step, pixels, ids, G, groups=None, **kw):
    """Every cell (or those of `groups`) of the `MonitorPSFGroups` p against its reference, `ungrouped` against the masked hits;
    returns the references by group."""
    of = _ids_of(rec, ids, G)
    assert p.n_groups == G and tuple(p.re.shape) == (G,) + tuple(pixels) and p.ungrouped.is_cuda
    refs = {}
    for g in range(G) if groups is None else groups:
        refs[g] = _reference(rec, mon, kwargs, step, pixels, valid=of == g, **kw)
        _assert_psf(p.group(g), refs[g])
    masked = _reference(rec, mon, kwargs, step, pixels, valid=of < 0, **kw)
    assert int(p.ungrouped) == int(masked.counts[0] + masked.counts[1])
    return refs


def _same_bits(a, b):
    return torch.equal(a.re, b.re) and torch.equal(a.im, b.im) and torch.equal(a.norm, b.norm) and torch.equal(a.counts, b.counts) \
        and torch.equal(a.skipped, b.skipped) and torch.equal(a.aliased, b.aliased)


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 130 rays, 5 segments, traced once per layout: (table, get(layout) -> (segs, records))."""
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(130, 3)
    return table, support.traced(table, lambda precision: _batch(o, d, intensity, precision), 5, _records)


# -- 1, 2: layouts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["focus", "direction"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts(case1, layout, setup, monkeypatch):
    table, get = case1
    segs, rec = get(layout)
    su = cases.SETUPS[setup]
    mons = cases.monitors_at(su["x"])
    table.monitors = []
    table.add_monitors(mons)
    ids = np.arange(130) % 3

    def refuse(self, *args, **kwargs):
        raise AssertionError("psf_grouped_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        psfs = table.psf_grouped_all(segs, WL, ids, step=STEP[setup], pixels=(17, 33), labels=["a", "b", "c"], **su["kwargs"])  # the table's own monitors
    assert len(psfs) == len(mons) and all(p.monitor is m for p, m in zip(psfs, mons)) and psfs[0].reference[0] == setup and psfs[0].labels == ["a", "b", "c"]
    for p, m in zip(psfs, mons):
        _assert_groups(p, rec, m, su["kwargs"], STEP[setup], (17, 33), ids, 3)
        assert int(p.ungrouped) == 0
    assert int(psfs[0].counts.sum()) >= 130 and int(psfs[cases.EMPTY].counts.sum()) == 0 and int(psfs[3].counts.min()) > 0
    one = table.psf_grouped_batch(mons[3], segs, WL, ids, step=STEP[setup], pixels=(17, 33), **su["kwargs"])
    assert _same_bits(one, psfs[3])


@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_one_group_is_psf_all(case1, layout):
    """G = 1 and every id 0: the partition copies the list as it is, and every bit is `psf_all`'s."""
    table, get = case1
    segs, _ = get(layout)
    su = cases.SETUPS["direction"]
    mons = cases.monitors_at(su["x"])
    args = dict(step=STEP["direction"], pixels=(17, 33), monitors=mons, **su["kwargs"])
    grouped, plain = table.psf_grouped_all(segs, WL, np.zeros(130, dtype=np.int64), **args), table.psf_all(segs, WL, **args)
    for a, b in zip(grouped, plain):
        assert a.n_groups == 1 and int(a.ungrouped) == 0
        assert torch.equal(a.re[0], b.re) and torch.equal(a.im[0], b.im) and torch.equal(a.norm[0], b.norm)
        assert (int(a.counts[0]), int(a.skipped[0]), int(a.aliased[0])) == (int(b.counts), int(b.skipped), int(b.aliased))


# -- 3: stability ---------------------------------------------------------------------------------------------------------------------------
def test_a_group_alone():
    """In slot layout the hits of group g keep their order, and a cell's chunks follow from its hit count alone: group g of the
    grouped call is bit for bit `psf_all` on a trace of the rays of group g alone.  It fails when the partition is not stable."""
    table = support.cfg2_table()
    n, G = 1027, 3
    batch = _batch(*cases.cfg2_arrays(n, 3))
    ids = np.random.default_rng(11).integers(0, G, n)
    mon = _far_monitor()
    args = dict(step=2e-5, pixels=(19, 21), **FAR)
    segs = table.trace_batch(batch, max_segments=5, layout="slots")
    grouped = table.psf_grouped_batch(mon, segs, WL, ids, **args)
    assert int(grouped.counts.sum()) > T  # more than one tile of the partition, every group in each
    for g in range(G):
        alone = table.trace_batch(batch.take(torch.as_tensor(np.nonzero(ids == g)[0], device="cuda")), max_segments=5, layout="slots")
        want, got = table.psf_batch(mon, alone, WL, **args), grouped.group(g)
        assert int(want.counts) == int(got.counts) > 512
        assert torch.equal(got.re, want.re) and torch.equal(got.im, want.im) and torch.equal(got.norm, want.norm)


# -- 4: the edges of the partition ----------------------------------------------------------------------------------------------------------
def _id_pattern(pattern, n, G, seed=5):
    if pattern == "blocks":
        return np.arange(n) * G // n
    if pattern == "interleaved":
        return np.arange(n) % G
    return np.random.default_rng(seed).integers(0, G, n)


@pytest.mark.parametrize("hits, pattern", [(T - 1, "blocks"), (T, "interleaved"), (T + 1, "random"), (2 * T + 1, "random"), (1, "blocks"), (63, "random"),
                                           (64, "interleaved"), (65, "blocks")])
def test_partition_edges(hits, pattern):
    """One monitor with exactly `hits` hits (asserted on the reference): with three segments a ray every ray of cfg 2 crosses the
    monitor at x = 7.5 once; for 2 T + 1 hits, five segments (two crossings) of T + 1 rays, the last of which keeps three.  A second
    monitor, at x = 2.5 where every ray crosses as often, follows in the concatenated list: its hits start in the middle of what would
    be a tile of that list, and it has tiles of its own."""
    table = support.cfg2_table()
    G = 3
    if hits == 2 * T + 1:
        n = T + 1
        segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=5, layout="slots")
        segs.count[n - 1] = 3
    else:
        n = hits
        segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=3, layout="slots")
    rec = _records(segs)
    ids = _id_pattern(pattern, n, G)
    mons = [_far_monitor(), oa.Monitor([2.5, 0, 0], 6, 6)]
    psfs = table.psf_grouped_all(segs, WL, ids, n_groups=G, step=2e-5, pixels=(9, 20), monitors=mons, **FAR)
    refs = _assert_groups(psfs[0], rec, mons[0], FAR, 2e-5, (9, 20), ids, G)
    assert sum(int(r.counts[0] + r.counts[1]) for r in refs.values()) == hits
    second = _assert_groups(psfs[1], rec, mons[1], FAR, 2e-5, (9, 20), ids, G)
    assert sum(int(r.counts[0] + r.counts[1]) for r in second.values()) == hits


def test_many_groups_most_of_them_empty():
    """G = 256 with all but three groups empty, and an empty group between two full ones (0, 2 full, 1 empty; 255 the third)."""
    table = support.cfg2_table()
    n, G = 1027, 256
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=5, layout="append")
    rec, mon = _records(segs), _far_monitor()
    ids = np.array([0, 2, 255])[np.random.default_rng(2).integers(0, 3, n)]
    p = table.psf_grouped_batch(mon, segs, WL, ids, n_groups=G, step=2e-5, pixels=(9, 11), **FAR)
    refs = _assert_groups(p, rec, mon, FAR, 2e-5, (9, 11), ids, G, groups=[0, 1, 2, 3, 128, 254, 255])
    assert refs[0].counts[0] > 0 and refs[2].counts[0] > 0 and refs[255].counts[0] > 0 and refs[1].counts[0] == 0
    used = p.counts.cpu().numpy()
    assert used[[0, 2, 255]].sum() == used.sum() == sum(int(refs[g].counts[0]) for g in (0, 2, 255)) and not p.re[1].any() and not p.im[3:255].any()


# -- 5, 6: chunks and launches --------------------------------------------------------------------------------------------------------------
def test_a_cell_of_many_chunks_beside_a_cell_of_three_hits():
    table = support.cfg2_table()
    n = 1030
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=3, layout="slots")  # one hit a ray
    rec, mon = _records(segs), _far_monitor()
    ids = np.zeros(n, dtype=np.int64)
    ids[[5, 500, 1029]] = 1
    p = table.psf_grouped_batch(mon, segs, WL, ids, step=2e-5, pixels=(33, 17), **FAR)
    refs = _assert_groups(p, rec, mon, FAR, 2e-5, (33, 17), ids, 2)
    assert refs[0].counts[0] >= 1025 and refs[1].counts[0] == 3
    assert psf_groups_plan(33, 17, [[int(refs[0].counts[0]), 3]])["chunks"] == [[3, 1]]


def test_more_than_one_launch():
    """2 monitors x 256 groups x four tiles of 65 x 65 samples: 2,048 pairs, more than a launch's partial rows hold."""
    table = support.cfg2_table()
    n, G = 520, 256
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=3, layout="slots")
    rec = _records(segs)
    mons = [_far_monitor(), _far_monitor().RotZ(0.1)]
    ids = np.arange(n) % G
    psfs = table.psf_grouped_all(segs, WL, ids, step=2e-5, pixels=(65, 65), monitors=mons, **FAR)
    cell_hits = [[int(v) for v in (p.counts + p.skipped).cpu()] for p in psfs]
    plan = psf_groups_plan(65, 65, cell_hits)
    assert plan["pairs_a_launch"] < 2 * G * 4 and plan["launches"] > 1
    for p, m in zip(psfs, mons):
        refs = _assert_groups(p, rec, m, FAR, 2e-5, (65, 65), ids, G, groups=[0, 7, 255])
        assert all(r.counts[0] >= 2 for r in refs.values())
        assert int(p.counts.sum()) == int(_reference(rec, m, FAR, 2e-5, (3, 3)).counts[0])


# -- 7: masking -----------------------------------------------------------------------------------------------------------------------------
def test_masking(case1):
    table, get = case1
    segs, rec = get("tiled")
    mon = _far_monitor()
    everything = len(table.record_all(segs, monitors=[mon])[0])
    args = dict(step=2e-5, pixels=(17, 33), **FAR)

    def check(p, ids, G):
        _assert_groups(p, rec, mon, FAR, 2e-5, (17, 33), ids, G)
        assert int(p.counts.sum()) + int(p.skipped.sum()) + int(p.ungrouped) == everything
        return int(p.ungrouped)

    ids = np.arange(130) % 3
    ids[::7] = -1
    assert check(table.psf_grouped_batch(mon, segs, WL, ids, **args), ids, 3) > 0
    ids = np.arange(130) % 5
    assert check(table.psf_grouped_batch(mon, segs, WL, ids, n_groups=3, **args), ids, 3) > 0  # ids 3 and 4 are no groups
    # a table shorter than the batch, through the engine: rays 100 .. 129 have no entry
    kind, _, local = reference_tables(None, (1.0, 0.0, 0.0), [mon])
    grid, pixels, step, centres = psf_grid(2e-5, (17, 33), (0.0, 0.0), 1)
    short = torch.as_tensor(np.arange(100) % 3, dtype=torch.int32, device="cuda")
    counts, norm, re, im, ungrouped = get_engine().monitor_psf_groups_many([monitor_struct(mon)], cases.axes_of(mon).reshape(1, 6), kind, local, grid, pixels,
                                                                           short, 3, segs, WL)
    got = oa.MonitorPSFGroups(mon, counts[0], norm[0], re[0], im[0], ungrouped[0], ("direction", (1.0, 0.0, 0.0)), grid[0], step, centres[0], "sqrt")
    assert check(got, np.arange(100) % 3, 3) >= 30
    nothing = table.psf_grouped_batch(mon, segs, WL, np.full(130, -1), n_groups=2, **args)
    assert int(nothing.ungrouped) == everything and not nothing.counts.any() and not nothing.re.any() and not nothing.im.any() and not nothing.norm.any()
    assert torch.isnan(nothing.normalised()).all() and math.isnan(float(nothing.strehl()))


# -- 8, 9: trees, per-ray wavelengths -----------------------------------------------------------------------------------------------------------
def test_trees():
    """The scene of tests/test_gpu_psf.py::test_lists_and_trees: children carry their input ray's group."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    kwargs = dict(direction=(1.0, 0.2, 0.0))
    eng = get_engine()
    eng.upload(table.compile())
    table_wl = batch.wavelength.double().cpu().numpy()
    ids = np.arange(320) % 4
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        rec = _records(segs)
        for p, m in zip(table.psf_grouped_all(segs, batch, ids, step=2e-6, pixels=(17, 18), monitors=mons, **kwargs), mons):
            refs = _assert_groups(p, rec, m, kwargs, 2e-6, (17, 18), ids, 4, wavelength=table_wl)
            assert all(r.counts[0] > 80 for r in refs.values())  # every tree crosses each monitor, most of them more than once


def test_per_ray_wavelengths_and_a_ray_without_one(case1):
    table, get = case1
    segs, rec = get("append")  # the segments of 130 rays; the wavelengths and groups of a batch multiplexed 2 x 65 rays
    mon = _far_monitor()
    o, d, intensity = cases.cfg2_arrays(65, 3)
    both = _batch(o, d, intensity[:65]).multiplexed_in_wavelength([WL, 1.5 * WL])
    ids, found = both.groups_by_wavelength()
    assert found.tolist() == [WL, 1.5 * WL] and ids.tolist() == [0] * 65 + [1] * 65
    wl = both.wavelength.double().cpu().numpy()
    p = table.psf_grouped_batch(mon, segs, both, ids, step=2e-5, pixels=(17, 33), labels=found.tolist(), **FAR)
    _assert_groups(p, rec, mon, FAR, 2e-5, (17, 33), ids.cpu().numpy(), 2, wavelength=wl)
    wl[7], wl[99] = 0.0, np.nan  # unusable: skipped in group 0 and in group 1 (through the engine: psf_grouped_all refuses such a batch)
    kind, _, local = reference_tables(None, (1.0, 0.0, 0.0), [mon])
    grid, pixels, step, centres = psf_grid(2e-5, (17, 33), (0.0, 0.0), 1)
    counts, norm, re, im, ungrouped = get_engine().monitor_psf_groups_many([monitor_struct(mon)], cases.axes_of(mon).reshape(1, 6), kind, local, grid, pixels,
                                                                           ids, 2, segs, torch.as_tensor(wl, device="cuda"))
    got = oa.MonitorPSFGroups(mon, counts[0], norm[0], re[0], im[0], ungrouped[0], ("direction", (1.0, 0.0, 0.0)), grid[0], step, centres[0], "sqrt")
    refs = _assert_groups(got, rec, mon, FAR, 2e-5, (17, 33), ids.cpu().numpy(), 2, wavelength=wl)
    assert refs[0].counts[1] >= 1 and refs[1].counts[1] >= 1 and got.skipped.tolist() == [int(refs[0].counts[1]), int(refs[1].counts[1])]


# -- 10, 11: determinism, streaming -------------------------------------------------------------------------------------------------------------
def test_determinism_and_streaming():
    table = support.cfg2_table()
    n, G = 1027, 4
    o, d, intensity = cases.cfg2_arrays(n, 3)
    ids = np.random.default_rng(4).integers(0, G, n)
    su = cases.SETUPS["direction"]
    mons = cases.monitors_at(su["x"])
    args = dict(step=2e-5, pixels=(33, 65), monitors=mons, **su["kwargs"])
    for layout in ("slots", "append"):
        segs = table.trace_batch(_batch(o, d, intensity), max_segments=5, layout=layout)
        a, b = (table.psf_grouped_all(segs, WL, ids, **args) for _ in range(2))
        for x, y in zip(a, b):
            assert _same_bits(x, y) and torch.equal(x.ungrouped, y.ungrouped) and x.re is not y.re
    rec = _records(segs)
    cut = (slice(0, 600), slice(600, None))
    half = [table.trace_batch(_batch(o[s], d[s], intensity[s]), max_segments=5, layout="slots") for s in cut]
    first = table.psf_grouped_all(half[0], WL, ids[cut[0]], n_groups=G, **args)
    part = [p.counts.clone() for p in first]
    again = table.psf_grouped_all(half[1], WL, ids[cut[1]], n_groups=G, into=first, **args)  # the second half's own ids
    assert all(x is y for x, y in zip(again, first))
    for p, m, k in zip(first, mons, part):
        refs = _assert_groups(p, rec, m, su["kwargs"], 2e-5, (33, 65), ids, G)
        assert bool((k <= p.counts).all()) and p.counts.tolist() == [int(refs[g].counts[0]) for g in range(G)]
    with pytest.raises(ValueError, match="into"):
        table.psf_grouped_all(half[1], WL, ids[cut[1]], n_groups=G + 1, into=first, **args)
    with pytest.raises(ValueError, match="into"):
        table.psf_grouped_all(half[1], WL, ids[cut[1]], n_groups=G, into=first, **{**args, "pixels": (33, 33)})


# -- 12: the C ABI ------------------------------------------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / norm / re / im / ungrouped of M monitors x G groups of ny x nz samples, with a guard region on either side of each."""

    def __init__(self, M, G, ny, nz):
        field = (torch.float64, (M, G, ny, nz))
        super().__init__(guard=64, counts=(torch.int64, (M, G, 3)), norm=(torch.float64, (M, G)), re=field, im=field, ungrouped=(torch.int64, (M,)))


def test_abi_errors(ctx):
    lib, c = ctx
    n = 130
    segs = SegmentBatch(2 * n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    segs.dx.fill_(1.0)
    segs.length.fill_(10.0)
    segs.intensity.fill_(0.25)
    segs.field("n").fill_(1.0)
    segs.pathlength.fill_(0.25)
    segs.ray.copy_(torch.arange(2 * n, dtype=torch.int32) % n)
    segs.count, segs.n_rays = torch.full((n,), 2, dtype=torch.int32, device="cuda"), n
    m = oa.Monitor([5, 0, 0], 2, 2)
    mon = monitor_struct(m)
    ny, nz, G = 5, 18, 2
    out = _Out(1, G, ny, nz)
    src, n_segments, count, n_rays = segment_source(segs)
    good_axes, good_ref, good_grid = cases.axes_of(m).reshape(1, 6), np.array([[1.0, 0.0, 0.0]]), np.array([[-2e-5, 1e-5, -8.5e-5, 1e-5]])
    wl = torch.full((n,), 0.5, dtype=torch.float64, device="cuda")
    ids = (torch.arange(n, dtype=torch.int32, device="cuda") % 3) - 1  # -1, 0, 1: 44 rays masked, 43 in each group
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, kind=1, ref=good_ref, grid=good_grid, ny_=ny, nz_=nz, groups=ids.data_ptr(), n_ids=n, G_=G,
             source=src, intensity=segs.intensity.data_ptr(), n_index=segs.field("n").data_ptr(), pathlength=segs.pathlength.data_ptr(), wavelength=None,
             n_wl=0, uniform=0.5, mode=0, n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(), norm=out.norm.data_ptr(),
             re=out.re.data_ptr(), im=out.im.data_ptr(), ungrouped=out.ungrouped.data_ptr(), acc=0):
        return lib.ot_monitor_psf_groups_many(ctx_, mons, M, ptr(axes), kind, ptr(ref), ptr(grid), ny_, nz_, groups, n_ids, G_,
                                              None if source is None else C.byref(source), intensity, n_index, pathlength, wavelength, n_wl, uniform, mode, n_seg,
                                              cnt, rays, counts, norm, re, im, ungrouped, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    def with_value(good, at, value):
        a = good.copy()
        a.flat[at] = value
        return a

    # everything the ungrouped call refuses ...
    for null in ("ctx_", "mons", "axes", "ref", "grid", "source", "n_index", "pathlength", "counts", "norm", "re", "im", "intensity"):
        expect(call(**{null: None}), "NULL")
    no_field = altered()
    no_field.base[3] = None
    expect(call(source=no_field), "NULL field")
    for M in (0, -3, (1 << 20) + 1):
        expect(call(M=M), "n_monitors")
    for kind in (2, -1):
        expect(call(kind=kind), "reference_kind")
    for bad in (0, -1, 513):
        expect(call(ny_=bad), "ny and nz")
        expect(call(nz_=bad), "ny and nz")
    for mode in (-1, 3):
        expect(call(mode=mode), "amplitude_mode")
    expect(call(acc=2), "accumulate")
    expect(call(n_seg=-1), "segment count")
    expect(call(source=altered(width=4)), "double-precision")
    expect(call(source=altered(width=2)), "width")
    expect(call(n_seg=n_segments + 1, cnt=None, rays=0), "capacity")
    expect(call(rays=0), "multiple of n_rays")
    expect(call(cnt=None), "n_rays without seg_count")
    expect(call(axes=with_value(good_axes, 1, np.nan)), "axes")
    expect(call(ref=with_value(good_ref, 2, np.inf)), "reference")
    expect(call(ref=np.zeros((1, 3))), "zero")
    expect(call(grid=with_value(good_grid, 0, np.nan)), "grid")
    expect(call(grid=with_value(good_grid, 3, np.inf)), "grid")
    for at in (1, 3):
        for step in (0.0, -1e-5):
            expect(call(grid=with_value(good_grid, at, step)), "steps")
    for uniform in (0.0, -0.5, np.nan, np.inf):
        expect(call(uniform=uniform), "wavelength_uniform")
    expect(call(wavelength=wl.data_ptr(), n_wl=0), "n_wavelengths")
    # ... and what the groups add
    expect(call(groups=None), "NULL")
    expect(call(ungrouped=None), "NULL")
    for bad in (0, -1, 257):
        expect(call(G_=bad), "n_groups")
    for bad in (0, -5, 1 << 31):
        expect(call(n_ids=bad), "n_group_ids")
    many = (abi.OtMonitor * 17)(*([mon] * 17))
    tables = dict(mons=many, M=17, axes=np.tile(good_axes, (17, 1)), ref=np.tile(good_ref, (17, 1)), grid=np.tile(good_grid, (17, 1)))
    expect(call(G_=256, **tables), "4096 cells")  # 17 x 256 = 4352 cells
    expect(call(G_=256, ny_=512, nz_=512, **{**tables, "mons": (abi.OtMonitor * 3)(*([mon] * 3)), "M": 3}), "2^27")  # 3 x 256 x 2^18 samples
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good: each of the 2 n segments crosses the monitor at x = 5; every sample of a group is -0.5 a hit, exactly
    # (tests/test_gpu_psf.py::test_abi_errors): 2 x 43 hits in either group, 2 x 44 in none
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.counts[0].tolist() == [[86, 0, 0], [86, 0, 0]] and out.norm[0].tolist() == [43.0, 43.0] and out.ungrouped.tolist() == [88] and out.guards_untouched()
    assert bool((out.re == -43.0).all()) and float(out.im.abs().max()) <= 43.0 * 2.0**-50
    assert call(acc=1, wavelength=wl.data_ptr(), n_wl=n, uniform=0.0) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    assert out.counts[0].tolist() == [[172, 0, 0], [172, 0, 0]] and out.ungrouped.tolist() == [176] and bool((out.re == -86.0).all())
    assert call(n_seg=0, cnt=None, rays=0) == 0 and lib.ot_ctx_synchronize(c) == 0  # no segments: zeros
    assert not out.counts.any() and not out.norm.any() and not out.re.any() and not out.ungrouped.any() and out.guards_untouched()


def test_single_precision_is_refused():
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(130, 3)
    segs = table.trace_batch(_batch(o, d, intensity, precision="f32"), max_segments=3)
    assert segs.precision == "f32"
    mon, ids = _far_monitor(), np.zeros(130, dtype=np.int64)
    with pytest.raises(ValueError, match="double-precision"):
        table.psf_grouped_all(segs, WL, ids, direction=(1, 0, 0), step=2e-5, monitors=[mon])
    with pytest.raises(ValueError, match="double-precision"):
        get_engine().monitor_psf_groups_many([monitor_struct(mon)], np.array([[0, 1, 0, 0, 0, 1.0]]), 1, np.array([[1.0, 0, 0]]), np.array([[0, 1e-5, 0, 1e-5]]),
                                             (3, 3), torch.zeros(130, dtype=torch.int32, device="cuda"), 1, segs, WL)


# -- 13: physics on the device --------------------------------------------------------------------------------------------------------------
def test_two_wavelengths_give_two_airy_patterns_and_their_mean():
    """The 1,257-ray NA 0.1 cone of tests/test_gpu_psf.py::test_a_converging_cone_gives_the_airy_pattern, multiplexed to WL and
    1.5 WL, on that test's grid: each group is the Airy pattern of its own wavelength and the unweighted incoherent sum their mean,
    to that test's 5e-3 of the peak (the reference alone: 1.86e-3 and 1.88e-3 at 1 and 1.5 WL, 1.03e-3 for the mean); every Strehl
    ratio 1 within the bound."""
    NA, F = 0.1, np.array([30.0, 0.0, 0.0])
    t = disc_grid(41, NA)
    d = np.stack([np.sqrt(1.0 - (t * t).sum(axis=1)), t[:, 0], t[:, 1]], axis=1)
    table = support.cfg2_table()
    batch = RayBatch.from_arrays(F - 2.0 * d, d, wavelength=WL, device="cuda").multiplexed_in_wavelength([WL, 1.5 * WL])
    segs = table.trace_batch(batch, max_segments=2, layout="slots")
    mon = oa.Monitor([29.0, 0, 0], 1, 1)
    step = 6 * 0.61 * WL / NA / 32
    ids, found = batch.groups_by_wavelength()
    p = table.psf_grouped_batch(mon, segs, batch, ids, focus=F, step=step, pixels=33, labels=found.tolist())
    lam = batch.wavelength.double().cpu().numpy()
    refs = _assert_groups(p, _records(segs), mon, dict(focus=F), step, (33, 33), ids.cpu().numpy(), 2, wavelength=lam)
    assert refs[0].counts.tolist() == refs[1].counts.tolist() == [1257, 0, 0] and int(p.ungrouped) == 0
    r = np.hypot(p.y[:, None], p.z[None, :])
    patterns = [airy(2 * np.pi * NA * r / w) for w in (WL, 1.5 * WL)]
    for g in range(2):
        err = float(np.abs(p.group(g).normalised().cpu().numpy() - patterns[g]).max())
        print(f"  Airy pattern at {found[g]:.3e}: largest error {err:.3g} of the peak")
        assert err <= 5e-3
    err = float(np.abs(p.normalised().cpu().numpy() - 0.5 * (patterns[0] + patterns[1])).max())
    print(f"  mean of the two patterns: largest error {err:.3g} of the peak")
    assert err <= 5e-3
    slack = max(refs[g].bound / refs[g].norm for g in range(2))
    for s in (*p.strehls().tolist(), float(p.strehl()), float(p.strehl("peak"))):
        assert (1 - slack) ** 2 <= s <= (1 + slack) ** 2


# -- 14 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "polychromatic_psf.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split(":")[0].strip(): ln for ln in out.stdout.splitlines() if ":" in ln}
    assert "polychromatic Strehl" in lines and "psf_all Strehl" in lines and "polychromatic MTF" in lines, out.stdout
    strehl = float(lines["polychromatic Strehl"].split(":")[1].split()[0])
    assert 0.0 < strehl <= 1.0, out.stdout
