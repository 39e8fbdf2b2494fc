"""GPU (MI355X): wavefront error per ray group — `OpticalTable.wavefront_grouped_all` / `wavefront_grouped_batch`, the 61 moments of
every (monitor, group) from one pass per 28 cells by the wavefront mode's group mode of k_mon_spots
(ot_monitor_wavefront_groups_many), with reference, pupil and piston per cell.

Reference, as in tests/test_gpu_wavefront.py: tests/wavefront_reference.py on the segment records copied from the device, here on
the records whose input ray has the cell's id, with the cell's own tables (tests/wavefront_group_cases.py).  Every cell first
asserts, from the REFERENCE, that no decision lies within 1e-7 of its boundary; counts must then be EQUAL and every sum within the
reference's derived `bound`, coefficients and rms within what those bounds allow (`_assert_wavefront` of the ungrouped tests).
Bit-for-bit statements (one group is the ungrouped call; a group is its masked call) are torch.equal."""
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
import wavefront_group_cases as gc
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine, segment_source, wavefront_groups_plan
from optable_amd.table import monitor_struct
from support import ctx  # noqa: F401  (the fixture)
from test_gpu_wavefront import _assert_wavefront, _batch, _cone, _hand_batch
from wavefront_reference import U, coefficient_bound, rms_interval

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = gc.G


def _records(segs):
    """(records, ray): the valid segment records of a batch copied from the device, and the input ray of each."""
    *records, ray = support.host_records(segs, "n", "pathlength", "ray")
    return tuple(records), ray


def _assert_cells(wfs, refs):
    for wfg, row in zip(wfs, refs):
        assert wfg.n_groups == len(row) and wfg.counts.is_cuda and wfg.sums.shape == (len(row), 61)
        for g, ref in enumerate(row):
            _assert_wavefront(wfg.group(g), ref)


def _same_bits(a, b):
    return torch.equal(a.counts, b.counts) and torch.equal(a.outside, b.outside) and torch.equal(a.sums, b.sums)


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 4,096 rays x 5 segments, traced once per layout: (table, get(layout) -> (segs, (records, ray)), ids)."""
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(gc.RAYS, gc.SEED)
    return table, support.traced(table, lambda precision: _batch(o, d, intensity, precision), gc.SEGMENTS, _records), gc.ids_of(gc.RAYS)


# -- 1: against the numpy reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["focus", "direction"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_against_the_reference(case1, layout, setup, monkeypatch):
    """G = 5 on two monitors, a reference per group and a pupil per cell with centres of their own, ids -1 (masked) .. 5 (>= G: in
    no cell either), both coordinates."""
    table, get, ids = case1
    segs, (records, ray) = get(layout)
    su = gc.SETUPS[setup]
    mons = gc.monitors_at(su["x"])

    def refuse(self, *args, **kwargs):
        raise AssertionError("wavefront_grouped_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        wfs = table.wavefront_grouped_all(segs, ids, n_groups=G, pupil=su["pupil"], monitors=mons, labels=list("abcde"), **{su["name"]: su["reference"]})
    assert len(wfs) == 2 and all(wf.monitor is m for wf, m in zip(wfs, mons)) and wfs[0].labels == list("abcde")
    assert wfs[0].coordinates == ("direction" if setup == "focus" else "position") and wfs[0].reference[0] == setup
    pistons = [wf.piston for wf in wfs]
    refs = gc.cell_references(records, ray, ids, mons, su["name"], su["reference"], su["pupil"], pistons, G)
    _assert_cells(wfs, refs)
    assert all(ref.counts[0] > 400 for row in refs for ref in row) and refs[0][0].counts[1] > 0  # every cell is hit; the first pupil clips
    member = sum(int(ref.counts.sum()) for ref in refs[0])
    everything = table.wavefront_batch(mons[0], segs, pupil=su["pupil"][0][0], piston=0.0, **{su["name"]: su["reference"][0]})
    assert 0 < member < int(everything.counts + everything.outside)  # the ids -1 and 5 are in no cell, and no tally of them is kept
    # the other coordinates on the first monitor, with a piston per group
    other = "position" if setup == "focus" else "direction"
    piston = np.linspace(2.0, 3.0, G)
    one = table.wavefront_grouped_batch(mons[0], segs, ids, n_groups=G, pupil=su["other"], coordinates=other, piston=piston, **{su["name"]: su["reference"]})
    assert np.array_equal(one.piston, piston) and one.coordinates == other
    _assert_cells([one], gc.cell_references(records, ray, ids, mons[:1], su["name"], su["reference"], [su["other"]], [piston], G, coordinates=other))


# -- 2, 3: the bit-for-bit statements --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_one_group_is_the_ungrouped_call_bit_for_bit(case1, layout):
    table, get, _ = case1
    segs = get(layout)[0]
    for setup, su in cases.SETUPS.items():
        mons = cases.monitors_at(su["x"])
        piston = [3.0, 2.5, 0.0, 2.75]
        plain = table.wavefront_all(segs, pupil=su["pupil"], monitors=mons, piston=piston, **su["kwargs"])
        grouped = table.wavefront_grouped_all(segs, np.zeros(gc.RAYS, dtype=np.int32), n_groups=1, pupil=su["pupil"], monitors=mons, piston=piston,
                                              **su["kwargs"])
        for a, b in zip(plain, grouped):
            assert b.n_groups == 1 and int(a.counts) + int(a.outside) == int(b.counts[0]) + int(b.outside[0])
            assert torch.equal(a.counts, b.counts[0]) and torch.equal(a.outside, b.outside[0]) and torch.equal(a.sums, b.sums[0])
        assert int(plain[0].counts) > 0 and int(plain[1].outside) > 0


def _masked_calls(table, segs, ids, mons, name, reference, pupil, piston, n_groups, **kw):
    """[g] -> the G = 1 call over `mons` with the ids (id == g ? 0 : -1) and the tables [:, g] of (reference, pupil, piston) [M, G, ...]."""
    out = []
    for g in range(n_groups):
        out.append(table.wavefront_grouped_all(segs, np.where(ids == g, 0, -1).astype(np.int32), n_groups=1, pupil=pupil[:, g], monitors=mons,
                                               piston=piston[:, g], **{name: reference[:, g]}, **kw))
    return out


def _assert_groups_are_their_masked_calls(wfs, masked):
    for g, alone in enumerate(masked):
        for wfg, one in zip(wfs, alone):
            assert torch.equal(wfg.counts[g], one.counts[0]) and torch.equal(wfg.outside[g], one.outside[0]), g
            assert torch.equal(wfg.sums[g], one.sums[0]), g


@pytest.mark.parametrize("layout", ["slots", "append"])
def test_a_group_is_its_masked_call_bit_for_bit(case1, layout):
    table, get, ids = case1
    segs = get(layout)[0]
    for su in gc.SETUPS.values():
        mons = gc.monitors_at(su["x"])
        reference = np.broadcast_to(su["reference"], (2, G, 3))
        piston = np.array([np.linspace(2.0, 3.0, G), np.linspace(7.0, 8.0, G)])
        wfs = table.wavefront_grouped_all(segs, ids, n_groups=G, pupil=su["pupil"], monitors=mons, piston=piston, **{su["name"]: reference})
        _assert_groups_are_their_masked_calls(wfs, _masked_calls(table, segs, ids, mons, su["name"], reference, su["pupil"], piston, G))
        assert int(wfs[0].counts.min()) > 0


# -- 4: many groups in one wave ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["a group per lane", "alternating", "a masked wave", "outside the window"])
def test_many_groups_in_one_wave(arrangement):
    """Hand-made batches, one segment per ray from a point source to a monitor, referenced per group to a focus of its own:
    64 groups in one wave (three launch windows); ids alternating 0, 1, 2 along the lanes; a wave all masked between two that are
    not; and a wave whose only hits belong to group 40, outside the first and the third window of 64 groups."""
    n = {"a group per lane": 64, "alternating": 200, "a masked wave": 192, "outside the window": 128}[arrangement]
    o, d, intensity = _cone(n, 0.15, 23)
    segs = _hand_batch(o, d, 9.0, intensity, pathlength=0.5)
    lane = np.arange(n)
    ids = {"a group per lane": lane, "alternating": lane % 3, "a masked wave": np.where((lane >= 64) & (lane < 128), -1, lane % 2),
           "outside the window": np.where(lane < 64, lane, 40)}[arrangement].astype(np.int32)
    n_groups = int(ids.max()) + 1
    mon = oa.Monitor([3.0, 0, 0], 4, 4)
    g_ = np.arange(n_groups, dtype=float)
    focus = np.stack([0.001 * g_, 0.0005 * g_, -0.0002 * g_], axis=1)
    pupil = np.stack([0.0 * g_, 0.001 * g_, 0.1 + 0.001 * g_], axis=1)  # (0.1: a third of the cone of 0.15 falls outside)
    piston = 0.5 + 0.001 * g_
    table = oa.OpticalTable()
    wf = table.wavefront_grouped_batch(mon, segs, ids, n_groups=n_groups, focus=focus, pupil=pupil, piston=piston)
    records, ray = _records(segs)
    refs = gc.cell_references(records, ray, ids, [mon], "focus", focus, [pupil], [piston], n_groups)
    _assert_cells([wf], refs)
    assert int(wf.counts.sum() + wf.outside.sum()) == int((ids >= 0).sum())
    if arrangement == "a group per lane":
        assert len(wavefront_groups_plan(1, 64)) == 3 and (wf.counts + wf.outside).tolist() == [1] * 64
    if arrangement == "outside the window":
        assert int(wf.counts[40] + wf.outside[40]) == 65 and int(wf.counts[40]) > 1
    masked = _masked_calls(table, segs, ids, [mon], "focus", focus[None], pupil[None], piston[None], n_groups)
    _assert_groups_are_their_masked_calls([wf], masked)


# -- 5: launch windows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n_groups,plan", [(1, 28, [(0, 28)]), (1, 29, [(0, 28), (28, 1)]), (6, 5, [(0, 28), (28, 2)]),
                                             (1, 256, [(28 * k, min(28, 256 - 28 * k)) for k in range(10)]), (3, 28, [(0, 28), (28, 28), (56, 28)])])
def test_launch_windows(case1, M, n_groups, plan):
    """Windows of 28 consecutive cells of [m][g]: full, a second launch of one cell, a monitor split between two launches, ten
    launches, and boundaries on monitor boundaries.  Every cell against its masked call, bit for bit (which
    test_a_group_is_its_masked_call_bit_for_bit and test_against_the_reference tie to the reference), and the cells on either side
    of every boundary against the reference itself."""
    assert wavefront_groups_plan(M, n_groups) == plan
    table, get, _ = case1
    segs, (records, ray) = get("slots")
    ids = gc.ids_of(gc.RAYS, seed=M * 1000 + n_groups, low=-1, high=n_groups + 1)
    mons, pupils = cases.group_monitors()
    mons, g_ = mons[:M], np.arange(n_groups, dtype=float)
    pupil = np.array([np.stack([p[0] + 0.0002 * g_, p[1] - 0.0001 * g_, p[2] + 0.0005 * g_], axis=1) for p in pupils[:M]])
    reference = np.broadcast_to(np.stack([1.0 + 0.0 * g_, 0.00001 * g_, 0.0 * g_], axis=1), (M, n_groups, 3))
    piston = 5.0 + 0.01 * np.arange(M)[:, None] + 0.001 * g_[None, :]
    wfs = table.wavefront_grouped_all(segs, ids, n_groups=n_groups, pupil=pupil, monitors=mons, piston=piston, direction=reference)
    _assert_groups_are_their_masked_calls(wfs, _masked_calls(table, segs, ids, mons, "direction", reference, pupil, piston, n_groups))
    edges = sorted({c for first, cells in plan for c in (first, first + cells - 1)})
    for cell in edges:
        m, g = divmod(cell, n_groups)
        ref = gc.cell_reference(records, ray, ids, g, mons[m], "direction", reference[m, g], pupil[m, g], float(piston[m, g]))
        _assert_wavefront(wfs[m].group(g), ref)
        assert ref.counts.sum() > 0
    assert sum(int(wf.counts.sum() + wf.outside.sum()) for wf in wfs) > 0


# -- 6: ray trees and lists --------------------------------------------------------------------------------------------------------
def test_a_half_mirror():
    """support.half_mirror: ids by input ray — every segment of a ray's tree lands in its group."""
    table = support.table_of(support.half_mirror(oa))
    n = 1003
    ids = np.random.default_rng(47).integers(-1, 4, n).astype(np.int32)  # {-1, 0, 1, 2, 3}, G = 3: -1 and 3 are masked
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 5)), max_segments=6)
    records, ray = _records(segs)
    assert ray.min() == 0 and ray.max() == n - 1 and len(ray) > 2 * n
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([2.5, 0, 0], 6, 6)]
    direction = np.array([[1.0, 0.0, 0.0], [1.0, 0.001, 0.0], [1.0, 0.0, -0.001]])
    pupil = np.array([[0.0, 0.0, 0.8], [0.01, 0.0, 0.7], [0.0, -0.01, 0.6]])
    wfs = table.wavefront_grouped_all(segs, ids, n_groups=3, direction=direction, pupil=pupil, monitors=mons)
    refs = gc.cell_references(records, ray, ids, mons, "direction", direction, [pupil, pupil], [wf.piston for wf in wfs], 3)
    _assert_cells(wfs, refs)
    assert all(ref.counts.sum() > 0 for row in refs for ref in row)


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (every hit splits): the [k][tree] slots with count[i], the append block and the
    dense list with holes — the `ray` of every node is its tree."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    ids = (np.arange(320) % 7 - 1).astype(np.int32)  # -1 .. 5, G = 5: -1 and 5 are masked
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    direction = np.stack([np.ones(G), 0.2 + 0.01 * np.arange(G), np.zeros(G)], axis=1)
    pupil = np.array([np.stack([0.01 * np.arange(G), np.zeros(G), 1.5 + 0.0 * np.arange(G)], axis=1),
                      np.stack([0.1 + 0.0 * np.arange(G), 0.01 * np.arange(G), 2.0 + 0.0 * np.arange(G)], axis=1)])
    eng = get_engine()
    eng.upload(table.compile())
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        records, ray = _records(segs)
        assert ray.min() == 0 and ray.max() == 319 and len(ray) > 2 * 320
        wfs = table.wavefront_grouped_all(segs, ids, n_groups=G, direction=direction, pupil=pupil, monitors=mons)
        refs = gc.cell_references(records, ray, ids, mons, "direction", direction, pupil, [wf.piston for wf in wfs], G)
        _assert_cells(wfs, refs)
        assert all(ref.counts.sum() >= 45 for row in refs for ref in row)  # every tree of a group crosses each monitor


# -- 7: piston=None ----------------------------------------------------------------------------------------------------------------
def test_piston_none(case1):
    """The two-call scheme per cell: the pistons are the means T00 / S00 of the pass with piston 0 (0 for an empty cell), the result
    is the explicit call's with them, and each is the cell's weighted mean of W by the reference, within its bound."""
    table, get, ids = case1
    segs, (records, ray) = get("tiled")
    su = gc.SETUPS["direction"]
    mons = gc.monitors_at(su["x"]) + [oa.Monitor([su["x"], 40, 0], 6, 6)]  # the third sees nothing
    pupil = np.concatenate([su["pupil"], su["pupil"][:1]])
    kw = dict(n_groups=G + 1, pupil=np.concatenate([pupil, pupil[:, :1]], axis=1), monitors=mons,
              direction=np.concatenate([su["reference"], su["reference"][:1]]))  # group 5 = the id in no cell before; G + 1 groups now
    ids = np.where(ids == 2, -1, ids).astype(np.int32)  # ... and group 2 is empty
    auto = table.wavefront_grouped_all(segs, ids, **kw)
    zero = table.wavefront_grouped_all(segs, ids, piston=0.0, **kw)
    same = table.wavefront_grouped_all(segs, ids, piston=np.array([wf.piston for wf in auto]), **kw)
    for m, (a, z, s) in enumerate(zip(auto, zero, same)):
        zs = z.sums.cpu().numpy()
        with np.errstate(all="ignore"):
            assert np.array_equal(a.piston, np.where(zs[:, 0] != 0.0, zs[:, 45] / zs[:, 0], 0.0))
        assert _same_bits(a, s) and torch.equal(a.counts, z.counts) and torch.equal(a.sums[:, :45], z.sums[:, :45])
        for g in range(G + 1):
            if m == 2 or g == 2:  # empty cells: piston 0 and NaN fits
                assert int(a.counts[g]) == 0 and a.piston[g] == 0.0 and not a.sums[g].any()
                assert torch.isnan(a.coefficients()[g]).all() and math.isnan(float(a.rms()[g])) and math.isnan(float(a.mean()[g]))
                continue
            ref = gc.cell_reference(records, ray, ids, g, mons[m], "direction", kw["direction"][g], kw["pupil"][m, g], 0.0)
            mean = ref.sums[45] / ref.sums[0]
            allowed = (ref.bound[45] + abs(mean) * ref.bound[0]) / (ref.sums[0] - ref.bound[0]) + 2 * U * abs(mean)
            assert abs(a.piston[g] - mean) <= allowed, (m, g, a.piston[g] - mean, allowed)
            _assert_wavefront(a.group(g), gc.cell_reference(records, ray, ids, g, mons[m], "direction", kw["direction"][g], kw["pupil"][m, g],
                                                            float(a.piston[g])))


# -- 8: determinism and streaming --------------------------------------------------------------------------------------------------
def test_determinism_and_streaming(case1):
    table, get, ids = case1
    su = gc.SETUPS["focus"]
    mons = gc.monitors_at(su["x"])
    kw = dict(n_groups=G, pupil=su["pupil"], monitors=mons, focus=su["reference"])
    for layout in ("slots", "append"):
        segs = get(layout)[0]
        a, b = (table.wavefront_grouped_all(segs, ids, **kw) for _ in range(2))
        assert all(_same_bits(x, y) and np.array_equal(x.piston, y.piston) and x.sums is not y.sums for x, y in zip(a, b))
    o, d, intensity = cases.cfg2_arrays(gc.RAYS, gc.SEED)
    _, (records, ray) = get("slots")
    parts = (slice(0, 2000), slice(2000, None))
    half = [table.trace_batch(_batch(o[s], d[s], intensity[s]), max_segments=gc.SEGMENTS, layout="slots") for s in parts]
    first = table.wavefront_grouped_all(half[0], ids[parts[0]], **kw)  # every chunk brings its own ids
    pistons = [wf.piston.copy() for wf in first]
    again = table.wavefront_grouped_all(half[1], ids[parts[1]], into=first, **kw)
    assert all(x is y for x, y in zip(again, first)) and all(np.array_equal(wf.piston, p) for wf, p in zip(first, pistons))
    _assert_cells(first, gc.cell_references(records, ray, ids, mons, "focus", su["reference"], su["pupil"], pistons, G))
    uniform = dict(pupil=(0.0, 0.0, 0.2), monitors=mons, focus=(0.0, 0.0, 0.0), piston=0.0)  # one table for all cells: G alone can differ
    plain = table.wavefront_grouped_all(half[0], ids[parts[0]], n_groups=G, **uniform)
    table.wavefront_grouped_all(half[1], ids[parts[1]], n_groups=G, into=plain, **uniform)
    for other in (G + 1, G - 1):
        with pytest.raises(ValueError, match="into"):
            table.wavefront_grouped_all(half[1], ids[parts[1]], n_groups=other, into=plain, **uniform)
    with pytest.raises(ValueError, match="into"):
        table.wavefront_grouped_all(half[1], ids[parts[1]], into=first, **{**kw, "pupil": su["pupil"] + 0.001})
    with pytest.raises(ValueError, match="into"):
        table.wavefront_grouped_all(half[1], ids[parts[1]], into=first, **{**kw, "focus": su["reference"][::-1]})
    with pytest.raises(ValueError, match="piston"):
        table.wavefront_grouped_all(half[1], ids[parts[1]], into=first, piston=0.125, **kw)


# -- 9: the physics, closed form ---------------------------------------------------------------------------------------------------
def test_two_point_sources_each_against_its_own():
    """Two point sources at different lab points are two groups, each referenced to its own source: W is the same for every ray of a
    group, so every group's rms is within its interval of 0.  The ungrouped call against the first source alone sees the second
    one's displacement: sideways as tilt (Noll 2, delta R / 2 as in tests/test_gpu_wavefront.py), along the normal as defocus."""
    n, R = 1500, 0.16
    F = np.array([[0.0, 0.0, 0.0], [0.02, 0.003, 0.0]])
    (o0, d0, i0), (o1, d1, i1) = _cone(n, 0.15, 31, source=F[0]), _cone(n, 0.15, 32, source=F[1])
    segs = _hand_batch(np.concatenate([o0, o1]), np.concatenate([d0, d1]), 9.0, np.concatenate([i0, i1]), pathlength=1.25)
    ids = np.repeat([0, 1], n).astype(np.int32)
    mon = oa.Monitor([3.0, 0, 0], 4, 4)
    table = oa.OpticalTable()
    wf = table.wavefront_grouped_batch(mon, segs, ids, focus=F, pupil=(0.0, 0.0, R), piston=1.25)
    records, ray = _records(segs)
    refs = gc.cell_references(records, ray, ids, [mon], "focus", F, [np.tile([0.0, 0.0, R], (2, 1))], [[1.25, 1.25]], 2)[0]
    _assert_cells([wf], [refs])
    rms = wf.rms(1).cpu().numpy()
    for g, ref in enumerate(refs):
        assert ref.counts[0] == n
        hi = rms_interval(ref.sums, ref.bound, 1)[1]
        assert rms[g] <= hi < 1e-12, (g, rms[g], hi)
    plain = table.wavefront_batch(mon, segs, focus=F[0], pupil=(0.0, 0.0, R), piston=1.25)
    assert int(plain.counts) == 2 * n and float(plain.rms(1)) > 1e-5  # one reference for two sources: tilt and defocus of the other
    both = plain.coefficients().cpu().numpy()
    alone = table.wavefront_grouped_batch(mon, segs, ids, focus=F[0], pupil=(0.0, 0.0, R), piston=1.25).coefficients().cpu().numpy()
    assert abs(alone[1, 1] - (-0.003) * R / 2) < 1e-6 and abs(alone[1, 3]) > 1e-6 and abs(both[1]) > 1e-5  # (F0 - F1) . a_y = -0.003: tilt
    assert np.abs(alone[0, 1:]).max() < 1e-12


# -- 10: chromatic -----------------------------------------------------------------------------------------------------------------
def test_chromatic_defocus_from_one_trace():
    """The example's singlet at three wavelengths, one trace of the multiplexed batch, a monitor in the converging beam at x = 8
    against one focus: group g's coefficients equal those of `wavefront_all` on that wavelength's batch traced alone within the
    sum of the two propagated bounds, and the defocus term is monotone in the wavelength."""
    n, R, focus = 2000, 0.034, (10.15, 0.0, 0.0)
    rng = np.random.default_rng(31)
    r, phi = 0.15 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    o, d = np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], axis=1), np.tile([1.0, 0.0, 0.0], (n, 1))
    intensity = 0.25 + 0.75 * rng.random(n)
    wavelengths = [780e-7, 560e-7, 400e-7]
    table, mon = oa.OpticalTable(), oa.Monitor([8.0, 0, 0], 2, 2)
    table.add_components([oa.BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n=oa.Glass_NBK7())])
    alone = [RayBatch.from_arrays(o, d, wavelength=wl, intensity=intensity, q=1j * np.pi * scenes.W0**2 / wl, device="cuda") for wl in wavelengths]
    batch = alone[0].multiplexed_in_wavelength(wavelengths)
    ids, found = batch.groups_by_wavelength()
    segs = table.trace_batch(batch, max_segments=4)
    records, ray = _records(segs)
    wf = table.wavefront_grouped_batch(mon, segs, ids, focus=focus, pupil=(0.0, 0.0, R), labels=found.tolist())
    assert wf.n_groups == 3 and wf.labels == sorted(wavelengths) and wf.counts.tolist() == [n] * 3
    refs = gc.cell_references(records, ray, ids.cpu().numpy(), [mon], "focus", focus, [np.tile([0.0, 0.0, R], (3, 1))], [wf.piston], 3)[0]
    _assert_cells([wf], [refs])
    c = wf.coefficients().cpu().numpy()
    for w, wl in enumerate(wavelengths):
        g = sorted(wavelengths).index(wl)
        segs_alone = table.trace_batch(alone[w], max_segments=4)
        plain = table.wavefront_batch(mon, segs_alone, focus=focus, pupil=(0.0, 0.0, R), piston=float(wf.piston[g]))
        ref_alone = cases.reference(support.host_records(segs_alone, "n", "pathlength"), mon, dict(focus=focus), (0.0, 0.0, R), float(wf.piston[g]))
        assert int(plain.counts) == n
        (_, da, _, _), (_, db, _, _) = coefficient_bound(refs[g].sums, refs[g].bound, 15), coefficient_bound(ref_alone.sums, ref_alone.bound, 15)
        diff = np.abs(c[g] - plain.coefficients().cpu().numpy())
        assert np.all(diff <= da + db + 2 * U * abs(wf.piston[g])), (g, diff, da + db)
    print(f"  defocus (blue, green, red): {c[:, 3]}; Strehl {wf.strehl().cpu().numpy()}")
    assert (np.diff(c[:, 3]) < 0).all() or (np.diff(c[:, 3]) > 0).all()
    assert abs(c[2, 3] - c[0, 3]) > 1e-6  # some ten waves between blue and red
    with pytest.raises(ValueError, match="labels"):
        table.wavefront_grouped_batch(mon, segs, ids, focus=focus, pupil=(0.0, 0.0, R)).strehl()


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "chromatic_wavefront.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "one trace" in out.stdout and "defocus monotone in the wavelength: True" in out.stdout, out.stdout
    assert out.stdout.count(" nm ") == 5


# -- 11: the C ABI -----------------------------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / sums of M monitors x G groups for ot_monitor_wavefront_groups_many, with a guard region on either side of each."""

    def __init__(self, M, n_groups):
        super().__init__(guard=64, counts=(torch.int64, (M, n_groups, 2)), sums=(torch.float64, (M, n_groups, 61)))


def test_abi_errors(ctx):
    lib, c = ctx
    n, n_g = 130, 4
    segs = SegmentBatch(2 * n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    segs.dx.fill_(1.0)
    segs.length.fill_(10.0)
    segs.intensity.fill_(0.5)
    segs.field("n").fill_(1.0)
    segs.ray.copy_(torch.arange(2 * n, dtype=torch.int32) % n)
    segs.count, segs.n_rays = torch.full((n,), 2, dtype=torch.int32, device="cuda"), n
    m = oa.Monitor([5, 0, 0], 2, 2)
    mon = monitor_struct(m)
    out = _Out(1, n_g)
    src, n_segments, count, n_rays = segment_source(segs)
    ids = torch.arange(n, dtype=torch.int32, device="cuda") % 5 - 1  # -1 .. 3: a fifth of the rays is masked
    good_axes = cases.axes_of(m).reshape(1, 6)
    good_ref, good_pupil, good_piston = np.tile([1.0, 0.0, 0.0], (n_g, 1)), np.tile([0.0, 0.0, 0.5], (n_g, 1)), np.full(n_g, 4.0)
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, kind=1, reference=good_ref, coords=1, pupil=good_pupil, piston=good_piston,
             groups=ids.data_ptr(), n_ids=n, n_groups=n_g, source=src, intensity=segs.intensity.data_ptr(), n_index=segs.field("n").data_ptr(),
             pathlength=segs.pathlength.data_ptr(), n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(),
             sums=out.sums.data_ptr(), acc=0):
        return lib.ot_monitor_wavefront_groups_many(ctx_, mons, M, ptr(axes), kind, ptr(reference), coords, ptr(pupil), ptr(piston), groups, n_ids,
                                                    n_groups, None if source is None else C.byref(source), intensity, n_index, pathlength, n_seg, cnt,
                                                    rays, counts, sums, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)
    for null in ("ctx_", "mons", "axes", "reference", "pupil", "piston", "source", "n_index", "pathlength", "counts", "sums"):
        expect(call(**{null: None}), "NULL")
    expect(call(groups=None), "NULL argument: groups")
    for bad in (0, 257, -1):
        expect(call(n_groups=bad), "n_groups must be 1 .. 256")
    for bad in (0, -5):
        expect(call(n_ids=bad), "n_group_ids must be 1 .. 2^31 - 1")
    expect(call(M=17, n_groups=256), "n_monitors * n_groups exceeds 4096 cells")  # refused before a table of that size is read
    expect(call(M=4097, n_groups=1), "exceeds 4096 cells")
    expect(call(M=0), "n_monitors")
    expect(call(kind=2), "reference_kind")
    expect(call(coords=-1), "coordinates")
    expect(call(acc=2), "accumulate")
    expect(call(n_seg=-1), "segment count")
    expect(call(source=altered(width=4)), "width must be 8")
    a = good_axes.copy()
    a.flat[1] = np.nan
    expect(call(axes=a), "axes must be finite")
    for k in (0, 3 * n_g - 1):  # the first and the last entry of the table by cell
        a = good_ref.copy()
        a.flat[k] = np.inf
        expect(call(reference=a), "reference must be finite")
        a = good_pupil.copy()
        a.flat[k] = np.nan
        expect(call(pupil=a), "pupil must be finite")
    a = good_piston.copy()
    a[n_g - 1] = np.nan
    expect(call(piston=a), "piston must be finite")
    for bad in (0.0, -1.0, np.inf):
        a = good_pupil.copy()
        a[n_g - 1, 2] = bad
        expect(call(pupil=a), "radius must be positive" if bad <= 0 else "pupil must be finite")
    a = good_ref.copy()
    a[2] = 0.0
    expect(call(reference=a), "must not be zero")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good.  Every segment runs from x = 0 to 10 along the axis and meets the monitor at P = 0 after t = 5:
    # W = 5 against the plane wave along x, W' = 1 with piston 4, p = q = 0, w = 0.5.  Group g: the rays with i % 5 - 1 = g, twice.
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    hits = np.array([2 * int((np.arange(n) % 5 - 1 == g).sum()) for g in range(n_g)])
    want = np.zeros((n_g, 61))
    want[:, 0] = want[:, 45] = want[:, 60] = 0.5 * hits
    assert out.counts[0].tolist() == [[int(h), 0] for h in hits]
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), want)
    assert out.guards_untouched()
    assert call(acc=1) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), 2 * want)
    assert call(n_ids=100) == 0 and lib.ot_ctx_synchronize(c) == 0  # a table shorter than the batch: nothing is read past its end
    assert out.counts[0, :, 0].tolist() == [2 * int((np.arange(100) % 5 - 1 == g).sum()) for g in range(n_g)]
    assert out.guards_untouched()


# -- 12: what is refused, and nothing to do ----------------------------------------------------------------------------------------
def test_single_precision_is_refused():
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(130, 3)
    segs = table.trace_batch(_batch(o, d, intensity, precision="f32"), max_segments=3)
    ids = np.zeros(130, dtype=np.int32)
    with pytest.raises(ValueError, match="wavefront_all needs a double-precision SegmentBatch"):
        table.wavefront_grouped_all(segs, ids, direction=(1, 0, 0), monitors=[oa.Monitor([7.5, 0, 0], 6, 6)])
    with pytest.raises(ValueError, match="double-precision"):
        get_engine().monitor_wavefront_groups_many([monitor_struct(oa.Monitor([7.5, 0, 0], 6, 6))], np.array([[0, 1, 0, 0, 0, 1.0]]), 1,
                                                   np.array([[[1.0, 0, 0]]]), 1, np.array([[[0, 0, 1.0]]]), np.zeros((1, 1)),
                                                   torch.zeros(130, dtype=torch.int32, device="cuda"), 1, segs)


def test_no_segments():
    table, eng = support.cfg2_table(), get_engine()
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    for wf in table.wavefront_grouped_all(none, np.zeros(3, dtype=np.int32), n_groups=4, direction=(1, 0, 0), monitors=cases.monitors_at(7.5)[:2]):
        assert wf.n_groups == 4 and not wf.counts.any() and not wf.outside.any() and not wf.sums.any() and not wf.piston.any()
        assert torch.isnan(wf.coefficients()).all() and wf.coefficients(4).shape == (4, 4)
