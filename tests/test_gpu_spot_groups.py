"""GPU (MI355X): spot statistics per ray group — `OpticalTable.spots_grouped_all` / `spots_grouped_batch`, the moments of every
monitor's hits per plane and per group of input rays, summed on the device by the group mode of k_mon_spots
(ot_monitor_spot_groups_many) with no hit list and no floating-point atomic.

Reference, in every comparison: tests/spots_reference.py on the segment records copied from the device, with
valid = (ids[ray] == g) for group g — the rule of the header in numpy, its sums formed with math.fsum.  Every case first asserts,
from the REFERENCE, that no decision lies within 1e-7 of its boundary (a subset of the records cannot lower the margin of the whole).
Counts must then be EQUAL, and the sums within the reference's own derived `bound` (tests/test_gpu_spots.py says where it comes
from); the rms radius of a cell within what those bounds allow (radius_interval)."""
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
from optable_amd.engine import get_engine, segment_source, spot_groups_plan
from optable_amd.table import monitor_struct
from spots_reference import radius_interval, spots_reference
from support import ctx  # noqa: F401  (the fixture)
from wavefront_cases import axes_of

pytestmark = pytest.mark.gpu

OFFSETS = np.array([-0.9, -0.3, 0.0, 0.45, 0.9])


def _reference(records, mon, offsets, weight="intensity", centre=(0.0, 0.0), valid=None, what=""):
    o, d, length, intensity = records[:4]
    s = monitor_struct(mon)
    ref = spots_reference(o, d, length, intensity if weight == "intensity" else None, list(s.M), list(s.origin), s.half_width, s.half_height, axes_of(mon),
                          centre, offsets, valid=valid)
    print(f"  {what}margin {ref.margin:.3g}, hits per plane {ref.counts.min()} .. {ref.counts.max()}")
    assert ref.margin > 1e-7  # a condition on the inputs
    return ref


def _group_references(records, ray, ids, groups, mon, offsets, **kw):
    """The reference of every group g of `groups`: the records whose ray has the id g (a ray beyond the table has none)."""
    ids = np.asarray(ids)
    known = (ray >= 0) & (ray < len(ids))
    of_record = np.where(known, ids[np.where(known, ray, 0)], -1)
    return {g: _reference(records, mon, offsets, valid=of_record == g, what=f"group {g}: ", **kw) for g in groups}


def _assert_sums(counts, sums, ref, factor=1.0, bound=None):
    bound = factor * ref.bound if bound is None else bound
    np.testing.assert_array_equal(counts, ref.counts)
    err = np.abs(sums - ref.sums)
    worst = np.argmax(err - bound)
    print(f"  sums: largest error {err.max():.3g}; nearest to its bound {err.flat[worst]:.3g} of {bound.flat[worst]:.3g}")
    assert np.all(err <= bound), float((err - bound).max())
    assert np.all(sums[ref.counts == 0] == 0.0)


def _assert_groups(sp, refs):
    """`sp` (a MonitorSpotGroups) against the references {g: Spots} of some or all of its groups."""
    counts, sums, offsets = sp.to_host()
    J, G = len(offsets), sp.n_groups
    assert counts.dtype == np.int64 and sums.dtype == np.float64 and counts.shape == (J, G) and sums.shape == (J, G, 6)
    assert sp.counts.is_cuda and sp.sums.is_cuda
    radius = sp.rms_radius().cpu().numpy()
    assert radius.shape == (J, G)
    for g, ref in refs.items():
        _assert_sums(counts[:, g], sums[:, g], ref)
        for j in np.nonzero(ref.counts > 0)[0]:
            lo, hi = radius_interval(ref.sums[j], ref.bound[j])
            assert lo <= radius[j, g] <= hi, (j, g, lo, radius[j, g], hi)
        assert np.isnan(radius[ref.counts == 0, g]).all()
        one = sp.group(g)
        assert torch.equal(one.counts, sp.counts[:, g]) and torch.equal(one.sums, sp.sums[:, g])


def _monitors():
    return [oa.Monitor([7.5, 0, 0], 6, 6),
            oa.Monitor([7.5, 0, 0], 0.5, 0.5),          # clips the beam
            oa.Monitor([7.5, 40, 0], 6, 6),             # where no segment passes
            oa.Monitor([7.5, 0, 0], 6, 6).RotZ(0.3)]    # planes displaced along a normal that is not x


EMPTY = 2
N1 = 5003
THIRDS = np.repeat([0, 1, 2], [1668, 1668, 1667]).astype(np.int32)                          # (a) contiguous thirds
SCATTERED = np.random.default_rng(41).integers(-1, 4, N1).astype(np.int32)                  # (b) {-1, 0, 1, 2, 3}: -1 and 3 are masked
TABLES = {"thirds": THIRDS, "scattered": SCATTERED}


@pytest.fixture(scope="module")
def case1():
    """The fixture of tests/test_gpu_spots.py, built anew: cfg 2, 5,003 rays, 5 segments — 25,015 slots: 13 workgroups of 2,048 with a
    ragged tail — four monitors, five planes: (table, monitors, get(layout, precision) -> (segs, (records, ray, [ungrouped
    reference per monitor], {table: [{g: reference} per monitor]}))), traced and reduced on the host on first use."""
    table, mons = support.cfg2_table(), _monitors()
    o, d = scenes.cfg2_rays(N1, 0)

    def derive(segs):
        *records, ray = support.host_records(segs, "ray")
        assert ray.min() == 0 and ray.max() == N1 - 1
        whole = [_reference(records, m, OFFSETS) for m in mons]
        grouped = {name: [_group_references(records, ray, ids, range(3), m, OFFSETS) for m in mons] for name, ids in TABLES.items()}
        return records, ray, whole, grouped

    return table, mons, support.traced(table, lambda precision: support.weighted_batch(o, d, precision), 5, derive)


# -- 1: layouts and precisions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_and_precisions(case1, layout, precision, monkeypatch):
    table, mons, get = case1
    segs, (records, ray, whole, grouped) = get(layout, precision)
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("spots_grouped_all converted the batch")

    for name, ids in TABLES.items():
        with monkeypatch.context() as mp:
            mp.setattr(SegmentBatch, "to_slots", refuse)
            mp.setattr(SegmentBatch, "astype", refuse)
            spots = table.spots_grouped_all(segs, ids, n_groups=3, offsets=OFFSETS)  # the table's own monitors, in their order
        assert len(spots) == len(mons) and all(sp.monitor is m and sp.n_groups == 3 for sp, m in zip(spots, mons))
        masked_rays = (ids < 0) | (ids >= 3)
        assert masked_rays.any() == (name == "scattered")
        for k, (sp, refs) in enumerate(zip(spots, grouped[name])):
            _assert_groups(sp, refs)
            # summed over g: the ungrouped reference's counts less the masked hits
            masked_hits = np.array([int(masked_rays[ray[h]].sum()) for h in whole[k].hits])
            np.testing.assert_array_equal(sp.counts.sum(dim=1).cpu().numpy(), whole[k].counts - masked_hits)
            assert torch.equal(sp.total().counts, sp.counts.sum(dim=1))
            if name == "scattered" and k == 0:
                assert masked_hits.min() > 0
        assert not spots[EMPTY].counts.any() and not spots[EMPTY].sums.any() and torch.isnan(spots[EMPTY].rms_radius()).all()
        assert torch.isnan(spots[EMPTY].centroid()).all() and np.isnan(spots[EMPTY].best_focus()[0]).all()
    two = table.spots_grouped_all(segs, THIRDS, offsets=OFFSETS, monitors=[mons[3], mons[0]])  # ... or those given; G = max id + 1
    assert two[0].n_groups == 3
    _assert_groups(two[0], grouped["thirds"][3])
    _assert_groups(two[1], grouped["thirds"][0])
    one = table.spots_grouped_batch(mons[1], segs, torch.from_numpy(SCATTERED).cuda(), n_groups=3)  # J = 1, ids on the device already
    assert one.offsets.tolist() == [0.0] and one.counts.shape == (1, 3)
    for g in range(3):
        ref = grouped["scattered"][1][g]
        assert int(one.counts[0, g]) == ref.counts[2] and np.all(np.abs(one.sums[0, g].cpu().numpy() - ref.sums[2]) <= ref.bound[2])


# -- 2: one group is the ungrouped call, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_one_group_is_the_ungrouped_call_bit_for_bit(case1, layout):
    """G = 1, every id 0: the grid, the butterflies' inputs, the row adds and the partials' order are those of `spots_all`."""
    table, mons, get = case1
    segs = get(layout, "f64")[0]
    plain = table.spots_all(segs, offsets=OFFSETS, monitors=mons)
    grouped = table.spots_grouped_all(segs, np.zeros(N1, dtype=np.int32), n_groups=1, offsets=OFFSETS, monitors=mons)
    for p, g in zip(plain, grouped):
        assert g.counts.shape == (5, 1) and g.sums.shape == (5, 1, 6)
        assert torch.equal(g.counts[:, 0], p.counts) and torch.equal(g.sums[:, 0], p.sums)
    assert int(plain[0].counts.min()) >= N1 and bool((plain[0].sums != 0).all())
    many = np.linspace(-0.9, 0.9, 300)  # more than one launch: the same split of the cell list
    p, g = table.spots_batch(mons[0], segs, offsets=many), table.spots_grouped_batch(mons[0], segs, np.zeros(N1, dtype=np.int32), offsets=many)
    assert g.n_groups == 1 and torch.equal(g.counts[:, 0], p.counts) and torch.equal(g.sums[:, 0], p.sums)


# -- 3: many groups in one wave --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["a group per lane", "alternating", "a masked wave"])
def test_many_groups_in_one_wave(arrangement):
    """256 hand-made segments along x, all through the monitor at x = 5 and its planes: four waves of one workgroup.  Every lane of
    a wave in a group of its own is the 64-step walk; alternating ids two steps with interleaved lanes; and a wave whose lanes are
    all masked walks nothing while its neighbours do."""
    rng = np.random.default_rng(29)
    n = 256
    o = np.stack([np.zeros(n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n)], axis=1)
    tilt = np.stack([np.ones(n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n)], axis=1)
    d = tilt / np.linalg.norm(tilt, axis=1, keepdims=True)
    length, intensity = np.full(n, 8.0), 0.25 + 0.75 * rng.random(n)
    segs = support.list_batch(o, d, length, intensity)
    records, ray = (o, d, length, intensity), np.arange(n)
    i = np.arange(n)
    ids, G = {"a group per lane": (i % 64, 64), "alternating": (i % 2, 2), "a masked wave": (np.where((i >= 64) & (i < 128), -1, i // 64), 4)}[arrangement]
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 2, 2)
    offsets = [-0.5, 0.0, 0.5]
    sp = table.spots_grouped_batch(mon, segs, ids.astype(np.int32), n_groups=G, offsets=offsets)
    refs = _group_references(records, ray, ids, range(G), mon, offsets)
    _assert_groups(sp, refs)
    per_group = np.bincount(ids[ids >= 0], minlength=G)
    assert sp.counts.cpu().numpy().tolist() == [per_group.tolist()] * 3  # every segment crosses every plane
    if arrangement == "a masked wave":
        assert per_group.tolist() == [64, 0, 64, 64] and not sp.sums[:, 1].any()
    again = table.spots_grouped_batch(mon, segs, ids.astype(np.int32), n_groups=G, offsets=offsets)
    assert torch.equal(again.counts, sp.counts) and torch.equal(again.sums, sp.sums)


# -- 4: launch boundaries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,pairs", [(100, 2), (256, 1), (255, 1)])
def test_launch_boundaries(case1, G, pairs):
    """4 monitors x 5 planes = 20 pairs on the slot segments of case 1, ids ray % G: G = 100 takes two pairs a launch, G = 256 one
    that fills the LDS, G = 255 one whose last cell is not the last of the LDS.  A sample of groups against the reference; the
    counts' total over g exactly the ungrouped reference's (every id is a group)."""
    table, mons, get = case1
    segs, (records, ray, whole, _) = get("slots", "f64")
    plan = spot_groups_plan(4, 5, G)
    assert len(plan) == 20 // pairs and all(cells == pairs * G and first % G == 0 for first, cells in plan)
    ids = (np.arange(N1) % G).astype(np.int32)
    spots = table.spots_grouped_all(segs, ids, n_groups=G, offsets=OFFSETS, monitors=mons)
    sample = (0, 1, G // 2, G - 2, G - 1)
    for k, (sp, m) in enumerate(zip(spots, mons)):
        _assert_groups(sp, _group_references(records, ray, ids, sample, m, OFFSETS))
        np.testing.assert_array_equal(sp.counts.sum(dim=1).cpu().numpy(), whole[k].counts)
        assert torch.equal(sp.counts[:, 0], sp.group(0).counts)
    assert not spots[EMPTY].counts.any() and not spots[EMPTY].sums.any()
    assert int(spots[0].counts.min()) > 0  # the wide monitor: every group has a ray on every plane


# -- 5: determinism and `into=` --------------------------------------------------------------------------------------------------
def test_determinism(case1):
    table, mons, get = case1
    for layout in ("slots", "append"):
        segs = get(layout, "f64")[0]
        a, b = (table.spots_grouped_all(segs, SCATTERED, n_groups=3, offsets=OFFSETS, monitors=mons) for _ in range(2))
        for x, y in zip(a, b):
            assert torch.equal(x.counts, y.counts) and torch.equal(x.sums, y.sums) and x.sums is not y.sums
        table.spots_grouped_all(segs, SCATTERED, n_groups=3, offsets=OFFSETS, monitors=mons, into=a)
        table.spots_grouped_all(segs, SCATTERED, n_groups=3, offsets=OFFSETS, monitors=mons, into=b)
        for x, y in zip(a, b):
            assert torch.equal(x.counts, y.counts) and torch.equal(x.sums, y.sums)
        assert int(a[0].counts.min()) > 0 and bool((a[0].sums[..., 0] != 0).all())


def test_streaming():
    """Two halves of a batch traced separately, the second added with `into=` and its own id table, against the reference of their
    concatenation: counts equal, sums within the bound."""
    table = support.cfg2_table()
    n = 2049
    o, d = scenes.cfg2_rays(n, 3)
    whole = support.weighted_batch(o, d)
    ids = np.random.default_rng(43).integers(-1, 3, n).astype(np.int32)  # {-1, 0, 1, 2}
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 0.7, 0.7), oa.Monitor([7.5, 40, 0], 6, 6)]
    parts = (slice(0, 1024), slice(1024, n))
    halves = []
    for part in parts:
        b = RayBatch.from_arrays(o[part], d[part], wavelength=scenes.WL, intensity=whole.intensity[part].cpu().numpy(), q=support.Q, device="cuda")
        halves.append(table.trace_batch(b, max_segments=5, layout="slots"))
    pieces = [support.host_records(h, "ray") for h in halves]
    records = tuple(np.concatenate(p) for p in zip(*(piece[:4] for piece in pieces)))
    ray = np.concatenate([pieces[0][4], pieces[1][4] + 1024])  # the second chunk's rays by their place in the whole batch
    spots = table.spots_grouped_all(halves[0], ids[parts[0]], n_groups=3, offsets=OFFSETS, monitors=mons)
    first = [sp.counts.clone() for sp in spots]
    again = table.spots_grouped_all(halves[1], ids[parts[1]], n_groups=3, offsets=OFFSETS, monitors=mons, into=spots)
    assert len(again) == len(spots) and all(a is b for a, b in zip(again, spots))
    for sp, m, before in zip(spots, mons, first):
        _assert_groups(sp, _group_references(records, ray, ids, range(3), m, OFFSETS))
        assert int(before.sum()) < int(sp.counts.sum()) or not sp.counts.any()
    again = table.spots_grouped_all(halves[0], ids[parts[0]], n_groups=3, offsets=OFFSETS, monitors=mons)  # without `into=`: from zero
    assert all(torch.equal(a.counts, b) for a, b in zip(again, first))


# -- 6: the use case -------------------------------------------------------------------------------------------------------------
def test_chromatic_focal_shift_from_one_trace():
    """A collimated bundle in three wavelengths through a biconvex N-BK7 lens (R = +-5, 0.4 thick, first vertex at x = 5; paraxial
    foci at x = 10.04 (400 nm), 10.16 (560 nm) and 10.22 (780 nm)), one trace of the multiplexed batch, a monitor at x = 10.14
    with 9 planes over +-0.2.  Each wavelength's cells against an ungrouped `spots_all` of that wavelength's batch traced alone:
    counts equal, sums within the sum of the two references' bounds; and the best focus moves with the colour as normal
    dispersion has it."""
    n = 2000
    rng = np.random.default_rng(31)
    r, phi = 0.15 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    o, d = np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], axis=1), np.tile([1.0, 0.0, 0.0], (n, 1))
    intensity = 0.25 + 0.75 * rng.random(n)
    wavelengths = [780e-7, 560e-7, 400e-7]
    table, mon = oa.OpticalTable(), oa.Monitor([10.14, 0, 0], 2, 2)
    table.add_components([oa.BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n=oa.Glass_NBK7())])
    offsets = np.linspace(-0.2, 0.2, 9)
    alone = [RayBatch.from_arrays(o, d, wavelength=wl, intensity=intensity, q=1j * np.pi * scenes.W0**2 / wl, device="cuda") for wl in wavelengths]
    batch = alone[0].multiplexed_in_wavelength(wavelengths)
    assert batch.n == 3 * n
    ids, found = batch.groups_by_wavelength()
    assert ids.is_cuda and ids.dtype == torch.int32 and found.tolist() == sorted(wavelengths)
    assert ids.cpu().tolist() == [2] * n + [1] * n + [0] * n  # group-major: every wave of the trace is one group (but two)
    segs = table.trace_batch(batch, max_segments=4)
    *records, ray = support.host_records(segs, "ray")
    sp = table.spots_grouped_batch(mon, segs, ids, offsets=offsets, labels=found.tolist())
    assert sp.n_groups == 3 and sp.labels == sorted(wavelengths)
    refs = _group_references(records, ray, ids.cpu().numpy(), range(3), mon, offsets)
    _assert_groups(sp, refs)
    for w, wl in enumerate(wavelengths):
        g = sorted(wavelengths).index(wl)
        segs_alone = table.trace_batch(alone[w], max_segments=4)
        ref_alone = _reference(support.host_records(segs_alone), mon, offsets, what=f"{wl * 1e7:.0f} nm alone: ")  # (asserts its margin)
        plain = table.spots_batch(mon, segs_alone, offsets=offsets)
        assert (ref_alone.counts == n).all() and torch.equal(sp.counts[:, g], plain.counts)
        diff = np.abs(sp.sums[:, g].cpu().numpy() - plain.sums.cpu().numpy())
        assert np.all(diff <= refs[g].bound + ref_alone.bound), float((diff - refs[g].bound - ref_alone.bound).max())
    x, radius = sp.best_focus()
    print(f"  best focus (blue, green, red): x = {10.14 + x[0]:.5f}, {10.14 + x[1]:.5f}, {10.14 + x[2]:.5f}; rms radius {radius}")
    assert x[0] < x[1] < x[2] and offsets[0] < x[0] and x[2] < offsets[-1]
    assert torch.equal(sp.total().counts, torch.full((9,), 3 * n, dtype=torch.int64, device="cuda"))


def test_the_example_runs():
    """examples/chromatic_focus.py as a user would run it: five wavelengths, 41 planes, one trace — a monotone focal shift."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "chromatic_focus.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "41 planes, one trace" in out.stdout and "monotone in the wavelength: True" in out.stdout, out.stdout
    assert out.stdout.count(" nm ") == 5


# -- 7: branching scenes ---------------------------------------------------------------------------------------------------------
def test_a_half_mirror():
    """support.half_mirror (a lens, then roof mirrors whose first reflects half): ids by input ray — every segment of a ray's
    tree lands in its group."""
    table = support.table_of(support.half_mirror(oa))
    n = 1003
    ids = np.random.default_rng(47).integers(-1, 4, n).astype(np.int32)  # {-1, 0, 1, 2, 3}, G = 3: -1 and 3 are masked
    segs = table.trace_batch(support.weighted_batch(*scenes.cfg2_rays(n, 5)), max_segments=6)
    *records, ray = support.host_records(segs, "ray")
    assert ray.min() == 0 and ray.max() == n - 1 and len(ray) > 2 * n
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([2.5, 0, 0], 6, 6)]
    offsets = [-0.5, 0.0, 0.25]
    for sp, m in zip(table.spots_grouped_all(segs, ids, n_groups=3, offsets=offsets, monitors=mons), mons):
        refs = _group_references(records, ray, ids, range(3), m, offsets)
        _assert_groups(sp, refs)
        assert all(ref.counts.min() > 0 for ref in refs.values())


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (every hit splits): the [k][tree] slots with count[i], the dense list with holes
    and the list in generation order — the `ray` of every node is its tree."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    ids = (np.arange(320) % 7 - 1).astype(np.int32)  # -1 .. 5, G = 5: -1 and 5 are masked
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    offsets = [-0.2, 0.0, 0.3]
    eng = get_engine()
    eng.upload(table.compile())
    assert eng.trees_plan("f64", 12)["slots"]
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        *records, ray = support.host_records(segs, "ray")
        assert ray.min() == 0 and ray.max() == 319 and len(ray) > 2 * 320
        for sp, m in zip(table.spots_grouped_all(segs, ids, n_groups=5, offsets=offsets, monitors=mons), mons):
            refs = _group_references(records, ray, ids, range(5), m, offsets)
            _assert_groups(sp, refs)
            assert all(ref.counts.min() >= 45 for ref in refs.values())  # every tree of a group crosses each plane


# -- 8: the C ABI ----------------------------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / sums of M monitors x J planes x G groups for ot_monitor_spot_groups_many, with a guard region on either side of each."""

    def __init__(self, M, J, G):
        super().__init__(guard=64, counts=(torch.int64, (M, J, G)), sums=(torch.float64, (M, J, G, 6)))


def test_abi_errors(ctx):
    lib, c = ctx
    n, J, G = 130, 3, 4
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
    out = _Out(1, J, G)
    src, n_segments, count, n_rays = segment_source(segs)
    assert (n_segments, n_rays) == (2 * n, n)
    ids = torch.arange(n, dtype=torch.int32, device="cuda") % 5 - 1  # -1 .. 3: a fifth of the rays is masked
    good_axes, good_centre, good_offsets = axes_of(m).reshape(1, 6), np.array([[0.25, -0.5]]), np.array([-1.0, 0.0, 6.0])
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, centre=good_centre, offsets=good_offsets, n_off=J, groups=ids.data_ptr(), n_ids=n,
             n_groups=G, source=src, intensity=segs.intensity.data_ptr(), n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays,
             counts=out.counts.data_ptr(), sums=out.sums.data_ptr(), acc=0):
        return lib.ot_monitor_spot_groups_many(ctx_, mons, M, ptr(axes), ptr(centre), ptr(offsets), n_off, groups, n_ids, n_groups,
                                               None if source is None else C.byref(source), intensity, n_seg, cnt, rays, counts, sums, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)
    for null in ("ctx_", "mons", "axes", "centre", "offsets", "source", "counts", "sums"):
        expect(call(**{null: None}), "NULL")
    expect(call(groups=None), "groups")
    expect(call(n_groups=0), "n_groups")
    expect(call(n_groups=257), "n_groups")
    expect(call(n_groups=-1), "n_groups")
    expect(call(n_ids=0), "n_group_ids")
    expect(call(n_ids=-5), "n_group_ids")
    expect(call(M=1 << 10, n_off=1 << 8, n_groups=8), "n_groups exceeds 2^20")  # the cell cap, refused before a monitor or an offset is read
    expect(call(M=1 << 10, n_off=(1 << 10) + 1, n_groups=1), "2^20")
    expect(call(M=0), "n_monitors")
    expect(call(n_off=0), "n_offsets")
    expect(call(acc=2), "accumulate")
    expect(call(n_seg=-1), "segment count")
    expect(call(source=altered(width=2)), "width")
    expect(call(source=altered(ray=None)), "NULL field")
    a = good_axes.copy()
    a.flat[1] = np.nan
    expect(call(axes=a), "axes")
    a = good_centre.copy()
    a.flat[0] = np.inf
    expect(call(centre=a), "centre")
    a = good_offsets.copy()
    a.flat[2] = np.nan
    expect(call(offsets=a), "offsets")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good.  Every one of the 2 n segments runs from x = 0 to 10 along the axis: it crosses the planes at x = 4
    # and 5 at P = (0, 0, 0), y = -0.25, z = 0.5, and ends before x = 11.  Group g: the rays with i % 5 - 1 = g, two segments each.
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    members = np.array([2 * int((np.arange(n) % 5 - 1 == g).sum()) for g in range(G)])
    unit = np.array([0.5, -0.125, 0.25, 0.03125, 0.125, -0.0625])  # (binary fractions: every sum is exact)
    want = members[:, None] * unit
    assert out.counts[0].tolist() == [members.tolist(), members.tolist(), [0] * G]
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), [want, want, np.zeros((G, 6))])
    assert out.guards_untouched()  # exactly M J G counts and 6 M J G sums, and nothing beyond
    assert call(acc=1) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    assert out.counts[0].tolist() == [(2 * members).tolist(), (2 * members).tolist(), [0] * G]
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), [2 * want, 2 * want, np.zeros((G, 6))])
    # a table shorter than the batch: the rays beyond it are in no group, and nothing is read past its end
    assert call(n_ids=100) == 0 and lib.ot_ctx_synchronize(c) == 0
    short = [2 * int((np.arange(100) % 5 - 1 == g).sum()) for g in range(G)]
    assert out.counts[0].tolist() == [short, short, [0] * G]
    assert call(intensity=None, n_groups=2) == 0 and lib.ot_ctx_synchronize(c) == 0  # intensity = NULL: weight 1; G = 2 writes the first 2 J cells
    flat = out.counts.reshape(-1)
    assert flat[: 2 * J].tolist() == [int(members[0]), int(members[1])] * 2 + [0, 0] and flat[2 * J:].tolist() == (short + short + [0] * G)[2 * J:]
    assert out.sums.reshape(-1, 6)[:4, 0].tolist() == [float(members[0]), float(members[1])] * 2
    assert out.guards_untouched()
