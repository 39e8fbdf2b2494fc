"""GPU (MI355X): wavefront error — `OpticalTable.wavefront_all` / `wavefront_batch`, the optical path of every monitor hit against
an ideal wave reduced on the device to 61 moments per monitor by the wavefront mode of k_mon_spots (ot_monitor_wavefront_many),
with no hit list and no floating-point atomic, and the Zernike coefficients, rms and Strehl ratio the host makes of them.

Reference, in every comparison: tests/wavefront_reference.py on the segment records copied from the device — the rule of the
header in numpy, its sums formed with math.fsum.  Every case first asserts, from the REFERENCE, that no decision (plane crossing
within the segment, rectangle, pupil rim) lies within 1e-7 of its boundary: a condition on the inputs, which
tests/test_wavefront_cpu.py also checks on the host through the C oracle's trace of the same seeded rays.  Counts (inside and
outside the pupil) must then be EQUAL, and every sum within `bound` of the reference, derived in its docstring from the roundings
of P, t, L, the dot products, the powers and the summation order — derived, not measured.  Coefficients and rms are held to what
those bounds allow to first order through the solve (coefficient_bound, rms_interval)."""
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
from optable_amd.engine import get_engine, segment_source, wavefront_plan
from optable_amd.table import monitor_struct
from optable_amd.wavefront import zernike
from support import ctx  # noqa: F401  (the fixture)
from wavefront_reference import U, coefficient_bound, gram, rms_interval

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(o, d, intensity, precision="f64"):
    return RayBatch.from_arrays(o, d, wavelength=scenes.WL, intensity=intensity, q=support.Q, precision=precision, device="cuda")


def _records(segs):
    """The valid segment records of a batch, copied from the device: (o, d, length, intensity, n, pathlength) as doubles."""
    return support.host_records(segs, "n", "pathlength")


def _assert_wavefront(wf, ref, terms=(1, 3, 4, 15)):
    """Counts equal, sums within the bound, and the derived quantities within what the bounds allow."""
    inside, outside, sums = wf.to_host()
    assert wf.counts.is_cuda and wf.outside.is_cuda and wf.sums.is_cuda and sums.dtype == np.float64 and sums.shape == (61,)
    assert (inside, outside) == tuple(ref.counts)
    err = np.abs(sums - ref.sums)
    worst = np.argmax(err - ref.bound)
    print(f"  sums: largest error {err.max():.3g}; nearest to its bound: sum {worst}, {err[worst]:.3g} of {ref.bound[worst]:.3g}")
    assert np.all(err <= ref.bound), (int(worst), float(err[worst]), float(ref.bound[worst]))
    if inside == 0:
        assert not sums.any() and math.isnan(float(wf.rms())) and math.isnan(float(wf.mean())) and torch.isnan(wf.coefficients()).all()
        return
    for k in terms:
        if inside < 4 * k:  # (a fit of few hits is checked on the host, in tests/test_wavefront_cpu.py)
            continue
        got = wf.coefficients(k).cpu().numpy()
        rcond = 1.0 / np.linalg.cond(gram(ref.sums, k))
        if rcond < 1e-10:  # hits that determine no such fit (the few lines of a ray fan): NaN below 1e-12, and nothing to compare near it
            assert rcond > 1e-14 or (np.isnan(got).all() and math.isnan(float(wf.rms(k))))
            continue
        c, dc, _, _ = coefficient_bound(ref.sums, ref.bound, k)
        got[0] -= wf.piston
        print(f"  {k} terms: largest coefficient error {np.abs(got - c).max():.3g} (bounds up to {dc.max():.3g})")
        assert np.all(np.abs(got - c) <= dc + U * abs(wf.piston)), (k, got - c, dc)
        lo, hi = rms_interval(ref.sums, ref.bound, k)
        assert lo <= float(wf.rms(k)) <= hi, (k, lo, float(wf.rms(k)), hi)


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 5,003 rays, 5 segments — 25,015 slots: 13 workgroups of 2,048 with a ragged tail — traced once per layout:
    (table, get(layout) -> (segs, records))."""
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(5003, 0)
    return table, support.traced(table, lambda precision: _batch(o, d, intensity, precision), 5, _records)


@pytest.mark.parametrize("setup", ["focus", "direction"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts(case1, layout, setup, monkeypatch):
    table, get = case1
    segs, records = get(layout)
    su = cases.SETUPS[setup]
    mons = cases.monitors_at(su["x"])
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("wavefront_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        wfs = table.wavefront_all(segs, pupil=su["pupil"], **su["kwargs"])  # the table's own monitors, piston=None
    assert len(wfs) == len(mons) and all(wf.monitor is m for wf, m in zip(wfs, mons))
    assert wfs[0].coordinates == ("direction" if setup == "focus" else "position") and wfs[0].reference[0] == setup
    refs = [cases.reference(records, m, su["kwargs"], p, wf.piston) for m, p, wf in zip(mons, su["pupil"], wfs)]
    for wf, ref in zip(wfs, refs):
        _assert_wavefront(wf, ref)
    assert refs[0].counts[0] >= 5003 and refs[0].counts[1] == 0 and refs[1].counts[0] > 0 and refs[1].counts[1] > 0  # the second pupil clips
    assert wfs[cases.EMPTY].to_host()[:2] == (0, 0) and wfs[cases.EMPTY].piston == 0.0
    # the piston the call found is the mean of W, so T00 all but vanishes
    assert abs(float(wfs[0].sums[45])) <= refs[0].bound[45] + abs(refs[0].sums[45])
    one = table.wavefront_batch(mons[3], segs, pupil=su["pupil"][3], piston=wfs[3].piston, **su["kwargs"])  # ... or one given
    assert torch.equal(one.sums, wfs[3].sums) and torch.equal(one.counts, wfs[3].counts) and torch.equal(one.outside, wfs[3].outside)
    # the other coordinates on the full monitor, asked for by name
    other = "position" if setup == "focus" else "direction"
    pupil = (0.0, 0.0, 0.5) if other == "position" else (0.0, 0.0, 0.01)
    wf = table.wavefront_batch(mons[0], segs, pupil=pupil, coordinates=other, piston=2.5, **su["kwargs"])
    _assert_wavefront(wf, cases.reference(records, mons[0], su["kwargs"], pupil, 2.5, coordinates=other))


@pytest.mark.parametrize("n,K", [(1, 1), (130, 3), (1027, 5)])
def test_batch_sizes(n, K):
    """1 x 1; 130 x 3 = 390 slots: a partial wave in a partial workgroup; 1,027 x 5 = 5,135: three workgroups, the last one ragged."""
    table = support.cfg2_table()
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=K, layout="slots")
    records = _records(segs)
    for su in cases.SETUPS.values():
        mons = cases.monitors_at(su["x"])
        for weight in ("intensity", "none"):
            wfs = table.wavefront_all(segs, pupil=su["pupil"], monitors=mons, weight=weight, **su["kwargs"])
            for wf, m, p in zip(wfs, mons, su["pupil"]):
                _assert_wavefront(wf, cases.reference(records, m, su["kwargs"], p, wf.piston, weight=weight))
    assert wfs[0].weight == "none" and (K > 1) == (int(wfs[0].counts) > 0)  # the beam reaches x = 7.5 on its second segment


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (every hit splits; n = 1.5 inside): the [k][tree] slots with count[i], the append
    block and the dense list with holes."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    kwargs, pupil = dict(direction=(1.0, 0.2, 0.0)), [(0.0, 0.0, 1.5), (0.1, 0.0, 2.0)]
    eng = get_engine()
    eng.upload(table.compile())
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        records = _records(segs)
        for wf, m, p in zip(table.wavefront_all(segs, pupil=pupil, monitors=mons, **kwargs), mons, pupil):
            ref = cases.reference(records, m, kwargs, p, wf.piston)
            _assert_wavefront(wf, ref)
            assert ref.counts.sum() >= 320  # every tree crosses each monitor


def test_more_monitors_than_one_group():
    """30 monitors: two launches, 28 + 2."""
    assert wavefront_plan(cases.GROUP_MONITORS) == [(0, 28), (28, 2)]
    table = support.cfg2_table()
    mons, pupils = cases.group_monitors()
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(1003, 5)), max_segments=5, layout="slots")
    records = _records(segs)
    kwargs = dict(direction=(1.0, 0.0, 0.0))
    piston = np.linspace(5.0, 5.5, len(mons))
    wfs = table.wavefront_all(segs, pupil=pupils, monitors=mons, piston=piston, **kwargs)
    for k, (wf, m, p) in enumerate(zip(wfs, mons, pupils)):
        assert wf.piston == piston[k]
        _assert_wavefront(wf, cases.reference(records, m, kwargs, p, piston[k]), terms=(4, 15))
    assert int(wfs[-1].counts) > 0 and int(wfs[0].outside) > 0


def test_more_monitors_than_one_group_streamed():
    """The 30 monitors and 1,003 rays above as two chunks of 512 and 491 rays, the second added with `into=`: every launch of the
    second call draws its own ticket, shares the call's partials and adds to what the first call left, with the first call's pistons."""
    assert wavefront_plan(cases.GROUP_MONITORS) == [(0, 28), (28, 2)]
    table = support.cfg2_table()
    mons, pupils = cases.group_monitors()
    o, d, intensity = cases.cfg2_arrays(1003, 5)
    chunks = [table.trace_batch(_batch(o[part], d[part], intensity[part]), max_segments=5, layout="slots") for part in (slice(0, 512), slice(512, 1003))]
    records = tuple(np.concatenate(parts) for parts in zip(*(_records(c) for c in chunks)))
    kwargs = dict(direction=(1.0, 0.0, 0.0))
    piston = np.linspace(5.0, 5.5, len(mons))
    wfs = table.wavefront_all(chunks[0], pupil=pupils, monitors=mons, piston=piston, **kwargs)
    table.wavefront_all(chunks[1], pupil=pupils, monitors=mons, into=wfs, **kwargs)
    for k, (wf, m, p) in enumerate(zip(wfs, mons, pupils)):
        assert wf.piston == piston[k]
        _assert_wavefront(wf, cases.reference(records, m, kwargs, p, piston[k]), terms=(4, 15))
    assert int(wfs[-1].counts) > 0


# -- closed forms, independent of the reference: one hand-made segment per ray --------------------------------------------------------
def _hand_batch(o, d, length, intensity=None, n_index=1.0, pathlength=0.0):
    n = len(o)
    segs = SegmentBatch(n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    for k, f in enumerate(("ox", "oy", "oz")):
        segs.field(f).copy_(torch.as_tensor(np.ascontiguousarray(o[:, k])))
    for k, f in enumerate(("dx", "dy", "dz")):
        segs.field(f).copy_(torch.as_tensor(np.ascontiguousarray(d[:, k])))
    segs.length.fill_(length)
    segs.intensity.copy_(torch.as_tensor(np.ones(n) if intensity is None else intensity))
    segs.field("n").fill_(n_index)
    segs.pathlength.fill_(pathlength)
    segs.ray.copy_(torch.arange(n, dtype=torch.int32))
    segs.count, segs.n_rays = torch.ones(n, dtype=torch.int32, device="cuda"), n
    return segs


def _cone(n, half_angle, seed, source=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    theta, phi = half_angle * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(theta), np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi)], axis=1)
    return np.tile(np.asarray(source, dtype=float), (n, 1)), d, 0.25 + 0.75 * rng.random(n)


def _closed_form(segs, mon, want, allowance=None, **kwargs):
    """wavefront_batch on `segs`; every Noll coefficient beyond the piston within its propagated bound (plus `allowance`) of `want`
    ({term number: value}, 0 elsewhere).  Returns (wavefront, reference)."""
    table = oa.OpticalTable()
    wf = table.wavefront_batch(mon, segs, piston=kwargs.pop("piston", 0.0), **kwargs)
    ref = cases.reference(_records(segs), mon, kwargs, kwargs["pupil"], wf.piston)
    _assert_wavefront(wf, ref)
    c = wf.coefficients().cpu().numpy()
    _, dc, _, _ = coefficient_bound(ref.sums, ref.bound, 15)
    expect = np.zeros(15)
    for k, v in want.items():
        expect[k - 1] = v
    extra = np.zeros(15) if allowance is None else allowance
    print(f"  coefficients 2..15 off by at most {np.abs(c - expect)[1:].max():.3g}; bounds {dc[1:].min():.3g} .. {dc[1:].max():.3g}")
    assert np.all(np.abs(c - expect)[1:] <= dc[1:] + extra[1:]), (c - expect, dc)
    return wf, ref


def test_a_point_source_referenced_to_itself():
    """Rays from F, referenced to F: W = 0 for every ray — rms and every coefficient beyond the piston within their bounds."""
    o, d, intensity = _cone(3001, 0.15, 11, source=(0.5, 0.1, -0.2))
    segs = _hand_batch(o, d, 9.0, intensity, pathlength=3.25)
    wf, ref = _closed_form(segs, oa.Monitor([3.0, 0, 0], 4, 4), {}, focus=(0.5, 0.1, -0.2), pupil=(0.0, 0.0, 0.16), piston=3.25)
    assert ref.counts[0] == 3001
    lo, hi = rms_interval(ref.sums, ref.bound, 1)
    assert float(wf.rms()) <= hi and hi < 1e-12 and abs(float(wf.mean()) - 3.25) <= 1e-12 and float(wf.strehl(1e-6)) > 1 - 1e-9


def test_a_focus_moved_sideways_is_tilt():
    """F = source + delta a_y: W = delta ty, so with p = ty / R the Noll-2 coefficient is delta R / 2 and the rest are 0."""
    delta, R = 0.003, 0.16
    o, d, intensity = _cone(3001, 0.15, 12)
    segs = _hand_batch(o, d, 9.0, intensity)
    mon = oa.Monitor([3.0, 0, 0], 4, 4)
    assert np.allclose(mon.tangent_Y, [0, 1, 0]) and np.allclose(mon.tangent_Z, [0, 0, 1])
    wf, ref = _closed_form(segs, mon, {2: delta * R / 2}, focus=(0.0, delta, 0.0), pupil=(0.0, 0.0, R))
    # nothing is left once the tilt is out: the residual Q - c . b cancels to the rounding its interval allows, far below the tilt
    hi = rms_interval(ref.sums, ref.bound, 3)[1]
    assert float(wf.rms(3)) <= hi < 1e-3 * float(wf.rms(1))


def test_a_focus_moved_along_the_normal_is_defocus():
    """F = source + delta normal, R = 0.05: W = delta sqrt(1 - rho^2 R^2) = delta (1 - rho^2 R^2 / 2 - rho^4 R^4 / 8 - ...), so the
    Noll-4 coefficient is -delta R^2 / (4 sqrt 3) to within the quartic term delta R^4 / 8 (which also feeds Noll 11 and the piston)."""
    delta, R = 0.01, 0.05
    o, d, intensity = _cone(4001, 0.05, 13)
    segs = _hand_batch(o, d, 9.0, intensity)
    quartic = delta * R**4 / 8
    allowance = np.zeros(15)
    allowance[[0, 3, 10]] = quartic
    wf, ref = _closed_form(segs, oa.Monitor([3.0, 0, 0], 4, 4), {4: -delta * R**2 / (4 * math.sqrt(3))}, allowance=allowance, focus=(delta, 0.0, 0.0),
                           pupil=(0.0, 0.0, R), piston=delta)
    assert ref.counts[0] == 4001 and quartic < 1e-8
    assert float(wf.rms(4)) <= quartic + rms_interval(ref.sums, ref.bound, 4)[1]


def test_a_tilted_collimated_bundle_is_tilt():
    """A collimated bundle along (cos theta, sin theta, 0), started on a plane normal to it, against direction = the monitor's
    normal: the ray from s e1 + z e2 meets the monitor at y = x_m tan theta + s / cos theta after t = x_m / cos theta +
    (y - x_m tan theta) sin theta, and W = t: pure tilt sin(theta) R / 2 in position coordinates about c_y = x_m tan theta."""
    theta, R, n = 0.02, 0.5, 3001
    rng = np.random.default_rng(14)
    r, phi = 0.45 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    D = np.array([math.cos(theta), math.sin(theta), 0.0])
    e1 = np.array([-math.sin(theta), math.cos(theta), 0.0])
    o = np.outer(r * np.cos(phi), e1) + np.outer(r * np.sin(phi), [0.0, 0.0, 1.0])
    segs = _hand_batch(o, np.tile(D, (n, 1)), 9.0, 0.25 + 0.75 * rng.random(n))
    wf, ref = _closed_form(segs, oa.Monitor([3.0, 0, 0], 4, 4), {2: math.sin(theta) * R / 2}, direction=(1.0, 0.0, 0.0),
                           pupil=(3.0 * math.tan(theta), 0.0, R), piston=3.0 / math.cos(theta))
    hi = rms_interval(ref.sums, ref.bound, 3)[1]
    assert ref.counts[0] == n and float(wf.rms(3)) <= hi < 1e-3 * float(wf.rms(1))


def test_lstsq_on_the_hit_lists(case1):
    """Another algorithm: np.linalg.lstsq on `record_all`'s hit lists (wavefrontList, tYList, tZList, IList) agrees with
    coefficients() within the propagated bounds plus lstsq's own rounding, 15 cond U max|W'| a coefficient (a backward-stable
    solve of a well-conditioned system whose right-hand side is W')."""
    table, get = case1
    segs, records = get("slots")
    su = cases.SETUPS["focus"]
    mon, pupil = cases.monitors_at(su["x"])[1], su["pupil"][1]
    wf = table.wavefront_batch(mon, segs, pupil=pupil, **su["kwargs"])
    ref = cases.reference(records, mon, su["kwargs"], pupil, wf.piston)
    (h,) = table.record_all(segs, monitors=[mon])
    Wl = h.wavefrontList(sort=None, **su["kwargs"]).cpu().numpy()
    p, q = (h.tYList(None).cpu().numpy() - pupil[0]) / pupil[2], (h.tZList(None).cpu().numpy() - pupil[1]) / pupil[2]
    w = h.IList(None).double().cpu().numpy()
    inside = p * p + q * q <= 1.0
    assert int(inside.sum()) == ref.counts[0] == int(wf.counts) and len(Wl) == ref.counts.sum()
    np.testing.assert_allclose(np.sort(Wl), np.sort(ref.W), rtol=0, atol=1e-12)
    root = np.sqrt(w[inside])
    design = (zernike(15, p[inside], q[inside]) * root).T
    Wp = Wl[inside] - wf.piston
    c, _, _, sv = np.linalg.lstsq(design, root * Wp, rcond=None)
    _, dc, _, _ = coefficient_bound(ref.sums, ref.bound, 15)
    own = 15 * (sv[0] / sv[-1]) * U * np.abs(Wp).max()
    got = wf.coefficients().cpu().numpy()
    got[0] -= wf.piston
    print(f"  lstsq against the sums: largest difference {np.abs(got - c).max():.3g}; bounds {dc.min():.3g} .. {dc.max():.3g} + {own:.3g}")
    assert np.all(np.abs(got - c) <= dc + own)


def test_determinism_and_streaming(case1):
    """The same call twice: the same bits.  Two halves of the rays through `into=` with the first call's piston: counts equal to the
    whole's and sums within the whole's bound."""
    table, get = case1
    su = cases.SETUPS["direction"]
    mons = cases.monitors_at(su["x"])
    for layout in ("slots", "append"):
        segs = get(layout)[0]
        a, b = (table.wavefront_all(segs, pupil=su["pupil"], monitors=mons, **su["kwargs"]) for _ in range(2))
        for x, y in zip(a, b):
            assert x.piston == y.piston and torch.equal(x.sums, y.sums) and torch.equal(x.counts, y.counts) and x.sums is not y.sums
    o, d, intensity = cases.cfg2_arrays(5003, 0)
    whole, records = get("slots")
    half = [table.trace_batch(_batch(o[s], d[s], intensity[s]), max_segments=5, layout="slots") for s in (slice(0, 2400), slice(2400, None))]
    first = table.wavefront_all(half[0], pupil=su["pupil"], monitors=mons, **su["kwargs"])
    pistons = [wf.piston for wf in first]
    again = table.wavefront_all(half[1], pupil=su["pupil"], monitors=mons, into=first, **su["kwargs"])
    assert again is first or all(x is y for x, y in zip(again, first))
    assert [wf.piston for wf in first] == pistons
    for wf, m, p in zip(first, mons, su["pupil"]):
        _assert_wavefront(wf, cases.reference(records, m, su["kwargs"], p, wf.piston))
    with pytest.raises(ValueError, match="piston"):
        table.wavefront_all(half[1], pupil=su["pupil"], monitors=mons, into=first, piston=0.125, **su["kwargs"])
    with pytest.raises(ValueError, match="into"):
        table.wavefront_all(half[1], pupil=(0.0, 0.0, 0.7), monitors=mons, into=first, **su["kwargs"])


def test_piston_none_against_an_explicit_piston(case1):
    table, get = case1
    segs, records = get("tiled")
    su = cases.SETUPS["focus"]
    mons = cases.monitors_at(su["x"])
    auto = table.wavefront_all(segs, pupil=su["pupil"], monitors=mons, **su["kwargs"])
    zero = table.wavefront_all(segs, pupil=su["pupil"], monitors=mons, piston=0.0, **su["kwargs"])
    for a, z in zip(auto, zero):
        s = z.sums.cpu().numpy()
        assert a.piston == (s[45] / s[0] if s[0] else 0.0)  # the mean of W the pass with piston 0 found
    same = table.wavefront_all(segs, pupil=su["pupil"], monitors=mons, piston=[wf.piston for wf in auto], **su["kwargs"])
    for a, s, z, m, p in zip(auto, same, zero, mons, su["pupil"]):
        assert torch.equal(a.sums, s.sums) and torch.equal(a.counts, s.counts)
        assert torch.equal(a.counts, z.counts) and torch.equal(a.outside, z.outside) and torch.equal(a.sums[:45], z.sums[:45])
        if int(a.counts) < 60:
            continue
        # the piston moves the sums, not what they say: mean, coefficients beyond the piston and rms agree within both bounds
        ra, rz = cases.reference(records, m, su["kwargs"], p, a.piston), cases.reference(records, m, su["kwargs"], p, 0.0)
        (_, da, _, _), (_, dz, _, _) = coefficient_bound(ra.sums, ra.bound, 15), coefficient_bound(rz.sums, rz.bound, 15)
        diff = np.abs(a.coefficients().cpu().numpy() - z.coefficients().cpu().numpy())
        assert np.all(diff <= da + dz + 4 * U * abs(a.piston)), (diff, da + dz)
        assert rms_interval(ra.sums, ra.bound, 1)[0] <= float(a.rms()) <= rms_interval(ra.sums, ra.bound, 1)[1]


def test_single_precision_is_refused():
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(130, 3)
    segs = table.trace_batch(_batch(o, d, intensity, precision="f32"), max_segments=3)
    assert segs.precision == "f32"
    with pytest.raises(ValueError, match="double-precision"):
        table.wavefront_all(segs, direction=(1, 0, 0), monitors=[oa.Monitor([7.5, 0, 0], 6, 6)])
    with pytest.raises(ValueError, match="double-precision"):
        get_engine().monitor_wavefront_many([monitor_struct(oa.Monitor([7.5, 0, 0], 6, 6))], np.array([[0, 1, 0, 0, 0, 1.0]]), 1, np.array([[1.0, 0, 0]]), 1,
                                            np.array([[0, 0, 1.0]]), np.zeros(1), segs)


def test_no_segments():
    table, eng = support.cfg2_table(), get_engine()
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    for wf in table.wavefront_all(none, direction=(1, 0, 0), monitors=cases.monitors_at(7.5)[:2]):
        assert wf.to_host()[:2] == (0, 0) and not wf.sums.any() and wf.piston == 0.0 and math.isnan(float(wf.rms()))
    assert table.wavefront_all(none, direction=(1, 0, 0), monitors=[]) == []


# -- the C ABI -------------------------------------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / sums of M monitors for ot_monitor_wavefront_many, with a guard region on either side of each."""

    def __init__(self, M):
        super().__init__(guard=64, counts=(torch.int64, (M, 2)), sums=(torch.float64, (M, 61)))


def test_abi_errors(ctx):
    lib, c = ctx
    n = 130
    segs = SegmentBatch(2 * n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    segs.dx.fill_(1.0)
    segs.length.fill_(10.0)
    segs.intensity.fill_(0.5)
    segs.field("n").fill_(1.0)
    segs.pathlength.fill_(0.25)
    segs.ray.copy_(torch.arange(2 * n, dtype=torch.int32) % n)
    segs.count, segs.n_rays = torch.full((n,), 2, dtype=torch.int32, device="cuda"), n
    m = oa.Monitor([5, 0, 0], 2, 2)
    mon = monitor_struct(m)
    out = _Out(1)
    src, n_segments, count, n_rays = segment_source(segs)
    good_axes, good_ref, good_pupil, good_piston = cases.axes_of(m).reshape(1, 6), np.array([[1.0, 0.0, 0.0]]), np.array([[0.25, -0.5, 1.0]]), np.array([5.0])
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, kind=1, ref=good_ref, coords=1, pupil=good_pupil, piston=good_piston, source=src,
             intensity=segs.intensity.data_ptr(), n_index=segs.field("n").data_ptr(), pathlength=segs.pathlength.data_ptr(), n_seg=n_segments,
             cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(), sums=out.sums.data_ptr(), acc=0):
        return lib.ot_monitor_wavefront_many(ctx_, mons, M, ptr(axes), kind, ptr(ref), coords, ptr(pupil), ptr(piston), None if source is None else C.byref(source),
                                             intensity, n_index, pathlength, n_seg, cnt, rays, counts, sums, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    def with_value(good, at, value):
        a = good.copy()
        a.flat[at] = value
        return a

    for null in ("ctx_", "mons", "axes", "ref", "pupil", "piston", "source", "n_index", "pathlength", "counts", "sums"):
        expect(call(**{null: None}), "NULL")
    no_field = altered()
    no_field.base[3] = None
    expect(call(source=no_field), "NULL field")
    expect(call(M=0), "n_monitors")
    expect(call(M=-3), "n_monitors")
    expect(call(M=(1 << 20) + 1), "n_monitors")
    expect(call(kind=2), "reference_kind")
    expect(call(kind=-1), "reference_kind")
    expect(call(coords=2), "coordinates")
    expect(call(coords=-1), "coordinates")
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
    expect(call(pupil=with_value(good_pupil, 0, np.nan)), "pupil")
    expect(call(pupil=with_value(good_pupil, 2, 0.0)), "radius")
    expect(call(pupil=with_value(good_pupil, 2, -1.0)), "radius")
    expect(call(pupil=with_value(good_pupil, 2, np.inf)), "pupil")
    expect(call(piston=np.array([np.nan])), "piston")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    assert call(kind=0, ref=np.zeros((1, 3))) == 0, lib.ot_last_error()  # (a focus at the monitor's origin is no zero direction)
    # the context is still good: each of the 2 n segments runs from x = 0 to 10 along the axis and crosses the monitor at x = 5 at
    # P = 0, t = 5: L = 5.25, W = L - P . u = 5.25, W' = 0.25, (p, q) = (-0.25, 0.5): binary fractions, every sum is exact
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    c2 = 2 * n
    want = np.array([0.5 * c2 * (-0.25) ** (g - b) * 0.5**b for g in range(9) for b in range(g + 1)]
                    + [0.5 * c2 * 0.25 * (-0.25) ** (g - b) * 0.5**b for g in range(5) for b in range(g + 1)] + [0.5 * c2 * 0.0625])
    assert out.counts[0].tolist() == [c2, 0] and out.guards_untouched()
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), want)
    assert call(acc=1) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    assert out.counts[0].tolist() == [2 * c2, 0]
    np.testing.assert_array_equal(out.sums[0].cpu().numpy(), 2 * want)
    assert call(intensity=None, pupil=np.array([[0.25, -0.5, 0.5]])) == 0 and lib.ot_ctx_synchronize(c) == 0  # weight 1; rho^2 = 1.25: outside
    assert out.counts[0].tolist() == [0, c2] and not out.sums.any() and out.guards_untouched()


def test_the_example_runs():
    """examples/wavefront.py as a user would run it: the spherical aberration of a biconvex lens, at the paraxial focus and at the
    best focus of the spots; the Noll-11 term is not zero and has the sign the reference computes from the same segments."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "wavefront.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split(":")[0].strip(): ln for ln in out.stdout.splitlines() if ":" in ln}
    assert "paraxial focus" in lines and "best focus" in lines, out.stdout
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import wavefront as example
    finally:
        sys.path.pop(0)
    table, mon, segs, focus, pupil = example.scene()
    wf = table.wavefront_batch(mon, segs, focus=focus, pupil=pupil)
    ref = cases.reference(_records(segs), mon, dict(focus=focus), pupil, wf.piston)
    c, dc, _, _ = coefficient_bound(ref.sums, ref.bound, 15)
    spherical = float(wf.coefficients()[10])
    assert abs(c[10]) > 100 * dc[10] and spherical != 0.0 and (spherical > 0) == (c[10] > 0)
    assert f"{spherical:.6e}" in lines["paraxial focus"], (spherical, lines["paraxial focus"])
