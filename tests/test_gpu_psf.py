"""GPU (MI355X): the diffraction PSF — `OpticalTable.psf_all` / `psf_batch`, the plane waves of every monitor hit summed over a grid
of samples by k_mon_psf (ot_monitor_psf_many): a hit list, per-axis phasor tables in LDS and a complex product on the fp64 matrix
cores, with no transcendental per pixel and no floating-point atomic.

Reference, in every comparison: tests/psf_reference.py on the segment records copied from the device — the header's definition in
numpy, the phases in np.longdouble.  Every case first asserts, from the REFERENCE, that no hit decision lies within 1e-7 of its
boundary.  Counts (used, skipped, aliased) must then be EQUAL and every sample of the field within the accuracy contract's bound,
norm (2 pi E + 2^-38), which the reference computes from the data; norm itself within the roundings of its sum."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys
import warnings

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
from optable_amd.engine import get_engine, psf_plan, segment_source
from optable_amd.psf import psf_grid
from optable_amd.table import monitor_struct
from optable_amd.wavefront import wavefront_reference as reference_tables
from psf_reference import airy, disc_grid, psf_reference
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = scenes.WL
WORST = [0.0]  # the largest device-against-reference error of the session, as a fraction of its bound


def _batch(o, d, intensity, precision="f64", wavelength=WL):
    return RayBatch.from_arrays(o, d, wavelength=wavelength, intensity=intensity, q=support.Q, precision=precision, device="cuda")


def _records(segs):
    """The valid segment records of a batch, copied from the device, by name."""
    return dict(zip(("o", "d", "length", "intensity", "n", "pathlength", "ray"), support.host_records(segs, "n", "pathlength", "ray")))


def _reference(rec, mon, kwargs, step, pixels, wavelength=WL, centre=(0.0, 0.0), amplitude="sqrt"):
    kind, _, local = reference_tables(kwargs.get("focus"), kwargs.get("direction"), [mon])
    grid, (ny, nz), _, _ = psf_grid(step, pixels, centre, 1)
    s = monitor_struct(mon)
    ref = psf_reference(rec["o"], rec["d"], rec["length"], rec["intensity"], rec["n"], rec["pathlength"], rec["ray"], list(s.M), list(s.origin), s.half_width,
                        s.half_height, cases.axes_of(mon), kind, local[0], grid[0], ny, nz, wavelength, ("sqrt", "linear", "unit").index(amplitude))
    assert ref.margin > cases.MARGIN  # a condition on the inputs
    return ref


def _assert_psf(psf, ref):
    """Counts equal, the field within the contract's bound, norm within the roundings of its sum."""
    used, skipped, aliased, norm, field = psf.to_host()
    assert psf.re.is_cuda and psf.im.is_cuda and psf.norm.is_cuda and psf.counts.is_cuda and field.shape == ref.field.shape
    assert (used, skipped, aliased) == tuple(ref.counts)
    assert abs(norm - ref.norm) <= (used + 2) * 2.0**-52 * ref.norm
    err = float(np.abs(field - ref.field).max()) if field.size else 0.0
    share = err / ref.bound if ref.bound else 0.0
    WORST[0] = max(WORST[0], share)
    print(f"  {used} hits, {field.shape}: largest error {err:.3g}, {share:.3g} of the bound {ref.bound:.3g} (norm {ref.norm:.4g}); session {WORST[0]:.3g}")
    assert err <= ref.bound, (err, ref.bound)
    if used == 0:
        assert norm == 0.0 and not field.any() and torch.isnan(psf.normalised()).all() and math.isnan(float(psf.strehl("peak")))
        assert np.isnan(psf.mtf()[0]).all() and np.isnan(psf.encircled_energy([1.0])).all()


# cfg 2 (tests/wavefront_cases.py): "focus": monitors in the diverging cone at x = 2.5 (half angle 0.15: |gy dy| <= 0.075 at half a
# wavelength a sample); "direction": monitors in the collimated beam at x = 7.5 (radius 0.75: |gy dy| <= 0.2 at 2e-5 a sample)
STEP = {"focus": 0.5 * WL, "direction": 2e-5}


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 130 rays, 5 segments, traced once per layout: (table, get(layout) -> (segs, records))."""
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(130, 3)
    return table, support.traced(table, lambda precision: _batch(o, d, intensity, precision), 5, _records)


@pytest.mark.parametrize("setup", ["focus", "direction"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts(case1, layout, setup, monkeypatch):
    table, get = case1
    segs, rec = get(layout)
    su = cases.SETUPS[setup]
    mons = cases.monitors_at(su["x"])
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("psf_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        psfs = table.psf_all(segs, WL, step=STEP[setup], pixels=(17, 33), **su["kwargs"])  # the table's own monitors
    assert len(psfs) == len(mons) and all(p.monitor is m for p, m in zip(psfs, mons)) and psfs[0].reference[0] == setup
    for p, m in zip(psfs, mons):
        _assert_psf(p, _reference(rec, m, su["kwargs"], STEP[setup], (17, 33)))
    assert int(psfs[0].counts) >= 130 and int(psfs[cases.EMPTY].counts) == 0 and int(psfs[3].counts) > 0
    one = table.psf_batch(mons[3], segs, WL, step=STEP[setup], pixels=(17, 33), **su["kwargs"])
    assert torch.equal(one.re, psfs[3].re) and torch.equal(one.im, psfs[3].im) and torch.equal(one.norm, psfs[3].norm)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1027])
def test_ray_counts(n):
    """Every ray of cfg 2 crosses the monitor at x = 7.5: n hits or more — a partial batch of 16, a full and an overfull wave, a round
    of 256 and one more hit, and at 1,027 rays three chunks or more with a ragged last one."""
    table = support.cfg2_table()
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(n, 3)), max_segments=5, layout="slots")
    rec, mon, kwargs = _records(segs), oa.Monitor([7.5, 0, 0], 6, 6), dict(direction=(1.0, 0.0, 0.0))
    ref = _reference(rec, mon, kwargs, 2e-5, (19, 21))
    hits = int(ref.counts[0])
    assert hits >= n and psf_plan(19, 21, [hits])["chunks"] == [-(-hits // 512)] and (n != 1027 or hits > 1024)
    _assert_psf(table.psf_batch(mon, segs, WL, step=2e-5, pixels=(19, 21), **kwargs), ref)


def test_more_than_one_hit_chunk(case1):
    """The plan's smallest chunk is 512 hits: the 514 of 257 rays (each crosses the monitor on its way to the mirrors and back) are two
    chunks of 257, whose partial images the last workgroup adds."""
    table = support.cfg2_table()
    segs = table.trace_batch(_batch(*cases.cfg2_arrays(257, 4)), max_segments=5, layout="append")
    rec, mon, kwargs = _records(segs), oa.Monitor([7.5, 0, 0], 6, 6), dict(direction=(1.0, 0.0, 0.0))
    ref = _reference(rec, mon, kwargs, 2e-5, (33, 17))
    plan = psf_plan(33, 17, [int(ref.counts[0])])
    assert 512 < ref.counts[0] <= 1024 and plan["chunks"] == [2] and plan["chunk_hits"] == [-(-int(ref.counts[0]) // 2)]
    _assert_psf(table.psf_batch(mon, segs, WL, step=2e-5, pixels=(33, 17), **kwargs), ref)


@pytest.mark.parametrize("pixels", [(1, 1), (1, 7), (16, 16), (33, 17), (65, 65), (512, 3)])
def test_pixel_tiles(case1, pixels):
    """One sample; less than a subtile; exactly one; 3 x 2 subtiles with ragged edges; four tiles of 2 + 3 subtiles an axis; eight
    tiles of 64 x 3."""
    table, get = case1
    segs, rec = get("slots")
    mon, kwargs = oa.Monitor([7.5, 0, 0], 6, 6), dict(direction=(1.0, 0.0, 0.0))
    step = (2e-6, 2e-5) if pixels[0] == 512 else 2e-5
    _assert_psf(table.psf_batch(mon, segs, WL, step=step, pixels=pixels, **kwargs), _reference(rec, mon, kwargs, step, pixels))


def test_monitors_with_grids_of_their_own(case1):
    """Four monitors, each with its own centre, one of them never hit: zeros, norm 0 and NaN methods for that one."""
    table, get = case1
    segs, rec = get("tiled")
    su = cases.SETUPS["direction"]
    mons = cases.monitors_at(su["x"])
    centres = [(0.0, 0.0), (1e-4, -5e-5), (0.0, 0.0), (-2e-4, 1e-4)]
    psfs = table.psf_all(segs, WL, step=(2e-5, 1e-5), pixels=(21, 40), centre=centres, monitors=mons, **su["kwargs"])
    for p, m, c in zip(psfs, mons, centres):
        assert p.centre == c
        _assert_psf(p, _reference(rec, m, su["kwargs"], (2e-5, 1e-5), (21, 40), centre=c))
    assert int(psfs[cases.EMPTY].counts) == 0 and float(psfs[cases.EMPTY].norm) == 0.0


def test_lists_and_trees():
    """Ray trees of the slab with reflectivity 0.2 (every hit splits; n = 1.5 inside), 64 wavelengths through the RayBatch: the
    [k][tree] slots with count[i], the append block and the dense list with holes."""
    table = oa.OpticalTable()
    table.add_components(W.cfg4_components(oa, reflectivity=0.2))
    o, d, wl = W.cfg4_rays(5, 4)  # x 64 wavelengths = 320 trees
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * W.W0**2 / wl)
    mons = [oa.Monitor([-1.5, 1.0, 0], 4, 4), oa.Monitor([1.5, -0.5, 0], 4, 4)]
    kwargs = dict(direction=(1.0, 0.2, 0.0))
    eng = get_engine()
    eng.upload(table.compile())
    table_wl = batch.wavelength.double().cpu().numpy()
    for segs, layout in ((eng.trace_trees(batch, 12, layout="slots"), "slots"), (eng.trace_trees(batch, 12, layout="append"), "append"),
                         (eng.trace_tree(batch, 12), "list")):
        assert segs.layout == layout
        rec = _records(segs)
        for p, m in zip(table.psf_all(segs, batch, step=2e-6, pixels=(17, 18), monitors=mons, **kwargs), mons):
            ref = _reference(rec, m, kwargs, 2e-6, (17, 18), wavelength=table_wl)
            _assert_psf(p, ref)
            assert ref.counts[0] >= 320 and ref.counts[1] == 0  # every tree crosses each monitor


def test_per_ray_wavelengths_and_a_ray_without_one(case1):
    """Wavelengths by the segments' `ray`; a ray whose wavelength is not positive (or not finite) is counted in `skipped` and adds
    nothing.  (psf_all refuses such a RayBatch: through the engine's own call.)"""
    table, get = case1
    segs, rec = get("append")
    mon, kwargs = oa.Monitor([7.5, 0, 0], 6, 6), dict(direction=(1.0, 0.0, 0.0))
    o, d, intensity = cases.cfg2_arrays(130, 3)
    wl = WL * (1.0 + 0.1 * np.random.default_rng(9).random(130))
    psf = table.psf_batch(mon, segs, _batch(o, d, intensity, wavelength=wl), step=2e-5, pixels=(17, 33), **kwargs)
    _assert_psf(psf, _reference(rec, mon, kwargs, 2e-5, (17, 33), wavelength=wl))
    wl[7], wl[40], wl[99] = 0.0, -WL, np.nan
    kind, _, local = reference_tables(None, (1.0, 0.0, 0.0), [mon])
    grid, pixels, step, centres = psf_grid(2e-5, (17, 33), (0.0, 0.0), 1)
    counts, norm, re, im = get_engine().monitor_psf_many([monitor_struct(mon)], cases.axes_of(mon).reshape(1, 6), kind, local, grid, pixels, segs,
                                                         torch.as_tensor(wl, device="cuda"))
    got = oa.MonitorPSF(mon, counts[0], norm[0], re[0], im[0], ("direction", (1.0, 0.0, 0.0)), grid[0], step, centres[0], "sqrt")
    ref = _reference(rec, mon, kwargs, 2e-5, (17, 33), wavelength=wl)
    assert ref.counts[1] >= 3 and ref.counts[0] + ref.counts[1] >= 130
    _assert_psf(got, ref)
    short = get_engine().monitor_psf_many([monitor_struct(mon)], cases.axes_of(mon).reshape(1, 6), kind, local, grid, pixels, segs,
                                          torch.as_tensor(wl[:100], device="cuda"))  # rays 100 .. 129 have no entry
    assert short[0][0].tolist() == _reference(rec, mon, kwargs, 2e-5, (17, 33), wavelength=wl[:100]).counts.tolist() and int(short[0][0, 1]) >= 32


@pytest.mark.parametrize("amplitude", ["sqrt", "linear", "unit"])
def test_amplitude_modes(case1, amplitude):
    table, get = case1
    segs, rec = get("slots")
    mon, su = oa.Monitor([2.5, 0, 0], 6, 6), cases.SETUPS["focus"]
    psf = table.psf_batch(mon, segs, WL, step=0.5 * WL, pixels=(9, 20), amplitude=amplitude, **su["kwargs"])
    ref = _reference(rec, mon, su["kwargs"], 0.5 * WL, (9, 20), amplitude=amplitude)
    _assert_psf(psf, ref)
    assert psf.amplitude == amplitude and (amplitude != "unit" or ref.norm == float(ref.counts[0]) >= 130.0)


def test_a_grid_coarse_enough_to_alias(case1):
    """At 5 wavelengths a sample the rays beyond |ty| or |tz| = 0.1 of the 0.15 cone turn more than half a cycle a sample."""
    table, get = case1
    segs, rec = get("slots")
    mon, su = oa.Monitor([2.5, 0, 0], 6, 6), cases.SETUPS["focus"]
    ref = _reference(rec, mon, su["kwargs"], 5 * WL, (17, 17))
    assert 0 < ref.counts[2] < ref.counts[0]
    with pytest.warns(RuntimeWarning, match=f"{ref.counts[2]} hits are aliased") as caught:
        psf = table.psf_batch(mon, segs, WL, step=5 * WL, pixels=(17, 17), **su["kwargs"])
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    _assert_psf(psf, ref)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        table.psf_batch(mon, segs, WL, step=0.5 * WL, pixels=(17, 17), **su["kwargs"])


def test_determinism_and_streaming():
    """The same call twice: the same bits.  Two chunks of the rays through `into=`: counts added, the field within the bound of the
    one-call reference."""
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(1027, 3)
    su = cases.SETUPS["direction"]
    mons = cases.monitors_at(su["x"])
    args = dict(step=2e-5, pixels=(33, 65), monitors=mons, **su["kwargs"])
    for layout in ("slots", "append"):
        segs = table.trace_batch(_batch(o, d, intensity), max_segments=5, layout=layout)
        a, b = (table.psf_all(segs, WL, **args) for _ in range(2))
        for x, y in zip(a, b):
            assert torch.equal(x.re, y.re) and torch.equal(x.im, y.im) and torch.equal(x.norm, y.norm) and torch.equal(x.counts, y.counts) and x.re is not y.re
    rec = _records(segs)
    half = [table.trace_batch(_batch(o[s], d[s], intensity[s]), max_segments=5, layout="slots") for s in (slice(0, 600), slice(600, None))]
    first = table.psf_all(half[0], WL, **args)
    part = [int(p.counts) for p in first]
    again = table.psf_all(half[1], WL, into=first, **args)
    assert all(x is y for x, y in zip(again, first))
    for p, m, k in zip(first, mons, part):
        ref = _reference(rec, m, su["kwargs"], 2e-5, (33, 65))
        assert k <= int(p.counts) == ref.counts[0]
        _assert_psf(p, ref)
    with pytest.raises(ValueError, match="into"):
        table.psf_all(half[1], WL, into=first, **{**args, "step": 1e-5})


def test_single_precision_is_refused():
    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(130, 3)
    segs = table.trace_batch(_batch(o, d, intensity, precision="f32"), max_segments=3)
    assert segs.precision == "f32"
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    with pytest.raises(ValueError, match="double-precision"):
        table.psf_all(segs, WL, direction=(1, 0, 0), step=2e-5, monitors=[mon])
    with pytest.raises(ValueError, match="double-precision"):
        get_engine().monitor_psf_many([monitor_struct(mon)], np.array([[0, 1, 0, 0, 0, 1.0]]), 1, np.array([[1.0, 0, 0]]), np.array([[0, 1e-5, 0, 1e-5]]), (3, 3),
                                      segs, WL)


def test_no_segments():
    table, eng = support.cfg2_table(), get_engine()
    eng.upload(table.compile())
    none = eng.trace_tree(RayBatch(0, "f64", "cuda"), 5)
    assert none.layout == "list" and none.n_valid == 0
    for p in table.psf_all(none, WL, direction=(1, 0, 0), step=2e-5, pixels=5, monitors=cases.monitors_at(7.5)[:2]):
        assert p.to_host()[:4] == (0, 0, 0, 0.0) and not p.re.any() and not p.im.any() and math.isnan(float(p.strehl()))
    assert table.psf_all(none, WL, direction=(1, 0, 0), step=2e-5, monitors=[]) == []


# -- the C ABI -------------------------------------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / norm / re / im of M monitors of ny x nz samples, with a guard region on either side of each."""

    def __init__(self, M, ny, nz):
        field = (torch.float64, (M, ny, nz))
        super().__init__(guard=64, counts=(torch.int64, (M, 3)), norm=(torch.float64, (M,)), re=field, im=field)


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
    ny, nz = 5, 18
    out = _Out(1, ny, nz)
    src, n_segments, count, n_rays = segment_source(segs)
    good_axes, good_ref, good_grid = cases.axes_of(m).reshape(1, 6), np.array([[1.0, 0.0, 0.0]]), np.array([[-2e-5, 1e-5, -8.5e-5, 1e-5]])
    wl = torch.full((n,), 0.5, dtype=torch.float64, device="cuda")
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731

    def call(ctx_=c, mons=C.byref(mon), M=1, axes=good_axes, kind=1, ref=good_ref, grid=good_grid, ny_=ny, nz_=nz, source=src,
             intensity=segs.intensity.data_ptr(), n_index=segs.field("n").data_ptr(), pathlength=segs.pathlength.data_ptr(), wavelength=None, n_wl=0,
             uniform=0.5, mode=0, n_seg=n_segments, cnt=count.data_ptr(), rays=n_rays, counts=out.counts.data_ptr(), norm=out.norm.data_ptr(),
             re=out.re.data_ptr(), im=out.im.data_ptr(), acc=0):
        return lib.ot_monitor_psf_many(ctx_, mons, M, ptr(axes), kind, ptr(ref), ptr(grid), ny_, nz_, None if source is None else C.byref(source), intensity,
                                       n_index, pathlength, wavelength, n_wl, uniform, mode, n_seg, cnt, rays, counts, norm, re, im, acc)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, src)

    def with_value(good, at, value):
        a = good.copy()
        a.flat[at] = value
        return a

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
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good: each of the 2 n segments runs from x = 0 to 10 along the axis and crosses the monitor at x = 5 at
    # P = 0, t = 5: L = 5.25 = W, 10.5 cycles at lambda 0.5, gy = gz = 0: every sample is a exp(i pi) = -0.5 a hit, exactly
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    c2 = 2 * n
    assert out.counts[0].tolist() == [c2, 0, 0] and float(out.norm[0]) == 0.5 * c2 and out.guards_untouched()
    assert bool((out.re == -0.5 * c2).all()) and float(out.im.abs().max()) <= 0.5 * c2 * 2.0**-50
    assert call(acc=1, wavelength=wl.data_ptr(), n_wl=n, uniform=0.0) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top, by the table
    assert out.counts[0].tolist() == [2 * c2, 0, 0] and float(out.norm[0]) == c2 and bool((out.re == -1.0 * c2).all())
    assert call(mode=2, intensity=None, kind=0, ref=np.zeros((1, 3))) == 0 and lib.ot_ctx_synchronize(c) == 0  # unit amplitudes need no intensity; F = the hit
    assert out.counts[0].tolist() == [c2, 0, 0] and float(out.norm[0]) == c2 and bool((out.re == -1.0 * c2).all()) and out.guards_untouched()
    assert call(n_seg=0, cnt=None, rays=0) == 0 and lib.ot_ctx_synchronize(c) == 0  # no segments: zeros
    assert not out.counts.any() and not out.norm.any() and not out.re.any() and not out.im.any() and out.guards_untouched()


# -- physics on the device --------------------------------------------------------------------------------------------------------------
def test_a_converging_cone_gives_the_airy_pattern():
    """The 1,257-ray cone of tests/test_psf_cpu.py — a 41 x 41 grid of direction cosines clipped to NA 0.1 — aimed through free
    space (beyond cfg 2's last component) at F from the sphere of radius 2 about it, onto a monitor one unit in front of F: the Airy
    pattern to 5e-3 of the peak on 33 x 33 samples out to 3 Airy radii, and a Strehl ratio of 1 to within the bound."""
    NA, F = 0.1, np.array([30.0, 0.0, 0.0])
    t = disc_grid(41, NA)
    d = np.stack([np.sqrt(1.0 - (t * t).sum(axis=1)), t[:, 0], t[:, 1]], axis=1)
    table = support.cfg2_table()
    segs = table.trace_batch(RayBatch.from_arrays(F - 2.0 * d, d, wavelength=WL, device="cuda"), max_segments=2, layout="slots")
    mon = oa.Monitor([29.0, 0, 0], 1, 1)
    step = 6 * 0.61 * WL / NA / 32
    psf = table.psf_batch(mon, segs, WL, focus=F, step=step, pixels=33)
    ref = _reference(_records(segs), mon, dict(focus=F), step, 33)
    assert ref.counts.tolist() == [1257, 0, 0]
    _assert_psf(psf, ref)
    v = 2 * np.pi * NA * np.hypot(psf.y[:, None], psf.z[None, :]) / WL
    err = float(np.abs(psf.normalised().cpu().numpy() - airy(v)).max())
    print(f"  Airy pattern: largest error {err:.3g} of the peak")
    assert err <= 5e-3
    slack = ref.bound / ref.norm
    assert (1 - slack) ** 2 <= float(psf.strehl("reference")) <= (1 + slack) ** 2 and float(psf.strehl("peak")) == float(psf.strehl())
    ee = psf.encircled_energy([0.61 * WL / NA, 3 * 0.61 * WL / NA])
    assert 0.7 < ee[0] < 0.95 and ee[1] > ee[0]  # (83.8 % of ALL the energy lies in the Airy disc; here of what the grid holds)


def test_the_example_runs():
    """examples/psf.py as a user would run it: the biconvex lens at its paraxial and at its best focus, the true Strehl ratio beside
    Marechal's."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "psf.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split(":")[0].strip(): ln for ln in out.stdout.splitlines() if ":" in ln}
    assert "paraxial focus" in lines and "best focus" in lines and "MTF" in lines and "encircled energy" in lines, out.stdout
    strehl = [float(lines[k].split("Strehl")[1].split()[0]) for k in ("paraxial focus", "best focus")]
    assert 0.0 < strehl[0] < strehl[1] <= 1.0, strehl
