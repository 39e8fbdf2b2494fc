"""GPU (MI355X): coherent detector images — `OpticalTable.field_all` / `field_batch`, the phasors a exp(i phi) of every monitor's
hits summed per bin on the device by the field mode of k_mon_count (ot_monitor_field_many), with no hit list.

Reference, in every comparison: numpy on the hit lists of the verified path, h in table.record_all(...):
    a = sqrt(h.IList)   (h.IList itself for amplitude="linear"),   x = h.pathlengthList / wavelength[h.ray_index],
    phi = 2 pi (x - floor x),   np.histogram2d(h.yList, h.zList, bins=[y_edges, z_edges], weights=a cos phi | a sin phi | a | a X)
with X = (|pathlength| + |t n|) / wavelength, the size in cycles of what the phase was reduced from.  As tests/test_gpu_image.py
does, every comparison first asserts from the REFERENCE values that no y or z lies within 1e-9 of a bin edge.

Counts must be EQUAL.  re and im of a bin must agree within
    sum_j a_j (2 pi 8 u X_j + 16 u)  +  2 c u sum_j a_j,      u = 2^-53, c = the bin's count.
Derivation (not a measurement).  Both sides form L = pathlength + t n and x = L / wavelength in double precision.  Each rounding
moves x by at most u X cycles: two for L on either side (the product and the sum here, one fused operation and its operands on
the device: 2 + 2), one for the division on either side (1 + 1), and two spare for a last-bit difference in t between the record
and the field pass of the same test — 8 u X cycles, 2 pi 8 u X radians, and |d cos|, |d sin| <= |d phi|.  The reduction
x - floor x is exact (Sterbenz) and so is 2 f.  sincospi against numpy's cos / sin of 2 pi f: 2 pi f rounds once (2 pi u f <= 7 u),
either library is within 1 ulp (u each), the product a cos phi rounds once on either side (2 u), sqrt is correctly rounded on
both — 16 u covers it.  The second term is the image test's bound for two summation orders of the same c doubles, |terms| <= a_j.
Every comparison prints the largest error next to its bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from optable_amd import abi
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import field_plan, get_engine, segment_source
from optable_amd.monitors import image_edges
from optable_amd.table import monitor_struct
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

U = 2.0**-53


EMPTY, DROPS, SPREAD = 2, 6, 7


def _reference(h, wavelength, y_edges, z_edges, amplitude="sqrt", keep=None):
    """(counts, re, im, bound) per bin from the hit list `h` (of its hits `keep`, a boolean mask, when given), after asserting
    that no coordinate is within 1e-9 of an edge."""
    def host(t):
        return t.double().cpu().numpy()

    y, z, I = host(h.yList(None)), host(h.zList(None)), host(h.IList(None))
    L, lam = host(h.pathlengthList(None)), support.hit_wavelengths(wavelength, h)
    parts = np.abs(host(h._gather(h.segs.pathlength, h.slot))) + np.abs(host(h.t) * host(h._gather(h.segs.n_index, h.slot)))
    if keep is not None:
        y, z, I, L, lam, parts = (v[keep] for v in (y, z, I, L, lam, parts))
    if len(y):
        clear = min(np.abs(y[:, None] - y_edges[None, :]).min(), np.abs(z[:, None] - z_edges[None, :]).min())
        print(f"  {len(y)} hits, smallest distance to a bin edge {clear:.3g}")
        assert clear > 1e-9
    a = np.sqrt(I) if amplitude == "sqrt" else I
    x = L / lam
    phi = 2 * np.pi * (x - np.floor(x))
    X = parts / lam

    def hist(w=None):
        return np.histogram2d(y, z, bins=[y_edges, z_edges], weights=w)[0]

    c, sum_a = hist(), hist(a)
    bound = 2 * np.pi * 8 * U * hist(a * X) + 16 * U * sum_a + 2 * c * U * sum_a
    return c.astype(np.int64), hist(a * np.cos(phi)), hist(a * np.sin(phi)), bound


def _assert_against(counts, re, im, ref, what=""):
    c, ref_re, ref_im, bound = ref
    np.testing.assert_array_equal(counts, c)
    err = np.maximum(np.abs(re - ref_re), np.abs(im - ref_im))
    at = np.unravel_index(np.argmax(err), err.shape)
    print(f"  {what}{int(c.sum())} in range, most in a bin {int(c.max())}; re / im: largest error {err[at]:.3g}, bound there {bound[at]:.3g}")
    assert np.all(err <= bound), float((err - bound).max())
    return c


def _assert_field(f, h, wavelength, amplitude="sqrt"):
    counts, re, im, y_edges, z_edges = f.to_host()
    assert f.monitor is h.monitor and counts.dtype == np.int64 and re.dtype == im.dtype == np.float64
    assert counts.shape == re.shape == im.shape == (len(y_edges) - 1, len(z_edges) - 1) == f.bins
    return _assert_against(counts, re, im, _reference(h, wavelength, y_edges, z_edges, amplitude))


@pytest.fixture(scope="module")
def case1():
    """cfg 2, 5,003 rays, 5 segments, eight monitors, f64: (table, monitors, batch, {layout: (segs, record_all hits)}), traced and
    recorded on first use."""
    table, mons = support.cfg2_table(), support.eight_monitors()
    batch = support.weighted_batch(*scenes.cfg2_rays(5003, 0))
    return table, mons, batch, support.traced(table, lambda precision: batch, 5, lambda segs: table.record_all(segs, monitors=mons))


@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_and_the_passes_through_lds(case1, layout, monkeypatch):
    table, mons, batch, get = case1
    segs, hits = get(layout)
    assert field_plan(len(mons), 30, 30) == {"path": "lds", "per_pass": 3, "passes": 3}
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("field_all converted the batch")

    for wavelength in (scenes.WL, batch):  # one value for all rays; the traced batch, gathered by the segments' ray
        with monkeypatch.context() as mp:
            mp.setattr(SegmentBatch, "to_slots", refuse)
            mp.setattr(SegmentBatch, "astype", refuse)
            fields = table.field_all(segs, wavelength)  # the table's own monitors, in their order, bins=30
        assert len(fields) == len(mons) and all(f.monitor is m for f, m in zip(fields, mons))
        assert all(f.counts.is_cuda and f.counts.dtype == torch.int64 and f.re.dtype == f.im.dtype == torch.float64 for f in fields)
        totals = [int(_assert_field(f, h, wavelength).sum()) for f, h in zip(fields, hits)]
        assert len(hits[EMPTY]) == 0 and totals[EMPTY] == 0 and not fields[EMPTY].re.any() and not fields[EMPTY].im.any()
        assert 0 < totals[DROPS] < len(hits[DROPS])  # hits outside the image range are dropped
        assert all(t == len(h) for k, (t, h) in enumerate(zip(totals, hits)) if k != DROPS)
    # the phases are no constant: the field of the spread beam is far from the sum of the amplitudes
    spread = fields[SPREAD]
    ratio = float(spread.field.abs().sum()) / float(torch.sqrt(hits[SPREAD].IList(None)).sum())
    print(f"  spread beam: sum |F| / sum a = {ratio:.3g}")
    assert ratio < 0.9
    assert torch.equal(spread.intensity(), spread.re**2 + spread.im**2) and spread.field.dtype == torch.complex128
    two = table.field_all(segs, batch, monitors=[mons[3], mons[0]])  # ... or those given
    _assert_field(two[0], hits[3], batch)
    _assert_field(two[1], hits[0], batch)
    _assert_field(table.field_batch(mons[SPREAD], segs, scenes.WL, bins=(7, 5)), hits[SPREAD], scenes.WL)


def test_counts_repeat_and_match_the_incoherent_image(case1):
    table, mons, batch, get = case1
    segs, _ = get("slots")
    one, two = table.field_all(segs, batch, monitors=mons), table.field_all(segs, batch, monitors=mons)
    images = table.image_all(segs, monitors=mons)
    for a, b, im in zip(one, two, images):
        assert torch.equal(a.counts, b.counts) and torch.equal(a.counts, im.counts)


def test_per_ray_wavelengths_through_a_dispersive_slab():
    """The chromatic slab of scenes.g15_cfg4 (NBK7: the index, and with it the path length, depends on the ray's wavelength), 40
    base rays x three wavelengths: the wavelength of a hit comes through its segment's `ray`."""
    rng = np.random.default_rng(4)
    jit = rng.uniform(-0.3, 0.3, (40, 2))
    o = np.stack([np.full(40, -3.0), 2 + jit[:, 0], jit[:, 1]], axis=1)
    d = np.tile([np.cos(np.pi / 6), -np.sin(np.pi / 6), 0.0], (40, 1))
    base = RayBatch.from_arrays(o, d, wavelength=scenes.WL, intensity=0.25 + 0.75 * rng.random(40), q=support.Q, device="cuda")
    batch = base.multiplexed_in_wavelength([780e-7, 560e-7, 400e-7])
    assert batch.n == 120 and len(set(batch.wavelength.tolist())) == 3
    table = oa.OpticalTable()
    table.add_components([oa.GlassSlab([0, 0, 0], width=2, height=2, thickness=0.5, n1=oa.Vacuum(), n2=oa.Glass_NBK7(), reflectivity=0)])
    mon = oa.Monitor([2, -0.9, 0], 3, 3)
    segs = table.trace_batch(batch, max_segments=5)
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) == 120 and len(set(h._gather(segs.pathlength, h.slot).tolist())) == 3  # behind the slab: every colour its own optical path
    f = table.field_batch(mon, segs, batch, bins=(7, 5))
    assert int(_assert_field(f, h, batch).sum()) == 120
    # one wavelength for all is another field: the gather is not a no-op
    g = table.field_batch(mon, segs, 780e-7, bins=(7, 5))
    _assert_field(g, h, 780e-7)
    assert torch.equal(f.counts, g.counts) and float((f.field - g.field).abs().max()) > 0.1


def test_global_path_and_accumulation():
    """(80, 80): 6,400 bins, more than the LDS budget — every hit a global atomic.  And `into=` over the two chunks of a batch
    against the whole batch in one call: counts equal, the field within the sum of the two chunks' bounds."""
    table = support.cfg2_table()
    mon = oa.Monitor([7.5, 0, 0], 2, 2)
    assert field_plan(1, 80, 80)["path"] == "global"
    whole = support.weighted_batch(*scenes.cfg2_rays(2049, 3))
    segs = table.trace_batch(whole, max_segments=5, layout="slots")
    h = table.record_all(segs, monitors=[mon])[0]
    full = table.field_all(segs, whole, bins=(80, 80), monitors=[mon])
    assert int(_assert_field(full[0], h, whole).sum()) == len(h) >= 2049 and int((full[0].counts > 0).sum()) > 200
    for bins in ((80, 80), (30, 30)):  # ... and through LDS
        chunks = [whole.slice(0, 1024), whole.slice(1024, 2049)]
        parts = [table.trace_batch(b, max_segments=5, layout="slots") for b in chunks]
        fields = table.field_all(parts[0], chunks[0], bins=bins, monitors=[mon])
        first = fields[0].counts.clone()
        assert table.field_all(parts[1], chunks[1], bins=bins, monitors=[mon], into=fields) == fields
        refs = [_reference(table.record_all(p, monitors=[mon])[0], b, fields[0].y_edges, fields[0].z_edges) for p, b in zip(parts, chunks)]
        summed = tuple(r0 + r1 for r0, r1 in zip(*refs))
        counts, re, im, _, _ = fields[0].to_host()
        _assert_against(counts, re, im, summed, what=f"{bins} in two chunks: ")
        assert int(first.sum()) < int(counts.sum())
        once = table.field_all(segs, whole, bins=bins, monitors=[mon])[0]
        assert torch.equal(once.counts, fields[0].counts)
        # without `into=` a call starts from zero again
        assert torch.equal(table.field_all(parts[0], chunks[0], bins=bins, monitors=[mon])[0].counts, first)


def _michelson(arm_difference, amplitude="sqrt"):
    """A Michelson interferometer: 257 collimated rays along -y, a 50 % splitter at 45 degrees at the origin, a mirror at the end
    of either arm (x = L1: the reflected ray; y = -L2: the transmitted one) and a monitor in the output port (x = -2, unrotated:
    its lab tangents are its own axes).  Both rays of a tree reach the monitor at the same point with the same intensity; their
    paths differ by 2 (L1 - L2) whatever the ray's offset.  Returns (field, hits, batch)."""
    wl = 2.0**-14  # 610 nm in the table's centimetres; L1 - L2 is an exact binary multiple of it
    L1 = 3.0
    L2 = L1 - arm_difference * wl / 2
    assert (L1 - L2) * 2 / wl == arm_difference  # exact
    i, j = np.divmod(np.arange(257), 17)  # the first 257 points of a 17 x 17 grid over 0.5 x 0.5, clear of the bin edges
    o = np.stack([(i - 8) / 32 + 1 / 64, np.full(257, 2.0), (j - 8) / 32 + 1 / 64], axis=1)
    batch = RayBatch.from_arrays(o, np.tile([0.0, -1.0, 0.0], (257, 1)), wavelength=wl, device="cuda")
    table = oa.OpticalTable()
    table.add_components([oa.BeamSplitter([0, 0, 0], width=2, height=2, eta=0.5).RotZ(np.pi / 4),
                          oa.SquareMirror([L1, 0, 0], width=2, height=2).RotZ(np.pi),
                          oa.SquareMirror([0, -L2, 0], width=2, height=2).RotZ(np.pi / 2)])
    mon = oa.Monitor([-2, 0, 0], 0.6, 0.6)
    segs = table.trace_batch(batch, max_segments=8)  # a tree is 1 + 2 + 4 rays
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) == 2 * 257 and torch.equal(h.ray_index(None), torch.arange(257, device="cuda").repeat_interleave(2))
    np.testing.assert_allclose(h.IList(None).cpu().numpy(), 0.5, rtol=0, atol=1e-15)  # R T = T R: either arm carries half
    f = table.field_batch(mon, segs, batch, bins=4, amplitude=amplitude)
    return f, h, batch


@pytest.mark.parametrize("amplitude", ["sqrt", "linear"])
def test_michelson_known_answer(amplitude):
    a = np.sqrt(0.5) if amplitude == "sqrt" else 0.5
    f, h, batch = _michelson(1000.0, amplitude)  # 2 (L1 - L2) = 1000 wavelengths: bright
    c = _assert_field(f, h, batch, amplitude)
    assert c.sum() == 2 * 257 and np.all(c % 2 == 0) and np.all(c > 0)
    one_arm = a * c / 2  # sum of a over one arm, per bin
    got = f.intensity().cpu().numpy()
    print(f"  bright: largest relative error of |F|^2 {np.abs(got / (4 * one_arm**2) - 1).max():.3g}")
    np.testing.assert_allclose(got, 4 * one_arm**2, rtol=1e-6, atol=0)
    f, h, batch = _michelson(1000.5, amplitude)  # half a wavelength more: dark
    c = _assert_field(f, h, batch, amplitude)
    assert c.sum() == 2 * 257
    got = f.field.abs().cpu().numpy()
    print(f"  dark: largest |F| / sum a {(got / (a * c)).max():.3g}")
    assert np.all(got < 1e-6 * a * c)


class _Out(support.Sentinel):
    """counts / re / im of M monitors of nby x nbz bins and `skipped` for ot_monitor_field_many, filled with a sentinel."""

    def __init__(self, M, nby, nbz):
        image = (torch.float64, (M, nby, nbz))
        super().__init__(counts=(torch.int64, (M, nby, nbz)), re=image, im=image, skipped=(torch.int64, (1,)))


def _call(lib, ctx, mons, segs, nby, nbz, out, wavelength=None, n_wavelengths=0, uniform=0.0, mode=0, accumulate=0, source=None, **planes):
    src, n, count, n_rays = segment_source(segs)
    table = (abi.OtMonitor * len(mons))(*[monitor_struct(m) for m in mons])
    axes, edges = support.image_tables(mons, nby, nbz)
    dp = C.POINTER(C.c_double)
    plane = {f: planes.get(f, segs.field(f).data_ptr()) for f in ("intensity", "n", "pathlength")}
    return lib.ot_monitor_field_many(ctx, table, len(mons), axes.ctypes.data_as(dp), edges.ctypes.data_as(dp), nby, nbz,
                                     C.byref(src if source is None else source), plane["intensity"], plane["n"], plane["pathlength"],
                                     None if wavelength is None else wavelength.data_ptr(), n_wavelengths, uniform, mode, n,
                                     None if count is None else count.data_ptr(), n_rays, out.counts.data_ptr(), out.re.data_ptr(),
                                     out.im.data_ptr(), out.skipped.data_ptr(), accumulate)


def test_the_guard_on_the_wavelength_gather(case1):
    """The library is told of 100 wavelengths; the buffer holds all 5,003, so a missing guard reads valid memory and fails the
    assertions below: nothing can fault.  Hits of rays 100.. are left out and counted; the others are binned as ever."""
    table, mons, batch, get = case1
    segs, hits = get("slots")
    pick = [0, SPREAD]  # every hit of these two lies inside its image
    wl = batch.wavelength.double().contiguous()
    assert wl.numel() == 5003
    eng = get_engine()
    out = _Out(2, 30, 30)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, [mons[k] for k in pick], segs, 30, 30, out, wavelength=wl, n_wavelengths=100) == 0, eng.lib.ot_last_error()
    torch.cuda.synchronize()
    beyond = 0
    for k, m in enumerate(pick):
        h = hits[m]
        known = (h.ray_index(None) < 100).cpu().numpy()
        assert 0 < known.sum() < len(h)
        beyond += int((~known).sum())
        ey, ez = image_edges(mons[m], 30, 30)
        _assert_against(out.counts[k].cpu().numpy(), out.re[k].cpu().numpy(), out.im[k].cpu().numpy(), _reference(h, batch, ey, ez, keep=known))
    assert int(out.skipped.item()) == beyond > 0
    # ... with all of them told of, nothing is left out
    with eng.lock:
        assert _call(eng.lib, eng._ctx, [mons[k] for k in pick], segs, 30, 30, out, wavelength=wl, n_wavelengths=5003) == 0
    torch.cuda.synchronize()
    assert int(out.skipped.item()) == 0 and int(out.counts.sum()) == sum(len(hits[m]) for m in pick)


def _list_of_segments(n):
    """n segments (0, 0, 0) + t (1, 0, 0) of length 10 as a list, `ray` = 0 .. n - 1: the monitor at x = 5 sees every one at P = 0."""
    return support.list_segments(n, dx=1.0, length=10.0, intensity=0.25, n=1.0, pathlength=np.arange(n) / 8)


def test_field_all_refuses_a_field_with_hits_left_out():
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 2, 2)
    segs = _list_of_segments(130)
    assert segs.layout == "list" and segs.n_rays is None  # (a list does not know how many rays it came from)
    o, d = np.zeros((130, 3)), np.tile([1.0, 0.0, 0.0], (130, 1))
    f = table.field_batch(mon, segs, RayBatch.from_arrays(o, d, wavelength=0.5, device="cuda"), bins=(7, 5))
    # L = 5 + k / 8 at wavelength 1 / 2: every phase a multiple of pi / 2, all in bin (3, 2); a = sqrt(1 / 4)
    ref = np.zeros((7, 5))
    ref[3, 2] = 130
    np.testing.assert_array_equal(f.counts.cpu().numpy(), ref)
    quarter = np.arange(130) % 4
    np.testing.assert_allclose(f.re[3, 2].item(), 0.5 * np.array([1, 0, -1, 0])[quarter].sum(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(f.im[3, 2].item(), 0.5 * np.array([0, 1, 0, -1])[quarter].sum(), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="30 hits"):
        table.field_batch(mon, segs, RayBatch.from_arrays(o[:100], d[:100], wavelength=0.5, device="cuda"), bins=(7, 5))


def test_abi_errors(ctx):
    lib, c = ctx
    segs, mon = _list_of_segments(130), oa.Monitor([5, 0, 0], 2, 2)
    out = _Out(1, 7, 5)
    wl = torch.full((130,), 0.5, dtype=torch.float64, device="cuda")

    def call(**kw):
        kw.setdefault("uniform", 0.5)
        return _call(lib, c, [mon], segs, 7, 5, out, **kw)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, segment_source(segs)[0])

    expect(call(source=altered(width=4)), "width must be 8")  # single-precision segments: refused, not approximated
    expect(call(source=altered(width=2)), "width")
    for plane in ("intensity", "n", "pathlength"):
        expect(call(**{plane: None}), "NULL")
    no_field = altered()
    no_field.base[6] = None
    expect(call(source=no_field), "NULL field")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        expect(call(uniform=bad), "wavelength_uniform")
    expect(call(wavelength=wl, n_wavelengths=0), "n_wavelengths")
    expect(call(wavelength=wl, n_wavelengths=-1), "n_wavelengths")
    for mode in (2, -1):
        expect(call(mode=mode), "amplitude_mode")
    expect(call(accumulate=2), "accumulate")  # ... and what ot_monitor_image_many refuses
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good; the array and the one value give the same field
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    assert int(out.counts[0, 3, 2]) == 130 == int(out.counts.sum()) and int(out.skipped.item()) == 0
    re, im = out.re.clone(), out.im.clone()
    assert call(wavelength=wl, n_wavelengths=130, uniform=float("nan")) == 0 and lib.ot_ctx_synchronize(c) == 0
    assert torch.allclose(out.re, re, rtol=0, atol=1e-12) and torch.allclose(out.im, im, rtol=0, atol=1e-12)
    assert call(accumulate=1) == 0 and lib.ot_ctx_synchronize(c) == 0  # ... and once more on top
    assert int(out.counts[0, 3, 2]) == 260 and torch.allclose(out.re, 2 * re, rtol=0, atol=1e-12)
