"""GPU (MI355X): coherent Gaussian-beam detector images — `OpticalTable.wave_all` / `wave_batch`, the complex sum of the hits'
Gaussian beams sampled at the bin centres by k_mon_wave (ot_monitor_wave_many), with no hit list.

Reference, in every comparison: numpy on the hit lists of the verified path, h in table.record_all(...), over ALL bin centres
(yc, zc) = midpoints of the edges, with no cut at 6 w:
    y0 = h.yList, z0 = h.zList, ty = h.tYList, tz = h.tZList, q = q[slot] + t, w^2 = wavelength |q|^2 / (n pi qi),
    cycles = (pathlength + t n) / wavelength + n (ty Dy + tz Dz) / wavelength + n qr (Dy^2 + Dz^2) / (2 wavelength |q|^2),
    u = a sqrt(2 / (pi w^2)) exp(-(Dy^2 + Dz^2) / w^2) exp(i (2 pi frac(cycles) - g)),  Dy = yc - y0, Dz = zc - z0,
    field[ky, kz] = sum over the hits of u,   counts = np.histogram2d(y0, z0, bins=[y_edges, z_edges]),
a = sqrt(I) or I, g = arctan2(qr, qi) or 0.  Every comparison first asserts from the REFERENCE values that no centre lies within
1e-9 of a bin edge.  counts must be EQUAL, to the reference and to `image_all`'s.

re and im of a bin must agree within the bound derived here (not measured), u = 2^-53, per hit and bin, as a fraction of |u|:
  * phase, 2 pi times an error in cycles.  The device forms f = frac(fma(t, n, pathlength) / wavelength), nw = n / wavelength,
    ry = nw ty with ty three products (in another order and contraction than torch's matrix product: its error is 3 u S_t,
    S_t = |d| . |a_y| >= |ty|, so S_t stands for |ty| below), kc = n qr / (2 wavelength |q|^2) (qr = q_re + t, two squares, a sum,
    three products, a division), and x = f + D (ry + kc D): at most 3 roundings on the path term, 8 on a tilt term and 12 on the
    curvature term, each relative to its own term or to a partial sum no larger than X = |L| / wavelength
    + n (S_ty |Dy| + S_tz |Dz|) / wavelength + n |qr| (Dy^2 + Dz^2) / (2 wavelength |q|^2).  numpy does the same work without the
    fused step.  Twelve a side: K = 24, an error of K u X cycles.
  * the cancellation in D = yc - y0.  yc = (e[k] + e[k + 1]) / 2 is the same double on both sides; y0 = P . a_y is three products
    and two sums in another order here than there: |d y0| <= 8 u S, S = |P| . |a_y|.  It moves the phase by 2 pi (|n ty /
    wavelength| + |n qr D / (wavelength |q|^2)|) dD — the cycle rate — and the envelope's exponent by 2 |D| dD / w^2.
  * a last-bit difference in t between the record pass and this one: dt = 4 u |t| (twice one ulp).  It moves L by n dt, y0 by
    S_t dt, qr by dt: the curvature by n (Dy^2 + Dz^2) dt / (2 wavelength |q|^2) cycles and w^2 by 2 |qr| dt / |q|^2 relative.
  * the envelope exp(-(Dy^2 + Dz^2) / w^2): w^2 is 9 roundings a side, the square and the division 2: the exponent moves by 24 u of
    itself; the device takes one exp per axis, numpy one: (2 E_EXP + 1) ulp of exp.
  * the phasor: two sincospi on the device (E_SC u each, absolute on a unit phasor), numpy's 2 pi frac, its sin and cos (4 u);
    with gouy the device rotates by (qi - i qr) / |q| where numpy subtracts arctan2 (4 u more).
  * the amplitude a sqrt(2 / (pi w^2)) (5 roundings and half of w^2's: 10 u a side) and the products env cs, A gy, gy gz (8 u a
    side): 36 u, 40 u with spare.
  * a bin centre the device leaves out lies more than 6 w from the hit's along an axis: below exp(-36) of the hit's peak
    a sqrt(2 / pi) / w, which is added for every hit to every bin.
  * two summation orders of the same c deposits: 2 c u sum |u| (the image test's bound), c = the hits with a non-zero u there.
E_EXP = 2 and E_SC = 2: the device math library's double exp differs from np.longdouble's by at most 0.85 ulp of exp on 1e5
arguments in [-37, 0], and its sincospi(2 f) by at most 0.87 x 2^-53 absolute on 1e5 f in [0, 1) (a measurement of the LIBRARY
functions on the MI355X by tools/bench_wave.py --probe, in a kernel of its own, not of k_mon_wave: profiles/wave_image_probe.json;
doubled for the arguments not sampled).
Every comparison prints the largest error beside its bound, and asserts that no bin's bound exceeds 3e-8 of the monitor's summed
peak amplitudes sum a sqrt(2 / pi) / w: a loose bound cannot hide a misplaced deposit.  With K = 24 and X <= 5e5 (cfg 2's paths at
780 nm over 5 segments) the phase term is 2 pi K u X < 8.4e-9 of a hit's peak.

`aliased`: per hit and axis the footprint is the bin centres within 6 w of the hit's; the cycle rate n ty / wavelength +
n qr D / (wavelength |q|^2) at its two end centres, times the mean bin width, above 0.5 on either axis makes the hit aliased (a hit
without a footprint is not).  The reference counts them, and asserts that every hit is at least 1e-6 away from the threshold and
that moving the 6 w limit by 1e-9 either way changes no hit's verdict."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from optable_amd import abi
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine, segment_source, wave_plan
from optable_amd.table import monitor_struct
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

U = 2.0**-53
K, E_EXP, E_SC = 24, 2, 2
CAP = 3e-8
EMPTY, DROPS, SPREAD = 2, 6, 7


class _Ref:
    """counts, field, bound per bin, the summed peak amplitudes and the aliased hits of one monitor, from its hit list."""

    def __init__(self, counts, field, bound, peaks, aliased):
        self.counts, self.field, self.bound, self.peaks, self.aliased = counts, field, bound, peaks, aliased

    def __add__(self, other):
        return _Ref(self.counts + other.counts, self.field + other.field, self.bound + other.bound, self.peaks + other.peaks, self.aliased + other.aliased)


def _aliased(v0, w, rate, curve, edges, reach):
    """Per hit: (has a footprint, the largest cycle rate over it times the mean bin width) along one axis, the footprint being the
    centres within `reach` w of v0.  rate + curve D is the cycle rate at the distance D."""
    c = 0.5 * (edges[1:] + edges[:-1])
    inside = np.abs(c[None, :] - v0[:, None]) <= (reach * w)[:, None]
    some = inside.any(axis=1)
    first, last = inside.argmax(axis=1), inside.shape[1] - 1 - inside[:, ::-1].argmax(axis=1)
    turn = np.maximum(np.abs(rate + curve * (c[first] - v0)), np.abs(rate + curve * (c[last] - v0))) * ((edges[-1] - edges[0]) / (len(edges) - 1))
    return some, np.where(some, turn, 0.0)


def _reference(h, wavelength, y_edges, z_edges, amplitude="sqrt", gouy=False, quiet=False):
    nby, nbz = len(y_edges) - 1, len(z_edges) - 1
    if len(h) == 0:
        return _Ref(np.zeros((nby, nbz), dtype=np.int64), np.zeros((nby, nbz), dtype=complex), np.zeros((nby, nbz)), 0.0, 0)
    y, z, I, t, P = support.host(h.yList(None)), support.host(h.zList(None)), support.host(h.IList(None)), support.host(h.t), support.host(h.P)
    ty, tz, direction = support.host(h.tYList(None)), support.host(h.tZList(None)), support.host(h.directionList(None))
    lam = support.hit_wavelengths(wavelength, h)
    qr = support.host(h._gather(h.segs.q_re, h.slot)) + t
    qi, n = support.host(h._gather(h.segs.q_im, h.slot)), support.host(h._gather(h.segs.n_index, h.slot))
    L = support.host(h._gather(h.segs.pathlength, h.slot)) + t * n
    q2 = qr * qr + qi * qi
    w2 = lam * q2 / (n * np.pi * qi)
    w = np.sqrt(w2)
    assert np.all(np.isfinite(w) & (w > 0))
    a = np.sqrt(I) if amplitude == "sqrt" else I
    g = np.arctan2(qr, qi) if gouy else np.zeros_like(qr)
    peak = a * np.sqrt(2 / np.pi) / w
    clear = min(np.abs(y[:, None] - y_edges[None, :]).min(), np.abs(z[:, None] - z_edges[None, :]).min())
    assert clear > 1e-9
    # the sampling verdicts, at 6 w and 1e-9 either side of it
    verdicts = []
    for reach in (6.0, 6.0 - 1e-9, 6.0 + 1e-9):
        some_y, turn_y = _aliased(y, w, n * ty / lam, n * qr / (lam * q2), y_edges, reach)
        some_z, turn_z = _aliased(z, w, n * tz / lam, n * qr / (lam * q2), z_edges, reach)
        turn = np.where(some_y & some_z, np.maximum(turn_y, turn_z), 0.0)
        verdicts.append(turn > 0.5)
        if reach == 6.0:
            margin = np.abs(turn - 0.5).min()
            footprints = int((some_y & some_z).sum())
    assert margin > 1e-6, margin
    assert np.array_equal(verdicts[0], verdicts[1]) and np.array_equal(verdicts[0], verdicts[2])
    aliased = int(verdicts[0].sum())
    yc, zc = 0.5 * (y_edges[1:] + y_edges[:-1]), 0.5 * (z_edges[1:] + z_edges[:-1])
    aY, aZ = np.abs(np.asarray(h.monitor.tangent_Y, dtype=float)), np.abs(np.asarray(h.monitor.tangent_Z, dtype=float))
    Sy, Sz, Sty, Stz = np.abs(P) @ aY, np.abs(P) @ aZ, np.abs(direction) @ aY, np.abs(direction) @ aZ
    dt = 4 * U * np.abs(t)
    field, bound, c, sum_mag = np.zeros((nby, nbz), dtype=complex), np.zeros((nby, nbz)), np.zeros((nby, nbz)), np.zeros((nby, nbz))
    x_max = 0.0
    for lo in range(0, len(y), 1024):  # (a thousand hits at a time: [hits, nby, nbz] temporaries)
        s = slice(lo, lo + 1024)

        def col(v):
            return v[s, None, None]

        Dy, Dz = (yc[None, :] - y[s, None])[:, :, None], (zc[None, :] - z[s, None])[:, None, :]
        r2 = Dy * Dy + Dz * Dz
        cycles = col(L) / col(lam) + col(n) * (col(ty) * Dy + col(tz) * Dz) / col(lam) + col(n) * col(qr) * r2 / (2 * col(lam) * col(q2))
        mag = col(a) * np.sqrt(2 / (np.pi * col(w2))) * np.exp(-r2 / col(w2))
        phase = 2 * np.pi * (cycles - np.floor(cycles)) - col(g)
        u = mag * np.cos(phase) + 1j * (mag * np.sin(phase))
        nl, curve = col(n) / col(lam), col(n) * np.abs(col(qr)) / (col(lam) * col(q2))
        X = np.abs(col(L)) / col(lam) + nl * (col(Sty) * np.abs(Dy) + col(Stz) * np.abs(Dz)) + curve * r2 / 2
        x_max = max(x_max, float(X.max()))
        dDy, dDz = 8 * U * col(Sy) + col(Sty) * col(dt), 8 * U * col(Sz) + col(Stz) * col(dt)
        cyc_err = (K * U * X + (nl * np.abs(col(ty)) + curve * np.abs(Dy)) * dDy + (nl * np.abs(col(tz)) + curve * np.abs(Dz)) * dDz
                   + nl * col(dt) + col(n) * r2 * col(dt) / (2 * col(lam) * col(q2)))
        exponent = (r2 / col(w2)) * (24 * U + 2 * np.abs(col(qr)) * col(dt) / col(q2)) + 2 * (np.abs(Dy) * dDy + np.abs(Dz) * dDz) / col(w2)
        rel = 2 * np.pi * cyc_err + exponent + (2 * (2 * E_EXP + 1) + 2 * E_SC + 4 + 4 + 40) * U + np.abs(col(qr)) * col(dt) / col(q2)
        field += u.sum(axis=0)
        bound += (mag * rel).sum(axis=0) + np.exp(-36.0) * peak[s].sum()
        c += (mag > 0).sum(axis=0)
        sum_mag += mag.sum(axis=0)
    bound += 2 * c * U * sum_mag
    counts = np.histogram2d(y, z, bins=[y_edges, z_edges])[0].astype(np.int64)
    if not quiet:
        print(f"  {len(y)} hits ({footprints} with a footprint, {aliased} aliased, nearest to the threshold {margin:.3g}), w from {w.min():.3g} to "
              f"{w.max():.3g}, X up to {x_max:.3g} cycles, smallest distance of a centre to a bin edge {clear:.3g}")
    return _Ref(counts, field, bound, float(peak.sum()), aliased)


def _footprints(h, wavelength, y_edges, z_edges):
    """How many hits reach a bin centre (within 6 w on both axes)."""
    if len(h) == 0:
        return 0
    w = support.host(h.spotsizeList(wavelength, None))
    yc, zc = 0.5 * (y_edges[1:] + y_edges[:-1]), 0.5 * (z_edges[1:] + z_edges[:-1])
    near_y = (np.abs(yc[None, :] - support.host(h.yList(None))[:, None]) <= 6 * w[:, None]).any(axis=1)
    near_z = (np.abs(zc[None, :] - support.host(h.zList(None))[:, None]) <= 6 * w[:, None]).any(axis=1)
    return int((near_y & near_z).sum())


def _assert_against(counts, re, im, ref, what=""):
    np.testing.assert_array_equal(counts, ref.counts)
    assert np.all(ref.bound <= CAP * ref.peaks), (float(ref.bound.max()), ref.peaks)  # the cap: asserted from the reference alone
    err = np.maximum(np.abs(re - ref.field.real), np.abs(im - ref.field.imag))
    at = np.unravel_index(np.argmax(err - ref.bound), err.shape)
    print(f"  {what}{int(ref.counts.sum())} centres in range, summed peaks {ref.peaks:.6g}; largest error {err.max():.3g}, nearest to its bound "
          f"{err[at]:.3g} of {ref.bound[at]:.3g}; largest bound {ref.bound.max():.3g} = {ref.bound.max() / max(ref.peaks, 1e-300):.3g} of the peaks")
    assert np.all(err <= ref.bound), (float(err[at]), float(ref.bound[at]))
    return ref.counts


def _assert_wave(f, h, wavelength, what="", amplitude="sqrt", gouy=False):
    counts, re, im, y_edges, z_edges = f.to_host()
    assert f.monitor is h.monitor and counts.dtype == np.int64 and re.dtype == im.dtype == np.float64
    assert counts.shape == re.shape == im.shape == (len(y_edges) - 1, len(z_edges) - 1) == f.bins
    ref = _reference(h, wavelength, y_edges, z_edges, amplitude, gouy)
    _assert_against(counts, re, im, ref, what)
    return ref


def _wave_all(table, *args, **kwargs):
    """wave_all with its RuntimeWarning checked against what it returns: one warning iff the call counted aliased hits."""
    before = kwargs["into"][0].aliased if kwargs.get("into") else 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = table.wave_all(*args, **kwargs)
    told = [w for w in caught if issubclass(w.category, RuntimeWarning) and "aliased" in str(w.message)]
    added = (out[0].aliased - before) if out else 0
    assert len(told) == (1 if added > 0 else 0), (len(told), added)
    if told:
        assert f"{added} hits" in str(told[0].message) and "smaller monitor or more bins" in str(told[0].message)
    return out


# -- 1, 2, 3: segments by hand ------------------------------------------------------------------------------------------------
WL_HAND = 0.5


def _hand_segments(y, z, w, valid, qr=None, n_index=None, intensity=None, ty=None, tz=None, pathlength=None):
    """len(y) slots of a [1][ray] slots layout: rays through (5, y, z) along (1, ty, tz) / norm from the plane x = 0, of length 10,
    onto a monitor at x = 5 (t = 5 norm), with q such that the spot size there is close to `w` at the wavelength WL_HAND:
    q_re = qr - t (qr = 0 where the spot is too small to be `qr` from its waist), and qi the larger root of
    w^2 = WL (qr^2 + qi^2) / (n pi qi).  Slot k is valid iff valid[k] (seg_count)."""
    N = len(y)
    qr = np.zeros(N) if qr is None else np.asarray(qr, dtype=float)
    n_index = np.ones(N) if n_index is None else np.asarray(n_index, dtype=float)
    ty, tz = (np.zeros(N) if v is None else np.asarray(v, dtype=float) for v in (ty, tz))
    half = n_index * np.pi * np.asarray(w, dtype=float) ** 2 / WL_HAND / 2
    qr = np.where(half > 2 * np.abs(qr), qr, 0.0)  # (a spot this small has its waist at the monitor)
    qi = half + np.sqrt(half**2 - qr**2)
    norm = np.sqrt(1 + ty**2 + tz**2)
    segs = SegmentBatch(N, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()

    def put(field, values):
        segs.field(field).copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)))

    put("oy", np.asarray(y) - 5 * ty), put("oz", np.asarray(z) - 5 * tz), put("q_re", qr - 5.0 * norm), put("q_im", qi), put("n", n_index)
    put("dx", 1 / norm), put("dy", ty / norm), put("dz", tz / norm)
    put("intensity", np.ones(N) if intensity is None else intensity)
    put("pathlength", np.zeros(N) if pathlength is None else pathlength)
    segs.length.fill_(10.0)
    segs.ray.copy_(torch.arange(N, dtype=torch.int32))
    segs.count = torch.from_numpy(np.asarray(valid, dtype=np.int32)).cuda()
    segs.n_rays = N
    assert segs.layout == "slots"
    return segs


@pytest.fixture(scope="module")
def hand():
    """130 slots, two full waves and two lanes: wave 0 has 64 hits, wave 1 hits in its lanes 0 (slot 64), 6, 36 and 63, wave 2 none
    (slot 128 misses the monitor, slot 129 would hit and is invalid by seg_count).  w from 0.01 to 20 on a 6 x 6 monitor of 7 x 5
    bins: footprints from no centre at all over one bin to all 35, clipped at every border and corner; directions
    (1, ty, tz) / norm with |ty|, |tz| <= 0.2, qr of both signs and zero, n of 1 and 1.5, path lengths in [0, 40].
    (segments, monitor, record_all's hits), made once."""
    rng = np.random.default_rng(11)
    N = 130
    y, z = rng.uniform(-2.9, 2.9, N), rng.uniform(-2.9, 2.9, N)
    w = np.exp(rng.uniform(np.log(0.01), np.log(20.0), N))
    # narrow spots at the four borders and two corners, a wide one in the middle, the widest in lane 63, the narrowest in lane 0
    y[:8], z[:8] = [2.97, -2.97, 0.1, 0.2, 2.96, -2.95, 0.05, 1.0], [0.3, -0.4, 2.98, -2.96, 2.97, -2.98, -0.07, 1.0]
    w[:8] = [0.3, 0.3, 0.3, 0.3, 0.2, 0.2, 3.0, 0.01]
    w[63], w[64] = 20.0, 0.013
    miss = np.ones(N, dtype=bool)
    miss[:64] = False
    miss[[64, 70, 100, 127, 129]] = False
    y[miss] = 100.0
    valid = np.ones(N, dtype=np.int32)
    valid[129] = 0
    qr = np.where(np.arange(N) % 3 == 0, 0.0, rng.uniform(-0.3, 0.3, N))
    ty, tz = rng.uniform(-0.2, 0.2, N), rng.uniform(-0.2, 0.2, N)
    ty[5], tz[5], ty[6], tz[6] = 0.2, -0.2, 0.0, 0.0
    segs = _hand_segments(y, z, w, valid, qr=qr, n_index=np.where(np.arange(N) % 2, 1.5, 1.0), intensity=0.25 + 0.75 * rng.random(N), ty=ty, tz=tz,
                          pathlength=rng.uniform(0.0, 40.0, N))
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 6, 6)
    h = table.record_all(segs, monitors=[mon])[0]
    assert sorted(h.slot.tolist()) == list(range(64)) + [64, 70, 100, 127]
    spot = support.host(h.spotsizeList(WL_HAND, None))
    assert spot.min() < 0.012 and spot.max() > 19 and (support.host(h.qList(None).real) > 0).any() and (support.host(h.qList(None).real) < 0).any()
    assert np.abs(support.host(h.tYList(None))).max() <= 0.2 and np.abs(support.host(h.tYList(None))).max() > 0.15
    return table, mon, segs, h


@pytest.mark.parametrize("gouy", [False, True])
@pytest.mark.parametrize("amplitude", ["sqrt", "linear"])
def test_hand_built_footprints_from_one_bin_to_the_whole_image(hand, amplitude, gouy):
    table, mon, segs, h = hand
    f = _wave_all(table, segs, WL_HAND, bins=(7, 5), monitors=[mon], amplitude=amplitude, gouy=gouy)[0]
    ref = _assert_wave(f, h, WL_HAND, amplitude=amplitude, gouy=gouy)
    assert ref.counts.sum() == 68 and torch.equal(f.counts, table.image_batch(mon, segs, bins=(7, 5)).counts)
    assert f.aliased == ref.aliased and 0 < ref.aliased < 68
    assert int((f.field.abs() > 0).sum()) == 35
    np.testing.assert_array_equal(f.irradiance().cpu().numpy(), (f.re**2 + f.im**2).cpu().numpy())
    np.testing.assert_allclose(f.power().cpu().numpy(), f.irradiance().cpu().numpy() * (6 / 7) * (6 / 5), rtol=1e-14)
    # the hit-list form of the same quantities
    q = h.qList(None)
    with np.errstate(divide="ignore"):  # (inf at a waist, on both sides)
        np.testing.assert_allclose(support.host(h.radiusList(None)), support.host(q.real**2 + q.imag**2) / support.host(q.real), rtol=1e-15)
    np.testing.assert_allclose(support.host(h.gouyList(None)), np.arctan2(support.host(q.real), support.host(q.imag)), rtol=1e-15)
    a = support.host(h.IList(None)) if amplitude == "linear" else np.sqrt(support.host(h.IList(None)))
    np.testing.assert_allclose(support.host(h.amplitudeList(WL_HAND, None, amplitude)), a * np.sqrt(2 / np.pi) / support.host(h.spotsizeList(WL_HAND, None)), rtol=1e-14)
    if gouy:  # the Gouy phase is not nothing here
        plain = _wave_all(table, segs, WL_HAND, bins=(7, 5), monitors=[mon], amplitude=amplitude)[0]
        assert float((plain.field - f.field).abs().max()) > 1e-3 * float(f.field.abs().max())


def test_more_centres_than_lanes():
    """bins = (130, 2): 130 y centres, more than a chunk of 63 — a beam that covers all of them, one that crosses the chunk boundary
    at bin 63 only, one inside a chunk, one between two centres (no footprint).  The same beams at bins = (1, 1)."""
    y = np.array([0.013, -2.5, -0.11, 1.3, 0.4])
    z = np.array([0.021, 1.1, 0.27, -0.7, 2.9])
    w = np.array([20.0, 3.0, 0.05, 0.05, 0.001])
    I = np.array([1.0, 0.5, 2.0, 0.75, 1.5])
    segs = _hand_segments(y, z, w, np.ones(5, dtype=np.int32), intensity=I, ty=[0.01, -0.02, 0.15, -0.2, 0.1], tz=[0.0, 0.03, -0.1, 0.05, 0.2],
                          qr=[0.2, -0.2, 0.0, 0.001, 0.0], pathlength=[0.0, 1.25, 7.0, 33.3, 2.0])
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 6, 6)
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) == 5
    f = _wave_all(table, segs, WL_HAND, bins=(130, 2), monitors=[mon])[0]
    ref = _assert_wave(f, h, WL_HAND)
    assert f.aliased == ref.aliased and int(f.counts.sum()) == 5
    yc = 0.5 * (f.y_edges[1:] + f.y_edges[:-1])
    reach = [np.flatnonzero(np.abs(yc - v) <= 6 * s) for v, s in zip(y, w)]
    assert len(reach[0]) == 130 and reach[2][0] < 63 <= reach[2][-1] and reach[3][0] > 63 and len(reach[3]) > 1 and len(reach[4]) == 0
    one = _wave_all(table, segs, WL_HAND, bins=(1, 1), monitors=[mon])[0]
    _assert_wave(one, h, WL_HAND)
    assert int(one.counts[0, 0]) == 5


def test_closed_form_the_power_of_one_beam():
    """One beam more than 8 w inside the rim of a monitor of 322 x 322 bins of w / 20 (the global path): the midpoint rule over
    |u|^2 gives back the hit's intensity — to 1e-16 of it with exact values — within the bound of the field summed over the bins,
    2 |u| b + b^2 times the bin area, and one rounding per bin summed."""
    w, I = 0.3, 0.8125
    segs = _hand_segments([0.0037], [-0.0052], [w], [1], qr=[0.11], intensity=[I], ty=[0.001], tz=[-0.002], pathlength=[3.3])
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 322 * w / 20, 322 * w / 20)
    assert wave_plan(1, 322, 322)["path"] == "global"
    h = table.record_all(segs, monitors=[mon])[0]
    spot = float(h.spotsizeList(WL_HAND, None)[0])
    assert abs(spot / w - 1) < 1e-3 and 161 * w / 20 - 0.0052 > 8 * spot
    f = _wave_all(table, segs, WL_HAND, bins=322, monitors=[mon])[0]
    ref = _assert_wave(f, h, WL_HAND)
    assert f.aliased == ref.aliased == 0
    area = (w / 20) ** 2
    allowed = float(((2 * np.abs(ref.field) * ref.bound + ref.bound**2) * area).sum()) + 322 * 322 * U * I + 2e-16 * I
    total = float(f.power().sum())
    print(f"  power {total:.17g} of {I:.17g}: off by {abs(total - I):.3g}, allowed {allowed:.3g}")
    assert abs(total - I) <= allowed < 1e-9 * I


def test_closed_form_two_beam_fringes():
    """Two equal hits at the same point, tilted by +-theta in y, equal paths, not aliased: irradiance = 4 I0 cos^2(2 pi theta y /
    lambda) with I0 = a^2 2 / (pi w^2) exp(-2 r^2 / w^2), bright at the centre; with one path longer by lambda / 2 the cosine is a
    sine and the centre is dark.  Within the summed bound of the field, 2 |U| b + b^2, and 1e-13 of the peak for the closed form
    itself (its y0 = 0 holds to a few u of 5 theta)."""
    theta, qr, qi, I = 0.2, 0.7, 9.0, 0.64
    dx = np.sqrt(1 - theta**2)
    w2 = WL_HAND * (qr**2 + qi**2) / (np.pi * qi)
    mon = oa.Monitor([5, 0, 0], 6, 6)
    table = oa.OpticalTable()
    for extra, bright in ((0.0, True), (WL_HAND / 2, False)):
        segs = SegmentBatch(2, "f64", "cuda")
        for f in abi.SEG_FIELDS:
            segs.field(f).zero_()
        t = 5.0
        for name, values in (("ox", [5 - t * dx] * 2), ("oy", [-t * theta, t * theta]), ("dx", [dx, dx]), ("dy", [theta, -theta]), ("length", [10.0, 10.0]),
                             ("intensity", [I, I]), ("q_re", [qr - t] * 2), ("q_im", [qi] * 2), ("n", [1.0, 1.0]), ("pathlength", [1.5, 1.5 + extra])):
            segs.field(name).copy_(torch.tensor(values, dtype=torch.float64))
        segs.ray.copy_(torch.arange(2, dtype=torch.int32))
        segs.count, segs.n_rays = torch.ones(2, dtype=torch.int32, device="cuda"), 2
        h = table.record_all(segs, monitors=[mon])[0]
        assert len(h) == 2 and float(h.yList(None).abs().max()) < 1e-14 and float((h.t - t).abs().max()) < 1e-14
        f = _wave_all(table, segs, WL_HAND, bins=(61, 3), monitors=[mon])[0]
        ref = _assert_wave(f, h, WL_HAND)
        assert f.aliased == ref.aliased == 0
        yc, zc = 0.5 * (f.y_edges[1:] + f.y_edges[:-1]), 0.5 * (f.z_edges[1:] + f.z_edges[:-1])
        I0 = I * 2 / (np.pi * w2) * np.exp(-2 * (yc[:, None] ** 2 + zc[None, :] ** 2) / w2)
        arg = 2 * np.pi * theta * yc[:, None] / WL_HAND
        want = 4 * I0 * (np.cos(arg) ** 2 if bright else np.sin(arg) ** 2)
        allowed = 2 * np.abs(ref.field) * ref.bound + ref.bound**2 + 1e-13 * 4 * I0.max()
        got = f.irradiance().cpu().numpy()
        print(f"  {'bright' if bright else 'dark'}: largest error {np.abs(got - want).max():.3g}, allowed there {allowed.flat[np.argmax(np.abs(got - want))]:.3g}; "
              f"centre {got[30, 1]:.6g} of 4 I0 = {4 * I0[30, 1]:.6g}")
        assert np.all(np.abs(got - want) <= allowed)
        assert abs(yc[30]) < 1e-14 and (got[30, 1] > 0.999 * 4 * I0[30, 1] if bright else got[30, 1] < 1e-12 * 4 * I0[30, 1])
        assert int((np.diff(np.sign(np.cos(arg[:, 0]))) != 0).sum()) >= 4  # several fringes across the image


# -- 4: cfg 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case4():
    """cfg 2, 5,003 rays, 5 segments, eight monitors: (table, monitors, {layout: (batch, segs, record_all hits)}), traced and
    recorded on first use."""
    table, mons, made = support.cfg2_table(), support.eight_monitors(), {}
    o, d = scenes.cfg2_rays(5003, 0)

    def get(layout):
        if layout not in made:
            batch = support.waisted_batch(o, d)
            segs = table.trace_batch(batch, max_segments=5, layout=layout)
            assert segs.layout == layout and segs.precision == "f64"
            made[layout] = (batch, segs, table.record_all(segs, monitors=mons))
        return made[layout]

    return table, mons, get


@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts(case4, layout, monkeypatch):
    table, mons, get = case4
    batch, segs, hits = get(layout)
    assert wave_plan(len(mons), 30, 30) == {"path": "lds", "per_pass": 3, "passes": 3}
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("wave_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        with pytest.warns(RuntimeWarning, match="aliased"):
            waves = table.wave_all(segs, scenes.WL)  # the table's own monitors, in their order, bins=30
        images = table.image_all(segs)
    assert len(waves) == len(mons) and all(f.monitor is m for f, m in zip(waves, mons))
    assert all(f.counts.is_cuda and f.counts.dtype == torch.int64 and f.re.dtype == f.im.dtype == torch.float64 for f in waves)
    refs = [_assert_wave(f, h, scenes.WL, what=f"monitor {k}: ") for k, (f, h) in enumerate(zip(waves, hits))]
    for f, im in zip(waves, images):
        assert torch.equal(f.counts, im.counts)
    aliased = sum(r.aliased for r in refs)
    footprints = sum(_footprints(h, scenes.WL, f.y_edges, f.z_edges) for f, h in zip(waves, hits))
    assert all(f.aliased == aliased for f in waves) and aliased > 0.9 * footprints > 0  # nearly every hit that reaches a bin centre, at 780 nm
    assert len(hits[EMPTY]) == 0 and refs[EMPTY].counts.sum() == 0 and not waves[EMPTY].field.abs().any()
    assert 0 < refs[DROPS].counts.sum() < len(hits[DROPS])  # centres off the image are counted nowhere
    if layout == "slots":
        with pytest.warns(RuntimeWarning, match="aliased"):
            per_ray = table.wave_all(segs, batch, monitors=[mons[3], mons[0]])  # the traced batch's wavelengths; the monitors given
        assert _assert_wave(per_ray[0], hits[3], batch).aliased + _assert_wave(per_ray[1], hits[0], batch).aliased == per_ray[0].aliased
        again = _wave_all(table, segs, scenes.WL)
        assert all(torch.equal(a.counts, b.counts) for a, b in zip(again, waves)) and again[0].aliased == aliased


# -- 5: the global path, accumulation -------------------------------------------------------------------------------------------
def test_global_path_and_accumulation():
    """(80, 80): 6,400 bins, more than the LDS budget — every deposit two global atomics.  And `into=` over the two chunks of a
    batch against the whole batch in one call and against the summed references, on either path; `aliased` accumulates."""
    table = support.cfg2_table()
    mon = oa.Monitor([7.5, 0, 0], 2, 2)
    assert wave_plan(1, 80, 80)["path"] == "global" and wave_plan(1, 30, 30)["path"] == "lds"
    whole = support.waisted_batch(*scenes.cfg2_rays(2049, 3))
    segs = table.trace_batch(whole, max_segments=5, layout="slots")
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) >= 2049
    chunks = [whole.slice(0, 1024), whole.slice(1024, 2049)]
    parts = [table.trace_batch(b, max_segments=5, layout="slots") for b in chunks]
    part_hits = [table.record_all(p, monitors=[mon])[0] for p in parts]
    for bins in ((80, 80), (30, 30)):
        waves = _wave_all(table, parts[0], chunks[0], bins=bins, monitors=[mon])
        first, first_aliased = waves[0].counts.clone(), waves[0].aliased
        assert _wave_all(table, parts[1], chunks[1], bins=bins, monitors=[mon], into=waves) == waves
        refs = [_reference(ph, b, waves[0].y_edges, waves[0].z_edges) for ph, b in zip(part_hits, chunks)]
        summed = refs[0] + refs[1]
        counts, re, im, _, _ = waves[0].to_host()
        _assert_against(counts, re, im, summed, what=f"{bins} in two chunks: ")
        assert int(first.sum()) < int(counts.sum())
        assert first_aliased == refs[0].aliased and waves[0].aliased == summed.aliased > first_aliased
        once = _wave_all(table, segs, whole, bins=bins, monitors=[mon])[0]
        assert torch.equal(once.counts, waves[0].counts) and once.aliased == summed.aliased
        _assert_wave(once, h, whole, what=f"{bins} at once: ")
        # without `into=` a call starts from zero again
        assert torch.equal(_wave_all(table, parts[0], chunks[0], bins=bins, monitors=[mon])[0].counts, first)


# -- 6: ray trees -------------------------------------------------------------------------------------------------------------
def _michelson(o, wavelength, arm_difference, wl_unit, w0=0.01):
    """The Michelson of tests/test_gpu_field.py with Gaussian rays: a 50 % splitter at 45 degrees at the origin, a mirror at the end
    of either arm (x = L1, y = -L2 with 2 (L1 - L2) = arm_difference * wl_unit), rays along -y from y = 2.  (table, batch, segs)."""
    L1 = 3.0
    L2 = L1 - arm_difference * wl_unit / 2
    batch = RayBatch.from_arrays(o, np.tile([0.0, -1.0, 0.0], (len(o), 1)), wavelength=wavelength, q=1j * np.pi * w0**2 / 780e-7, device="cuda")
    table = oa.OpticalTable()
    table.add_components([oa.BeamSplitter([0, 0, 0], width=2, height=2, eta=0.5).RotZ(np.pi / 4),
                          oa.SquareMirror([L1, 0, 0], width=2, height=2).RotZ(np.pi),
                          oa.SquareMirror([0, -L2, 0], width=2, height=2).RotZ(np.pi / 2)])
    return table, batch, table.trace_batch(batch, max_segments=8)  # a tree is 1 + 2 + 4 rays


def test_ray_trees_inherit_the_wavelength():
    """257 trees of two colours: both children of a tree reach the monitor, and the wavelength of either comes through its
    segment's `ray`, the index of the tree's input ray."""
    i, j = np.divmod(np.arange(257), 17)
    o = np.stack([(i - 8) / 32 + 1 / 64, np.full(257, 2.0), (j - 8) / 32 + 1 / 64], axis=1)
    wl = np.where(np.arange(257) % 2, 780e-7, 400e-7)
    table, batch, segs = _michelson(o, wl, 0.5 / 780e-7, 780e-7)  # L2 = 2.75
    mon = oa.Monitor([-2, 0, 0], 0.6, 0.6)
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) == 2 * 257 and torch.equal(h.ray_index(None), torch.arange(257, device="cuda").repeat_interleave(2))
    f = _wave_all(table, segs, batch, bins=(9, 4), monitors=[mon])[0]
    ref = _assert_wave(f, h, batch)
    assert ref.counts.sum() == 2 * 257 and f.aliased == ref.aliased
    g = _wave_all(table, segs, 780e-7, bins=(9, 4), monitors=[mon])[0]  # one wavelength for all is another image
    _assert_wave(g, h, 780e-7)
    assert torch.equal(g.counts, f.counts) and float((g.field - f.field).abs().max()) > 1e-3 * float(f.field.abs().max())


def test_one_tree_is_an_interferometer():
    """ONE on-axis Gaussian ray through the Michelson onto a monitor 0.05 wide: 2 (L1 - L2) = 1000 wavelengths is the bright port,
    a mirror moved by a quarter of a wavelength (1000.5) the dark one.  The reference's own totals differ by more than a factor of
    10 — asserted first — and the device's totals agree with them within the summed bound."""
    wl = 2.0**-14  # (610 nm in the table's centimetres; L1 - L2 is an exact binary multiple of it)
    mon = oa.Monitor([-2, 0, 0], 0.05, 0.05)
    totals, wanted = [], []
    for arm in (1000.0, 1000.5):
        table, batch, segs = _michelson(np.array([[1 / 1024, 2.0, -1 / 2048]]), wl, arm, wl)
        h = table.record_all(segs, monitors=[mon])[0]
        assert len(h) == 2
        f = _wave_all(table, segs, batch, bins=30, monitors=[mon])[0]
        ref = _assert_wave(f, h, batch)
        assert f.aliased == ref.aliased == 0
        area = (0.05 / 30) ** 2
        allowed = float(((2 * np.abs(ref.field) * ref.bound + ref.bound**2) * area).sum()) + 900 * U * float((np.abs(ref.field) ** 2).sum() * area)
        wanted.append((float((np.abs(ref.field) ** 2).sum() * area), allowed))
        totals.append(float(f.power().sum()))
    print(f"  bright {totals[0]:.6g} (reference {wanted[0][0]:.6g}), dark {totals[1]:.6g} (reference {wanted[1][0]:.6g})")
    assert wanted[0][0] > 10 * wanted[1][0]
    for got, (want, allowed) in zip(totals, wanted):
        assert abs(got - want) <= allowed
    assert totals[0] > 10 * totals[1]


# -- 7, 8: hits left out, refusals --------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / re / im of M monitors of nby x nbz bins, `skipped` and `aliased` for ot_monitor_wave_many, filled with a sentinel."""

    def __init__(self, M, nby, nbz):
        image, one = (torch.float64, (M, nby, nbz)), (torch.int64, (1,))
        super().__init__(counts=(torch.int64, (M, nby, nbz)), re=image, im=image, skipped=one, aliased=one)


def _call(lib, ctx, mons, segs, nby, nbz, out, wavelength=None, n_wavelengths=0, uniform=0.0, mode=0, gouy=0, accumulate=0, source=None, **planes):
    src, n, count, n_rays = segment_source(segs)
    table = (abi.OtMonitor * len(mons))(*[monitor_struct(m) for m in mons])
    axes, edges = support.image_tables(mons, nby, nbz)
    dp = C.POINTER(C.c_double)
    plane = {f: planes.get(f, segs.field(f).data_ptr()) for f in ("intensity", "n", "pathlength", "q_re", "q_im")}
    return lib.ot_monitor_wave_many(ctx, table, len(mons), axes.ctypes.data_as(dp), edges.ctypes.data_as(dp), nby, nbz,
                                    C.byref(src if source is None else source), plane["intensity"], plane["n"], plane["pathlength"], plane["q_re"],
                                    plane["q_im"], None if wavelength is None else wavelength.data_ptr(), n_wavelengths, uniform, mode, gouy, n,
                                    None if count is None else count.data_ptr(), n_rays, planes.get("counts", out.counts.data_ptr()),
                                    planes.get("re", out.re.data_ptr()), planes.get("im", out.im.data_ptr()),
                                    planes.get("skipped", out.skipped.data_ptr()), planes.get("aliased", out.aliased.data_ptr()), accumulate)


def test_a_batch_without_q_is_refused(case4):
    table, mons, get = case4
    o, d = scenes.cfg2_rays(300, 5)
    plain = RayBatch.from_arrays(o, d, wavelength=scenes.WL, device="cuda")  # no q
    segs = table.trace_batch(plain, max_segments=5, layout="slots")
    pick = [mons[0], mons[SPREAD]]
    hits = table.record_all(segs, monitors=pick)
    n_hits = sum(len(h) for h in hits)
    assert n_hits >= 600
    with pytest.raises(ValueError, match=f"{n_hits} hits"):
        table.wave_all(segs, scenes.WL, monitors=pick)
    eng = get_engine()
    out = _Out(2, 30, 30)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, pick, segs, 30, 30, out, uniform=scenes.WL) == 0, eng.lib.ot_last_error()
    torch.cuda.synchronize()
    assert int(out.skipped.item()) == n_hits and int(out.aliased.item()) == 0
    assert not out.counts.any() and not out.re.any() and not out.im.any()
    # ... and the guard on the wavelength gather: the library is told of 100 wavelengths (the buffer holds all 5,003 of another
    # batch, so a missing guard reads valid memory and fails the assertion: nothing can fault)
    batch, segs, hits = get("slots")
    wl = batch.wavelength.double().contiguous()
    with eng.lock:
        assert _call(eng.lib, eng._ctx, [mons[0]], segs, 30, 30, _Out(1, 30, 30), wavelength=wl, n_wavelengths=5003) == 0
        out = _Out(1, 30, 30)
        assert _call(eng.lib, eng._ctx, [mons[0]], segs, 30, 30, out, wavelength=wl, n_wavelengths=100) == 0
    torch.cuda.synchronize()
    known = int((hits[0].ray_index(None) < 100).sum())
    assert 0 < known < len(hits[0]) and int(out.skipped.item()) == len(hits[0]) - known and int(out.counts.sum()) == known


def test_abi_errors(ctx):
    lib, c = ctx
    y = np.linspace(-2.5, 2.5, 130) + 0.0123
    segs = _hand_segments(y, np.full(130, 0.3), np.full(130, 0.5), np.ones(130, dtype=np.int32))
    mon = oa.Monitor([5, 0, 0], 6, 6)
    out = _Out(1, 7, 5)
    wl = torch.full((130,), WL_HAND, dtype=torch.float64, device="cuda")

    def call(**kw):
        kw.setdefault("uniform", WL_HAND)
        return _call(lib, c, [mon], segs, 7, 5, out, **kw)

    expect, altered = functools.partial(support.expect_invalid, lib), functools.partial(support.altered, segment_source(segs)[0])

    expect(call(source=altered(width=2)), "width")
    expect(call(source=altered(width=4)), "double-precision")  # single precision is refused, as for fields
    for plane in ("intensity", "n", "pathlength", "q_re", "q_im", "counts", "re", "im", "skipped", "aliased"):
        expect(call(**{plane: None}), "NULL")
    no_field = altered()
    no_field.base[6] = None
    expect(call(source=no_field), "NULL field")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        expect(call(uniform=bad), "wavelength_uniform")
    expect(call(wavelength=wl, n_wavelengths=0), "n_wavelengths")
    expect(call(wavelength=wl, n_wavelengths=-1), "n_wavelengths")
    for bad in (-1, 2):
        expect(call(mode=bad), "amplitude_mode")
        expect(call(gouy=bad), "gouy")
    expect(call(accumulate=2), "accumulate")  # ... and what ot_monitor_image_many refuses
    expect(call(source=altered(capacity=64)), "capacity")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good; the array and the one value give the same image; accumulate doubles the field
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    assert int(out.counts.sum()) == 130 and int(out.skipped.item()) == 0 and int(out.aliased.item()) == 0
    re, im = out.re.clone(), out.im.clone()
    assert float((re**2 + im**2).sum()) > 10
    assert call(wavelength=wl, n_wavelengths=130, uniform=float("nan")) == 0 and lib.ot_ctx_synchronize(c) == 0
    assert torch.allclose(out.re, re, rtol=0, atol=1e-12) and torch.allclose(out.im, im, rtol=0, atol=1e-12)
    assert call(accumulate=1) == 0 and lib.ot_ctx_synchronize(c) == 0
    assert int(out.counts.sum()) == 260 and torch.allclose(out.re, 2 * re, rtol=0, atol=1e-12) and torch.allclose(out.im, 2 * im, rtol=0, atol=1e-12)
