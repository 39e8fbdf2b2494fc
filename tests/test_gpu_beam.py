"""GPU (MI355X): Gaussian-beam detector images — `OpticalTable.beam_all` / `beam_batch`, every monitor hit spread over its spot
size on the device by the beam mode of k_mon_count (ot_monitor_beam_many), with no hit list.

Reference, in every comparison: numpy and scipy.special.erf on the hit lists of the verified path, h in table.record_all(...):
    y0 = h.yList, z0 = h.zList, q = q[slot] + t, w^2 = wavelength (qr^2 + qi^2) / (n pi qi),
    Fy[j, k] = (erf(sqrt2 (ey[k + 1] - y0_j) / w_j) - erf(sqrt2 (ey[k] - y0_j) / w_j)) / 2,   Fz likewise,
    power[ky, kz] = sum_j I_j Fy[j, ky] Fz[j, kz]      — over ALL edges, with no cut at 5 w,
    counts = np.histogram2d(y0, z0, bins=[y_edges, z_edges]).
Every comparison first asserts from the REFERENCE values that no centre lies within 1e-9 of a bin edge.  Single-precision segments
are compared with the reference computed from the same single-precision records widened to double.

counts must be EQUAL, to the reference and to `image_all`'s.  power of a bin must agree within the bound derived here (not
measured), u = 2^-53:
  * the argument a = sqrt2 (e - y0) / w.  Both sides subtract, scale and divide once each (3 u |a| a side) and form w from
    qr = q_re + t, two squares, their sum, two products in the numerator and two in the denominator, a division and a correctly
    rounded square root: 9 roundings of w^2, 4.5 u + u on w a side — 17 u |a| for both, REL = 20 u with spare.  A last-bit difference
    in t between the record pass and the beam pass of the same test moves qr by u |t| and w by u |t| |qr| / (qr^2 + qi^2) relative:
    twice that is added.
  * the cancellation in e - y0.  The edges are the same doubles on both sides; y0 = P . a_y is three products and two sums
    evaluated in another order and contraction here than there: |d y0| <= 8 u S, S = |P| . |a_y| (gamma_3 a side, spare for t).
    It moves a by sqrt2 8 u S / w whatever e - y0 is: for narrow beams far from the axis this is the dominant term.
  * d erf / d a = 2 / sqrt(pi) exp(-a^2), so an edge's erf moves by 2 / sqrt(pi) exp(-a^2) (REL |a| + sqrt2 8 u S / w), plus the two
    libraries' own errors (E_REF + E_DEV) ulp of erf(a), an ulp being at most 2 u |erf(a)|.
  * F = (erf(a1) - erf(a0)) / 2 adds half of either edge's error and one rounding a side (2 u F); the deposit I Fy Fz two products
    a side (4 u I Fy Fz); a bin the device leaves out holds less than erfc(5 sqrt2) / 2 < 8e-24 of the hit along that axis (1.6e-23 I
    covers both axes).
  * two summation orders of the same c deposits: 2 c u sum (the image test's bound), c = the hits with a non-zero share in the bin.
E_REF = 2: Cephes' erf, which scipy wraps, documents a peak relative error of 3.7e-16 = 1.7 ulp.  E_DEV = 6: the device math
library's double erf differs from scipy's by at most 3 ulp of erf on 1e5 arguments in [-8, 8], 0.17 ulp on average (a measurement of
the LIBRARY function on the MI355X by tools/bench_beam.py --probe, in a kernel of its own, not of k_mon_count: profiles/
beam_image_erf_probe.json; doubled for the arguments not sampled).
Every comparison prints the largest error beside its bound, and asserts that no bin's bound exceeds 1e-10 of the monitor's total hit
intensity: a loose bound cannot hide a misplaced deposit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from scipy.special import erf

import optable_amd as oa
import scenes
import support
from optable_amd import abi
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import beam_plan, get_engine, segment_source
from optable_amd.monitors import MonitorHits, image_edges
from optable_amd.table import monitor_struct
from support import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

U = 2.0**-53
REL, E_REF, E_DEV = 20, 2, 6
EMPTY, DROPS, SPREAD = 2, 6, 7


def _reference(h, wavelength, y_edges, z_edges):
    """(counts, power, bound) per bin from the hit list `h`, after asserting that no centre is within 1e-9 of an edge."""
    nby, nbz = len(y_edges) - 1, len(z_edges) - 1
    if len(h) == 0:
        return np.zeros((nby, nbz), dtype=np.int64), np.zeros((nby, nbz)), np.zeros((nby, nbz)), 0.0
    y, z, I, t, P = support.host(h.yList(None)), support.host(h.zList(None)), support.host(h.IList(None)), support.host(h.t), support.host(h.P)
    lam = support.hit_wavelengths(wavelength, h)
    qr = support.host(h._gather(h.segs.q_re, h.slot)) + t
    qi, n = support.host(h._gather(h.segs.q_im, h.slot)), support.host(h._gather(h.segs.n_index, h.slot))
    w = np.sqrt(lam * (qr * qr + qi * qi) / (n * np.pi * qi))
    assert np.all(np.isfinite(w) & (w > 0))
    clear = min(np.abs(y[:, None] - y_edges[None, :]).min(), np.abs(z[:, None] - z_edges[None, :]).min())
    print(f"  {len(y)} hits, w from {w.min():.3g} to {w.max():.3g}, smallest distance of a centre to a bin edge {clear:.3g}")
    assert clear > 1e-9
    rel = REL * U + 2 * U * np.abs(t) * np.abs(qr) / (qr * qr + qi * qi)

    def axis(v, edges, tangent):
        a = np.sqrt(2.0) * (edges[None, :] - v[:, None]) / w[:, None]
        E = erf(a)
        S = np.abs(P) @ np.abs(np.asarray(tangent, dtype=float))
        d_edge = 2 / np.sqrt(np.pi) * np.exp(-a * a) * (rel[:, None] * np.abs(a) + (np.sqrt(2.0) * 8 * U * S / w)[:, None]) + 2 * (E_REF + E_DEV) * U * np.abs(E)
        F = 0.5 * np.diff(E, axis=1)
        return F, 0.5 * (d_edge[:, 1:] + d_edge[:, :-1]) + 2 * U * np.abs(F)

    Fy, dFy = axis(y, y_edges, h.monitor.tangent_Y)
    Fz, dFz = axis(z, z_edges, h.monitor.tangent_Z)
    power = np.einsum("j,jy,jz->yz", I, Fy, Fz)
    c = (Fy > 0).astype(np.float64).T @ (Fz > 0).astype(np.float64)
    bound = (np.einsum("j,jy,jz->yz", I, dFy, Fz) + np.einsum("j,jy,jz->yz", I, Fy, dFz) + np.einsum("j,jy,jz->yz", I, dFy, dFz)
             + 4 * U * power + 1.6e-23 * I.sum() + 2 * c * U * power)
    counts = np.histogram2d(y, z, bins=[y_edges, z_edges])[0].astype(np.int64)
    return counts, power, bound, float(I.sum())


def _assert_against(counts, power, ref, what=""):
    c, ref_power, bound, total = ref
    np.testing.assert_array_equal(counts, c)
    assert np.all(bound <= 1e-10 * total), (float(bound.max()), total)  # the cap: asserted from the reference alone
    err = np.abs(power - ref_power)
    at = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"  {what}{int(c.sum())} centres in range, power {ref_power.sum():.6g} of {total:.6g}; largest error {err.max():.3g}, "
          f"nearest to its bound {err[at]:.3g} of {bound[at]:.3g}; largest bound {bound.max():.3g}")
    assert np.all(err <= bound), (float(err[at]), float(bound[at]))
    return c


def _assert_beam(b, h, wavelength, what=""):
    counts, power, y_edges, z_edges = b.to_host()
    assert b.monitor is h.monitor and counts.dtype == np.int64 and power.dtype == np.float64
    assert counts.shape == power.shape == (len(y_edges) - 1, len(z_edges) - 1) == b.bins
    return _assert_against(counts, power, _reference(h, wavelength, y_edges, z_edges), what)


# -- 1, 2: segments by hand ---------------------------------------------------------------------------------------------------
WL_HAND = 0.5


def _hand_segments(y, z, w, valid, qr=None, n_index=None, intensity=None):
    """len(y) slots of a [1][ray] slots layout: rays (0, y, z) + t (1, 0, 0) of length 10 onto a monitor at x = 5 (t = 5), with q such
    that the spot size there is `w` at the wavelength WL_HAND: q_re = qr - 5 (qr = 0 where the spot is too small to be `qr` from
    its waist), and qi the larger root of w^2 = WL (qr^2 + qi^2) / (n pi qi).  Slot k is valid iff valid[k] (seg_count)."""
    N = len(y)
    qr = np.zeros(N) if qr is None else np.asarray(qr, dtype=float)
    n_index = np.ones(N) if n_index is None else np.asarray(n_index, dtype=float)
    half = n_index * np.pi * np.asarray(w, dtype=float) ** 2 / WL_HAND / 2
    qr = np.where(half > 2 * np.abs(qr), qr, 0.0)  # (a spot this small has its waist at the monitor)
    qi = half + np.sqrt(half**2 - qr**2)
    segs = SegmentBatch(N, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()

    def put(field, values):
        segs.field(field).copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)))

    put("oy", y), put("oz", z), put("q_re", qr - 5.0), put("q_im", qi), put("n", n_index)
    put("intensity", np.ones(N) if intensity is None else intensity)
    segs.dx.fill_(1.0)
    segs.length.fill_(10.0)
    segs.ray.copy_(torch.arange(N, dtype=torch.int32))
    segs.count = torch.from_numpy(np.asarray(valid, dtype=np.int32)).cuda()
    segs.n_rays = N
    assert segs.layout == "slots"
    return segs


def test_hand_built_footprints_from_one_bin_to_the_whole_image():
    """130 slots, two full waves and two lanes: wave 0 has 64 hits, wave 1 hits in its lanes 0 (slot 64), 6, 36 and 63, wave 2 none
    (slot 128 misses the monitor, slot 129 would hit and is invalid by seg_count).  w from 0.01 to 20 on a 6 x 6 monitor of 7 x 5 bins:
    footprints of one bin up to all 35, clipped at every border."""
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
    segs = _hand_segments(y, z, w, valid, qr=qr, n_index=np.where(np.arange(N) % 2, 1.5, 1.0), intensity=0.25 + 0.75 * rng.random(N))
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 6, 6)
    h = table.record_all(segs, monitors=[mon])[0]
    assert sorted(h.slot.tolist()) == list(range(64)) + [64, 70, 100, 127]
    np.testing.assert_allclose(support.host(h.spotsizeList(WL_HAND, None)), w[h.slot.cpu().numpy()], rtol=1e-12)
    b = table.beam_batch(mon, segs, WL_HAND, bins=(7, 5))
    c = _assert_beam(b, h, WL_HAND)
    assert c.sum() == 68 and torch.equal(b.counts, table.image_batch(mon, segs, bins=(7, 5)).counts)
    assert int((b.power > 0).sum()) == 35 and float(b.power.sum()) < float(h.IList(None).sum())
    area = (6 / 7) * (6 / 5)
    np.testing.assert_allclose(b.irradiance().cpu().numpy(), b.power.cpu().numpy() / area, rtol=1e-14)


def test_more_edges_than_lanes():
    """bins = (130, 2): 131 y edges, more than a wave has lanes — beams that cover all of them, one that crosses the chunk boundary
    only, one inside a chunk.  The same beams at bins = (1, 1) against the closed form."""
    y = np.array([0.013, -2.5, 2.7, -0.11, 1.3, 0.4])
    z = np.array([0.021, 1.1, -2.2, 0.3, -0.7, 2.9])
    w = np.array([20.0, 3.0, 1.5, 0.05, 0.5, 0.004])
    I = np.array([1.0, 0.5, 0.25, 2.0, 0.75, 1.5])
    segs = _hand_segments(y, z, w, np.ones(6, dtype=np.int32), intensity=I)
    table, mon = oa.OpticalTable(), oa.Monitor([5, 0, 0], 6, 6)
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) == 6
    b = table.beam_batch(mon, segs, WL_HAND, bins=(130, 2))
    _assert_beam(b, h, WL_HAND)
    assert int((b.power > 0).sum()) == 260  # the widest alone reaches every bin
    one = table.beam_batch(mon, segs, WL_HAND, bins=(1, 1))
    _assert_beam(one, h, WL_HAND)
    s = np.sqrt(2.0)
    closed = (I * 0.25 * (erf(s * (3 - y) / w) + erf(s * (3 + y) / w)) * (erf(s * (3 - z) / w) + erf(s * (3 + z) / w))).sum()
    bounds = [_reference(h, WL_HAND, *image_edges(mon, *bins))[2].sum() for bins in ((1, 1), (130, 2))]
    print(f"  (1, 1): {float(one.power[0, 0]):.15g} against the closed form {closed:.15g}, bound {bounds[0]:.3g}; (130, 2) sums to "
          f"{float(b.power.sum()):.15g}, bound {bounds[1] + 260 * U * closed:.3g}")
    assert abs(float(one.power[0, 0]) - closed) <= bounds[0]
    assert abs(float(b.power.cpu().numpy().sum()) - closed) <= bounds[1] + 260 * U * closed  # (the sum of 260 bins: 260 roundings more)
    assert int(one.counts[0, 0]) == 6


# -- 3: cfg 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case3():
    """cfg 2, 5,003 rays, 5 segments, eight monitors: (table, monitors, {(layout, precision): (batch, segs, record_all hits)}), traced
    and recorded on first use."""
    table, mons, made = support.cfg2_table(), support.eight_monitors(), {}
    o, d = scenes.cfg2_rays(5003, 0)

    def get(layout, precision):
        if (layout, precision) not in made:
            batch = support.waisted_batch(o, d, precision)
            segs = table.trace_batch(batch, max_segments=5, layout=layout)
            assert segs.layout == layout and segs.precision == precision
            made[layout, precision] = (batch, segs, table.record_all(segs, monitors=mons))
        return made[layout, precision]

    return table, mons, get


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["slots", "tiled", "append"])
def test_layouts_and_precisions(case3, layout, precision, monkeypatch):
    table, mons, get = case3
    batch, segs, hits = get(layout, precision)
    assert beam_plan(len(mons), 30, 30) == {"path": "lds", "per_pass": 4, "passes": 2}
    table.monitors = []
    table.add_monitors(mons)

    def refuse(self, *args, **kwargs):
        raise AssertionError("beam_all converted the batch")

    with monkeypatch.context() as mp:
        mp.setattr(SegmentBatch, "to_slots", refuse)
        mp.setattr(SegmentBatch, "astype", refuse)
        beams = table.beam_all(segs, scenes.WL)  # the table's own monitors, in their order, bins=30
        images = table.image_all(segs)
    assert len(beams) == len(mons) and all(b.monitor is m for b, m in zip(beams, mons))
    assert all(b.counts.is_cuda and b.counts.dtype == torch.int64 and b.power.dtype == torch.float64 for b in beams)
    totals = [int(_assert_beam(b, h, scenes.WL, what=f"monitor {k}: ").sum()) for k, (b, h) in enumerate(zip(beams, hits))]
    for b, im in zip(beams, images):
        assert torch.equal(b.counts, im.counts)
    assert len(hits[EMPTY]) == 0 and totals[EMPTY] == 0 and not beams[EMPTY].power.any()
    assert 0 < totals[DROPS] < len(hits[DROPS])  # centres off the image are counted nowhere ...
    slots = torch.cat([h.slot for h in hits])
    assert len(torch.unique(slots)) < len(slots)  # ... and one slot hits several monitors
    if layout == "slots" and precision == "f64":
        per_ray = table.beam_all(segs, batch, monitors=[mons[3], mons[0]])  # the traced batch's wavelengths; the monitors given
        _assert_beam(per_ray[0], hits[3], batch)
        _assert_beam(per_ray[1], hits[0], batch)
        again = table.beam_all(segs, scenes.WL)
        assert all(torch.equal(a.counts, b.counts) for a, b in zip(again, beams))


def test_tails_of_centres_off_the_image(case3):
    """The 0.4 x 6 monitor under RotX(0.5): its lab-tangent projection leaves the image range, so some centres are counted nowhere;
    their tails are inside all the same (the reference sums every hit)."""
    table, mons, get = case3
    _, segs, hits = get("slots", "f64")
    h = hits[DROPS]
    ey, ez = image_edges(mons[DROPS], 30, 30)
    y, z = support.host(h.yList(None)), support.host(h.zList(None))
    outside = (y < ey[0]) | (y > ey[-1]) | (z < ez[0]) | (z > ez[-1])
    assert 0 < outside.sum() < len(h)
    b = table.beam_batch(mons[DROPS], segs, scenes.WL)
    _assert_beam(b, h, scenes.WL)
    assert int(b.counts.sum()) == int((~outside).sum())
    inside_only = MonitorHits.__new__(MonitorHits)
    keep = torch.from_numpy(~outside).cuda()
    inside_only.monitor, inside_only.segs = h.monitor, h.segs
    inside_only.slot, inside_only.P, inside_only.t, inside_only.ray = h.slot[keep], h.P[keep], h.t[keep], h.ray[keep]
    _, without, bound, _ = _reference(inside_only, scenes.WL, ey, ez)
    gap = b.power.cpu().numpy() - without
    print(f"  the off-image centres add up to {gap.max():.3g} to a bin, bound there {bound.flat[np.argmax(gap)]:.3g}")
    assert gap.max() > 1e3 * bound.flat[np.argmax(gap)]  # the tails are there, and far above the bound


# -- 4, 5: the global path, accumulation ----------------------------------------------------------------------------------------
def test_global_path_and_accumulation():
    """(80, 80): 6,400 bins, more than the LDS budget — every deposit a global atomic, narrow beams and beams as wide as the image.
    And `into=` over the two chunks of a batch against the whole batch in one call, on either path."""
    table = support.cfg2_table()
    mon = oa.Monitor([7.5, 0, 0], 2, 2)
    assert beam_plan(1, 80, 80)["path"] == "global" and beam_plan(1, 30, 30)["path"] == "lds"
    whole = support.waisted_batch(*scenes.cfg2_rays(2049, 3))
    segs = table.trace_batch(whole, max_segments=5, layout="slots")
    h = table.record_all(segs, monitors=[mon])[0]
    full = table.beam_all(segs, whole, bins=(80, 80), monitors=[mon])
    assert int(_assert_beam(full[0], h, whole).sum()) == len(h) >= 2049
    w = support.host(h.spotsizeList(whole, None))
    assert w.min() < 2 / 80 and w.max() > 0.5  # less than a bin across, and a spot as wide as the monitor
    for bins in ((80, 80), (30, 30)):
        chunks = [whole.slice(0, 1024), whole.slice(1024, 2049)]
        parts = [table.trace_batch(b, max_segments=5, layout="slots") for b in chunks]
        beams = table.beam_all(parts[0], chunks[0], bins=bins, monitors=[mon])
        first = beams[0].counts.clone()
        assert table.beam_all(parts[1], chunks[1], bins=bins, monitors=[mon], into=beams) == beams
        refs = [_reference(table.record_all(p, monitors=[mon])[0], b, beams[0].y_edges, beams[0].z_edges) for p, b in zip(parts, chunks)]
        summed = tuple(r0 + r1 for r0, r1 in zip(*refs))
        counts, power, _, _ = beams[0].to_host()
        _assert_against(counts, power, summed, what=f"{bins} in two chunks: ")
        assert int(first.sum()) < int(counts.sum())
        once = table.beam_all(segs, whole, bins=bins, monitors=[mon])[0]
        assert torch.equal(once.counts, beams[0].counts)
        _assert_beam(once, h, whole, what=f"{bins} at once: ")
        assert float(beams[0].power.sum()) <= summed[3] and float(once.power.sum()) <= summed[3]  # sum of power <= sum of I
        # without `into=` a call starts from zero again
        assert torch.equal(table.beam_all(parts[0], chunks[0], bins=bins, monitors=[mon])[0].counts, first)


# -- 6: ray trees -------------------------------------------------------------------------------------------------------------
def test_ray_trees_inherit_the_wavelength():
    """The Michelson of tests/test_gpu_field.py with Gaussian beams of two colours: both children of a tree reach the monitor, and
    the wavelength of either comes through its segment's `ray`, the index of the tree's input ray."""
    i, j = np.divmod(np.arange(257), 17)
    o = np.stack([(i - 8) / 32 + 1 / 64, np.full(257, 2.0), (j - 8) / 32 + 1 / 64], axis=1)
    wl = np.where(np.arange(257) % 2, 780e-7, 400e-7)
    batch = RayBatch.from_arrays(o, np.tile([0.0, -1.0, 0.0], (257, 1)), wavelength=wl, q=1j * np.pi * 0.01**2 / 780e-7, device="cuda")
    table = oa.OpticalTable()
    table.add_components([oa.BeamSplitter([0, 0, 0], width=2, height=2, eta=0.5).RotZ(np.pi / 4),
                          oa.SquareMirror([3.0, 0, 0], width=2, height=2).RotZ(np.pi),
                          oa.SquareMirror([0, -2.75, 0], width=2, height=2).RotZ(np.pi / 2)])
    mon = oa.Monitor([-2, 0, 0], 0.6, 0.6)
    segs = table.trace_batch(batch, max_segments=8)
    h = table.record_all(segs, monitors=[mon])[0]
    assert len(h) == 2 * 257 and torch.equal(h.ray_index(None), torch.arange(257, device="cuda").repeat_interleave(2))
    b = table.beam_batch(mon, segs, batch, bins=(9, 4))
    assert int(_assert_beam(b, h, batch).sum()) == 2 * 257
    # the two arms differ in length, and the colours in spot size: one wavelength for all is another image
    w = support.host(h.spotsizeList(batch, None))
    assert len(set(np.round(w, 7))) == 4
    g = table.beam_batch(mon, segs, 780e-7, bins=(9, 4))
    _assert_beam(g, h, 780e-7)
    assert torch.equal(g.counts, b.counts) and float((g.power - b.power).abs().max()) > 1e-3


# -- 7, 8: hits left out, refusals --------------------------------------------------------------------------------------------
class _Out(support.Sentinel):
    """counts / power of M monitors of nby x nbz bins and `skipped` for ot_monitor_beam_many, filled with a sentinel."""

    def __init__(self, M, nby, nbz):
        super().__init__(counts=(torch.int64, (M, nby, nbz)), power=(torch.float64, (M, nby, nbz)), skipped=(torch.int64, (1,)))


def _call(lib, ctx, mons, segs, nby, nbz, out, wavelength=None, n_wavelengths=0, uniform=0.0, accumulate=0, source=None, **planes):
    src, n, count, n_rays = segment_source(segs)
    table = (abi.OtMonitor * len(mons))(*[monitor_struct(m) for m in mons])
    axes, edges = support.image_tables(mons, nby, nbz)
    dp = C.POINTER(C.c_double)
    plane = {f: planes.get(f, segs.field(f).data_ptr()) for f in ("intensity", "q_re", "q_im", "n")}
    return lib.ot_monitor_beam_many(ctx, table, len(mons), axes.ctypes.data_as(dp), edges.ctypes.data_as(dp), nby, nbz,
                                    C.byref(src if source is None else source), plane["intensity"], plane["q_re"], plane["q_im"], plane["n"],
                                    None if wavelength is None else wavelength.data_ptr(), n_wavelengths, uniform, n,
                                    None if count is None else count.data_ptr(), n_rays, planes.get("counts", out.counts.data_ptr()),
                                    planes.get("power", out.power.data_ptr()), planes.get("skipped", out.skipped.data_ptr()), accumulate)


def test_a_batch_without_q_is_refused(case3):
    table, mons, _ = case3
    o, d = scenes.cfg2_rays(300, 5)
    plain = RayBatch.from_arrays(o, d, wavelength=scenes.WL, device="cuda")  # no q
    segs = table.trace_batch(plain, max_segments=5, layout="slots")
    pick = [mons[0], mons[SPREAD]]
    hits = table.record_all(segs, monitors=pick)
    n_hits = sum(len(h) for h in hits)
    assert n_hits >= 600
    with pytest.raises(ValueError, match=f"{n_hits} hits"):
        table.beam_all(segs, scenes.WL, monitors=pick)
    eng = get_engine()
    out = _Out(2, 30, 30)
    with eng.lock:
        assert _call(eng.lib, eng._ctx, pick, segs, 30, 30, out, uniform=scenes.WL) == 0, eng.lib.ot_last_error()
    torch.cuda.synchronize()
    assert int(out.skipped.item()) == n_hits and not out.counts.any() and not out.power.any()
    # ... and the guard on the wavelength gather: the library is told of 100 wavelengths (the buffer holds all 5,003 of another
    # batch, so a missing guard reads valid memory and fails the assertion: nothing can fault)
    batch, segs, hits = case3[2]("slots", "f64")
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
    for plane in ("intensity", "q_re", "q_im", "n", "counts", "power", "skipped"):
        expect(call(**{plane: None}), "NULL")
    no_field = altered()
    no_field.base[6] = None
    expect(call(source=no_field), "NULL field")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        expect(call(uniform=bad), "wavelength_uniform")
    expect(call(wavelength=wl, n_wavelengths=0), "n_wavelengths")
    expect(call(wavelength=wl, n_wavelengths=-1), "n_wavelengths")
    expect(call(accumulate=2), "accumulate")  # ... and what ot_monitor_image_many refuses
    expect(call(source=altered(capacity=64)), "capacity")
    assert lib.ot_ctx_synchronize(c) == 0
    assert out.untouched()  # nothing was launched or zeroed
    # the context is still good; the array and the one value give the same image; accumulate adds
    assert call() == 0, lib.ot_last_error()
    assert lib.ot_ctx_synchronize(c) == 0
    assert int(out.counts.sum()) == 130 and int(out.skipped.item()) == 0
    power = out.power.clone()
    assert float(power.sum()) > 100
    assert call(wavelength=wl, n_wavelengths=130, uniform=float("nan")) == 0 and lib.ot_ctx_synchronize(c) == 0
    assert torch.allclose(out.power, power, rtol=0, atol=1e-12)
    assert call(accumulate=1) == 0 and lib.ot_ctx_synchronize(c) == 0
    assert int(out.counts.sum()) == 260 and torch.allclose(out.power, 2 * power, rtol=0, atol=1e-12)
