"""CPU: the diffraction PSF's host side — the binding against the header, the planner against the kernel's constants, what
`OpticalTable.psf_all` refuses before the engine is asked and what it hands over, `MonitorPSF`'s methods against numpy on synthetic
fields, and two physics checks of the definition itself (tests/psf_reference.py): a uniform disc of direction cosines gives the Airy
pattern, and a small spherical aberration gives the Strehl ratio the Marechal approximation predicts."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import optable_amd as oa
import support
from optable_amd import abi, engine
from optable_amd import psf as psfm
from psf_reference import airy, disc_grid, plane_wave_sum, psf_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = 780e-7


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_psf_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_psf_many is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = abi.SYMBOLS["ot_monitor_psf_many"]
    assert restype is C.c_int and len(argtypes) == len(params) == 25
    for p, a in zip(params, argtypes):
        if "*" in p:
            assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (p, a)
        elif p.startswith("int32_t"):
            assert a is C.c_int32, (p, a)
        elif p.startswith("int64_t"):
            assert a is C.c_int64, (p, a)
        elif p.startswith("double"):
            assert a is C.c_double, (p, a)
        else:
            raise AssertionError(p)
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["ctx", "mons", "n_monitors", "axes", "reference_kind", "reference", "grid", "ny", "nz", "src", "intensity", "n_index", "pathlength",
                     "wavelength", "n_wavelengths", "wavelength_uniform", "amplitude_mode", "n_segments", "seg_count", "n_rays", "counts", "norm", "re", "im",
                     "accumulate"]
    assert oa.MonitorPSF is psfm.MonitorPSF


def test_planner_and_its_constants():
    header = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    kernels = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()

    def constant(name):
        return int(re.search(rf"\b{name}\s*=\s*(\d+)", kernels).group(1))

    assert int(re.search(r"#define\s+OT_PSF_MAX_SAMPLES\s+(\d+)", header).group(1)) == engine.PSF_MAX_SAMPLES == constant("MON_PSF_MAX_SAMPLES") == psfm.MAX_SAMPLES
    assert int(re.search(r"#define\s+OT_PSF_SCRATCH_BYTES\s+(\d+)", header).group(1)) == engine.PSF_SCRATCH_BYTES
    assert engine.PSF_CHUNK_MIN == constant("MON_PSF_CHUNK_MIN") and engine.PSF_MAX_CHUNKS == constant("MON_PSF_MAX_CHUNKS")
    assert engine.PSF_PARTIAL_ROWS == constant("MON_PSF_PARTIAL_ROWS") and constant("MON_PSF_TILE") == 64 and engine.PSF_ROW == 2 * 64 * 64 + 8
    assert engine.PSF_AMPLITUDES == psfm.AMPLITUDES
    # tiles: subtiles of 16 split evenly into parts of at most 4
    assert engine.psf_plan(1, 1)["tiles"] == [(0, 1, 0, 1)]
    assert engine.psf_plan(33, 17)["tiles"] == [(0, 33, 0, 17)]
    assert engine.psf_plan(65, 65)["tiles"] == [(0, 32, 0, 32), (0, 32, 32, 33), (32, 33, 0, 32), (32, 33, 32, 33)]
    assert engine.psf_plan(512, 3)["tiles"] == [(64 * k, 64, 0, 3) for k in range(8)]
    for n in range(1, 513):
        parts = engine._psf_parts(n)
        assert parts[0][0] == 0 and sum(c for _, c in parts) == n and all(1 <= c <= 64 for _, c in parts)
        assert all(a + c == b for (a, c), (b, _) in zip(parts, parts[1:])) and all(a % 16 == 0 for a, _ in parts)
    # chunks: a function of the hit count alone
    plan = engine.psf_plan(129, 129, [0, 1, 512, 513, 1027, 2_000_000])
    assert plan["chunks"] == [1, 1, 1, 2, 3, 256] and plan["chunk_hits"] == [0, 1, 512, 257, 343, 7813]
    assert len(plan["tiles"]) == 9 and plan["pairs_a_launch"] == 4 and plan["launches"] == 14
    assert plan["pairs_a_launch"] * max(plan["chunks"]) <= engine.PSF_PARTIAL_ROWS
    assert engine.psf_plan(33, 33, [100, 100]) == {"tiles": [(0, 33, 0, 33)], "chunks": [1, 1], "chunk_hits": [100, 100], "pairs_a_launch": 2, "launches": 1}
    for ny, nz in ((0, 5), (5, 0), (513, 5), (5, 513)):
        with pytest.raises(ValueError):
            engine.psf_plan(ny, nz)


class _Recorder:
    """Stands in for the engine: keeps what psf_all hands over."""
    aliased = 0

    def monitor_psf_many(self, mons, axes, kind, reference, grid, pixels, segs, wavelength, amplitude_mode=0, into=None):
        self.axes, self.kind, self.reference, self.grid, self.pixels, self.wavelength, self.mode, self.into, self.n = (
            axes, kind, reference, grid, pixels, wavelength, amplitude_mode, into, len(mons))
        if into is not None:
            into[0][:, 0] += 1
            into[0][:, 2] += self.aliased
            return into
        counts = torch.zeros((len(mons), 3), dtype=torch.int64)
        counts[:, 2] = self.aliased
        return counts, torch.zeros(len(mons), dtype=torch.float64), torch.zeros((len(mons), *pixels), dtype=torch.float64), torch.zeros(
            (len(mons), *pixels), dtype=torch.float64)


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table, segs = oa.OpticalTable(), support.host_segments()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6)]
    table.add_monitors(mons)
    good = dict(direction=(1, 0, 0), step=1e-5)
    with pytest.raises(ValueError, match="exactly one"):
        table.psf_all(segs, WL, step=1e-5)
    with pytest.raises(ValueError, match="exactly one"):
        table.psf_all(segs, WL, focus=(1, 0, 0), direction=(1, 0, 0), step=1e-5)
    with pytest.raises(ValueError, match="direction"):
        table.psf_all(segs, WL, direction=(0, 0, 0), step=1e-5)
    with pytest.raises(ValueError, match="step"):
        table.psf_all(segs, WL, direction=(1, 0, 0))
    for step in (0.0, -1e-5, np.nan, np.inf, (1e-5, 0.0), (1e-5,), (1e-5, 1e-5, 1e-5), "fine", True):
        with pytest.raises(ValueError, match="step"):
            table.psf_all(segs, WL, direction=(1, 0, 0), step=step)
    for pixels in (0, 513, (5, 0), (5, 513), 2.5, (3, 3, 3), "many", True, -1):
        with pytest.raises(ValueError, match="pixels"):
            table.psf_all(segs, WL, pixels=pixels, **good)
    for centre in ((0.0, np.nan), (1.0,), [(0, 0)] * 3, "middle"):
        with pytest.raises(ValueError, match="centre"):
            table.psf_all(segs, WL, centre=centre, **good)
    for amplitude in ("power", None, 0, "Sqrt"):
        with pytest.raises(ValueError, match="amplitude"):
            table.psf_all(segs, WL, amplitude=amplitude, **good)
    for wavelength in (0.0, -WL, np.nan, "red", None):
        with pytest.raises(ValueError, match="wavelength"):
            table.psf_all(segs, wavelength, **good)
    with pytest.raises(ValueError, match="double-precision"):
        table.psf_all(support.host_segments(precision="f32"), WL, **good)
    with pytest.raises(AssertionError, match="the engine was asked for"):
        table.psf_all(segs, WL, **good)
    # `into`: the list of ONE earlier call for the same monitors, reference, grid and amplitude
    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    first, other = table.psf_all(segs, WL, pixels=(5, 7), **good), table.psf_all(segs, WL, pixels=(5, 7), **good)
    monkeypatch.setattr(table_module, "_engine", refuse)
    for kwargs in ({"step": 2e-5}, {"pixels": (7, 5)}, {"centre": (0.0, 1e-6)}, {"amplitude": "unit"}, {"direction": (1, 0.1, 0)}, {"monitors": mons[::-1]},
                   {"monitors": mons[:1]}):
        with pytest.raises(ValueError, match="into"):
            table.psf_all(segs, WL, **{**good, "pixels": (5, 7), **kwargs}, into=first)
    with pytest.raises(ValueError, match="into"):
        table.psf_all(segs, WL, focus=(1, 0, 0), step=1e-5, pixels=(5, 7), into=first)
    for into in ([first[0], other[1]], first[::-1], first[:1], (first[0].re, first[0].im), [first[0], "psf"]):
        with pytest.raises(ValueError, match="into"):
            table.psf_all(segs, WL, pixels=(5, 7), **good, into=into)


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table, segs = oa.OpticalTable(), support.host_segments()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6).RotZ(0.3)]
    table.add_monitors(mons)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        psfs = table.psf_all(segs, WL, focus=(9.0, 0.5, 0.0), step=1e-4)
    assert rec.n == 2 and rec.kind == 0 and rec.pixels == (65, 65) and rec.mode == 0 and rec.wavelength == WL and rec.into is None
    np.testing.assert_array_equal(rec.axes, [np.concatenate([m.tangent_Y, m.tangent_Z]) for m in mons])
    np.testing.assert_allclose(rec.reference[0], [1.5, 0.5, 0.0], atol=1e-15)  # the focus in the monitor's frame
    np.testing.assert_allclose(rec.grid, [[-32e-4, 1e-4, -32e-4, 1e-4]] * 2, rtol=1e-15)
    assert [p.monitor for p in psfs] == mons and all(isinstance(p, oa.MonitorPSF) for p in psfs)
    p = psfs[0]
    assert p.reference == ("focus", (9.0, 0.5, 0.0)) and p.step == (1e-4, 1e-4) and p.centre == (0.0, 0.0) and p.amplitude == "sqrt"
    assert p.re.shape == (65, 65) and len(p.y) == len(p.z) == 65 and abs(p.y[32]) < 1e-18 and p.extent == (p.y[0], p.y[-1], p.z[0], p.z[-1])
    psfs = table.psf_all(segs, WL, direction=(0, 2, 0), step=(1e-5, 2e-5), pixels=(4, 7), centre=[(1e-5, 0.0), (0.0, -2e-5)], amplitude="unit",
                         monitors=mons[::-1])
    assert rec.kind == 1 and rec.mode == 2 and rec.pixels == (4, 7)
    np.testing.assert_allclose(rec.grid, [[1e-5 - 1.5e-5, 1e-5, -6e-5, 2e-5], [-1.5e-5, 1e-5, -2e-5 - 6e-5, 2e-5]], rtol=1e-14, atol=1e-20)
    assert psfs[0].monitor is mons[1] and psfs[0].reference == ("direction", (0.0, 1.0, 0.0)) and psfs[1].centre == (0.0, -2e-5)
    np.testing.assert_allclose(psfs[1].z, -2e-5 + (np.arange(7) - 3) * 2e-5, atol=1e-20)
    again = table.psf_all(segs, WL, direction=(0, 2, 0), step=(1e-5, 2e-5), pixels=(4, 7), centre=[(1e-5, 0.0), (0.0, -2e-5)], amplitude="unit",
                          monitors=mons[::-1], into=psfs)
    assert all(a is b for a, b in zip(again, psfs)) and rec.into[0] is psfs[0]._stack[0] and int(psfs[1].counts) == 1
    one = table.psf_batch(mons[1], segs, WL, direction=(1, 0, 0), step=1e-5, pixels=3, amplitude="linear")
    assert rec.n == 1 and rec.mode == 1 and one.monitor is mons[1] and one.re.shape == (3, 3)
    # aliased hits: one RuntimeWarning a call that finds any, for what THIS call added
    rec.aliased = 5
    with pytest.warns(RuntimeWarning, match="10 hits are aliased") as caught:
        psfs = table.psf_all(segs, WL, direction=(1, 0, 0), step=1e-5, pixels=3)
    assert len(caught) == 1 and int(psfs[0].aliased) == 5
    with pytest.warns(RuntimeWarning, match="10 hits are aliased"):
        table.psf_all(segs, WL, direction=(1, 0, 0), step=1e-5, pixels=3, into=psfs)
    rec.aliased = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        table.psf_all(segs, WL, direction=(1, 0, 0), step=1e-5, pixels=3, into=psfs)
    assert table.psf_all(segs, WL, direction=(1, 0, 0), step=1e-5, monitors=[]) == []


def _psf(field, norm, step=(0.5, 0.25), centre=(0.0, 0.0), counts=(3, 0, 0)):
    field = np.asarray(field, dtype=np.complex128)
    ny, nz = field.shape
    grid = (centre[0] - (ny - 1) / 2 * step[0], step[0], centre[1] - (nz - 1) / 2 * step[1], step[1])
    return oa.MonitorPSF(None, torch.tensor(counts, dtype=torch.int64), torch.tensor(float(norm), dtype=torch.float64), torch.tensor(field.real.copy()),
                         torch.tensor(field.imag.copy()), ("focus", (0.0, 0.0, 0.0)), grid, step, centre, "sqrt")


def test_methods_on_hand_made_fields():
    rng = np.random.default_rng(5)
    field = rng.normal(size=(9, 11)) + 1j * rng.normal(size=(9, 11))
    p = _psf(field, 4.0)
    I = np.abs(field) ** 2
    assert p.field.dtype == torch.complex128
    np.testing.assert_allclose(p.field.numpy(), field, rtol=0, atol=0)
    np.testing.assert_allclose(p.intensity().numpy(), I, rtol=1e-15)
    np.testing.assert_allclose(p.normalised().numpy(), I / 16.0, rtol=1e-15)
    assert float(p.strehl()) == pytest.approx(I[4, 5] / 16.0, rel=1e-15) and float(p.strehl("peak")) == pytest.approx(I.max() / 16.0, rel=1e-15)
    with pytest.raises(ValueError, match="at"):
        p.strehl("centre")
    mtf, fy, fz = p.mtf()
    want = np.abs(np.fft.fftshift(np.fft.fft2(I))) / I.sum()
    np.testing.assert_allclose(mtf, want, rtol=1e-13)
    assert mtf[4, 5] == pytest.approx(1.0, rel=1e-14) and fy[4] == 0.0 and fz[5] == 0.0  # the zero frequency in the middle
    np.testing.assert_allclose(fy, np.fft.fftshift(np.fft.fftfreq(9, 0.5)))
    np.testing.assert_allclose(fz, np.fft.fftshift(np.fft.fftfreq(11, 0.25)))
    radii = [0.0, 0.3, 0.6, 1.0, 10.0]
    r = np.hypot(p.y[:, None], p.z[None, :])
    np.testing.assert_allclose(p.encircled_energy(radii, about="reference"), [I[r <= x].sum() / I.sum() for x in radii], rtol=1e-14)
    cy, cz = (I.sum(1) @ p.y) / I.sum(), (I.sum(0) @ p.z) / I.sum()
    rc = np.hypot(p.y[:, None] - cy, p.z[None, :] - cz)
    got = p.encircled_energy(radii)
    np.testing.assert_allclose(got, [I[rc <= x].sum() / I.sum() for x in radii], rtol=1e-14)
    assert got[-1] == pytest.approx(1.0, rel=1e-15) and np.all(np.diff(got) >= 0)
    with pytest.raises(ValueError, match="about"):
        p.encircled_energy(radii, about="peak")
    used, skipped, aliased, norm, host = p.to_host()
    assert (used, skipped, aliased, norm) == (3, 0, 0, 4.0) and host.dtype == np.complex128 and np.array_equal(host, field)
    # no sample on the reference: an even count, or a centre off it
    for q in (_psf(field[:8], 4.0), _psf(field, 4.0, centre=(0.1, 0.0))):
        with pytest.raises(ValueError, match="reference"):
            q.strehl()
        assert float(q.strehl("peak")) > 0
    assert float(_psf(field, 4.0, centre=(0.5, -0.25)).strehl()) == pytest.approx(I[3, 6] / 16.0, rel=1e-15)  # the reference one sample off the middle
    # a monitor never hit: zeros, norm 0, NaN methods
    dark = _psf(np.zeros((5, 5)), 0.0, counts=(0, 0, 0))
    assert not dark.intensity().any() and torch.isnan(dark.normalised()).all() and math.isnan(float(dark.strehl())) and math.isnan(float(dark.strehl("peak")))
    assert np.isnan(dark.mtf()[0]).all() and np.isnan(dark.encircled_energy([1.0, 2.0])).all() and dark.to_host()[3] == 0.0


# -- the definition is the PSF: two checks of the reference itself -----------------------------------------------------------------------
NA = 0.1


def _samples(n, radii):
    """n samples out to `radii` Airy radii 0.61 WL / NA on either side, and v = 2 pi NA r / WL of the grid."""
    y = np.linspace(-radii, radii, n) * 0.61 * WL / NA
    return y, 2 * np.pi * NA * np.hypot(y[:, None], y[None, :]) / WL


@pytest.mark.parametrize("grid,tolerance", [(41, 5e-3)])
def test_a_uniform_disc_of_direction_cosines_gives_the_airy_pattern(grid, tolerance):
    """NA 0.1 at 780e-7: a 41 x 41 grid of direction cosines clipped to the disc (1,257 rays), constant W, on 33 x 33 samples out to
    3 Airy radii reproduces (2 J1(v) / v)^2 to 1.9e-3 of the peak (the 21-grid 6.2e-3, the 81-grid 8.3e-4)."""
    t = disc_grid(grid, NA)
    assert grid != 41 or len(t) == 1257
    y, v = _samples(33, 3.0)
    U, norm = plane_wave_sum(t[:, 0], t[:, 1], np.full(len(t), 1.25), WL, y, y)
    err = np.abs(np.abs(U) ** 2 / norm**2 - airy(v)).max()
    print(f"  {len(t)} rays: largest error {err:.3g} of the peak")
    assert err <= tolerance
    assert abs(np.abs(U[16, 16]) ** 2 / norm**2 - 1.0) < 1e-15


def test_a_small_spherical_aberration_gives_the_marechal_strehl():
    """W = 0.05 rho^4 waves on the 81 x 81 disc: Strehl 0.991269 against Marechal's 0.991274."""
    t = disc_grid(81, NA)
    rho2 = (t * t).sum(axis=1) / NA**2
    W = 0.05 * rho2**2  # waves
    U, norm = plane_wave_sum(t[:, 0], t[:, 1], W * WL, WL, [0.0], [0.0])
    strehl = float(np.abs(U[0, 0]) ** 2 / norm**2)
    marechal = math.exp(-((2 * np.pi * W.std()) ** 2))
    print(f"  Strehl {strehl:.6f}, Marechal {marechal:.6f}")
    assert abs(strehl - marechal) <= 1e-4 and strehl < 0.995


def test_the_reference_of_a_hand_made_hit():
    """One segment along x through a monitor at x = 5: P = 0, t = 5, L = 5.25, W = L (direction reference), gy = gz = 0: the field is
    a exp(2 pi i frac(L / lambda)) on every sample, and the bound is norm (2 pi 16 2^-53 L / lambda + 2^-38)."""
    m = oa.Monitor([5, 0, 0], 2, 2)
    from optable_amd.table import monitor_struct

    s = monitor_struct(m)
    ref = psf_reference([[0, 0, 0]], [[1, 0, 0]], [10.0], [0.25], [1.0], [0.25], [0], list(s.M), list(s.origin), s.half_width, s.half_height,
                        np.concatenate([m.tangent_Y, m.tangent_Z]), 1, [1.0, 0.0, 0.0], (-1e-5, 1e-5, -1e-5, 1e-5), 3, 3, 0.5)
    assert ref.counts.tolist() == [1, 0, 0] and ref.norm == 0.5 and ref.hits.tolist() == [0]
    np.testing.assert_allclose(ref.field, np.full((3, 3), 0.5 * np.exp(2j * np.pi * 0.5)), atol=1e-16)
    assert ref.bound == pytest.approx(0.5 * (2 * np.pi * 16 * 2.0**-53 * 5.25 / 0.5 + 2.0**-38), rel=1e-12)
    none = psf_reference([[0, 0, 0]], [[1, 0, 0]], [10.0], [0.25], [1.0], [0.25], [0], list(s.M), list(s.origin), s.half_width, s.half_height,
                         np.concatenate([m.tangent_Y, m.tangent_Z]), 1, [1.0, 0.0, 0.0], (-1e-5, 1e-5, -1e-5, 1e-5), 3, 3, np.array([-1.0]))
    assert none.counts.tolist() == [0, 1, 0] and none.norm == 0.0 and not none.field.any()
