"""CPU: the public surface of coherent Gaussian-beam detector images (`OpticalTable.wave_all` / `wave_batch`: the complex sum of the
hits' Gaussian beams per monitor bin, on the device, ot_monitor_wave_many) — the calls and the binding, the LDS budget and the plan
of passes, what is refused before the engine is asked, what is handed over and what comes back (the `aliased` warning and the
`skipped` error included), the hit-list form of the same quantities (`MonitorHits.radiusList` / `gouyList` / `amplitudeList`)
against the package's own `Ray`, and the registers of the new kernel and of the one it leaves alone.  No library call is made."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import optable_amd as oa
import support
from optable_amd import abi
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import Engine
from optable_amd.monitors import MonitorHits
from test_build_resources import kernels  # noqa: F401  (the fixture: the code objects of the last build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calls_exist():
    from optable_amd import engine, monitors

    assert callable(oa.OpticalTable.wave_all) and callable(oa.OpticalTable.wave_batch)
    assert callable(Engine.monitor_wave_many) and callable(engine.wave_plan)
    for method in ("to_host", "irradiance", "power"):
        assert callable(getattr(monitors.MonitorWave, method))
    assert isinstance(monitors.MonitorWave.field, property) and isinstance(monitors.MonitorWave.bins, property)
    for accessor in ("radiusList", "gouyList", "amplitudeList"):
        assert callable(getattr(MonitorHits, accessor))
    assert "ot_monitor_wave_many" in abi.SYMBOLS


def _declared(text, name):
    decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert decl, f"{name} is not declared in the header"
    return [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = _declared(text, "ot_monitor_wave_many")
    restype, argtypes = abi.SYMBOLS["ot_monitor_wave_many"]
    assert restype is C.c_int and len(argtypes) == len(names) == 27
    # ot_monitor_field_many's list with q_re, q_im after pathlength, gouy after amplitude_mode and aliased after skipped
    want = _declared(text, "ot_monitor_field_many")
    for after, new in (("pathlength", ["q_re", "q_im"]), ("amplitude_mode", ["gouy"]), ("skipped", ["aliased"])):
        at = want.index(after) + 1
        want[at:at] = new
    assert names == want
    widths = {"n_monitors": C.c_int32, "nby": C.c_int32, "nbz": C.c_int32, "amplitude_mode": C.c_int32, "gouy": C.c_int32, "accumulate": C.c_int32,
              "n_wavelengths": C.c_int64, "n_segments": C.c_int64, "n_rays": C.c_int64, "wavelength_uniform": C.c_double}
    for name, kind in zip(names, argtypes):  # pointers as pointers, the integers by their width, the one double
        assert kind is widths[name] if name in widths else kind not in (C.c_int32, C.c_int64, C.c_double), name
    # ... and the field call's binding differs from this one in just those places
    field = list(abi.SYMBOLS["ot_monitor_field_many"][1])
    for after, new in (("pathlength", [C.c_void_p, C.c_void_p]), ("amplitude_mode", [C.c_int32]), ("skipped", [C.c_void_p])):
        at = names.index(after) + 1
        field[at:at] = new
    assert field == list(argtypes)
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)


def test_budget_and_pass_planner():
    from optable_amd import engine

    text = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bMON_WAVE_LDS_BINS\s*=\s*([^;]+);", text)
    strip = re.search(r"\bMON_WAVE_STRIP\s*=\s*(\d+)", text)
    assert found and strip and int(strip.group(1)) == 256
    # 64 KB of LDS a workgroup, less the 128-byte tally of the record mode and four waves' strips of 256 doubles, at 20 bytes a bin
    assert eval(found.group(1).replace("/", "//"), {"MON_MAX": 32, "MON_WAVES": 4, "MON_WAVE_STRIP": 256}) == engine.WAVE_LDS_BINS == 2860
    assert engine.WAVE_LDS_BINS < engine.FIELD_LDS_BINS
    plan = engine.wave_plan
    assert plan(1, 30, 30) == {"path": "lds", "per_pass": 1, "passes": 1}
    assert plan(3, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 1}      # 2,700 bins
    assert plan(4, 30, 30) == {"path": "lds", "per_pass": 2, "passes": 2}      # as even as they come: 2 + 2, not 3 + 1
    assert plan(8, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 3}
    assert plan(1, 2860, 1)["path"] == "lds" and plan(1, 2861, 1)["path"] == "global"  # just over the budget
    assert plan(3, 80, 80) == {"path": "global", "per_pass": 3, "passes": 1}
    assert plan(40, 80, 80) == {"path": "global", "per_pass": 20, "passes": 2}
    # the other planners keep their budgets
    assert engine.image_plan(6, 30, 30) == {"path": "lds", "per_pass": 6, "passes": 1}
    assert engine.field_plan(6, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 2}
    assert engine.beam_plan(6, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 2}
    assert (engine.IMAGE_LDS_BINS, engine.FIELD_LDS_BINS, engine.BEAM_LDS_BINS) == (5450, 3270, 5109)
    for n, nby, nbz in ((0, 3, 3), (1, 0, 3), (1, 3, 0), (1, 1 << 12, (1 << 12) + 1)):
        with pytest.raises(ValueError):
            plan(n, nby, nbz)


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table = oa.OpticalTable()
    mon = oa.Monitor([1, 0, 0], 2, 2)
    good, rays = support.host_segments(), support.host_rays(4, q=1.5j)
    with pytest.raises(ValueError, match=r"wavelength=0\.0: a beam field needs"):
        table.wave_all(good, monitors=[mon])  # the default
    for bad in (0.0, -780e-7, float("nan"), float("inf"), "red", None):
        with pytest.raises(ValueError, match="wavelength"):
            table.wave_all(good, bad, monitors=[mon])
        with pytest.raises(ValueError, match="wavelength"):
            table.wave_batch(mon, good, bad)
    with pytest.raises(ValueError, match="RayBatch of 5 rays"):
        table.wave_all(good, support.host_rays(5, q=1.5j), monitors=[mon])
    for value in (0.0, -1.0, float("nan"), float("inf")):
        dark = support.host_rays(4, q=1.5j)
        dark.wavelength[2] = value
        with pytest.raises(ValueError, match="finite wavelength > 0"):
            table.wave_all(good, dark, monitors=[mon])
    for bins in (0, -3, (30, 0), (30,), 2.5, "30", None, True):
        with pytest.raises(ValueError, match="bins"):
            table.wave_all(good, rays, bins=bins, monitors=[mon])
        with pytest.raises(ValueError, match="bins"):
            table.wave_batch(mon, good, rays, bins=bins)
    for amplitude in ("power", 0, None, "SQRT"):
        with pytest.raises(ValueError, match="amplitude"):
            table.wave_all(good, rays, monitors=[mon], amplitude=amplitude)
        with pytest.raises(ValueError, match="amplitude"):
            table.wave_batch(mon, good, rays, amplitude=amplitude)
    for gouy in (0, 1, None, "yes", 1.0):
        with pytest.raises(ValueError, match="gouy"):
            table.wave_all(good, rays, monitors=[mon], gouy=gouy)
        with pytest.raises(ValueError, match="gouy"):
            table.wave_batch(mon, good, rays, gouy=gouy)
    # single precision is refused with field_all's reasoning, not approximated
    with pytest.raises(ValueError, match="double-precision SegmentBatch.*refused, not approximated"):
        table.wave_all(support.host_segments(precision="f32"), rays, monitors=[mon])
    # ... and what is good gets that far
    for kwargs in ({}, {"gouy": True}, {"amplitude": "linear", "gouy": False}):
        with pytest.raises(AssertionError, match="the engine was asked for"):
            table.wave_all(good, rays, bins=(7, 5), monitors=[mon], **kwargs)
    # the other modes' own words are what they were
    with pytest.raises(ValueError, match=r"wavelength=0\.0: a field needs a finite wavelength > 0 \(pass it, or the RayBatch that was traced\)"):
        table.field_all(good, monitors=[mon])
    with pytest.raises(ValueError, match=r"wavelength=0\.0: a beam image needs"):
        table.beam_all(good, monitors=[mon])


class _Recorder:
    """Stands in for the engine: keeps what wave_all hands over; `adds` aliased hits a call, into the counter it returns."""

    skipped, adds = 0, 0

    def monitor_wave_many(self, structs, axes, edges, bins, segs, wavelength, amplitude_mode=0, gouy=0, into=None):
        self.structs, self.axes, self.edges, self.bins, self.wavelength, self.into = structs, axes, edges, bins, wavelength, into
        self.amplitude_mode, self.gouy = amplitude_mode, gouy
        shape = (len(structs),) + tuple(bins)
        if into is not None:
            into[4].add_(self.adds)
            return into
        return (torch.zeros(shape, dtype=torch.int64), torch.full(shape, 3.0, dtype=torch.float64), torch.full(shape, -4.0, dtype=torch.float64),
                torch.tensor([self.skipped]), torch.tensor([self.adds]))


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table = oa.OpticalTable()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([1, 2, 3], 0.3, 1.7).RotZ(0.3)]
    segs, rays = support.host_segments(), support.host_rays(4, q=1.5j)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no aliased hit, no warning
        waves = table.wave_all(segs, 780e-7, bins=(7, 5), monitors=mons)
    assert rec.wavelength == 780e-7 and rec.bins == (7, 5) and rec.into is None and (rec.amplitude_mode, rec.gouy) == (0, 0)
    assert rec.edges.shape == (2, 14) and rec.axes.shape == (2, 6)
    for k, (m, f) in enumerate(zip(mons, waves)):
        np.testing.assert_array_equal(rec.edges[k, :8], np.linspace(-m.width / 2, m.width / 2, 8))
        np.testing.assert_array_equal(rec.axes[k], np.concatenate([m.tangent_Y, m.tangent_Z]))
        np.testing.assert_array_equal(f.y_edges, rec.edges[k, :8])
        np.testing.assert_array_equal(f.z_edges, rec.edges[k, 8:])
        assert f.monitor is m and f.bins == (7, 5) and f.counts.dtype == torch.int64 and f.re.dtype == f.im.dtype == torch.float64
        assert f.aliased == 0 and f.field.dtype == torch.complex128 and bool((f.field == complex(3.0, -4.0)).all())
        np.testing.assert_array_equal(f.irradiance().numpy(), 25.0)  # re^2 + im^2
        np.testing.assert_allclose(f.power().numpy(), 25.0 * (m.width / 7) * (m.height / 5), rtol=1e-13)  # times the bin's area
        counts, re, im, ey, ez = f.to_host()
        assert counts.shape == re.shape == im.shape == (7, 5) and ey is f.y_edges and ez is f.z_edges
    table.wave_all(segs, 780e-7, bins=(7, 5), monitors=mons, amplitude="linear", gouy=True)
    assert (rec.amplitude_mode, rec.gouy) == (1, 1)
    # the traced batch: its wavelengths as a double tensor; `into` hands the earlier tensors back
    again = table.wave_all(segs, rays, bins=(7, 5), monitors=mons, into=waves)
    assert again == waves and all(rec.into[k] is waves[0]._stack[k] for k in range(5)) and len(rec.into) == 5
    assert torch.is_tensor(rec.wavelength) and rec.wavelength.dtype == torch.float64 and rec.wavelength.shape == (4,)
    for bad in (waves[:1], waves[::-1]):
        with pytest.raises(ValueError, match="into"):
            table.wave_all(segs, rays, bins=(7, 5), monitors=mons[:len(bad)], into=bad)
    with pytest.raises(ValueError, match="into"):
        table.wave_all(segs, rays, bins=(5, 7), monitors=mons, into=waves)
    foreign = [oa.monitors.MonitorField(m, f.counts, f.re, f.im, f.y_edges, f.z_edges, stack=(f.counts, f.re, f.im, None, k)) for k, (m, f) in enumerate(zip(mons, waves))]
    with pytest.raises(ValueError, match="into"):  # another mode's list is no wave list
        table.wave_all(segs, rays, bins=(7, 5), monitors=mons, into=foreign)
    with pytest.raises(ValueError, match="into"):  # nor is a list put together from two calls
        table.wave_all(segs, rays, bins=(7, 5), monitors=mons, into=[waves[0], table.wave_all(segs, rays, bins=(7, 5), monitors=mons)[1]])
    table.add_monitors(mons[:1])
    assert [f.monitor for f in table.wave_all(segs, rays)] == mons[:1] and rec.bins == (30, 30)
    assert table.wave_batch(mons[1], segs, 780e-7, bins=4, gouy=True).monitor is mons[1] and rec.bins == (4, 4) and rec.gouy == 1
    # aliased hits: one RuntimeWarning that names the count and the remedy; the count comes back, and `into=` accumulates it
    rec.adds = 5
    with pytest.warns(RuntimeWarning, match=r"5 hits are aliased.*smaller monitor or more bins") as caught:
        waves = table.wave_all(segs, rays, bins=(7, 5), monitors=mons)
    assert len(caught) == 1 and all(f.aliased == 5 for f in waves)
    rec.adds = 2
    with pytest.warns(RuntimeWarning, match=r"2 hits are aliased") as caught:
        table.wave_all(segs, rays, bins=(7, 5), monitors=mons, into=waves)
    assert len(caught) == 1 and all(f.aliased == 7 for f in waves)
    rec.adds = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a chunk that adds none says nothing
        table.wave_all(segs, rays, bins=(7, 5), monitors=mons, into=waves)
    assert all(f.aliased == 7 for f in waves)
    # hits the device left out are an error, with their number and the causes
    rec.skipped = 17
    with pytest.raises(ValueError, match=r"17 hits left out.*no q.*wavelength.*index"):
        table.wave_all(segs, rays, monitors=mons)


class _AnyMode:
    """Stands in for the engine in all four image modes: counts the calls, keeps `into` and hands it back, or new tensors of the
    mode's shapes (counts, `planes` images, `tallies` one-element counters)."""

    calls = 0

    def _answer(self, planes, tallies, structs, bins, into):
        self.calls, self.into = self.calls + 1, into
        if into is not None:
            return into
        shape = (len(structs),) + tuple(bins)
        return (torch.zeros(shape, dtype=torch.int64), *(torch.zeros(shape, dtype=torch.float64) for _ in range(planes)),
                *(torch.zeros(1, dtype=torch.int64) for _ in range(tallies)))

    def monitor_image_many(self, structs, axes, edges, bins, segs, into=None):
        return self._answer(1, 0, structs, bins, into)

    def monitor_field_many(self, structs, axes, edges, bins, segs, wavelength, amplitude_mode=0, into=None):
        return self._answer(2, 1, structs, bins, into)

    def monitor_beam_many(self, structs, axes, edges, bins, segs, wavelength, into=None):
        return self._answer(1, 1, structs, bins, into)

    def monitor_wave_many(self, structs, axes, edges, bins, segs, wavelength, amplitude_mode=0, gouy=0, into=None):
        return self._answer(2, 2, structs, bins, into)


def test_into_takes_the_list_of_its_own_mode_only(monkeypatch):
    """Every mode hands the tensors of its own earlier list back to the engine (`_stack` less the position) and refuses the list of
    each other mode with its own words, before the engine is asked."""
    from optable_amd import table as table_module

    rec = _AnyMode()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table = oa.OpticalTable()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([1, 2, 3], 0.3, 1.7).RotZ(0.3)]
    segs = support.host_segments()
    calls = {"image": lambda **kw: table.image_all(segs, bins=(7, 5), monitors=mons, **kw),
             "field": lambda **kw: table.field_all(segs, 780e-7, bins=(7, 5), monitors=mons, **kw),
             "beam": lambda **kw: table.beam_all(segs, 780e-7, bins=(7, 5), monitors=mons, **kw),
             "wave": lambda **kw: table.wave_all(segs, 780e-7, bins=(7, 5), monitors=mons, **kw)}
    lists = {mode: call() for mode, call in calls.items()}
    assert [len(made[0]._stack) for made in lists.values()] == [3, 5, 4, 6] and rec.calls == 4
    for mode, call in calls.items():
        own, asked = lists[mode], rec.calls
        assert call(into=own) == own and rec.calls == asked + 1
        assert len(rec.into) == len(own[0]._stack) - 1 and all(a is b for a, b in zip(rec.into, own[0]._stack))
        assert [f._stack[-1] for f in own] == [0, 1]
        for other, theirs in lists.items():
            if other != mode:
                with pytest.raises(ValueError, match=rf"into: the list an earlier {mode}_all returned for the same monitors and bins"):
                    call(into=theirs)
        assert rec.calls == asked + 1  # none of the refused calls reached the engine


def test_hit_list_accessors_against_the_package_own_ray():
    """The three slots by hand of tests/test_beam_cpu.py (n = 1, 1.5, 1; q before and behind the waist), five hits on them:
    `radiusList` is `Ray.radius_of_curvature(q)`, `gouyList` is arctan2(Re q, Im q) and `amplitudeList` is a sqrt(2 / pi) over
    `Ray.spot_size(t)`, with a float and with the batch's per-ray wavelengths, in either amplitude convention."""
    segs = SegmentBatch(3, "f64", "cpu")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    q = np.array([-2.0 + 1.5j, 0.25 + 0.375j, 3.5 + 40.0j])
    n = np.array([1.0, 1.5, 1.0])
    intensity = np.array([0.81, 0.25, 2.25])
    direction = np.array([[1.0, 0.0, 0.0], [-0.6, 0.8, 0.0], [0.6, 0.0, 0.8]])
    segs.q_re.copy_(torch.from_numpy(q.real.copy()))
    segs.q_im.copy_(torch.from_numpy(q.imag.copy()))
    segs.n_index.copy_(torch.from_numpy(n))
    segs.intensity.copy_(torch.from_numpy(intensity))
    for k, f in enumerate(("dx", "dy", "dz")):
        segs.field(f).copy_(torch.from_numpy(direction[:, k].copy()))
    segs.ray.copy_(torch.tensor([0, 0, 1], dtype=torch.int32))
    segs.n_valid = 3
    slot = torch.tensor([0, 1, 1, 2, 2])
    t = torch.tensor([0.25, 0.7, 1.9, 0.1, 2.5], dtype=torch.float64)
    P = torch.tensor([[0.0, 0.5, 0.1], [0.0, -0.5, 0.2], [0.0, 0.1, 0.3], [0.0, 0.2, -0.4], [0.0, -0.1, 0.0]], dtype=torch.float64)
    hits = MonitorHits(oa.Monitor([1, 0, 0], 2, 2), segs, slot, P, t)
    want_q = q[slot.numpy()] + t.numpy()
    order = hits._order("YZ").numpy()
    assert order.tolist() != list(range(5))

    def ray_of(k, wavelength):
        r = oa.Ray([0, 0, 0], direction[slot[k]], wavelength=wavelength)
        r.qo, r._n = complex(q[slot[k]]), float(n[slot[k]])
        assert r.q_at_z(float(t[k])) == want_q[k]
        return r

    def expected(wavelengths):
        rays = [ray_of(k, wavelengths[k]) for k in range(5)]
        radius = np.array([r.radius_of_curvature(r.q_at_z(float(t[k]))) for k, r in enumerate(rays)])
        spot = np.array([r.spot_size(float(t[k])) for k, r in enumerate(rays)])
        return radius, spot

    wl = 0.4375
    radius, spot = expected([wl] * 5)
    assert (radius > 0).any() and (radius < 0).any()  # behind and before the waist
    np.testing.assert_allclose(hits.radiusList(None).numpy(), radius, rtol=1e-14)
    np.testing.assert_allclose(hits.radiusList().numpy(), radius[order], rtol=1e-14)
    np.testing.assert_allclose(hits.radiusList("ID").numpy(), radius, rtol=1e-14)
    np.testing.assert_allclose(hits.gouyList(None).numpy(), np.arctan2(want_q.real, want_q.imag), rtol=1e-15)
    np.testing.assert_allclose(hits.gouyList().numpy(), np.arctan2(want_q.real, want_q.imag)[order], rtol=1e-15)
    I = intensity[slot.numpy()]
    np.testing.assert_allclose(hits.amplitudeList(wl, None).numpy(), np.sqrt(I) * np.sqrt(2 / np.pi) / spot, rtol=1e-14)
    np.testing.assert_allclose(hits.amplitudeList(wl, None, amplitude="linear").numpy(), I * np.sqrt(2 / np.pi) / spot, rtol=1e-14)
    np.testing.assert_allclose(hits.amplitudeList(wl).numpy(), (np.sqrt(I) * np.sqrt(2 / np.pi) / spot)[order], rtol=1e-14)
    with pytest.raises(ValueError, match="amplitude"):
        hits.amplitudeList(wl, None, amplitude="power")
    rays = RayBatch.from_arrays(np.zeros((2, 3)), np.tile([1.0, 0, 0], (2, 1)), wavelength=np.array([0.4375, 0.3125]), device="cpu")
    _, spot = expected([0.4375, 0.4375, 0.4375, 0.3125, 0.3125])
    np.testing.assert_allclose(hits.amplitudeList(rays, None).numpy(), np.sqrt(I) * np.sqrt(2 / np.pi) / spot, rtol=1e-14)
    # the integral of |u|^2 over the plane is a^2: the peak is a sqrt(2 / pi) / w
    np.testing.assert_allclose((hits.amplitudeList(rays, None).numpy() * spot) ** 2 * np.pi / 2, I, rtol=1e-14)


def test_the_wave_kernel_and_the_count_kernel_keep_four_waves_per_simd(kernels):  # noqa: F811
    """k_mon_wave is a kernel of its own: on gfx950 up to 128 registers are four waves per SIMD, and it stays there — exp and
    sincospi as calls — without scratch memory or a spilled vector register; k_mon_count is what it was."""
    wave = [k for k in kernels if re.match(r"_Z\d+k_mon_wave", k["name"])]
    assert len(wave) == 1
    k = wave[0]
    assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert len(k["args"]) >= 9 and "MonWave" in k["name"] and "beam" not in k["name"]
    count = [k for k in kernels if re.match(r"_Z\d+k_mon_count", k["name"])]
    assert len(count) == 1 and count[0]["vgpr"] <= 128 and count[0]["scratch"] == 0 and count[0]["vgpr_spill"] == 0, count
