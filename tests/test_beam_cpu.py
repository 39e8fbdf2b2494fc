"""CPU: the public surface of Gaussian-beam detector images (`OpticalTable.beam_all` / `beam_batch`: every monitor hit spread over
its spot size on the device, ot_monitor_beam_many) — the calls and the binding, the LDS budget and the plan of passes, what is
refused before the engine is asked, what is handed over and what comes back, the hit-list form of the same quantities
(`MonitorHits.qList` / `spotsizeList` / `waistList` / `waistdistanceList`) against the package's own `Ray`, and the registers of the
kernel the mode lives in.  No library call is made."""
import os
import re

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

    assert callable(oa.OpticalTable.beam_all) and callable(oa.OpticalTable.beam_batch)
    assert callable(Engine.monitor_beam_many) and callable(engine.beam_plan)
    assert callable(monitors.MonitorBeam.to_host) and callable(monitors.MonitorBeam.irradiance)
    for accessor in ("qList", "spotsizeList", "waistList", "waistdistanceList"):
        assert callable(getattr(MonitorHits, accessor))
    assert "ot_monitor_beam_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_beam_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_beam_many is not declared in the header"
    declared = [a.strip() for a in decl.group(1).split(",")]
    restype, argtypes = abi.SYMBOLS["ot_monitor_beam_many"]
    assert len(argtypes) == len(declared) == 22
    # ot_monitor_field_many's list with q_re, q_im for pathlength and re, im -> power, and no amplitude_mode
    names = [a.split()[-1].lstrip("*") for a in declared]
    assert names == ["ctx", "mons", "n_monitors", "axes", "edges", "nby", "nbz", "src", "intensity", "q_re", "q_im", "n_index", "wavelength",
                     "n_wavelengths", "wavelength_uniform", "n_segments", "seg_count", "n_rays", "counts", "power", "skipped", "accumulate"]
    import ctypes as C

    for name, kind in zip(names, argtypes):  # pointers as pointers, the integers by their width, the one double
        want = {"n_monitors": C.c_int32, "nby": C.c_int32, "nbz": C.c_int32, "accumulate": C.c_int32, "n_wavelengths": C.c_int64,
                "n_segments": C.c_int64, "n_rays": C.c_int64, "wavelength_uniform": C.c_double}.get(name)
        assert kind is want if want else kind not in (C.c_int32, C.c_int64, C.c_double), name
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)


def test_budget_and_pass_planner():
    from optable_amd import engine

    text = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bMON_BEAM_LDS_BINS\s*=\s*([^;]+);", text)
    assert found
    # 64 KB of LDS a workgroup, less the 128-byte tally of the record mode and four waves' strips of 128 doubles, at 12 bytes a bin
    assert eval(found.group(1).replace("/", "//"), {"MON_MAX": 32, "MON_WAVES": 4, "MON_BEAM_STRIP": 128}) == engine.BEAM_LDS_BINS == 5109
    assert engine.BEAM_LDS_BINS < engine.IMAGE_LDS_BINS
    plan = engine.beam_plan
    assert plan(1, 30, 30) == {"path": "lds", "per_pass": 1, "passes": 1}
    assert plan(5, 30, 30) == {"path": "lds", "per_pass": 5, "passes": 1}      # 4,500 bins
    assert plan(6, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 2}      # as even as they come: 3 + 3, not 5 + 1
    assert plan(8, 30, 30) == {"path": "lds", "per_pass": 4, "passes": 2}
    assert plan(1, 5109, 1)["path"] == "lds" and plan(1, 5110, 1)["path"] == "global"  # just over the budget
    assert plan(3, 80, 80) == {"path": "global", "per_pass": 3, "passes": 1}
    assert plan(40, 80, 80) == {"path": "global", "per_pass": 20, "passes": 2}
    assert engine.image_plan(6, 30, 30) == {"path": "lds", "per_pass": 6, "passes": 1}  # the point image keeps its own budget
    assert engine.field_plan(6, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 2}
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
    with pytest.raises(ValueError, match=r"wavelength=0\.0: a beam image needs"):
        table.beam_all(good, monitors=[mon])  # the default
    for bad in (0.0, -780e-7, float("nan"), float("inf"), "red", None):
        with pytest.raises(ValueError, match="wavelength"):
            table.beam_all(good, bad, monitors=[mon])
        with pytest.raises(ValueError, match="wavelength"):
            table.beam_batch(mon, good, bad)
    with pytest.raises(ValueError, match="RayBatch of 5 rays"):
        table.beam_all(good, support.host_rays(5, q=1.5j), monitors=[mon])
    for value in (0.0, -1.0, float("nan"), float("inf")):
        dark = support.host_rays(4, q=1.5j)
        dark.wavelength[2] = value
        with pytest.raises(ValueError, match="finite wavelength > 0"):
            table.beam_all(good, dark, monitors=[mon])
    for bins in (0, -3, (30, 0), (30,), 2.5, "30", None, True):
        with pytest.raises(ValueError, match="bins"):
            table.beam_all(good, rays, bins=bins, monitors=[mon])
        with pytest.raises(ValueError, match="bins"):
            table.beam_batch(mon, good, rays, bins=bins)
    # ... and what is good gets that far, single-precision segments included: a spot size is not phase-sensitive
    for segs in (good, support.host_segments(precision="f32")):
        with pytest.raises(AssertionError, match="the engine was asked for"):
            table.beam_all(segs, rays, bins=(7, 5), monitors=[mon])
    # field_all's own words are what they were
    with pytest.raises(ValueError, match=r"wavelength=0\.0: a field needs a finite wavelength > 0 \(pass it, or the RayBatch that was traced\)"):
        table.field_all(good, monitors=[mon])
    with pytest.raises(ValueError, match="wavelength must be a float or the RayBatch that was traced, not 'red'"):
        table.field_all(good, "red", monitors=[mon])


class _Recorder:
    """Stands in for the engine: keeps what beam_all hands over."""

    skipped = 0

    def monitor_beam_many(self, structs, axes, edges, bins, segs, wavelength, into=None):
        self.structs, self.axes, self.edges, self.bins, self.wavelength, self.into = structs, axes, edges, bins, wavelength, into
        shape = (len(structs),) + tuple(bins)
        return torch.zeros(shape, dtype=torch.int64), torch.full(shape, 3.0, dtype=torch.float64), torch.tensor([self.skipped])


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table = oa.OpticalTable()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([1, 2, 3], 0.3, 1.7).RotZ(0.3)]
    segs, rays = support.host_segments(), support.host_rays(4, q=1.5j)
    beams = table.beam_all(segs, 780e-7, bins=(7, 5), monitors=mons)
    assert rec.wavelength == 780e-7 and rec.bins == (7, 5) and rec.into is None
    assert rec.edges.shape == (2, 14) and rec.axes.shape == (2, 6)
    for k, (m, b) in enumerate(zip(mons, beams)):
        np.testing.assert_array_equal(rec.edges[k, :8], np.linspace(-m.width / 2, m.width / 2, 8))
        np.testing.assert_array_equal(rec.axes[k], np.concatenate([m.tangent_Y, m.tangent_Z]))
        np.testing.assert_array_equal(b.y_edges, rec.edges[k, :8])
        np.testing.assert_array_equal(b.z_edges, rec.edges[k, 8:])
        assert b.monitor is m and b.bins == (7, 5) and b.counts.dtype == torch.int64 and b.power.dtype == torch.float64
        area = (m.width / 7) * (m.height / 5)
        np.testing.assert_allclose(b.irradiance().numpy(), 3.0 / area, rtol=1e-13)  # power over the bin's area
        counts, power, ey, ez = b.to_host()
        assert counts.shape == power.shape == (7, 5) and ey is b.y_edges and ez is b.z_edges
    # the traced batch: its wavelengths as a double tensor; `into` hands the earlier tensors back
    again = table.beam_all(segs, rays, bins=(7, 5), monitors=mons, into=beams)
    assert again == beams and rec.into[0] is beams[0]._stack[0] and rec.into[1] is beams[0]._stack[1] and len(rec.into) == 3
    assert torch.is_tensor(rec.wavelength) and rec.wavelength.dtype == torch.float64 and rec.wavelength.shape == (4,)
    for bad in (beams[:1], beams[::-1]):
        with pytest.raises(ValueError, match="into"):
            table.beam_all(segs, rays, bins=(7, 5), monitors=mons[:len(bad)], into=bad)
    with pytest.raises(ValueError, match="into"):
        table.beam_all(segs, rays, bins=(5, 7), monitors=mons, into=beams)
    with pytest.raises(ValueError, match="into"):  # another mode's list is no beam list
        table.beam_all(segs, rays, bins=(7, 5), monitors=mons, into=[oa.monitors.MonitorImage(m, b.counts, b.power, b.y_edges, b.z_edges) for m, b in zip(mons, beams)])
    table.add_monitors(mons[:1])
    assert [b.monitor for b in table.beam_all(segs, rays)] == mons[:1] and rec.bins == (30, 30)
    assert table.beam_batch(mons[1], segs, 780e-7, bins=4).monitor is mons[1] and rec.bins == (4, 4)
    # hits the device left out are an error, with their number and the causes
    rec.skipped = 17
    with pytest.raises(ValueError, match=r"17 hits left out.*no q.*wavelength.*index"):
        table.beam_all(segs, rays, monitors=mons)


def test_hit_list_accessors_against_the_package_own_ray():
    """Three slots by hand (n = 1, 1.5, 1; q before and behind the waist), five hits on them: `qList` is q + t exactly, `spotsizeList`
    is `Ray.spot_size(t)`, `waistList` is `Ray.waist(q)` and `waistdistanceList` is `Monitor.get_waist_distance`'s value, sign rule
    included, to a few ulp — with a float and with the batch's per-ray wavelengths."""
    segs = SegmentBatch(3, "f64", "cpu")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    q = np.array([-2.0 + 1.5j, 0.25 + 0.375j, 3.5 + 40.0j])
    n = np.array([1.0, 1.5, 1.0])
    direction = np.array([[1.0, 0.0, 0.0], [-0.6, 0.8, 0.0], [0.6, 0.0, 0.8]])
    segs.q_re.copy_(torch.from_numpy(q.real.copy()))
    segs.q_im.copy_(torch.from_numpy(q.imag.copy()))
    segs.n_index.copy_(torch.from_numpy(n))
    for k, f in enumerate(("dx", "dy", "dz")):
        segs.field(f).copy_(torch.from_numpy(direction[:, k].copy()))
    segs.ray.copy_(torch.tensor([0, 0, 1], dtype=torch.int32))
    segs.n_valid = 3
    slot = torch.tensor([0, 1, 1, 2, 2])
    t = torch.tensor([0.25, 0.7, 1.9, 0.1, 2.5], dtype=torch.float64)
    P = torch.tensor([[0.0, 0.5, 0.1], [0.0, -0.5, 0.2], [0.0, 0.1, 0.3], [0.0, 0.2, -0.4], [0.0, -0.1, 0.0]], dtype=torch.float64)
    mon = oa.Monitor([1, 0, 0], 2, 2)
    hits = MonitorHits(mon, segs, slot, P, t)
    assert hits.slot.tolist() == slot.tolist()
    want_q = q[slot.numpy()] + t.numpy()
    assert hits.qList(None).dtype == torch.complex128
    np.testing.assert_array_equal(hits.qList(None).numpy(), want_q)
    order = hits._order("YZ").numpy()
    assert order.tolist() != list(range(5))
    np.testing.assert_array_equal(hits.qList().numpy(), want_q[order])
    np.testing.assert_array_equal(hits.qList("ID").numpy(), want_q)

    def ray_of(k, wavelength):
        r = oa.Ray([0, 0, 0], direction[slot[k]], wavelength=wavelength)
        r.qo, r._n = complex(q[slot[k]]), float(n[slot[k]])
        assert r.n == n[slot[k]] and r.q_at_z(float(t[k])) == want_q[k]
        return r

    def expected(wavelengths):
        rays = [ray_of(k, wavelengths[k]) for k in range(5)]
        spot = [r.spot_size(float(t[k])) for k, r in enumerate(rays)]
        waist = [r.waist(r.q_at_z(float(t[k]))) for k, r in enumerate(rays)]
        dist = []
        for k, r in enumerate(rays):  # Monitor.get_waist_distance
            z = r.distance_to_waist(r.q_at_z(float(t[k])))
            dist.append(-z if np.dot(r.direction, mon.normal) > 0 else z)
        return np.array(spot), np.array(waist), np.array(dist)

    wl = 0.4375
    spot, waist, dist = expected([wl] * 5)
    assert len(set(np.round(spot, 9))) == 5 and (dist > 0).any() and (dist < 0).any()
    assert np.sign(dist).tolist() != np.sign(want_q.real).tolist()  # the sign rule turned some
    np.testing.assert_allclose(hits.spotsizeList(wl, None).numpy(), spot, rtol=1e-14)
    np.testing.assert_allclose(hits.waistList(wl, None).numpy(), waist, rtol=1e-14)
    np.testing.assert_array_equal(hits.waistdistanceList(None).numpy(), dist)
    np.testing.assert_allclose(hits.spotsizeList(wl).numpy(), spot[order], rtol=1e-14)
    np.testing.assert_array_equal(hits.waistdistanceList().numpy(), dist[order])
    rays = RayBatch.from_arrays(np.zeros((2, 3)), np.tile([1.0, 0, 0], (2, 1)), wavelength=np.array([0.4375, 0.3125]), device="cpu")
    spot, waist, _ = expected([0.4375, 0.4375, 0.4375, 0.3125, 0.3125])
    np.testing.assert_allclose(hits.spotsizeList(rays, None).numpy(), spot, rtol=1e-14)
    np.testing.assert_allclose(hits.waistList(rays, None).numpy(), waist, rtol=1e-14)
    np.testing.assert_allclose(hits.waistList(rays).numpy(), waist[order], rtol=1e-14)


def test_the_beam_mode_costs_the_count_kernel_no_occupancy(kernels):  # noqa: F811
    """The beam pass is a mode of k_mon_count, not a kernel: on gfx950 up to 128 registers are four waves per SIMD, and a pass that
    calls erf stays there without scratch memory or a spilled vector register."""
    count = [k for k in kernels if re.match(r"_Z\d+k_mon_count", k["name"])]
    assert len(count) == 1
    k = count[0]
    assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert len(k["args"]) >= 11  # ... and it takes the three trailing structs
    assert not [k["name"] for k in kernels if "beam" in k["name"]]  # (its argument type MonBeam apart, which the mangled name spells out)
