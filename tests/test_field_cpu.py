"""CPU: the public surface of coherent detector images (`OpticalTable.field_all` / `field_batch`: the phasors of every monitor's
hits summed per bin on the device, ot_monitor_field_many) — the calls and the binding, the LDS budget and the plan of passes,
what is refused before the engine is asked, and the hit-list form of the same quantity (`MonitorHits.pathlengthList` /
`phaseList`) against the package's own `Ray`.  No library call is made."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calls_exist():
    from optable_amd import engine, monitors

    assert callable(oa.OpticalTable.field_all) and callable(oa.OpticalTable.field_batch)
    assert callable(Engine.monitor_field_many) and callable(engine.field_plan)
    assert callable(monitors.MonitorField.to_host) and callable(monitors.MonitorField.intensity)
    assert callable(MonitorHits.pathlengthList) and callable(MonitorHits.phaseList)
    assert "ot_monitor_field_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_field_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_field_many is not declared in the header"
    restype, argtypes = abi.SYMBOLS["ot_monitor_field_many"]
    assert len(argtypes) == len(decl.group(1).split(",")) == 23
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)


def test_budget_and_pass_planner():
    from optable_amd import engine

    text = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bMON_FIELD_LDS_BINS\s*=\s*([^;]+);", text)
    assert found
    # 64 KB of LDS a workgroup, less the 128-byte tally of the record mode, at 20 bytes a bin (re, im, count)
    assert eval(found.group(1).replace("/", "//"), {"MON_MAX": 32}) == engine.FIELD_LDS_BINS == 3270
    plan = engine.field_plan
    assert plan(1, 30, 30) == {"path": "lds", "per_pass": 1, "passes": 1}
    assert plan(3, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 1}      # 2,700 bins
    assert plan(4, 30, 30) == {"path": "lds", "per_pass": 2, "passes": 2}      # as even as they come: 2 + 2, not 3 + 1
    assert plan(8, 30, 30) == {"path": "lds", "per_pass": 3, "passes": 3}
    assert plan(1, 3270, 1)["path"] == "lds" and plan(1, 3271, 1)["path"] == "global"  # just over the budget
    assert plan(3, 80, 80) == {"path": "global", "per_pass": 3, "passes": 1}
    assert engine.image_plan(6, 30, 30) == {"path": "lds", "per_pass": 6, "passes": 1}  # the incoherent image keeps its own budget
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
    good, rays = support.host_segments(), support.host_rays(4)
    with pytest.raises(ValueError, match="double-precision"):
        table.field_all(support.host_segments(precision="f32"), 780e-7, monitors=[mon])
    with pytest.raises(ValueError, match=r"wavelength=0\.0"):
        table.field_all(good, monitors=[mon])  # the default
    for bad in (0.0, -780e-7, float("nan"), float("inf"), "red", None):
        with pytest.raises(ValueError, match="wavelength"):
            table.field_all(good, bad, monitors=[mon])
        with pytest.raises(ValueError, match="wavelength"):
            table.field_batch(mon, good, bad)
    with pytest.raises(ValueError, match="RayBatch of 5 rays"):
        table.field_all(good, support.host_rays(5), monitors=[mon])
    for value in (0.0, -1.0, float("nan"), float("inf")):
        dark = support.host_rays(4)
        dark.wavelength[2] = value
        with pytest.raises(ValueError, match="finite wavelength > 0"):
            table.field_all(good, dark, monitors=[mon])
    for amplitude in ("power", "", None, 0):
        with pytest.raises(ValueError, match="amplitude"):
            table.field_all(good, rays, monitors=[mon], amplitude=amplitude)
    for bins in (0, -3, (30, 0), (30,), 2.5, "30", None, True):
        with pytest.raises(ValueError, match="bins"):
            table.field_all(good, rays, bins=bins, monitors=[mon])
        with pytest.raises(ValueError, match="bins"):
            table.field_batch(mon, good, rays, bins=bins)
    with pytest.raises(AssertionError, match="the engine was asked for"):  # ... and what is good gets that far
        table.field_all(good, rays, bins=(7, 5), monitors=[mon], amplitude="linear")


class _Recorder:
    """Stands in for the engine: keeps what field_all hands over."""

    skipped = 0

    def monitor_field_many(self, structs, axes, edges, bins, segs, wavelength, amplitude_mode=0, into=None):
        self.structs, self.axes, self.edges, self.bins, self.wavelength, self.mode, self.into = structs, axes, edges, bins, wavelength, amplitude_mode, into
        shape = (len(structs),) + tuple(bins)
        return (torch.zeros(shape, dtype=torch.int64), torch.ones(shape, dtype=torch.float64), torch.full(shape, 2.0, dtype=torch.float64),
                torch.tensor([self.skipped]))


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table = oa.OpticalTable()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([1, 2, 3], 0.3, 1.7).RotZ(0.3)]
    segs, rays = support.host_segments(), support.host_rays(4)
    fields = table.field_all(segs, 780e-7, bins=(7, 5), monitors=mons)
    assert rec.wavelength == 780e-7 and rec.mode == 0 and rec.bins == (7, 5) and rec.into is None
    assert rec.edges.shape == (2, 14) and rec.axes.shape == (2, 6)
    for k, (m, f) in enumerate(zip(mons, fields)):
        np.testing.assert_array_equal(rec.edges[k, :8], np.linspace(-m.width / 2, m.width / 2, 8))
        np.testing.assert_array_equal(rec.axes[k], np.concatenate([m.tangent_Y, m.tangent_Z]))
        np.testing.assert_array_equal(f.y_edges, rec.edges[k, :8])
        np.testing.assert_array_equal(f.z_edges, rec.edges[k, 8:])
        assert f.monitor is m and f.bins == (7, 5) and f.counts.dtype == torch.int64
        assert f.field.dtype == torch.complex128 and bool((f.field == 1 + 2j).all()) and bool((f.intensity() == 5.0).all())
        counts, re, im, ey, ez = f.to_host()
        assert counts.shape == re.shape == im.shape == (7, 5) and ey is f.y_edges and ez is f.z_edges
    # the traced batch: its wavelengths as a double tensor; "linear" is mode 1; `into` hands the earlier tensors back
    again = table.field_all(segs, rays, bins=(7, 5), monitors=mons, into=fields, amplitude="linear")
    assert again == fields and rec.mode == 1 and rec.into[0] is fields[0]._stack[0] and len(rec.into) == 4
    assert torch.is_tensor(rec.wavelength) and rec.wavelength.dtype == torch.float64 and rec.wavelength.shape == (4,)
    for bad in (fields[:1], fields[::-1]):
        with pytest.raises(ValueError, match="into"):
            table.field_all(segs, rays, bins=(7, 5), monitors=mons[:len(bad)], into=bad)
    with pytest.raises(ValueError, match="into"):
        table.field_all(segs, rays, bins=(5, 7), monitors=mons, into=fields)
    table.add_monitors(mons[:1])
    assert [f.monitor for f in table.field_all(segs, rays)] == mons[:1] and rec.bins == (30, 30)
    assert table.field_batch(mons[1], segs, 780e-7, bins=4, amplitude="linear").monitor is mons[1] and rec.bins == (4, 4) and rec.mode == 1
    # hits the device left out are an error, with their number
    rec.skipped = 17
    with pytest.raises(ValueError, match="17 hits"):
        table.field_all(segs, rays, monitors=mons)


def test_hit_list_accessors_against_the_package_own_ray():
    """Three slots by hand (n = 1, 1.5, 1), five hits on them: `pathlengthList` is pathlength + t n exactly, `phaseList` is
    `Ray.phase(t)` to 1e-12 rad — with a float and with the batch's per-ray wavelengths."""
    segs = SegmentBatch(3, "f64", "cpu")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    pl, n = np.array([0.0, 2.75, 3.125 + 2.0**-20]), np.array([1.0, 1.5, 1.0])
    segs.pathlength.copy_(torch.from_numpy(pl))
    segs.n_index.copy_(torch.from_numpy(n))
    segs.ray.copy_(torch.tensor([0, 0, 1], dtype=torch.int32))
    segs.n_valid = 3
    assert segs.layout == "list"
    slot = torch.tensor([0, 1, 1, 2, 2])
    t = torch.tensor([0.25, 0.7, 1.9, 0.1, 2.5], dtype=torch.float64)
    P = torch.tensor([[0.0, 0.5, 0.1], [0.0, -0.5, 0.2], [0.0, 0.1, 0.3], [0.0, 0.2, -0.4], [0.0, -0.1, 0.0]], dtype=torch.float64)
    hits = MonitorHits(oa.Monitor([1, 0, 0], 2, 2), segs, slot, P, t)
    assert hits.slot.tolist() == slot.tolist()  # (already in reference order: ray-major, stable)
    want = pl[slot.numpy()] + t.numpy() * n[slot.numpy()]
    np.testing.assert_array_equal(hits.pathlengthList(None).numpy(), want)
    order = hits._order("YZ").numpy()
    assert order.tolist() != list(range(5))
    np.testing.assert_array_equal(hits.pathlengthList().numpy(), want[order])
    np.testing.assert_array_equal(hits.pathlengthList("ID").numpy(), want)

    def ray_phase(k, wavelength):
        r = oa.Ray([0, 0, 0], [1, 0, 0], wavelength=wavelength)
        r._n, r._pathlength = float(n[slot[k]]), float(pl[slot[k]])
        assert r.pathlength(float(t[k])) == want[k]
        return r.phase(float(t[k]))

    wl = 0.4375
    got = hits.phaseList(wl, None).numpy()
    assert np.all((got >= 0) & (got < 2 * np.pi)) and len(set(np.round(got, 6))) == 5
    np.testing.assert_allclose(got, [ray_phase(k, wl) for k in range(5)], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(hits.phaseList(wl).numpy(), got[order])
    rays = RayBatch.from_arrays(np.zeros((2, 3)), np.tile([1.0, 0, 0], (2, 1)), wavelength=np.array([0.4375, 0.3125]), device="cpu")
    per_ray = [0.4375, 0.4375, 0.4375, 0.3125, 0.3125]
    np.testing.assert_allclose(hits.phaseList(rays, None).numpy(), [ray_phase(k, per_ray[k]) for k in range(5)], rtol=0, atol=1e-12)
    np.testing.assert_allclose(hits.phaseList(rays).numpy(), np.array([ray_phase(k, per_ray[k]) for k in range(5)])[order], rtol=0, atol=1e-12)
