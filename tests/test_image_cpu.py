"""CPU: the public surface of detector images (`OpticalTable.image_all` / `image_batch`: the hits of every monitor binned on
the device, ot_monitor_image_many) — the calls and the binding, the validation of `bins`, the edge tables handed to the library
and the plan of passes.  No library call is made."""
import os
import re

import numpy as np
import pytest

import optable_amd as oa
from optable_amd import abi
from optable_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calls_exist():
    from optable_amd import engine, monitors

    assert callable(oa.OpticalTable.image_all) and callable(oa.OpticalTable.image_batch)
    assert callable(Engine.monitor_image_many) and callable(engine.image_plan)
    assert callable(monitors.MonitorImage.to_host)
    assert "ot_monitor_image_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_image_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_image_many is not declared in the header"
    restype, argtypes = abi.SYMBOLS["ot_monitor_image_many"]
    assert len(argtypes) == len(decl.group(1).split(",")) == 15
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)


@pytest.mark.parametrize("bins", [0, -3, (30, 0), (0, 30), (30,), (3, 4, 5), 2.5, (30, 2.0), "30", None, True, (True, 3)])
def test_bad_bins_are_refused_before_any_device_work(bins, monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table = oa.OpticalTable()
    mon = oa.Monitor([1, 0, 0], 2, 2)
    with pytest.raises(ValueError):
        table.image_all(None, bins=bins, monitors=[mon])
    with pytest.raises(ValueError):
        table.image_batch(mon, None, bins=bins)


def test_good_bins():
    from optable_amd.monitors import image_bins

    assert image_bins(30) == (30, 30) and image_bins((7, 5)) == (7, 5) and image_bins([30, 1]) == (30, 1)
    assert image_bins(np.int64(4)) == (4, 4) and image_bins((np.int32(2), 3)) == (2, 3)


class _Recorder:
    """Stands in for the engine: keeps what image_all hands over."""

    def monitor_image_many(self, structs, axes, edges, bins, segs, into=None):
        self.structs, self.axes, self.edges, self.bins, self.into = structs, axes, edges, bins, into
        import torch

        return torch.zeros((len(structs),) + tuple(bins), dtype=torch.int64), torch.zeros((len(structs),) + tuple(bins), dtype=torch.float64)


def test_edges_and_axes_handed_over(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table = oa.OpticalTable()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([7.5, 0, 0], 0.4, 6).RotX(0.5), oa.Monitor([1, 2, 3], 0.3, 1.7).RotZ(0.3)]
    for nby, nbz in ((30, 30), (7, 5), (30, 1), (80, 80)):
        images = table.image_all(None, bins=(nby, nbz), monitors=mons)
        assert rec.bins == (nby, nbz) and rec.edges.shape == (3, nby + nbz + 2) and rec.axes.shape == (3, 6) and rec.into is None
        assert rec.edges.dtype == np.float64 and rec.axes.dtype == np.float64
        for k, (m, im) in enumerate(zip(mons, images)):
            ey, ez = rec.edges[k, :nby + 1], rec.edges[k, nby + 1:]
            np.testing.assert_array_equal(ey, np.linspace(-m.width / 2, m.width / 2, nby + 1))
            np.testing.assert_array_equal(ez, np.linspace(-m.height / 2, m.height / 2, nbz + 1))
            np.testing.assert_array_equal(ey, np.histogram_bin_edges([], nby, (-m.width / 2, m.width / 2)))
            np.testing.assert_array_equal(ez, np.histogram_bin_edges([], nbz, (-m.height / 2, m.height / 2)))
            np.testing.assert_array_equal(im.y_edges, ey)
            np.testing.assert_array_equal(im.z_edges, ez)
            np.testing.assert_array_equal(rec.axes[k], np.concatenate([m.tangent_Y, m.tangent_Z]))  # the LAB tangents of yList / zList
            assert im.monitor is m and im.bins == (nby, nbz) and im.counts.dtype.is_floating_point is False
    # `into`: the earlier call's tensors go back to the engine, and the same list comes back
    again = table.image_all(None, bins=(80, 80), monitors=mons, into=images)
    assert again == images and rec.into[0] is images[0]._stack[0] and rec.into[1] is images[0]._stack[1]
    for bad in (images[:2], images[::-1]):
        with pytest.raises(ValueError):
            table.image_all(None, bins=(80, 80), monitors=mons[:len(bad)], into=bad)
    with pytest.raises(ValueError):
        table.image_all(None, bins=(7, 5), monitors=mons, into=images)  # other bins
    # the table's own monitors, one image
    table.add_monitors(mons[:2])
    assert [im.monitor for im in table.image_all(None)] == mons[:2] and rec.bins == (30, 30)
    assert table.image_batch(mons[2], None, bins=4).monitor is mons[2] and rec.bins == (4, 4) and len(rec.structs) == 1


def _constant(name, text):
    found = re.search(rf"\b{name}\s*=\s*([^;]+);", text)
    assert found, name
    return eval(found.group(1).replace("/", "//"), {"MON_MAX": 32})  # (plain integer arithmetic)


def test_pass_planner():
    from optable_amd import engine

    # the budget is the library's own: 64 KB of LDS a workgroup, less the 128-byte tally of the record mode, at 12 bytes a bin
    text = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    assert _constant("MON_MAX", text) == engine.IMAGE_MAX_MONITORS == 32
    assert _constant("MON_IMG_LDS_BINS", text) == engine.IMAGE_LDS_BINS == 5450
    assert _constant("MON_IMG_MAX_BINS", text) == engine.IMAGE_MAX_BINS == 1 << 24
    plan = engine.image_plan
    assert plan(1, 30, 30) == {"path": "lds", "per_pass": 1, "passes": 1}
    assert plan(6, 30, 30) == {"path": "lds", "per_pass": 6, "passes": 1}      # 5,400 bins
    assert plan(7, 30, 30) == {"path": "lds", "per_pass": 4, "passes": 2}      # several at a time, as even as they come
    assert plan(8, 30, 30) == {"path": "lds", "per_pass": 4, "passes": 2}
    assert plan(32, 30, 30) == {"path": "lds", "per_pass": 6, "passes": 6}
    assert plan(1, 5450, 1)["path"] == "lds" and plan(1, 1, 5451)["path"] == "global"  # just over the budget
    assert plan(3, 80, 80) == {"path": "global", "per_pass": 3, "passes": 1}
    assert plan(33, 7, 5) == {"path": "lds", "per_pass": 17, "passes": 2}     # 35 bins each: the 32 monitors of a launch decide
    assert plan(33, 80, 80) == {"path": "global", "per_pass": 17, "passes": 2}
    for n, nby, nbz in ((0, 3, 3), (1, 0, 3), (1, 3, 0), (1, 1 << 12, (1 << 12) + 1)):
        with pytest.raises(ValueError):
            plan(n, nby, nbz)
