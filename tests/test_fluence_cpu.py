"""CPU: the public surface of fluence maps (`OpticalTable.fluence_map`: a SegmentBatch rasterised into a projected view on the
device, ot_fluence_map) — the calls and the binding, what is refused before the engine is asked, what is handed over and what
comes back, the planner and its constants, the numpy reference of the GPU tests against closed forms, and the two kernels the
one-monitor record call no longer needs.  No library call is made."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import optable_amd as oa
from fluence_reference import U, fluence_reference
import support
from optable_amd import abi
from optable_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(3)


def test_the_calls_exist():
    from optable_amd import engine, fluence

    assert callable(oa.OpticalTable.fluence_map) and callable(Engine.fluence_map) and callable(engine.fluence_plan)
    assert oa.FluenceMap is fluence.FluenceMap and callable(fluence.FluenceMap.to_host)
    for name in ("pixels", "skipped", "extent"):
        assert isinstance(getattr(fluence.FluenceMap, name), property)
    assert "ot_fluence_map" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_fluence_map\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_fluence_map is not declared in the header"
    names = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "axes", "u_edges", "nu", "v_edges", "nv", "w_lo", "w_hi", "src", "intensity", "n_segments", "seg_count", "n_rays",
                     "counts", "fluence", "skipped", "accumulate"]
    restype, argtypes = abi.SYMBOLS["ot_fluence_map"]
    assert restype is C.c_int and len(argtypes) == len(names) == 17
    widths = {"nu": C.c_int32, "nv": C.c_int32, "accumulate": C.c_int32, "n_segments": C.c_int64, "n_rays": C.c_int64, "w_lo": C.c_double,
              "w_hi": C.c_double}
    for name, kind in zip(names, argtypes):  # pointers as pointers, the integers by their width, the two doubles
        assert kind is widths[name] if name in widths else kind not in (C.c_int32, C.c_int64, C.c_double), name
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)


def test_planner_and_its_constants():
    from optable_amd import engine

    text = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bSEG_RASTER_MAX_PIXELS\s*=\s*([^;]+);", text)
    assert found and eval(found.group(1)) == engine.FLUENCE_MAX_PIXELS == 1 << 24
    assert engine.fluence_plan(73, 74) == {"path": "lds"}      # 5,402 pixels
    assert engine.fluence_plan(74, 74) == {"path": "global"}   # 5,476 pixels; the budget is 5,450
    assert engine.fluence_plan(5450, 1)["path"] == "lds" and engine.fluence_plan(1, 5451)["path"] == "global"
    assert engine.fluence_plan(1 << 12, 1 << 12)["path"] == "global"
    for nu, nv in ((0, 3), (3, 0), (-1, 5), (1 << 12, (1 << 12) + 1)):
        with pytest.raises(ValueError):
            engine.fluence_plan(nu, nv)


ROI = (-1.0, 9.0, -3.01, 2.97, -0.5, float("inf"))


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table, segs = oa.OpticalTable(), support.host_segments()
    for view in ("z", "3D", "XY", 2, None, ""):
        with pytest.raises(ValueError, match="view"):
            table.fluence_map(segs, view=view, roi=ROI)
    for roi in ((0, 1, 0, 1), (0, 1, 0, 1, 0, 1, 0), "roi", 7, (0, 1, 0, 1, 0, "deep"), (0, 1, 0, None, 0, 1),
                (1, 0, 0, 1, 0, 1), (0, 0, 0, 1, 0, 1), (0, 1, 2, 1, 0, 1), (0, float("inf"), 0, 1, 0, 1), (float("nan"), 1, 0, 1, 0, 1),
                (0, 1, 0, 1, 1, 0), (0, 1, 0, 1, float("nan"), 1)):
        with pytest.raises(ValueError, match="roi"):
            table.fluence_map(segs, view="Z", roi=roi)
    # the depth of one view is an image axis of another
    with pytest.raises(ValueError, match="roi"):
        table.fluence_map(segs, view="X", roi=ROI)  # z runs to +inf
    for pixels in (0, -3, (30, 0), (30,), 2.5, "30", None, True):
        with pytest.raises(ValueError, match="bins"):
            table.fluence_map(segs, roi=ROI, pixels=pixels)
    with pytest.raises(ValueError, match="pixels do not resolve"):
        table.fluence_map(segs, roi=(1.0, np.nextafter(1.0, 2.0), 0, 1, 0, 1), pixels=4)
    for weight in ("power", None, 0, "Intensity"):
        with pytest.raises(ValueError, match="weight"):
            table.fluence_map(segs, roi=ROI, weight=weight)
    # ... and what is good gets that far; an empty table has no box to fall back on
    for kwargs in ({}, {"view": "Z", "pixels": (7, 5)}, {"weight": "none"}):
        with pytest.raises(AssertionError, match="the engine was asked for"):
            table.fluence_map(segs, roi=ROI, **kwargs)
    with pytest.raises(ValueError):
        table.fluence_map(segs)


class _Recorder:
    """Stands in for the engine: keeps what fluence_map hands over."""

    def fluence_map(self, axes, u_edges, v_edges, depth, segs, weighted=True, into=None):
        self.axes, self.u_edges, self.v_edges, self.depth, self.weighted, self.into = axes, u_edges, v_edges, depth, weighted, into
        if into is not None:
            into[2].add_(2)
            return into
        shape = (len(u_edges) - 1, len(v_edges) - 1)
        return torch.zeros(shape, dtype=torch.int64), torch.full(shape, 3.0, dtype=torch.float64), torch.tensor([5])


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table, segs = oa.OpticalTable(), support.host_segments()
    roi = (-1.0, 9.0, -3.01, 2.97, -0.5, 0.75)
    ranges = {"x": roi[0:2], "y": roi[2:4], "z": roi[4:6]}
    for view, (u, v, w), lab in (("Z", "xyz", [0, 1, 2]), ("X", "yzx", [1, 2, 0]), ("Y", "zxy", [2, 0, 1])):
        fm = table.fluence_map(segs, view=view, roi=roi, pixels=(7, 5))
        np.testing.assert_array_equal(rec.axes, EYE[lab])  # the lab axes of ray.py's dimension_dict, then the depth
        np.testing.assert_array_equal(rec.u_edges, np.linspace(*ranges[u], 8))
        np.testing.assert_array_equal(rec.v_edges, np.linspace(*ranges[v], 6))
        assert tuple(rec.depth) == ranges[w] and rec.weighted is True and rec.into is None
        assert isinstance(fm, oa.FluenceMap) and fm.view == view and fm.roi == roi and fm.pixels == (7, 5) and fm.weight == "intensity"
        assert fm.u_edges is rec.u_edges and fm.v_edges is rec.v_edges and fm.skipped == 5
        assert fm.extent == ranges[u] + ranges[v]
        assert fm.counts.dtype == torch.int64 and fm.fluence.dtype == torch.float64
        counts, fluence, ue, ve = fm.to_host()
        assert counts.shape == fluence.shape == (7, 5) and (fluence == 3.0).all() and ue is fm.u_edges and ve is fm.v_edges
    # an infinite depth range goes through as it is; weight="none" asks for plain path length; an int is both axes
    fm = table.fluence_map(segs, view="Z", roi=ROI, pixels=4, weight="none")
    assert tuple(rec.depth) == (-0.5, float("inf")) and rec.weighted is False and fm.pixels == (4, 4) and fm.weight == "none"
    # into= hands the earlier tensors back, and the lazily read counter follows them
    fm = table.fluence_map(segs, view="Y", roi=roi, pixels=(7, 5))
    again = table.fluence_map(segs, view="Y", roi=list(roi), pixels=(7, 5), into=fm)
    assert again is fm and rec.into[0] is fm.counts and rec.into[1] is fm.fluence and len(rec.into) == 3 and fm.skipped == 7
    for kwargs in ({"view": "Z"}, {"pixels": (5, 7)}, {"pixels": 7}, {"weight": "none"}, {"roi": (-1.0, 9.0, -3.0, 2.97, -0.5, 0.75)}):
        with pytest.raises(ValueError, match="into"):
            table.fluence_map(segs, **{"view": "Y", "roi": roi, "pixels": (7, 5), **kwargs}, into=fm)
    with pytest.raises(ValueError, match="into"):
        table.fluence_map(segs, view="Y", roi=roi, pixels=(7, 5), into=(fm.counts, fm.fluence))
    # roi=None: the table's box
    table.add_components([oa.Lens([5, 0, 0], focal_length=5, radius=1.0)])
    with pytest.raises(ValueError, match="roi"):  # one flat component: a box of no depth along x
        table.fluence_map(segs, pixels=3)
    table.add_components([oa.Lens([10, 0, 0], focal_length=5, radius=2.0)])
    fm = table.fluence_map(segs, pixels=3)
    box = tuple(float(b) for b in table.get_bbox())
    assert fm.roi == box and fm.extent == box[:4] and tuple(rec.depth) == box[4:]


# -- the reference against closed forms -----------------------------------------------------------------------------------------
E2 = np.array([0.0, 1.0, 2.0])


def _one(o, d, length, intensity=None, ue=E2, ve=E2, w=(-1.0, 1.0)):
    return fluence_reference([o], [d], [length], None if intensity is None else [intensity], EYE, ue, ve, *w)


def test_reference_diagonal_through_a_2_x_2_grid():
    r = _one([0, 0, 0], [1, 1, 0], 2 * np.sqrt(2))
    assert r.counts.tolist() == [[1, 0], [0, 1]] and r.skipped == 0  # the corner is a piece of no length: nothing in (0, 1), (1, 0)
    np.testing.assert_allclose(r.fluence, [[np.sqrt(2), 0], [0, np.sqrt(2)]], rtol=4 * U)
    assert len(r.pieces) == 2
    # ... both ways, weighted, and longer than the box: clipped at its walls
    r = _one([3, 3, 0], [-2, -2, 0], 10.0, intensity=0.5)
    assert r.counts.tolist() == [[1, 0], [0, 1]]
    np.testing.assert_allclose(r.fluence, [[np.sqrt(0.5), 0], [0, np.sqrt(0.5)]], rtol=8 * U)
    np.testing.assert_allclose(r.clipped, 2 * np.sqrt(2), rtol=8 * U)
    # off the diagonal: three pixels, lengths by similar triangles (v = u + 0.5: crossings at u = 0.5, 1, 1.5)
    r = _one([0, 0.5, 0], [1, 1, 0], 10.0)
    assert r.counts.tolist() == [[1, 1], [0, 1]]
    np.testing.assert_allclose(r.fluence, [[np.sqrt(0.5), np.sqrt(0.5)], [0, np.sqrt(0.5)]], rtol=8 * U)


def test_reference_axis_parallel_segments_and_grid_lines():
    ue = ve = np.array([0.0, 1.0, 2.0, 3.0])
    run = lambda v, **kw: _one([0.25, v, 0], kw.pop("d", [1, 0, 0]), kw.pop("length", 2.5), ue=ue, ve=ve, **kw)  # noqa: E731
    between = run(1.5)
    assert between.counts.tolist() == [[0, 1, 0], [0, 1, 0], [0, 1, 0]]
    assert between.fluence[:, 1].tolist() == [0.75, 1.0, 0.75] and sorted(between.pieces.tolist()) == [0.75, 0.75, 1.0]
    assert run(1.0).counts[:, 1].tolist() == [1, 1, 1]                      # along a grid line: the upper pixel
    assert run(np.nextafter(1.0, 0.0)).counts[:, 0].tolist() == [1, 1, 1]   # ... a hair below it: the lower one
    assert run(0.0).counts[:, 0].tolist() == [1, 1, 1]                      # the box's lower wall: inside
    assert run(3.0).counts[:, 2].tolist() == [1, 1, 1]                      # the closing edge: the last pixel, closed
    assert run(np.nextafter(3.0, 4.0)).counts.sum() == 0 and run(np.nextafter(0.0, -1.0)).counts.sum() == 0  # outside
    # both directions of travel give the same image; starting on a line, a piece lies on the side it moves to
    back = _one([2.75, 1.5, 0], [-1, 0, 0], 2.5, ue=ue, ve=ve)
    assert np.array_equal(back.counts, between.counts) and np.array_equal(back.fluence, between.fluence)
    assert _one([1.0, 0.5, 0], [1, 0, 0], 0.5, ue=ue, ve=ve).counts[:, 0].tolist() == [0, 1, 0]
    assert _one([1.0, 0.5, 0], [-1, 0, 0], 0.5, ue=ue, ve=ve).counts[:, 0].tolist() == [1, 0, 0]
    assert _one([0.5, 1.0, 0], [0, -1, 0], 0.5, ue=ue, ve=ve).counts[0].tolist() == [1, 0, 0]
    # ending on a line adds no piece beyond it
    assert _one([0.5, 0.5, 0], [1, 0, 0], 0.5, ue=ue, ve=ve).counts[:, 0].tolist() == [1, 0, 0]
    # the depth: inside iff w_lo <= w <= w_hi for a segment at rest in w, clipped for one that moves
    assert run(1.5, w=(0.0, 0.0)).counts.sum() == 3 and run(1.5, w=(0.5, 1.0)).counts.sum() == 0
    deep = _one([0.5, 0.5, -2.0], [0, 0, 1], 10.0, ue=ue, ve=ve, w=(-1.0, 1.0))
    assert deep.counts[0, 0] == 1 and deep.counts.sum() == 1 and deep.fluence[0, 0] == 2.0


def test_reference_segments_that_deposit_nothing():
    zero = _one([0.5, 0.5, 0], [1, 0, 0], 0.0)
    assert zero.counts.sum() == 0 and zero.skipped == 0 and len(zero.pieces) == 0
    # unbounded: clipped by finite walls it is a segment like any other ...
    r = _one([0.5, 0.5, 0], [1, 0, 0], np.inf)
    assert r.counts[:, 0].tolist() == [1, 1] and r.fluence[:, 0].tolist() == [0.5, 1.0] and r.skipped == 0
    r = _one([0.5, 0.5, 0], [0, 0, 1], np.inf)
    assert r.counts[0, 0] == 1 and r.fluence[0, 0] == 1.0 and r.skipped == 0
    # ... leaving along the depth of a box that has no far wall it is skipped; entirely outside it is neither
    r = _one([0.5, 0.5, 0], [0, 0, 1], np.inf, w=(-1.0, np.inf))
    assert r.counts.sum() == 0 and r.skipped == 1
    r = _one([5.0, 0.5, 0], [0, 0, 1], np.inf, w=(-1.0, np.inf))
    assert r.counts.sum() == 0 and r.skipped == 0
    for o, d, length in (([np.nan, 0.5, 0], [1, 0, 0], 1.0), ([0.5, 0.5, 0], [1, np.nan, 0], 1.0), ([0.5, 0.5, 0], [1, 0, 0], np.nan),
                         ([0.5, 0.5, 0], [0, 0, 0], 1.0)):
        r = _one(o, d, length)
        assert r.counts.sum() == 0 and r.skipped == 1
    r = fluence_reference([[np.nan, 0, 0], [0.5, 0.5, 0]], [[1, 0, 0]] * 2, [1.0, 0.25], None, EYE, E2, E2, -1, 1, valid=[False, True])
    assert r.skipped == 0 and r.counts[0, 0] == 1 and r.fluence[0, 0] == 0.25  # a slot that holds no segment is not looked at


def _liang_barsky(o, d, length, lo, hi):
    """Length of the part of o + t d / |d|, 0 <= t <= length, inside the box [lo, hi], segment by segment."""
    total = 0.0
    for p, q, L in zip(o, d, length):
        q = q / np.sqrt(q @ q)
        t0, t1 = 0.0, L
        for k in range(3):
            if q[k] == 0.0:
                if not lo[k] <= p[k] <= hi[k]:
                    t1 = -1.0
            else:
                a, b = sorted(((lo[k] - p[k]) / q[k], (hi[k] - p[k]) / q[k]))
                t0, t1 = max(t0, a), min(t1, b)
        total += max(t1 - t0, 0.0)
    return total


def test_reference_conserves_length():
    rng = np.random.default_rng(5)
    n = 2000
    o, d = rng.uniform(-3, 3, (n, 3)), rng.normal(size=(n, 3))
    d[::7, 1] = 0.0  # some at rest along an axis, some along two
    d[::11, :2] = [1.0, 0.0]
    o[::13, 0] = 0.5  # ... some of them on a grid line
    length = rng.uniform(0, 6, n)
    for view, lab in (("Z", [0, 1, 2]), ("Y", [2, 0, 1])):
        lo, hi = np.array([-2.0, -1.5, -1.0]), np.array([2.0, 1.0, 2.5])
        ue, ve = np.linspace(lo[lab[0]], hi[lab[0]], 18), np.linspace(lo[lab[1]], hi[lab[1]], 12)
        r = fluence_reference(o, d, length, None, EYE[lab], ue, ve, lo[lab[2]], hi[lab[2]])
        want = _liang_barsky(o, d, length, lo, hi)
        assert r.skipped == 0 and r.counts.sum() == len(r.pieces) > n
        # nothing twice, nothing lost: a few roundings a piece
        assert abs(r.fluence.sum() - want) <= 16 * U * len(r.pieces) * 12.0
        assert abs(r.clipped - want) <= 16 * U * n * 12.0
        np.testing.assert_array_equal(r.fluence, r.abs_fluence)
        assert (r.bound[r.counts > 0] > 0).all() and (r.bound[r.counts == 0] == 0).all()


def test_the_one_monitor_kernels_are_gone():
    sources = glob.glob(os.path.join(ROOT, "optable_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "optable_amd", "csrc", "*.hip"))
    assert len(sources) > 5
    for path in sources:
        text = open(path).read()
        assert "k_mon_test" not in text and "k_mon_compact" not in text, path
