"""CPU: the public surface of spot statistics (`OpticalTable.spots_all` / `spots_batch`, `MonitorSpots`: the moments of every
monitor's hits on the monitor and on planes displaced along its normal, summed on the device, ot_monitor_spots_many) — the calls
and the binding, the planner and its constant, what is refused before the engine is asked, the arithmetic of `MonitorSpots` on
hand-made sums, and the numpy reference of the GPU tests against closed forms.  No library call is made."""
import os
import re

import numpy as np
import pytest
import torch

import optable_amd as oa
import support
from optable_amd import abi
from optable_amd.engine import Engine
from spots_reference import U, radius_interval, spots_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE9 = np.eye(3).ravel()
YZ = np.array([0.0, 1.0, 0.0, 0.0, 0.0, 1.0])


def test_the_calls_exist():
    from optable_amd import engine, spots

    assert callable(oa.OpticalTable.spots_all) and callable(oa.OpticalTable.spots_batch)
    assert callable(Engine.monitor_spots_many) and callable(engine.spots_plan)
    assert oa.MonitorSpots is spots.MonitorSpots
    for name in ("power", "centroid", "covariance", "rms_y", "rms_z", "rms_radius", "best_focus", "to_host"):
        assert callable(getattr(spots.MonitorSpots, name)), name
    assert "ot_monitor_spots_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_spots_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_spots_many is not declared in the header"
    names = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "mons", "n_monitors", "axes", "centre", "offsets", "n_offsets", "src", "intensity", "n_segments", "seg_count", "n_rays",
                     "counts", "sums", "accumulate"]
    restype, argtypes = abi.SYMBOLS["ot_monitor_spots_many"]
    assert restype is C.c_int and len(argtypes) == len(names) == 15
    widths = {"n_monitors": C.c_int32, "n_offsets": C.c_int32, "accumulate": C.c_int32, "n_segments": C.c_int64, "n_rays": C.c_int64}
    for name, kind in zip(names, argtypes):  # pointers as pointers, the integers by their width
        assert kind is widths[name] if name in widths else kind not in (C.c_int32, C.c_int64, C.c_double), name
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)


def test_planner_and_its_constant():
    from optable_amd import engine

    text = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bMON_SPOT_CELLS\s*=\s*(\d+)", text)
    assert found and int(found.group(1)) == engine.SPOT_CELLS == 256
    assert 4 * 7 * 8 * engine.SPOT_CELLS <= 65536  # four waves' rows of seven doubles a cell in the LDS of a launch
    assert engine.spots_plan(1, 1) == [(0, 1)]
    assert engine.spots_plan(1, 256) == [(0, 256)] and engine.spots_plan(1, 257) == [(0, 256), (256, 1)]
    assert engine.spots_plan(8, 32) == [(0, 256)]
    assert engine.spots_plan(2, 200) == [(0, 256), (256, 144)]  # a group ends inside a monitor's planes
    plan = engine.spots_plan(1 << 10, 1 << 10)
    assert len(plan) == 4096 and plan[-1] == ((1 << 20) - 256, 256)
    for m, j in ((0, 3), (3, 0), (-1, 5), (1 << 10, (1 << 10) + 1)):
        with pytest.raises(ValueError):
            engine.spots_plan(m, j)


class _Recorder:
    """Stands in for the engine: keeps what spots_all hands over."""

    def monitor_spots_many(self, mons, axes, centre, offsets, segs, weighted=True, into=None):
        self.axes, self.centre, self.offsets, self.weighted, self.into, self.n = axes, centre, offsets, weighted, into, len(mons)
        if into is not None:
            into[0].add_(1)
            return into
        return torch.zeros((len(mons), len(offsets)), dtype=torch.int64), torch.zeros((len(mons), len(offsets), 6), dtype=torch.float64)


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table, segs = oa.OpticalTable(), support.host_segments()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6)]
    table.add_monitors(mons)
    for weight in ("power", None, 0, "Intensity"):
        with pytest.raises(ValueError, match="weight"):
            table.spots_all(segs, weight=weight)
    for offsets in ((), [], [0.0, np.nan], [np.inf], "focus", [[0.0, 1.0]], None):
        with pytest.raises(ValueError, match="offsets"):
            table.spots_all(segs, offsets=offsets)
    for centre in ((0.0, np.nan), (np.inf, 0.0), (1.0,), [(0, 0)] * 3, "middle", (0, 0, 0)):
        with pytest.raises(ValueError, match="centre"):
            table.spots_all(segs, centre=centre)
    with pytest.raises(AssertionError, match="the engine was asked for"):
        table.spots_all(segs, offsets=[-1.0, 0.0, 1.0], centre=(0.1, 0.2), weight="none")
    # `into`: the list of ONE earlier call for the same monitors, offsets, weight and centre
    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    first = table.spots_all(segs, offsets=[-1.0, 0.0, 1.0])
    other = table.spots_all(segs, offsets=[-1.0, 0.0, 1.0])
    monkeypatch.setattr(table_module, "_engine", refuse)
    for kwargs in ({"offsets": [-1.0, 0.0, 2.0]}, {"offsets": [-1.0, 0.0]}, {"weight": "none"}, {"centre": (0.0, 1e-3)}, {"monitors": mons[::-1]},
                   {"monitors": mons[:1]}):
        with pytest.raises(ValueError, match="into"):
            table.spots_all(segs, **{"offsets": [-1.0, 0.0, 1.0], **kwargs}, into=first)
    for into in ([first[0], other[1]], first[::-1], first[:1], (first[0].counts, first[0].sums), [first[0], "spots"]):
        with pytest.raises(ValueError, match="into"):
            table.spots_all(segs, offsets=[-1.0, 0.0, 1.0], into=into)


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table, segs = oa.OpticalTable(), support.host_segments()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6).RotZ(0.3)]
    table.add_monitors(mons)
    spots = table.spots_all(segs)
    assert rec.n == 2 and rec.weighted is True and rec.into is None
    np.testing.assert_array_equal(rec.offsets, [0.0])
    np.testing.assert_array_equal(rec.centre, np.zeros((2, 2)))
    np.testing.assert_array_equal(rec.axes, [np.concatenate([m.tangent_Y, m.tangent_Z]) for m in mons])  # the images' axes
    assert [s.monitor for s in spots] == mons and all(isinstance(s, oa.MonitorSpots) for s in spots)
    assert all(s.weight == "intensity" and s.centre == (0.0, 0.0) and s.counts.shape == (1,) and s.sums.shape == (1, 6) for s in spots)
    spots = table.spots_all(segs, offsets=np.linspace(-1, 1, 5), weight="none", centre=[(0.1, 0.2), (0.3, 0.4)], monitors=mons[::-1])
    assert rec.weighted is False and rec.centre.tolist() == [[0.1, 0.2], [0.3, 0.4]] and len(rec.offsets) == 5
    assert spots[0].monitor is mons[1] and spots[0].centre == (0.1, 0.2) and spots[1].centre == (0.3, 0.4) and spots[0].weight == "none"
    assert table.spots_all(segs, centre=(0.5, -0.5))[1].centre == (0.5, -0.5)  # one for all
    again = table.spots_all(segs, offsets=np.linspace(-1, 1, 5), weight="none", centre=[(0.1, 0.2), (0.3, 0.4)], monitors=mons[::-1], into=spots)
    assert all(a is b for a, b in zip(again, spots)) and rec.into[0] is spots[0]._stack[0] and int(spots[1].counts[0]) == 1
    one = table.spots_batch(mons[1], segs, offsets=[0.0, 0.5])
    assert rec.n == 1 and one.monitor is mons[1] and one.offsets.tolist() == [0.0, 0.5]
    counts, sums, offsets = one.to_host()
    assert counts.dtype == np.int64 and sums.shape == (2, 6) and offsets is one.offsets


def _spots(offsets, counts, sums, centre=(0.0, 0.0)):
    return oa.MonitorSpots(None, np.asarray(offsets, dtype=float), torch.tensor(counts, dtype=torch.int64), torch.tensor(sums, dtype=torch.float64),
                           "intensity", centre)


def _sums_of(w, y, z):
    return [w.sum(), (w * y).sum(), (w * z).sum(), (w * y * y).sum(), (w * z * z).sum(), (w * y * z).sum()]


def test_moments_on_hand_made_sums():
    rng = np.random.default_rng(3)
    w, y, z = 0.25 + rng.random(50), rng.normal(0.3, 0.1, 50), rng.normal(-0.2, 0.05, 50)
    sp = _spots([0.0, 1.0], [50, 0], [_sums_of(w, y - 0.25, z + 0.25), [0.0] * 6], centre=(0.25, -0.25))
    my, mz = (w * y).sum() / w.sum(), (w * z).sum() / w.sum()
    cov = np.cov(np.stack([y, z]), aweights=w, bias=True)
    np.testing.assert_allclose(sp.power().numpy(), [w.sum(), 0.0], rtol=1e-14)
    np.testing.assert_allclose(sp.centroid()[0].numpy(), [my, mz], rtol=1e-13)  # `centre` is added back
    np.testing.assert_allclose(sp.covariance()[0].numpy(), cov, rtol=1e-11)
    np.testing.assert_allclose([sp.rms_y()[0], sp.rms_z()[0], sp.rms_radius()[0]], [np.sqrt(cov[0, 0]), np.sqrt(cov[1, 1]), np.sqrt(cov[0, 0] + cov[1, 1])],
                               rtol=1e-11)
    # a plane without hits is NaN everywhere but in its power
    assert torch.isnan(sp.centroid()[1]).all() and torch.isnan(sp.covariance()[1]).all() and torch.isnan(sp.rms_radius()[1])
    assert tuple(sp.centroid().shape) == (2, 2) and tuple(sp.covariance().shape) == (2, 2, 2)
    # a variance that rounding left below zero is 0: one point, Wyy / W - (Wy / W)^2 = 0.01 - 0.1^2 < 0 in doubles
    one = _spots([0.0], [1], [[1.0, 0.1, 0.0, 0.01, 0.0, 0.0]])
    assert 0.01 - 0.1 * 0.1 < 0 and float(one.rms_y()[0]) == 0.0 and float(one.rms_radius()[0]) == 0.0


def _parabola(offsets, vertex, floor, slope2, counts=None):
    """Sums of planes whose var_y is floor + slope2 (x - vertex)^2, with W = 1, a zero centroid and no z."""
    offsets = np.asarray(offsets, dtype=float)
    sums = np.zeros((len(offsets), 6))
    sums[:, 0], sums[:, 3] = 1.0, floor + slope2 * (offsets - vertex) ** 2
    return _spots(offsets, [5] * len(offsets) if counts is None else counts, sums)


def test_best_focus():
    # an exact parabola: the vertex, between the samples, on uneven spacing too
    for offsets in (np.linspace(-0.5, 0.5, 11), [-0.5, -0.4, -0.1, 0.25, 0.5]):
        x, r = _parabola(offsets, -0.13, 4e-6, 0.01).best_focus()
        assert abs(x + 0.13) < 1e-12 and abs(r - 2e-3) < 1e-12
    # at an end point: the sampled minimum
    x, r = _parabola(np.linspace(0.0, 1.0, 5), -0.13, 0.0, 0.01).best_focus()
    assert x == 0.0 and abs(r - 0.1 * 0.13) < 1e-15
    x, r = _parabola(np.linspace(-1.0, -0.25, 4), -0.13, 0.0, 0.01).best_focus()
    assert x == -0.25 and abs(r - 0.1 * 0.12) < 1e-15
    # a neighbour with fewer than two hits does not qualify: the sampled minimum; planes with fewer than two are never the answer
    x, r = _parabola([-0.5, -0.25, 0.0, 0.25], -0.13, 0.0, 0.01, counts=[5, 5, 1, 5]).best_focus()
    assert x == -0.25
    x, r = _parabola([-0.5, -0.25, 0.0, 0.25], -0.2, 0.0, 0.01, counts=[5, 1, 5, 5]).best_focus()
    assert x == 0.0
    x, r = _parabola([0.0, 1.0], 0.0, 0.0, 1.0, counts=[1, 0]).best_focus()
    assert np.isnan(x) and np.isnan(r)
    assert _parabola([0.3], 0.0, 0.0, 1.0).best_focus() == (0.3, 0.3)  # one plane
    # unsorted or repeated offsets: refused
    for offsets in ([0.0, -0.5, 0.5], [0.0, 0.0, 0.5]):
        with pytest.raises(ValueError, match="sorted"):
            _parabola(offsets, 0.1, 0.0, 1.0).best_focus()


# -- the reference against closed forms -----------------------------------------------------------------------------------------
def _cone(n=360, x0=9.7, theta_max=0.05, seed=2):
    """n rays through the point (x0, 0, 0), in opposite pairs (a zero centroid): segments from x = x0 - 3 of length 8."""
    rng = np.random.default_rng(seed)
    tan, phi = np.tan(theta_max * np.sqrt(rng.random(n // 2))), rng.uniform(0, 2 * np.pi, n // 2)
    tan, phi = np.concatenate([tan, tan]), np.concatenate([phi, phi + np.pi])
    d = np.stack([np.ones(n), tan * np.cos(phi), tan * np.sin(phi)], axis=1)
    return np.array([x0, 0.0, 0.0]) - 3.0 * d, d, np.full(n, 8.0), tan


def test_reference_cone_through_a_point():
    o, d, length, tan = _cone()
    offsets = np.linspace(-0.6, 0.6, 25)
    r = spots_reference(o, d, length, None, EYE9, [10.0, 0, 0], 3.0, 3.0, YZ, (0.0, 0.0), offsets)
    assert r.margin > 1e-7 and (r.counts == len(tan)).all()
    z0 = 9.7 - 10.0  # where the point lies along the monitor's normal
    want = np.abs(offsets - z0) * np.sqrt(np.mean(tan**2))
    sp = _spots(offsets, r.counts, r.sums)
    got = sp.rms_radius().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    for j in range(len(offsets)):
        lo, hi = radius_interval(r.sums[j], r.bound[j])
        assert lo <= got[j] <= hi and hi - lo < 1e-6
    np.testing.assert_allclose(sp.centroid().numpy(), 0.0, atol=1e-14)
    assert sp.power().tolist() == [len(tan)] * 25  # weight 1: W is the count
    x, radius = sp.best_focus()
    assert abs(x - z0) < 1e-9 and radius < 1e-7  # var_r is exactly quadratic: the vertex, not the nearest sample (-0.3 is one here, too)
    x, radius = _spots(offsets[::3] + 0.01, *spots_reference(o, d, length, None, EYE9, [10.0, 0, 0], 3.0, 3.0, YZ, (0.0, 0.0), offsets[::3] + 0.01)[:2]).best_focus()
    assert abs(x - z0) < 1e-9 and radius < 1e-7  # ... between the samples


def test_reference_rules():
    # the rectangle clips; a weight scales; a slot that holds no segment is not looked at; the margin is the nearest decision
    o = np.array([[0.0, 0.5, 0.0], [0.0, 1.5, 0.0], [0.0, -0.25, 0.75], [0.0, 0.0, 0.0]])
    d = np.tile([1.0, 0.0, 0.0], (4, 1))
    r = spots_reference(o, d, [10.0, 10.0, 10.0, 2.0], [0.5, 1.0, 2.0, 4.0], EYE9, [5.0, 0, 0], 1.0, 1.0, YZ, (0.0, 0.0), [0.0, -3.5, 5.5], valid=[1, 1, 1, 1])
    assert r.counts.tolist() == [2, 3, 0]  # ray 1 is outside the rectangle; ray 3 ends at x = 2; nothing reaches x = 10.5
    assert [h.tolist() for h in r.hits] == [[0, 2], [0, 2, 3], []]
    np.testing.assert_allclose(r.sums[0], [2.5, 0.25 - 0.5, 1.5, 0.125 + 0.125, 1.125, -0.375], rtol=4 * U)
    assert r.margin == 0.25  # |Pz| = 0.75 against the half height 1
    r = spots_reference(o, d, [10.0] * 4, None, EYE9, [5.0, 0, 0], 1.0, 1.0, YZ, (0.5, 0.0), [0.0], valid=[1, 0, 1, 1])
    assert r.counts.tolist() == [3] and r.sums[0, 0] == 3.0 and r.sums[0, 1] == 0.0 - 0.75 - 0.5
    # the monitor's own rule at its plane: a segment that starts on it (|t| < 1e-9) or behind it does not hit
    r = spots_reference([[5.0, 0, 0], [6.0, 0, 0], [4.0, 0, 0]], [[1.0, 0, 0]] * 3, [1.0] * 3, None, EYE9, [5.0, 0, 0], 1.0, 1.0, YZ, (0, 0), [0.0, 0.5])
    assert [h.tolist() for h in r.hits] == [[2], [0]] and r.margin == 0.0  # (the third ends exactly on the monitor: t == length hits)
    # a rotated frame: the normal is column 0 of M
    c, s = np.cos(0.3), np.sin(0.3)
    M = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).ravel()
    r = spots_reference([[0.0, 0, 0]], [[c, s, 0]], [20.0], None, M, [5 * c, 5 * s, 0], 1.0, 1.0, YZ, (0, 0), [0.0, 2.0, 16.0])
    assert r.counts.tolist() == [1, 1, 0]
    np.testing.assert_allclose(r.sums[:2, 1:], 0.0, atol=1e-15)
