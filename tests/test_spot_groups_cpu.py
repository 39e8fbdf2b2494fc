"""CPU: the public surface of spot statistics per ray group (`OpticalTable.spots_grouped_all` / `spots_grouped_batch`,
`MonitorSpotGroups`, `RayBatch.groups_by_wavelength`: the moments of every monitor's hits per plane and per group of input rays,
summed on the device, ot_monitor_spot_groups_many) — the calls and the binding, the planner and its constants, what is refused
before the engine is asked, and the arithmetic of `MonitorSpotGroups` on hand-made sums.  No library call is made."""
import os
import re

import numpy as np
import pytest
import torch

import optable_amd as oa
import support
from optable_amd import abi
from optable_amd.batch import RayBatch
from optable_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_calls_exist():
    from optable_amd import engine, spots

    assert callable(oa.OpticalTable.spots_grouped_all) and callable(oa.OpticalTable.spots_grouped_batch)
    assert callable(Engine.monitor_spot_groups_many) and callable(engine.spot_groups_plan) and callable(spots.spot_group_ids)
    assert callable(RayBatch.groups_by_wavelength)
    assert oa.MonitorSpotGroups is spots.MonitorSpotGroups
    for name in ("group", "total", "power", "centroid", "rms_radius", "best_focus", "to_host"):
        assert callable(getattr(spots.MonitorSpotGroups, name)), name
    assert "ot_monitor_spot_groups_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = _header()
    decl = re.search(r"\bint\s+ot_monitor_spot_groups_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_spot_groups_many is not declared in the header"
    names = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "mons", "n_monitors", "axes", "centre", "offsets", "n_offsets", "groups", "n_group_ids", "n_groups", "src", "intensity",
                     "n_segments", "seg_count", "n_rays", "counts", "sums", "accumulate"]
    restype, argtypes = abi.SYMBOLS["ot_monitor_spot_groups_many"]
    assert restype is C.c_int and len(argtypes) == len(names) == 18
    widths = {"n_monitors": C.c_int32, "n_offsets": C.c_int32, "n_groups": C.c_int32, "accumulate": C.c_int32, "n_group_ids": C.c_int64,
              "n_segments": C.c_int64, "n_rays": C.c_int64}
    types = dict(zip(names, [a.strip().rsplit(None, 1)[0] + ("*" if "*" in a else "") for a in decl.group(1).split(",")]))
    for name, kind in zip(names, argtypes):  # pointers as pointers, the integers by their width — the binding's and the header's
        assert kind is widths[name] if name in widths else kind not in (C.c_int32, C.c_int64, C.c_double), name
        if name in widths:
            assert types[name] == {C.c_int32: "int32_t", C.c_int64: "int64_t"}[widths[name]], (name, types[name])
        else:
            assert "*" in types[name], (name, types[name])
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)
    # the arguments the grouped call shares with ot_monitor_spots_many are that call's, in its order
    plain = abi.SYMBOLS["ot_monitor_spots_many"][1]
    assert argtypes[:7] == plain[:7] and argtypes[10:] == plain[7:]


def test_planner_and_its_constants():
    from optable_amd import engine

    kernels = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bMON_SPOT_CELLS\s*=\s*(\d+)", kernels)
    assert found and int(found.group(1)) == engine.SPOT_CELLS == 256
    define = re.search(r"#define\s+OT_SPOT_GROUPS_MAX\s+(\d+)\b", _header())
    assert define and int(define.group(1)) == engine.SPOT_GROUPS_MAX == 256
    for G in range(1, 257):  # a launch: whole pairs, at least one, within the LDS of MON_SPOT_CELLS cells
        plan = engine.spot_groups_plan(2, 3, G)
        most = (int(found.group(1)) // G) * G
        assert G <= most <= int(found.group(1)) and most % G == 0
        assert all(first % G == 0 and cells % G == 0 and 0 < cells <= most for first, cells in plan)
        assert [first for first, _ in plan] == list(range(0, 6 * G, most)) and sum(cells for _, cells in plan) == 6 * G
    assert engine.spot_groups_plan(1, 1, 1) == [(0, 1)]
    assert engine.spot_groups_plan(8, 32, 1) == [(0, 256)] == engine.spots_plan(8, 32)
    assert engine.spot_groups_plan(1, 32, 8) == [(0, 256)]
    assert engine.spot_groups_plan(1, 33, 8) == [(0, 256), (256, 8)]
    assert engine.spot_groups_plan(4, 5, 100) == [(200 * k, 200) for k in range(10)]  # 2 pairs a launch
    assert engine.spot_groups_plan(4, 5, 256) == [(256 * k, 256) for k in range(20)]  # 1 pair a launch
    assert engine.spot_groups_plan(4, 5, 255) == [(255 * k, 255) for k in range(20)]
    assert engine.spot_groups_plan(1, 3, 100) == [(0, 200), (200, 100)]  # the last launch: the pair that is left
    assert len(engine.spot_groups_plan(64, 64, 256)) == 4096  # 2^20 cells
    for m, j, g in ((1, 1, 257), (1, 1, 0), (1, 1, -1), (0, 1, 1), (1, 0, 1), (64, 64, 257), (1 << 10, 1 << 10, 2), (4097, 1, 256)):
        with pytest.raises(ValueError):
            engine.spot_groups_plan(m, j, g)


class _Recorder:
    """Stands in for the engine: keeps what spots_grouped_all hands over."""

    def monitor_spot_groups_many(self, mons, axes, centre, offsets, groups, n_groups, segs, weighted=True, into=None):
        self.axes, self.centre, self.offsets, self.weighted, self.into, self.n = axes, centre, offsets, weighted, into, len(mons)
        self.groups, self.n_groups = groups, n_groups
        if into is not None:
            into[0].add_(1)
            return into
        J = len(offsets)
        return torch.zeros((len(mons), J, n_groups), dtype=torch.int64), torch.zeros((len(mons), J, n_groups, 6), dtype=torch.float64)


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table, segs = oa.OpticalTable(), support.host_segments()  # 4 rays
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6)]
    table.add_monitors(mons)
    ids = [0, 1, 2, 1]
    for groups in ([0, 1, 2], [0, 1, 2, 1, 0], [], [[0, 1], [2, 1]], 1, None):  # one id per input ray
        with pytest.raises(ValueError, match="groups"):
            table.spots_grouped_all(segs, groups)
    for groups in ([0.0, 1.0, 2.0, 1.0], np.array(ids, dtype=np.float32), torch.tensor(ids, dtype=torch.float64), ["a", "b", "c", "d"],
                   [True, False, True, False], torch.tensor(ids) > 0):
        with pytest.raises(ValueError, match="groups"):
            table.spots_grouped_all(segs, groups)
    for n_groups in (0, -1, 257, 2.0, "3", True):
        with pytest.raises(ValueError, match="n_groups"):
            table.spots_grouped_all(segs, ids, n_groups=n_groups)
    with pytest.raises(ValueError, match="n_groups"):
        table.spots_grouped_all(segs, [0, 1, 256, 1])  # max id + 1 = 257 groups
    for weight in ("power", None, 0, "Intensity"):
        with pytest.raises(ValueError, match="weight"):
            table.spots_grouped_all(segs, ids, weight=weight)
    for offsets in ((), [], [0.0, np.nan], [np.inf], "focus", [[0.0, 1.0]], None):
        with pytest.raises(ValueError, match="offsets"):
            table.spots_grouped_all(segs, ids, offsets=offsets)
    for centre in ((0.0, np.nan), (np.inf, 0.0), (1.0,), [(0, 0)] * 3, "middle", (0, 0, 0)):
        with pytest.raises(ValueError, match="centre"):
            table.spots_grouped_all(segs, ids, centre=centre)
    with pytest.raises(ValueError, match="labels"):
        table.spots_grouped_all(segs, ids, labels=[780e-7, 560e-7])
    with pytest.raises(AssertionError, match="the engine was asked for"):
        table.spots_grouped_all(segs, ids, offsets=[-1.0, 0.0, 1.0], centre=(0.1, 0.2), weight="none")
    # `into`: the list of ONE earlier call for the same monitors, offsets, weight, centre and G
    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    first = table.spots_grouped_all(segs, ids, offsets=[-1.0, 0.0, 1.0])
    other = table.spots_grouped_all(segs, ids, offsets=[-1.0, 0.0, 1.0])
    plain = [oa.MonitorSpots(m, np.array([-1.0, 0.0, 1.0]), torch.zeros(3, dtype=torch.int64), torch.zeros((3, 6), dtype=torch.float64), "intensity",
                             (0.0, 0.0)) for m in mons]
    monkeypatch.setattr(table_module, "_engine", refuse)
    for kwargs in ({"offsets": [-1.0, 0.0, 2.0]}, {"offsets": [-1.0, 0.0]}, {"weight": "none"}, {"centre": (0.0, 1e-3)}, {"monitors": mons[::-1]},
                   {"monitors": mons[:1]}, {"n_groups": 4}, {"n_groups": 2}):
        with pytest.raises(ValueError, match="into"):
            table.spots_grouped_all(segs, ids, **{"offsets": [-1.0, 0.0, 1.0], **kwargs}, into=first)
    for into in ([first[0], other[1]], first[::-1], first[:1], (first[0].counts, first[0].sums), [first[0], "spots"], plain):
        with pytest.raises(ValueError, match="into"):
            table.spots_grouped_all(segs, ids, offsets=[-1.0, 0.0, 1.0], into=into)


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table, segs = oa.OpticalTable(), support.host_segments()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6).RotZ(0.3)]
    table.add_monitors(mons)
    spots = table.spots_grouped_all(segs, [2, 0, 1, 0])
    assert rec.n == 2 and rec.weighted is True and rec.into is None and rec.n_groups == 3  # max id + 1
    assert rec.groups.dtype == torch.int32 and rec.groups.is_contiguous() and rec.groups.tolist() == [2, 0, 1, 0]
    np.testing.assert_array_equal(rec.offsets, [0.0])
    np.testing.assert_array_equal(rec.centre, np.zeros((2, 2)))
    np.testing.assert_array_equal(rec.axes, [np.concatenate([m.tangent_Y, m.tangent_Z]) for m in mons])  # the images' axes
    assert [s.monitor for s in spots] == mons and all(isinstance(s, oa.MonitorSpotGroups) for s in spots)
    assert all(s.weight == "intensity" and s.centre == (0.0, 0.0) and s.counts.shape == (1, 3) and s.sums.shape == (1, 3, 6) and s.n_groups == 3
               and s.labels is None for s in spots)
    # an n_groups below max id + 1 is no error: such ids are masked on the device, and handed over as they are — and so is -1
    for groups in ([5, 0, -1, 1], np.array([5, 0, -1, 1], dtype=np.int64), torch.tensor([5, 0, -1, 1], dtype=torch.int16)):
        got = table.spots_grouped_all(segs, groups, n_groups=2, labels=["red", "blue"])
        assert rec.n_groups == 2 and rec.groups.dtype == torch.int32 and rec.groups.tolist() == [5, 0, -1, 1]
        assert got[0].n_groups == 2 and got[0].labels == ["red", "blue"] and got[0].counts.shape == (1, 2)
    table.spots_grouped_all(segs, [-1, -1, -1, -1])  # all masked: one group, which nobody is in
    assert rec.n_groups == 1
    spots = table.spots_grouped_all(segs, [0, 1, 0, 1], offsets=np.linspace(-1, 1, 5), weight="none", centre=[(0.1, 0.2), (0.3, 0.4)], monitors=mons[::-1])
    assert rec.weighted is False and rec.centre.tolist() == [[0.1, 0.2], [0.3, 0.4]] and len(rec.offsets) == 5
    assert spots[0].monitor is mons[1] and spots[0].centre == (0.1, 0.2) and spots[1].centre == (0.3, 0.4) and spots[0].weight == "none"
    again = table.spots_grouped_all(segs, [1, 1, 0, 0], offsets=np.linspace(-1, 1, 5), weight="none", centre=[(0.1, 0.2), (0.3, 0.4)], monitors=mons[::-1],
                                    into=spots)  # the id table is the chunk's own
    assert all(a is b for a, b in zip(again, spots)) and rec.into[0] is spots[0]._stack[0] and int(spots[1].counts[0, 0]) == 1
    assert rec.groups.tolist() == [1, 1, 0, 0]
    one = table.spots_grouped_batch(mons[1], segs, [0, 1, 0, 1], offsets=[0.0, 0.5], labels=(1, 2))
    assert rec.n == 1 and one.monitor is mons[1] and one.offsets.tolist() == [0.0, 0.5] and one.labels == [1, 2]
    counts, sums, offsets = one.to_host()
    assert counts.dtype == np.int64 and counts.shape == (2, 2) and sums.shape == (2, 2, 6) and offsets is one.offsets


def test_spot_group_ids():
    from optable_amd.spots import spot_group_ids

    ids, G = spot_group_ids(np.array([3, 0, 3, 1], dtype=np.uint8), 4)
    assert G == 4 and ids.dtype == torch.int32 and ids.tolist() == [3, 0, 3, 1]
    ids, G = spot_group_ids(torch.tensor([3, 0, 3, 1]), None, 2)
    assert G == 2 and ids.tolist() == [3, 0, 3, 1]
    own = torch.tensor([1, 0], dtype=torch.int32)
    assert spot_group_ids(own, 2)[0].data_ptr() == own.data_ptr()  # what is already as the engine takes it is not copied
    assert spot_group_ids([0] * 7, 7, 256)[1] == 256
    with pytest.raises(ValueError, match="32 bits"):
        spot_group_ids(np.array([0, 1 << 31]), 2, 1)


def _sums_of(w, y, z):
    return [w.sum(), (w * y).sum(), (w * z).sum(), (w * y * y).sum(), (w * z * z).sum(), (w * y * z).sum()]


def test_groups_on_hand_made_sums():
    rng = np.random.default_rng(5)
    J, G = 2, 3
    offsets = np.array([0.0, 1.0])
    counts = np.array([[40, 0, 7], [12, 30, 1]])
    sums = np.zeros((J, G, 6))
    for j in range(J):
        for g in range(G):
            c = counts[j, g]
            if c:
                sums[j, g] = _sums_of(0.25 + rng.random(c), rng.normal(0.3 * g, 0.1, c) - 0.25, rng.normal(-0.2, 0.05 * (j + 1), c) + 0.25)
    grouped = oa.MonitorSpotGroups(None, offsets, torch.tensor(counts), torch.tensor(sums), "intensity", (0.25, -0.25), labels=[780, 560, 400])
    assert grouped.n_groups == G and grouped.labels == [780, 560, 400] and grouped.centre == (0.25, -0.25)
    for g in range(G):
        sp = grouped.group(g)
        want = oa.MonitorSpots(None, offsets, torch.tensor(counts[:, g]), torch.tensor(sums[:, g]), "intensity", (0.25, -0.25))
        assert isinstance(sp, oa.MonitorSpots) and sp.centre == want.centre and sp.weight == "intensity" and sp.offsets is offsets
        assert torch.equal(sp.counts, want.counts) and torch.equal(sp.sums, want.sums)
        for name in ("power", "centroid", "covariance", "rms_y", "rms_z", "rms_radius"):
            a, b = getattr(sp, name)(), getattr(want, name)()
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), (g, name)
        # ... and the [J, G] forms are the groups' side by side
        for name in ("power", "centroid", "rms_radius"):
            a, b = getattr(grouped, name)()[:, g], getattr(want, name)()
            assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b)), (g, name)
    assert tuple(grouped.power().shape) == (J, G) and tuple(grouped.centroid().shape) == (J, G, 2) and tuple(grouped.rms_radius().shape) == (J, G)
    assert torch.isnan(grouped.rms_radius()[0, 1]) and torch.isnan(grouped.centroid()[0, 1]).all() and float(grouped.power()[0, 1]) == 0.0
    total = grouped.total()
    assert isinstance(total, oa.MonitorSpots) and total.counts.tolist() == [47, 43] and total.counts.dtype == torch.int64
    np.testing.assert_allclose(total.sums.numpy(), sums.sum(axis=1), rtol=1e-15)
    grouped.counts[0, 1] += 5  # `group` gives views: what an `into=` call adds shows there
    assert int(grouped.group(1).counts[0]) == 5
    for g in (-1, 3):
        with pytest.raises(IndexError):
            grouped.group(g)
    with pytest.raises(ValueError, match="labels"):
        oa.MonitorSpotGroups(None, offsets, torch.tensor(counts), torch.tensor(sums), "intensity", (0, 0), labels=[1, 2])


def test_best_focus_per_group():
    # parabolas with different vertices and floors: var_y = floor + slope2 (x - vertex)^2, W = 1, a zero centroid and no z
    offsets = np.linspace(-0.5, 0.5, 11)
    vertex, floor, slope2 = np.array([-0.13, 0.0, 0.271, 0.9]), np.array([4e-6, 0.0, 1e-6, 0.0]), np.array([0.01, 0.02, 0.005, 0.01])
    G = len(vertex)
    sums = np.zeros((len(offsets), G, 6))
    sums[..., 0] = 1.0
    sums[..., 3] = floor + slope2 * (offsets[:, None] - vertex) ** 2
    counts = np.full((len(offsets), G), 5)
    grouped = oa.MonitorSpotGroups(None, offsets, torch.tensor(counts), torch.tensor(sums), "intensity", (0.0, 0.0))
    x, r = grouped.best_focus()
    assert isinstance(x, np.ndarray) and isinstance(r, np.ndarray) and x.shape == r.shape == (G,)
    np.testing.assert_allclose(x[:3], vertex[:3], atol=1e-12)
    np.testing.assert_allclose(r[:3], np.sqrt(floor[:3]), atol=1e-9)
    assert x[3] == 0.5 and abs(r[3] - 0.1 * 0.4) < 1e-15  # a vertex outside the scan: the sampled minimum at its end
    for g in range(G):
        want = oa.MonitorSpots(None, offsets, torch.tensor(counts[:, g]), torch.tensor(sums[:, g]), "intensity", (0.0, 0.0)).best_focus()
        assert (x[g], r[g]) == want
    counts[:, 1] = 1  # a group with fewer than two hits anywhere: NaN, the others as before
    x2, r2 = oa.MonitorSpotGroups(None, offsets, torch.tensor(counts), torch.tensor(sums), "intensity", (0.0, 0.0)).best_focus()
    assert np.isnan(x2[1]) and np.isnan(r2[1]) and x2[0] == x[0] and x2[2] == x[2]


def test_groups_by_wavelength():
    wl = np.array([560e-7, 780e-7, 400e-7, 780e-7, 400e-7, 560e-7, 560e-7])  # three wavelengths in scrambled order
    batch = RayBatch.from_arrays(np.zeros((7, 3)), np.tile([1.0, 0.0, 0.0], (7, 1)), wavelength=wl, device="cpu")
    ids, found = batch.groups_by_wavelength()
    assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.device == batch.wavelength.device and tuple(ids.shape) == (7,)
    assert found.tolist() == [400e-7, 560e-7, 780e-7] and ids.tolist() == [1, 2, 0, 2, 0, 1, 1]
    assert torch.equal(found[ids.long()], batch.wavelength)
    # multiplexed in wavelength: copy w of the batch is one group — group-major ids
    many = support.host_rays(5).multiplexed_in_wavelength([780e-7, 560e-7, 400e-7])
    ids, found = many.groups_by_wavelength()
    assert found.tolist() == [400e-7, 560e-7, 780e-7] and ids.tolist() == [2] * 5 + [1] * 5 + [0] * 5
    one, found = support.host_rays(3).groups_by_wavelength()
    assert one.tolist() == [0, 0, 0] and found.tolist() == [780e-7]


def test_a_biconvex_lens_of_a_glass():
    """examples/chromatic_focus.py builds its singlet of a Material: two faces, and the scene compiles."""
    glass = oa.Glass_NBK7()
    lens = oa.BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n=glass)
    assert len(lens.components) == 2 and glass.n(400e-9) > glass.n(780e-9)  # normal dispersion
    table = oa.OpticalTable()
    table.add_components([lens])
    assert table.compile() is not None
    with pytest.raises(AssertionError, match="n must be"):
        oa.BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n="glass")
