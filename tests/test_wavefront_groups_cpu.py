"""CPU: the public surface of wavefront error per ray group (`OpticalTable.wavefront_grouped_all` / `wavefront_grouped_batch`,
`MonitorWavefrontGroups`: the 61 moments of every (monitor, group) of input rays, summed on the device,
ot_monitor_wavefront_groups_many) — the calls and the binding, the planner and its constants, the shape rules of the per-cell
tables, what is refused before the engine is asked, what is handed over, and the arithmetic of `MonitorWavefrontGroups` on sums
that tests/wavefront_reference.py makes of synthetic hits with known Zernike content.  No library call is made."""
import math
import os
import re

import numpy as np
import pytest
import torch

import optable_amd as oa
import support
from optable_amd import abi
from optable_amd.engine import Engine
from optable_amd.wavefront import zernike
from wavefront_reference import wavefront_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_calls_exist():
    from optable_amd import engine, wavefront

    assert callable(oa.OpticalTable.wavefront_grouped_all) and callable(oa.OpticalTable.wavefront_grouped_batch)
    assert callable(Engine.monitor_wavefront_groups_many) and callable(engine.wavefront_groups_plan)
    assert oa.MonitorWavefrontGroups is wavefront.MonitorWavefrontGroups
    for name in ("group", "coefficients", "rms", "strehl", "mean", "power", "to_host"):
        assert callable(getattr(wavefront.MonitorWavefrontGroups, name)), name
    assert "ot_monitor_wavefront_groups_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = _header()
    decl = re.search(r"\bint\s+ot_monitor_wavefront_groups_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_wavefront_groups_many is not declared in the header"
    names = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "mons", "n_monitors", "axes", "reference_kind", "reference", "coordinates", "pupil", "piston", "groups", "n_group_ids",
                     "n_groups", "src", "intensity", "n_index", "pathlength", "n_segments", "seg_count", "n_rays", "counts", "sums", "accumulate"]
    restype, argtypes = abi.SYMBOLS["ot_monitor_wavefront_groups_many"]
    assert restype is C.c_int and len(argtypes) == len(names) == 22
    widths = {"n_monitors": C.c_int32, "reference_kind": C.c_int32, "coordinates": C.c_int32, "n_groups": C.c_int32, "accumulate": C.c_int32,
              "n_group_ids": C.c_int64, "n_segments": C.c_int64, "n_rays": C.c_int64}
    types = dict(zip(names, [a.strip().rsplit(None, 1)[0] + ("*" if "*" in a else "") for a in decl.group(1).split(",")]))
    for name, kind in zip(names, argtypes):  # pointers as pointers, the integers by their width — the binding's and the header's
        assert kind is widths[name] if name in widths else kind not in (C.c_int32, C.c_int64, C.c_double), name
        if name in widths:
            assert types[name] == {C.c_int32: "int32_t", C.c_int64: "int64_t"}[widths[name]], (name, types[name])
        else:
            assert "*" in types[name], (name, types[name])
    assert abi.ABI_VERSION == 14  # an added function breaks no client
    assert re.search(r"#define\s+OT_ABI_VERSION\s+14\b", text)
    # the arguments the grouped call shares with ot_monitor_wavefront_many are that call's, in its order
    plain = abi.SYMBOLS["ot_monitor_wavefront_many"][1]
    assert argtypes[:9] == plain[:9] and argtypes[12:] == plain[9:]
    assert argtypes[9:12] == abi.SYMBOLS["ot_monitor_spot_groups_many"][1][7:10]  # groups, n_group_ids, n_groups as the spot groups'


def test_planner_and_its_constants():
    from optable_amd import engine

    kernels = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    found = re.search(r"\bMON_WAVEFRONT_CELLS\s*=\s*(\d+)", kernels)
    assert found and int(found.group(1)) == engine.WAVEFRONT_MONITORS == 28
    define = re.search(r"#define\s+OT_WAVEFRONT_GROUP_CELLS_MAX\s+(\d+)\b", _header())
    assert define and int(define.group(1)) == engine.WAVEFRONT_GROUP_CELLS_MAX == 4096
    assert engine.wavefront_groups_plan(1, 1) == [(0, 1)]
    assert engine.wavefront_groups_plan(1, 28) == [(0, 28)] == engine.wavefront_plan(28)
    assert engine.wavefront_groups_plan(1, 29) == [(0, 28), (28, 1)]
    assert engine.wavefront_groups_plan(6, 5) == [(0, 28), (28, 2)]  # monitor 5 is split between the two launches
    assert engine.wavefront_groups_plan(3, 28) == [(0, 28), (28, 28), (56, 28)]
    assert engine.wavefront_groups_plan(1, 256) == [(28 * k, 28) for k in range(9)] + [(252, 4)]
    for M, G in ((1, 8), (1, 64), (16, 256), (4096, 1), (7, 13)):
        plan = engine.wavefront_groups_plan(M, G)
        assert len(plan) == math.ceil(M * G / 28) and sum(cells for _, cells in plan) == M * G  # ceil(M G / 28) passes
        assert plan == engine.wavefront_plan(M * G)  # a window is 28 consecutive cells wherever a monitor begins
    for M, G in ((1, 0), (1, -1), (1, 257), (0, 1), (17, 256), (4097, 1), (2, 2049)):
        with pytest.raises(ValueError):
            engine.wavefront_groups_plan(M, G)


def test_shape_rules_of_the_tables():
    from optable_amd.wavefront import wavefront_group_piston, wavefront_group_pupil, wavefront_group_reference

    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0.5, 0], 6, 4).RotZ(0.3)]
    M, G = 2, 3
    one, per_m, per_g = np.array([1.0, 2.0, 3.0]), np.arange(6.0).reshape(2, 3) + 1, np.arange(9.0).reshape(3, 3) + 1
    per_cell = np.arange(18.0).reshape(2, 3, 3) + 1
    kind, lab, local = wavefront_group_reference(one, None, mons, G)
    assert kind == 0 and lab.shape == local.shape == (M, G, 3) and (lab == one).all()
    assert (wavefront_group_reference(per_m, None, mons, G)[1] == per_m[:, None, :]).all()
    assert (wavefront_group_reference(per_g, None, mons, G)[1] == per_g[None, :, :]).all()
    assert (wavefront_group_reference(per_cell, None, mons, G)[1] == per_cell).all()
    # local is what the ungrouped helper gives for the same vector and monitor, bit for bit
    from optable_amd.wavefront import wavefront_reference as plain_reference

    for k_name, kw in (("focus", 0), ("direction", 1)):
        kind, lab, local = wavefront_group_reference(per_cell if kw == 0 else None, per_cell if kw == 1 else None, mons, G)
        assert kind == kw
        for g in range(G):
            _, lab_p, local_p = plain_reference(per_cell[:, g] if kw == 0 else None, per_cell[:, g] if kw == 1 else None, mons)
            assert np.array_equal(lab[:, g], lab_p) and np.array_equal(local[:, g], local_p), (k_name, g)
    # M == G: a [M, 3] table could be either and is read as per MONITOR
    square = np.arange(6.0).reshape(2, 3) + 1
    assert (wavefront_group_reference(square, None, mons, 2)[1] == square[:, None, :]).all()
    assert (wavefront_group_pupil(square, 0, mons, 2) == square[:, None, :]).all()
    assert (wavefront_group_piston([5.0, 6.0], 2, 2) == [[5.0, 5.0], [6.0, 6.0]]).all()
    assert (wavefront_group_piston([5.0, 6.0, 7.0], 2, 3) == [[5.0, 6.0, 7.0]] * 2).all()  # M != G: per group
    assert (wavefront_group_piston(1.5, 2, 3) == 1.5).all() and wavefront_group_piston(np.ones((2, 3)), 2, 3).shape == (2, 3)
    # with three monitors three numbers are one vector for all, as for wavefront_all
    three = mons + [oa.Monitor([9.5, 0, 0], 6, 6)]
    assert (wavefront_group_reference(one, None, three, 2)[1] == one).all()
    pupil = wavefront_group_pupil(None, 1, mons, G)  # a plane wave: the largest circle of every monitor, for all its groups
    assert pupil.shape == (M, G, 3) and pupil[0].tolist() == [[0.0, 0.0, 3.0]] * G and pupil[1].tolist() == [[0.0, 0.0, 2.0]] * G
    assert all(t.flags["C_CONTIGUOUS"] for t in (lab, local, pupil))
    with pytest.raises(ValueError, match="pupil"):
        wavefront_group_pupil(None, 0, mons, G)
    for bad in (np.ones((4, 3)), np.ones((3, 2, 3)), np.ones(4), [1.0, np.nan, 0.0], "here", np.ones((2, 3, 3, 1))):
        with pytest.raises(ValueError, match="focus"):
            wavefront_group_reference(bad, None, mons, G)
    with pytest.raises(ValueError, match="exactly one"):
        wavefront_group_reference(one, one, mons, G)
    with pytest.raises(ValueError, match="direction"):
        wavefront_group_reference(None, [[1, 0, 0], [0, 0, 0], [0, 1, 0]], mons, G)
    for bad in ([0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [[0, 0, 1], [0, 0, 1], [0, 0, 0]], np.ones((2, 2, 3))):
        with pytest.raises(ValueError, match="pupil"):
            wavefront_group_pupil(bad, 0, mons, G)
    for bad in ([1.0, 2.0, 3.0, 4.0], np.inf, "p", np.ones((3, 2))):
        with pytest.raises(ValueError, match="piston"):
            wavefront_group_piston(bad, M, G)


class _Recorder:
    """Stands in for the engine: keeps what wavefront_grouped_all hands over; sums[..., 0] = 2 and sums[..., 45] = 3 (a mean W of 1.5)
    except in cell (0, 0), which is empty."""

    calls = 0

    def monitor_wavefront_groups_many(self, mons, axes, kind, reference, coordinates, pupil, piston, groups, n_groups, segs, weighted=True, into=None):
        self.calls += 1
        self.axes, self.kind, self.reference, self.coordinates, self.pupil, self.piston = axes, kind, reference, coordinates, pupil, np.array(piston)
        self.groups, self.n_groups, self.weighted, self.into, self.n = groups, n_groups, weighted, into, len(mons)
        if into is not None:
            into[0].add_(1)
            return into
        sums = torch.zeros((len(mons), n_groups, 61), dtype=torch.float64)
        sums[..., 0], sums[..., 45] = 2.0, 3.0
        sums[0, 0] = 0.0
        return torch.zeros((len(mons), n_groups, 2), dtype=torch.int64), sums


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table, segs = oa.OpticalTable(), support.host_segments()  # 4 rays
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6)]
    table.add_monitors(mons)
    ids, u = [0, 1, 2, 1], (1.0, 0.0, 0.0)
    for groups in ([0, 1, 2], [], [[0, 1], [2, 1]], None, [0.0, 1.0, 2.0, 1.0], [True, False, True, False]):
        with pytest.raises(ValueError, match="groups"):
            table.wavefront_grouped_all(segs, groups, direction=u)
    for n_groups in (0, -1, 257, 2.0, True):
        with pytest.raises(ValueError, match="n_groups"):
            table.wavefront_grouped_all(segs, ids, n_groups=n_groups, direction=u)
    with pytest.raises(ValueError, match="no wavefront of 17 monitors x 256 groups"):
        table.wavefront_grouped_all(segs, ids, n_groups=256, direction=u, monitors=[mons[0]] * 17)
    with pytest.raises(ValueError, match="weight"):
        table.wavefront_grouped_all(segs, ids, direction=u, weight="power")
    with pytest.raises(ValueError, match="labels"):
        table.wavefront_grouped_all(segs, ids, direction=u, labels=[1, 2])
    with pytest.raises(ValueError, match="exactly one"):
        table.wavefront_grouped_all(segs, ids)
    with pytest.raises(ValueError, match="pupil"):
        table.wavefront_grouped_all(segs, ids, focus=(0, 0, 0))
    with pytest.raises(ValueError, match="pupil"):
        table.wavefront_grouped_all(segs, ids, direction=u, pupil=np.ones((4, 3)))
    with pytest.raises(ValueError, match="coordinates"):
        table.wavefront_grouped_all(segs, ids, direction=u, coordinates="pupil")
    with pytest.raises(ValueError, match="piston"):
        table.wavefront_grouped_all(segs, ids, direction=u, piston=[1.0] * 4)
    with pytest.raises(ValueError, match="wavefront_all needs a double-precision SegmentBatch"):
        table.wavefront_grouped_all(support.host_segments(precision="f32"), ids, direction=u)
    with pytest.raises(AssertionError, match="the engine was asked for"):
        table.wavefront_grouped_all(segs, ids, direction=u, piston=0.0)
    # `into`: the list of ONE earlier call for the same monitors, G, references, pupils, coordinates and weight
    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    kw = dict(direction=np.array([[1.0, 0, 0], [1.0, 0.1, 0], [1.0, 0, 0.1]]), pupil=(0.0, 0.0, 2.0), piston=[1.0, 2.0, 3.0])
    first, other = table.wavefront_grouped_all(segs, ids, **kw), table.wavefront_grouped_all(segs, ids, **kw)
    plain = [oa.MonitorWavefront(m, torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64), torch.zeros(61, dtype=torch.float64),
                                 ("direction", u), (0, 0, 2.0), "position", 1.0, "intensity") for m in mons]
    monkeypatch.setattr(table_module, "_engine", refuse)
    for change in ({"direction": kw["direction"][::-1]}, {"pupil": (0.0, 0.0, 2.5)}, {"weight": "none"}, {"coordinates": "direction"}, {"monitors": mons[::-1]},
                   {"monitors": mons[:1]}, {"piston": [1.0, 2.0, 3.5]}, {"piston": 1.0}):
        with pytest.raises(ValueError, match="into"):
            table.wavefront_grouped_all(segs, ids, **{**kw, **change}, into=first)
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    uniform = table.wavefront_grouped_all(segs, ids, direction=u, piston=1.0)  # one reference for all: G alone can differ
    monkeypatch.setattr(table_module, "_engine", refuse)
    for n_groups in (4, 2):
        with pytest.raises(ValueError, match="into"):
            table.wavefront_grouped_all(segs, ids, direction=u, piston=1.0, n_groups=n_groups, into=uniform)
    with pytest.raises(ValueError, match="into"):
        table.wavefront_grouped_all(segs, ids, focus=(0, 0, 0), pupil=(0.0, 0.0, 2.0), coordinates="position", into=first)
    for into in ([first[0], other[1]], first[::-1], first[:1], (first[0].counts, first[0].sums), plain):
        with pytest.raises(ValueError, match="into"):
            table.wavefront_grouped_all(segs, ids, **kw, into=into)


def test_what_is_handed_over_and_what_comes_back(monkeypatch):
    from optable_amd import table as table_module

    rec = _Recorder()
    monkeypatch.setattr(table_module, "_engine", lambda: rec)
    table, segs = oa.OpticalTable(), support.host_segments()
    mons = [oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 4).RotZ(0.3)]
    table.add_monitors(mons)
    focus = np.array([[10.0, 0.0, 0.0], [10.0, 0.1, 0.0], [10.0, 0.0, 0.1]])  # per group: M = 2, G = 3
    wfs = table.wavefront_grouped_all(segs, [2, 0, 1, 0], focus=focus, pupil=(0.0, 0.0, 0.1), piston=[[1, 2, 3], [4, 5, 6]], labels=[4e-5, 5e-5, 6e-5])
    assert rec.calls == 1 and rec.n == 2 and rec.weighted is True and rec.into is None and rec.n_groups == 3 and rec.kind == 0 and rec.coordinates == 0
    assert rec.groups.dtype == torch.int32 and rec.groups.is_contiguous() and rec.groups.tolist() == [2, 0, 1, 0]
    assert rec.reference.shape == rec.pupil.shape == (2, 3, 3) and rec.piston.tolist() == [[1, 2, 3], [4, 5, 6]]
    np.testing.assert_array_equal(rec.axes, [np.concatenate([m.tangent_Y, m.tangent_Z]) for m in mons])
    np.testing.assert_allclose(rec.reference[0], focus - [7.5, 0, 0], atol=1e-15)  # the focus in monitor 0's frame (its axes are the lab's)
    R = np.asarray(mons[1].transform_matrix, dtype=float).reshape(3, 3)
    np.testing.assert_allclose(rec.reference[1], (focus - np.asarray(mons[1].origin, dtype=float)) @ R, atol=1e-14)
    assert [wf.monitor for wf in wfs] == mons and all(isinstance(wf, oa.MonitorWavefrontGroups) for wf in wfs)
    for k, wf in enumerate(wfs):
        assert wf.n_groups == 3 and wf.labels == [4e-5, 5e-5, 6e-5] and wf.weight == "intensity" and wf.coordinates == "direction"
        assert wf.counts.shape == wf.outside.shape == (3,) and wf.sums.shape == (3, 61) and wf.reference[0] == "focus"
        assert np.array_equal(wf.reference[1], focus) and np.array_equal(wf.pupil, [[0.0, 0.0, 0.1]] * 3) and wf.piston.tolist() == [[1, 2, 3], [4, 5, 6]][k]
        one = wf.group(1)
        assert isinstance(one, oa.MonitorWavefront) and one.reference == ("focus", (10.0, 0.1, 0.0)) and one.piston == [2.0, 5.0][k] and one.pupil == (0.0, 0.0, 0.1)
    # piston=None: the pass with piston 0, then the sums about every cell's mean T00 / S00 — 0 for the empty cell
    rec.calls = 0
    wfs = table.wavefront_grouped_all(segs, [0, 1, 0, 1], direction=(1.0, 0.0, 0.0), weight="none")
    assert rec.calls == 2 and rec.weighted is False and rec.kind == 1 and rec.coordinates == 1 and rec.n_groups == 2
    assert rec.piston.tolist() == [[0.0, 1.5], [1.5, 1.5]] and wfs[0].piston.tolist() == [0.0, 1.5] and wfs[1].piston.tolist() == [1.5, 1.5]
    assert rec.pupil.tolist() == [[[0.0, 0.0, 3.0]] * 2, [[0.0, 0.0, 2.0]] * 2]
    # into=: the earlier call's pistons and this call's ids
    again = table.wavefront_grouped_all(segs, [1, 1, 0, 0], direction=(1.0, 0.0, 0.0), weight="none", into=wfs)
    assert rec.calls == 3 and all(a is b for a, b in zip(again, wfs)) and rec.into[0] is wfs[0]._stack[0] and rec.groups.tolist() == [1, 1, 0, 0]
    assert rec.piston.tolist() == [[0.0, 1.5], [1.5, 1.5]] and int(wfs[1].counts[0]) == 1  # (the recorder added 1 to every count)
    table.wavefront_grouped_all(segs, [1, 1, 0, 0], direction=(1.0, 0.0, 0.0), weight="none", into=wfs, piston=[[0.0, 1.5], [1.5, 1.5]])
    one = table.wavefront_grouped_batch(mons[1], segs, [5, 0, -1, 1], n_groups=2, direction=(1.0, 0.0, 0.0), piston=0.0, labels=("a", "b"))
    assert rec.n == 1 and rec.groups.tolist() == [5, 0, -1, 1] and one.monitor is mons[1] and one.labels == ["a", "b"]
    inside, outside, sums = one.to_host()
    assert inside.dtype == outside.dtype == np.int64 and inside.shape == outside.shape == (2,) and sums.shape == (2, 61)


def _synthetic(n, seed, content, piston):
    """The sums wavefront_reference makes of `n` hits of a collimated bundle along x on a monitor at x = 1 (position coordinates,
    pupil (0, 0, 1)) whose path lengths carry W = sum content[j] Z_j: (the reference, the weighted rms of W about its mean)."""
    rng = np.random.default_rng(seed)
    r, phi = np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    y, z = r * np.cos(phi), r * np.sin(phi)
    W = sum(c * zernike(15, y, z)[j - 1] for j, c in content.items())
    o, d = np.stack([np.zeros(n), y, z], axis=1), np.tile([1.0, 0.0, 0.0], (n, 1))
    w = 0.5 + rng.random(n)
    ref = wavefront_reference(o, d, np.full(n, 2.0), w, np.ones(n), W - 1.0, np.eye(3).ravel(), [1.0, 0.0, 0.0], 3.0, 3.0,
                              [0.0, 1.0, 0.0, 0.0, 0.0, 1.0], 1, [1.0, 0.0, 0.0], 1, (0.0, 0.0, 1.0), piston)
    assert ref.counts.tolist() == [n, 0]
    mean = (w * W).sum() / w.sum()
    return ref, math.sqrt((w * (W - mean) ** 2).sum() / w.sum())


def test_groups_on_sums_of_known_zernike_content():
    """Three groups of a few hundred synthetic hits: defocus with tilt, coma with astigmatism, and an empty one."""
    content = [{1: 2.0, 2: 3e-4, 4: -5e-4}, {1: 2.5, 5: 1e-4, 8: 2e-4}, {}]
    piston = np.array([2.0, 2.4, 0.0])
    (ref0, rms0), (ref1, rms1) = _synthetic(400, 1, content[0], piston[0]), _synthetic(300, 2, content[1], piston[1])
    refs, direct = [ref0, ref1], [rms0, rms1]
    counts, sums = np.array([400, 300, 0]), np.stack([refs[0].sums, refs[1].sums, np.zeros(61)])
    wavelengths = [5e-3, 6e-3, 7e-3]
    wf = oa.MonitorWavefrontGroups(None, torch.tensor(counts), torch.zeros(3, dtype=torch.int64), torch.tensor(sums), ("direction", np.tile([1.0, 0, 0], (3, 1))),
                                   np.tile([0.0, 0.0, 1.0], (3, 1)), "position", piston, "intensity", labels=wavelengths)
    assert wf.n_groups == 3 and wf.labels == wavelengths and wf.piston.tolist() == piston.tolist()
    c = wf.coefficients().numpy()
    assert c.shape == (3, 15) and tuple(wf.coefficients(4).shape) == (3, 4) and tuple(wf.rms().shape) == (3,) and tuple(wf.mean().shape) == (3,)
    for g in range(2):
        want = np.zeros(15)
        for j, v in content[g].items():
            want[j - 1] = v
        np.testing.assert_allclose(c[g], want, atol=1e-12)
        one = wf.group(g)
        assert isinstance(one, oa.MonitorWavefront) and one.piston == piston[g] and one.sums.data_ptr() == wf.sums[g].data_ptr()  # a view
        assert torch.equal(one.coefficients(), wf.coefficients()[g]) and torch.equal(one.rms(4), wf.rms(4)[g]) and torch.equal(one.mean(), wf.mean()[g])
        assert abs(float(wf.rms(1)[g]) - direct[g]) < 1e-12  # the rms about the mean, formed from the hits themselves
        assert float(wf.rms(15)[g]) < 1e-9
        marechal = math.exp(-(2 * math.pi * float(one.rms()) / wavelengths[g]) ** 2)
        assert 0.3 < marechal < 0.99 and float(wf.strehl()[g]) == pytest.approx(marechal, rel=1e-13) == pytest.approx(float(one.strehl(wavelengths[g])), rel=1e-13)
    assert float(wf.rms(4)[0]) < 1e-9 < float(wf.rms(4)[1])  # tilt and defocus out: nothing is left of group 0
    assert torch.isnan(wf.coefficients()[2]).all() and torch.isnan(wf.rms()[2]) and torch.isnan(wf.strehl()[2]) and torch.isnan(wf.mean()[2])
    assert wf.power().tolist() == sums[:, 0].tolist()
    assert torch.allclose(wf.strehl(6e-3)[:2], torch.stack([wf.group(g).strehl(6e-3) for g in range(2)]), rtol=1e-13, atol=0)
    assert torch.equal(wf.strehl([5e-3, 6e-3, 7e-3])[:2], wf.strehl()[:2])
    wf.sums[2] += torch.tensor(refs[0].sums)  # `group` gives views: what an `into=` call adds shows there
    wf.counts[2] += 400
    np.testing.assert_allclose(wf.group(2).coefficients().numpy()[1:], c[0][1:], atol=1e-12)
    for g in (-1, 3):
        with pytest.raises(IndexError):
            wf.group(g)
    bare = oa.MonitorWavefrontGroups(None, torch.tensor(counts), torch.zeros(3, dtype=torch.int64), torch.tensor(sums), ("direction", np.tile([1.0, 0, 0], (3, 1))),
                                     np.tile([0.0, 0.0, 1.0], (3, 1)), "position", piston, "intensity")
    with pytest.raises(ValueError, match="labels"):
        bare.strehl()
    for bad in ([5e-3, 6e-3], 0.0, -1.0, "green"):
        with pytest.raises(ValueError, match="wavelength"):
            bare.strehl(bad)
    with pytest.raises(ValueError, match="labels"):
        oa.MonitorWavefrontGroups(None, torch.tensor(counts), torch.zeros(3, dtype=torch.int64), torch.tensor(sums), ("direction", np.zeros((3, 3))),
                                  np.ones((3, 3)), "position", piston, "intensity", labels=[1, 2])


def test_the_seeded_gpu_cases_keep_their_margins():
    """The cells of tests/test_gpu_wavefront_groups.py's first case through the C oracle's trace of the same seeded rays: the
    reference alone keeps every decision 1e-7 from its boundary (`cell_reference` asserts it), and every cell is hit."""
    import scenes
    import wavefront_cases as cases
    import wavefront_group_cases as gc
    from optable_amd.batch import RayBatch
    from oracle import oracle as orc

    table = support.cfg2_table()
    o, d, intensity = cases.cfg2_arrays(gc.RAYS, gc.SEED)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, intensity=intensity, q=support.Q, device="cpu")
    h = orc.trace(table.compile(), batch.to_host(), max_trace_num=gc.SEGMENTS)
    records = (np.stack([h["ox"], h["oy"], h["oz"]], 1), np.stack([h["dx"], h["dy"], h["dz"]], 1), h["length"], h["intensity"], h["n"], h["pathlength"])
    ray, ids = np.asarray(h["ray"], dtype=np.int64), gc.ids_of(gc.RAYS)
    assert set(ids.tolist()) == set(range(-1, gc.G + 1))
    for su in gc.SETUPS.values():
        mons = gc.monitors_at(su["x"])
        refs = gc.cell_references(records, ray, ids, mons, su["name"], su["reference"], su["pupil"], np.zeros((2, gc.G)), gc.G)
        assert all(ref.counts[0] > 400 for row in refs for ref in row) and refs[0][0].counts[1] > 0
        other = "position" if su["name"] == "focus" else "direction"
        refs = gc.cell_references(records, ray, ids, mons[:1], su["name"], su["reference"], [su["other"]], np.zeros((1, gc.G)), gc.G, coordinates=other)
        assert all(ref.counts[0] > 400 for ref in refs[0])
