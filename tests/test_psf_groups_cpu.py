"""CPU: the diffraction PSF per ray group without a device — `MonitorPSFGroups` on hand-made tensors against a numpy restatement, the
planner `psf_groups_plan` against a brute-force one, what `OpticalTable.psf_grouped_all` refuses before the engine is asked, and
the binding's signature against the header.  No library call is made."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from optable_amd import abi, engine
from optable_amd import psf as psfm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = scenes.WL
T = engine.PSF_PART_TILE


def _header():
    return open(os.path.join(ROOT, "include", "optable_hip.h")).read()


def test_binding_matches_the_header():
    decl = re.search(r"int\s+ot_monitor_psf_groups_many\s*\(([^;]*)\)\s*;", _header())
    assert decl, "ot_monitor_psf_groups_many is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = abi.SYMBOLS["ot_monitor_psf_groups_many"]
    assert restype is C.c_int and len(argtypes) == len(params) == 29
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
    plain = [" ".join(p.split()).split()[-1].lstrip("*") for p in re.search(r"int\s+ot_monitor_psf_many\s*\(([^;]*)\)\s*;", _header()).group(1).split(",")]
    assert names == plain[:9] + ["groups", "n_group_ids", "n_groups"] + plain[9:-1] + ["ungrouped", "accumulate"]
    assert oa.MonitorPSFGroups is psfm.MonitorPSFGroups and callable(oa.OpticalTable.psf_grouped_all) and callable(oa.OpticalTable.psf_grouped_batch)
    assert callable(engine.Engine.monitor_psf_groups_many)


def test_constants():
    kernels = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    assert int(re.search(r"#define\s+OT_PSF_GROUP_CELLS_MAX\s+(\d+)", _header()).group(1)) == engine.PSF_GROUP_CELLS_MAX == 4096
    assert int(re.search(r"\bMON_PSF_PART_TILE\s*=\s*(\d+)", kernels).group(1)) == T
    threads = int(re.search(r"\bMON_THREADS\s*=\s*(\d+)", kernels).group(1))
    assert T % threads == 0 and T <= 2048
    assert int(re.search(r"\bMON_PSF_GROUPS_MAX\s*=\s*(\d+)", kernels).group(1)) == engine.SPOT_GROUPS_MAX


def _brute_plan(ny, nz, cell_hits, tile):
    """The rule in words: a partition tile is `tile` consecutive hits of one monitor (one tile for none); a cell's hits go to one more
    chunk for every 512, 256 at most; a launch takes as many (cell, pixel tile) pairs as keep its workgroups within 1024."""
    tiles_of = []
    for row in cell_hits:
        hits, count = sum(row), 0
        while count * tile < hits:
            count += 1
        tiles_of.append(max(count, 1))
    chunks = []
    for row in cell_hits:
        out = []
        for h in row:
            c = 1
            while c * 512 < h and c < 256:
                c += 1
            out.append(c)
        chunks.append(out)
    pixel_tiles = len(engine.psf_plan(ny, nz)["tiles"])
    pairs = sum(len(row) for row in cell_hits) * pixel_tiles
    most = max(c for row in chunks for c in row)
    a_launch = 1
    while a_launch < pairs and (a_launch + 1) * most <= 1024:
        a_launch += 1
    launches = 0
    while launches * a_launch < pairs:
        launches += 1
    return {"partition_tiles": tiles_of, "chunks": chunks, "pairs_a_launch": a_launch, "launches": launches}


def test_planner_against_a_restatement():
    edge = [0, 1, 511, 512, 513, T, T + 1]
    for ny, nz in ((1, 1), (33, 17), (65, 65), (129, 70)):
        for cell_hits in ([edge], [[h] for h in edge], [edge, edge[::-1]], [[0, 0], [T, T + 1], [3, 200_000]], [[1] * 256] * 2):
            for tile in (T, 256):
                assert engine.psf_groups_plan(ny, nz, cell_hits, tile=tile) == _brute_plan(ny, nz, cell_hits, tile), (ny, nz, cell_hits, tile)
    plan = engine.psf_groups_plan(65, 65, [[2] * 256] * 2)
    assert plan["pairs_a_launch"] == 1024 and plan["launches"] == 2 and plan["partition_tiles"] == [1, 1]
    assert engine.psf_groups_plan(65, 65, np.array([[T - 1, 1, 1]]))["partition_tiles"] == [2]
    for bad in ([[1] * 257], [[1] * 256] * 17, [[1, 2], [3]], [[]]):
        with pytest.raises(ValueError):
            engine.psf_groups_plan(5, 5, bad)
    with pytest.raises(ValueError):
        engine.psf_groups_plan(512, 512, [[1] * 256] * 3)  # 3 x 256 x 2^18 samples
    with pytest.raises(ValueError):
        engine.psf_groups_plan(0, 5, [[1]])


def test_refused_before_the_engine_is_asked(monkeypatch):
    from optable_amd import table as table_module

    def refuse():
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(table_module, "_engine", refuse)
    table, segs = oa.OpticalTable(), support.host_segments()  # four rays
    table.add_monitors([oa.Monitor([7.5, 0, 0], 6, 6), oa.Monitor([8.5, 0, 0], 6, 6)])
    good, ids = dict(direction=(1, 0, 0), step=1e-5), [0, 1, 0, 1]
    with pytest.raises(ValueError, match="exactly one"):
        table.psf_grouped_all(segs, WL, ids, step=1e-5)
    with pytest.raises(ValueError, match="step"):
        table.psf_grouped_all(segs, WL, ids, direction=(1, 0, 0))
    with pytest.raises(ValueError, match="pixels"):
        table.psf_grouped_all(segs, WL, ids, pixels=513, **good)
    with pytest.raises(ValueError, match="amplitude"):
        table.psf_grouped_all(segs, WL, ids, amplitude="power", **good)
    for groups in ([0, 1, 0], [0.0, 1.0, 0.0, 1.0], "abcd", [[0, 1], [0, 1]], torch.zeros(4), []):
        with pytest.raises(ValueError, match="groups"):
            table.psf_grouped_all(segs, WL, groups, **good)
    for n_groups in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="n_groups"):
            table.psf_grouped_all(segs, WL, ids, n_groups=n_groups, **good)
    with pytest.raises(ValueError, match="labels"):
        table.psf_grouped_all(segs, WL, ids, labels=["red"], **good)
    for wavelength in (0.0, -WL, np.nan, "red", None):
        with pytest.raises(ValueError, match="wavelength"):
            table.psf_grouped_all(segs, wavelength, ids, **good)
    with pytest.raises(ValueError, match="double-precision"):
        table.psf_grouped_all(support.host_segments(precision="f32"), WL, ids, **good)
    with pytest.raises(AssertionError, match="the engine was asked for"):
        table.psf_grouped_all(segs, WL, ids, **good)
    with pytest.raises(AssertionError, match="the engine was asked for"):
        table.psf_grouped_all(segs, WL, [-1, 5, 0, 1], n_groups=2, labels=["red", "blue"], **good)  # ids outside 0 .. G - 1 mask, they are no error


# -- MonitorPSFGroups on hand-made tensors ----------------------------------------------------------------------------------------
STEPS, NORMS = (0.5, 0.25), (4.0, 2.5, 0.0)


def _made(fields=None, norms=NORMS, labels=None, centre=(0.0, 0.0)):
    rng = np.random.default_rng(5)
    if fields is None:
        fields = rng.normal(size=(3, 9, 11)) + 1j * rng.normal(size=(3, 9, 11))
        fields[2] = 0.0  # a group without a hit
    fields = np.asarray(fields, dtype=np.complex128)
    G, ny, nz = fields.shape
    grid = (centre[0] - (ny - 1) / 2 * STEPS[0], STEPS[0], centre[1] - (nz - 1) / 2 * STEPS[1], STEPS[1])
    counts = torch.tensor([[7, 1, 0], [5, 0, 2], [0, 0, 0]][:G], dtype=torch.int64)
    return fields, oa.MonitorPSFGroups(None, counts, torch.tensor(norms[:G], dtype=torch.float64), torch.tensor(fields.real.copy()),
                                       torch.tensor(fields.imag.copy()), torch.tensor(4, dtype=torch.int64), ("focus", (1.0, 2.0, 3.0)), grid, STEPS, centre,
                                       "sqrt", labels=labels)


def test_groups_are_views_and_the_coherent_sum():
    fields, p = _made(labels=[400, 560, 780])
    assert p.n_groups == 3 and p.labels == [400, 560, 780] and int(p.ungrouped) == 4
    assert p.counts.tolist() == [7, 5, 0] and p.skipped.tolist() == [1, 0, 0] and p.aliased.tolist() == [0, 2, 0]
    assert p.reference == ("focus", (1.0, 2.0, 3.0)) and p.step == STEPS and p.amplitude == "sqrt" and len(p.y) == 9 and len(p.z) == 11 and abs(p.y[4]) < 1e-15
    for g in range(3):
        one = p.group(g)
        assert isinstance(one, oa.MonitorPSF) and one.re.data_ptr() == p.re[g].data_ptr() and one.im.data_ptr() == p.im[g].data_ptr()
        assert one.norm.data_ptr() == p.norm[g].data_ptr() and (int(one.counts), int(one.skipped), int(one.aliased)) == (
            int(p.counts[g]), int(p.skipped[g]), int(p.aliased[g]))
        np.testing.assert_array_equal(one.y, p.y)
        assert one.step == p.step and one.reference == p.reference and one.extent == p.extent
    np.testing.assert_allclose(p.group(0).normalised().numpy(), np.abs(fields[0]) ** 2 / 16.0, rtol=1e-14)
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            p.group(bad)
    whole = p.coherent()
    assert isinstance(whole, oa.MonitorPSF) and (int(whole.counts), int(whole.skipped), int(whole.aliased)) == (12, 1, 2) and float(whole.norm) == 6.5
    np.testing.assert_allclose(whole.field.numpy(), fields.sum(axis=0), rtol=1e-14)
    used, skipped, aliased, norm, field, ungrouped = p.to_host()
    assert used.tolist() == [7, 5, 0] and skipped.tolist() == [1, 0, 0] and aliased.tolist() == [0, 2, 0] and norm.tolist() == list(NORMS) and ungrouped == 4
    np.testing.assert_array_equal(field, fields)
    with pytest.raises(ValueError, match="labels"):
        _made(labels=[400, 560])


@pytest.mark.parametrize("weights", [None, (1.0, 0.25, 3.0), (0.0, 2.0, 0.0)])
def test_the_incoherent_sum_against_numpy(weights):
    fields, p = _made()
    w = np.ones(3) if weights is None else np.asarray(weights)
    I = np.tensordot(w, np.abs(fields) ** 2, axes=1)
    d = float((w * np.asarray(NORMS) ** 2).sum())
    np.testing.assert_allclose(p.intensity(weights).numpy(), I, rtol=1e-14)
    np.testing.assert_allclose(p.normalised(weights).numpy(), I / d, rtol=1e-14)
    assert abs(float(p.strehl(weights=weights)) - I[4, 5] / d) <= 1e-14 * I[4, 5] / d
    assert abs(float(p.strehl("peak", weights=weights)) - I.max() / d) <= 1e-14 * I.max() / d
    mtf, fy, fz = p.mtf(weights)
    np.testing.assert_allclose(mtf, np.abs(np.fft.fftshift(np.fft.fft2(I))) / I.sum(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(fy, np.fft.fftshift(np.fft.fftfreq(9, STEPS[0])))
    np.testing.assert_allclose(fz, np.fft.fftshift(np.fft.fftfreq(11, STEPS[1])))
    assert abs(mtf[4, 5] - 1.0) < 1e-14
    radii = np.array([0.3, 0.8, 1.5, 10.0])
    for about in ("centroid", "reference"):
        cy, cz = (0.0, 0.0) if about == "reference" else ((I.sum(axis=1) @ p.y) / I.sum(), (I.sum(axis=0) @ p.z) / I.sum())
        r = np.hypot(p.y[:, None] - cy, p.z[None, :] - cz)
        np.testing.assert_allclose(p.encircled_energy(radii, about=about, weights=weights), [I[r <= rad].sum() / I.sum() for rad in radii], rtol=1e-13)
    assert p.encircled_energy(10.0, weights=weights)[0] == pytest.approx(1.0)


def test_strehl_per_group_and_perfect_groups():
    fields, p = _made()
    s = p.strehls()
    assert s.shape == (3,) and abs(float(s[0]) - abs(fields[0][4, 5]) ** 2 / 16.0) < 1e-14 and torch.isnan(s[2])  # a group without a hit: NaN
    assert torch.equal(p.strehls("peak")[:2], torch.stack([p.group(g).strehl("peak") for g in range(2)]))
    # every group perfect: |U_g| = norm_g on the reference, whatever the weights
    perfect = np.zeros((2, 3, 3), dtype=np.complex128)
    perfect[0, 1, 1], perfect[1, 1, 1] = 4.0j, -2.5
    _, q = _made(perfect, norms=(4.0, 2.5))
    for weights in (None, (0.2, 5.0)):
        assert float(q.strehl(weights=weights)) == pytest.approx(1.0, abs=1e-15) and float(q.normalised(weights)[1, 1]) == pytest.approx(1.0, abs=1e-15)
    assert q.strehls().tolist() == [1.0, 1.0]


def test_nan_rules_and_refusals():
    fields, p = _made()
    dark = (0.0, 0.0, 1.0)  # only the group without a hit counts: the denominator is 0
    assert torch.isnan(p.normalised(dark)).all() and np.isnan(float(p.strehl(weights=dark))) and np.isnan(float(p.strehl("peak", weights=dark)))
    assert np.isnan(p.mtf(dark)[0]).all() and np.isnan(p.encircled_energy([1.0], weights=dark)).all()
    assert not torch.isnan(p.intensity(dark)).any() and not p.intensity(dark).any()
    _, none = _made(np.zeros((2, 3, 3)), norms=(0.0, 0.0))
    assert torch.isnan(none.normalised()).all() and np.isnan(float(none.strehl())) and torch.isnan(none.strehls()).all() and np.isnan(none.mtf()[0]).all()
    for weights in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, -0.5, 1.0), (1.0, np.nan, 1.0), "rgb", 2.0):
        for method in (p.intensity, p.normalised, p.mtf, lambda weights: p.strehl(weights=weights), lambda weights: p.encircled_energy([1.0], weights=weights)):
            with pytest.raises(ValueError, match="weights"):
                method(weights)
    with pytest.raises(ValueError, match="at must be"):
        p.strehl("middle")
    with pytest.raises(ValueError, match="about"):
        p.encircled_energy([1.0], about="edge")
    _, off = _made(centre=(0.1, 0.0))
    with pytest.raises(ValueError, match="no sample lies on the reference"):
        off.strehl()
    assert float(off.strehl("peak")) > 0.0
