"""CPU: the wavefront surface without a device — the calls, the binding against the header, the planner and its constant, every
refusal raised before the engine is asked, the Noll tables against the closed-form disc integrals, the arithmetic of
`MonitorWavefront` on hand-made sums, the reference on hand-made segments, and the margins of the seeded cases the GPU tests run
(through the C oracle's trace of the same rays)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import optable_amd as oa
import support
import wavefront_cases as cases
from optable_amd import abi, engine, table as table_module
from optable_amd import wavefront as wfm
from optable_amd.batch import SegmentBatch
from wavefront_reference import S_PAIRS, coefficient_bound, rms_interval, wavefront_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calls_exist():
    assert callable(oa.OpticalTable.wavefront_all) and callable(oa.OpticalTable.wavefront_batch) and oa.MonitorWavefront is wfm.MonitorWavefront
    assert callable(engine.Engine.monitor_wavefront_many) and callable(engine.wavefront_plan)
    assert callable(oa.monitors.MonitorHits.wavefrontList)
    for name in ("power", "mean", "gram", "coefficients", "rms", "strehl", "to_host"):
        assert callable(getattr(oa.MonitorWavefront, name))
    assert "ot_monitor_wavefront_many" in abi.SYMBOLS


def test_binding_has_the_arguments_the_header_declares():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_wavefront_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_wavefront_many is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = abi.SYMBOLS["ot_monitor_wavefront_many"]
    assert restype is C.c_int and len(argtypes) == len(params) == 19
    for p, a in zip(params, argtypes):
        if "*" in p:
            assert a is C.c_void_p or hasattr(a, "_type_") and not isinstance(a._type_, str), (p, a)
        elif p.startswith("int32_t"):
            assert a is C.c_int32, (p, a)
        elif p.startswith("int64_t"):
            assert a is C.c_int64, (p, a)
        else:
            raise AssertionError(p)
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["ctx", "mons", "n_monitors", "axes", "reference_kind", "reference", "coordinates", "pupil", "piston", "src", "intensity", "n_index",
                     "pathlength", "n_segments", "seg_count", "n_rays", "counts", "sums", "accumulate"]


def test_planner_and_its_constant():
    header = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    kernels = open(os.path.join(ROOT, "optable_amd", "csrc", "misc_kernels.h")).read()
    monitors = int(re.search(r"#define\s+OT_WAVEFRONT_MONITORS\s+(\d+)", header).group(1))
    sums = int(re.search(r"#define\s+OT_WAVEFRONT_SUMS\s+(\d+)", header).group(1))
    assert monitors == engine.WAVEFRONT_MONITORS == int(re.search(r"\bMON_WAVEFRONT_CELLS\s*=\s*(\d+)", kernels).group(1)) == 28
    assert sums == engine.WAVEFRONT_SUMS == wfm.N_SUMS == 61 == wfm.N_S + wfm.N_T + 1
    assert 4 * (sums + 2) * 8 * monitors <= 57344  # four waves' rows of 63 doubles a monitor in the 56 KB the spot statistics use
    assert (sums + 2) * monitors <= 7 * 256        # ... and seven values a thread of the last workgroup
    assert engine.wavefront_plan(1) == [(0, 1)] and engine.wavefront_plan(28) == [(0, 28)]
    assert engine.wavefront_plan(29) == [(0, 28), (28, 1)] and engine.wavefront_plan(60) == [(0, 28), (28, 28), (56, 4)]
    for bad in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError):
            engine.wavefront_plan(bad)
    assert wfm.place(0, 0) == 0 and wfm.place(1, 0) == 1 and wfm.place(0, 1) == 2 and wfm.place(0, 8) == 44 and wfm.place(2, 2) == 12
    assert [wfm.place(a, b) for a, b in S_PAIRS] == list(range(45)) and list(wfm.MONOMIALS) == list(S_PAIRS[:15])


def test_every_refusal_is_raised_before_the_engine_is_asked(monkeypatch):
    def never():
        raise AssertionError("the engine was asked")

    monkeypatch.setattr(table_module, "_engine", never)
    t = oa.OpticalTable()
    m1, m2 = oa.Monitor([1, 0, 0], 2, 2), oa.Monitor([2, 0, 0], 2, 1)
    t.add_monitors([m1, m2])
    segs, single = SegmentBatch(64, "f64", "cpu"), SegmentBatch(64, "f32", "cpu")
    good = dict(focus=(1.0, 0.0, 0.0), pupil=(0.0, 0.0, 0.1))
    for kwargs in (dict(pupil=(0, 0, 1)),                                                      # neither focus nor direction
                   dict(focus=(1, 0, 0), direction=(1, 0, 0), pupil=(0, 0, 1)),                # both
                   dict(focus=(1, 0, 0)),                                                      # a focus needs a pupil
                   dict(focus=(1, 0), pupil=(0, 0, 1)), dict(focus=(1, 0, np.nan), pupil=(0, 0, 1)), dict(focus="here", pupil=(0, 0, 1)),
                   dict(focus=[(1, 0, 0)] * 3, pupil=(0, 0, 1)),                               # one per monitor means two
                   dict(direction=(0, 0, 0)), dict(direction=(np.inf, 0, 0)), dict(direction=[(1, 0, 0), (0, 0, 0)]),
                   dict(good, pupil=(0, 0, 0)), dict(good, pupil=(0, 0, -1)), dict(good, pupil=(0, np.nan, 1)), dict(good, pupil=(0, 0)),
                   dict(good, pupil=[(0, 0, 1)] * 3), dict(good, pupil=(0, 0, np.inf)),
                   dict(good, coordinates=2), dict(good, coordinates="angle"), dict(good, coordinates=True), dict(good, coordinates=0.5),
                   dict(good, weight="power"), dict(good, weight=None),
                   dict(good, piston=np.nan), dict(good, piston=(1.0, 2.0, 3.0)), dict(good, piston="mean"), dict(good, piston=[0.0, np.inf]),
                   dict(good, into=[]), dict(good, into=[None, None])):
        with pytest.raises(ValueError):
            t.wavefront_all(segs, **kwargs)
    with pytest.raises(ValueError, match="double-precision"):
        t.wavefront_all(single, **good)
    with pytest.raises(ValueError, match="double-precision"):
        t.wavefront_batch(m1, single, direction=(1, 0, 0))
    with pytest.raises(ValueError):
        oa.monitors.MonitorHits.wavefrontList(type("Hits", (), {"monitor": m1})())  # neither focus nor direction: refused before the hits are looked at
    # what the accepted forms become
    kind, lab, local = wfm.wavefront_reference(None, (2.0, 0.0, 0.0), [m1, m2.RotZ(math.pi / 2)])
    assert kind == 1 and lab.tolist() == [[1, 0, 0], [1, 0, 0]] and np.allclose(local, [[1, 0, 0], [0, -1, 0]], atol=1e-15)
    assert wfm.wavefront_pupil(None, 1, [m1, m2]).tolist() == [[0, 0, 1.0], [0, 0, 0.5]]
    assert wfm.wavefront_coordinates(None, 0) == 0 and wfm.wavefront_coordinates(None, 1) == 1 and wfm.wavefront_coordinates("position", 0) == 1
    kind, _, local = wfm.wavefront_reference((3.0, 1.0, 0.5), None, [m1])
    assert kind == 0 and local.tolist() == [[2.0, 1.0, 0.5]]


def _disc(a, b):
    """(1 / pi) int over the unit disc of p^a q^b, closed form."""
    if a % 2 or b % 2:
        return 0.0
    return math.gamma((a + 1) / 2) * math.gamma((b + 1) / 2) / math.gamma((a + b) / 2 + 2) / math.pi


def test_noll_tables_are_orthonormal_over_the_disc():
    S = np.array([_disc(a, b) for a, b in S_PAIRS])
    A = wfm.noll_matrix()
    G = A @ S[wfm._PRODUCT] @ A.T
    assert np.abs(G - np.eye(15)).max() < 1e-13
    # Noll's order: radial order, then azimuthal; even j are the cosine terms (p), odd the sine terms (q)
    p, q = np.array([0.3, -0.2, 0.7]), np.array([0.4, 0.5, -0.1])
    rho, theta = np.hypot(p, q), np.arctan2(q, p)
    Z = wfm.zernike(15, p, q)
    np.testing.assert_allclose(Z[3], math.sqrt(3) * (2 * rho**2 - 1), atol=1e-15)
    np.testing.assert_allclose(Z[6], math.sqrt(8) * (3 * rho**3 - 2 * rho) * np.sin(theta), atol=1e-15)
    np.testing.assert_allclose(Z[7], math.sqrt(8) * (3 * rho**3 - 2 * rho) * np.cos(theta), atol=1e-15)
    np.testing.assert_allclose(Z[10], math.sqrt(5) * (6 * rho**4 - 6 * rho**2 + 1), atol=1e-15)
    np.testing.assert_allclose(Z[13], math.sqrt(10) * rho**4 * np.cos(4 * theta), atol=1e-15)
    np.testing.assert_allclose(Z[14], math.sqrt(10) * rho**4 * np.sin(4 * theta), atol=1e-15)
    assert len(wfm.NOLL_NAMES) == 15 and wfm.NOLL_NAMES[10] == "spherical"


def _sums(w, Wp, p, q):
    return np.array([math.fsum(w * p**a * q**b) for a, b in S_PAIRS] + [math.fsum(w * Wp * p**a * q**b) for a, b in wfm.MONOMIALS]
                    + [math.fsum(w * Wp * Wp)])


def _made(sums, inside, piston, outside=0):
    return oa.MonitorWavefront(None, torch.tensor(inside), torch.tensor(outside), torch.as_tensor(sums), ("focus", (0.0, 0.0, 0.0)), (0.0, 0.0, 1.0),
                               "direction", piston, "intensity")


@pytest.mark.parametrize("n", [40, 20000])
def test_planted_coefficients_come_back(n):
    """Coefficients of 1e-5 under an offset of 12.3, the mean taken out as the piston: back to rounding, and the rms after 1, 3, 4
    and 15 terms is that of the terms left, computed hit by hit."""
    rng = np.random.default_rng(n)
    rho, theta = np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    p, q, w = rho * np.cos(theta), rho * np.sin(theta), 0.25 + 0.75 * rng.random(n)
    c = 1e-5 * rng.normal(size=15)
    c[0] = 12.3
    Z = wfm.zernike(15, p, q)
    W = c @ Z
    piston = float((w * W).sum() / w.sum())
    wf = _made(_sums(w, W - piston, p, q), n, piston)
    got = wf.coefficients().numpy()
    assert np.abs(got - c).max() < (1e-13 if n == 40 else 1e-15), np.abs(got - c).max()
    assert abs(float(wf.mean()) - piston) < 1e-14 and abs(float(wf.power()) - w.sum()) < 1e-9 * n
    G, b = wf.gram(4)
    assert G.shape == (4, 4) and b.shape == (4,) and torch.allclose(G, G.T)
    for terms in (1, 3, 4, 15):
        # the weighted least-squares residual of the first `terms` terms, by another route
        root = np.sqrt(w)
        fit, *_ = np.linalg.lstsq((Z[:terms] * root).T, root * (W - piston), rcond=None)
        left = W - piston - fit @ Z[:terms]
        want = math.sqrt((w * left * left).sum() / w.sum())
        assert abs(float(wf.rms(terms)) - want) < 1e-10 if terms < 15 else float(wf.rms(terms)) < 1e-9, (terms, float(wf.rms(terms)), want)
    assert abs(float(wf.strehl(1e-4)) - math.exp(-((2 * math.pi * float(wf.rms()) / 1e-4) ** 2))) < 1e-15
    inside, outside, sums = wf.to_host()
    assert (inside, outside) == (n, 0) and sums.shape == (61,)
    for bad in (0, 16, 1.5, True):
        with pytest.raises(ValueError):
            wf.coefficients(bad)


def test_an_undetermined_fit_is_nan():
    rng = np.random.default_rng(3)
    p, q = rng.uniform(-0.5, 0.5, 10), rng.uniform(-0.5, 0.5, 10)
    few = _made(_sums(np.ones(10), 0.1 * p, p, q), 10, 0.0)
    assert torch.isnan(few.coefficients(15)).all() and math.isnan(float(few.rms(15))) and math.isnan(float(few.strehl(1e-4, 15)))  # fewer hits than terms
    assert few.coefficients(15).shape == (15,)
    assert abs(float(few.coefficients(3)[1]) - 0.05) < 1e-15 and float(few.rms(3)) < 1e-9                                       # ... 3 terms are fine
    line = np.linspace(-0.9, 0.9, 50)  # every hit on the line q = 0: tilt along q is not determined
    on_line = _made(_sums(np.ones(50), 0.2 * line, line, np.zeros(50)), 50, 0.0)
    assert torch.isnan(on_line.coefficients(3)).all() and math.isnan(float(on_line.rms(3)))
    assert abs(float(on_line.coefficients(2)[1]) - 0.1) < 1e-15
    none = _made(np.zeros(61), 0, 0.0)
    assert math.isnan(float(none.mean())) and math.isnan(float(none.rms())) and torch.isnan(none.coefficients(1)).all() and float(none.power()) == 0.0


def _cone_records(n, F, seed):
    rng = np.random.default_rng(seed)
    theta, phi = 0.2 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(theta), np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi)], axis=1)
    back = rng.uniform(0.5, 2.0, n)  # every ray starts somewhere on its line through F, its path length counted from F
    return (np.asarray(F) - back[:, None] * d, d, np.full(n, 20.0), 0.5 + rng.random(n), np.ones(n), -back)


def test_reference_a_cone_through_a_point_has_a_constant_path():
    F = np.array([0.3, -0.2, 0.1])
    o, d, length, intensity, n_index, pathlength = _cone_records(500, F, 5)
    mon = oa.Monitor([4.0, 0, 0], 6, 6).RotZ(0.2)
    M, origin = wfm.local_frame(mon)
    ref = wavefront_reference(o, d, length, intensity, n_index, pathlength, M.ravel(), origin, 3, 3, cases.axes_of(mon), 0, M.T @ (F - origin), 0,
                              (-0.197, 0.0, 0.25), 0.0)  # (the tangents are the lab's: the rotated monitor sees the cone's axis at ty = -sin 0.2)
    assert ref.counts.tolist() == [500, 0] and ref.margin > 1e-7
    assert np.abs(ref.W).max() < 1e-14 and np.all(np.abs(ref.sums[45:]) <= ref.bound[45:])  # W = 0 for every ray: T and Q vanish
    assert abs(ref.sums[0] - intensity.sum()) < 1e-12
    c, dc, _, _ = coefficient_bound(ref.sums, ref.bound, 15)
    assert np.all(np.abs(c) <= dc) and rms_interval(ref.sums, ref.bound, 1)[1] < 1e-12
    # against another point the path is not constant; outside a smaller pupil the hits are counted, not summed
    other = wavefront_reference(o, d, length, None, n_index, pathlength, M.ravel(), origin, 3, 3, cases.axes_of(mon), 0, M.T @ (F + [0, 0.01, 0] - origin), 0,
                                (-0.197, 0.0, 0.1), 0.0)
    assert 0 < other.counts[0] < 500 and other.counts.sum() == 500 and other.sums[0] == other.counts[0] and np.ptp(other.W) > 1e-3
    # the hit-by-hit accessor's formula on the same hits (numpy in place of torch)
    lo, ld = (o - origin) @ M, d @ M
    t = -lo[:, 0] / ld[:, 0]
    W = wfm.hit_wavefront(0, (M.T @ (F - origin)).tolist(), lo + t[:, None] * ld, t, ld, n_index, pathlength)
    assert np.abs(W).max() < 1e-14
    # a plane wave along u: rays along u from a plane normal to it have W = x_m u_x, whatever the monitor's pose
    u = np.array([math.cos(0.1), math.sin(0.1), 0.0])
    e1, e2 = np.array([-math.sin(0.1), math.cos(0.1), 0.0]), np.array([0.0, 0.0, 1.0])
    rng = np.random.default_rng(6)
    oo = np.outer(rng.uniform(-0.5, 0.5, 200), e1) + np.outer(rng.uniform(-0.5, 0.5, 200), e2)
    flat = wavefront_reference(oo, np.tile(u, (200, 1)), np.full(200, 20.0), None, np.ones(200), np.zeros(200), M.ravel(), origin, 3, 3, cases.axes_of(mon), 1,
                               M.T @ u, 1, (0.0, 0.0, 3.0), 0.0)
    assert flat.counts.tolist() == [200, 0] and np.abs(flat.W - origin @ u).max() < 1e-14


def test_the_seeded_gpu_cases_keep_their_margin():
    """The cfg 2 cases of tests/test_gpu_wavefront.py, traced by the C oracle: every decision of the reference is 1e-7 from its
    boundary (cases.reference asserts it), the clipping pupils clip and the empty monitor stays empty."""
    table = support.cfg2_table()
    for n, seed, K in cases.CFG2_BATCHES:
        records = cases.oracle_records(table, *cases.cfg2_arrays(n, seed), K)
        for name, su in cases.SETUPS.items():
            mons = cases.monitors_at(su["x"])
            refs = [cases.reference(records, m, su["kwargs"], p, 0.0) for m, p in zip(mons, su["pupil"])]
            assert refs[cases.EMPTY].counts.tolist() == [0, 0]
            if n == 5003:
                assert refs[0].counts[0] >= n and refs[0].counts[1] == 0 and refs[1].counts.min() > 0
                other = (0.0, 0.0, 0.5) if name == "focus" else (0.0, 0.0, 0.01)
                cases.reference(records, mons[0], su["kwargs"], other, 2.5, coordinates=1 if name == "focus" else 0)
    records = cases.oracle_records(table, *cases.cfg2_arrays(1003, 5), 5)
    for m, p in zip(*cases.group_monitors()):
        assert cases.reference(records, m, dict(direction=(1.0, 0.0, 0.0)), p, 5.0).counts[0] > 0
