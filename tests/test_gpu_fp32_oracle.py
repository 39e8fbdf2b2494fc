"""GPU (MI355X): the single-precision PRODUCTION kernels against the oracle and the reference's fixtures directly.

BASELINE quotes cfg 3 and cfg 5 in fp32.  tests/test_gpu_fp32_contract.py compares the fp32 kernels with the fp64
kernels, and the fp64 kernels are compared with the oracle elsewhere: a chain, in which a defect shared by every HIP
variant would cancel.  Here the chain is closed: the fp32 trace as `trace_batch` launches it by default (cfg 3: pair
queue + records in LDS; cfg 5: rolling lists over the instanced lattice, records in LDS) is held against the CPU
oracle (fp64, pinned by the reference's fixtures) on the same inputs, and against fixtures g09 / g10, which hold
numbers the reference itself produced.  Contract: at least 99.95 % of the rays visit exactly the same
surfaces; on those rays every segment start agrees to 2e-3; every other ray is an edge case — its deciding hit lies
within 1e-4 of an aperture edge, or the deciding segment is shorter than 1e-4 (optable_amd/fp32_audit.py)."""
import numpy as np
import pytest
import torch

import helpers
import optable_amd as oa
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine
from optable_amd.fp32_audit import assert_explained, audit, audit_traces

pytestmark = pytest.mark.gpu
EDGE, SHORT = 1e-4, 1e-4


def slots_from_reference_order(ref, n, K):
    """A [k][ray] SegmentBatch (on the CPU) from a trace in the reference's order (input ray major, then segment
    order): what fp32_audit compares the device's slots with."""
    ray = np.asarray(ref["ray"], dtype=np.int64)
    first = np.r_[0, np.flatnonzero(np.diff(ray)) + 1]
    k = np.arange(len(ray)) - np.repeat(first, np.diff(np.r_[first, len(ray)]))
    out = SegmentBatch(n * K, "f64", "cpu")
    slot = torch.from_numpy(k * n + ray)
    for f in abi.SEG_FIELDS:
        out.field(f).zero_()
        out.field(f)[slot] = torch.from_numpy(np.asarray(ref[f], dtype=np.float64))
    out.surface.fill_(-9)
    out.surface[slot] = torch.from_numpy(np.asarray(ref["surface"], dtype=np.int32))
    out.ray[slot] = torch.from_numpy(ray.astype(np.int32))
    out.count = torch.from_numpy(np.bincount(ray, minlength=n).astype(np.int32))
    out.n_rays = n
    return out


def check_against(scene, ref_slots, s32, n, K):
    s32 = s32.as_kray_slots(K)  # (the production layout of a heavy scene is the dense append-order list)
    rep = audit(scene, ref_slots, s32, K)
    assert rep["same"].mean() >= 0.9995, rep["same"].mean()
    edge = (rep["margin"] < EDGE) | (np.minimum(rep["len64"], rep["len32"]) < SHORT)
    assert edge.all(), [(int(r), int(k), float(m)) for r, k, m in zip(rep["ray"][~edge], rep["kstar"][~edge], rep["margin"][~edge])]
    c = np.abs(ref_slots.count.cpu().numpy())
    valid = (np.arange(K)[:, None] < c[None, :]) & rep["same"][None, :]
    worst = 0.0
    for f in ("ox", "oy", "oz"):
        a = ref_slots.field(f).cpu().numpy().reshape(K, n)
        with np.errstate(invalid="ignore"):
            b = s32.field(f).cpu().numpy().reshape(K, n).astype(np.float64)
        worst = max(worst, float(np.abs(a - b)[valid].max()))
    assert worst < 2e-3, worst
    return rep


@pytest.mark.parametrize("name,n", [("cfg3", 20_000), ("cfg5", 3_000)])
def test_fp32_production_kernel_matches_oracle(name, n, oracle):
    wl = W.baseline_workloads(oa)[name]
    table = oa.OpticalTable()
    table.add_components(wl.components())
    o, d, lam = wl.rays(n, 0)
    q = 1j * np.pi * W.W0**2 / lam
    K = wl.max_segments
    b32 = RayBatch.from_arrays(o, d, wavelength=lam, q=q, precision="f32")
    s32 = table.trace_batch(b32, max_segments=K)  # the DEFAULT call: the layout and kernel the bench quotes for these configs
    info = get_engine().last_launch()
    assert s32.layout == "append" and info["kernel"] == 2 and info["pair_queue"] & 2 and info["pair_queue"] & 4, info  # records of the live rays in LDS, dense list
    if name == "cfg3":
        assert info["pair_queue"] & 1 and info["mixed"] == 1, info  # ... through the pair queue
    else:
        assert info["pair_queue"] & 16, info  # ... the workgroup-wide block pool
    scene = table.compile()
    host = RayBatch.from_arrays(o, d, wavelength=lam, q=q, device="cpu").to_host()
    ref = oracle.trace(scene, host, max_trace_num=K)
    rep = check_against(scene, slots_from_reference_order(ref, n, K), s32, n, K)
    # the general audit reads the oracle's records directly: prefix check, every cause (polygons, cylinders, TIR, ties)
    assert_explained(audit_traces(scene, ref, s32.to_host(reference_order=True), prec="f32", tol=2e-3, rays=host))
    # the [k][ray] slots are the same computation: identical records (tests/test_gpu_append.py) — spot-check the count here
    slots = table.trace_batch(b32, max_segments=K, layout="slots")
    np.testing.assert_array_equal(slots.count.cpu().numpy(), s32.count.cpu().numpy())
    assert rep["same"].sum() >= 0.9995 * n


@pytest.mark.parametrize("fixture", ["g09_cfg5", "g10_cfg3"])
def test_fp32_against_reference_fixture(fixture):
    """The reference's own numbers (tests/golden, generated by tools/make_golden.py from /root/reference): same contract."""
    gold = helpers.golden(fixture)
    table, sc = helpers.build(fixture)
    n, K = len(gold["in_origin"]), int(gold["limit"][0])
    b32 = RayBatch.from_arrays(gold["in_origin"], gold["in_direction"], wavelength=gold["in_wavelength"], q=gold["in_q"],
                               intensity=gold["in_intensity"], n_index=gold["in_n"], pathlength=gold["in_pathlength"],
                               precision="f32", normalize=False)
    s32 = table.trace_batch(b32, max_segments=K)
    scene = table.compile()
    # leaf of every reference segment: the leaf whose surface the NEXT segment of the tree starts on is not recorded in the
    # fixture, so surfaces are compared through the oracle's labelling of the same (pinned) trace
    from oracle import oracle as orc

    host = RayBatch.from_arrays(gold["in_origin"], gold["in_direction"], wavelength=gold["in_wavelength"], q=gold["in_q"],
                                intensity=gold["in_intensity"], n_index=gold["in_n"], pathlength=gold["in_pathlength"],
                                device="cpu", normalize=False).to_host()
    ref = orc.trace(scene, host, max_trace_num=K)
    np.testing.assert_array_equal(ref["ray"], gold["seg_tree"])  # the oracle IS the fixture ...
    np.testing.assert_allclose(np.stack([ref["ox"], ref["oy"], ref["oz"]], 1), gold["seg_origin"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ref["length"], gold["seg_length"], rtol=1e-9, atol=1e-9)
    fix = dict(ref)
    for k, ax in enumerate("xyz"):  # ... and the numbers compared are the reference's
        fix["o" + ax], fix["d" + ax] = gold["seg_origin"][:, k], gold["seg_direction"][:, k]
    fix["length"], fix["intensity"], fix["pathlength"], fix["n"] = gold["seg_length"], gold["seg_intensity"], gold["seg_pathlength"], gold["seg_n"]
    rep = check_against(scene, slots_from_reference_order(fix, n, K), s32, n, K)
    assert_explained(audit_traces(scene, ref, s32.to_host(reference_order=True), prec="f32", tol=2e-3, rays=host))
    # fields beyond the positions, on the rays whose sequences agree (one diverging ray takes only itself out of the
    # comparison, never the whole of it), at what 20-50 fp32 bounces leave: 2e-3 relative
    got = s32.to_host(reference_order=True)
    same = rep["same"]
    g, w = same[got["ray"]], same[gold["seg_tree"]]
    assert w.any() and np.array_equal(got["ray"][g], gold["seg_tree"][w])  # the same records of the same rays, in the same order
    finite = np.isfinite(gold["seg_length"][w])
    np.testing.assert_allclose(got["length"][g][finite], gold["seg_length"][w][finite], rtol=2e-3, atol=2e-3)
    np.testing.assert_array_equal(np.isinf(got["length"][g]), ~finite)
    np.testing.assert_allclose(got["pathlength"][g], gold["seg_pathlength"][w], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(got["intensity"][g], gold["seg_intensity"][w], rtol=1e-5, atol=1e-6)
    for k, ax in enumerate("xyz"):
        np.testing.assert_allclose(got["d" + ax][g], gold["seg_direction"][w][:, k], rtol=2e-3, atol=2e-3, err_msg="d" + ax)
    np.testing.assert_allclose(got["n"][g], gold["seg_n"][w], rtol=2e-3, atol=2e-3)
