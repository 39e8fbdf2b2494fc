"""GPU (MI355X): `OpticalTable.record_batch` — Monitor.record on ONE monitor (ot_monitor_record_f64, which runs the count / scan /
emit passes of ot_monitor_record_many with one monitor) — against the C oracle on the host copy of the same segments: a yardstick
of its own, next to the comparison of `record_all` with `record_batch` in tests/test_gpu_record_all.py.
Slot sets must be identical, in ascending slot order; P and t agree to 1e-12.  Identical sets need inputs with no hit on an edge:
every comparison first asserts, from the ORACLE's values, that no hit lies within 1e-9 of the monitor's half-width or half-height
or of the limits on t (the condition of tests/test_gpu_record_all.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
import support
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine
from optable_amd.table import monitor_struct

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)


EMPTY = 2


@pytest.mark.parametrize("layout", ["slots", "append"])
def test_against_the_oracle(oracle, layout):
    """cfg 2, 5,003 rays x 5 segments, double precision: slot arrays, and the append layout's list with holes."""
    table = oa.OpticalTable()
    table.add_components(scenes.cfg2_components(oa))
    o, d = scenes.cfg2_rays(5003, 0)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q, device="cuda")
    segs = table.trace_batch(batch, max_segments=5, layout=layout)
    assert segs.layout == layout and segs.precision == "f64"
    if layout == "append":
        assert bool((segs.ray[:segs.n_valid] < 0).any())  # 25,015 records do not fill whole chunks: there are holes
    host = segs.to_host(reference_order=False)                  # the valid records, in slot order ...
    slot_of = torch.nonzero(segs.valid_mask()).flatten().cpu().numpy()  # ... and the slot each of them lies in
    assert len(slot_of) == len(host["ox"]) == 5003 * 5
    found = []
    for m in support.six_monitors():
        got = table.record_batch(m, segs)
        idx, P, t = oracle.monitor_record(monitor_struct(m), host)
        P = P.reshape(-1, 3)
        if len(idx):  # clear of the edges, from the oracle's values
            assert np.all(np.abs(np.abs(P[:, 1]) - m.width / 2) > 1e-9) and np.all(np.abs(np.abs(P[:, 2]) - m.height / 2) > 1e-9)
            assert np.all(t - 1e-9 > 1e-9) and np.all(host["length"][idx] - t > 1e-9)
        assert np.all(np.diff(idx) > 0)
        # the library call gives the slots ascending, as the oracle walks them; MonitorHits keeps them in the reference's order
        slot, P_dev, t_dev = get_engine().monitor_record(monitor_struct(m), segs)
        np.testing.assert_array_equal(slot.cpu().numpy(), slot_of[idx])
        np.testing.assert_allclose(P_dev.cpu().numpy().reshape(-1, 3), P, **TOL)
        np.testing.assert_allclose(t_dev.cpu().numpy(), t, **TOL)
        order = torch.argsort(got.slot)
        assert torch.equal(got.slot[order], slot) and torch.equal(got.P[order], P_dev) and torch.equal(got.t[order], t_dev)
        assert len(got) == len(idx) and bool((got.ray[1:] >= got.ray[:-1]).all())
        found.append(len(idx))
    assert found[EMPTY] == 0 and 0 < found[5] < found[0] and sum(f > 0 for f in found) >= 3


def test_no_segments():
    eng = get_engine()
    segs = SegmentBatch(64, "f64", "cuda")
    segs.n_valid = 0
    mon = monitor_struct(oa.Monitor([7.5, 0, 0], 6, 6))
    idx = torch.full((64,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((4, 64), -7.0, dtype=torch.float64, device="cuda")
    n_hits = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ss = segs.c_struct()
    for n_rays in (0, -1):  # a list, a list with holes
        n_hits.fill_(-7)
        with eng.lock:
            assert eng.lib.ot_monitor_record_f64(eng._ctx, C.byref(mon), C.byref(ss), 0, None, n_rays, idx.data_ptr(), *(out[k].data_ptr() for k in range(4)),
                                                 n_hits.data_ptr()) == 0
        torch.cuda.synchronize()
        assert int(n_hits.item()) == 0 and bool((idx == -7).all()) and bool((out == -7.0).all())
