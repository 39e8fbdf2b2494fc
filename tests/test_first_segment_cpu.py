"""CPU: the first-segment token of a SegmentBatch (batch.py), on host tensors — what sets it, what every entry of it is compared
with, what ends it, and that the resident-plane token beside it answers as before.  No engine and no device: `engine` and
`stream` are whatever objects the caller compares by."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import support
from optable_amd import abi
from optable_amd.batch import RayBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY, N, I, ALL = abi.RESIDENT_RAY, abi.RESIDENT_N, abi.RESIDENT_INTENSITY, abi.RESIDENT_ALL
BIT = abi.UNIFORM_BIT
ELEVEN = ("ox", "oy", "oz", "dx", "dy", "dz", "q_re", "q_im", "intensity", "n", "pathlength")
ONE64 = int(np.float64(1.0).view(np.int64))
ONE32 = int(np.float32(1.0).view(np.int32))
NEG0 = int(np.float64(-0.0).view(np.uint64))
ENGINE, STREAM = object(), 1234
n, K = 130, 5
_out = functools.partial(support.host_out, n, K)
POINT = {"ox": 0, "oy": 0, "oz": 0, "q_re": 0, "q_im": ONE64, "pathlength": 0, "n": ONE64, "intensity": ONE64}  # a point source (cfg 2)
POINT_MASK = sum(BIT[f] for f in POINT)


def _values(**change):
    v = {f: POINT.get(f) for f in ELEVEN}  # the engine asks every field: None where the batch is not uniform in it
    v.update(change)
    return v


def _set(out, values=None, layout="slots", engine=ENGINE, stream=STREAM, rays=n):
    out._set_first(values if values is not None else _values(), rays, layout, engine, stream)
    return out


def _mask(out, values=None, layout="slots", engine=ENGINE, stream=STREAM, rays=n):
    return out.first_mask(rays, layout, values if values is not None else _values(), engine, stream)


def test_header_and_binding_agree_on_the_bits_and_the_option():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    listed = re.search(r"OT_FIRST_FIELDS = ([^}]*)\}", text).group(1)
    names = re.findall(r"OT_UNIFORM_(\w+)", listed)
    header_bit = {m.group(1): int(m.group(2)) for m in re.finditer(r"OT_UNIFORM_(\w+) = 1 << (\d+)", text)}
    assert sorted(name.lower() for name in names) == sorted(ELEVEN)
    assert sum(1 << header_bit[name] for name in names) == abi.FIRST_FIELDS == sum(BIT[f] for f in ELEVEN)
    assert set(abi.FIRST_FIELD.values()) == set(ELEVEN) and all(BIT[f] == bit for bit, f in abi.FIRST_FIELD.items())
    assert not abi.FIRST_FIELDS & (BIT["wavelength"] | abi.UNIFORM_ID | abi.UNIFORM_FLAGS)
    assert abi.FIRST_FIELDS << 8 < 1 << 32 and not (abi.FIRST_FIELDS << 8) & ALL  # they ride above the planes in one kernel argument
    assert re.search(r"OT_OPT_RESIDENT = (\d+)", text).group(1) == str(abi.OPT_RESIDENT)  # the same option id: its values are exercised on the GPU
    # the old mask keeps its three bits
    assert ALL == RAY | N | I and set(abi.RESIDENT_FIELD) == {RAY, N, I}
    for name in ("ot_trace_reuse_f64", "ot_trace_reuse_f32", "ot_trace_tiled_reuse_f64", "ot_trace_tiled_reuse_f32", "ot_trace_reuse_plan"):
        assert name in abi.SYMBOLS and re.search(rf"\bint {name}\(", text)
    assert len(abi.SYMBOLS["ot_trace_reuse_f64"][1]) == len(abi.SYMBOLS["ot_trace_resident_f64"][1]) + 1
    assert len(abi.SYMBOLS["ot_trace_tiled_reuse_f32"][1]) == len(abi.SYMBOLS["ot_trace_tiled_resident_f32"][1]) + 1


def test_a_fresh_batch_has_no_token_and_a_set_one_answers():
    out = _out()
    assert out._first is None and _mask(out) == 0
    assert _mask(_set(out)) == POINT_MASK
    assert _mask(out) == POINT_MASK  # asking does not use it up
    assert out._first["values"] == POINT  # {record field: bit pattern}, the fields with a known pattern only
    # a field whose value the input does not know is not kept, at either end
    assert _mask(_set(_out(), _values(ox=None))) == POINT_MASK & ~BIT["ox"]
    assert _mask(_set(_out()), _values(q_im=None)) == POINT_MASK & ~BIT["q_im"]
    assert _mask(_set(_out()), {}) == 0
    assert _set(_out(), {f: None for f in ELEVEN})._first is None and _set(_out(), {})._first is None
    # what is no record field is no entry
    assert "wavelength" not in _set(_out(), dict(_values(), wavelength=5))._first["values"]


def test_a_changed_value_is_written_again():
    out = _set(_out())
    moved = int(np.float64(0.25).view(np.int64))
    assert _mask(out, _values(oy=moved)) == POINT_MASK & ~BIT["oy"]
    assert _mask(out, _values(oz=NEG0)) == POINT_MASK & ~BIT["oz"]  # -0.0 against 0.0: another pattern
    assert _mask(out, _values(q_im=ONE32)) == POINT_MASK & ~BIT["q_im"]  # the same number in another precision
    assert _mask(out, _values(dx=ONE64)) == POINT_MASK  # uniform now, not when the records were written
    assert _mask(out) == POINT_MASK  # (none of the questions above changed it)


@pytest.mark.parametrize("field", ["ox", "q_im", "pathlength", "n_index", "count"])
def test_a_version_bump_kills_it(field):
    out = _set(_out())
    getattr(out, field)[3:5] = 1  # any in-place torch write
    assert _mask(out) == 0
    out = _set(_out())
    getattr(out, field).data[3:5] = 1  # the hole: not seen
    assert _mask(out) == POINT_MASK
    assert _mask(out.forget_resident()) == 0 and out._first is None


def test_only_the_planes_concerned_are_watched():
    out = _set(_out(), _values(n=None, intensity=None))
    out.dx.fill_(2.0)
    out.length.fill_(2.0)
    out.n_index.fill_(2.0)
    out.ray.zero_()
    assert _mask(out) == POINT_MASK & ~(BIT["n"] | BIT["intensity"])
    out.oz.zero_()
    assert _mask(out) == 0


def test_a_replaced_tensor_kills_it():
    out = _set(_out())
    out.count = out.count.clone()
    assert _mask(out) == 0
    out = _set(_out())
    out.q_re = out.q_re.clone()
    assert _mask(out) == 0


def test_tiles_stand_on_the_block():
    out = _set(_out(tiled=True), layout="tiled")
    assert _mask(out, layout="tiled") == POINT_MASK
    out.length[0, 0] = 1.0  # a view of the block: one counter
    assert _mask(out, layout="tiled") == 0
    out = _set(_out(tiled=True), layout="tiled")
    out.ox.data.fill_(-1)
    assert _mask(out, layout="tiled") == POINT_MASK


def test_another_n_layout_engine_or_stream_kills_it():
    out = _set(_out())
    assert _mask(out, rays=n - 1) == 0
    assert _mask(out, layout="tiled") == 0
    assert _mask(out, engine=object()) == 0
    assert _mask(out, stream=STREAM + 1) == 0
    assert _mask(out) == POINT_MASK


def test_tensors_without_a_version_counter_carry_no_token():
    with torch.inference_mode():
        out = _out()
    assert _mask(_set(out)) == 0 and out._first is None


def test_copies_made_for_readers_carry_no_token():
    out = _set(_out(tiled=True), layout="tiled")
    assert out.to_slots()._first is None and out.astype("f32")._first is None
    assert _set(_out()).astype("f32")._first is None


def test_the_resident_token_answers_as_before_beside_it():
    values = {N: ONE64, I: ONE64}
    out = _out()
    out._set_resident(ALL, n, "slots", values, ENGINE, STREAM)
    before = dict(out._resident)
    _set(out)
    assert out._resident == before and out._resident["planes"] == ALL
    assert out.resident_mask(n, "slots", values, ENGINE, STREAM) == ALL
    # a write to a plane only the first-segment token watches ends that one alone
    out.ox[0] = 1.0
    assert _mask(out) == 0 and out.resident_mask(n, "slots", values, ENGINE, STREAM) == ALL
    # ... and the other way round
    out = _set(_out())
    out._set_resident(RAY, n, "slots", {}, ENGINE, STREAM)
    out.ray[0] = 1
    assert out.resident_mask(n, "slots", {}, ENGINE, STREAM) == 0 and _mask(out) == POINT_MASK
    # setting the old token does not touch the new one; forget_resident ends both
    out._set_resident(ALL, n, "slots", values, ENGINE, STREAM)
    assert _mask(out) == POINT_MASK
    out.forget_resident()
    assert out._resident is None and out._first is None


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_point_source_batch_knows_the_patterns_the_token_takes(precision):
    o = np.zeros((n, 3))
    d = np.tile([1.0, 0.0, 0.0], (n, 1)) + np.random.default_rng(0).uniform(-0.1, 0.1, (n, 3))
    batch = RayBatch.from_arrays(o, d, wavelength=780e-7, q=1j, precision=precision, device="cpu")
    values = {f: batch.uniform_bits(f) for f in abi.FIRST_FIELD.values()}
    assert {f for f, v in values.items() if v is not None} == set(POINT)
    out = _set(_out(precision), values)
    assert _mask(out, values) == POINT_MASK
    moved = RayBatch.from_arrays(o + [0.0, 0.5, 0.0], d, wavelength=780e-7, q=1j, precision=precision, device="cpu")
    assert _mask(out, {f: moved.uniform_bits(f) for f in ELEVEN}) == POINT_MASK & ~BIT["oy"]
    batch.ox.mul_(2.0)  # an edit ends the batch's own hint (one staging block: every field of it)
    assert _mask(out, {f: batch.uniform_bits(f) for f in ELEVEN}) == 0
