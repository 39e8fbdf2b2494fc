"""CPU: the resident-plane token of a SegmentBatch (batch.py), on host tensors — what sets it, what every entry of it is compared
with, and what ends it.  No engine and no device: `engine` and `stream` are whatever objects the caller compares by."""
import functools
import re
import os

import numpy as np
import pytest
import torch

import support
from optable_amd import abi
from optable_amd.batch import RayBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY, N, I, ALL = abi.RESIDENT_RAY, abi.RESIDENT_N, abi.RESIDENT_INTENSITY, abi.RESIDENT_ALL
ONE64 = int(np.float64(1.0).view(np.int64))
ONE32 = int(np.float32(1.0).view(np.int32))
ENGINE, STREAM = object(), 1234
n, K = 130, 5
_out = functools.partial(support.host_out, n, K)


def _values(one=ONE64):
    return {N: one, I: one}


def _set(out, planes=ALL, layout="slots", values=None, engine=ENGINE, stream=STREAM, rays=n):
    out._set_resident(planes, rays, layout, values if values is not None else _values(), engine, stream)
    return out


def _mask(out, layout="slots", values=None, engine=ENGINE, stream=STREAM, rays=n):
    return out.resident_mask(rays, layout, values if values is not None else _values(), engine, stream)


def test_header_and_binding_agree_on_the_bits():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    for name, value in (("RAY", RAY), ("N", N), ("INTENSITY", I)):
        assert re.search(rf"OT_RESIDENT_{name} = 1 << (\d+)", text).group(1) == str(value.bit_length() - 1)
    assert re.search(r"OT_OPT_RESIDENT = (\d+)", text).group(1) == str(abi.OPT_RESIDENT)
    assert ALL == RAY | N | I and set(abi.RESIDENT_FIELD) == {RAY, N, I}


def test_a_fresh_batch_has_no_token_and_a_set_one_answers():
    out = _out()
    assert _mask(out) == 0
    assert _mask(_set(out)) == ALL
    assert _mask(out) == ALL  # asking does not use it up
    assert _mask(_set(_out(), planes=RAY | N)) == RAY | N
    assert _mask(_set(_out(), planes=0)) == 0
    # a plane whose value the input does not know is not kept, at either end
    assert _mask(_set(_out(), values={N: ONE64, I: None})) == RAY | N
    assert _mask(_set(_out()), values={N: None, I: ONE64}) == RAY | I
    assert _mask(_set(_out()), values={}) == RAY


@pytest.mark.parametrize("field", ["ray", "n_index", "intensity", "count"])
def test_a_version_bump_kills_it(field):
    out = _set(_out())
    getattr(out, field)[3:5] = 1  # any in-place torch write
    assert _mask(out) == 0
    out = _set(_out())
    getattr(out, field).data[3:5] = 1  # the hole: not seen
    assert _mask(out) == ALL
    assert _mask(out.forget_resident()) == 0


def test_only_the_planes_concerned_are_watched():
    out = _set(_out(), planes=RAY)
    out.intensity.fill_(2.0)
    out.ox.fill_(2.0)
    assert _mask(out) == RAY
    out.ray.zero_()
    assert _mask(out) == 0


def test_a_replaced_tensor_kills_it():
    out = _set(_out())
    out.count = out.count.clone()
    assert _mask(out) == 0
    out = _set(_out())
    out.ray = out.ray.clone()
    assert _mask(out) == 0


def test_tiles_stand_on_the_block():
    out = _set(_out(tiled=True), layout="tiled")
    assert _mask(out, layout="tiled") == ALL
    out.ox[0, 0] = 1.0  # a view of the block: one counter
    assert _mask(out, layout="tiled") == 0
    out = _set(_out(tiled=True), layout="tiled")
    out.ray.data.fill_(-1)
    assert _mask(out, layout="tiled") == ALL


def test_another_n_layout_engine_stream_or_value_kills_it():
    out = _set(_out())
    assert _mask(out, rays=n - 1) == 0
    assert _mask(out, layout="tiled") == 0
    assert _mask(out, engine=object()) == 0
    assert _mask(out, stream=STREAM + 1) == 0
    assert _mask(out) == ALL  # (none of the questions above changed it)
    half = int(np.float64(0.5).view(np.int64))
    assert _mask(out, values={N: half, I: ONE64}) == RAY | I
    assert _mask(out, values={N: ONE64, I: half}) == RAY | N
    assert _mask(out, values={N: ONE32, I: ONE32}) == RAY  # the same number in another precision is another pattern


def test_tensors_without_a_version_counter_carry_no_token():
    with torch.inference_mode():
        out = _out()
    assert _mask(_set(out)) == 0


def test_copies_made_for_readers_carry_no_token():
    out = _set(_out(tiled=True), layout="tiled")
    assert out.to_slots()._resident is None and out.astype("f32")._resident is None
    assert _set(_out()).astype("f32")._resident is None


@pytest.mark.parametrize("precision, one", [("f64", ONE64), ("f32", ONE32)])
def test_ray_batches_know_the_value_of_a_uniform_field(precision, one):
    o = np.zeros((n, 3))
    d = np.tile([1.0, 0.0, 0.0], (n, 1)) + np.random.default_rng(0).uniform(-0.1, 0.1, (n, 3))
    batch = RayBatch.from_arrays(o, d, wavelength=780e-7, precision=precision, device="cpu")
    assert batch.uniform_bits("n") == one and batch.uniform_bits("intensity") == one
    assert batch.uniform_bits("dx") is None  # not uniform
    assert batch.uniform_bits("ox") == 0
    # passed on with the hint
    assert batch.slice(3, 70).uniform_bits("n") == one and batch.clone().uniform_bits("intensity") == one
    many = batch.multiplexed_in_wavelength([500e-7, 600e-7])
    assert many.uniform_bits("n") == one and many.uniform_bits("wavelength") is None
    assert batch.take(torch.arange(n)).uniform_bits("n") is None and batch.with_ids(torch.arange(n)).uniform_bits("n") is None
    # a batch that never compared on the host knows no value
    assert RayBatch(n, precision, "cpu").uniform_bits("n") is None
    # an edit ends the value with the hint (the fields are rows of one staging block: one counter)
    part = batch.slice(0, 64)
    batch.intensity.mul_(0.5)
    assert batch.uniform_bits("intensity") is None and batch.uniform_bits("n") is None and part.uniform_bits("n") is None
    other = RayBatch.from_arrays(o, d, intensity=0.5, n_index=np.linspace(1, 2, n), precision=precision, device="cpu")
    assert other.uniform_bits("intensity") not in (None, one) and other.uniform_bits("n") is None
    assert other.forget_uniform().uniform_bits("intensity") is None


def test_subnormal_intensities_are_not_trusted_to_survive_a_product():
    from optable_amd.engine import _keeps_bits

    assert _keeps_bits(ONE64, "f64") == ONE64 and _keeps_bits(ONE32, "f32") == ONE32 and _keeps_bits(0, "f64") == 0
    assert _keeps_bits(None, "f64") is None
    assert _keeps_bits(int(np.float64(5e-324).view(np.int64)), "f64") is None
    assert _keeps_bits(int(np.float32(1e-45).view(np.int32)), "f32") is None
    assert _keeps_bits(int(np.float32(-0.0).view(np.int32)) & 0xFFFFFFFF, "f32") is not None
