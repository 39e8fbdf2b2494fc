"""CPU: the uniform-field hint of RayBatch (optable_amd/batch.py) — which fields `from_arrays` flags, what drops a flag, which
constructors pass the hint on.  The tensors live on the host here; the rule is the same on the device (tests/test_gpu_uniform.py)."""
import numpy as np
import pytest
import torch

from optable_amd import abi
from optable_amd.batch import RayBatch

BIT = abi.UNIFORM_BIT
SCALARS = BIT["wavelength"] | BIT["q_re"] | BIT["q_im"] | BIT["intensity"] | BIT["n"] | BIT["pathlength"]
ORIGIN = BIT["ox"] | BIT["oy"] | BIT["oz"]
DIRECTION = BIT["dx"] | BIT["dy"] | BIT["dz"]
N = 37


def _spread(n=N, seed=0):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1, 1, (n, 3))
    d = rng.uniform(0.1, 1, (n, 3))
    return o, d


def _batch(o=None, d=None, precision="f64", **kw):
    so, sd = _spread()
    kw.setdefault("wavelength", 780e-7)
    kw.setdefault("q", 1j * 0.15)
    return RayBatch.from_arrays(so if o is None else o, sd if d is None else d, precision=precision, device="cpu", **kw)


def test_bits_mirror_the_header():
    """abi.UNIFORM_BIT is OT_UNIFORM_* of include/optable_hip.h: bit k = the k-th real field of ot_rays, then id, then flags."""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "optable_hip.h")).read()
    declared = {m.group(1).lower(): 1 << int(m.group(2)) for m in re.finditer(r"OT_UNIFORM_([A-Z_]+) = 1 << (\d+)", text)}
    assert declared == BIT and len(BIT) == 14
    assert abi.UNIFORM_ALL == sum(BIT.values()) == (1 << 14) - 1
    assert re.search(r"OT_OPT_UNIFORM = (\d+)", text).group(1) == str(abi.OPT_UNIFORM)
    assert abi.ABI_VERSION == 14  # additive: no version step


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_scalar_fields_are_flagged(precision):
    b = _batch(precision=precision)
    assert b.uniform_mask == SCALARS | BIT["id"] | BIT["flags"]
    # without q the q rows are zeros: uniform too
    assert _batch(q=None, precision=precision).uniform_mask == SCALARS | BIT["id"] | BIT["flags"]


def test_constant_and_varying_columns():
    o, d = _spread()
    point = np.tile([0.0, 0.5, -0.25], (N, 1))
    assert _batch(o=point).uniform_mask & (ORIGIN | DIRECTION) == ORIGIN
    beam = np.tile([1.0, 0.0, 0.0], (N, 1))
    assert _batch(d=beam).uniform_mask & (ORIGIN | DIRECTION) == DIRECTION
    # one constant column among varying ones
    o2 = o.copy()
    o2[:, 1] = 2.0
    assert _batch(o=o2).uniform_mask & ORIGIN == BIT["oy"]
    # array-valued "scalars": a constant array is flagged, a varying one is not
    b = _batch(wavelength=np.full(N, 500e-7), intensity=np.linspace(0.5, 1.0, N))
    assert b.uniform_mask & BIT["wavelength"] and not b.uniform_mask & BIT["intensity"]
    # (a direction that normalisation makes uniform is uniform: the comparison is on what the batch holds)
    assert _batch(d=np.outer(np.linspace(1, 2, N), [1.0, 0.0, 0.0])).uniform_mask & DIRECTION == DIRECTION


def test_one_differing_element_is_not_flagged():
    for where in (0, N // 2, N - 1):
        o = np.zeros((N, 3))
        o[where, 2] = 1e-300
        m = _batch(o=o).uniform_mask
        assert m & ORIGIN == BIT["ox"] | BIT["oy"], where
    wl = np.full(N, 780e-7)
    wl[-1] = np.nextafter(780e-7, 1.0)
    assert not _batch(wavelength=wl).uniform_mask & BIT["wavelength"]
    # ... unless the batch's precision cannot tell them apart: the comparison is made after the conversion
    assert _batch(wavelength=wl, precision="f32").uniform_mask & BIT["wavelength"]


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_signed_zeros_are_not_merged(precision):
    o = np.zeros((N, 3))
    o[3, 0] = -0.0
    m = _batch(o=o, precision=precision).uniform_mask
    assert m & ORIGIN == BIT["oy"] | BIT["oz"]
    assert _batch(o=-np.zeros((N, 3)), precision=precision).uniform_mask & ORIGIN == ORIGIN  # all -0.0: one bit pattern


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_nan_is_not_flagged(precision):
    assert not _batch(pathlength=float("nan"), precision=precision).uniform_mask & BIT["pathlength"]
    pl = np.zeros(N)
    pl[5] = np.nan
    assert not _batch(pathlength=pl, precision=precision).uniform_mask & BIT["pathlength"]
    assert not _batch(pathlength=np.full(N, np.nan), precision=precision).uniform_mask & BIT["pathlength"]


def test_ids_and_flags():
    assert _batch(ids=np.arange(N)).uniform_mask & BIT["id"]
    assert not _batch(ids=np.arange(N)[::-1]).uniform_mask & BIT["id"]
    assert not _batch(ids=np.zeros(N, dtype=np.int32)).uniform_mask & BIT["id"]
    b = _batch()
    b.flags.copy_(torch.zeros(N, dtype=torch.int32))  # (what callers do to mark dead rays)
    assert not b.uniform_mask & BIT["flags"] and b.uniform_mask & BIT["id"]
    b = _batch()
    b.id = torch.arange(N, dtype=torch.int32)  # another tensor object: the entry was taken from the old one
    assert not b.uniform_mask & BIT["id"]


def test_empty_batch_has_no_hint():
    assert RayBatch.from_arrays(np.zeros((0, 3)), np.zeros((0, 3)), device="cpu", normalize=False).uniform_mask == 0
    assert _batch().slice(4, 4).uniform_mask == 0


def test_in_place_write_drops_the_field():
    o = np.zeros((N, 3))
    # `id` and `flags` are tensors of their own (the twelve real fields are rows of ONE staging block: next test)
    b = _batch(o=o)
    full = b.uniform_mask
    assert full == SCALARS | ORIGIN | BIT["id"] | BIT["flags"]
    b.flags.fill_(abi.RAY_HAS_Q)
    assert b.uniform_mask == full & ~BIT["flags"]
    b.id.add_(0)
    assert b.uniform_mask == full & ~BIT["flags"] & ~BIT["id"]
    assert b.uniform_mask == full & ~BIT["flags"] & ~BIT["id"]  # reading the mask does not change it


def test_write_to_a_staging_row_drops_every_row():
    """The real fields of a from_arrays batch are rows of one staging block and share its version counter: an in-place write
    to any of them — a varying one included — drops the hint of all twelve; `id` and `flags` are tensors of their own."""
    b = _batch(o=np.zeros((N, 3)))
    assert b.uniform_mask & (SCALARS | ORIGIN) == SCALARS | ORIGIN
    b.dx.mul_(1.0)
    assert b.uniform_mask == BIT["id"] | BIT["flags"]
    b = _batch()
    b.intensity.mul_(0.5)
    assert b.uniform_mask == BIT["id"] | BIT["flags"]
    b = _batch()
    b.wavelength[3] = 500e-7
    assert b.uniform_mask == BIT["id"] | BIT["flags"]
    # dropped for good: putting the value back does not bring the hint back
    b.wavelength[3] = 780e-7
    assert b.uniform_mask == BIT["id"] | BIT["flags"]


def test_forget_uniform_and_read_only_mask():
    b = _batch()
    assert b.uniform_mask
    with pytest.raises(AttributeError):
        b.uniform_mask = 0
    assert b.forget_uniform() is b and b.uniform_mask == 0


def test_slice_propagates():
    b = _batch(o=np.zeros((N, 3)))
    full = b.uniform_mask
    assert b.slice(0, 10).uniform_mask == full
    assert b.slice(5, 20).uniform_mask == full & ~BIT["id"]  # id[lo:hi] is arange only from 0
    s = b.slice(0, 10)
    b.flags.fill_(0)  # a slice is a view: a write to the source is a write to it
    assert s.uniform_mask == full & ~BIT["flags"]
    s2 = b.slice(0, 10)
    s2.intensity.mul_(2.0)  # ... and the other way round
    assert b.uniform_mask == BIT["id"]


def test_multiplexed_in_wavelength_propagates_all_but_wavelength():
    b = _batch(o=np.zeros((N, 3)))
    m = b.multiplexed_in_wavelength(np.linspace(400e-7, 1100e-7, 4))
    assert m.uniform_mask == (SCALARS | ORIGIN | BIT["flags"]) & ~BIT["wavelength"]
    assert m.n == 4 * N and torch.equal(m.id, b.id.repeat(4))
    m.intensity.mul_(0.5)  # repeat() made tensors of their own: one field goes, the source keeps everything
    assert m.uniform_mask == (SCALARS | ORIGIN | BIT["flags"]) & ~BIT["wavelength"] & ~BIT["intensity"]
    assert b.uniform_mask == SCALARS | ORIGIN | BIT["id"] | BIT["flags"]
    # an entry already dropped in the source is not passed on
    b.flags.fill_(0)
    assert not b.multiplexed_in_wavelength([500e-7, 600e-7]).uniform_mask & BIT["flags"]


def test_clone_propagates():
    b = _batch(o=np.zeros((N, 3)))
    c = b.clone()
    assert c.uniform_mask == b.uniform_mask == SCALARS | ORIGIN | BIT["id"] | BIT["flags"]
    c.ox.add_(1.0)  # a clone's fields are tensors of their own
    assert c.uniform_mask == b.uniform_mask & ~BIT["ox"]
    assert b.uniform_mask == SCALARS | ORIGIN | BIT["id"] | BIT["flags"]


def test_constructors_that_carry_no_hint():
    b = _batch(o=np.zeros((N, 3)))
    assert b.take(torch.arange(N)).uniform_mask == 0
    assert b.sorted_spatially()[0].uniform_mask == 0
    assert b.astype("f32").uniform_mask == 0
    assert b.with_ids(torch.arange(N)).uniform_mask == 0
    assert RayBatch(N, device="cpu").uniform_mask == 0
    assert RayBatch(N, device="cpu", initialise=False).uniform_mask == 0
    assert b.uniform_mask  # (none of them touched the source)


def test_inference_mode_carries_no_hint():
    """Tensors made under torch.inference_mode() have no version counter to watch: such a batch is built as before and carries
    no hint; a batch built outside keeps its rule inside (an in-place write there still moves the counter)."""
    with torch.inference_mode():
        b = _batch(o=np.zeros((N, 3)))
        assert b.uniform_mask == 0 and b.clone().uniform_mask == 0 and b.slice(0, 5).uniform_mask == 0
    b = _batch(o=np.zeros((N, 3)))
    with torch.inference_mode():
        assert b.uniform_mask == SCALARS | ORIGIN | BIT["id"] | BIT["flags"]
        b.flags.fill_(0)
        assert b.uniform_mask == SCALARS | ORIGIN | BIT["id"]
        assert b.clone().uniform_mask == 0  # (the clone's tensors are inference tensors)


def test_the_numpy_alias_is_part_of_the_documented_hole():
    b = _batch()
    b.intensity.numpy()[3] = 5.0  # shares the memory, moves no counter
    assert b.uniform_mask & BIT["intensity"]
    assert b.forget_uniform().uniform_mask == 0
