"""GPU (MI355X): the uniform-field hint in the lane-per-ray kernel (k_trace_fused, k_stream_ceiling: kernels.h load_ray).  A field
flagged in a batch's `uniform_mask` is read once per wave instead of once per ray; the records must be the ones the kernel writes
with the hint switched off (OT_OPT_UNIFORM = 0), bit for bit.  n = 130: even (paired 16-byte stores), two full waves and a partial
one; n = 129: odd (unpaired stores)."""
import numpy as np
import pytest
import torch

import scenes
import support
from optable_amd import abi

pytestmark = pytest.mark.gpu

BIT = abi.UNIFORM_BIT
SCALARS = BIT["wavelength"] | BIT["q_re"] | BIT["q_im"] | BIT["intensity"] | BIT["n"] | BIT["pathlength"]
ORIGIN = BIT["ox"] | BIT["oy"] | BIT["oz"]
DIRECTION = BIT["dx"] | BIT["dy"] | BIT["dz"]
IDF = BIT["id"] | BIT["flags"]

# scene -> (components, segments per ray, a ray that hits: origin, direction)
SCENES = {
    "cfg2": (scenes.cfg2_components, 5, np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])),
    "snell": (scenes.cfg4_components, 3, np.array([-3.0, 2.0, 0.0]), np.array([np.cos(np.pi / 6), -np.sin(np.pi / 6), 0.0])),
}
def _engine(name):
    return support.engine_for(SCENES[name][0], (__name__, name))


def _rays(name, n, spread_origin, spread_direction, seed=7):
    _, _, o0, d0 = SCENES[name]
    rng = np.random.default_rng(seed)
    o = np.tile(o0, (n, 1))
    d = np.tile(d0, (n, 1))
    if spread_origin:
        o = o + rng.uniform(-0.05, 0.05, (n, 3))
    if spread_direction:
        d = d + rng.uniform(-0.03, 0.03, (n, 3))
    return o, d


def _varying(n):
    """the six 'scalar' fields as arrays with no two elements alike"""
    j = np.arange(n)
    return dict(wavelength=scenes.WL * (1 + 1e-3 * j / n), intensity=1.0 - 0.5 * j / n, q=support.Q * (1 + 1e-3 * j / n) + 1e-3 * (j + 1),
                n_index=1.0 + 1e-3 * (j + 1) / n, pathlength=1e-3 * (j + 1))


# mask class -> (batch maker, the mask it must have)
def _classes(name, n, precision):
    rev = np.arange(n, dtype=np.int32)[::-1].copy()
    return {
        "none": (lambda: support.batch(*_rays(name, n, True, True), precision, ids=rev, **_varying(n)), BIT["flags"]),  # (flags: dropped below)
        "scalars": (lambda: support.batch(*_rays(name, n, True, True), precision), SCALARS | IDF),
        "scalars+origin": (lambda: support.batch(*_rays(name, n, False, True), precision), SCALARS | ORIGIN | IDF),
        "direction": (lambda: support.batch(*_rays(name, n, True, False), precision, ids=rev, **_varying(n)), DIRECTION | BIT["flags"]),
        "flags+id": (lambda: support.batch(*_rays(name, n, True, True), precision, **_varying(n)), IDF),
        "everything": (lambda: support.batch(*_rays(name, n, False, False), precision), abi.UNIFORM_ALL),
    }


def _same(a, b, what=""):
    for f in a:
        assert torch.equal(a[f], b[f]), (what, f)


def _trace_both(eng, batch, K, layout):
    """(records with the hint, records with OT_OPT_UNIFORM = 0) of the same batch"""
    n = batch.n
    hinted = support.valid_records(eng.trace(batch, K, layout=layout), n, K)
    eng.set_option(abi.OPT_UNIFORM, 0)
    try:
        plain = support.valid_records(eng.trace(batch, K, layout=layout), n, K)
    finally:
        eng.set_option(abi.OPT_UNIFORM, 1)
    return hinted, plain


@pytest.mark.parametrize("layout", ["slots", "tiled"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_hinted_trace_equals_unhinted(name, precision, layout):
    eng = _engine(name)
    K = SCENES[name][1]
    for n in (130, 129):
        for label, (make, mask) in _classes(name, n, precision).items():
            batch = make()
            if label == "none":
                batch.flags.copy_(batch.flags.clone())  # an in-place write: `flags` is no longer vouched for
                mask = 0
            assert batch.uniform_mask == mask, (label, n, bin(batch.uniform_mask))
            hinted, plain = _trace_both(eng, batch, K, layout)
            _same(hinted, plain, (label, n))
            assert eng.last_launch()["kernel"] == 1  # the lane-per-ray kernel
            assert int(hinted["count"].abs().min()) >= 2, (label, n)  # (the rays do hit something)
            assert batch.uniform_mask == mask  # a trace writes nothing into the caller's batch


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_dead_rays_and_foreign_ids(name, precision):
    eng = _engine(name)
    K = SCENES[name][1]
    for n in (130, 129):
        batch = support.batch(*_rays(name, n, False, True), precision)
        flags = batch.flags.cpu()
        flags[::3] |= abi.RAY_DEAD
        batch.flags.copy_(flags)
        assert batch.uniform_mask == SCALARS | ORIGIN | BIT["id"]
        for layout in ("slots", "tiled"):
            hinted, plain = _trace_both(eng, batch, K, layout)
            _same(hinted, plain, ("dead", n, layout))
            assert torch.equal(hinted["count"][::3], torch.ones_like(hinted["count"][::3]))  # returned as they came: one record
        # ids that are not arange(n) are not flagged, and the records do not depend on them
        ids = (np.arange(n, dtype=np.int32) * 7) % n
        other = support.batch(*_rays(name, n, False, True), precision, ids=ids)
        assert other.uniform_mask == SCALARS | ORIGIN | BIT["flags"]
        hinted, plain = _trace_both(eng, other, K, "slots")
        _same(hinted, plain, ("ids", n))


def test_the_kernel_reads_a_flagged_field_once():
    """That the mask reaches the kernel, shown through the documented hole: a write through `.data` does not move the version
    counter, so the field stays flagged and every ray is traced with element 0 of it; `forget_uniform()` is the way out."""
    eng = _engine("cfg2")
    n = 130
    batch = support.batch(*_rays("cfg2", n, False, True), "f64")
    batch.intensity.data[5] = 3.0
    assert batch.uniform_mask & BIT["intensity"]
    first = eng.trace(batch, 5).intensity[:n].clone()
    assert torch.equal(first, torch.ones_like(first))
    batch.forget_uniform()
    assert batch.uniform_mask == 0
    first = eng.trace(batch, 5).intensity[:n].clone()
    assert first[5].item() == 3.0 and int((first == 1.0).sum()) == n - 1


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_in_place_edits_are_followed(precision):
    """The CPU rules on device tensors, and the traced records after an edit."""
    eng = _engine("cfg2")
    n = 130
    batch = support.batch(*_rays("cfg2", n, False, True), precision)
    assert batch.uniform_mask == SCALARS | ORIGIN | IDF
    batch.intensity.mul_(0.5)  # a row of the staging block: every real field's entry goes with it
    assert batch.uniform_mask == IDF
    first = eng.trace(batch, 5).intensity[:n]
    assert torch.equal(first, torch.full_like(first, 0.5))
    for layout in ("slots", "tiled"):
        _same(*_trace_both(eng, batch, 5, layout), what=layout)
    # slices, clones and wavelength copies pass the hint on; gathers do not
    batch = support.batch(*_rays("cfg2", n, False, True), precision)
    full = batch.uniform_mask
    assert batch.slice(0, 64).uniform_mask == full and batch.slice(3, 64).uniform_mask == full & ~BIT["id"]
    assert batch.clone().uniform_mask == full
    assert batch.multiplexed_in_wavelength([500e-7, 600e-7]).uniform_mask == full & ~BIT["wavelength"] & ~BIT["id"]
    assert batch.take(torch.arange(n, device="cuda")).uniform_mask == 0 and batch.sorted_spatially()[0].uniform_mask == 0
    part = batch.slice(3, 64 + 3)
    _same(*_trace_both(eng, part, 5, "slots"), what="slice")
    batch.flags.fill_(abi.RAY_HAS_Q)
    assert batch.uniform_mask == full & ~BIT["flags"] and part.uniform_mask == full & ~IDF


def test_one_wavelength_edit_changes_one_ray():
    eng = _engine("snell")
    n, K = 130, 3
    batch = support.batch(*_rays("snell", n, True, False), "f64")
    assert batch.uniform_mask == SCALARS | DIRECTION | IDF
    before = eng.trace(batch, K)
    assert int(before.count.min()) == K  # every slot compared below is a written one
    before = {f: support.bits(before.field(f)[: K * n]).view(K, n).clone() for f in abi.SEG_FIELDS}
    batch.wavelength[7] = 500e-7
    assert not batch.uniform_mask & BIT["wavelength"]
    after = eng.trace(batch, K)
    assert int(after.count.min()) == K
    after = {f: support.bits(after.field(f)[: K * n]).view(K, n).clone() for f in abi.SEG_FIELDS}
    others = torch.arange(n, device="cuda") != 7
    for f in abi.SEG_FIELDS:
        assert torch.equal(before[f][:, others], after[f][:, others]), f
    assert not torch.equal(before["dy"][1, 7], after["dy"][1, 7])  # inside the glass the ray of another colour goes another way


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_stream_ceiling_honours_the_hint(precision, tiled):
    from optable_amd.batch import SegmentBatch

    eng = _engine("cfg2")
    K = 5
    for n in (130, 129):
        batch = support.batch(*_rays("cfg2", n, False, True), precision)
        assert batch.uniform_mask == SCALARS | ORIGIN | IDF
        got = []
        for option in (1, 0):
            out = SegmentBatch(n * K, precision, "cuda", tiled=tiled)
            eng.set_option(abi.OPT_UNIFORM, option)
            try:
                eng.stream_ceiling(batch, K, out)
            finally:
                eng.set_option(abi.OPT_UNIFORM, 1)
            out.n_rays = n
            got.append(support.valid_records(out, n, K))
        _same(got[0], got[1], (n, tiled))
        assert int(got[0]["count"].min()) == K


def test_heavy_scene_ignores_the_hint():
    """A scene that goes to the rolling lists reads the full arrays: same records from a hinted batch and an unhinted clone."""
    import optable_amd as oa
    from optable_amd.engine import get_engine

    table = oa.OpticalTable()
    table.add_components(scenes.cfg3_components(oa))
    eng = get_engine()
    eng.upload(table.compile())
    n, K = 1030, 20
    batch = support.batch(*scenes.cfg3_rays(n, 2), "f32")
    plain = batch.clone().forget_uniform()
    assert batch.uniform_mask == SCALARS | BIT["ox"] | IDF and plain.uniform_mask == 0
    a = support.valid_records(eng.trace(batch, K), n, K)
    assert eng.last_launch()["kernel"] != 1
    b = support.valid_records(eng.trace(plain, K), n, K)
    _same(a, b)


def test_mask_bits_outside_the_set_are_refused():
    import ctypes as C

    from optable_amd.batch import SegmentBatch

    eng = _engine("cfg2")
    batch = support.batch(*_rays("cfg2", 130, False, True), "f64")
    out = SegmentBatch(130 * 5, "f64", "cuda")
    out.count = torch.empty(130, dtype=torch.int32, device="cuda")
    rs, ss = batch.c_struct(), out.c_struct()
    rc = eng.lib.ot_trace_uniform_f64(eng._ctx, C.byref(rs), 130, 5, C.byref(ss), out.count.data_ptr(), None, 0, abi.UNIFORM_ALL + 1)
    assert rc != 0 and b"uniform_mask" in eng.lib.ot_last_error()


_KW = {"wavelength": "wavelength", "intensity": "intensity", "n": "n_index", "pathlength": "pathlength"}


def _only(field, n, precision):
    """A Snell-scene batch in which `field` alone holds one value: its siblings vary, `id` is not arange, `flags` is written to."""
    o, d = _rays("snell", n, True, True)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    kw = _varying(n)
    if field[0] in "od":
        (o if field[0] == "o" else d)[:, "xyz".index(field[1])] = SCENES["snell"][2 if field[0] == "o" else 3]["xyz".index(field[1])]
    elif field in ("q_re", "q_im"):
        q = kw["q"]
        kw["q"] = (support.Q.imag * 0 + 0.25) + 1j * q.imag if field == "q_re" else q.real + 1j * support.Q.imag
    else:
        kw[_KW[field]] = {"wavelength": scenes.WL, "intensity": 0.75, "n": 1.0, "pathlength": 0.5}[field]
    batch = support.batch(o, d, precision, ids=np.arange(n, dtype=np.int32)[::-1].copy(), normalize=False, **kw)
    batch.flags.copy_(batch.flags.clone())
    return batch


@pytest.mark.parametrize("layout", ["slots", "tiled"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_every_bit_names_its_own_field(precision, layout):
    """One field of a group flagged, its siblings varying — a bit that read a neighbour's array would show — and, through the
    documented hole, that the kernel does read element 0 of exactly that field: with element 5 changed behind torch's back the
    hinted trace still gives the records of the untouched batch."""
    eng = _engine("snell")
    n, K = 130, 3
    for field in abi.RAY_FIELDS:
        batch = _only(field, n, precision)
        assert batch.uniform_mask == BIT[field], (field, bin(batch.uniform_mask))
        hinted, plain = _trace_both(eng, batch, K, layout)
        _same(hinted, plain, field)
        t = batch.field(field)
        t.data[5] = t.data[5] * 1.5 + 0.01
        assert batch.uniform_mask == BIT[field]
        poked, seen = _trace_both(eng, batch, K, layout)
        _same(poked, plain, ("element 0 for every ray", field))
        if field != "wavelength" and int(plain["count"][5]) == int(seen["count"][5]):  # (read per ray, the edit shows in ray 5's records)
            assert any(not torch.equal(seen[f], plain[f]) for f in abi.SEG_FIELDS), field
