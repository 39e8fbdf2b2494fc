"""GPU (MI355X): first-segment fields in the lane-per-ray kernel (k_trace_fused; include/optable_hip.h: ot_trace_reuse_*).  Segment 0
of a ray is the input ray handed through, so a trace into an output an earlier trace of the same engine wrote leaves, at k = 0,
the planes unwritten whose field the batch holds one bit pattern in — the same pattern as last time.  The records must be the ones
a trace into a FRESH output writes, bit for bit.  That the skip ran, and where, is shown through the documented hole: a plane
poisoned through `.data` (torch does not see the write) keeps its poison in the slots the launch left alone, and nowhere else.
n = 130: even (paired 16-byte stores), two full waves and a partial one; n = 129: odd (unpaired)."""
import numpy as np
import pytest
import torch

import scenes
import support
from optable_amd import abi

pytestmark = pytest.mark.gpu

RAY, N, I = abi.RESIDENT_RAY, abi.RESIDENT_N, abi.RESIDENT_INTENSITY
BIT = abi.UNIFORM_BIT
ELEVEN = ("ox", "oy", "oz", "dx", "dy", "dz", "q_re", "q_im", "intensity", "n", "pathlength")
POINT = ("ox", "oy", "oz", "q_re", "q_im", "pathlength")  # what cfg 2's point source adds to the resident n and intensity
VARYING = ("dx", "dy", "dz", "length", "surface")
ALL_FIELDS = abi.SEG_FIELDS + ("ray", "surface")
SIZES = (130, 129)
GRID = [(p, lay) for p in ("f64", "f32") for lay in ("slots", "tiled")]


# scene -> (components, the planes ot_trace_resident_plan reports for a batch with uniform n and intensity: unchanged by this feature)
SCENES = {
    "cfg2": (scenes.cfg2_components, RAY | N | I),
    "half": (support.half_mirror, RAY | N),
    "snell": (scenes.cfg4_components, RAY),
    "cfg3": (scenes.cfg3_components, 0),
}
def _engine(name):
    return support.engine_for(SCENES[name][0], (__name__, name))


def _check(got, want, kept0=(), kept_all=(), live=None, what=""):
    """`got` = (planes, count, valid) of the poisoned output, `want` of the fresh one: the same records, except that the fields
    `kept0` hold poison at k = 0 (live: for these rays only; the others hold the record) and `kept_all` wherever a record is."""
    (g, gc, valid), (w, wc, wvalid) = got, want
    assert torch.equal(gc, wc) and torch.equal(valid, wvalid), (what, "count")
    for f in ALL_FIELDS:
        poison = support.value_poison(g[f], f)
        if f in kept_all:
            assert bool((g[f][valid] == poison).all()), (what, f, "resident plane")
            continue
        assert torch.equal(g[f][1:][valid[1:]], w[f][1:][valid[1:]]), (what, f, "k >= 1")
        if f in kept0:
            rays = valid[0] if live is None else valid[0] & live
            assert bool((g[f][0][rays] == poison).all()), (what, f, "slot 0 was written")
            assert torch.equal(g[f][0][valid[0] & ~rays], w[f][0][valid[0] & ~rays]), (what, f, "slot 0 of the other rays")
        else:
            assert torch.equal(g[f][0][valid[0]], w[f][0][valid[0]]), (what, f, "slot 0")


def _mask(fields):
    return sum(BIT[f] for f in fields)


@pytest.mark.parametrize("precision, layout", GRID)
def test_second_trace_into_the_same_output(precision, layout):
    eng = _engine("cfg2")
    K = 5
    everything = tuple(f for f in ALL_FIELDS if f not in ("ray", "n", "intensity"))
    for n in SIZES:
        batch, again = support.batch(*scenes.cfg2_rays(n, 0), precision), support.batch(*scenes.cfg2_rays(n, 1), precision)
        assert eng.first_plan(precision, again.uniform_mask, n, K) == _mask(POINT + ("n", "intensity"))
        want = support.planes(eng.trace(again, K, layout=layout), n, K)
        assert int(want[1].min()) == K and eng.last_launch()["kernel"] == 1
        out = eng.trace(batch, K, out=support.new_out(n, K, precision, layout), layout=layout)
        assert set(out._first["values"]) == set(POINT + ("n", "intensity"))
        assert eng.trace(again, K, out=out, layout=layout) is out
        _check(support.planes(out, n, K), want, what=(n, "second"))
        # the skip ran, at k = 0 and nowhere else; the planes that vary are repaired at every k
        support.poison_behind_torch(out, everything)
        eng.trace(again, K, out=out, layout=layout)
        _check(support.planes(out, n, K), want, kept0=POINT, what=(n, "poisoned"))
        # ... together with the resident planes, which keep theirs at every k
        support.poison_behind_torch(out, ALL_FIELDS)
        eng.trace(again, K, out=out, layout=layout)
        _check(support.planes(out, n, K), want, kept0=POINT, kept_all=("ray", "n", "intensity"), what=(n, "poisoned, all planes"))
        # a write torch sees, to one watched plane, ends the first-segment token (the other one stands on other tensors)
        eng.trace(again, K, out=out.forget_resident(), layout=layout)
        support.poison_behind_torch(out, everything)
        out.q_re.mul_(1.0)
        eng.trace(again, K, out=out, layout=layout)
        _check(support.planes(out, n, K), want, what=(n, "visible write"))
        # ... and forget_resident()
        support.poison_behind_torch(out, ALL_FIELDS)
        eng.trace(again, K, out=out.forget_resident(), layout=layout)
        _check(support.planes(out, n, K), want, what=(n, "forgotten"))


def _varied(n, precision, but, seed=5):
    """cfg 2's rays with EVERY field of the eleven different from ray to ray, except `but`"""
    rng = np.random.default_rng(seed)
    o, d = scenes.cfg2_rays(n, seed)
    o = o + rng.uniform(-0.01, 0.01, (n, 3))
    cols = {"ox": o[:, 0], "oy": o[:, 1], "oz": o[:, 2], "dx": d[:, 0], "dy": d[:, 1], "dz": d[:, 2]}
    if but in cols:
        cols[but][:] = cols[but][0]  # (directions are handed over as they are: normalize=False)
    q = support.Q * (1 + rng.uniform(0, 0.1, n)) + rng.uniform(0.1, 0.2, n)
    if but == "q_re":
        q = q.real[0] + 1j * q.imag
    if but == "q_im":
        q = q.real + 1j * q.imag[0]
    kw = {"intensity": rng.uniform(0.5, 1.0, n), "n_index": rng.uniform(1.0, 1.1, n), "pathlength": rng.uniform(0.0, 1.0, n)}
    key = {"intensity": "intensity", "n": "n_index", "pathlength": "pathlength"}.get(but)
    if key:
        kw[key] = float(kw[key][0])
    batch = support.batch(o, d, precision, q=q, normalize=False, **kw)
    assert batch.uniform_mask & abi.FIRST_FIELDS == BIT[but], (but, batch.uniform_mask)
    return batch


@pytest.mark.parametrize("precision, layout", GRID)
def test_each_field_flagged_alone_among_varying_siblings(precision, layout):
    eng = _engine("cfg2")
    K = 5
    poisoned = abi.SEG_FIELDS + ("surface",)
    for n in SIZES:
        for f in ELEVEN:
            batch = _varied(n, precision, f)
            um = batch.uniform_mask
            fresh = support.new_out(n, K, precision, layout, zero_count=True)
            assert support.trace_call(eng, "reuse", batch, K, fresh, layout, um, 0, 0) == 0
            want = support.planes(fresh, n, K)
            assert int(want[1].abs().min()) >= 1
            # the first launch into an output writes whole records whatever the caller says (no ray has an old record)
            out = support.new_out(n, K, precision, layout, zero_count=True)
            support.poison_behind_torch(out, poisoned)
            assert support.trace_call(eng, "reuse", batch, K, out, layout, um, 0, abi.FIRST_FIELDS) == 0
            _check(support.planes(out, n, K), want, what=(n, f, "first launch"))
            # the second: that plane's slot 0 alone keeps poison ...
            support.poison_behind_torch(out, poisoned)
            assert support.trace_call(eng, "reuse", batch, K, out, layout, um, 0, BIT[f]) == 0
            _check(support.planes(out, n, K), want, kept0=(f,), what=(n, f))
            # ... also when the caller flags all eleven: the library masks its word with the uniform mask
            support.poison_behind_torch(out, poisoned)
            assert support.trace_call(eng, "reuse", batch, K, out, layout, um, 0, abi.FIRST_FIELDS) == 0
            _check(support.planes(out, n, K), want, kept0=(f,), what=(n, f, "all bits"))


@pytest.mark.parametrize("precision, layout", GRID)
def test_a_changed_source_is_written(precision, layout):
    eng = _engine("cfg2")
    K = 5
    everything = tuple(f for f in ALL_FIELDS if f not in ("ray", "n", "intensity"))
    for n in SIZES:
        o, d = scenes.cfg2_rays(n, 0)
        first = support.batch(o, d, precision)
        moved = o + [0.0, 0.015625, 0.0]
        minus = o.copy()
        minus[:, 2] = -0.0
        spread = o.copy()
        spread[:, 0] = np.linspace(-0.01, 0.01, n)
        for name, origin, written in (("moved", moved, ("oy",)), ("minus zero", minus, ("oz",)), ("not uniform", spread, ("ox",))):
            second = support.batch(origin, d, precision)
            want = support.planes(eng.trace(second, K, layout=layout), n, K)
            out = eng.trace(first, K, out=support.new_out(n, K, precision, layout), layout=layout)
            support.poison_behind_torch(out, everything)
            eng.trace(second, K, out=out, layout=layout)
            _check(support.planes(out, n, K), want, kept0=tuple(f for f in POINT if f not in written), what=(n, name))
            # what that launch wrote is what the next one may keep (a pattern, if it has one)
            support.poison_behind_torch(out, everything)
            eng.trace(second, K, out=out, layout=layout)
            _check(support.planes(out, n, K), want, kept0=tuple(f for f in POINT if f != "ox" or name != "not uniform"), what=(n, name, "again"))
        # first launch not uniform in a field, second uniform: written
        out = eng.trace(support.batch(spread, d, precision), K, out=support.new_out(n, K, precision, layout), layout=layout)
        assert "ox" not in out._first["values"]
        want = support.planes(eng.trace(first, K, layout=layout), n, K)
        support.poison_behind_torch(out, everything)
        eng.trace(first, K, out=out, layout=layout)
        _check(support.planes(out, n, K), want, kept0=tuple(f for f in POINT if f != "ox"), what=(n, "uniform after spread"))


@pytest.mark.parametrize("name", ["half", "snell"])
@pytest.mark.parametrize("precision, layout", GRID)
def test_the_first_segment_does_not_depend_on_the_scene(name, precision, layout):
    """A mirror with reflectivity 0.5 changes `intensity` on the way, a refracting scene (preset FB) `n` as well: not resident planes
    (ot_trace_resident_plan reports what it did), yet segment 0 carries the input's values.  Through the C ABI: `Engine.trace`
    does not flag these two fields of its own accord (engine.py _launch)."""
    eng = _engine(name)
    planes = SCENES[name][1]
    K = 5 if name == "half" else 3
    for n in SIZES:
        if name == "half":
            batch = support.batch(*scenes.cfg2_rays(n, 0), precision)
        else:
            o, d, _ = scenes.cfg4_rays(n, 0, n_wavelengths=1)
            batch = support.batch(o, d, precision)
        um = batch.uniform_mask
        assert eng.resident_plan(precision, um, n, K) == planes and eng.resident_plan(precision, 0, n, K) == RAY
        assert eng.first_plan(precision, um, n, K) == um & abi.FIRST_FIELDS and eng.first_plan(precision, 0, n, K) == 0
        out = support.new_out(n, K, precision, layout, zero_count=True)
        assert support.trace_call(eng, "reuse", batch, K, out, layout, um, 0, 0) == 0
        want = support.planes(out, n, K)
        assert int(want[1].abs().min()) >= 2 and eng.last_launch()["kernel"] == 1
        support.poison_behind_torch(out, ("n", "intensity"))
        assert support.trace_call(eng, "reuse", batch, K, out, layout, um, abi.RESIDENT_ALL, BIT["n"] | BIT["intensity"]) == 0
        resident = tuple(f for bit, f in ((N, "n"), (I, "intensity")) if planes & bit)
        _check(support.planes(out, n, K), want, kept0=("n", "intensity"), kept_all=resident, what=(name, n))
        # Engine.trace: those two planes of a reused output are written whole where the scene changes them
        out = eng.trace(batch, K, out=support.new_out(n, K, precision, layout), layout=layout)
        assert out._resident["planes"] == planes and {"n", "intensity"} <= set(out._first["values"])
        support.poison_behind_torch(out, ("n", "intensity", "pathlength"))
        eng.trace(batch, K, out=out, layout=layout)
        _check(support.planes(out, n, K), want, kept0=("pathlength",), kept_all=resident, what=(name, n, "engine"))


@pytest.mark.parametrize("precision, layout", GRID)
def test_dead_rays_get_whole_records_and_a_cap_of_one(precision, layout):
    eng = _engine("cfg2")
    everything = tuple(f for f in ALL_FIELDS if f not in ("ray", "n", "intensity"))
    for n in SIZES:
        first, second = support.batch(*scenes.cfg2_rays(n, 0), precision), support.batch(*scenes.cfg2_rays(n, 1), precision)
        for b, step in ((first, 3), (second, 5)):
            flags = b.flags.cpu()
            flags[::step] |= abi.RAY_DEAD
            b.flags.copy_(flags)
        K = 5
        want = support.planes(eng.trace(second, K, layout=layout), n, K)
        assert torch.equal(want[1][::5], torch.ones_like(want[1][::5]))  # returned as they came: one record
        out = eng.trace(first, K, out=support.new_out(n, K, precision, layout), layout=layout)
        assert out._first is not None
        support.poison_behind_torch(out, everything)
        eng.trace(second, K, out=out, layout=layout)
        live = torch.ones(n, dtype=torch.bool, device="cuda")
        live[::5] = False
        _check(support.planes(out, n, K), want, kept0=POINT, live=live, what=(n, "dead"))
        # K = 1: the record the loop writes is segment 0
        plain, again = support.batch(*scenes.cfg2_rays(n, 0), precision), support.batch(*scenes.cfg2_rays(n, 1), precision)
        want = support.planes(eng.trace(again, 1, layout=layout), n, 1)
        out = eng.trace(plain, 1, out=support.new_out(n, 1, precision, layout), layout=layout)
        eng.trace(again, 1, out=out, layout=layout)
        _check(support.planes(out, n, 1), want, what=(n, "K = 1"))
        support.poison_behind_torch(out, everything)
        eng.trace(again, 1, out=out, layout=layout)
        _check(support.planes(out, n, 1), want, kept0=POINT, what=(n, "K = 1, poisoned"))


def test_a_cap_the_packed_counts_do_not_hold_drops_the_mask():
    eng = _engine("cfg2")
    n = 130
    for precision in ("f64", "f32"):
        assert eng.first_plan(precision, abi.UNIFORM_ALL, n, (1 << 15) - 1) == abi.FIRST_FIELDS
        assert eng.first_plan(precision, abi.UNIFORM_ALL, n, 1 << 15) == 0
        assert eng.first_plan(precision, abi.UNIFORM_ALL, 0, 5) == 0
        assert eng.first_plan(precision, BIT["wavelength"] | abi.UNIFORM_ID | abi.UNIFORM_FLAGS | BIT["oy"], n, 5) == BIT["oy"]
    assert eng.resident_plan("f64", abi.UNIFORM_ALL, n, (1 << 15) - 1) == RAY | N | I and eng.resident_plan("f64", abi.UNIFORM_ALL, n, 1 << 15) == 0


@pytest.mark.parametrize("precision, layout", GRID)
def test_knobs_and_entry_points(precision, layout):
    eng = _engine("cfg2")
    K = 5
    everything = tuple(f for f in ALL_FIELDS if f not in ("ray", "n", "intensity"))
    for n in SIZES:
        batch, again = support.batch(*scenes.cfg2_rays(n, 0), precision), support.batch(*scenes.cfg2_rays(n, 1), precision)
        um = again.uniform_mask
        want = support.planes(eng.trace(again, K, layout=layout), n, K)
        out = eng.trace(batch, K, out=support.new_out(n, K, precision, layout), layout=layout)
        # OT_OPT_RESIDENT 2: planes only; 0: neither; OT_OPT_UNIFORM 0: no first-segment fields (and no resident n / intensity)
        for option, value, kept in ((abi.OPT_RESIDENT, 2, ("ray", "n", "intensity")), (abi.OPT_RESIDENT, 0, ()), (abi.OPT_UNIFORM, 0, ("ray",))):
            eng.set_option(option, value)
            try:
                assert eng.first_plan(precision, um, n, K) == 0
                support.poison_behind_torch(out, ALL_FIELDS)
                eng.trace(again, K, out=out, layout=layout)
                _check(support.planes(out, n, K), want, kept_all=kept, what=(n, option, value))
            finally:
                eng.set_option(option, 1)
            eng.trace(again, K, out=out.forget_resident(), layout=layout)  # whole records again, and both tokens
            assert eng.first_plan(precision, um, n, K) == um & abi.FIRST_FIELDS
        support.poison_behind_torch(out, everything)
        eng.trace(again, K, out=out, layout=layout)
        _check(support.planes(out, n, K), want, kept0=POINT, what=(n, "knobs back"))
        # the old entry points are the new ones with an empty first mask: the same records, nothing kept at slot 0
        for family, masks in (("resident", (um, 0)), ("resident", (um, abi.RESIDENT_ALL)), ("reuse", (um, abi.RESIDENT_ALL, 0)), ("uniform", (um,))):
            support.poison_behind_torch(out, everything)
            assert support.trace_call(eng, family, again, K, out, layout, *masks) == 0
            _check(support.planes(out, n, K), want, what=(n, family, masks))
        # bits outside the eleven, and outside the planes, are refused by name
        for bad in (BIT["wavelength"], abi.UNIFORM_ID, abi.UNIFORM_FLAGS, 1 << 14):
            assert support.trace_call(eng, "reuse", again, K, out, layout, um, 0, bad) < 0
            assert b"first_mask" in eng.lib.ot_last_error()
        assert support.trace_call(eng, "reuse", again, K, out, layout, um, abi.RESIDENT_ALL + 1, 0) < 0
        assert b"resident_mask" in eng.lib.ot_last_error()
        assert support.trace_call(eng, "resident", again, K, out, layout, um, abi.RESIDENT_ALL + 1) < 0
        assert b"resident_mask" in eng.lib.ot_last_error()


def test_a_heavy_scene_ignores_the_mask_and_leaves_no_token():
    eng = _engine("cfg3")
    n, K = 130, 20
    batch = support.batch(*scenes.cfg3_rays(n, 2), "f32")
    um = batch.uniform_mask
    assert um & abi.FIRST_FIELDS and eng.first_plan("f32", um, n, K) == 0 and eng.resident_plan("f32", um, n, K) == 0
    want = support.planes(eng.trace(batch, K), n, K)
    assert eng.last_launch()["kernel"] == 2
    out = eng.trace(batch, K, out=support.new_out(n, K, "f32", "slots"))
    assert out._first is None and out._resident is None
    support.poison_behind_torch(out, ALL_FIELDS)
    eng.trace(batch, K, out=out)
    _check(support.planes(out, n, K), want, what="rolling")
    support.poison_behind_torch(out, ALL_FIELDS)
    assert support.trace_call(eng, "reuse", batch, K, out, "slots", um, abi.RESIDENT_ALL, abi.FIRST_FIELDS) == 0
    _check(support.planes(out, n, K), want, what="rolling, C ABI")
