"""GPU (MI355X): resident planes in the lane-per-ray kernel (k_trace_fused; include/optable_hip.h: OT_RESIDENT_*).  A trace into an
output that an earlier trace of the same engine wrote leaves the planes `ray`, `n` and `intensity` unwritten where the old records
reach and the scene keeps them invariant; the records must be the ones a trace into a FRESH output writes, bit for bit, in every
slot k < |count|.  That the skip ran is shown through the documented hole: a plane poisoned through `.data` (torch does not see
the write) keeps its poison.  n = 130: even (paired 16-byte stores), two full waves and a partial one; n = 129: odd (unpaired)."""
import numpy as np
import pytest
import torch

import scenes
import support
from optable_amd import abi

pytestmark = pytest.mark.gpu

RAY, N, I = abi.RESIDENT_RAY, abi.RESIDENT_N, abi.RESIDENT_INTENSITY
PLANES = {RAY: "ray", N: "n", I: "intensity"}
SIZES = (130, 129)
GRID = [(p, lay) for p in ("f64", "f32") for lay in ("slots", "tiled")]


# scene -> (components, the planes the library must report for a batch with uniform n and intensity)
SCENES = {
    "cfg2": (scenes.cfg2_components, RAY | N | I),
    "half": (support.half_mirror, RAY | N),       # a mirror with reflectivity 0.5: the intensity changes on the way
    "snell": (scenes.cfg4_components, RAY),       # refracting (preset FB): n changes on the way
    "cfg3": (scenes.cfg3_components, 0),          # 56 leaves: the rolling lists
}
def _engine(name):
    return support.engine_for(SCENES[name][0], (__name__, name))


def _long(n, seed=0):
    """cfg 2's own rays: out of the lens's focus, through the lens, twice off the roof mirrors, back through the lens — 5 segments"""
    return scenes.cfg2_rays(n, seed)


def _snell_rays(n, seed=0):
    o, d, _ = scenes.cfg4_rays(n, seed, n_wavelengths=1)
    return o, d


def _same(a, b, what="", but=()):
    for f in a:
        if f not in but:
            assert torch.equal(a[f], b[f]), (what, f)


POISON = {"ray": -7, "n": 123.0, "intensity": 77.0}


def _poison(out, fields=("ray", "n", "intensity")):
    """behind torch's back: the token stays"""
    for f in fields:
        out.field(f).data.fill_(POISON[f])


def _poisoned(rec, f):
    want = torch.full_like(rec[f].view(out_dtype(rec[f], f)), POISON[f])
    return torch.equal(rec[f].view(out_dtype(rec[f], f)), want)


def out_dtype(t, f):
    return torch.int32 if f == "ray" else {torch.int64: torch.float64, torch.int32: torch.float32}[t.dtype]


@pytest.mark.parametrize("precision, layout", GRID)
def test_second_trace_into_the_same_output(precision, layout):
    eng = _engine("cfg2")
    K = 5
    for n in SIZES:
        batch, again = support.batch(*_long(n, 0), precision), support.batch(*_long(n, 1), precision)
        fresh = support.valid_records(eng.trace(again, K, layout=layout), n, K)
        assert int(fresh["count"].min()) == K and eng.last_launch()["kernel"] == 1
        out = eng.trace(batch, K, out=support.new_out(n, K, precision, layout), layout=layout)
        assert out.resident_mask(n, layout, {N: again.uniform_bits("n"), I: again.uniform_bits("intensity")}, eng, eng._stream) == RAY | N | I
        assert eng.trace(again, K, out=out, layout=layout) is out
        _same(support.valid_records(out, n, K), fresh, (n, "second"))
        # the skip ran: poison written where torch does not see it survives in the three planes, and nowhere else
        _poison(out)
        eng.trace(again, K, out=out, layout=layout)
        rec = support.valid_records(out, n, K)
        _same(rec, fresh, (n, "poisoned"), but=("ray", "n", "intensity"))
        for f in ("ray", "n", "intensity"):
            assert _poisoned(rec, f), (n, f)
        # ... with the option off every record is written whole
        eng.set_option(abi.OPT_RESIDENT, 0)
        try:
            eng.trace(again, K, out=out, layout=layout)
            _same(support.valid_records(out, n, K), fresh, (n, "option off"))
            assert out._resident is None
        finally:
            eng.set_option(abi.OPT_RESIDENT, 1)
        # ... and after a write torch sees (any one of the watched tensors)
        eng.trace(again, K, out=out, layout=layout)
        _poison(out)
        out.ray.fill_(-7)
        eng.trace(again, K, out=out, layout=layout)
        _same(support.valid_records(out, n, K), fresh, (n, "visible write"))
        # ... and after forget_resident()
        _poison(out)
        eng.trace(again, K, out=out.forget_resident(), layout=layout)
        _same(support.valid_records(out, n, K), fresh, (n, "forgotten"))
        # a batch with another intensity: that plane is written again, the other two stay
        dim = support.batch(*_long(n, 1), precision, intensity=0.5)
        fresh_dim = support.valid_records(eng.trace(dim, K, layout=layout), n, K)
        _poison(out)
        eng.trace(dim, K, out=out, layout=layout)
        rec = support.valid_records(out, n, K)
        _same(rec, fresh_dim, (n, "dim"), but=("ray", "n"))
        assert _poisoned(rec, "ray") and _poisoned(rec, "n")
        # a batch that does not know its values (no host comparison): `ray` alone
        unknown = again.clone()
        unknown._uniform_value = {}
        _poison(out.forget_resident())
        eng.trace(unknown, K, out=out, layout=layout)   # whole records; the token it leaves holds `ray` only
        _poison(out)
        eng.trace(unknown, K, out=out, layout=layout)
        rec = support.valid_records(out, n, K)
        _same(rec, fresh, (n, "unknown"), but=("ray",))
        assert _poisoned(rec, "ray")


@pytest.mark.parametrize("precision, layout", GRID)
def test_rays_that_live_longer_than_last_time(precision, layout):
    """Whole waves and mixed waves of rays that escaped after 1-3 segments go through all 5 the second time: the wave writes full
    records from the first segment on that any of its rays is past its old count."""
    eng = _engine("cfg2")
    K = 5
    for n in SIZES:
        o, d, idx = support.short_rays(n)
        short, long_ = support.batch(o, d, precision), support.batch(*_long(n), precision)
        assert short.uniform_bits("n") == long_.uniform_bits("n") and short.uniform_bits("intensity") == long_.uniform_bits("intensity")
        long_out = eng.trace(long_, K, layout=layout)
        fresh_long = support.valid_records(long_out, n, K)
        fresh_short = support.valid_records(eng.trace(short, K, layout=layout), n, K)
        c = fresh_short["count"].abs().cpu().numpy()
        print("segments of the short rays:", np.bincount(c[idx], minlength=K + 1).tolist())
        assert c[idx].max() <= 3 and c[idx].min() == 1 and len(set(c[idx].tolist())) >= 2, np.bincount(c[idx]).tolist()
        assert (c[np.setdiff1d(np.arange(n), idx)] == K).all()
        assert (c[:64] < K).all() and (c[64:128] < K).any() and (c[64:128] == K).any()  # a whole wave, a mixed wave
        out = eng.trace(short, K, out=support.new_out(n, K, precision, layout), layout=layout)
        _same(support.valid_records(out, n, K), fresh_short, (n, "short"))
        _poison(out)  # whatever the old records do not cover must be written, whatever they cover may stay
        eng.trace(long_, K, out=out, layout=layout)
        rec = support.valid_records(out, n, K)
        _same(rec, fresh_long, (n, "long after short"), but=("ray", "n", "intensity"))
        got, want = out.to_slots(), long_out.to_slots()
        old = torch.arange(K, device="cuda")[:, None] < torch.as_tensor(c, device="cuda")[None, :]  # slots the first launch wrote
        for f in ("ray", "n", "intensity"):
            g, w = support.bits(got.field(f)[: K * n]).view(K, n), support.bits(want.field(f)[: K * n]).view(K, n)
            assert torch.equal(g[~old], w[~old]), (n, f, "slots past the old count")
            poison = support.bits(torch.full((1,), POISON[f], dtype=got.field(f).dtype, device="cuda"))
            assert bool(((g[old] == w[old]) | (g[old] == poison)).all()), (n, f)  # (what the old records cover may stay as it was)
            assert bool((g[0] == poison).all()), (n, f)  # segment 0: no ray is past its old count, every wave skips
        # the same without poison: equal everywhere
        out = eng.trace(short, K, out=support.new_out(n, K, precision, layout), layout=layout)
        eng.trace(long_, K, out=out, layout=layout)
        _same(support.valid_records(out, n, K), fresh_long, (n, "long after short, clean"))
        # ... and back: shorter than last time
        eng.trace(short, K, out=out, layout=layout)
        _same(support.valid_records(out, n, K), fresh_short, (n, "short after long"))
        eng.trace(long_, K, out=out, layout=layout)
        _same(support.valid_records(out, n, K), fresh_long, (n, "long again"))


@pytest.mark.parametrize("precision, layout", GRID)
def test_dead_rays_and_a_larger_cap(precision, layout):
    eng = _engine("cfg2")
    for n in SIZES:
        o, d, idx = support.short_rays(n)
        first, second = support.batch(o, d, precision), support.batch(*_long(n), precision)
        for b, step in ((first, 3), (second, 5)):
            flags = b.flags.cpu()
            flags[::step] |= abi.RAY_DEAD
            b.flags.copy_(flags)
        K1, K2 = 5, 7
        fresh = support.valid_records(eng.trace(second, K2, layout=layout), n, K2)
        assert torch.equal(fresh["count"][::5], torch.ones_like(fresh["count"][::5]))  # returned as they came: one record
        out = eng.trace(first, K1, out=support.new_out(n, K2, precision, layout), layout=layout)
        assert out._resident is not None
        eng.trace(second, K2, out=out, layout=layout)
        _same(support.valid_records(out, n, K2), fresh, (n, "dead"))
        eng.trace(first, K1, out=out, layout=layout)
        _same(support.valid_records(out, n, K1), support.valid_records(eng.trace(first, K1, layout=layout), n, K1), (n, "dead, back"))


@pytest.mark.parametrize("name", ["half", "snell"])
@pytest.mark.parametrize("precision, layout", GRID)
def test_planes_the_scene_changes_are_written(name, precision, layout):
    """A mirror with reflectivity 0.5: `intensity` is not resident; a refracting scene (preset FB): neither is `n`.  The library
    says so (ot_trace_resident_plan), and poison in such a plane is repaired while `ray` keeps it."""
    eng = _engine(name)
    planes = SCENES[name][1]
    K = 5 if name == "half" else 3
    for n in SIZES:
        batch = support.batch(*(_long(n) if name == "half" else _snell_rays(n)), precision)
        assert eng.resident_plan(precision, batch.uniform_mask, n, K) == planes
        assert eng.resident_plan(precision, 0, n, K) == RAY  # without the hint: `ray` alone
        fresh = support.valid_records(eng.trace(batch, K, layout=layout), n, K)
        assert int(fresh["count"].abs().min()) >= 2 and eng.last_launch()["kernel"] == 1
        out = eng.trace(batch, K, out=support.new_out(n, K, precision, layout), layout=layout)
        assert out._resident["planes"] == planes
        _poison(out)
        eng.trace(batch, K, out=out, layout=layout)
        rec = support.valid_records(out, n, K)
        kept = tuple(f for bit, f in PLANES.items() if planes & bit)
        _same(rec, fresh, (name, n), but=kept)
        for f in kept:
            assert _poisoned(rec, f), (name, n, f)
        # a caller's mask that is wrong for the scene skips nothing that changes: the library masks it
        _poison(out)
        support.trace_call(eng, "resident", batch, K, out, layout, batch.uniform_mask, abi.RESIDENT_ALL)
        rec = support.valid_records(out, n, K)
        _same(rec, fresh, (name, n, "all bits"), but=kept)


def test_rolling_list_scene_has_no_plan():
    eng = _engine("cfg3")
    n, K = 130, 20
    batch = support.batch(*scenes.cfg3_rays(n, 2), "f32")
    assert eng.resident_plan("f32", batch.uniform_mask, n, K) == 0
    fresh = support.valid_records(eng.trace(batch, K), n, K)
    assert eng.last_launch()["kernel"] == 2
    out = eng.trace(batch, K, out=support.new_out(n, K, "f32", "slots"))
    assert out._resident is None
    _poison(out)
    eng.trace(batch, K, out=out)
    _same(support.valid_records(out, n, K), fresh, "rolling")
    # and for the light scenes: no rays, or a cap the kernel's packed counts do not hold
    eng = _engine("cfg2")
    assert eng.resident_plan("f64", abi.UNIFORM_ALL, 0, 5) == 0 and eng.resident_plan("f64", abi.UNIFORM_ALL, n, 1 << 15) == 0
    assert eng.resident_plan("f64", abi.UNIFORM_ALL, n, (1 << 15) - 1) == RAY | N | I


@pytest.mark.parametrize("precision, layout", GRID)
def test_old_entry_points_write_the_records_of_the_new_ones_with_an_empty_mask(precision, layout):
    eng = _engine("cfg2")
    K = 5
    for n in SIZES:
        o, d, _ = support.short_rays(n)
        batch = support.batch(o, d, precision)
        recs = []
        for family, masks in (("uniform", (batch.uniform_mask,)), ("resident", (batch.uniform_mask, 0)), ("resident", (0, 0))):
            out = support.new_out(n, K, precision, layout)
            out.count = torch.zeros(n, dtype=torch.int32, device="cuda")
            out.n_rays = n
            assert support.trace_call(eng, family, batch, K, out, layout, *masks) == 0
            recs.append(support.valid_records(out, n, K))
        _same(recs[0], recs[1], (n, "uniform / resident"))
        _same(recs[0], recs[2], (n, "no masks"))
        out = support.new_out(n, K, precision, layout)
        out.count = torch.zeros(n, dtype=torch.int32, device="cuda")
        assert support.trace_call(eng, "resident", batch, K, out, layout, 0, abi.RESIDENT_ALL + 1) < 0  # bits outside the mask
        assert b"resident_mask" in eng.lib.ot_last_error()
