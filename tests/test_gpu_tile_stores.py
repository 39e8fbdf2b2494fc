"""GPU (MI355X): the tiled segment stores of the lane-per-ray kernel (k_trace_fused / k_stream_ceiling with OUT = SegTiles, kernels.h).
A tile is written one element per lane from ONE place in the segment loop, never through the lane pairs of the slot arrays.  The
records must be those of the slot arrays, bit for bit, whatever OT_OPT_PAIR_STORES says; nothing may be written past a ray's count
(unused slots and the last tile's padding keep a poison written beforehand); and a reused output (resident planes, first-segment
fields) holds what a fresh one holds.  n = 130: two full waves and a two-lane one, even (went through the pairs before); 129: odd."""
import numpy as np
import pytest
import torch

import scenes
from optable_amd import abi

pytestmark = pytest.mark.gpu

ALL_FIELDS = abi.SEG_FIELDS + ("ray", "surface")
RESIDENT = ("ray", "n", "intensity")
POINT = ("ox", "oy", "oz", "q_re", "q_im", "pathlength")  # what cfg 2's point source adds to the resident n and intensity at k = 0
Q = 1j * np.pi * scenes.W0**2 / scenes.WL
POISON_BYTE = 0xA5
POISON_REAL, POISON_INT = 123.0, -7
COMPONENTS = {"cfg2": scenes.cfg2_components, "snell": scenes.cfg4_components}
_compiled = {}


def _engine(name):
    import optable_amd as oa
    from optable_amd.engine import get_engine

    if name not in _compiled:
        table = oa.OpticalTable()
        table.add_components(COMPONENTS[name](oa))
        _compiled[name] = table.compile()
    eng = get_engine()
    eng.upload(_compiled[name])
    return eng


def _batch(o, d, precision, **kw):
    from optable_amd.batch import RayBatch

    kw.setdefault("wavelength", scenes.WL)
    kw.setdefault("q", Q)
    return RayBatch.from_arrays(o, d, precision=precision, device="cuda", **kw)


def _new_out(n, K, precision, layout, poison=True):
    """a fresh output; tiles: every byte of the block, padding included, poisoned (a write torch sees: there is no token yet)"""
    from optable_amd.batch import SegmentBatch

    out = SegmentBatch(n * K, precision, "cuda", tiled=(layout == "tiled"))
    if poison:
        if out.tiled:
            out.block.fill_(POISON_BYTE)
        else:
            for f in ALL_FIELDS:
                out.field(f).view(torch.uint8).fill_(POISON_BYTE)
    return out


def _bits(t):
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _byte_poison(plane):
    return _bits(torch.full((plane.element_size(),), POISON_BYTE, dtype=torch.uint8, device=plane.device).view(plane.dtype))


def _planes(segs, n, K):
    """every field as bit patterns [K, n], `count`, and which slots hold records"""
    s = segs.to_slots()
    out = {f: _bits(s.field(f)[: K * n]).view(K, n).clone() for f in ALL_FIELDS}
    count = segs.count.clone()
    return out, count, torch.arange(K, device=count.device)[:, None] < count.abs()[None, :]


def _same_records(got, want, what):
    (g, gc, valid), (w, wc, wvalid) = got, want
    assert torch.equal(gc, wc) and torch.equal(valid, wvalid), (what, "count")
    for f in ALL_FIELDS:
        assert torch.equal(g[f][valid], w[f][valid]), (what, f)


def _untouched_beyond_the_counts(out, n, K, what):
    """a tiled output poisoned byte by byte before its first trace: slots k >= |count| and the padding behind slot n * K hold the poison"""
    assert out.tiled
    valid = (torch.arange(K, device="cuda")[:, None] < out.count.abs()[None, :]).reshape(-1)
    for f in ALL_FIELDS:
        flat = _bits(out.field(f).reshape(-1))
        poison = _byte_poison(flat)
        assert out.capacity % 64 == 0 and flat.numel() == out.capacity
        assert bool((flat[: K * n][~valid] == poison).all()), (what, f, "a slot past a ray's count was written")
        assert bool((flat[K * n:] == poison).all()), (what, f, "the last tile's padding was written")


def _short(n):
    """cfg 2's rays with those of wave 0 and every other ray of wave 1 aimed past the lens: they miss everything (1 segment) or meet
    the roof mirrors alone (2 or 3).  Wave 0 is a whole wave of short rays, wave 1 a mixed one, the rest goes the whole path."""
    o, d = scenes.cfg2_rays(n, 0)
    idx = np.concatenate([np.arange(0, 64), np.arange(64, 128, 2)])
    idx = idx[idx < n]
    tan = np.linspace(0.21, 0.6, idx.size)  # past the lens's rim (radius 1 at x = 5) from tan = 0.2 on
    d[idx] = np.stack([np.ones(idx.size), tan, np.zeros(idx.size)], axis=1)
    d[idx[::4]] = [0.0, 1.0, 0.0]  # and straight up: nothing there
    return o, d, idx


def _with_pair_option(eng, value, fn):
    eng.set_option(abi.OPT_PAIR_STORES, value)
    try:
        return fn()
    finally:
        eng.set_option(abi.OPT_PAIR_STORES, 1)


@pytest.mark.parametrize("precision, sizes", [("f64", (2, 64, 129, 130)), ("f32", (130,))])
def test_tiles_equal_slots_bit_for_bit(precision, sizes):
    eng = _engine("cfg2")
    for n in sizes:
        batch = _batch(*scenes.cfg2_rays(n, 0), precision)
        for K in (5, 7):  # 7: every ray leaves two slots unused
            want = _planes(_with_pair_option(eng, 1, lambda: eng.trace(batch, K, out=_new_out(n, K, precision, "slots"), layout="slots")), n, K)
            assert int(want[1].min()) == 5 and eng.last_launch()["kernel"] == 1
            blocks = []
            for option in (0, 1):
                out = _with_pair_option(eng, option, lambda: eng.trace(batch, K, out=_new_out(n, K, precision, "tiled"), layout="tiled"))
                _same_records(_planes(out, n, K), want, (n, K, "OT_OPT_PAIR_STORES", option))
                _untouched_beyond_the_counts(out, n, K, (n, K, option))
                blocks.append(out.block.clone())
            assert torch.equal(blocks[0], blocks[1]), (n, K, "the option changes the tiles")


def test_nothing_beyond_a_rays_count_is_written():
    """Rays of mixed lifetimes inside one wave: the whole path, past the lens (one to three records) and dead on arrival."""
    eng = _engine("cfg2")
    n, precision = 130, "f64"
    o, d, idx = _short(n)
    mixed = np.arange(64, 128, 2)  # the short rays of the mixed wave over the whole range past the rim: roof mirrors alone, or nothing
    d[mixed] = np.stack([np.ones(mixed.size), np.linspace(0.21, 0.6, mixed.size), np.zeros(mixed.size)], axis=1)
    batch = _batch(o, d, precision)
    flags = batch.flags.cpu()
    dead = np.arange(65, 128, 5)  # odd and even lanes of the mixed wave, short and long rays among them
    flags[dead] |= abi.RAY_DEAD
    batch.flags.copy_(flags)
    for K in (5, 7):
        want = _planes(eng.trace(batch, K, out=_new_out(n, K, precision, "slots"), layout="slots"), n, K)
        c = want[1].abs().cpu().numpy()
        assert (c[dead] == 1).all() and (c[:64] <= 3).all() and (c[128:] == 5).all()
        print("segments per ray in the mixed wave:", np.bincount(c[64:128], minlength=K + 1).tolist())
        assert {1, 5} <= set(c[64:128].tolist()) and (c[mixed] <= 3).all(), np.bincount(c[64:128]).tolist()  # one wave: one record, the whole path
        out = eng.trace(batch, K, out=_new_out(n, K, precision, "tiled"), layout="tiled")
        _same_records(_planes(out, n, K), want, (K, "mixed lifetimes"))
        assert bool((want[0]["surface"][0][torch.as_tensor(dead, device="cuda")] == -2).all())
        _untouched_beyond_the_counts(out, n, K, (K, "mixed lifetimes"))


def _poison_behind_torch(out, fields):
    """through .data: torch does not see the write, the tokens stay"""
    for f in fields:
        out.field(f).data.fill_(POISON_INT if f in ("ray", "surface") else POISON_REAL)


def _value_poison(plane, f):
    dt = torch.int32 if f in ("ray", "surface") else {torch.int64: torch.float64, torch.int32: torch.float32}[plane.dtype]
    return _bits(torch.full((1,), POISON_INT if dt == torch.int32 else POISON_REAL, dtype=dt, device=plane.device))


def test_reuse_second_and_third_trace():
    eng = _engine("cfg2")
    n, K, precision = 130, 5, "f64"
    first, again = _batch(*scenes.cfg2_rays(n, 0), precision), _batch(*scenes.cfg2_rays(n, 1), precision)
    want = _planes(eng.trace(again, K, out=_new_out(n, K, precision, "tiled"), layout="tiled"), n, K)
    _same_records(want, _planes(eng.trace(again, K, layout="slots"), n, K), "fresh tiles against slots")
    out = eng.trace(first, K, out=_new_out(n, K, precision, "tiled"), layout="tiled")
    assert out._resident["planes"] == abi.RESIDENT_RAY | abi.RESIDENT_N | abi.RESIDENT_INTENSITY
    assert set(out._first["values"]) == set(POINT + ("n", "intensity"))
    for turn in ("second", "third"):
        assert eng.trace(again, K, out=out, layout="tiled") is out
        _same_records(_planes(out, n, K), want, turn)
        _untouched_beyond_the_counts(out, n, K, turn)
    # both masks ran: poison survives in the resident planes at every k, in the first-segment fields at k = 0, and nowhere else
    _poison_behind_torch(out, ALL_FIELDS)
    eng.trace(again, K, out=out, layout="tiled")
    g, gc, valid = _planes(out, n, K)
    assert torch.equal(gc, want[1])
    for f in ALL_FIELDS:
        poison = _value_poison(g[f], f)
        if f in RESIDENT:
            assert bool((g[f] == poison).all()), (f, "resident plane")
            continue
        assert torch.equal(g[f][1:], want[0][f][1:]), (f, "k >= 1")
        if f in POINT:
            assert bool((g[f][0] == poison).all()), (f, "slot 0 was written")
        else:
            assert torch.equal(g[f][0], want[0][f][0]), (f, "slot 0")


def test_reuse_a_ray_that_lives_longer_makes_its_wave_write_whole_records():
    eng = _engine("cfg2")
    n, K, precision = 130, 5, "f64"
    o, d, idx = _short(n)
    short, long_ = _batch(o, d, precision), _batch(*scenes.cfg2_rays(n, 0), precision)
    want, wc, _ = _planes(eng.trace(long_, K, layout="slots"), n, K)
    assert int(wc.min()) == K
    out = eng.trace(short, K, out=_new_out(n, K, precision, "tiled"), layout="tiled")
    old = out.count.abs().cpu().numpy()
    assert old[:64].max() <= 3 and old[:64].min() == 1 and (old[64:128] < K).any() and (old[64:128] == K).any() and (old[128:] == K).all()
    _poison_behind_torch(out, ALL_FIELDS)
    eng.trace(long_, K, out=out, layout="tiled")
    g, gc, _ = _planes(out, n, K)
    assert torch.equal(gc, wc)
    for lo, hi in ((0, 64), (64, 128), (128, n)):
        whole_from = int(old[lo:hi].min())  # the first segment at which a ray of this wave is past its old count
        whole_from = K if whole_from >= K else whole_from
        for f in ALL_FIELDS:
            poison = _value_poison(g[f], f)
            assert torch.equal(g[f][whole_from:, lo:hi], want[f][whole_from:, lo:hi]), (lo, f, "full records once a ray lives longer")
            for k in range(whole_from):
                kept = f in RESIDENT or (k == 0 and f in POINT)
                if kept:
                    assert bool((g[f][k, lo:hi] == poison).all()), (lo, f, k, "a plane the wave may skip was written")
                else:
                    assert torch.equal(g[f][k, lo:hi], want[f][k, lo:hi]), (lo, f, k)
    # and without poison: the records of a fresh output, there and back
    out = eng.trace(short, K, out=_new_out(n, K, precision, "tiled"), layout="tiled")
    short_want = _planes(out, n, K)
    short_want = ({f: v.clone() for f, v in short_want[0].items()}, short_want[1].clone(), short_want[2])
    eng.trace(long_, K, out=out, layout="tiled")
    _same_records(_planes(out, n, K), (want, wc, torch.ones(K, n, dtype=torch.bool, device="cuda")), "long after short")
    eng.trace(short, K, out=out, layout="tiled")
    _same_records(_planes(out, n, K), short_want, "short after long")


def test_a_refracting_scene_fresh_and_reused():
    """the cfg 4 components (an N-BK7 slab: preset FB, the kernel that is not built for four waves per SIMD in double precision)"""
    eng = _engine("snell")
    K, precision = 3, "f64"
    o, d, wl = scenes.cfg4_rays(65, 4, n_wavelengths=2)
    n = len(o)
    assert n == 130
    batch = _batch(o, d, precision, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl)
    want = _planes(eng.trace(batch, K, out=_new_out(n, K, precision, "slots"), layout="slots"), n, K)
    assert int(want[1].abs().min()) >= 2 and eng.last_launch()["kernel"] == 1
    out = eng.trace(batch, K, out=_new_out(n, K, precision, "tiled"), layout="tiled")
    _same_records(_planes(out, n, K), want, "fresh")
    _untouched_beyond_the_counts(out, n, K, "fresh")
    assert out._resident["planes"] == abi.RESIDENT_RAY  # n changes on the way
    for turn in ("second", "third"):
        eng.trace(batch, K, out=out, layout="tiled")
        _same_records(_planes(out, n, K), want, turn)
    _poison_behind_torch(out, ("ray", "n", "length", "surface"))
    eng.trace(batch, K, out=out, layout="tiled")
    g, _, valid = _planes(out, n, K)
    assert bool((g["ray"] == _value_poison(g["ray"], "ray")).all())
    for f in ("n", "length", "surface"):
        assert torch.equal(g[f][1:][valid[1:]], want[0][f][1:][valid[1:]]), f
    for f in ("length", "surface"):
        assert torch.equal(g[f][0], want[0][f][0]), f


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_stream_ceiling_writes_whole_tiles_and_honours_the_hint(precision):
    eng = _engine("cfg2")
    n, K = 130, 5
    rng = np.random.default_rng(7)
    o = np.zeros((n, 3))
    d = np.tile([1.0, 0.0, 0.0], (n, 1)) + rng.uniform(-0.03, 0.03, (n, 3))
    batch = _batch(o, d, precision)
    BIT = abi.UNIFORM_BIT
    scalars = BIT["wavelength"] | BIT["q_re"] | BIT["q_im"] | BIT["intensity"] | BIT["n"] | BIT["pathlength"]
    assert batch.uniform_mask == scalars | BIT["ox"] | BIT["oy"] | BIT["oz"] | BIT["id"] | BIT["flags"]
    got = []
    for layout, option in (("tiled", 1), ("tiled", 0), ("slots", 1)):
        out = _new_out(n, K, precision, layout)
        eng.set_option(abi.OPT_UNIFORM, option)
        try:
            eng.stream_ceiling(batch, K, out)
        finally:
            eng.set_option(abi.OPT_UNIFORM, 1)
        out.n_rays = n
        got.append(_planes(out, n, K))
        assert int(got[-1][1].min()) == K == int(got[-1][1].max())
        for f in ALL_FIELDS:  # a whole record in every slot: no field keeps the bytes the output was filled with
            assert not bool((got[-1][0][f] == _byte_poison(got[-1][0][f])).any()), (layout, option, f)
        if layout == "tiled":
            _untouched_beyond_the_counts(out, n, K, ("stream ceiling", option))
    _same_records(got[0], got[1], "hint on / off")
    _same_records(got[0], got[2], "tiles / slots")
    # what it writes: the ray handed through K times, ox advanced by one per record, ray = i, surface = id
    ox = got[0][0]["ox"].view(torch.float64 if precision == "f64" else torch.float32)
    assert torch.equal(ox, torch.arange(K, device="cuda", dtype=ox.dtype)[:, None].expand(K, n))
    assert torch.equal(got[0][0]["ray"], torch.arange(n, device="cuda", dtype=torch.int32)[None, :].expand(K, n))
