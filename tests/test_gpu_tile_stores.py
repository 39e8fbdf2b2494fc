"""GPU (MI355X): the tiled segment stores of the lane-per-ray kernel (k_trace_fused / k_stream_ceiling with OUT = SegTiles, kernels.h).
A tile is written one element per lane from ONE place in the segment loop, never through the lane pairs of the slot arrays.  The
records must be those of the slot arrays, bit for bit, whatever OT_OPT_PAIR_STORES says; nothing may be written past a ray's count
(unused slots and the last tile's padding keep a poison written beforehand); and a reused output (resident planes, first-segment
fields) holds what a fresh one holds.  n = 130: two full waves and a two-lane one, even (went through the pairs before); 129: odd."""
import numpy as np
import pytest
import torch

import scenes
import support
from optable_amd import abi

pytestmark = pytest.mark.gpu

ALL_FIELDS = abi.SEG_FIELDS + ("ray", "surface")
RESIDENT = ("ray", "n", "intensity")
POINT = ("ox", "oy", "oz", "q_re", "q_im", "pathlength")  # what cfg 2's point source adds to the resident n and intensity at k = 0
COMPONENTS = {"cfg2": scenes.cfg2_components, "snell": scenes.cfg4_components}
def _engine(name):
    return support.engine_for(COMPONENTS[name], (__name__, name))


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
        batch = support.batch(*scenes.cfg2_rays(n, 0), precision)
        for K in (5, 7):  # 7: every ray leaves two slots unused
            want = support.planes(_with_pair_option(eng, 1, lambda: eng.trace(batch, K, out=support.new_out(n, K, precision, "slots", support.POISON_BYTE), layout="slots")), n, K)
            assert int(want[1].min()) == 5 and eng.last_launch()["kernel"] == 1
            blocks = []
            for option in (0, 1):
                out = _with_pair_option(eng, option, lambda: eng.trace(batch, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled"))
                support.same_records(support.planes(out, n, K), want, (n, K, "OT_OPT_PAIR_STORES", option))
                assert out.tiled
                support.untouched_beyond_the_counts(out, n, K, (n, K, option))
                blocks.append(out.block.clone())
            assert torch.equal(blocks[0], blocks[1]), (n, K, "the option changes the tiles")


def test_nothing_beyond_a_rays_count_is_written():
    """Rays of mixed lifetimes inside one wave: the whole path, past the lens (one to three records) and dead on arrival."""
    eng = _engine("cfg2")
    n, precision = 130, "f64"
    o, d, idx = support.short_rays(n)
    mixed = np.arange(64, 128, 2)  # the short rays of the mixed wave over the whole range past the rim: roof mirrors alone, or nothing
    d[mixed] = np.stack([np.ones(mixed.size), np.linspace(0.21, 0.6, mixed.size), np.zeros(mixed.size)], axis=1)
    batch = support.batch(o, d, precision)
    flags = batch.flags.cpu()
    dead = np.arange(65, 128, 5)  # odd and even lanes of the mixed wave, short and long rays among them
    flags[dead] |= abi.RAY_DEAD
    batch.flags.copy_(flags)
    for K in (5, 7):
        want = support.planes(eng.trace(batch, K, out=support.new_out(n, K, precision, "slots", support.POISON_BYTE), layout="slots"), n, K)
        c = want[1].abs().cpu().numpy()
        assert (c[dead] == 1).all() and (c[:64] <= 3).all() and (c[128:] == 5).all()
        print("segments per ray in the mixed wave:", np.bincount(c[64:128], minlength=K + 1).tolist())
        assert {1, 5} <= set(c[64:128].tolist()) and (c[mixed] <= 3).all(), np.bincount(c[64:128]).tolist()  # one wave: one record, the whole path
        out = eng.trace(batch, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled")
        support.same_records(support.planes(out, n, K), want, (K, "mixed lifetimes"))
        assert bool((want[0]["surface"][0][torch.as_tensor(dead, device="cuda")] == -2).all())
        assert out.tiled
        support.untouched_beyond_the_counts(out, n, K, (K, "mixed lifetimes"))


def test_reuse_second_and_third_trace():
    eng = _engine("cfg2")
    n, K, precision = 130, 5, "f64"
    first, again = support.batch(*scenes.cfg2_rays(n, 0), precision), support.batch(*scenes.cfg2_rays(n, 1), precision)
    want = support.planes(eng.trace(again, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled"), n, K)
    support.same_records(want, support.planes(eng.trace(again, K, layout="slots"), n, K), "fresh tiles against slots")
    out = eng.trace(first, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled")
    assert out._resident["planes"] == abi.RESIDENT_RAY | abi.RESIDENT_N | abi.RESIDENT_INTENSITY
    assert set(out._first["values"]) == set(POINT + ("n", "intensity"))
    for turn in ("second", "third"):
        assert eng.trace(again, K, out=out, layout="tiled") is out
        support.same_records(support.planes(out, n, K), want, turn)
        assert out.tiled
        support.untouched_beyond_the_counts(out, n, K, turn)
    # both masks ran: poison survives in the resident planes at every k, in the first-segment fields at k = 0, and nowhere else
    support.poison_behind_torch(out, ALL_FIELDS)
    eng.trace(again, K, out=out, layout="tiled")
    g, gc, valid = support.planes(out, n, K)
    assert torch.equal(gc, want[1])
    for f in ALL_FIELDS:
        poison = support.value_poison(g[f], f)
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
    o, d, idx = support.short_rays(n)
    short, long_ = support.batch(o, d, precision), support.batch(*scenes.cfg2_rays(n, 0), precision)
    want, wc, _ = support.planes(eng.trace(long_, K, layout="slots"), n, K)
    assert int(wc.min()) == K
    out = eng.trace(short, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled")
    old = out.count.abs().cpu().numpy()
    assert old[:64].max() <= 3 and old[:64].min() == 1 and (old[64:128] < K).any() and (old[64:128] == K).any() and (old[128:] == K).all()
    support.poison_behind_torch(out, ALL_FIELDS)
    eng.trace(long_, K, out=out, layout="tiled")
    g, gc, _ = support.planes(out, n, K)
    assert torch.equal(gc, wc)
    for lo, hi in ((0, 64), (64, 128), (128, n)):
        whole_from = int(old[lo:hi].min())  # the first segment at which a ray of this wave is past its old count
        whole_from = K if whole_from >= K else whole_from
        for f in ALL_FIELDS:
            poison = support.value_poison(g[f], f)
            assert torch.equal(g[f][whole_from:, lo:hi], want[f][whole_from:, lo:hi]), (lo, f, "full records once a ray lives longer")
            for k in range(whole_from):
                kept = f in RESIDENT or (k == 0 and f in POINT)
                if kept:
                    assert bool((g[f][k, lo:hi] == poison).all()), (lo, f, k, "a plane the wave may skip was written")
                else:
                    assert torch.equal(g[f][k, lo:hi], want[f][k, lo:hi]), (lo, f, k)
    # and without poison: the records of a fresh output, there and back
    out = eng.trace(short, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled")
    short_want = support.planes(out, n, K)
    short_want = ({f: v.clone() for f, v in short_want[0].items()}, short_want[1].clone(), short_want[2])
    eng.trace(long_, K, out=out, layout="tiled")
    support.same_records(support.planes(out, n, K), (want, wc, torch.ones(K, n, dtype=torch.bool, device="cuda")), "long after short")
    eng.trace(short, K, out=out, layout="tiled")
    support.same_records(support.planes(out, n, K), short_want, "short after long")


def test_a_refracting_scene_fresh_and_reused():
    """the cfg 4 components (an N-BK7 slab: preset FB, the kernel that is not built for four waves per SIMD in double precision)"""
    eng = _engine("snell")
    K, precision = 3, "f64"
    o, d, wl = scenes.cfg4_rays(65, 4, n_wavelengths=2)
    n = len(o)
    assert n == 130
    batch = support.batch(o, d, precision, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl)
    want = support.planes(eng.trace(batch, K, out=support.new_out(n, K, precision, "slots", support.POISON_BYTE), layout="slots"), n, K)
    assert int(want[1].abs().min()) >= 2 and eng.last_launch()["kernel"] == 1
    out = eng.trace(batch, K, out=support.new_out(n, K, precision, "tiled", support.POISON_BYTE), layout="tiled")
    support.same_records(support.planes(out, n, K), want, "fresh")
    assert out.tiled
    support.untouched_beyond_the_counts(out, n, K, "fresh")
    assert out._resident["planes"] == abi.RESIDENT_RAY  # n changes on the way
    for turn in ("second", "third"):
        eng.trace(batch, K, out=out, layout="tiled")
        support.same_records(support.planes(out, n, K), want, turn)
    support.poison_behind_torch(out, ("ray", "n", "length", "surface"))
    eng.trace(batch, K, out=out, layout="tiled")
    g, _, valid = support.planes(out, n, K)
    assert bool((g["ray"] == support.value_poison(g["ray"], "ray")).all())
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
    batch = support.batch(o, d, precision)
    BIT = abi.UNIFORM_BIT
    scalars = BIT["wavelength"] | BIT["q_re"] | BIT["q_im"] | BIT["intensity"] | BIT["n"] | BIT["pathlength"]
    assert batch.uniform_mask == scalars | BIT["ox"] | BIT["oy"] | BIT["oz"] | BIT["id"] | BIT["flags"]
    got = []
    for layout, option in (("tiled", 1), ("tiled", 0), ("slots", 1)):
        out = support.new_out(n, K, precision, layout, support.POISON_BYTE)
        eng.set_option(abi.OPT_UNIFORM, option)
        try:
            eng.stream_ceiling(batch, K, out)
        finally:
            eng.set_option(abi.OPT_UNIFORM, 1)
        out.n_rays = n
        got.append(support.planes(out, n, K))
        assert int(got[-1][1].min()) == K == int(got[-1][1].max())
        for f in ALL_FIELDS:  # a whole record in every slot: no field keeps the bytes the output was filled with
            assert not bool((got[-1][0][f] == support.byte_poison(got[-1][0][f])).any()), (layout, option, f)
        if layout == "tiled":
            assert out.tiled
            support.untouched_beyond_the_counts(out, n, K, ("stream ceiling", option))
    support.same_records(got[0], got[1], "hint on / off")
    support.same_records(got[0], got[2], "tiles / slots")
    # what it writes: the ray handed through K times, ox advanced by one per record, ray = i, surface = id
    ox = got[0][0]["ox"].view(torch.float64 if precision == "f64" else torch.float32)
    assert torch.equal(ox, torch.arange(K, device="cuda", dtype=ox.dtype)[:, None].expand(K, n))
    assert torch.equal(got[0][0]["ray"], torch.arange(n, device="cuda", dtype=torch.int32)[None, :].expand(K, n))
