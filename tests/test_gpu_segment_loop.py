"""GPU (MI355X): the segment loop of the lane-per-ray kernel (kernels.h k_trace_fused).  Its counter is a scalar the slot base, the
first-segment mask and the ray's count are all derived from, and a hit advances the ray in place (trace_core.h advance): a lane whose
ray ended keeps whatever the interaction left in its registers, which must never be stored or traced.  The yardsticks are code that
has neither: the rolling-lists kernel on the same batch (OT_OPT_KERNEL = 2, slot layout), records and counts bit for bit, and, where
a case is about reuse, a trace into a fresh output.  n = 129 and 130: two full waves plus one and two lanes."""
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


def _components(name, oa):
    if name == "cfg2":
        return scenes.cfg2_components(oa)
    if name == "ends":  # cfg 2 and an absorbing plate above the cone of its source, for rays aimed at it
        return scenes.cfg2_components(oa) + [oa.Block([2.0, 1.5, 0.0], width=0.4, height=0.4)]
    if name == "split":  # half-silvered mirrors: one the source aims at directly (k = 0), one on the axis behind the lens (k = 1)
        return [oa.Lens([5, 0, 0], focal_length=5, radius=1.0), oa.Mirror([2.0, 1.5, 0.0], radius=0.2, reflectivity=0.5, transmission=0.5),
                oa.Mirror([8, 0, 0], radius=0.3, reflectivity=0.5, transmission=0.5), oa.MirrorPair([10, 0, 0], 4, 4)]
    if name == "snell":
        return scenes.cfg4_components(oa)
    if name == "sphere":  # spherical faces (preset FE) and a mirror that sends the rays back through them
        return [oa.BiConvexLens([5, 0, 0], CT=0.6, R1=20.0, R2=-20.0, diameter=5.08, EFL=20.0), oa.Mirror([10, 0, 0], radius=3.0)]
    raise KeyError(name)


def _engine(name):
    return support.engine_for(lambda oa: _components(name, oa), (__name__, name))


def _forced(eng, kernel, fn):
    eng.set_option(abi.OPT_KERNEL, kernel)
    try:
        out = fn()
        assert eng.last_launch()["kernel"] == kernel, eng.last_launch()
        return out
    finally:
        eng.set_option(abi.OPT_KERNEL, 0)


def _rolling(eng, batch, K, precision="f64"):
    """THE yardstick: the rolling-lists kernel, [k][ray] slots, into a fresh output"""
    n = batch.n
    return support.planes(_forced(eng, 2, lambda: eng.trace(batch, K, out=support.new_out(n, K, precision, "slots", support.POISON_BYTE), layout="slots")), n, K)


def _fused(eng, batch, K, layout, precision="f64", out=None):
    n = batch.n
    out = support.new_out(n, K, precision, layout, support.POISON_BYTE) if out is None else out
    return _forced(eng, 1, lambda: eng.trace(batch, K, out=out, layout=layout))


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tiled", "slots"])
@pytest.mark.parametrize("n", [129, 130])
def test_cfg2_every_cap_equals_the_rolling_lists(n, layout):
    """K = 1, 2, 5; 7 exceeds every ray's life: the loop ends because no lane of the wave is active"""
    eng = _engine("cfg2")
    batch = support.batch(*scenes.cfg2_rays(n, 0))
    for K in (1, 2, 5, 7):
        want = _rolling(eng, batch, K)
        assert int(want[1].min()) == int(want[1].max()) == min(K, 5)
        out = _fused(eng, batch, K, layout)
        support.same_records(support.planes(out, n, K), want, (n, K, layout))
        support.untouched_beyond_the_counts(out, n, K, (n, K, layout))


@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_cfg2_single_precision(layout):
    eng = _engine("cfg2")
    n, K = 130, 5
    batch = support.batch(*scenes.cfg2_rays(n, 0), "f32")
    out = _fused(eng, batch, K, layout, "f32")
    support.same_records(support.planes(out, n, K), _rolling(eng, batch, K, "f32"), layout)
    support.untouched_beyond_the_counts(out, n, K, layout)


def _aimed(n, idx, target):
    """cfg 2's rays, those at `idx` aimed from the source at `target`"""
    o, d = scenes.cfg2_rays(n, 0)
    t = np.asarray(target, dtype=float)
    d[idx] = t / np.linalg.norm(t)
    return o, d


def _every_end(n):
    """Wave 1 (rays 64..127) mixes every way a ray ends: past the lens's rim, where a ray meets nothing or the roof mirrors alone
    (escapes at k = 0, 1 or 2); aimed at the absorbing plate (no outgoing ray); dead on arrival; and the whole path (the cap)."""
    o, d = scenes.cfg2_rays(n, 0)
    rim = np.arange(64, 128, 2)
    d[rim] = np.stack([np.ones(rim.size), np.linspace(0.21, 0.6, rim.size), np.zeros(rim.size)], axis=1)
    up = np.array([66, 90, 114])
    d[up] = [0.0, 1.0, 0.0]  # nothing there
    plate = np.array([67, 71, 99, 121])
    d[plate] = np.array([2.0, 1.5, 0.0]) / 2.5
    dead = np.array([65, 70, 101, 127])
    return o, d, rim, up, plate, dead


@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_one_wave_mixing_every_way_a_ray_ends(layout):
    eng = _engine("ends")
    n = 130
    o, d, rim, up, plate, dead = _every_end(n)
    batch = support.batch(o, d)
    flags = batch.flags.cpu()
    flags[dead] |= abi.RAY_DEAD
    batch.flags.copy_(flags)
    for K in (5, 7):
        want = _rolling(eng, batch, K)
        c = want[1].cpu().numpy()
        surface0 = want[0]["surface"][0].cpu().numpy()
        print("segments per ray in the mixed wave:", np.bincount(c[64:128], minlength=K + 1).tolist())
        assert (c >= 1).all(), "no branching hit in this scene"
        assert (c[dead] == 1).all() and (surface0[dead] == -2).all()
        assert (c[up] == 1).all() and (surface0[up] == -1).all()              # escaped at k = 0
        assert (c[plate] == 1).all() and (surface0[plate] >= 0).all()         # absorbed: one record, of a hit
        assert {1, 2, 3, 5} <= set(c[64:128].tolist()), np.bincount(c[64:128]).tolist()  # escapes at k = 0, 1 and 2, and the cap
        assert (c[128:] == 5).all() and (c[:64] == 5).all()
        out = _fused(eng, batch, K, layout)
        support.same_records(support.planes(out, n, K), want, (K, layout))
        support.untouched_beyond_the_counts(out, n, K, (K, layout))


@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_a_half_silvered_mirror_at_the_first_an_inner_and_the_last_segment(layout):
    """count = -(k + 1) where the tree branches, and the records up to there are the rolling lists'"""
    eng = _engine("split")
    n = 130
    first = np.array([3, 64, 77, 126, 129])  # aimed at the half-silvered mirror beside the lens: a branching hit at k = 0
    o, d = _aimed(n, first, [2.0, 1.5, 0.0])
    batch = support.batch(o, d)
    for K, behind_the_lens in ((1, None), (2, "the last segment"), (5, "an inner segment")):
        want = _rolling(eng, batch, K)
        c = want[1].cpu().numpy()
        assert (c[first] == -1).all()
        rest = np.delete(c, first)
        if behind_the_lens is None:
            assert (rest == 1).all()
        else:  # rays near the axis meet the second one at k = 1, the others pass it by and go on
            assert (rest == -2).any() and (rest == K).any() and set(rest.tolist()) <= {-2, K}, np.unique(rest).tolist()
            for lo, hi in ((0, 64), (64, 128)):
                assert (c[lo:hi] == -2).any() and (c[lo:hi] == K).any(), "every full wave mixes the two"
        out = _fused(eng, batch, K, layout)
        support.same_records(support.planes(out, n, K), want, (K, layout, behind_the_lens))
        support.untouched_beyond_the_counts(out, n, K, (K, layout))


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_reuse_second_and_third_trace_equal_a_fresh_output(layout):
    eng = _engine("cfg2")
    n, K = 130, 5
    first, again = support.batch(*scenes.cfg2_rays(n, 0)), support.batch(*scenes.cfg2_rays(n, 1))
    want = support.planes(_fused(eng, again, K, layout), n, K)
    support.same_records(want, _rolling(eng, again, K), "a fresh output against the rolling lists")
    out = _fused(eng, first, K, layout)
    for turn in ("second", "third"):
        assert _fused(eng, again, K, layout, out=out) is out
        support.same_records(support.planes(out, n, K), want, (turn, layout))
        support.untouched_beyond_the_counts(out, n, K, (turn, layout))
    if layout != "tiled":
        return
    # both masks ran (fm at k = 0 and `whole` come from the scalar counter): poison survives in the resident planes at every k,
    # in the first-segment fields at k = 0, and nowhere else
    assert out._resident["planes"] == abi.RESIDENT_RAY | abi.RESIDENT_N | abi.RESIDENT_INTENSITY
    assert set(out._first["values"]) == set(POINT + ("n", "intensity"))
    support.poison_behind_torch(out)
    _fused(eng, again, K, layout, out=out)
    g, gc, _ = support.planes(out, n, K)
    assert torch.equal(gc, want[1])
    for f in ALL_FIELDS:
        poison = support.value_poison(g[f], f)
        if f in RESIDENT:
            assert bool((g[f] == poison).all()), (f, "a resident plane was written")
            continue
        assert torch.equal(g[f][1:], want[0][f][1:]), (f, "k >= 1")
        if f in POINT:
            assert bool((g[f][0] == poison).all()), (f, "slot 0 was written")
        else:
            assert torch.equal(g[f][0], want[0][f][0]), (f, "slot 0")


def test_reuse_a_ray_that_lives_longer_than_last_time():
    """the wave of such a ray writes whole records from the first segment on at which one of its rays is past its old count;
    before that, and in the other waves, the skip runs: poison survives exactly there"""
    eng = _engine("cfg2")
    n, K, layout = 130, 5, "tiled"
    short, long_ = support.batch(*support.short_rays(n)[:2]), support.batch(*scenes.cfg2_rays(n, 0))
    want, wc, wvalid = _rolling(eng, long_, K)
    assert int(wc.min()) == K
    out = _fused(eng, short, K, layout)
    support.same_records(support.planes(out, n, K), _rolling(eng, short, K), "the short rays")
    old = out.count.abs().cpu().numpy()
    assert old[:64].max() <= 3 and old[:64].min() == 1 and (old[64:128] < K).any() and (old[64:128] == K).any() and (old[128:] == K).all()
    support.poison_behind_torch(out)
    _fused(eng, long_, K, layout, out=out)
    g, gc, _ = support.planes(out, n, K)
    assert torch.equal(gc, wc)
    for lo, hi in ((0, 64), (64, 128), (128, n)):
        whole_from = min(int(old[lo:hi].min()), K)
        for f in ALL_FIELDS:
            poison = support.value_poison(g[f], f)
            assert torch.equal(g[f][whole_from:, lo:hi], want[f][whole_from:, lo:hi]), (lo, f, "full records once a ray lives longer")
            for k in range(whole_from):
                if f in RESIDENT or (k == 0 and f in POINT):
                    assert bool((g[f][k, lo:hi] == poison).all()), (lo, f, k, "a plane the wave may skip was written")
                else:
                    assert torch.equal(g[f][k, lo:hi], want[f][k, lo:hi]), (lo, f, k)
    # and without poison, there and back: what a fresh output holds
    out = _fused(eng, short, K, layout)
    _fused(eng, long_, K, layout, out=out)
    support.same_records(support.planes(out, n, K), (want, wc, wvalid), "long after short")
    _fused(eng, short, K, layout, out=out)
    support.same_records(support.planes(out, n, K), _rolling(eng, short, K), "short after long")


# ------------------------------------------------------------------------------------------------------------------------------------
def _snell_rays():
    """cfg 4's rays through the N-BK7 slab (flat interfaces, two wavelengths), some of them started INSIDE the glass at 45 degrees
    to its faces: past the critical angle, they are reflected totally from face to face until they leave by the slab's edge."""
    o, d, wl = scenes.cfg4_rays(65, 4, n_wavelengths=2)
    inside = np.arange(3, len(o), 7)
    o[inside] = [-0.25, -0.9, 0.0]
    d[inside] = [np.sqrt(0.5), np.sqrt(0.5), 0.0]
    return o, d, wl, inside


@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_the_refracting_scene_with_total_internal_reflection_fresh_and_reused(layout):
    eng = _engine("snell")
    o, d, wl, inside = _snell_rays()
    n = len(o)
    assert n == 130
    batch = support.batch(o, d, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl)
    for K in (3, 6):
        want = _rolling(eng, batch, K)
        c = want[1].cpu().numpy()
        print("K", K, "segments per ray:", np.bincount(c, minlength=K + 1).tolist(), "started inside:", sorted(set(c[inside].tolist())))
        assert (c >= 1).all()
        assert (c[inside] == min(K, 5)).all(), "four total reflections (y = -0.65, -0.15, 0.35, 0.85), then out by the edge"
        nn = want[0]["n"].view(torch.float64)
        assert bool((nn[: min(K, 5), inside] == nn[0, inside]).all()), "total internal reflection keeps the ray's n"
        assert int(np.delete(c, inside).min()) >= 2
        out = _fused(eng, batch, K, layout)
        support.same_records(support.planes(out, n, K), want, (K, layout, "fresh"))
        support.untouched_beyond_the_counts(out, n, K, (K, layout, "fresh"))
        for turn in ("second", "third"):
            _fused(eng, batch, K, layout, out=out)
            support.same_records(support.planes(out, n, K), want, (K, layout, turn))
            support.untouched_beyond_the_counts(out, n, K, (K, layout, turn))


@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_a_scene_with_spherical_faces(layout):
    """the preset with curved surfaces and count gates shares the loop"""
    eng = _engine("sphere")
    n, K = 130, 6
    batch = support.batch(*scenes.cfg2_rays(n, 0))
    want = _rolling(eng, batch, K)
    c = want[1].cpu().numpy()
    print("segments per ray:", np.bincount(c, minlength=K + 1).tolist())
    assert (c >= 1).all() and c.max() >= 5, "through both faces, off the mirror and back through both"
    out = _fused(eng, batch, K, layout)
    support.same_records(support.planes(out, n, K), want, layout)
    support.untouched_beyond_the_counts(out, n, K, layout)


@pytest.mark.parametrize("layout", ["tiled", "slots"])
def test_the_grid_stride_path_equals_the_default_grid(layout):
    """One workgroup per CU and more than two grids of rays: every workgroup goes round the outer loop three times, the last time
    for 130 rays in all.  The ray pointers are re-read and the per-ray state re-initialised between iterations."""
    eng = _engine("cfg2")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, K = 2 * cus * 256 + 130, 5
    batch = support.batch(*scenes.cfg2_rays(n, 3))
    want = _fused(eng, batch, K, layout)
    full_grid = eng.last_launch()["workgroups"]
    eng.set_option(abi.OPT_BLOCKS_PER_CU, 1)
    try:
        out = _fused(eng, batch, K, layout)
        launch = eng.last_launch()
    finally:
        eng.set_option(abi.OPT_BLOCKS_PER_CU, 0)
    assert launch["workgroups"] == cus and launch["workgroups"] * 256 * 2 < n <= full_grid * 256, (launch, full_grid)
    assert torch.equal(out.count, want.count) and int(want.count.min()) == K
    for f in ALL_FIELDS:
        assert torch.equal(support.bits(out.field(f).reshape(-1)), support.bits(want.field(f).reshape(-1))), (layout, f)
