"""GPU: differential fuzzing — random scenes x random rays, HIP path vs the CPU oracle.
Rays that graze an aperture edge can legitimately fall on different sides in two IEEE implementations
(the oracle polishes roots with Brent, the kernel with Newton; 1/d and x*(1/f) round differently), so
the contract is: at most 0.2 % of the rays may visit a different surface sequence, and every other ray
must agree on every segment to 1e-9 (q: 1e-6, looser only because of the asphere finite differences).  Every ray
that does take another sequence must be explained (optable_amd.fp32_audit.audit_traces): the two traces agree up
to where they part, and the decision there is marginal in the fp64 trace."""
import numpy as np
import pytest

import scenes
from optable_amd import abi
from optable_amd.fp32_audit import assert_explained, audit_traces

pytestmark = pytest.mark.gpu


def random_scene(oa, rng):
    comps = []
    n = int(rng.integers(4, 11))
    for _ in range(n):
        pos = [rng.uniform(2, 26), rng.uniform(-4, 4), rng.uniform(-0.5, 0.5)]
        ang = rng.uniform(-np.pi, np.pi)
        kind = int(rng.integers(0, 11))
        if kind == 0:
            c = oa.Mirror(pos, radius=rng.uniform(0.5, 1.5)).RotZ(ang)
        elif kind == 1:
            c = oa.Lens(pos, focal_length=rng.uniform(3, 12) * rng.choice([-1, 1]), radius=rng.uniform(0.6, 1.4)).RotZ(0.3 * ang)
        elif kind == 2:
            c = oa.GlassSlab(pos, width=2, height=2, thickness=rng.uniform(0.2, 0.8), n1=1, n2=rng.uniform(1.3, 1.8)).RotZ(0.4 * ang)
        elif kind == 3:
            c = oa.Prism(pos, width=1.5, height=2, n1=1, n2=1.5).RotZ(ang)
        elif kind == 4:
            c = oa.BiConvexLens(pos, CT=0.5, R1=rng.uniform(6, 15), R2=-rng.uniform(6, 15), diameter=2.4, n=1.52).RotZ(0.2 * ang)
        elif kind == 5:
            c = oa.SquareMirror(pos, width=1.6, height=1.2).RotZ(ang).RotY(rng.uniform(-0.2, 0.2))
        elif kind == 6:
            c = oa.Block(pos, width=1.0, height=1.0).RotZ(ang)
        elif kind == 7:
            c = oa.CylMirror(pos, radius=1.2, height=2.0, theta_range=(np.pi / 2, np.pi)).RotZ(ang)
        elif kind == 8:
            c = oa.ASphericParametricLens(pos, CT=0.6, diameter=2.4, n=1.5, R=rng.uniform(5, 12), kappa=-1, a4=1e-4).RotZ(0.15 * ang)
        elif kind == 9:
            c = oa.TriangularPrism(pos, width=1.5, height=2, n1=1, n2=1.5, max_interact_count_2=None, max_interact_count_3=None).RotZ(ang)
        else:
            c = oa.CircleGlassSlab(pos, radius=1.0, thickness=0.3, n1=1.0, n2=1.6).RotZ(0.3 * ang)
        comps.append(c)
    return comps


@pytest.mark.parametrize("seed", range(12))
def test_random_scene_matches_oracle(seed, oracle):
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    rng = np.random.default_rng(1000 + seed)
    table = oa.OpticalTable()
    table.add_components(random_scene(oa, rng))
    scene = table.compile()
    assert scene.max_children <= 1
    n, K = 3000, 12
    o = np.stack([np.zeros(n), rng.uniform(-4, 4, n), rng.uniform(-0.4, 0.4, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.15, 0.15, n), rng.uniform(-0.03, 0.03, n)], 1)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=1j * np.pi * scenes.W0**2 / scenes.WL)
    got = table.trace_batch(batch, max_segments=K, layout="slots").to_host(reference_order=True)
    host = batch.to_host()
    ref = oracle.trace(scene, host, max_trace_num=K)
    assert_explained(audit_traces(scene, ref, got, prec="f64", tol=1e-9, rays=host))
    # per-ray surface sequences
    def sequences(x):
        seq = [[] for _ in range(n)]
        for r, s in zip(x["ray"], x["surface"]):
            seq[r].append(int(s))
        return seq
    a, b = sequences(got), sequences(ref)
    same = np.array([x == y for x, y in zip(a, b)])
    assert (~same).mean() <= 0.002, f"{(~same).sum()} of {n} rays took a different path"
    keep_g, keep_r = same[got["ray"]], same[ref["ray"]]
    has_asphere = bool(np.any(np.isin(scene.node_table()["shape"], [5, 6])))
    for f in abi.SEG_FIELDS:
        x, y = got[f][keep_g], ref[f][keep_r]
        if f in ("q_re", "q_im"):
            np.testing.assert_allclose(x, y, rtol=2e-3 if has_asphere else 1e-6, atol=1e-6, err_msg=f)
        else:
            np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-9, err_msg=f)


def random_branching_scene(oa, rng):
    comps = random_scene(oa, rng)
    for _ in range(int(rng.integers(1, 4))):
        pos = [rng.uniform(2, 20), rng.uniform(-3, 3), 0.0]
        pick = int(rng.integers(0, 3))
        if pick == 0:
            comps.append(oa.BeamSplitter(pos, width=2, height=2, eta=rng.uniform(0.2, 0.8)).RotZ(rng.uniform(-1, 1)))
        elif pick == 1:
            comps.append(oa.GlassSlab(pos, width=2, height=2, thickness=0.4, n1=1, n2=1.5, reflectivity=0.15).RotZ(rng.uniform(-0.5, 0.5)))
        else:
            comps.append(oa.Mirror(pos, radius=1.2, reflectivity=0.6, transmission=0.4).RotZ(rng.uniform(-1, 1)))
    return comps


@pytest.mark.parametrize("seed", range(8))
def test_random_branching_scene_matches_oracle(seed, oracle):
    """Same, for ray TREES: generation-by-generation kernels, FIFO order, per-tree max_trace_num budget."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    rng = np.random.default_rng(2000 + seed)
    table = oa.OpticalTable()
    table.add_components(random_branching_scene(oa, rng))
    scene = table.compile()
    assert scene.max_children == 2
    n, cap = 1500, 14
    o = np.stack([np.zeros(n), rng.uniform(-3, 3, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.12, 0.12, n), rng.uniform(-0.02, 0.02, n)], 1)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=1j * np.pi * scenes.W0**2 / scenes.WL)
    segs = table.trace_batch(batch, max_segments=cap, layout="slots")
    got = segs.to_host(reference_order=True)
    host = batch.to_host()
    ref = oracle.trace(scene, host, max_trace_num=cap)
    assert_explained(audit_traces(scene, ref, got, prec="f64", tol=1e-9, rays=host))

    def per_tree(x):
        seq = [[] for _ in range(n)]
        for r, s in zip(x["ray"], x["surface"]):
            seq[r].append(int(s))
        return seq
    a, b = per_tree(got), per_tree(ref)
    same = np.array([x == y for x, y in zip(a, b)])
    assert (~same).mean() <= 0.002, f"{(~same).sum()} of {n} trees differ"
    keep_g, keep_r = same[got["ray"]], same[ref["ray"]]
    has_asphere = bool(np.any(np.isin(scene.node_table()["shape"], [5, 6])))
    for f in abi.SEG_FIELDS:
        x, y = got[f][keep_g], ref[f][keep_r]
        tol = (2e-3 if has_asphere else 1e-6) if f in ("q_re", "q_im") else 1e-9
        np.testing.assert_allclose(x, y, rtol=tol, atol=max(tol, 1e-9), err_msg=f)
    if hasattr(segs, "capped"):
        np.testing.assert_array_equal(segs.capped.cpu().numpy()[same], ref["capped"].astype(bool)[same])


def random_large_scene(oa, rng):
    """14-36 top-level components (=> top-level grid), lens / mirror arrays with >= 24 children
    (=> group grids), dispersive glasses, doublets, wedge plates, mirror cubes."""
    comps = []
    glasses = [oa.Glass_NBK7, oa.Glass_UVFS, oa.Glass_NSF57, oa.Glass_NSK2]
    n = int(rng.integers(14, 37))
    for _ in range(n):
        pos = [rng.uniform(3, 40), rng.uniform(-6, 6), rng.uniform(-0.4, 0.4)]
        ang = rng.uniform(-np.pi, np.pi)
        kind = int(rng.integers(0, 12))
        glass = glasses[int(rng.integers(0, len(glasses)))]()
        if kind == 0:
            c = oa.Mirror(pos, radius=rng.uniform(0.5, 1.3)).RotZ(ang)
        elif kind == 1:
            c = oa.Lens(pos, focal_length=rng.uniform(3, 12), radius=rng.uniform(0.6, 1.2)).RotZ(0.3 * ang)
        elif kind == 2:
            c = oa.GlassSlab(pos, width=2, height=2, thickness=rng.uniform(0.2, 0.8), n1=oa.Vacuum(), n2=glass).RotZ(0.4 * ang)
        elif kind == 3:
            c = oa.Prism(pos, width=1.5, height=2, n1=1, n2=glass).RotZ(ang)
        elif kind == 4:
            c = oa.MLA(pos, N=(6, 5), pitch=0.4, focal_length=rng.uniform(2, 6), radius=0.19).RotZ(0.3 * ang)
        elif kind == 5:
            c = oa.MMA(origin=pos, N=(5, 6), pitch=0.4, roc=rng.uniform(15, 40), n=1.5, thickness=0.1,
                       reflectivity=1, transmission=0).RotZ(np.pi + 0.3 * ang)
        elif kind == 6:
            c = oa.DMD(pos, N=(6, 6), pitch=0.3, tilt_angle=rng.uniform(0.1, 0.4)).RotZ(np.pi + 0.3 * ang)
        elif kind == 7:
            c = oa.Doublet(pos, CT1=0.4, CT2=0.25, R1=rng.uniform(6, 12), R2=-rng.uniform(5, 9), R3=-rng.uniform(15, 40),
                           diameter=2.2, n12=oa.Glass_NSK2(), n23=oa.Glass_NSF57()).RotZ(0.15 * ang)
        elif kind == 8:
            c = oa.WedgePlate(pos, width=2, height=2, thickness=0.4, wedge_angle=rng.uniform(0.01, 0.1), n1=1.0, n2=glass).RotZ(0.3 * ang)
        elif kind == 9:
            c = oa.MirrorCube(pos, L=rng.uniform(0.6, 1.2)).RotZ(ang)
        elif kind == 10:
            c = oa.ASphericExactSphericalLens(pos, EFL=rng.uniform(5, 12), CT=0.6, diameter=2.2, n=1.5).RotZ(0.15 * ang)
        else:
            c = oa.SquareMirror(pos, width=1.6, height=1.2).RotZ(ang).RotY(rng.uniform(-0.2, 0.2))
        comps.append(c)
    return comps


def _large_case(oa, seed):
    rng = np.random.default_rng(3000 + seed)
    table = oa.OpticalTable()
    table.add_components(random_large_scene(oa, rng))
    n = 4000
    o = np.stack([np.zeros(n), rng.uniform(-6, 6, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.15, 0.15, n), rng.uniform(-0.03, 0.03, n)], 1)
    wl = rng.uniform(400e-7, 1100e-7, n)
    return table, o, d, wl


def _sequences(x, n):
    seq = [[] for _ in range(n)]
    for r, s in zip(x["ray"], x["surface"]):
        seq[r].append(int(s))
    return seq


@pytest.mark.parametrize("seed", range(8))
def test_random_large_scene_matches_oracle(seed, oracle):
    """Scenes big enough for every acceleration structure (top-level grid, group grids, blocked kernel),
    with Sellmeier glasses and a different wavelength per ray, against the plain oracle (which has none
    of those structures: it tests every component like the reference)."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    table, o, d, wl = _large_case(oa, seed)
    scene = table.compile()
    assert scene.root_grid >= 0
    n, K = len(o), 16
    batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl)
    got = table.trace_batch(batch, max_segments=K, layout="slots").to_host(reference_order=True)
    host = batch.to_host()
    ref = oracle.trace(scene, host, max_trace_num=K)
    assert_explained(audit_traces(scene, ref, got, prec="f64", tol=1e-7, rays=host))
    a, b = _sequences(got, n), _sequences(ref, n)
    same = np.array([x == y for x, y in zip(a, b)])
    assert (~same).mean() <= 0.002, f"{(~same).sum()} of {n} rays took a different path"
    keep_g, keep_r = same[got["ray"]], same[ref["ray"]]
    has_asphere = bool(np.any(np.isin(scene.node_table()["shape"], [5, 6])))
    for f in abi.SEG_FIELDS:
        x, y = got[f][keep_g], ref[f][keep_r]
        # 1e-7: ten times inside the north-star contract (1e-6).  Rounding differences of ~1e-16 per operation
        # grow along 16 bounces through curved glass and corner reflectors (one segment in 16000 reaches 5e-9).
        tol = (2e-3 if has_asphere else 1e-6) if f in ("q_re", "q_im") else 1e-7
        np.testing.assert_allclose(x, y, rtol=tol, atol=tol, err_msg=f)


@pytest.mark.parametrize("seed", range(4))
def test_random_large_scene_fp32_tracks_fp64(seed):
    """fp32 entry point on the same scenes: at least 95 % of the rays visit the same surfaces as fp64, and
    those agree to 2e-3 in position on every segment (chaotic multi-bounce paths amplify the 6e-8 rounding)."""
    import optable_amd as oa
    from optable_amd.batch import RayBatch

    table, o, d, wl = _large_case(oa, seed)
    n, K = len(o), 16
    out = {}
    for prec in ("f64", "f32"):
        batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl, precision=prec)
        out[prec] = table.trace_batch(batch, max_segments=K, layout="slots").to_host(reference_order=True)
    assert_explained(audit_traces(table.compile(), out["f64"], out["f32"], prec="f32", tol=2e-3, rays=batch.to_host()))
    a, b = _sequences(out["f64"], n), _sequences(out["f32"], n)
    same = np.array([x == y for x, y in zip(a, b)])
    assert same.mean() >= 0.95, same.mean()
    k64, k32 = same[out["f64"]["ray"]], same[out["f32"]["ray"]]
    for f in ("ox", "oy", "oz"):
        err = np.abs(out["f64"][f][k64] - out["f32"][f][k32].astype(np.float64))
        assert err.max() < 2e-3, (f, err.max())


def random_planar_scene(oa, rng, irises=False):
    """14-48 planar components, overlapping and tilted out of the plane at random: the scenes the pair-queue kernel is
    launched for (planar leaves directly under a top-level grid).  Circular / rectangular apertures only, or with
    `irises` also absorbing plates with a hole (boolean apertures: the F_POLY preset of the same kernel)."""
    comps = []
    glasses = [oa.Glass_NBK7, oa.Glass_UVFS, oa.Glass_NSF57]
    for _ in range(int(rng.integers(14, 49))):
        pos = [rng.uniform(3, 40), rng.uniform(-6, 6), rng.uniform(-0.4, 0.4)]
        ang = rng.uniform(-np.pi, np.pi)
        kind = int(rng.integers(0, 7 if irises else 5))
        if kind >= 5:
            comps.append(oa.Block(pos, hole=oa.Circle(rng.uniform(0.2, 0.7)) if kind == 5 else oa.Rectangle(rng.uniform(0.3, 1.2), rng.uniform(0.3, 1.0)),
                                  width=rng.uniform(1.5, 2.5), height=2).RotZ(0.4 * ang))
            continue
        glass = glasses[int(rng.integers(0, len(glasses)))]()
        if kind == 0:
            c = oa.Mirror(pos, radius=rng.uniform(0.5, 1.6)).RotZ(ang)
        elif kind == 1:
            c = oa.Lens(pos, focal_length=rng.uniform(3, 12), radius=rng.uniform(0.6, 1.4)).RotZ(0.3 * ang)
        elif kind == 2:
            c = oa.GlassSlab(pos, width=2, height=2, thickness=rng.uniform(0.2, 0.8), n1=oa.Vacuum(), n2=glass).RotZ(0.4 * ang)
        elif kind == 3:
            c = oa.Prism(pos, width=1.5, height=2, n1=1, n2=glass).RotZ(ang)
        else:
            c = oa.SquareMirror(pos, width=rng.uniform(1.0, 2.5), height=1.2).RotZ(ang).RotY(rng.uniform(-0.3, 0.3))
        comps.append(c)
    return comps


@pytest.mark.parametrize("seed", range(8))
def test_random_planar_scene_pair_queue_variants_agree(seed, oracle):
    """The heavy-scene kernel on random planar scenes, in both precisions, in its three forms — every lane walking its own cells, the wave-wide
    pair queue over global records, the pair queue with the records in LDS — and the lane-per-ray kernel: the same bits
    from all four (ragged ray counts, dead rays, finite lengths, dispersive glass, a different wavelength per ray, mirrors
    tilted out of the table plane), and the fp64 trace of the same scene against the oracle."""
    import torch
    import optable_amd as oa
    from optable_amd.batch import RayBatch
    from optable_amd.engine import get_engine

    rng = np.random.default_rng(5000 + seed)
    table = oa.OpticalTable()
    table.add_components(random_planar_scene(oa, rng, irises=seed >= 6))  # the last seeds: boolean apertures as well
    scene = table.compile()
    assert scene.root_grid >= 0
    n, K = 20_000 + 37 * seed, 12
    o = np.stack([np.zeros(n), rng.uniform(-6, 6, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.15, 0.15, n), rng.uniform(-0.03, 0.03, n)], 1)
    wl = rng.uniform(400e-7, 1100e-7, n)
    eng = get_engine()
    for prec in ("f32", "f64"):
        batch = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl, precision=prec)
        batch.flags[::11] |= abi.RAY_DEAD
        length = torch.full((n,), float("inf"), dtype=batch.ox.dtype, device=batch.device)
        length[3::7] = 9.0
        batch.length = length
        outs, shapes = [], []
        try:
            for kern, flat, rec in ((2, 0, 0), (2, 1, 0), (2, 1, 1), (1, 0, 0)):  # the last one: the lane-per-ray kernel
                eng.set_option(abi.OPT_KERNEL, kern)
                eng.set_option(abi.OPT_FLAT_QUEUE, flat)
                eng.set_option(abi.OPT_LDS_RECORDS, rec)
                outs.append(table.trace_batch(batch, max_segments=K, layout="slots"))
                shapes.append(eng.last_launch()["pair_queue"])
        finally:
            eng.set_option(abi.OPT_KERNEL, 0)
            eng.set_option(abi.OPT_FLAT_QUEUE, 1)
            eng.set_option(abi.OPT_LDS_RECORDS, -1)
        # (records in LDS: single precision only, and only when the image leaves room for them)
        assert shapes[:2] == [0, 1] and shapes[2] in ((1, 3) if prec == "f32" else (1,)) and shapes[3] == 0
        valid = outs[0].valid_mask()
        for other in outs[1:]:
            assert torch.equal(outs[0].count, other.count)
            for f in abi.SEG_FIELDS + ("ray", "surface"):
                assert torch.equal(outs[0].field(f)[valid], other.field(f)[valid]), (prec, f)
    # and the scene itself, in double precision, against the oracle
    b64 = RayBatch.from_arrays(o, d, wavelength=wl, q=1j * np.pi * scenes.W0**2 / wl)
    got = table.trace_batch(b64, max_segments=K, layout="slots").to_host(reference_order=True)
    host = b64.to_host()
    ref = oracle.trace(scene, host, max_trace_num=K)
    assert_explained(audit_traces(scene, ref, got, prec="f64", tol=1e-7, rays=host))
    a, b = _sequences(got, n), _sequences(ref, n)
    same = np.array([x == y for x, y in zip(a, b)])
    assert (~same).mean() <= 0.002, f"{(~same).sum()} of {n} rays took a different path"
    keep_g, keep_r = same[got["ray"]], same[ref["ray"]]
    for f in abi.SEG_FIELDS:
        np.testing.assert_allclose(got[f][keep_g], ref[f][keep_r], rtol=1e-7, atol=1e-7, err_msg=f)
