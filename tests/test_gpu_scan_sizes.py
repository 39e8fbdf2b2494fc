"""GPU (MI355X): the users of the device-wide exclusive scan (csrc/misc_kernels.h: k_scan_tiles, k_scan_spine, k_scan_apply) at the
sizes where the scan changes shape — more than one tile of 2,048 elements, and a second round of the spine beyond 524,288 — each
against a numpy rule or the C oracle, never against another device path alone:
  * the count-gate ranks of a generation (int32 -> int32): trees whose rays lie on both sides of a wave, workgroup, scan-tile and
    spine-round boundary, with a limited surface hit on both sides (tests/scan_cases.py; tests/test_scan_cases_cpu.py proves it);
  * the one-pass generation kernel's look-back over 8,256 tiles, against the rule of the gate-free twin;
  * Monitor.record's count table (int32 -> int64) of 2,369 elements, of two launches, and of 531,265 elements."""
import ctypes as C

import numpy as np
import pytest
import torch

import optable_amd as oa
import scan_cases as S
import scenes
import support
from optable_amd import abi
from optable_amd.batch import RayBatch, SegmentBatch
from optable_amd.engine import get_engine
from optable_amd.table import monitor_struct

pytestmark = pytest.mark.gpu

_rules = {}


def _rule(name, variant):
    if (name, variant) not in _rules:
        _rules[name, variant] = S.gated_rule(S.gated(name, variant))
    return _rules[name, variant]


def _device(array):
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def _rays(case, precision):
    o, d = S.origins(case)
    return RayBatch.from_arrays(o, d, wavelength=scenes.WL, ids=case.ids, precision=precision)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == np.shape(want) and np.array_equal(got, want), what


def _records_are(segs, rule, what):
    m = len(rule.surface)
    assert segs.n_valid == m, (what, segs.n_valid, m)
    _same(segs.surface[:m], rule.surface, (what, "surface"))
    _same(segs.ray[:m], rule.ray, (what, "ray"))
    _same(segs.length[:m].double(), rule.length, (what, "length"))  # 4, 6, 8 or inf: exact in either precision


def _children_start_where_their_parents_ended(kids, case, rule, what):
    """Every child starts on its parent's hit point — the plane of the parent's surface, the parent's own (y, z) — in parent order."""
    parent = rule.parent
    surface = np.full(case.n, -1)
    surface[rule.processed] = rule.surface
    assert kids.n == len(parent), (what, kids.n, len(parent))
    _same(kids.ox.double(), S.PLANE_X[surface[parent]], (what, "child ox"))
    _same(kids.oy.double(), case.y[parent], (what, "child oy"))
    _same(kids.oz.double(), case.z[parent], (what, "child oz"))


# -- 1: one generation through the gated scene --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name,variant", S.GATED_CASES)
def test_a_gated_generation_is_the_rule(name, variant, precision):
    """Engine.generation_step with the caller's trees: records, children, parent list and the count table are the rule's, whatever
    OT_OPT_GEN_ONEPASS says (a scene with limited surfaces keeps the two passes)."""
    case, rule = S.gated(name, variant), _rule(name, variant)
    eng = support.engine_for(S.gated_components, "scan cases: gated")
    batch, tree, counts0 = _rays(case, precision), _device(case.tree), _device(case.counts0)
    try:
        for onepass in (0, 1, -1):
            eng.set_option(abi.OPT_GEN_ONEPASS, onepass)
            what = (name, variant, precision, onepass)
            segs, kids, parent = eng.generation_step(batch, counts=counts0.clone(), tree=tree)
            assert segs.n_valid == case.n
            _records_are(segs, rule, what)
            _same(parent, rule.parent, (what, "parent"))
            _children_start_where_their_parents_ended(kids, case, rule, what)
            _same(segs.counts_table, rule.counts, (what, "counts"))
    finally:
        eng.set_option(abi.OPT_GEN_ONEPASS, -1)
    assert eng.generation_mismatches() == 0


def test_budgets_and_gates_together():
    """ot_trace_generation_f64 itself, budgets smaller than some trees: the rays beyond a tree's budget leave no record, consume no
    count and emit nothing, a tree that uses its budget up emits nothing, and budget[] is what the header says."""
    case = S.gated("two spine rounds", "behind")
    budget0 = S.budgets(case)
    rule = S.gated_rule(case, budget0)
    assert 0 < len(rule.surface) < case.n and np.any(budget0 < case.sizes) and np.any(budget0 > case.sizes)
    eng = support.engine_for(S.gated_components, "scan cases: gated")
    n = case.n
    rays, tree, counts, budget = _rays(case, "f64"), _device(case.tree), _device(case.counts0), _device(budget0)
    out, nxt = SegmentBatch(n, "f64", "cuda"), RayBatch(n, "f64", "cuda", initialise=False)
    guarded = support.Sentinel(guard=64, next_tree=(torch.int32, (n,)), state=(torch.int64, (2,)))
    guarded.state.zero_()
    rs, ss, ns = rays.c_struct(), out.c_struct(), nxt.c_struct()
    with eng.lock:
        abi.check(eng._fn("ot_trace_generation", "f64")(eng._ctx, C.byref(rs), tree.data_ptr(), n, budget.data_ptr(), C.byref(ss), n,
                                                        guarded.state.data_ptr(), C.byref(ns), guarded.next_tree.data_ptr(), n,
                                                        guarded.state.data_ptr() + 8, counts.data_ptr(), case.n_classes), eng.lib)
    written, n_next = guarded.state.tolist()
    out.n_valid = written
    _records_are(out, rule, "budgets")
    assert n_next == len(rule.parent)
    _same(guarded.next_tree[:n_next], case.tree[rule.parent], "the children's trees")  # (no OT_OPT_GEN_PARENT_INDEX: tree ids)
    assert bool((guarded.next_tree[n_next:] == guarded.fill).all()) and guarded.guards_untouched()
    _children_start_where_their_parents_ended(nxt.slice(0, n_next), case, rule, "budgets")
    _same(budget, rule.budget, "budget")
    _same(counts, rule.counts, "counts")


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("onepass", [1, 0])
def test_the_gate_free_twin_is_the_rule(onepass, precision):
    """528,384 rays with 0, 1 or 2 children each through ot_trace_tree_*, every ray a tree of its own so that a child's tree is its
    parent's index, into segment arrays of exactly one generation: the call comes back after the first one.  With
    OT_OPT_GEN_ONEPASS = 1 that generation is k_gen_one's, its offsets from a look-back over 8,256 tiles; with 0 the two passes'."""
    case = S.gated("two spine rounds", "closed")
    rule = S.twin_rule(case)
    n, total = case.n, int(rule.children.sum())
    rule.ray = np.arange(n, dtype=np.int32)  # (the trees of this call, not the case's)
    assert -(-n // S.WAVE) == 8_256 and sorted(set(rule.children.tolist())) == [0, 1, 2]
    eng = support.engine_for(S.twin_components, "scan cases: twin")
    assert eng.scene.max_children == 2 and not eng.scene.limited
    rays = _rays(case, precision)
    out = SegmentBatch(n, precision, "cuda")
    bufs = [RayBatch(2 * n, precision, "cuda", initialise=False) for _ in range(2)]
    trees = [torch.full((2 * n,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    tree = torch.arange(n, dtype=torch.int32, device="cuda")
    budget = torch.full((n,), 2, dtype=torch.int32, device="cuda")  # the ray itself and room for one more: the children are wanted
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    result = (C.c_int64 * 5)()
    rs, ss, sa, sb = rays.c_struct(), out.c_struct(), bufs[0].c_struct(), bufs[1].c_struct()
    try:
        eng.set_option(abi.OPT_GEN_ONEPASS, onepass)
        with eng.lock:
            abi.check(eng._fn("ot_trace_tree", precision)(eng._ctx, C.byref(rs), tree.data_ptr(), n, budget.data_ptr(), C.byref(ss), n, state.data_ptr(),
                                                          C.byref(sa), trees[0].data_ptr(), C.byref(sb), trees[1].data_ptr(), 2 * n, None, 0, -1.0, result), eng.lib)
    finally:
        eng.set_option(abi.OPT_GEN_ONEPASS, -1)
    written, n_next, where, generations, reason = (int(x) for x in result)
    assert (written, n_next, generations, reason) == (n, total, 1, 1) and where in (1, 2)  # (reason 1: no room for the next generation)
    assert state.tolist() == [n, total]
    out.n_valid = written
    _records_are(out, rule, ("twin", onepass))
    _same(trees[where - 1][:total], rule.parent, "parent")
    assert bool((trees[where - 1][total:] == -7).all()) and bool((trees[2 - where] == -7).all())
    _children_start_where_their_parents_ended(bufs[where - 1].slice(0, total), case, rule, ("twin", onepass))
    _same(budget, np.ones(n, dtype=np.int32), "budget")
    assert eng.generation_mismatches() == 0


# -- 2: a traced scene against the oracle -------------------------------------------------------------------------------------------
def _gated_lattice(k_max=5):
    """support.lattice(5) with two of its beam splitters count-limited."""
    comps = []
    for k in range(k_max):
        comps.append(oa.BeamSplitter([2.0 * (k + 1), 0, 0], width=6, height=2, eta=0.5, max_interact_count=2 if k == 0 else None).RotZ(np.pi / 4))
        comps.append(oa.Mirror([2.0 * (k + 1), 3.0 + 0.1 * k, 0], radius=2).RotZ(-np.pi / 2))
        comps.append(oa.BeamSplitter([2.0 * (k + 1) + 1.0, 1.5, 0], width=6, height=2, eta=0.3, max_interact_count=5 if k == 1 else None).RotZ(-np.pi / 4))
    return support.table_of(comps).compile()


def test_gated_trees_of_a_traced_scene_match_the_oracle(oracle):
    """3,000 bushy trees under a cap of 40 through two count-limited beam splitters: the generation loop (probe, per-surface scans,
    ranks) and the lane-per-tree kernel (a column per tree, FIFO on the chip) against the oracle, records and count table."""
    scene = _gated_lattice()
    assert [c.max_interact_count for c in scene.limited] == [2, 5] and scene.max_children == 2
    n, cap = 3000, 40
    rng = np.random.default_rng(5)
    o = np.stack([np.zeros(n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.01, 0.01, n)], 1)
    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, q=support.Q)
    ref = oracle.trace(scene, batch.to_host(), max_trace_num=cap)
    # at most `cap` generations: more than cap * 2,048 records means a generation of more than 2,048 rays — scan tiles end inside trees
    assert len(ref["ray"]) > cap * S.SCAN_TILE and ref["counts"].shape == (2, n)
    assert ref["counts"].max(1).tolist() == [2, 5]  # gates that close
    eng = get_engine()
    eng.upload(scene)
    assert eng.trees_plan("f64", cap, n)["kernel"] and eng.trees_plan("f64", cap, n)["full"]
    slots = eng.trees_plan("f64", cap, n)["slots"]
    for what, segs in (("generations", eng.trace_tree(batch, cap)), ("lane per tree", eng.trace_trees(batch, cap, layout="slots" if slots else "append"))):
        got = segs.to_host(reference_order=True)
        np.testing.assert_array_equal(got["ray"], ref["ray"], err_msg=what)
        np.testing.assert_array_equal(got["surface"], ref["surface"], err_msg=what)
        for f in abi.SEG_FIELDS:
            np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=1e-9, err_msg=f"{what} {f}")
        _same(segs.counts_table, ref["counts"], (what, "counts"))
    assert eng.generation_mismatches() == 0


# -- 3: Monitor.record ----------------------------------------------------------------------------------------------------------------
def _list_of(case):
    y, z = S.MONITOR_POSITIONS[case.position].T
    return support.list_segments(case.n, oy=y, oz=z, dx=1.0, length=case.k + 0.5, intensity=1.0)


def _holes(case):
    """(segs, valid): ray = -1 on a seeded tenth of the slots of a list that says it has holes"""
    segs = _list_of(case)
    valid = np.random.default_rng(31).random(case.n) >= 0.1
    segs.ray[_device(~valid)] = -1
    segs.append = True
    return segs, valid


def _slots(case, n_rays=3000):
    """(segs, valid): the slots as [k][ray] planes of 3,000 rays whose seg_count leaves a seeded tenth of the rays no slot, cuts some
    rays short and says of some, by its sign, that their tree branched"""
    segs = _list_of(case)
    K = case.n // n_rays
    assert K * n_rays == case.n
    rng = np.random.default_rng(32)
    count = np.full(n_rays, K, dtype=np.int32)
    pick = rng.random(n_rays)
    count[pick < 0.1] = 0
    count[(pick >= 0.1) & (pick < 0.2)] = rng.integers(1, K, n_rays)[(pick >= 0.1) & (pick < 0.2)]
    count[pick >= 0.9] *= -1
    slot = np.arange(case.n)
    segs.ray.copy_(_device((slot % n_rays).astype(np.int32)))
    segs.count, segs.n_rays, segs.n_valid = _device(count), n_rays, None
    return segs, slot // n_rays < np.abs(count)[slot % n_rays]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("source", ["list", "holes", "slots"])
@pytest.mark.parametrize("name", ["two tiles", "two launches"])
def test_record_all_is_the_rule(name, source, precision):
    """table.record_all over 150,000 hand-made slots: 32 monitors (a count table of 2,369 elements, two scan tiles) and 40 (a second
    launch that takes first[32] over) — every monitor's slots, hit points and distances, bit for bit."""
    case = S.monitor(name)
    segs, valid = {"list": lambda c: (_list_of(c), None), "holes": _holes, "slots": _slots}[source](case)
    assert segs.layout == {"list": "list", "holes": "append", "slots": "slots"}[source]
    if valid is not None:
        assert 0.05 < 1 - valid.mean() < 0.3
    if precision == "f32":
        segs = segs.astype("f32")
    rule = S.monitor_rule(case, valid)
    hits = oa.OpticalTable().record_all(segs, monitors=S.monitors(oa, case.M))
    assert len(hits) == case.M
    for m, (got, (slot, P, t)) in enumerate(zip(hits, rule)):
        what = (name, source, precision, m)
        order = torch.argsort(got.slot)
        if source != "slots":  # (a list's reference order is its own)
            assert bool((order == torch.arange(len(got), device=order.device)).all()), what
        _same(got.slot[order], slot, (what, "slot"))
        _same(got.P[order], P, (what, "P"))
        _same(got.t[order], t, (what, "t"))


def test_record_many_over_two_spine_rounds():
    """ot_monitor_record_many over 34,000,000 single-precision slots and 32 monitors: a count table of 531,265 elements, 260 scan
    tiles, a second round of the 64-bit spine.  first[], the total and every monitor's list are the rule's; nothing is written
    behind the lists."""
    case = S.monitor("two spine rounds")
    assert S.scan_elements(case.n, case.M) == 531_265 > S.SPINE_ROUND
    rule = S.monitor_rule(case)
    sizes = [len(slot) for slot, _, _ in rule]
    total, M, n = sum(sizes), case.M, case.n
    eng = get_engine()
    position, k = _device(case.position).int(), _device(case.k)
    where = torch.from_numpy(S.MONITOR_POSITIONS).float().cuda()
    zero = lambda: torch.zeros(n, dtype=torch.float32, device="cuda")  # noqa: E731
    fields = dict(ox=zero(), oy=where[:, 0].index_select(0, position), oz=where[:, 1].index_select(0, position),
                  dx=torch.ones(n, dtype=torch.float32, device="cuda"), dy=zero(), dz=zero(), length=k.float() + 0.5)
    ray = torch.arange(n, dtype=torch.int32, device="cuda")
    del position, k
    src = abi.OtSegmentSource()
    for j, f in enumerate(abi.MON_FIELDS):
        src.base[j] = fields[f].data_ptr()
    src.ray, src.width, src.tile_stride, src.ray_stride, src.capacity = ray.data_ptr(), 4, 64 * 4, 64 * 4, n
    capacity = total + 64
    real = {f: (torch.float64, (capacity,)) for f in ("Px", "Py", "Pz", "t")}
    out = support.Sentinel(guard=64, first=(torch.int64, (M + 1,)), total=(torch.int64, (1,)), idx=(torch.int64, (capacity,)), **real)
    table = (abi.OtMonitor * M)(*[monitor_struct(m) for m in S.monitors(oa, M)])
    with eng.lock:
        abi.check(eng.lib.ot_monitor_record_many(eng._ctx, table, M, C.byref(src), n, None, 0, capacity, out.first.data_ptr(), out.idx.data_ptr(),
                                                 out.Px.data_ptr(), out.Py.data_ptr(), out.Pz.data_ptr(), out.t.data_ptr(), out.total.data_ptr()), eng.lib)
    assert int(out.total[0]) == total
    _same(out.first, np.concatenate([[0], np.cumsum(sizes)]), "first")
    _same(out.idx[:total], np.concatenate([slot for slot, _, _ in rule]), "slot")
    for j, f in enumerate(("Px", "Py", "Pz")):
        _same(getattr(out, f)[:total], np.concatenate([P[:, j] for _, P, _ in rule]), f)
    _same(out.t[:total], np.concatenate([t for _, _, t in rule]), "t")
    assert out.guards_untouched()
    assert all(bool((getattr(out, f)[total:] == out.fill).all()) for f in ("idx", "Px", "Py", "Pz", "t"))  # the room past the total, too
