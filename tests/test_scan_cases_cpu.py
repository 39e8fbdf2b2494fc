"""CPU: what tests/scan_cases.py claims of its cases, proved from the builders' own arrays — the boundaries lie inside the trees,
the hits on the sides stated, the scans as long as stated — and two checks of the numpy rules themselves.  No device."""
import numpy as np
import pytest

import optable_amd as oa
import scan_cases as S


def test_the_restated_structure():
    assert S.SCAN_TILE == 8 * S.WORKGROUP and S.SPINE_ROUND == 256 * S.SCAN_TILE == 524_288
    assert S.slot_partition(150_000) == (8, 2048, 74) and S.slot_partition(34_000_000) == (8, 2048, 16_602)
    assert S.slot_partition(1 << 26)[0] == 16
    assert S.scan_elements(150_000, 32) == 2_369 and S.scan_elements(150_000, 40) == 2_369
    assert S.scan_elements(34_000_000, 32) == 531_265 and -(-531_265 // S.SCAN_TILE) == 260
    assert sorted({n for n, _, _ in S.LAYOUTS.values()}) == [1, 64, 65, 300, 2_560, 528_384]


def test_start_points_are_exact_and_clear_of_every_rim():
    for table in (S.POSITIONS, S.MONITOR_POSITIONS):
        assert np.array_equal(table.astype(np.float32).astype(np.float64), table) and np.array_equal(table * 64, np.round(table * 64))
    y, z = S.POSITIONS[:, 0], S.POSITIONS[:, 1]
    for s in range(3):  # the discs
        off = np.hypot(y - S.CENTRE[s, 0], z - S.CENTRE[s, 1]) - S.RADIUS[s]
        assert np.all(np.abs(off) >= S.MARGIN)
        assert np.array_equal(off < 0, S.MEETS[S.POSITION_CLASS, s])  # the class of a start point is what its ray meets
    off = np.maximum(np.abs(y), np.abs(z)) - S.TWIN_HALF  # the twin's square: the same rays meet it as A's disc
    assert np.all(np.abs(off) >= S.MARGIN) and np.array_equal(off < 0, S.MEETS[S.POSITION_CLASS, 0])
    y, z = S.MONITOR_POSITIONS[:, 0], S.MONITOR_POSITIONS[:, 1]
    assert np.all(np.abs(np.abs(y) - S.MONITOR_HALF) >= 0.25) and np.all(np.abs(np.abs(z) - S.MONITOR_HALF) >= 0.25)
    # the poses: a half turn with exact entries, every leaf facing -x
    for c in S.gated_components(oa) + S.twin_components(oa) + S.monitors(oa, 3):
        assert np.array_equal(c.normal, [-1.0, 0.0, 0.0]) and np.array_equal(c.transform_matrix @ c.transform_matrix.T, np.identity(3))
        assert np.linalg.det(c.transform_matrix) == 1.0


def test_layouts_hold_the_trees_they_name():
    ends = lambda name: set(np.cumsum(S.LAYOUTS[name][1]).tolist())  # noqa: E731
    assert 64 in ends("a wave and a ray") and {64, 256, 2048} <= ends("edges")  # a tree ends on the boundary, the next starts on it
    for name, (n, sizes, planted) in S.LAYOUTS.items():
        assert sum(sizes) == n
        assert 1 in sizes  # trees of one ray
    n, sizes, _ = S.LAYOUTS["two spine rounds"]
    t = S._index_of(sizes, 40_860)
    assert sizes[t] == 5_000 and 45_860 // S.SCAN_TILE - -(-40_860 // S.SCAN_TILE) == 2  # whole scan tiles inside one tree
    case = S.gated("two spine rounds", "behind")
    inside = slice(40_860, 45_860)
    for s in range(2):
        hits_per_tile = np.bincount(np.arange(n)[inside][S.MEETS[case.cls[inside], s]] // S.SCAN_TILE)
        assert np.count_nonzero(hits_per_tile) == 4
    boundaries = sorted(b for _, b in S.LAYOUTS["two spine rounds"][2])
    assert boundaries == [S.WAVE, S.WORKGROUP, S.SCAN_TILE, S.SPINE_ROUND]


@pytest.mark.parametrize("name,variant", [c for c in S.GATED_CASES if c[1] != "seeded"])
def test_planted_trees_straddle_their_boundary_as_stated(name, variant):
    case = S.gated(name, variant)
    rule = S.gated_rule(case)
    assert len(case.planted) == len(S.LAYOUTS[name][2]) > 0
    for t, boundary, _ in case.planted:
        h, e = int(case.start[t]), int(case.start[t] + case.sizes[t])
        assert h < boundary < e and 0 <= case.column[t] < case.n_classes
        for s in range(2):
            hit = np.flatnonzero(S.MEETS[case.cls[h:e], s]) + h  # the tree's geometric hits on s
            assert np.any(hit < boundary) and np.any(hit >= boundary)
            left = int(S.MAX_COUNT[s] - case.counts0[s, case.column[t]])
            assert 1 <= left <= len(hit)
            deciding = hit[left - 1]  # the last hit the gate lets through
            if variant == "behind":
                assert deciding >= boundary and left >= 2
            else:
                assert deciding < boundary
            assert np.any(hit > max(deciding, boundary - 1))  # hits behind the boundary that find the gate closed
            # ... and the rule says so: the deciding ray may end on s (A takes a ray that meets both), no later ray of the tree does
            assert np.all(rule.surface[deciding + 1:e] != s)
            if case.cls[deciding] != S.A_AND_B or s == 0:
                assert rule.surface[deciding] == s
        assert case.counts0[:, case.column[t]].tolist() == ((S.MAX_COUNT - 2).tolist() if variant == "behind" else [0, 0])
        assert rule.counts[:, case.column[t]].tolist() == S.MAX_COUNT.tolist()


@pytest.mark.parametrize("name,variant", S.GATED_CASES)
def test_every_case_is_well_formed(name, variant):
    case = S.gated(name, variant)
    assert np.all(np.diff(case.tree) >= 0) and case.tree[0] == 0 and len(case.tree) == case.n
    assert np.array_equal(case.tree[case.head], case.tree) and np.all((case.head == 0) | (case.tree[case.head - 1] != case.tree))
    for s in range(2):
        assert set(case.counts0[s].tolist()) <= set(S.start_values(s).tolist())
    assert case.counts0.shape == (2, len(case.sizes))
    listed = case.column[(case.column >= 0) & (case.column < case.n_classes)]
    assert len(set(listed.tolist())) == len(listed)  # a column per tree
    if len(case.sizes) >= 5:
        assert sorted(case.outside.values()) == [-3, case.n_classes + 5] and not set(case.outside) & {p[0] for p in case.planted}
        rule = S.gated_rule(case)
        for t in case.outside:  # never gated: the nearest surface met, whatever the table says; the table as it was
            rays = slice(int(case.start[t]), int(case.start[t] + case.sizes[t]))
            assert np.array_equal(rule.surface[rays], np.array([0, 0, 1, 2, -1])[case.cls[rays]])
        assert np.array_equal(rule.counts[:, list(case.outside)], case.counts0[:, list(case.outside)])
    o, d = S.origins(case)
    assert np.array_equal(o.astype(np.float32).astype(np.float64), o) and np.all(o[:, 0] == 0) and np.all(d == [1, 0, 0])


def _loop_rule(case, budget=None):
    """gated_rule as the reference runs it: ray by ray, a counter per (surface, id)."""
    count = {(s, c): int(case.counts0[s, c]) for s in range(2) for c in range(case.n_classes)}
    left = [case.n + 1] * len(case.sizes) if budget is None else [int(b) for b in budget]
    doomed = [case.sizes[t] >= left[t] for t in range(len(case.sizes))]
    surface, ray, length, children = [], [], [], []
    for i in range(case.n):
        t, c = int(case.tree[i]), int(case.ids[i])
        if left[t] <= 0:
            children.append(0)
            continue
        left[t] -= 1
        best = -1
        for s in (2, 1, 0):  # farthest first: the nearest open surface stays
            if not S.MEETS[case.cls[i], s]:
                continue
            if s < 2 and 0 <= c < case.n_classes:
                if count[s, c] >= S.MAX_COUNT[s]:
                    continue
                count[s, c] += 1
            best = s
        surface.append(best)
        ray.append(t)
        length.append(S.PLANE_X[best] if best >= 0 else np.inf)
        children.append(1 if best >= 0 and not doomed[t] else 0)
    table = np.array([[count[s, c] for c in range(case.n_classes)] for s in range(2)])
    return surface, ray, length, children, table, left


@pytest.mark.parametrize("variant", ["behind", "closed"])
@pytest.mark.parametrize("budgeted", [False, True])
def test_the_cumsum_rule_is_the_ray_by_ray_rule(variant, budgeted):
    case = S.gated("two workgroups", variant)
    budget = S.budgets(case) if budgeted else None
    rule = S.gated_rule(case, budget)
    surface, ray, length, children, table, left = _loop_rule(case, budget)
    assert rule.surface.tolist() == surface and rule.ray.tolist() == ray and rule.length.tolist() == length
    assert rule.children.tolist() == children and np.array_equal(rule.counts, table) and rule.budget.tolist() == left
    assert int(rule.processed.sum()) == len(surface) and (len(surface) < case.n) == budgeted
    # (a start count above the cap stays: the table is never lowered)
    assert np.all(rule.counts >= case.counts0) and np.all(rule.counts <= np.maximum(case.counts0, S.MAX_COUNT[:, None]))


@pytest.mark.parametrize("name", ["two workgroups", "two scan tiles"])
def test_the_rule_is_the_oracles(name, oracle):
    """The C oracle traces its input rays one after the other over one table: with a cap of one ray a tree, the rays of a column
    meet the gates in input order, which is the order of a tree's rays inside a generation."""
    case = S.gated(name, "behind")
    table = oa.OpticalTable()
    table.add_components(S.gated_components(oa))
    o, d = S.origins(case)
    zeros, ones = np.zeros(case.n), np.ones(case.n)
    # (the oracle indexes its table by every id: the two trees with ids outside the table get columns that never fill)
    T = case.n_classes
    assert sorted(case.outside.values()) == [-3, T + 5]
    ids = np.where(case.ids < 0, T, np.where(case.ids >= T, T + 1, case.ids))
    counts = np.hstack([case.counts0, np.full((2, 2), -1_000_000, dtype=np.int32)])
    rays = dict(ox=o[:, 0], oy=o[:, 1], oz=o[:, 2], dx=d[:, 0], dy=d[:, 1], dz=d[:, 2], wavelength=ones * 780e-7, intensity=ones, q_re=zeros, q_im=zeros,
                n=ones, pathlength=zeros, id=ids, flags=np.zeros(case.n, dtype=np.int32))
    ref = oracle.trace(table.compile(), rays, max_trace_num=1, counts=counts, n_classes=T + 2)
    rule = S.gated_rule(case)
    assert np.array_equal(ref["ray"], np.arange(case.n)) and np.array_equal(ref["surface"], rule.surface)
    assert np.array_equal(ref["length"], rule.length) and np.array_equal(ref["counts"][:, :T], rule.counts)


@pytest.mark.parametrize("variant", ["behind", "closed"])
def test_a_lost_spine_carry_changes_the_straddling_tree(variant):
    """Mutation check: ranks from a scan whose second spine round starts from zero (every prefix from element 524,288 on short of
    the total before it).  The rays of the straddling tree behind the boundary then find the gates open: the case sees the defect."""
    case = S.gated("two spine rounds", variant)
    good = S.gated_rule(case)
    bad = S.gated_rule(case, scan=lambda flags: S.lost_spine_carry(S.exclusive_scan(flags)))
    t, boundary, _ = case.planted[-1]
    assert boundary == S.SPINE_ROUND
    e = int(case.start[t] + case.sizes[t])
    assert np.array_equal(good.surface[:boundary], bad.surface[:boundary])
    for s in range(2):
        assert np.count_nonzero(bad.surface[boundary:e] == s) > np.count_nonzero(good.surface[boundary:e] == s)
    assert np.array_equal(good.surface[e:], bad.surface[e:])  # (a tree that lies behind the boundary whole takes differences: it is blind to it)


@pytest.mark.parametrize("name", list(S.MONITOR_CASES))
def test_monitor_cases_reach_the_scan_sizes_they_name(name):
    case = S.monitor(name)
    boundary = S.SPINE_ROUND if name == "two spine rounds" else S.SCAN_TILE
    assert S.scan_elements(case.n, case.M) > boundary and case.grid == S.slot_partition(case.n)[2]
    assert (case.M > S.MON_MAX) == (name == "two launches")
    assert case.k.min() == 0 and case.k.max() == case.M
    rule = S.monitor_rule(case)
    m, g = S._straddled(case.n, case.M, boundary)  # element `boundary` is count[m][g]: the monitor's entries lie on both sides of it
    assert 0 < g < case.grid and m < min(case.M, S.MON_MAX)
    groups = rule[m][0] // case.span
    assert np.any(groups == g - 1) and np.any(groups == g) and np.any(groups < g - 2) and np.any(groups > g + 1)
    per_group = np.stack([np.bincount(slot // case.span, minlength=case.grid) for slot, _, _ in rule])  # count[monitor][workgroup]
    assert case.empty and case.full and not per_group[:, list(case.empty)].any() and np.all(per_group[:, list(case.full)] == case.span)
    total = int(per_group.sum())
    assert total == sum(len(slot) for slot, _, _ in rule) and total < 4_000_000  # the hit lists stay small
    if name == "two spine rounds":
        assert 0.03 < case.k.mean() < 0.07
        ex = S.exclusive_scan(per_group[:S.MON_MAX].reshape(-1))  # the scan itself: its total before the second spine round is not zero
        assert ex[S.SPINE_ROUND] > 0 and ex[-1] > ex[S.SPINE_ROUND]
    else:  # the rule, literally
        y, z = S.MONITOR_POSITIONS[case.position].T
        for mm, (slot, P, t) in enumerate(rule):
            assert np.array_equal(slot, np.flatnonzero((mm < case.k) & (np.abs(y) <= 1) & (np.abs(z) <= 1)))
            assert np.array_equal(P, np.stack([0 * y, -y, z], 1)[slot]) and np.all(t == mm + 1)
    assert np.array_equal((case.k + 0.5).astype(np.float32).astype(np.float64), case.k + 0.5)
