"""Hand-made inputs for the users of the device-wide exclusive scan (`exclusive_scan`, optable_amd/csrc/misc_kernels.h) at the
sizes where the scan changes shape, and the numpy rules that say what must come out.  Host arrays only: nothing here touches the
device or the built library; tests/test_scan_cases_cpu.py proves the conditions the cases claim, tests/test_gpu_scan_sizes.py
runs them.

Every value is exact in single and double precision and every decision is an integer one, so the expected output is exact."""
import types

import numpy as np

# -- 1: the structure of the kernels, restated (not imported: a test of these sizes must not move with the code it tests) ---------
WAVE = 64                      # a wavefront: k_gen_probe / k_gen_pass look for a tree's head inside it first (csrc/kernels.h)
WORKGROUP = 256                # the block of every generation kernel, and MON_THREADS (csrc/misc_kernels.h)
SCAN_TILE = 2048               # SCAN_THREADS * SCAN_ITEMS = 256 * 8 (csrc/misc_kernels.h)
SPINE_ROUND = 256 * SCAN_TILE  # k_scan_spine scans SCAN_THREADS tile sums a round and carries the total on: 524,288 elements
MON_MAX = 32                   # monitors of one launch of k_mon_count / k_mon_emit (csrc/misc_kernels.h)


def slot_partition(n):
    """(iters, span, grid) of csrc/optable_hip.hip slot_partition(n, through_lds = false): workgroups of `iters` visits of 256 slots."""
    iters = max(8, n >> 22)
    span = iters * 256
    return iters, span, -(-n // span)


def scan_elements(n_slots, n_monitors):
    """Elements of the scan of one launch of Monitor.record's passes: count[monitor][workgroup] and one more."""
    return min(n_monitors, MON_MAX) * slot_partition(n_slots)[2] + 1


FACING_MINUS_X = np.diag([-1.0, -1.0, 1.0])  # the pose of every leaf and monitor here: half a turn about z, with no sin(pi) in it


def _facing(component):
    component.transform_matrix = FACING_MINUS_X.copy()
    return component


# -- 2: one generation through a gated scene --------------------------------------------------------------------------------------
# Surfaces 0, 1, 2 = A, B, C: discs in planes x = 4, 6, 8 about (y, z) = (0, 0), (1, 0), (0, 0); A and B count-limited.
CENTRE = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
RADIUS = np.array([1.0, 1.0, 6.0])
PLANE_X = np.array([4.0, 6.0, 8.0])
MAX_COUNT = np.array([3, 2])  # of A and B
TWIN_HALF = 1.0               # the gate-free twin: A is a beam splitter, a square of 2 x 2
MARGIN = 0.05

A_ONLY, A_AND_B, B_ONLY, CATCH, NOTHING = range(5)  # what a ray along +x meets: the class of its start point
# start points (y, z), multiples of 1/64, two per class: row 2 * class and the one after it
POSITIONS = np.array([[-0.5, 0.0], [-0.25, 0.5],     # A only
                      [0.5, 0.0], [0.5, 0.25],       # A and B
                      [1.5, 0.0], [1.25, -0.5],      # B only
                      [0.0, 3.0], [-2.0, 1.5],       # neither: the catch C
                      [0.0, 8.0], [7.0, 0.0]])       # nothing at all
POSITION_CLASS = np.repeat(np.arange(5), 2)
MEETS = np.array([[True, False, True], [True, True, True], [False, True, True], [False, False, True], [False, False, False]])  # [class][surface]


def gated_components(ns):
    """The gated scene from the package `ns`: A (3 interactions), B (2), the catch C."""
    return [_facing(ns.Mirror([4, 0, 0], radius=1, max_interact_count=int(MAX_COUNT[0]))),
            _facing(ns.Mirror([6, 1, 0], radius=1, max_interact_count=int(MAX_COUNT[1]))),
            _facing(ns.Mirror([8, 0, 0], radius=6))]


def twin_components(ns):
    """The gate-free twin: a beam splitter (two children) in A's place, B unlimited."""
    return [_facing(ns.BeamSplitter([4, 0, 0], width=2 * TWIN_HALF, height=2 * TWIN_HALF, eta=0.5)),
            _facing(ns.Mirror([6, 1, 0], radius=1)), _facing(ns.Mirror([8, 0, 0], radius=6))]


def start_values(slot):
    m = int(MAX_COUNT[slot])
    return np.array([0, 1, m - 1, m, m + 2])


def gated_case(n, sizes, planted=(), seed=0):
    """A generation of n rays in trees of the given sizes (input order), tree t with column t of the start table.
    planted: (tree, boundary, variant) — the tree's rays around index `boundary` and its start counts are set so that for A and for B
      "behind": one geometric hit lies before the boundary, the deciding one (the (max - start)-th) and further ones behind it;
      "closed": the gate closes before the boundary and further geometric hits lie behind it.
    Everything else is seeded: start points, start counts from start_values, and two unplanted trees with ids outside the table."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert sizes.sum() == n and sizes.min() >= 1
    T = len(sizes)
    rng = np.random.default_rng(seed)
    start = np.cumsum(sizes) - sizes
    tree = np.repeat(np.arange(T, dtype=np.int32), sizes)
    position = rng.integers(0, len(POSITIONS), n)
    counts0 = np.stack([rng.choice(start_values(s), T) for s in range(2)]).astype(np.int32)
    column = np.arange(T, dtype=np.int32)
    free = [t for t in range(T) if t not in {p[0] for p in planted} and sizes[t] >= 3]
    outside = {}
    if len(free) >= 2:  # never gated, and they leave the table as it is
        outside = {free[0]: -3, free[-1]: T + 5}
        for t, value in outside.items():
            column[t] = value
    for t, boundary, variant in planted:
        h, e = int(start[t]), int(start[t] + sizes[t])
        assert h + 8 <= boundary <= e - 8, (t, h, boundary, e)
        quiet = np.where(np.arange(h, boundary) & 1, 2 * CATCH, 2 * NOTHING + 1)
        if variant == "behind":
            position[h:boundary] = quiet
            position[boundary - 3], position[boundary - 2] = 2 * A_ONLY, 2 * B_ONLY + 1
            counts0[:, t] = MAX_COUNT - 2
            position[boundary:boundary + 6] = [2 * CATCH + 1, 2 * A_ONLY + 1, 2 * B_ONLY, 2 * A_ONLY, 2 * B_ONLY + 1, 2 * A_AND_B]
        else:
            assert variant == "closed"
            position[boundary - 8:boundary] = [2 * A_ONLY, 2 * A_ONLY + 1, 2 * A_ONLY, 2 * A_ONLY + 1, 2 * B_ONLY, 2 * B_ONLY + 1, 2 * B_ONLY, 2 * A_AND_B]
            counts0[:, t] = 0
            position[boundary:boundary + 3] = [2 * A_ONLY + 1, 2 * B_ONLY, 2 * A_AND_B + 1]
    return types.SimpleNamespace(n=n, sizes=sizes, start=start, tree=tree, head=np.repeat(start, sizes), ids=np.repeat(column, sizes), column=column,
                                 outside=outside, position=position, cls=POSITION_CLASS[position], y=POSITIONS[position, 0], z=POSITIONS[position, 1],
                                 counts0=counts0, n_classes=T, planted=tuple(planted))


def origins(case):
    """(o [n, 3], d [n, 3]): every ray from x = 0 along +x."""
    return np.stack([np.zeros(case.n), case.y, case.z], 1), np.tile([1.0, 0.0, 0.0], (case.n, 1))


def exclusive_scan(flags):
    return np.cumsum(flags) - flags


def lost_spine_carry(ex, at=SPINE_ROUND):
    """What a scan whose spine forgets its running total at element `at` would leave: every later prefix short of ex[at]."""
    out = ex.copy()
    out[at:] -= ex[at]
    return out


def gated_rule(case, budget=None, scan=exclusive_scan):
    """The reference's rule for one generation (optical_component.py:140-149, 359-362, as count_gate<GATE_TABLE> and k_gen_counts of
    csrc restate it): a ray passes limited surface s iff start count + earlier rays of its tree (input order) that meet s < max_s;
    it ends on the nearest surface it meets and passes, C always open; ids outside the table are never gated and count nothing.
    budget[tree]: only a tree's first budget[tree] rays are processed, the others leave no record, hit and child, and a tree that
    uses its budget up emits no children (include/optable_hip.h: ot_trace_generation_*).  `scan`: the exclusive scan the ranks
    come from, for the mutation check.  Records in input order of the processed rays."""
    n, head, tree = case.n, case.head, case.tree
    size = case.sizes[tree]
    left = np.full(len(case.sizes), n + 1, dtype=np.int64) if budget is None else np.asarray(budget, dtype=np.int64)
    active = np.arange(n) - head < left[tree]
    doomed = size >= left[tree]
    meets = MEETS[case.cls] & active[:, None]
    listed = (case.ids >= 0) & (case.ids < case.n_classes)
    col = np.where(listed, case.ids, 0)
    passes = np.ones((n, 3), dtype=bool)
    counts = case.counts0.copy()
    for s in range(2):
        ex = scan(meets[:, s].astype(np.int64))
        rank = ex - ex[head]
        passes[:, s] = ~listed | (case.counts0[s, col] + rank < MAX_COUNT[s])
        last = case.start + case.sizes - 1
        own = np.flatnonzero((case.column >= 0) & (case.column < case.n_classes))  # the trees with a column (each its own)
        c0 = case.counts0[s, case.column[own]]
        total = c0 + rank[last[own]] + meets[last[own], s]  # start count + the tree's geometric hits
        counts[s, case.column[own]] = np.where(total < MAX_COUNT[s], total, np.maximum(c0, MAX_COUNT[s]))
    open_ = meets & passes
    surface = np.where(open_.any(1), np.argmax(open_, 1), -1).astype(np.int32)  # (the surfaces are listed nearest first)
    length = np.where(surface >= 0, PLANE_X[np.maximum(surface, 0)], np.inf)
    children = np.where(active & ~doomed & (surface >= 0), 1, 0)
    return types.SimpleNamespace(processed=active, surface=surface[active], ray=tree[active], length=length[active], children=children,
                                 parent=np.repeat(np.arange(n), children), counts=counts,
                                 budget=left - np.minimum(case.sizes, left))


def budgets(case, seed=5):
    """Rays a tree may still process, seeded: more than it has, exactly as many (used up: no children), half as many, one; a planted
    tree four past its boundary, inside the rays planted there."""
    rng = np.random.default_rng(seed)
    sizes = case.sizes
    budget = np.choose(rng.integers(0, 4, len(sizes)), [sizes + 3, sizes, np.maximum(sizes // 2, 1), np.ones_like(sizes)])
    for t, boundary, _ in case.planted:
        budget[t] = boundary - case.start[t] + 4
    return budget.astype(np.int32)


def twin_rule(case):
    """The gate-free twin: the nearest surface met; two children at the beam splitter, one at a mirror, none for a ray that meets nothing."""
    surface = np.array([0, 0, 1, 2, -1], dtype=np.int32)[case.cls]
    length = np.array([4.0, 4.0, 6.0, 8.0, np.inf])[case.cls]
    children = np.array([2, 2, 1, 1, 0])[case.cls]
    return types.SimpleNamespace(processed=np.ones(case.n, dtype=bool), surface=surface, ray=case.tree, length=length, children=children,
                                 parent=np.repeat(np.arange(case.n), children))


def _filled(n, rng, fixed):
    """Tree sizes summing to n: the (start, size) pairs of `fixed` where they are asked for, seeded sizes of 1 .. 600 between them."""
    sizes, at = [], 0
    for start, size in sorted(fixed) + [(n, 0)]:
        while at < start:
            step = int(min(rng.integers(1, 601), start - at))
            sizes.append(step)
            at += step
        if size:
            sizes.append(size)
            at += size
    assert at == n
    return sizes


def _index_of(sizes, start):
    return int(np.flatnonzero(np.cumsum(sizes) - np.asarray(sizes) == start)[0])


# name -> (n, tree sizes, [(start of a planted tree, boundary)]); every planted layout is built in both variants
def _layouts():
    rng = np.random.default_rng(11)
    big_fixed = [(30, 60), (200, 100), (2000, 100), (40_860, 5000), (SPINE_ROUND - 3000, 4000)]
    return {
        "one ray": (1, [1], []),
        "a wave": (64, [1, 1, 20, 42], []),
        "a wave and a ray": (65, [64, 1], []),                                  # a tree that ends on 64, the next starting on it
        "two workgroups": (300, [40, 50, 1, 1, 100, 108], [(40, 64), (192, 256)]),
        "two scan tiles": (2560, [30, 60, 110, 100, 1700, 100, 1, 1, 458], [(30, 64), (200, 256), (2000, 2048)]),
        "edges": (2560, [64, 192, 1792, 1, 511], []),                           # trees that end on 64, 256 and 2,048; the next one a single ray
        "two spine rounds": (SPINE_ROUND + 2 * SCAN_TILE, _filled(SPINE_ROUND + 2 * SCAN_TILE, rng, big_fixed),
                             [(30, 64), (200, 256), (2000, 2048), (SPINE_ROUND - 3000, SPINE_ROUND)]),  # and 5,000 rays from 40,860: two whole scan tiles and parts of two more in one tree
    }


LAYOUTS = _layouts()
GATED_CASES = [(name, variant) for name, (_, _, planted) in LAYOUTS.items() for variant in (("behind", "closed") if planted else ("seeded",))]
_gated = {}


def gated(name, variant):
    """The case of a layout and a variant, built once."""
    if (name, variant) not in _gated:
        n, sizes, planted = LAYOUTS[name]
        _gated[name, variant] = gated_case(n, sizes, [(_index_of(sizes, start), boundary, variant) for start, boundary in planted],
                                           seed=GATED_CASES.index((name, variant)) + 1)
    return _gated[name, variant]


# -- 3: segment lists for Monitor.record --------------------------------------------------------------------------------------------
# Monitor m is the plane x = m + 1, 2 x 2; slot s runs from (0, y, z) along +x for k + 0.5: it crosses the planes of the monitors m < k,
# inside the aperture or far outside it, at t = m + 1 and the local point (0, -y, z) (the pose FACING_MINUS_X turns y over).
MONITOR_POSITIONS = np.array([[0.75, 0.75], [-0.75, 0.25], [0.0, -0.75], [5.0, 0.0], [0.5, -7.0]])
MONITOR_HALF = 1.0


def monitors(ns, M):
    return [_facing(ns.Monitor([m + 1, 0, 0], 2 * MONITOR_HALF, 2 * MONITOR_HALF)) for m in range(M)]


def monitor_case(n, M, rate, seed, empty=(), full=()):
    """n slots against M monitors: k > 0 for a seeded share `rate` of the slots (then uniform in 1 .. M), the start points seeded;
    the workgroup spans listed in `empty` hold no hit at all, those in `full` hits of every slot on every monitor."""
    rng = np.random.default_rng(seed)
    _, span, grid = slot_partition(n)
    k = np.where(rng.random(n, dtype=np.float32) < rate, rng.integers(1, M + 1, n, dtype=np.int8), np.int8(0)).astype(np.int8)
    position = rng.integers(0, len(MONITOR_POSITIONS), n, dtype=np.int8)
    for g in empty:
        k[g * span:(g + 1) * span] = 0
    for g in full:
        k[g * span:(g + 1) * span], position[g * span:(g + 1) * span] = M, g % 3
    return types.SimpleNamespace(n=n, M=M, span=span, grid=grid, k=k, position=position, empty=tuple(empty), full=tuple(full))


def monitor_rule(case, valid=None):
    """Per monitor the slots that hit it, ascending (np.flatnonzero), with the local hit point and the distance: (slot, P [h, 3], t)."""
    y, z = MONITOR_POSITIONS[:, 0], MONITOR_POSITIONS[:, 1]
    inside = ((np.abs(y) <= MONITOR_HALF) & (np.abs(z) <= MONITOR_HALF))[case.position]
    some = np.flatnonzero((case.k > 0) & inside & (True if valid is None else valid))  # the slots that hit any monitor
    out = []
    for m in range(case.M):
        slot = some[case.k[some] > m]
        P = np.stack([np.zeros(len(slot)), -y[case.position[slot]], z[case.position[slot]]], 1)
        out.append((slot, P, np.full(len(slot), m + 1.0)))
    return out


def _straddled(n, M, boundary):
    """(monitor, workgroup) of element `boundary` of the scan over count[monitor][workgroup]."""
    return divmod(boundary, slot_partition(n)[2])


def _monitor_cases():
    small, large = 150_000, 34_000_000
    _, g_small = _straddled(small, 32, SCAN_TILE)
    _, g_large = _straddled(large, 32, SPINE_ROUND)
    return {  # name -> (n, M, rate, seed, empty spans, full spans): hits in the workgroups on both sides of the element boundary
        "two tiles": (small, 32, 0.02, 21, (0, g_small - 2, g_small + 1), (g_small - 1, g_small)),
        "two launches": (small, 40, 0.02, 22, (0, g_small - 2, g_small + 1), (g_small - 1, g_small)),
        "two spine rounds": (large, 32, 0.003, 23, (0, g_large - 2, g_large + 1, 16_000), (g_large - 1, g_large, 4_000)),
    }


MONITOR_CASES = _monitor_cases()
_monitor = {}


def monitor(name):
    if name not in _monitor:
        _monitor[name] = monitor_case(*MONITOR_CASES[name])
    return _monitor[name]
