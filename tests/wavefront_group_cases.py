"""The seeded cases of tests/test_gpu_wavefront_groups.py and the glue from segment records to tests/wavefront_reference.py per
(monitor, group): the reference of cell (m, g) is `wavefront_reference` on the records whose input ray has id g, with that cell's
own reference, pupil and piston.  Scenes, seeds, references and pupils are chosen so that the REFERENCE alone keeps every decision
1e-7 from its boundary (asserted per cell; tests/test_wavefront_groups_cpu.py checks it on the host through the C oracle's trace)."""
import numpy as np

import optable_amd as oa
import wavefront_cases as cases
from optable_amd.table import monitor_struct
from optable_amd.wavefront import wavefront_coordinates, wavefront_reference as reference_tables
from wavefront_reference import wavefront_reference

RAYS, SEED, SEGMENTS, G = 4096, 21, 5, 5


def ids_of(n, seed=SEED, low=-1, high=G + 1):
    """Random ids in low .. high - 1: by default -1 (masked) .. G (one id >= G, in no group either)."""
    return np.random.default_rng(seed + 100).integers(low, high, n).astype(np.int32)


def monitors_at(x):
    return [oa.Monitor([x, 0, 0], 6, 6), oa.Monitor([x, 0, 0], 6, 6).RotZ(0.3)]


g_ = np.arange(G, dtype=float)
# cfg 2 as in wavefront_cases.SETUPS, with a reference per group [G, 3] and a pupil per cell [2, G, 3] whose centres differ.
#   "focus": the diverging cone at x = 2.5 in direction coordinates (half angle 0.15; the rotated monitor's a_y sees the axis at -0.2955);
#   "direction": the collimated beam at x = 7.5 (radius 0.75) in position coordinates.
# `other`: the pupil [G, 3] used with the coordinates that are not the default.
SETUPS = {
    "focus": dict(x=2.5, name="focus", reference=np.stack([0.004 + 0.001 * g_, 0.003 - 0.0005 * g_, -0.002 + 0.0007 * g_], axis=1),
                  pupil=np.stack([np.stack([0.01 * g_ - 0.02, 0.004 * g_, 0.1 + 0.015 * g_], axis=1),
                                  np.stack([-0.29 + 0.005 * g_, 0.002 * g_, 0.17 + 0.0 * g_], axis=1)]),
                  other=np.stack([0.01 * g_, -0.005 * g_, 0.3 + 0.0 * g_], axis=1)),
    "direction": dict(x=7.5, name="direction", reference=np.stack([1.0 + 0.0 * g_, 0.001 * g_, -0.0005 * g_], axis=1),
                      pupil=np.stack([np.stack([0.05 * g_ - 0.1, 0.02 * g_, 0.5 + 0.05 * g_], axis=1),
                                      np.stack([0.02 * g_, -0.01 * g_, 0.85 + 0.0 * g_], axis=1)]),
                      other=np.stack([0.0005 * g_, 0.0 * g_, 0.01 + 0.002 * g_], axis=1)),
}


def members(ray, ids, g):
    """Which records belong to group g: those whose input ray is inside the table and has id g."""
    ray, ids = np.asarray(ray), np.asarray(ids)
    known = (ray >= 0) & (ray < len(ids))
    out = np.zeros(len(ray), dtype=bool)
    out[known] = ids[ray[known]] == g
    return out


def cell_reference(records, ray, ids, g, mon, name, vector, pupil, piston, coordinates=None, weight="intensity"):
    """tests/wavefront_reference.py for cell (mon, g) on `records` = (o, d, length, intensity, n, pathlength) with the records'
    `ray`: `name` = "focus" | "direction" with the lab `vector`, the cell's pupil (c_y, c_z, R) and piston; asserts the margin."""
    o, d, length, intensity, n_index, pathlength = records
    kind, _, local = reference_tables(vector if name == "focus" else None, vector if name == "direction" else None, [mon])
    s = monitor_struct(mon)
    ref = wavefront_reference(o, d, length, intensity if weight == "intensity" else None, n_index, pathlength, list(s.M), list(s.origin), s.half_width,
                              s.half_height, cases.axes_of(mon), kind, local[0], wavefront_coordinates(coordinates, kind), pupil, piston,
                              valid=members(ray, ids, g))
    assert ref.margin >= cases.MARGIN, (g, ref.margin)  # a condition on the inputs
    return ref


def cell_references(records, ray, ids, mons, name, reference, pupil, piston, n_groups, **kw):
    """[m][g] of `cell_reference`; reference [G, 3] or [M, G, 3], pupil and piston [M, G, ...]."""
    reference = np.broadcast_to(reference, (len(mons), n_groups, 3))
    return [[cell_reference(records, ray, ids, g, mon, name, reference[m, g], pupil[m][g], float(piston[m][g]), **kw) for g in range(n_groups)]
            for m, mon in enumerate(mons)]
