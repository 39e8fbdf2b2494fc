"""The seeded cases tests/test_gpu_wavefront.py runs on the device and tests/test_wavefront_cpu.py checks on the host (through the
C oracle's trace of the same rays): scenes, monitors, references and pupils chosen so that the REFERENCE alone keeps every decision
1e-7 from its boundary, and the glue from segment records to tests/wavefront_reference.py."""
import numpy as np

import optable_amd as oa
import scenes
from optable_amd.table import monitor_struct
from optable_amd.wavefront import wavefront_coordinates, wavefront_pupil, wavefront_reference as reference_tables
from wavefront_reference import wavefront_reference

MARGIN = 1e-7


def cfg2_arrays(n, seed):
    """cfg 2's rays with per-ray intensities 0.25 + 0.75 u: (o, d, intensity)."""
    o, d = scenes.cfg2_rays(n, seed)
    return o, d, 0.25 + 0.75 * np.random.default_rng(seed + 7).random(n)


def axes_of(m):
    return np.concatenate([m.tangent_Y, m.tangent_Z]).astype(float)


def monitors_at(x):
    """A full monitor, one whose pupil will clip, one no segment reaches and one rotated about z, all on the axis at `x`."""
    return [oa.Monitor([x, 0, 0], 6, 6), oa.Monitor([x, 0, 0], 6, 6), oa.Monitor([x, 40, 0], 6, 6), oa.Monitor([x, 0, 0], 6, 6).RotZ(0.3)]


EMPTY = 2
# cfg 2: a point source at the origin, the f = 5 lens at x = 5, the mirror pair at x = 10.
#   "focus": monitors in the diverging cone at x = 2.5 against a focus a little off the source, in direction coordinates (the cone's
#   half angle is 0.15: R = 0.16 holds it, 0.1 clips it);  "direction": monitors in the collimated beam at x = 7.5 (radius 0.75)
#   against the plane wave along x, in position coordinates (R = 0.8 holds it, 0.4 clips it; the rotated monitor sees it tilted).
SETUPS = {
    "focus": dict(x=2.5, kwargs=dict(focus=(0.004, 0.003, -0.002)), pupil=[(0.0, 0.0, 0.16), (0.01, -0.02, 0.1), (0.0, 0.0, 0.16), (0.0, 0.0, 0.3)]),
    "direction": dict(x=7.5, kwargs=dict(direction=(1.0, 0.0, 0.0)), pupil=[(0.0, 0.0, 0.8), (0.05, 0.1, 0.4), (0.0, 0.0, 0.8), (0.0, 0.0, 0.85)]),
}


def reference(records, mon, kwargs, pupil, piston, weight="intensity", coordinates=None):
    """tests/wavefront_reference.py for one monitor on `records` = (o, d, length, intensity, n, pathlength), with the arguments of
    `OpticalTable.wavefront_all`; asserts the margin."""
    o, d, length, intensity, n_index, pathlength = records
    kind, _, local = reference_tables(kwargs.get("focus"), kwargs.get("direction"), [mon])
    pupil = wavefront_pupil(pupil, kind, [mon])[0]
    s = monitor_struct(mon)
    ref = wavefront_reference(o, d, length, intensity if weight == "intensity" else None, n_index, pathlength, list(s.M), list(s.origin), s.half_width,
                              s.half_height, axes_of(mon), kind, local[0], wavefront_coordinates(coordinates, kind), pupil, piston)
    print(f"  margin {ref.margin:.3g}, inside {ref.counts[0]}, outside {ref.counts[1]}")
    assert ref.margin > MARGIN  # a condition on the inputs
    return ref


def oracle_records(table, o, d, intensity, K):
    """The segments the C oracle traces for these rays, as `records`."""
    from optable_amd.batch import RayBatch
    from oracle import oracle as orc

    batch = RayBatch.from_arrays(o, d, wavelength=scenes.WL, intensity=intensity, q=1j * np.pi * scenes.W0**2 / scenes.WL, device="cpu")
    h = orc.trace(table.compile(), batch.to_host(), max_trace_num=K)
    return (np.stack([h["ox"], h["oy"], h["oz"]], 1), np.stack([h["dx"], h["dy"], h["dz"]], 1), h["length"], h["intensity"], h["n"], h["pathlength"])


# the seeded cfg 2 batches of the GPU tests: (rays, seed, segments)
CFG2_BATCHES = ((5003, 0, 5), (1, 3, 1), (130, 3, 3), (1027, 3, 5))
GROUP_MONITORS = 30  # more than one launch holds


def group_monitors():
    """30 monitors along the collimated beam of cfg 2, every third one rotated, with pupils of their own."""
    mons = [oa.Monitor([5.2 + 0.15 * k, 0, 0], 6, 6) for k in range(GROUP_MONITORS)]
    mons = [m.RotZ(0.05 * (k % 5)) if k % 3 == 2 else m for k, m in enumerate(mons)]
    return mons, [(0.01 * (k % 4), -0.01 * (k % 3), 0.5 + 0.01 * k) for k in range(GROUP_MONITORS)]
