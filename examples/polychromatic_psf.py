#!/usr/bin/env python3
"""The polychromatic image of a singlet from ONE trace: the lens of examples/chromatic_focus.py — a collimated bundle within a
pupil of radius 0.15, multiplexed in five wavelengths (`RayBatch.multiplexed_in_wavelength`), through a biconvex N-BK7 lens
(R = +-5, 0.4 thick) — with a monitor at x = 9.5 in the converging beams.  `spots_grouped_all` finds the plane of the smallest
spot of all wavelengths together; `psf_grouped_all` then sums, on the device, one diffraction image PER WAVELENGTH about that common
focus: the group of a hit is the wavelength of its input ray (`RayBatch.groups_by_wavelength`).  White light adds the
INTENSITIES of its wavelengths: `MonitorPSFGroups.strehl()` and `.mtf()` are the polychromatic Strehl ratio and MTF.  Beside them
what `psf_all` says on the same segments: it adds the FIELDS of all hits, as if the five wavelengths could interfere, which is no
image any instrument forms.
The rays fill the pupil on a uniform grid of positions, and behind this lens a ray's direction cosine is all but proportional to
its height: the sums are diffraction PSFs (optable_amd/psf.py: the model).
    python examples/polychromatic_psf.py            (needs an MI355X and the built library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optable_amd import BiConvexLens, Glass_NBK7, Monitor, OpticalTable  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

WAVELENGTHS = [400e-7, 486e-7, 560e-7, 656e-7, 780e-7]
RADIUS, X_MONITOR = 0.15, 9.5
NA = RADIUS / 5.0  # the marginal ray's direction cosine behind the lens, to one digit: sets the scale of the grid, nothing else


def main():
    g = np.linspace(-RADIUS, RADIUS, 81)
    y, z = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    keep = y * y + z * z <= RADIUS * RADIUS
    y, z = y[keep], z[keep]
    n = len(y)
    bundle = RayBatch.from_arrays(np.stack([np.zeros(n), y, z], axis=1), np.tile([1.0, 0.0, 0.0], (n, 1)), wavelength=WAVELENGTHS[0], intensity=1.0 / n)
    batch = bundle.multiplexed_in_wavelength(WAVELENGTHS)
    table = OpticalTable()
    table.add_components([BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n=Glass_NBK7())])
    monitor = Monitor([X_MONITOR, 0, 0], 1.0, 1.0)
    table.add_monitors([monitor])
    segs = table.trace_batch(batch, max_segments=4)
    ids, found = batch.groups_by_wavelength()
    labels = found.tolist()

    spot = table.spots_grouped_all(segs, ids, offsets=np.linspace(0.2, 1.0, 81), labels=labels)[0]
    x_focus = X_MONITOR + float(spot.total().best_focus()[0])
    step = 0.61 * WAVELENGTHS[0] / NA / 6
    psf = table.psf_grouped_batch(monitor, segs, batch, ids, focus=(x_focus, 0.0, 0.0), step=step, pixels=65, labels=labels)
    mixed = table.psf_batch(monitor, segs, batch, focus=(x_focus, 0.0, 0.0), step=step, pixels=65)

    print(f"{n} rays x {len(WAVELENGTHS)} wavelengths through a biconvex N-BK7 lens, one trace; common best focus x = {x_focus:.6f}; "
          f"65 x 65 samples {step:.3e} apart")
    print("  wavelength     hits   Strehl at the common focus")
    strehls = psf.strehls().cpu().numpy()
    for k, wl in enumerate(psf.labels):
        print(f"  {wl * 1e7:7.0f} nm  {int(psf.counts[k]):7d}   {strehls[k]:.6f}")
    print(f"polychromatic Strehl: {float(psf.strehl()):.6f}   (the intensities of the wavelengths added; ungrouped hits: {int(psf.ungrouped)})")
    print(f"psf_all Strehl: {float(mixed.strehl()):.6f}   (the fields of all wavelengths added coherently: not an image)")
    cutoff = 2 * NA / WAVELENGTHS[-1]
    for name, (mtf, fy, _) in (("polychromatic MTF", psf.mtf()), ("psf_all MTF", mixed.mtf())):
        row = mtf[:, mtf.shape[1] // 2]
        at = [int(np.argmin(np.abs(fy - f * cutoff))) for f in (0.25, 0.5, 0.75)]
        print(f"{name}: at 0.25, 0.5, 0.75 of the red cutoff 2 NA / lambda = {cutoff:.1f} cycles per unit along y: " + ", ".join(f"{row[k]:.3f}" for k in at))


if __name__ == "__main__":
    main()
