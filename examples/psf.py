#!/usr/bin/env python3
"""The diffraction image of a biconvex lens from ONE trace: the scene of examples/wavefront.py — 20,000 rays parallel to x within a
radius of 0.15 through BiConvexLens(R = +-5, thickness 0.4, n = 1.5), a monitor at x = 9.5 in the converging beam.  `psf_batch` sums
the plane wave of every hit over a grid of samples about a focus, on the device: the point-spread function, and from it the TRUE
Strehl ratio (the peak of the image against the image of the same rays all in phase), the MTF and the encircled energy — once
about the paraxial focus and once about the best focus `spots_all` finds.  Beside it the Marechal approximation
exp(-(2 pi rms / lambda)^2) from `wavefront_batch`: it holds for small aberrations only (at 0.05 wave of spherical aberration the
two agree to 1e-5, at 0.25 wave they differ by 2.7e-3) and says nothing about the shape of the image.
The rays fill the lens uniformly in POSITION, and behind this lens the direction cosine of a ray is all but proportional to its
height, so they sample the direction cosines uniformly too: the sum is the diffraction PSF (optable_amd/psf.py: the model).
    python examples/psf.py            (needs an MI355X and the built library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavefront import PUPIL, WL, X_MONITOR, scene  # noqa: E402  (examples/wavefront.py: the same lens, rays and monitor)

NA = 0.15 / 5.1  # the marginal ray's direction cosine behind the lens, to two digits: sets the scale of the grid, nothing else
AIRY = 0.61 * WL / NA


def main():
    table, monitor, segs, focus, pupil = scene()
    spot = table.spots_batch(monitor, segs, offsets=np.linspace(0.5, 1.1, 61))
    offset, _ = spot.best_focus()
    step = AIRY / 8
    print(f"20000 rays through a biconvex lens (R = +-5, n = 1.5); 129 x 129 samples {step:.3e} apart (an eighth of the Airy radius {AIRY:.3e})")
    print("                    x focus     hits   Strehl (true)   Strehl (peak)   Strehl (Marechal)")
    best = None
    for name, x in (("paraxial focus", focus[0]), ("best focus", X_MONITOR + offset)):
        psf = table.psf_batch(monitor, segs, WL, focus=(x, 0.0, 0.0), step=step, pixels=129)
        wf = table.wavefront_batch(monitor, segs, focus=(x, 0.0, 0.0), pupil=PUPIL)
        print(f"{name:>14}: {x:10.6f}  {int(psf.counts):7d}   Strehl {float(psf.strehl()):.6f}        {float(psf.strehl('peak')):.6f}        {float(wf.strehl(WL)):.6f}")
        best = psf
    mtf, fy, _ = best.mtf()
    cutoff = 2 * NA / WL
    row = mtf[:, mtf.shape[1] // 2]
    at = [int(np.argmin(np.abs(fy - f * cutoff))) for f in (0.25, 0.5, 0.75)]
    print(f"           MTF: at 0.25, 0.5, 0.75 of the cutoff 2 NA / lambda = {cutoff:.1f} cycles per unit along y, best focus: "
          + ", ".join(f"{row[k]:.3f}" for k in at))
    radii = np.array([0.5, 1.0, 2.0, 4.0]) * AIRY
    print("encircled energy: within 0.5, 1, 2, 4 Airy radii of the centroid, best focus: " + ", ".join(f"{e:.3f}" for e in best.encircled_energy(radii)))


if __name__ == "__main__":
    main()
