#!/usr/bin/env python3
"""The wavefront error of a biconvex lens from ONE trace: 20,000 rays parallel to x within a radius of 0.15 through
BiConvexLens(R = +-5, thickness 0.4, n = 1.5), a monitor at x = 9.5 in the converging beam.  `wavefront_all` reduces the optical
path of every hit against a spherical wave about a focus to 61 moments on the device, with no hit list; the host turns them into
Zernike coefficients, the rms wavefront error and the Strehl ratio — once about the paraxial focus, where spherical aberration
shows as defocus and a spherical term, and once about the best focus `spots_all` finds, where the defocus is balanced.
    python examples/wavefront.py            (needs an MI355X and the built library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optable_amd import BiConvexLens, Monitor, OpticalTable  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

WL, W0, N = 780e-7, 0.05, 20_000
CT, R1, R2, INDEX, X_LENS, X_MONITOR, PUPIL = 0.4, 5.0, -5.0, 1.5, 5.0, 9.5, (0.0, 0.0, 0.03)


def paraxial_focus():
    """x of the paraxial focus: the thick-lens focal length and its back focal distance behind the second vertex."""
    f = 1.0 / ((INDEX - 1) * (1 / R1 - 1 / R2 + (INDEX - 1) * CT / (INDEX * R1 * R2)))
    return X_LENS + CT + f * (1 - (INDEX - 1) * CT / (INDEX * R1))


def scene():
    """(table, monitor, traced segments, paraxial focus, pupil)."""
    rng = np.random.default_rng(0)
    r, phi = 0.15 * np.sqrt(rng.random(N)), rng.uniform(0, 2 * np.pi, N)
    origins = np.stack([np.zeros(N), r * np.cos(phi), r * np.sin(phi)], axis=1)
    batch = RayBatch.from_arrays(origins, np.tile([1.0, 0.0, 0.0], (N, 1)), wavelength=WL, intensity=1.0 / N, q=1j * np.pi * W0**2 / WL)
    table, monitor = OpticalTable(), Monitor([X_MONITOR, 0, 0], 0.2, 0.2)
    table.add_components([BiConvexLens([X_LENS, 0, 0], CT=CT, R1=R1, R2=R2, diameter=2.0, n=INDEX)])
    table.add_monitors([monitor])
    return table, monitor, table.trace_batch(batch, max_segments=4), (paraxial_focus(), 0.0, 0.0), PUPIL


def main():
    table, monitor, segs, focus, pupil = scene()
    spot = table.spots_batch(monitor, segs, offsets=np.linspace(0.5, 1.1, 61))
    offset, radius = spot.best_focus()
    print(f"{N} rays of radius 0.15 through a biconvex lens (R = +-5, n = 1.5); monitor at x = {X_MONITOR}, pupil radius {pupil[2]} in direction")
    print("                    x focus   inside  outside   rms W (piston out)   defocus (Noll 4)   spherical (Noll 11)   rms, 4 terms out    Strehl")
    for name, x in (("paraxial focus", focus[0]), ("best focus", X_MONITOR + offset)):
        wf = table.wavefront_batch(monitor, segs, focus=(x, 0.0, 0.0), pupil=pupil)
        c = wf.coefficients()
        inside, outside, _ = wf.to_host()
        print(f"{name:>14}: {x:10.6f}  {inside:7d}  {outside:7d}   {float(wf.rms()):.6e}         {float(c[3]):+.6e}      {float(c[10]):+.6e}         "
              f"{float(wf.rms(4)):.6e}    {float(wf.strehl(WL)):.4f}")
    print(f"(the smallest spot, rms radius {radius:.3e}, lies {focus[0] - X_MONITOR - offset:+.4f} before the paraxial focus)")


if __name__ == "__main__":
    main()
