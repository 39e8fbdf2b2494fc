#!/usr/bin/env python3
"""The chromatic focal shift of a singlet from ONE trace: a collimated bundle of 20,000 rays within a pupil of radius 0.15,
multiplexed in five wavelengths (`RayBatch.multiplexed_in_wavelength`: 100,000 rays), through a biconvex N-BK7 lens (R = +-5,
0.4 thick), with one monitor at x = 10.15 and 41 virtual planes displaced along its normal from x = 9.85 to 10.45.
`spots_grouped_all` reduces the hits of every (plane, wavelength) to a count, the power, the centroid and the second moments on
the device — the group of a hit is the wavelength of its input ray (`RayBatch.groups_by_wavelength`) — and `best_focus()` gives the
plane of the smallest spot per wavelength: blue focuses short, red long.
    python examples/chromatic_focus.py            (needs an MI355X and the built library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optable_amd import BiConvexLens, Glass_NBK7, Monitor, OpticalTable  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

wavelengths = [400e-7, 486e-7, 560e-7, 656e-7, 780e-7]
w0, n, x_mon = 0.05, 20_000, 10.15
rng = np.random.default_rng(0)
r, phi = 0.15 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
origins = np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], axis=1)
bundle = RayBatch.from_arrays(origins, np.tile([1.0, 0.0, 0.0], (n, 1)), wavelength=wavelengths[0], intensity=1.0 / n,
                              q=1j * np.pi * w0**2 / wavelengths[0])
batch = bundle.multiplexed_in_wavelength(wavelengths)

table = OpticalTable()
table.add_components([BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n=Glass_NBK7())])
table.add_monitors([Monitor([x_mon, 0, 0], 1.0, 1.0)])

segs = table.trace_batch(batch, max_segments=4)
ids, found = batch.groups_by_wavelength()
offsets = np.linspace(-0.3, 0.3, 41)
spot = table.spots_grouped_all(segs, ids, offsets=offsets, labels=found.tolist())[0]
at, smallest = spot.best_focus()
power = spot.power().cpu().numpy()
print(f"{n} rays x {len(wavelengths)} wavelengths through a biconvex N-BK7 lens; monitor at x = {x_mon}, {len(offsets)} planes, one trace")
print("  wavelength   best focus x   shift from the first   rms radius    power")
for g, wl in enumerate(spot.labels):
    print(f"  {wl * 1e7:7.0f} nm   {x_mon + at[g]:12.6f}   {at[g] - at[0]:+20.6f}   {smallest[g]:10.3e}  {power[len(offsets) // 2, g]:7.4f}")
print("chromatic focal shift, longest against shortest wavelength:", f"{at[-1] - at[0]:+.6f}")
print("monotone in the wavelength:", bool((np.diff(at) > 0).all()))
white = spot.total()
print(f"all wavelengths together: best focus x = {x_mon + white.best_focus()[0]:.6f}, rms radius {white.best_focus()[1]:.3e}")
