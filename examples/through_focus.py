#!/usr/bin/env python3
"""A through-focus scan from ONE trace: the scene of examples/beam_image.py — 20,000 rays parallel to x within a pupil of radius
0.02, through a thin lens of focal length 5 — with one monitor at x = 10.5 and 41 virtual planes displaced along its normal from
x = 9.5 to 11.5.  `spots_all` reduces the hits of every plane to its count, power, centroid and second moments on the device, with
no hit list and no image; `best_focus()` interpolates the variance, which is exactly quadratic in the offset.
    python examples/through_focus.py            (needs an MI355X and the built library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optable_amd import Lens, Monitor, OpticalTable  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

wl, w0, n = 780e-7, 0.05, 20_000
rng = np.random.default_rng(0)
r, phi = 0.02 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
origins = np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], axis=1)
batch = RayBatch.from_arrays(origins, np.tile([1.0, 0.0, 0.0], (n, 1)), wavelength=wl, intensity=1.0 / n, q=1j * np.pi * w0**2 / wl)

table = OpticalTable()
table.add_components([Lens([5, 0, 0], focal_length=5, radius=1.0)])
table.add_monitors([Monitor([10.5, 0, 0], 0.1, 0.1)])

segs = table.trace_batch(batch, max_segments=3)
offsets = np.linspace(-1.0, 1.0, 41)
spot = table.spots_all(segs, offsets=offsets)[0]
counts, _, _ = spot.to_host()
power, radius, centroid = spot.power().cpu().numpy(), spot.rms_radius().cpu().numpy(), spot.centroid().cpu().numpy()
print(f"{n} rays through f = 5; monitor 0.1 x 0.1 at x = 10.5, {len(offsets)} planes")
print("  offset        x     hits    power   rms radius   centroid y, z")
for j, off in enumerate(offsets):
    print(f"  {off:+6.2f}  {10.5 + off:7.2f}  {counts[j]:7d}  {power[j]:7.4f}  {radius[j]:11.4e}  {centroid[j, 0]:+.2e}, {centroid[j, 1]:+.2e}")
at, smallest = spot.best_focus()
print(f"best focus: offset {at:+.6f} (x = {10.5 + at:.6f}), rms radius {smallest:.3e}")
