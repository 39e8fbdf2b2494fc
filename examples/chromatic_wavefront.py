#!/usr/bin/env python3
"""The chromatic aberration of a singlet as WAVEFRONT ERROR, from ONE trace: the bundle of examples/chromatic_focus.py — 20,000
collimated rays within a pupil of radius 0.15, multiplexed in five wavelengths — through the same biconvex N-BK7 lens (R = +-5,
0.4 thick).  A monitor in the converging beam at x = 8 measures every wavelength's wavefront against the spherical wave that
converges on ONE point, F = (10.15, 0, 0): `wavefront_grouped_all` reduces the hits of every wavelength to its own 61 moments on
the device — the group of a hit is the wavelength of its input ray — and the host fits Zernike terms to each.  A focus that lies
delta beyond F shows as the defocus term (Noll 4) c4 = delta R^2 / (4 sqrt 3) in direction coordinates of pupil radius R, so the
column "focus from c4" can be read beside the offset of the smallest spot that `spots_grouped_all(...).best_focus()` finds on 41
planes about x = 10.15 from the same trace (the two differ by the spherical aberration, which moves the smallest spot).
    python examples/chromatic_wavefront.py            (needs an MI355X and the built library)"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optable_amd import BiConvexLens, Glass_NBK7, Monitor, OpticalTable  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

wavelengths = [400e-7, 486e-7, 560e-7, 656e-7, 780e-7]
w0, n, x_focus, x_pupil, R = 0.05, 20_000, 10.15, 8.0, 0.034
rng = np.random.default_rng(0)
r, phi = 0.15 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
origins = np.stack([np.zeros(n), r * np.cos(phi), r * np.sin(phi)], axis=1)
bundle = RayBatch.from_arrays(origins, np.tile([1.0, 0.0, 0.0], (n, 1)), wavelength=wavelengths[0], intensity=1.0 / n,
                              q=1j * np.pi * w0**2 / wavelengths[0])
batch = bundle.multiplexed_in_wavelength(wavelengths)

table = OpticalTable()
table.add_components([BiConvexLens([5, 0, 0], CT=0.4, R1=5.0, R2=-5.0, diameter=2.0, n=Glass_NBK7())])
in_beam, at_focus = Monitor([x_pupil, 0, 0], 1.0, 1.0), Monitor([x_focus, 0, 0], 1.0, 1.0)

segs = table.trace_batch(batch, max_segments=4)
ids, found = batch.groups_by_wavelength()
wf = table.wavefront_grouped_batch(in_beam, segs, ids, focus=(x_focus, 0.0, 0.0), pupil=(0.0, 0.0, R), labels=found.tolist())
spot = table.spots_grouped_batch(at_focus, segs, ids, offsets=np.linspace(-0.3, 0.3, 41), labels=found.tolist())
c = wf.coefficients().cpu().numpy()
rms, rms_focused, strehl = wf.rms(1).cpu().numpy(), wf.rms(4).cpu().numpy(), wf.strehl().cpu().numpy()
smallest_at, _ = spot.best_focus()
from_c4 = c[:, 3] * 4 * math.sqrt(3) / R**2
print(f"{n} rays x {len(wavelengths)} wavelengths through a biconvex N-BK7 lens; wavefront at x = {x_pupil} against the focus x = {x_focus}, one trace")
print("  wavelength   defocus c4 [waves]   rms [waves]   rms, tilt and defocus out   Strehl   focus from c4   smallest spot")
for g, wl in enumerate(wf.labels):
    print(f"  {wl * 1e7:7.0f} nm   {c[g, 3] / wl:+18.3f}   {rms[g] / wl:11.3f}   {rms_focused[g] / wl:25.3f}   {strehl[g]:6.4f}"
          f"   {x_focus + from_c4[g]:13.6f}   {x_focus + smallest_at[g]:13.6f}")
print("defocus monotone in the wavelength:", bool((np.diff(c[:, 3]) < 0).all() or (np.diff(c[:, 3]) > 0).all()))
print("hits inside the pupil per wavelength:", wf.counts.cpu().tolist(), "outside:", wf.outside.cpu().tolist())
