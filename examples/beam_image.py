#!/usr/bin/env python3
"""A focused Gaussian beam seen through-focus: 20,000 rays of waist 0.05, parallel to x within a pupil of radius 0.02, through a
thin lens of focal length 5, onto three monitors before, at and behind the focus.  `image_all` treats a ray as a point: at the
focus all of them fall into one or two bins.  `beam_all` spreads every hit over its spot size `Ray.spot_size(t)`, so the monitor
shows the irradiance the beams put on it.
    python examples/beam_image.py            (needs an MI355X and the built library)"""
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
table.add_monitors([Monitor([x, 0, 0], 0.1, 0.1) for x in (9.0, 10.0, 11.0)])

segs = table.trace_batch(batch, max_segments=3)
points = table.image_all(segs, bins=25)
beams = table.beam_all(segs, batch, bins=25)
print(f"{n} rays of waist {w0} through f = 5; monitors 0.1 x 0.1, 25 x 25 bins")
for hits, image, beam in zip(table.record_all(segs), points, beams):
    w = hits.spotsizeList(batch, None)
    power = beam.power.cpu().numpy()
    y = 0.5 * (beam.y_edges[1:] + beam.y_edges[:-1])
    width = 2 * np.sqrt((power.sum(axis=1) * y**2).sum() / power.sum())  # 2 sigma of the image along y: the 1 / e^2 radius of a Gaussian
    print(f"  x = {beam.monitor.origin[0]:4.1f}: spot size {float(w.mean()):.4f}; points in {int((image.counts > 0).sum()):3d} bins, "
          f"beams in {int((beam.power > 1e-6 * power.max()).sum()):3d}; power on the monitor {power.sum():.4f}, peak irradiance "
          f"{float(beam.irradiance().max()):9.1f}, 1 / e^2 radius of the image {width:.4f}")
