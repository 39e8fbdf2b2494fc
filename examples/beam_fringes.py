#!/usr/bin/env python3
"""A Mach-Zehnder interferometer traced with two Gaussian rays — ONE input ray of waist 0.1 that the first 50 % splitter turns into
the two arms — and a slightly tilted mirror in one arm.  Both arms reach the monitor behind the second splitter; `wave_batch` sums
their two Gaussian beams coherently (envelope, wavefront curvature, tilt and the model's phase, sampled at the bin centres), so the
monitor shows the fringes of an interferometer: their period is lambda / (2 sin theta) for beams at +-theta, here lambda / sin(delta)
for one beam square on the monitor and one tilted by delta.  `beam_batch` adds the powers of the same two beams: a flat spot, whatever
the tilt.  `field_all` would light two bins.
    python examples/beam_fringes.py            (needs an MI355X and the built library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optable_amd import BeamSplitter, Monitor, OpticalTable, SquareMirror  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

wl, w0, delta = 780e-7, 0.1, 1.6e-3  # the tilted arm leaves its mirror delta off the other arm's direction
batch = RayBatch.from_arrays(np.array([[0.0, 2.0, 0.0]]), np.array([[0.0, -1.0, 0.0]]), wavelength=wl, q=1j * np.pi * w0**2 / wl)

table = OpticalTable()
table.add_components([BeamSplitter([0, 0, 0], width=2, height=2, eta=0.5).RotZ(np.pi / 4),            # reflects to +x, transmits to -y
                      SquareMirror([3, 0, 0], width=2, height=2).RotZ(5 * np.pi / 4 + delta / 2),  # +x -> -y, tilted by delta / 2
                      SquareMirror([0, -3, 0], width=2, height=2).RotZ(np.pi / 4),                  # -y -> +x
                      BeamSplitter([3, -3, 0], width=2, height=2, eta=0.5).RotZ(np.pi / 4)])        # the arms meet again
mon = Monitor([5, -3, 0], 0.5, 0.5)  # the +x port
table.add_monitors([mon])

segs = table.trace_batch(batch, max_segments=12)  # a tree of 1 + 2 + 4 rays, 9 segments
hits = table.record_all(segs)[0]
ty = hits.tYList(None).cpu().numpy()
print(f"{len(hits)} beams on the monitor: tilts {ty}, spot sizes {hits.spotsizeList(batch, None).cpu().numpy()}, "
      f"radii of curvature {hits.radiusList(None).cpu().numpy()}")
theta = 0.5 * abs(ty[0] - ty[1])  # +-theta about their bisector (to first order in the tilt)

bins = (256, 5)
wave = table.wave_batch(mon, segs, batch, bins=bins)
beam = table.beam_batch(mon, segs, batch, bins=bins)
y = 0.5 * (wave.y_edges[1:] + wave.y_edges[:-1])
row = wave.irradiance().cpu().numpy()[:, bins[1] // 2]
flat = beam.irradiance().cpu().numpy()[:, bins[1] // 2]

# the fringe period: the strongest line of the row's spectrum (zero-padded 16 x, the envelope's own line at 0 left out)
spectrum = np.abs(np.fft.rfft((row - row.mean()) * np.hanning(len(row)), 16 * len(row)))
freq = np.fft.rfftfreq(16 * len(row), y[1] - y[0])
lowest = np.searchsorted(freq, 4 / (y[-1] - y[0]))
period = 1 / freq[lowest + np.argmax(spectrum[lowest:])]


def depth(v):
    """(max - min) / (max + min) over the central fifth of the row: 1 for full fringes, 0 for a flat top."""
    mid = v[2 * len(v) // 5:3 * len(v) // 5]
    return (mid.max() - mid.min()) / (mid.max() + mid.min())


print(f"aliased hits: {wave.aliased} (bin {y[1] - y[0]:.4g}, fringe period {period:.4g}: {period / (y[1] - y[0]):.1f} bins a fringe)")
print(f"fringe period from wave_batch: {period:.6g}    lambda / (2 sin theta): {wl / (2 * np.sin(theta)):.6g}    (theta = {theta:.6g})")
print(f"modulation depth at the centre: wave_batch {depth(row):.4f}, beam_batch {depth(flat):.4f} (no fringes, only the envelope: it adds powers)")
print(f"power on the monitor: wave_batch {float(wave.power().sum()):.5f}, beam_batch {float(beam.power.sum()):.5f}, "
      f"the two hits carry {float(hits.IList(None).sum()):.5f}")
