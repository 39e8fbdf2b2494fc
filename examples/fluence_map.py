#!/usr/bin/env python3
"""Where the light went: the fluence map of a traced batch — `OpticalTable.render(type="Z", roi=...)` as numbers.  cfg 2 of the
benchmarks: a point source at the focus of a thin lens (f = 5 at x = 5), a cone of half-angle 0.15, collimated by the lens and sent
back by the mirror pair at x = 10.  Every pixel of the (x, y) view holds the intensity-weighted path length of the segments inside
it: the cone opening from the focus at the origin, the collimated beam behind the lens, the returning beam on top of it.
    python examples/fluence_map.py [rays]        (needs an MI355X and the built library)
Saves fluence_map.png when matplotlib imports, fluence_map.npy (the fluence channel) otherwise."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optable_amd as oa  # noqa: E402
from optable_amd import workloads as W  # noqa: E402
from optable_amd.batch import RayBatch  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
table = oa.OpticalTable()
table.add_components(W.cfg2_components(oa))
batch = RayBatch.from_arrays(*W.cfg2_rays(n, 0), wavelength=W.WL, intensity=1.0 / n, q=1j * np.pi * W.W0**2 / W.WL)
segs = table.trace_batch(batch, max_segments=5)

roi = (-1.0, 12.0, -2.0, 2.0, -np.inf, np.inf)  # x and y of the image; all depths
fm = table.fluence_map(segs, view="Z", roi=roi, pixels=(520, 160))
counts, fluence, x_edges, y_edges = fm.to_host()
print(f"{n} rays, {int(segs.count.abs().sum())} segments -> {int(counts.sum())} pieces in {fm.pixels[0]} x {fm.pixels[1]} pixels; {fm.skipped} segments skipped")
x = 0.5 * (x_edges[1:] + x_edges[:-1])
lit = (fluence > 1e-3 * fluence.max()).sum(axis=1) * (y_edges[1] - y_edges[0])  # height of the lit region, column by column
for at in (0.0, 1.0, 2.5, 4.9, 7.5):
    k = int(np.argmin(np.abs(x - at)))
    print(f"  x = {x[k]:5.2f}: the beam is {lit[k]:.3f} high, peak fluence {fluence[k].max():.4g}")
try:
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    fig, ax = plt.subplots(figsize=(10, 3.5))
    shown = ax.imshow(np.log10(np.maximum(fluence.T, 1e-6 * fluence.max())), origin="lower", extent=fm.extent, aspect="auto", cmap="magma")
    fig.colorbar(shown, ax=ax, label="log10 fluence")
    ax.set_xlabel("X"), ax.set_ylabel("Y")
    fig.savefig("fluence_map.png", dpi=150, bbox_inches="tight")
    print("wrote fluence_map.png")
except ImportError:
    np.save("fluence_map.npy", fluence)
    print("wrote fluence_map.npy")
