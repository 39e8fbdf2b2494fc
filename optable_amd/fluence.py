"""Fluence maps: a SegmentBatch rasterised into a projected view of the table on the device (`OpticalTable.fluence_map`).

The view is the reference's `OpticalTable.render(type="Z" | "X" | "Y", roi=...)`: the image axes (u, v) are the lab axes
`VIEW_AXES[view]` (ray.py:255 `dimension_dict`), the remaining axis is the depth, and `roi = (x0, x1, y0, y1, z0, z1)` gives
the range of every lab axis (optical_table.py:198-206).  Where `render` draws a line per `Ray`, a fluence map holds, per pixel,
the number of segment pieces inside it and their intensity-weighted path length.
"""
import numpy as np

from .monitors import WEIGHTS, image_bins  # noqa: F401  (WEIGHTS: importable from here too)

VIEW_AXES = {"Z": (0, 1, 2), "X": (1, 2, 0), "Y": (2, 0, 1)}  # view -> lab axes of (u, v, depth)


def fluence_view(view, roi, pixels):
    """The arguments of a fluence map, checked and in the engine's terms: (axes [3, 3], u_edges, v_edges, (w_lo, w_hi), roi as
    a tuple of six floats).  ValueError for a view other than "Z" / "X" / "Y", a roi that is not six numbers with finite,
    increasing image ranges and an ordered depth range (whose bounds may be infinite), or `pixels` that `image_bins` refuses."""
    if not isinstance(view, str) or view not in VIEW_AXES:
        raise ValueError(f'view must be "Z", "X" or "Y", not {view!r}')
    nu, nv = image_bins(pixels)
    try:
        roi = tuple(float(r) for r in roi)
    except (TypeError, ValueError):
        raise ValueError(f"roi must be (x0, x1, y0, y1, z0, z1), not {roi!r}") from None
    if len(roi) != 6:
        raise ValueError(f"roi must be (x0, x1, y0, y1, z0, z1), not {roi!r}")
    iu, iv, iw = VIEW_AXES[view]
    (u_lo, u_hi), (v_lo, v_hi), (w_lo, w_hi) = (roi[2 * k:2 * k + 2] for k in (iu, iv, iw))
    if not (np.isfinite([u_lo, u_hi, v_lo, v_hi]).all() and u_lo < u_hi and v_lo < v_hi):
        raise ValueError(f"roi: the ranges of the image axes of view {view!r} must be finite and increasing, not {roi!r}")
    if not w_lo <= w_hi:  # (a NaN too)
        raise ValueError(f"roi: the depth range of view {view!r} must be ordered, not {roi!r}")
    u_edges, v_edges = np.linspace(u_lo, u_hi, nu + 1), np.linspace(v_lo, v_hi, nv + 1)
    if not ((np.diff(u_edges) > 0).all() and (np.diff(v_edges) > 0).all()):
        raise ValueError(f"roi: {pixels!r} pixels do not resolve {roi!r} in double precision")
    return np.eye(3)[[iu, iv, iw]], u_edges, v_edges, (w_lo, w_hi), roi


class FluenceMap:
    """A SegmentBatch as an image of a projected view (`OpticalTable.fluence_map`): `counts` (int64) and `fluence` (float64),
    [nu, nv] device tensors over `u_edges` x `v_edges` (numpy) — per pixel the number of segment pieces of positive length inside
    it and the sum of intensity x length over them (`weight="none"`: the plain path length).  `skipped`: segments that deposited
    nothing because they hold a NaN, have no direction, or run on without end inside the box.  Counts are exact and the same
    every run; the fluence is atomic fp64 adds whose last bits depend on the order of arrival."""

    def __init__(self, view, roi, weight, counts, fluence, skipped, u_edges, v_edges):
        self.view, self.roi, self.weight, self.counts, self.fluence, self.u_edges, self.v_edges = view, roi, weight, counts, fluence, u_edges, v_edges
        self._skipped = skipped  # a one-element device tensor, which `into=` adds to: read when asked for

    @property
    def pixels(self):
        return tuple(self.counts.shape)

    @property
    def skipped(self):
        return int(self._skipped.item())

    @property
    def extent(self):
        """(u_lo, u_hi, v_lo, v_hi): plt.imshow(fm.to_host()[1].T, origin="lower", extent=fm.extent)."""
        return (float(self.u_edges[0]), float(self.u_edges[-1]), float(self.v_edges[0]), float(self.v_edges[-1]))

    def to_host(self):
        """(counts, fluence, u_edges, v_edges) as numpy arrays."""
        return self.counts.cpu().numpy(), self.fluence.cpu().numpy(), self.u_edges, self.v_edges
