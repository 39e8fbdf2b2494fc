"""Spot statistics: the moments of a monitor's hits on the monitor and on a stack of planes displaced along its normal
(`OpticalTable.spots_all` / `spots_batch`), summed on the device with no hit list and no image (ot_monitor_spots_many).

What the reference computes hit by hit on a `Monitor` — `sum_intensity`, `avg_intensity`, the `Std(...)` annotations of
`render_scatter`, and by search in `calibrate_symmetric_4f` the plane of best focus — as small expressions on J-sized tensors.
"""
import numpy as np

from .monitors import WEIGHTS  # noqa: F401  (importable from here too)

SUMS = ("W", "Wy", "Wz", "Wyy", "Wzz", "Wyz")


def spot_offsets(offsets):
    """`offsets` as the float64 vector the engine takes: one or more finite numbers (a scalar is one plane).  ValueError else."""
    try:
        offsets = np.atleast_1d(np.asarray(offsets, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"offsets must be finite numbers, not {offsets!r}") from None
    if offsets.ndim != 1 or len(offsets) < 1 or not np.isfinite(offsets).all():
        raise ValueError(f"offsets must be one or more finite numbers, not {offsets!r}")
    return np.ascontiguousarray(offsets)


def spot_centres(centre, n_monitors):
    """`centre` as the [n_monitors, 2] float64 table the engine takes: None (0, 0), one (y, z) for all, or one per monitor."""
    if centre is None:
        return np.zeros((n_monitors, 2))
    try:
        centre = np.asarray(centre, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"centre must be None, one (y, z) or one (y, z) per monitor, not {centre!r}") from None
    if centre.shape == (2,):
        centre = np.tile(centre, (n_monitors, 1))
    if centre.shape != (n_monitors, 2) or not np.isfinite(centre).all():
        raise ValueError(f"centre must be None, one finite (y, z) or one per monitor ({n_monitors}), not {centre!r}")
    return np.ascontiguousarray(centre)


class MonitorSpots:
    """The hits of one monitor as moments, per plane (`OpticalTable.spots_all`): `offsets` (numpy, J) — plane j is the monitor
    moved by offsets[j] along its normal; `counts` (int64, J) and `sums` (float64, J x 6: W, Wy, Wz, Wyy, Wzz, Wyz of the hits'
    weights w and coordinates y, z relative to `centre`) are device tensors.  `weight`: "intensity" or "none" (w = 1); `centre`:
    the (c_y, c_z) subtracted from the coordinates before they were summed.  Counts are exact; the sums are the same bits every
    run.  Every method is per plane, NaN where a plane has no hit."""

    def __init__(self, monitor, offsets, counts, sums, weight, centre, stack=None):
        self.monitor, self.offsets, self.counts, self.sums, self.weight = monitor, offsets, counts, sums, weight
        self.centre = (float(centre[0]), float(centre[1]))
        self._stack = stack  # (counts, sums of the whole call, this monitor's place in it): what `into=` adds to

    def _moments(self):
        import torch

        W, Wy, Wz, Wyy, Wzz, Wyz = self.sums.unbind(-1)
        nan = torch.full_like(W, float("nan"))
        some = self.counts > 0
        my, mz = torch.where(some, Wy / W, nan), torch.where(some, Wz / W, nan)
        return some, nan, my, mz, Wyy / W - my * my, Wzz / W - mz * mz, Wyz / W - my * mz

    def power(self):
        """W, the summed weight of the hits (J)."""
        return self.sums[..., 0]

    def centroid(self):
        """(y, z) of the weighted centroid, `centre` added back (J x 2)."""
        import torch

        _, _, my, mz, *_ = self._moments()
        return torch.stack([my + self.centre[0], mz + self.centre[1]], dim=-1)

    def covariance(self):
        """The weighted covariance of (y, z) (J x 2 x 2); variances that rounding left a hair below zero are 0."""
        import torch

        some, nan, _, _, vy, vz, cyz = self._moments()
        vy, vz, cyz = torch.where(some, vy.clamp_min(0.0), nan), torch.where(some, vz.clamp_min(0.0), nan), torch.where(some, cyz, nan)
        return torch.stack([torch.stack([vy, cyz], dim=-1), torch.stack([cyz, vz], dim=-1)], dim=-2)

    def rms_y(self):
        return self.covariance()[..., 0, 0].sqrt()

    def rms_z(self):
        return self.covariance()[..., 1, 1].sqrt()

    def rms_radius(self):
        """sqrt(var_y + var_z) (J)."""
        cov = self.covariance()
        return (cov[..., 0, 0] + cov[..., 1, 1]).sqrt()

    def best_focus(self):
        """(offset, rms_radius) of the smallest spot.  var_r = var_y + var_z is minimised over the planes with at least two hits;
        where the smallest lies inside the scan and both its neighbours qualify, the vertex of the parabola through the three
        (offset, var_r) is returned — var_r is exactly quadratic in the offset for a bundle whose rays reach all three planes, so
        the vertex is exact there, which is why the variance is interpolated and not the radius; else the sampled minimum.
        (nan, nan) when no plane qualifies.  The offsets must be strictly increasing: ValueError otherwise."""
        x = np.asarray(self.offsets, dtype=np.float64)
        if len(x) > 1 and not (np.diff(x) > 0).all():
            raise ValueError("best_focus needs sorted, distinct offsets")
        cov = self.covariance().cpu().numpy()
        var = cov[:, 0, 0] + cov[:, 1, 1]
        ok = (self.counts.cpu().numpy() >= 2) & np.isfinite(var)
        if not ok.any():
            return float("nan"), float("nan")
        i = int(np.argmin(np.where(ok, var, np.inf)))
        if 0 < i < len(x) - 1 and ok[i - 1] and ok[i + 1]:
            u0, u2 = x[i - 1] - x[i], x[i + 1] - x[i]
            s0, s2 = (var[i - 1] - var[i]) / u0, (var[i + 1] - var[i]) / u2
            a = (s2 - s0) / (u2 - u0)
            b = s2 - a * u2
            if a > 0.0:
                return float(x[i] - b / (2.0 * a)), float(np.sqrt(max(var[i] - b * b / (4.0 * a), 0.0)))
        return float(x[i]), float(np.sqrt(var[i]))

    def to_host(self):
        """(counts, sums, offsets) as numpy arrays."""
        return self.counts.cpu().numpy(), self.sums.cpu().numpy(), self.offsets
