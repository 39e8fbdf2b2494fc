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


def spot_group_ids(groups, n_rays, n_groups=None, device=None):
    """`groups` as (the contiguous int32 device tensor the engine takes, G): an integer array or tensor of one id per input ray
    (`n_rays` of them; None: any length).  n_groups=None: max id + 1.  Ids outside 0 .. G - 1 are kept as they are — such rays are
    masked (-1 is the way to say so), which is why an `n_groups` below max id + 1 is no error.  ValueError: ids that are no
    integers, another length, an `n_groups` outside 1 .. 256."""
    import torch

    from .engine import SPOT_GROUPS_MAX

    if torch.is_tensor(groups):
        ids = groups
        if ids.dtype in (torch.bool,) or ids.is_floating_point() or ids.is_complex():
            raise ValueError(f"groups must be integer ids, not {ids.dtype}")
    else:
        try:
            array = np.asarray(groups)
        except (TypeError, ValueError):
            raise ValueError(f"groups must be integer ids, one per ray, not {groups!r}") from None
        if array.dtype.kind not in "iu":
            raise ValueError(f"groups must be integer ids, not {array.dtype}")
        if array.size and (array.min() < -(2**31) or array.max() >= 2**31):
            raise ValueError("groups: ids must fit 32 bits")
        ids = torch.from_numpy(np.ascontiguousarray(array.astype(np.int32, copy=False)))
    if ids.dim() != 1 or ids.numel() < 1 or (n_rays is not None and ids.numel() != int(n_rays)):
        raise ValueError(f"groups must be one id per input ray ({'any number' if n_rays is None else int(n_rays)}), not of shape {tuple(ids.shape)}")
    if n_groups is None:
        n_groups = max(int(ids.max()) + 1, 1)
    if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not 1 <= int(n_groups) <= SPOT_GROUPS_MAX:
        raise ValueError(f"n_groups must be 1 .. {SPOT_GROUPS_MAX}, not {n_groups!r}")
    ids = ids.to(dtype=torch.int32)
    if device is not None:
        ids = ids.to(device)
    return ids.contiguous(), int(n_groups)


class MonitorSpotGroups:
    """The hits of one monitor as moments, per plane and per RAY GROUP (`OpticalTable.spots_grouped_all`): `counts` (int64, J x G)
    and `sums` (float64, J x G x 6) are device tensors, `offsets`, `weight` and `centre` as for `MonitorSpots`; `n_groups` = G;
    `labels`: what the groups stand for, one per group (the wavelengths, say), or None.  A hit belongs to the group of the input
    ray its segment descends from; rays whose id is outside 0 .. G - 1 are in no group.  `group(g)` is a `MonitorSpots` on views
    of group g, so everything that class computes is there per group."""

    def __init__(self, monitor, offsets, counts, sums, weight, centre, labels=None, stack=None):
        self.monitor, self.offsets, self.counts, self.sums, self.weight = monitor, offsets, counts, sums, weight
        self.centre = (float(centre[0]), float(centre[1]))
        self.n_groups = int(counts.shape[-1])
        self.labels = None if labels is None else list(labels)
        if self.labels is not None and len(self.labels) != self.n_groups:
            raise ValueError(f"labels: one per group ({self.n_groups}), not {len(self.labels)}")
        self._stack = stack

    def group(self, g):
        """Group g as a `MonitorSpots` (views: an `into=` call that adds to this object shows there too)."""
        g = int(g)
        if not 0 <= g < self.n_groups:
            raise IndexError(f"group {g} of {self.n_groups}")
        return MonitorSpots(self.monitor, self.offsets, self.counts[:, g], self.sums[:, g], self.weight, self.centre)

    def total(self):
        """All groups together as a `MonitorSpots`: counts exactly, sums in the order of the groups (masked rays are in neither)."""
        return MonitorSpots(self.monitor, self.offsets, self.counts.sum(dim=1), self.sums.sum(dim=1), self.weight, self.centre)

    def _all(self):
        return MonitorSpots(self.monitor, self.offsets, self.counts, self.sums, self.weight, self.centre)

    def power(self):
        """W per plane and group (J x G)."""
        return self.sums[..., 0]

    def centroid(self):
        """(y, z) of the weighted centroid per plane and group, `centre` added back (J x G x 2)."""
        return self._all().centroid()

    def rms_radius(self):
        """sqrt(var_y + var_z) per plane and group (J x G), NaN where a cell has no hit."""
        return self._all().rms_radius()

    def best_focus(self):
        """`MonitorSpots.best_focus` of every group: (offsets, rms radii), two numpy arrays of length G."""
        found = [self.group(g).best_focus() for g in range(self.n_groups)]
        return np.array([f[0] for f in found]), np.array([f[1] for f in found])

    def to_host(self):
        """(counts, sums, offsets) as numpy arrays."""
        return self.counts.cpu().numpy(), self.sums.cpu().numpy(), self.offsets
