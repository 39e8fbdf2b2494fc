"""Rectangular recorder plane (reference: optable/monitor.py).

`record` is the step right after the trace inside `_single_ray_tracing`
(optical_table.py:145-146): every finished segment is intersected with the monitor's
rectangle, honouring the segment's length (monitor.py:183-193).  On the MI355X path the
intersection pass runs on the device over the trace's segment stream
(`ot_monitor_record_f64`); this class keeps the reference's accessors on top of the hits.
Plots are out of scope.
"""
import numpy as np

from .components import OpticalComponent
from .shapes import Rectangle


class Monitor(OpticalComponent):
    def __init__(self, origin, width, height, **kwargs):
        super().__init__(origin, **kwargs)
        self.width, self.height = width, height
        self.surface = Rectangle(width, height)
        self._edge_color = "orange"
        self._initialize()

    def _initialize(self):
        self._data_raw = []  # (P_local, intensity, t, ray)
        self._sorted_data = []
        self._updated = False
        self._sort_method = None

    def clear(self):
        self._initialize()

    def get_bbox(self):
        return OpticalComponent.get_bbox(self)

    # -- recording -------------------------------------------------------------------------
    def record(self, rays):
        """Record a list of finished `Ray` segments (device pass via the engine)."""
        from .table import record_monitor_hits

        record_monitor_hits(self, rays)

    def _extend(self, hits):
        self._data_raw.extend(hits)
        self._updated = True

    # -- accessors (monitor.py:24-156) -----------------------------------------------------
    @property
    def ndata(self):
        return len(self._data_raw)

    @property
    def raw_yList(self):
        return np.array([d[0][1] for d in self._data_raw])

    @property
    def raw_zList(self):
        return np.array([d[0][2] for d in self._data_raw])

    @property
    def sortYZIndex(self):
        return np.lexsort((self.raw_zList, self.raw_yList))

    @property
    def sortIDindex(self):
        return np.argsort([d[3]._id for d in self._data_raw])

    def get_data(self, sort="YZ"):
        if (not self._sorted_data) or self._updated or self._sort_method != sort:
            order = {"YZ": lambda: self.sortYZIndex, "ID": lambda: self.sortIDindex}.get(sort)
            if order is not None:
                self._sort_method = sort
                self._sorted_data = [self._data_raw[i] for i in order()]
            self._updated = False
        return self._sorted_data

    data = property(lambda self: self.get_data())

    def _column(self, pick, sort):
        if self.ndata == 0:
            return np.array([])
        return np.array([pick(d) for d in self.get_data(sort=sort)])

    def get_rays(self, sort="YZ"):
        return [] if self.ndata == 0 else [d[3] for d in self.get_data(sort=sort)]

    def get_PList(self, sort="YZ"):
        return self._column(lambda d: d[0], sort)

    def get_yList(self, sort="YZ"):
        axis = self.tangent_Y
        return self._column(lambda d: np.dot(d[0], axis), sort)

    def get_zList(self, sort="YZ"):
        axis = self.tangent_Z
        return self._column(lambda d: np.dot(d[0], axis), sort)

    def get_IList(self, sort="YZ"):
        return self._column(lambda d: d[1], sort)

    def get_tList(self, sort="YZ"):
        return self._column(lambda d: d[2], sort)

    def get_directionList(self, sort="YZ"):
        return self._column(lambda d: d[3].direction, sort)

    def get_tYList(self, sort="YZ"):
        return np.dot(self.get_directionList(sort=sort), self.tangent_Y)

    def get_tZList(self, sort="YZ"):
        return np.dot(self.get_directionList(sort=sort), self.tangent_Z)

    rays = property(lambda self: self.get_rays())
    PList = property(lambda self: self.get_PList())
    yList = property(lambda self: self.get_yList())
    zList = property(lambda self: self.get_zList())
    IList = property(lambda self: self.get_IList())
    tList = property(lambda self: self.get_tList())
    directionList = property(lambda self: self.get_directionList())
    tYList = property(lambda self: self.get_tYList())
    tZList = property(lambda self: self.get_tZList())

    def get_ray_i(self, idx):
        return self.rays[idx], [self.yList[idx], self.zList[idx], self.tYList[idx], self.tZList[idx], self.IList[idx]]

    def get_ray_id(self, ray_id):
        for idx, r in enumerate(self.rays):
            if r._id == ray_id:
                return self.get_ray_i(idx)
        return None, None

    def get_waist_distance(self):
        out = []
        for r, t in zip(self.rays, self.tList):
            z = r.distance_to_waist(r.q_at_z(t))
            out.append(-z if np.dot(r.direction, self.normal) > 0 else z)
        return np.array(out)

    def get_beam_waist(self):
        """Gaussian waist of every recorded ray at the monitor (monitor.py:218-225; upstream reads an undefined
        `self.rList` there — `self.rays` is what the loop needs)."""
        return np.array([r.waist(r.q_at_z(t)) for r, t in zip(self.rays, self.tList)])

    def get_delta_pos(self):
        """Spacings of the hits sorted by y (monitor.py:227-238)."""
        y, z = self.yList, self.zList
        if len(y) == 0 or len(z) == 0:
            return np.array([0.0]), np.array([0.0])
        order = np.argsort(y)
        return np.diff(y[order]), np.diff(z[order])

    def _get_hist_y(self):
        return np.histogram(self.yList, bins=30, range=(-self.width / 2, self.width / 2))

    @property
    def std_histy(self):
        """Standard deviation of the 30-bin y histogram (monitor.py:248-253)."""
        counts, bins = self._get_hist_y()
        mean = np.sum(counts * bins[:-1]) / np.sum(counts)
        return np.sqrt(np.sum(counts * bins[:-1] ** 2) / np.sum(counts) - mean**2)

    @property
    def sum_intensity(self):
        return np.sum([d[1] for d in self.get_data()])

    @property
    def avg_intensity(self):
        return np.mean([d[1] for d in self.get_data()])

    def export_rays_npz(self, filename: str):
        print(f"Exporting {self.ndata} rays to {filename} ...")
        np.savez(filename, xList=self.yList, yList=self.zList, tXList=self.tYList, tYList=self.tZList, IList=self.IList)


class MonitorHits:
    """`Monitor.record` results for a SegmentBatch, kept on the device (no Python objects).

    Mirrors the accessors of `Monitor` (monitor.py:33-156): `yList/zList` are the local hit point
    projected on the monitor's LAB tangents (as upstream does), `tYList/tZList` the same projections
    of the segment directions, `IList` the intensities, `tList` the distances.  `sort="YZ"` orders by
    local y then z (np.lexsort((z, y))), `sort="ID"` by input-ray index, `sort=None` keeps
    reference order (input-ray-major, then segment order)."""

    def __init__(self, monitor, segs, slot, P, t):
        import torch

        self.monitor, self.segs = monitor, segs
        ray = self._gather(segs.ray, slot).long()
        if segs.layout == "slots":  # [k][ray] slots: reference order is ray-major, then k
            order = torch.argsort(ray * (segs.capacity // max(segs.n_rays, 1)) + slot // max(segs.n_rays, 1))
        else:
            order = torch.argsort(ray, stable=True)
        self.slot, self.P, self.t, self.ray = slot[order], P[order], t[order], ray[order]

    def __len__(self):
        return int(self.slot.numel())

    @staticmethod
    def _gather(field, slot):
        """`field` at the slots `slot`: the fields of a tiled batch are strided [tiles, 64] views (read in place), all others 1-D."""
        return field[slot // 64, slot % 64] if field.dim() == 2 else field[slot]

    def _order(self, sort):
        import torch

        if sort is None:
            return torch.arange(len(self), device=self.slot.device)
        if sort == "ID":
            return torch.argsort(self.ray, stable=True)
        if sort == "YZ":
            by_z = torch.argsort(self.P[:, 2], stable=True)
            return by_z[torch.argsort(self.P[by_z, 1], stable=True)]
        raise ValueError(f"unknown sort {sort!r}")

    def _axis(self, which):
        import torch

        vec = self.monitor.tangent_Y if which == "Y" else self.monitor.tangent_Z
        return torch.as_tensor(np.asarray(vec, dtype=float), device=self.slot.device)

    def PList(self, sort="YZ"):
        return self.P[self._order(sort)]

    def yList(self, sort="YZ"):
        return self.P[self._order(sort)] @ self._axis("Y")

    def zList(self, sort="YZ"):
        return self.P[self._order(sort)] @ self._axis("Z")

    def tList(self, sort="YZ"):
        return self.t[self._order(sort)]

    def IList(self, sort="YZ"):
        return self._gather(self.segs.intensity, self.slot[self._order(sort)])

    def ray_index(self, sort="YZ"):
        return self.ray[self._order(sort)]

    def pathlengthList(self, sort="YZ"):
        """The optical path length of every hit, `Ray.pathlength(t)` of its segment: pathlength[slot] + t * n[slot]."""
        order = self._order(sort)
        s = self.slot[order]
        return self._gather(self.segs.pathlength, s) + self.t[order] * self._gather(self.segs.n_index, s)

    def wavefrontList(self, focus=None, direction=None, sort="YZ"):
        """The optical path W of every hit against an ideal wave, hit by hit — what `OpticalTable.wavefront_all` reduces: exactly
        one of `focus` (a lab point F: W = L + n ((F_loc - P) . d), the path at the foot of the perpendicular from F onto the ray)
        or `direction` (a lab vector u, made unit: W = L - n (P . u_loc)), with L = `pathlengthList`, P the local hit point and d
        the renormalised local direction of the segment (double)."""
        import torch

        from .wavefront import hit_wavefront, local_frame, wavefront_reference

        kind, _, local = wavefront_reference(focus, direction, [self.monitor])
        order = self._order(sort)
        s = self.slot[order]
        M = torch.as_tensor(local_frame(self.monitor)[0], device=self.slot.device)
        d = self.directionList(sort).double() @ M  # rows: M^T D
        d = d * (1.0 / torch.sqrt((d * d).sum(dim=1)))[:, None]
        return hit_wavefront(kind, local[0].tolist(), self.P[order].double(), self.t[order].double(), d, self._gather(self.segs.n_index, s).double(),
                             self._gather(self.segs.pathlength, s).double())

    def phaseList(self, wavelength, sort="YZ"):
        """The phase of every hit in [0, 2 pi), `Ray.phase(t)` of its segment: 2 pi (x - floor x) with x = pathlengthList / wavelength
        cycles.  `wavelength`: a float for all rays, or the `RayBatch` that was traced (its wavelengths, as double, by the hits'
        `ray_index`).  What `OpticalTable.field_all` sums per bin, as a list."""
        import torch

        if hasattr(wavelength, "wavelength"):
            wavelength = wavelength.wavelength.double()[self.ray_index(sort)]
        x = self.pathlengthList(sort).double() / wavelength
        return 2 * np.pi * (x - torch.floor(x))

    def _wavelengths(self, wavelength, sort):
        """`wavelength` per hit: a float for all rays as it is, the `RayBatch` that was traced by the hits' `ray_index`, as double."""
        return wavelength.wavelength.double()[self.ray_index(sort)] if hasattr(wavelength, "wavelength") else wavelength

    def qList(self, sort="YZ"):
        """The complex beam parameter of every hit at the monitor, `Ray.q_at_z(t)` of its segment: q[slot] + t (complex128)."""
        import torch

        order = self._order(sort)
        s = self.slot[order]
        return torch.complex(self._gather(self.segs.q_re, s).double() + self.t[order], self._gather(self.segs.q_im, s).double())

    def spotsizeList(self, wavelength, sort="YZ"):
        """The 1 / e^2 radius of every hit's beam at the monitor, `Ray.spot_size(t)` of its segment: sqrt(-wavelength / (n pi
        Im(1 / q))) with q = `qList`, written without the reciprocal — the w over which `OpticalTable.beam_all` spreads the hit.
        `wavelength` as for `phaseList`.  NaN or inf where the segment carries no q."""
        import torch

        q = self.qList(sort)
        n = self._gather(self.segs.n_index, self.slot[self._order(sort)]).double()
        return torch.sqrt(self._wavelengths(wavelength, sort) * (q.real**2 + q.imag**2) / (n * np.pi * q.imag))

    def waistList(self, wavelength, sort="YZ"):
        """The waist radius of every hit's beam, `Monitor.get_beam_waist`: `Ray.waist(q)` = sqrt(wavelength Im(q) / (n pi))."""
        import torch

        n = self._gather(self.segs.n_index, self.slot[self._order(sort)]).double()
        return torch.sqrt(self._wavelengths(wavelength, sort) * self.qList(sort).imag / (n * np.pi))

    def waistdistanceList(self, sort="YZ"):
        """The distance of every hit from its beam's waist, `Monitor.get_waist_distance`: Re(q) at the monitor, with the sign
        turned for rays that travel along the monitor's normal (direction . normal > 0)."""
        import torch

        along = self.directionList(sort).double() @ torch.as_tensor(np.asarray(self.monitor.normal, dtype=float), device=self.slot.device)
        z = self.qList(sort).real
        return torch.where(along > 0, -z, z)

    def radiusList(self, sort="YZ"):
        """The radius of curvature of every hit's wavefront at the monitor, `Ray.radius_of_curvature(q)` = |q|^2 / Re(q) with q =
        `qList` (inf at a waist, negative before it): the R of the curvature phase k r^2 / (2 R) in `OpticalTable.wave_all`."""
        q = self.qList(sort)
        return (q.real**2 + q.imag**2) / q.real

    def gouyList(self, sort="YZ"):
        """The Gouy phase of every hit's beam at the monitor, atan2(Re(q), Im(q)) with q = `qList`: what `wave_all(gouy=True)`
        subtracts from the phase.  The tracer's q does not accumulate it across lenses: exact only for a beam that has met no
        focusing element since its waist."""
        import torch

        q = self.qList(sort)
        return torch.atan2(q.real, q.imag)

    def amplitudeList(self, wavelength, sort="YZ", amplitude="sqrt"):
        """The on-axis field amplitude of every hit's beam at the monitor, a sqrt(2 / pi) / w with w = `spotsizeList` and a =
        sqrt(IList) (amplitude="sqrt") or IList ("linear"): the peak of |u| in `OpticalTable.wave_all`, whose square integrates
        to a^2 over the plane."""
        import torch

        if amplitude not in ("sqrt", "linear"):
            raise ValueError(f"amplitude must be 'sqrt' or 'linear', not {amplitude!r}")
        a = self.IList(sort).double()
        if amplitude == "sqrt":
            a = torch.sqrt(a)
        return a * np.sqrt(2 / np.pi) / self.spotsizeList(wavelength, sort)

    def directionList(self, sort="YZ"):
        import torch

        s = self.slot[self._order(sort)]
        return torch.stack([self._gather(f, s) for f in (self.segs.dx, self.segs.dy, self.segs.dz)], dim=1)

    def tYList(self, sort="YZ"):
        return self.directionList(sort).double() @ self._axis("Y")  # (double like the axis: a single-precision history widens here)

    def tZList(self, sort="YZ"):
        return self.directionList(sort).double() @ self._axis("Z")

    def export_rays_npz(self, filename: str):
        """`Monitor.export_rays_npz` (monitor.py:255-269) from the device tensors: the same five arrays in the
        monitor's default "YZ" order (xList / yList are the hit point along the monitor's Y / Z tangents,
        tXList / tYList the direction along them)."""
        print(f"Exporting {len(self)} rays to {filename} ...")
        arrays = {"xList": self.yList(), "yList": self.zList(), "tXList": self.tYList(), "tYList": self.tZList(), "IList": self.IList()}
        np.savez(filename, **{k: v.double().cpu().numpy() for k, v in arrays.items()})


def image_bins(bins):
    """`bins` of an image as (nby, nbz): an int (both axes) or a pair of ints, each at least 1; anything else is a ValueError."""
    import operator

    pair = bins if isinstance(bins, (tuple, list)) else (bins, bins)
    try:
        if len(pair) != 2 or any(isinstance(b, bool) for b in pair):
            raise TypeError
        nby, nbz = (operator.index(b) for b in pair)
    except TypeError:
        raise ValueError(f"bins must be an int or (nby, nbz), not {bins!r}") from None
    if nby < 1 or nbz < 1:
        raise ValueError(f"bins must be at least 1, not {bins!r}")
    return nby, nbz


WEIGHTS = ("intensity", "none")  # what a hit or a segment piece weighs in fluence_map, spots_all and wavefront_all


def check_weight(weight):
    if not isinstance(weight, str) or weight not in WEIGHTS:
        raise ValueError(f'weight must be "intensity" or "none", not {weight!r}')


def image_edges(monitor, nby, nbz):
    """The bin edges of a monitor's image, as `Monitor.render_hist` / `_get_hist_y` bin it (monitor.py:195-200, 271-289):
    nby equal bins over +-width / 2 along y, nbz over +-height / 2 along z — what np.histogram_bin_edges gives for that range."""
    return (np.linspace(-monitor.width / 2, monitor.width / 2, nby + 1), np.linspace(-monitor.height / 2, monitor.height / 2, nbz + 1))


class _MonitorBins:
    """What the images of a monitor share: `monitor`, int64 `counts` and the float64 planes the class names in PLANES, [nby, nbz]
    device tensors over `y_edges` x `z_edges` (numpy)."""

    PLANES = ()

    def __init__(self, monitor, counts, planes, y_edges, z_edges, stack):
        self.monitor, self.counts, self.y_edges, self.z_edges = monitor, counts, y_edges, z_edges
        for name, plane in zip(self.PLANES, planes):
            setattr(self, name, plane)
        # the call's tensors, which `into=` adds to: its [M, nby, nbz] counts and planes, then its one-element tallies (skipped,
        # aliased: the modes that have them), and last this monitor's position among the M
        self._stack = stack

    @property
    def bins(self):
        return tuple(self.counts.shape)

    def _bin_area(self):
        """Every bin's area (y width x z width), a float64 [nby, nbz] tensor on the images' device."""
        import torch

        return torch.as_tensor(np.outer(np.diff(self.y_edges), np.diff(self.z_edges)), device=self.counts.device)

    def to_host(self):
        """(counts, the planes in the order of PLANES, y_edges, z_edges) as numpy arrays."""
        return (self.counts.cpu().numpy(), *(getattr(self, name).cpu().numpy() for name in self.PLANES), self.y_edges, self.z_edges)


class _MonitorPhasors(_MonitorBins):
    """The two coherent images: per bin a complex sum, kept as `re` and `im`."""

    PLANES = ("re", "im")

    def __init__(self, monitor, counts, re, im, y_edges, z_edges, stack=None):
        super().__init__(monitor, counts, (re, im), y_edges, z_edges, stack)

    @property
    def field(self):
        """re + i im, a complex128 tensor."""
        import torch

        return torch.complex(self.re, self.im)


class MonitorImage(_MonitorBins):
    """A monitor's hits as an image, binned on the device (`OpticalTable.image_all`): `counts` (int64) and `intensity` (float64,
    the sum of the hits' intensities), [nby, nbz] device tensors over `y_edges` x `z_edges` (numpy) of the coordinates
    `MonitorHits.yList` / `zList` give — np.histogram2d(yList, zList, bins=[y_edges, z_edges], weights=IList).  Counts are exact
    and the same every run; the intensity sums are atomic fp64 adds whose last bits depend on the order of arrival."""

    PLANES = ("intensity",)

    def __init__(self, monitor, counts, intensity, y_edges, z_edges, stack=None):
        super().__init__(monitor, counts, (intensity,), y_edges, z_edges, stack)


class MonitorField(_MonitorPhasors):
    """A monitor's hits as a coherent image, summed on the device (`OpticalTable.field_all`): `counts` (int64) and `re`, `im`
    (float64), [nby, nbz] device tensors over `y_edges` x `z_edges` (numpy) — per bin the number of hits and the sum of their
    phasors a exp(i phi), a = sqrt(IList) (or IList: amplitude="linear"), phi = `MonitorHits.phaseList`.  Counts are exact and the
    same every run; re and im are atomic fp64 sums whose last bits depend on the order of arrival."""

    def intensity(self):
        """|field|^2 = re^2 + im^2: what a detector reads."""
        return self.re**2 + self.im**2


class MonitorBeam(_MonitorBins):
    """A monitor's hits as the image their Gaussian beams make, summed on the device (`OpticalTable.beam_all`): `counts` (int64,
    the hit centres, as `MonitorImage.counts`) and `power` (float64), [nby, nbz] device tensors over `y_edges` x `z_edges` (numpy)
    — per bin the sum over the hits of IList times the share of a Gaussian spot of radius `MonitorHits.spotsizeList` around
    (yList, zList) that falls into the bin, the beam taken at normal incidence.  Counts are exact and the same every run; power
    is atomic fp64 sums whose last bits depend on the order of arrival."""

    PLANES = ("power",)

    def __init__(self, monitor, counts, power, y_edges, z_edges, stack=None):
        super().__init__(monitor, counts, (power,), y_edges, z_edges, stack)

    def irradiance(self):
        """`power` per unit area: every bin's power over its area (y width x z width), a float64 [nby, nbz] device tensor."""
        return self.power / self._bin_area()


class MonitorWave(_MonitorPhasors):
    """A monitor's hits as the coherent image their Gaussian beams make, summed on the device (`OpticalTable.wave_all`): `counts`
    (int64, the hit centres, as `MonitorImage.counts`) and `re`, `im` (float64), [nby, nbz] device tensors over `y_edges` x
    `z_edges` (numpy) — per bin the sum over the hits of the beam's complex field at the bin's CENTRE: amplitude
    `MonitorHits.amplitudeList` under a Gaussian envelope of radius `spotsizeList` around (yList, zList), with the phase
    `phaseList` plus the beam's tilt (`tYList`, `tZList`) and wavefront curvature (`radiusList`) across the monitor.  `aliased`:
    how many hits of the call (all its monitors together, every call that added `into` it) turn their phase more than half a cycle
    from one bin centre to the next somewhere on their footprint — where it is not 0 the image is undersampled.  Counts are exact
    and the same every run; re and im are atomic fp64 sums whose last bits depend on the order of arrival."""

    def __init__(self, monitor, counts, re, im, y_edges, z_edges, aliased=0, stack=None):
        super().__init__(monitor, counts, re, im, y_edges, z_edges, stack)
        self.aliased = aliased

    def irradiance(self):
        """|field|^2 = re^2 + im^2: power per unit area at every bin's centre, a float64 [nby, nbz] device tensor."""
        return self.re**2 + self.im**2

    def power(self):
        """`irradiance()` times the bin's area (y width x z width): the power a bin receives, midpoint rule."""
        return self.irradiance() * self._bin_area()
