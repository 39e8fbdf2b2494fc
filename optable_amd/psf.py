"""Diffraction PSF: the plane waves of a monitor's hits summed over a grid of image samples (`OpticalTable.psf_all` / `psf_batch`)
on the device (ot_monitor_psf_many), and what the host makes of the image: the true Strehl ratio, the MTF and the encircled
energy.

Every hit j of a monitor has an amplitude a_j and a phase, in cycles, x_j(k, l) = x0_j + gy_j y_k + gz_j z_l at the sample
(y_k, z_l) (include/optable_hip.h); the field is U[k, l] = sum_j a_j exp(2 pi i x_j(k, l)) and `norm` = sum_j a_j, what |U| is
where every hit arrives in phase.  The model: each ray is a plane-wave sample.  The result is the diffraction PSF when the rays
sample the direction cosines (`focus=`) or the pupil positions (`direction=`) uniformly, with the intensity as weight; for any
other ray distribution it is that distribution's weighted sum.  There is no pi on reflection, every hit of a monitor adds to one field
(as in `field_all`; `psf_grouped_all` / `MonitorPSFGroups` keep a field per group of rays), and the image repeats with the period wavelength / (n x ray spacing).  The reference has no PSF;
this module is defined by the header and by this text.
"""
import numpy as np

AMPLITUDES = ("sqrt", "linear", "unit")  # amplitude_mode 0, 1, 2 of ot_monitor_psf_many
MAX_SAMPLES = 512


def _pair(value, what, kind):
    """`value` as a pair of `kind` (int or float): one number for both axes, or (y, z)."""
    pair = value if isinstance(value, (tuple, list, np.ndarray)) else (value, value)
    if len(pair) != 2 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer) if kind is int else (int, float, np.integer, np.floating))
                             for v in pair):
        raise ValueError(f"{what} must be one {'int' if kind is int else 'number'} or a pair (y, z), not {value!r}")
    return kind(pair[0]), kind(pair[1])


def psf_pixels(pixels):
    """(ny, nz) of `pixels`: one int or a pair, each 1 .. 512."""
    ny, nz = _pair(pixels, "pixels", int)
    if not 1 <= ny <= MAX_SAMPLES or not 1 <= nz <= MAX_SAMPLES:
        raise ValueError(f"pixels must be 1 .. {MAX_SAMPLES} along each axis, not {pixels!r}")
    return ny, nz


def psf_step(step):
    """(dy, dz) of `step`: one number or a pair, finite and > 0."""
    if step is None:
        raise ValueError("step= is required: the spacing of the samples, in lengths with focus= and in direction cosines with direction=")
    dy, dz = _pair(step, "step", float)
    if not (np.isfinite(dy) and np.isfinite(dz) and dy > 0.0 and dz > 0.0):
        raise ValueError(f"step must be finite and > 0, not {step!r}")
    return dy, dz


def psf_grid(step, pixels, centre, n_monitors):
    """The [M, 4] table (y0, dy, z0, dz) of the call and the samples' coordinates: sample k of an axis of n lies at
    c + (k - (n - 1) / 2) x step, so an odd count puts a sample on the reference itself (centre = (0, 0)).  `centre`: one (y, z) for
    all monitors or one per monitor.  Returns (grid, (ny, nz), (dy, dz), centres [M, 2])."""
    from .wavefront import _rows

    (ny, nz), (dy, dz) = psf_pixels(pixels), psf_step(step)
    centres = _rows(centre, n_monitors, 2, "centre")
    grid = np.empty((n_monitors, 4))
    grid[:, 0], grid[:, 1] = centres[:, 0] - (ny - 1) / 2 * dy, dy
    grid[:, 2], grid[:, 3] = centres[:, 1] - (nz - 1) / 2 * dz, dz
    return np.ascontiguousarray(grid), (ny, nz), (dy, dz), centres


def psf_amplitude(amplitude):
    if not isinstance(amplitude, str) or amplitude not in AMPLITUDES:
        raise ValueError(f"amplitude must be 'sqrt', 'linear' or 'unit', not {amplitude!r}")
    return AMPLITUDES.index(amplitude)


class MonitorPSF:
    """The hits of one monitor as a diffraction image (`OpticalTable.psf_all`).  Device tensors: `counts` (the hits summed),
    `skipped` (hits left out: no usable ray, wavelength or phase), `aliased` (hits whose phase turns more than half a cycle from one
    sample to the next: summed all the same) — int64 scalars — `norm` (sum of the amplitudes, a float64 scalar) and `re`, `im`
    (float64 [ny, nz]).  Plain attributes: `y`, `z` (the samples' coordinates, numpy: lengths about the focus or direction cosines
    about the plane wave), `extent` = (y[0], y[-1], z[0], z[-1]), `reference` = ("focus" | "direction", the lab vector), `step`,
    `centre`, `amplitude`.  The same bits every run.  Everything is NaN where `norm` is 0."""

    def __init__(self, monitor, counts, norm, re, im, reference, grid, step, centre, amplitude, stack=None):
        self.monitor, self.counts, self.skipped, self.aliased, self.norm, self.re, self.im = monitor, counts[0], counts[1], counts[2], norm, re, im
        self.reference = (reference[0], tuple(float(v) for v in reference[1]))
        self.step, self.centre, self.amplitude = tuple(float(v) for v in step), tuple(float(v) for v in centre), amplitude
        ny, nz = re.shape
        self.y = float(grid[0]) + np.arange(ny) * float(grid[1])
        self.z = float(grid[2]) + np.arange(nz) * float(grid[3])
        self.extent = (self.y[0], self.y[-1], self.z[0], self.z[-1])
        self._stack = stack  # (counts, norm, re, im of the whole call, this monitor's place in it): what `into=` adds to

    @property
    def field(self):
        """re + i im, complex128 [ny, nz]."""
        import torch

        return torch.complex(self.re, self.im)

    def intensity(self):
        """|U|^2 = re^2 + im^2."""
        return self.re * self.re + self.im * self.im

    def normalised(self):
        """|U|^2 / norm^2: 1 where every hit arrives in phase; NaN where norm is 0."""
        import torch

        n2 = self.norm * self.norm
        return self.intensity() / torch.where(n2 > 0, n2, torch.full_like(n2, float("nan")))

    def _reference_sample(self):
        """(k, l) of the sample that lies on the reference (coordinates 0, 0), or None: within a millionth of a step."""
        at = []
        for axis, step in ((self.y, self.step[0]), (self.z, self.step[1])):
            k = int(np.argmin(np.abs(axis)))
            if abs(axis[k]) > 1e-6 * step:
                return None
            at.append(k)
        return tuple(at)

    def strehl(self, at="reference"):
        """The Strehl ratio: the normalised intensity at the sample on the reference (at="reference"; ValueError when the grid has
        none: an even count, or a centre off it) or at the brightest sample (at="peak")."""
        if at == "peak":
            return self.normalised().max()
        if at != "reference":
            raise ValueError(f'at must be "reference" or "peak", not {at!r}')
        where = self._reference_sample()
        if where is None:
            raise ValueError("no sample lies on the reference: use an odd number of pixels with centre=(0, 0), or at=\"peak\"")
        return self.normalised()[where]

    def _host_intensity(self):
        re, im = self.re.detach().cpu().numpy().astype(np.float64, copy=False), self.im.detach().cpu().numpy().astype(np.float64, copy=False)
        return re * re + im * im, float(self.norm)

    def mtf(self):
        """(mtf, fy, fz): |FFT2(intensity)| / sum(intensity) with the zero frequency in the middle (numpy, [ny, nz]) and its
        frequency axes in cycles per unit of `y` / `z`.  NaN where norm is 0 or the image is dark."""
        I, norm = self._host_intensity()
        total = I.sum()
        fy, fz = np.fft.fftshift(np.fft.fftfreq(len(self.y), self.step[0])), np.fft.fftshift(np.fft.fftfreq(len(self.z), self.step[1]))
        if not (norm > 0.0 and total > 0.0):
            return np.full(I.shape, np.nan), fy, fz
        return np.abs(np.fft.fftshift(np.fft.fft2(I))) / total, fy, fz

    def encircled_energy(self, radii, about="centroid"):
        """The share of the image's energy (the sum of the intensity over the samples) within each of `radii` of its centroid
        (about="centroid") or of the reference (about="reference": the coordinates 0, 0), numpy.  NaN where norm is 0."""
        if about not in ("centroid", "reference"):
            raise ValueError(f'about must be "centroid" or "reference", not {about!r}')
        radii = np.atleast_1d(np.asarray(radii, dtype=np.float64))
        I, norm = self._host_intensity()
        total = I.sum()
        if not (norm > 0.0 and total > 0.0):
            return np.full(radii.shape, np.nan)
        cy, cz = (0.0, 0.0) if about == "reference" else ((I.sum(axis=1) @ self.y) / total, (I.sum(axis=0) @ self.z) / total)
        r = np.hypot(self.y[:, None] - cy, self.z[None, :] - cz)
        return np.array([I[r <= rad].sum() / total for rad in radii])

    def to_host(self):
        """(used, skipped, aliased, norm, field): three ints, a float and the complex field as a numpy array."""
        field = self.re.detach().cpu().numpy() + 1j * self.im.detach().cpu().numpy()
        return int(self.counts), int(self.skipped), int(self.aliased), float(self.norm), field


def psf_weights(weights, n_groups):
    """`weights` of the incoherent sums as a float64 numpy vector of one non-negative finite number per group; None: all 1 (the hits'
    amplitudes already carry their power)."""
    if weights is None:
        return np.ones(n_groups)
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"weights must be one non-negative number per group ({n_groups}), not {weights!r}") from None
    if w.shape != (n_groups,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError(f"weights must be one non-negative number per group ({n_groups}), not {weights!r}")
    return w


class MonitorPSFGroups:
    """The hits of one monitor as diffraction images PER RAY GROUP (`OpticalTable.psf_grouped_all`): one field per group — the
    wavelengths of a multiplexed batch, its field points — from one trace.  Fields of different groups are never added on the
    device: white light adds the INTENSITIES of its wavelengths.  Device tensors: `counts`, `skipped`, `aliased` (int64 [G]), `norm`
    (float64 [G]), `re`, `im` (float64 [G, ny, nz]) as `MonitorPSF`'s per group, and `ungrouped` (an int64 scalar: the hits of rays
    in no group, which are in no image).  Plain attributes as `MonitorPSF`, plus `n_groups` = G and `labels` (what the groups
    stand for, one per group, or None).  `group(g)` is a `MonitorPSF` on views of group g, `coherent()` one of the fields added —
    what `psf_all` gives; the other methods are about the INCOHERENT sum sum_g w_g |U_g|^2 with `weights` w (one non-negative
    number per group, spectral weights say; None: all 1, the hits' amplitudes already carry their power)."""

    def __init__(self, monitor, counts, norm, re, im, ungrouped, reference, grid, step, centre, amplitude, labels=None, stack=None):
        self.monitor, self.norm, self.re, self.im, self.ungrouped = monitor, norm, re, im, ungrouped
        self.counts, self.skipped, self.aliased = counts[:, 0], counts[:, 1], counts[:, 2]
        self.n_groups = int(re.shape[0])
        if labels is not None and len(labels) != self.n_groups:
            raise ValueError(f"labels: one per group ({self.n_groups}), not {len(labels)}")
        self.labels = None if labels is None else list(labels)
        self.reference = (reference[0], tuple(float(v) for v in reference[1]))
        self.step, self.centre, self.amplitude = tuple(float(v) for v in step), tuple(float(v) for v in centre), amplitude
        self._grid, self._counts = tuple(float(v) for v in grid), counts
        _, ny, nz = re.shape
        self.y = self._grid[0] + np.arange(ny) * self._grid[1]
        self.z = self._grid[2] + np.arange(nz) * self._grid[3]
        self.extent = (self.y[0], self.y[-1], self.z[0], self.z[-1])
        self._stack = stack  # (counts, norm, re, im, ungrouped of the whole call, this monitor's place in it): what `into=` adds to

    def group(self, g):
        """Group g as a `MonitorPSF` on views of this object's tensors: everything that class computes, per group."""
        g = int(g)
        if not 0 <= g < self.n_groups:
            raise IndexError(f"group {g} of {self.n_groups}")
        return MonitorPSF(self.monitor, self._counts[g], self.norm[g], self.re[g], self.im[g], self.reference, self._grid, self.step, self.centre,
                          self.amplitude)

    def coherent(self):
        """The fields of all groups ADDED, as a `MonitorPSF` (new tensors): what `psf_all` gives on the same hits, up to the order of
        the sum — hits of different groups interfere in it."""
        return MonitorPSF(self.monitor, self._counts.sum(dim=0), self.norm.sum(), self.re.sum(dim=0), self.im.sum(dim=0), self.reference, self._grid,
                          self.step, self.centre, self.amplitude)

    def _weights(self, weights):
        import torch

        return torch.from_numpy(psf_weights(weights, self.n_groups)).to(self.re.device)

    def intensity(self, weights=None):
        """sum_g w_g |U_g|^2, [ny, nz]."""
        w = self._weights(weights)
        return ((self.re * self.re + self.im * self.im) * w[:, None, None]).sum(dim=0)

    def normalised(self, weights=None):
        """The incoherent sum over sum_g w_g norm_g^2: 1 where every hit of every group arrives in phase with its own group; NaN
        where the denominator is 0."""
        import torch

        d = (self._weights(weights) * self.norm * self.norm).sum()
        return self.intensity(weights) / torch.where(d > 0, d, torch.full_like(d, float("nan")))

    def strehl(self, at="reference", weights=None):
        """The polychromatic Strehl ratio: `normalised(weights)` at the sample on the reference (at="reference"; ValueError when
        the grid has none) or at its brightest sample (at="peak")."""
        if at == "peak":
            return self.normalised(weights).max()
        if at != "reference":
            raise ValueError(f'at must be "reference" or "peak", not {at!r}')
        where = self.group(0)._reference_sample()
        if where is None:
            raise ValueError("no sample lies on the reference: use an odd number of pixels with centre=(0, 0), or at=\"peak\"")
        return self.normalised(weights)[where]

    def strehls(self, at="reference"):
        """The Strehl ratio of every group on its own, a [G] tensor (`MonitorPSF.strehl` per group)."""
        import torch

        return torch.stack([self.group(g).strehl(at=at) for g in range(self.n_groups)])

    def _host_intensity(self, weights):
        w = psf_weights(weights, self.n_groups)
        re, im, norm = self.re.detach().cpu().numpy(), self.im.detach().cpu().numpy(), self.norm.detach().cpu().numpy()
        return np.tensordot(w, re * re + im * im, axes=1), float(np.sum(w * norm * norm))

    def mtf(self, weights=None):
        """(mtf, fy, fz) of the incoherent sum, as `MonitorPSF.mtf`: the polychromatic MTF.  NaN where the denominator of
        `normalised` is 0 or the image is dark."""
        I, d = self._host_intensity(weights)
        total = I.sum()
        fy, fz = np.fft.fftshift(np.fft.fftfreq(len(self.y), self.step[0])), np.fft.fftshift(np.fft.fftfreq(len(self.z), self.step[1]))
        if not (d > 0.0 and total > 0.0):
            return np.full(I.shape, np.nan), fy, fz
        return np.abs(np.fft.fftshift(np.fft.fft2(I))) / total, fy, fz

    def encircled_energy(self, radii, about="centroid", weights=None):
        """The share of the incoherent sum's energy within each of `radii` of its centroid or of the reference, as
        `MonitorPSF.encircled_energy`.  NaN where the denominator of `normalised` is 0."""
        if about not in ("centroid", "reference"):
            raise ValueError(f'about must be "centroid" or "reference", not {about!r}')
        radii = np.atleast_1d(np.asarray(radii, dtype=np.float64))
        I, d = self._host_intensity(weights)
        total = I.sum()
        if not (d > 0.0 and total > 0.0):
            return np.full(radii.shape, np.nan)
        cy, cz = (0.0, 0.0) if about == "reference" else ((I.sum(axis=1) @ self.y) / total, (I.sum(axis=0) @ self.z) / total)
        r = np.hypot(self.y[:, None] - cy, self.z[None, :] - cz)
        return np.array([I[r <= rad].sum() / total for rad in radii])

    def to_host(self):
        """(used, skipped, aliased, norm, field, ungrouped): int64 [G] three times, float64 [G], the complex fields [G, ny, nz] (numpy)
        and an int."""
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        return host(self.counts), host(self.skipped), host(self.aliased), host(self.norm), host(self.re) + 1j * host(self.im), int(self.ungrouped)
