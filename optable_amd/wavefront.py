"""Wavefront error: the hits of a monitor as the moments of their optical path difference over a unit pupil
(`OpticalTable.wavefront_all` / `wavefront_batch`), summed on the device with no hit list (ot_monitor_wavefront_many), and what the
host makes of them: the least-squares coefficients of the Noll-ordered orthonormal Zernike polynomials up to radial order 4, the
rms wavefront error left after any number of them is fitted out, and the Strehl ratio of the Marechal approximation.

The device returns 61 sums per monitor (include/optable_hip.h): S[a, b] = sum w p^a q^b (a + b <= 8), T[a, b] = sum w W' p^a q^b
(a + b <= 4) and Q = sum w W'^2, W' = W - piston.  A polynomial basis Z_i = sum_k A[i, k] m_k over the 15 monomials m_k = p^a q^b
of degree <= 4 has the Gram matrix G = A [S of m_k m_l] A^T and the right-hand side b = A T: any basis of that degree comes out of
the same sums exactly.  The reference has no wavefront analysis; this module is defined by the header and by this text.
"""
import math

import numpy as np

from .monitors import WEIGHTS  # noqa: F401  (importable from here too)

COORDINATES = ("direction", "position")  # 0, 1 of ot_monitor_wavefront_many
DEGREE, TERMS, N_S, N_T, N_SUMS = 4, 15, 45, 15, 61
RCOND = 1e-12  # a Gram matrix whose reciprocal condition is below this determines no fit


def place(a, b):
    """Where the pair (a, b) sits among the monomials p^a q^b ordered by degree g = a + b, then b: g (g + 1) / 2 + b."""
    g = a + b
    return g * (g + 1) // 2 + b


MONOMIALS = tuple((g - b, b) for g in range(DEGREE + 1) for b in range(g + 1))  # the 15 (a, b) of T, in its order
_PRODUCT = np.array([[place(a + c, b + d) for (c, d) in MONOMIALS] for (a, b) in MONOMIALS])  # m_k m_l among the 45 of S

# The first 15 Zernike polynomials in Noll's order, orthonormal over the unit disc ((1 / pi) int Z_i Z_j dA = delta_ij), as
# {(a, b): coefficient of p^a q^b} with p = rho cos(theta), q = rho sin(theta): data, checked against the closed-form disc
# integrals of p^a q^b in tests/test_wavefront_cpu.py.
_R3, _R5, _R6, _R8, _R10 = math.sqrt(3.0), math.sqrt(5.0), math.sqrt(6.0), math.sqrt(8.0), math.sqrt(10.0)
NOLL = (
    ("piston", {(0, 0): 1.0}),
    ("tilt p", {(1, 0): 2.0}),
    ("tilt q", {(0, 1): 2.0}),
    ("defocus", {(2, 0): 2 * _R3, (0, 2): 2 * _R3, (0, 0): -_R3}),
    ("astigmatism 45", {(1, 1): 2 * _R6}),
    ("astigmatism 0", {(2, 0): _R6, (0, 2): -_R6}),
    ("coma q", {(2, 1): 3 * _R8, (0, 3): 3 * _R8, (0, 1): -2 * _R8}),
    ("coma p", {(3, 0): 3 * _R8, (1, 2): 3 * _R8, (1, 0): -2 * _R8}),
    ("trefoil q", {(2, 1): 3 * _R8, (0, 3): -_R8}),
    ("trefoil p", {(3, 0): _R8, (1, 2): -3 * _R8}),
    ("spherical", {(4, 0): 6 * _R5, (2, 2): 12 * _R5, (0, 4): 6 * _R5, (2, 0): -6 * _R5, (0, 2): -6 * _R5, (0, 0): _R5}),
    ("secondary astigmatism 0", {(4, 0): 4 * _R10, (0, 4): -4 * _R10, (2, 0): -3 * _R10, (0, 2): 3 * _R10}),
    ("secondary astigmatism 45", {(3, 1): 8 * _R10, (1, 3): 8 * _R10, (1, 1): -6 * _R10}),
    ("tetrafoil 0", {(4, 0): _R10, (2, 2): -6 * _R10, (0, 4): _R10}),
    ("tetrafoil 45", {(3, 1): 4 * _R10, (1, 3): -4 * _R10}),
)
NOLL_NAMES = tuple(name for name, _ in NOLL)


def noll_matrix():
    """A [15, 15]: row i holds Noll term i + 1 over the 15 monomials in T's order."""
    A = np.zeros((TERMS, len(MONOMIALS)))
    for i, (_, poly) in enumerate(NOLL):
        for (a, b), c in poly.items():
            A[i, place(a, b)] = c
    return A


_A = noll_matrix()


def zernike(terms, p, q):
    """The first `terms` Noll terms at the points (p, q) (numpy arrays): [terms, ...]."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    mono = np.stack([p**a * q**b for a, b in MONOMIALS])
    return np.tensordot(_A[:_terms(terms)], mono, axes=1)


def _terms(terms):
    if isinstance(terms, bool) or not isinstance(terms, (int, np.integer)) or not 1 <= terms <= TERMS:
        raise ValueError(f"terms must be 1 .. {TERMS}, not {terms!r}")
    return int(terms)


# -- the arguments of OpticalTable.wavefront_all as the tables the engine takes ----------------------------------------------------
def _rows(value, n_monitors, width, what):
    """`value` as a finite [n_monitors, width] float64 table: one row for all monitors or one per monitor."""
    try:
        value = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be {width} finite numbers, or as many per monitor, not {value!r}") from None
    if value.shape == (width,):
        value = np.tile(value, (n_monitors, 1))
    if value.shape != (n_monitors, width) or not np.isfinite(value).all():
        raise ValueError(f"{what} must be {width} finite numbers, or as many per monitor ({n_monitors}), not {value!r}")
    return np.ascontiguousarray(value)


def local_frame(monitor):
    """(M, origin) of a monitor's pose: local = M^T (x - origin); the columns of M are the local axes in the lab."""
    return np.asarray(monitor.transform_matrix, dtype=np.float64).reshape(3, 3), np.asarray(monitor.origin, dtype=np.float64)


def wavefront_reference(focus, direction, monitors):
    """(reference_kind, lab [M, 3], local [M, 3]) of exactly one of `focus` (a point, kind 0) or `direction` (a vector, made unit,
    kind 1), one for all monitors or one per monitor, in the lab frame; `local` is what the device takes: M^T (F - origin), M^T u."""
    if (focus is None) == (direction is None):
        raise ValueError("exactly one of focus= (a point) or direction= (a vector) says what the wavefront is measured against")
    n = len(monitors)
    if focus is not None:
        lab = _rows(focus, n, 3, "focus")
        local = np.array([local_frame(m)[0].T @ (f - local_frame(m)[1]) for m, f in zip(monitors, lab)]).reshape(n, 3)
        return 0, lab, np.ascontiguousarray(local)
    lab = _rows(direction, n, 3, "direction")
    norm = np.sqrt((lab * lab).sum(axis=1))
    if not (norm > 0.0).all() or not np.isfinite(norm).all():
        raise ValueError(f"direction must not be zero, not {direction!r}")
    lab = lab / norm[:, None]
    local = np.array([local_frame(m)[0].T @ u for m, u in zip(monitors, lab)]).reshape(n, 3)
    return 1, lab, np.ascontiguousarray(local)


def wavefront_pupil(pupil, kind, monitors):
    """`pupil` as [M, 3] (c_y, c_z, R), R > 0: one for all or one per monitor; None with a direction: the largest circle about the
    monitor's centre, (0, 0, min(width, height) / 2); with a focus it must be given."""
    if pupil is None:
        if kind == 0:
            raise ValueError("pupil=(c_y, c_z, R) is required with focus=: the direction coordinates have no natural extent")
        pupil = [(0.0, 0.0, min(m.width, m.height) / 2) for m in monitors]
        if not monitors:
            return np.zeros((0, 3))
    pupil = _rows(pupil, len(monitors), 3, "pupil")
    if not (pupil[:, 2] > 0.0).all():
        raise ValueError(f"the pupil's radius must be positive, not {pupil[:, 2]!r}")
    return pupil


def wavefront_coordinates(coordinates, kind):
    """0 (direction) or 1 (position); None: direction for a focus, position for a plane wave."""
    if coordinates is None:
        return 0 if kind == 0 else 1
    if isinstance(coordinates, str) and coordinates in COORDINATES:
        return COORDINATES.index(coordinates)
    if isinstance(coordinates, bool) or not isinstance(coordinates, (int, np.integer)) or coordinates not in (0, 1):
        raise ValueError(f'coordinates must be None, 0 / "direction" or 1 / "position", not {coordinates!r}')
    return int(coordinates)


def wavefront_piston(piston, n_monitors):
    """`piston` as [M] finite doubles: a number for all monitors or one per monitor."""
    try:
        piston = np.asarray(piston, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"piston must be None, a finite number or one per monitor, not {piston!r}") from None
    if piston.ndim == 0:
        piston = np.full(n_monitors, float(piston))
    if piston.shape != (n_monitors,) or not np.isfinite(piston).all():
        raise ValueError(f"piston must be None, a finite number or one per monitor ({n_monitors}), not {piston!r}")
    return np.ascontiguousarray(piston)


# -- the same arguments per (monitor, group): OpticalTable.wavefront_grouped_all ------------------------------------------------------
def _cells(value, n_monitors, n_groups, width, what):
    """`value` as a finite [n_monitors, n_groups, width] float64 table (width 0: [n_monitors, n_groups] of numbers): one entry for
    all cells, one per monitor [M, ...], one per group [G, ...] — only when M != G: an ambiguous shape is read as per monitor —
    or one per cell [M, G, ...]."""
    M, G, tail = n_monitors, n_groups, ((width,) if width else ())
    entry = f"{width} finite numbers" if width else "a finite number"
    error = f"{what} must be {entry}: one for all, one per monitor ({M}), one per group ({G}) or [{M}, {G}], not "
    try:
        value = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(error + repr(value)) from None
    if value.shape == tail:
        table = np.broadcast_to(value, (M, G) + tail)
    elif value.shape == (M,) + tail:
        table = np.broadcast_to(value.reshape((M, 1) + tail), (M, G) + tail)
    elif value.shape == (G,) + tail:
        table = np.broadcast_to(value.reshape((1, G) + tail), (M, G) + tail)
    elif value.shape == (M, G) + tail:
        table = value
    else:
        raise ValueError(error + f"of shape {value.shape}")
    if not np.isfinite(table).all():
        raise ValueError(error + repr(value))
    return np.ascontiguousarray(table)


def wavefront_group_reference(focus, direction, monitors, n_groups):
    """`wavefront_reference` per (monitor, group): (reference_kind, lab [M, G, 3], local [M, G, 3]).  `focus` / `direction`: one
    for all, one per monitor [M, 3], one per group [G, 3] (when M == G a [M, 3] table is read as per MONITOR) or [M, G, 3]."""
    if (focus is None) == (direction is None):
        raise ValueError("exactly one of focus= (a point) or direction= (a vector) says what the wavefront is measured against")
    M, G = len(monitors), int(n_groups)
    kind = 0 if focus is not None else 1
    lab = _cells(focus if kind == 0 else direction, M, G, 3, ("focus", "direction")[kind])
    if kind == 1:
        norm = np.sqrt((lab * lab).sum(axis=-1))
        if not (norm > 0.0).all() or not np.isfinite(norm).all():
            raise ValueError(f"direction must not be zero, not {direction!r}")
        lab = lab / norm[..., None]
    local = np.empty((M, G, 3))
    for k, m in enumerate(monitors):
        R, origin = local_frame(m)
        for g in range(G):  # (the expressions of wavefront_reference: the same bits for the same vector)
            local[k, g] = R.T @ (lab[k, g] - origin) if kind == 0 else R.T @ lab[k, g]
    return kind, np.ascontiguousarray(lab), np.ascontiguousarray(local)


def wavefront_group_pupil(pupil, kind, monitors, n_groups):
    """`wavefront_pupil` per (monitor, group): [M, G, 3] (c_y, c_z, R), R > 0, in the shapes of `wavefront_group_reference`; None
    with a direction: (0, 0, min(width, height) / 2) of every monitor, for all its groups."""
    M, G = len(monitors), int(n_groups)
    if pupil is None:
        if kind == 0:
            raise ValueError("pupil=(c_y, c_z, R) is required with focus=: the direction coordinates have no natural extent")
        pupil = np.array([(0.0, 0.0, min(m.width, m.height) / 2) for m in monitors], dtype=np.float64).reshape(M, 1, 3).repeat(G, axis=1)
    pupil = _cells(pupil, M, G, 3, "pupil")
    if not (pupil[..., 2] > 0.0).all():
        raise ValueError(f"the pupil's radius must be positive, not {pupil[..., 2]!r}")
    return pupil


def wavefront_group_piston(piston, n_monitors, n_groups):
    """`wavefront_piston` per (monitor, group): [M, G] finite doubles from a number, [M], [G] (read as per monitor when M == G) or [M, G]."""
    return _cells(piston, n_monitors, int(n_groups), 0, "piston")


def hit_wavefront(kind, local, P, t, d, n_index, pathlength):
    """The header's W of hits, hit by hit (torch or numpy alike): P [h, 3] the local hit points, t [h] the distances, d [h, 3] the
    renormalised local directions, n_index and pathlength [h] of the hits' segments; `local` the three numbers of the reference."""
    L = t * n_index + pathlength
    if kind == 0:
        return L + n_index * ((local[0] - P[:, 0]) * d[:, 0] + (local[1] - P[:, 1]) * d[:, 1] + (local[2] - P[:, 2]) * d[:, 2])
    return L - n_index * (P[:, 0] * local[0] + P[:, 1] * local[1] + P[:, 2] * local[2])


class MonitorWavefront:
    """The hits of one monitor as a wavefront (`OpticalTable.wavefront_all`): `counts` (the hits inside the pupil) and `outside`
    (the others, which add to no sum) are int64 scalars, `sums` the 61 float64 sums S, T, Q of the header, all on the device;
    `reference` = ("focus" | "direction", the lab vector), `pupil` = (c_y, c_z, R), `coordinates` = "direction" | "position",
    `piston` the number subtracted from every W before it was summed, `weight` "intensity" or "none".  Counts are exact; the
    sums are the same bits every run.  Every method is a small float64 expression on the sums, NaN where the fit is not determined:
    fewer hits inside than terms, or a Gram matrix with a reciprocal condition below 1e-12.  Lengths are the table's."""

    def __init__(self, monitor, counts, outside, sums, reference, pupil, coordinates, piston, weight, stack=None):
        self.monitor, self.counts, self.outside, self.sums, self.weight = monitor, counts, outside, sums, weight
        self.reference = (reference[0], tuple(float(v) for v in reference[1]))
        self.pupil, self.coordinates, self.piston = tuple(float(v) for v in pupil), coordinates, float(piston)
        self._stack = stack  # (counts, sums of the whole call, this monitor's place in it): what `into=` adds to

    def _host(self):
        return int(self.counts), self.sums.detach().cpu().numpy().astype(np.float64, copy=False)

    def _tensor(self, value):
        import torch

        return torch.as_tensor(np.asarray(value, dtype=np.float64), device=self.sums.device)

    def _fit(self, terms):
        """(c', b, S00, Q) of the first `terms` terms fitted to W' = W - piston, or None where the fit is not determined."""
        terms = _terms(terms)
        inside, s = self._host()
        S, T, Q = s[:N_S], s[N_S:N_S + N_T], s[N_S + N_T]
        if inside < terms or not np.isfinite(s).all() or not S[0] > 0.0:
            return None
        A = _A[:terms]
        G, b = A @ S[_PRODUCT] @ A.T, A @ T
        sv = np.linalg.svd(G, compute_uv=False)
        if not sv[0] > 0.0 or sv[-1] / sv[0] < RCOND:
            return None
        return np.linalg.solve(G, b), b, S[0], Q

    def power(self):
        """S[0, 0], the summed weight of the hits inside the pupil."""
        return self.sums[0]

    def mean(self):
        """The weighted mean of W over the pupil: piston + T[0, 0] / S[0, 0]."""
        inside, s = self._host()
        return self._tensor(self.piston + s[N_S] / s[0] if inside > 0 and s[0] != 0.0 else np.nan)

    def gram(self, terms=TERMS):
        """(G, b): the Gram matrix sum w Z_i Z_j [terms, terms] and the right-hand side sum w W' Z_i [terms] of the first `terms`
        Noll terms, W' = W - piston."""
        A = _A[:_terms(terms)]
        _, s = self._host()
        return self._tensor(A @ s[:N_S][_PRODUCT] @ A.T), self._tensor(A @ s[N_S:N_S + N_T])

    def coefficients(self, terms=TERMS):
        """The least-squares coefficients of the first `terms` Noll-ordered orthonormal Zernike polynomials of W over the pupil, in
        length units ([terms]); term 1 includes the piston."""
        fit = self._fit(terms)
        if fit is None:
            return self._tensor(np.full(_terms(terms), np.nan))
        c = fit[0].copy()
        c[0] += self.piston
        return self._tensor(c)

    def rms(self, terms=1):
        """The rms of W left after the first `terms` terms are fitted out, sqrt((Q - c . b) / S[0, 0]): terms = 1 the rms wavefront
        error (piston out), 3 without tilt, 4 without tilt and defocus.  A value that rounding left a hair below zero is 0."""
        fit = self._fit(terms)
        if fit is None:
            return self._tensor(np.nan)
        c, b, S00, Q = fit
        return self._tensor(math.sqrt(max((Q - float(c @ b)) / S00, 0.0)))

    def strehl(self, wavelength, terms=1):
        """exp(-(2 pi rms(terms) / wavelength)^2), the Marechal approximation of the Strehl ratio."""
        import torch

        return torch.exp(-((2.0 * math.pi / float(wavelength)) * self.rms(terms)) ** 2)

    def to_host(self):
        """(inside, outside, sums): two ints and the 61 sums as a numpy array."""
        return int(self.counts), int(self.outside), self.sums.detach().cpu().numpy()


class MonitorWavefrontGroups:
    """The hits of one monitor as a wavefront per RAY GROUP (`OpticalTable.wavefront_grouped_all`): `counts` and `outside` (int64,
    [G]) and `sums` (float64, [G, 61]) are device tensors; `n_groups` = G; `labels`: what the groups stand for, one per group (the
    wavelengths, say), or None.  Every group has its own ideal wave and pupil: `reference` = ("focus" | "direction", the lab
    vectors [G, 3]), `pupil` [G, 3] (c_y, c_z, R) and `piston` [G] are numpy arrays; `coordinates` and `weight` as for
    `MonitorWavefront`.  A hit belongs to the group of the input ray its segment descends from; rays whose id is outside
    0 .. G - 1 are in no group and in no tally.  `group(g)` is a `MonitorWavefront` on views of group g, and every fit here is that
    class's, group by group; `strehl` is Marechal's approximation per group — wavefronts of different wavelengths are not
    combined into one (the polychromatic image is `psf_grouped_all`'s)."""

    def __init__(self, monitor, counts, outside, sums, reference, pupil, coordinates, piston, weight, labels=None, stack=None):
        self.monitor, self.counts, self.outside, self.sums, self.weight, self.coordinates = monitor, counts, outside, sums, weight, coordinates
        self.n_groups = int(sums.shape[0])
        G = self.n_groups
        self.reference = (reference[0], np.array(reference[1], dtype=np.float64).reshape(G, 3))
        self.pupil, self.piston = np.array(pupil, dtype=np.float64).reshape(G, 3), np.array(piston, dtype=np.float64).reshape(G)
        self.labels = None if labels is None else list(labels)
        if self.labels is not None and len(self.labels) != G:
            raise ValueError(f"labels: one per group ({G}), not {len(self.labels)}")
        self._stack = stack  # (counts, sums of the whole call, this monitor's place in it): what `into=` adds to

    def group(self, g):
        """Group g as a `MonitorWavefront` (views: an `into=` call that adds to this object shows there too)."""
        g = int(g)
        if not 0 <= g < self.n_groups:
            raise IndexError(f"group {g} of {self.n_groups}")
        return MonitorWavefront(self.monitor, self.counts[g], self.outside[g], self.sums[g], (self.reference[0], self.reference[1][g]), self.pupil[g],
                                self.coordinates, self.piston[g], self.weight)

    def _each(self, what):
        import torch

        return torch.stack([what(self.group(g)) for g in range(self.n_groups)])

    def power(self):
        """S[0, 0] of every group ([G])."""
        return self.sums[:, 0]

    def mean(self):
        """The weighted mean of W over every group's pupil ([G]), NaN for a group without a hit inside."""
        return self._each(lambda wf: wf.mean())

    def coefficients(self, terms=TERMS):
        """`MonitorWavefront.coefficients` of every group: [G, terms], NaN rows where a group's fit is not determined."""
        return self._each(lambda wf: wf.coefficients(terms))

    def rms(self, terms=1):
        """`MonitorWavefront.rms` of every group: [G]."""
        return self._each(lambda wf: wf.rms(terms))

    def strehl(self, wavelength=None, terms=1):
        """Marechal's Strehl ratio of every group ([G]).  wavelength: a number for all groups, one per group, or None: `labels` are
        the groups' wavelengths (ValueError if there are none)."""
        import torch

        if wavelength is None:
            if self.labels is None:
                raise ValueError("strehl: wavelength=None takes the groups' labels as their wavelengths, and this result has none")
            wavelength = self.labels
        try:
            lam = np.asarray(wavelength, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"strehl: wavelength must be a number, one per group or None, not {wavelength!r}") from None
        if lam.ndim == 0:
            lam = np.full(self.n_groups, float(lam))
        if lam.shape != (self.n_groups,) or not (np.isfinite(lam) & (lam > 0)).all():
            raise ValueError(f"strehl: {self.n_groups} finite wavelengths > 0, not {wavelength!r}")
        return torch.exp(-((2.0 * math.pi / torch.as_tensor(lam, device=self.sums.device)) * self.rms(terms)) ** 2)

    def to_host(self):
        """(inside, outside, sums): int64 [G] twice and the sums [G, 61], numpy arrays."""
        return self.counts.cpu().numpy(), self.outside.cpu().numpy(), self.sums.detach().cpu().numpy()
