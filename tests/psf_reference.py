"""The definition of ot_monitor_psf_many (include/optable_hip.h) in numpy: the hit test of Monitor.record in double (the decisions,
with the margin every decision keeps from its boundary), then everything a hit contributes — P, t, d, L, W, gy, gz and the phase
x = x0 + gy y_k + gz z_l — in np.longdouble from the segments' float64 values, the phasors from longdouble sin and cos, the sum in
complex longdouble.  The sum is separable, exp(2 pi i x) = c Ey[k] Ez[l] with each factor the phasor of its own fraction, which
extended precision evaluates to a few 2^-64: the reference of the accuracy contract, whose bound it also computes from the data:
    |U_device - U_exact| <= norm (2 pi E + 2^-38),  E = 16 x 2^-53 x max_j(|L_j| + n_j |F_loc - P_j|) / min_j lambda_j
(kind 1: |P_j| in place of |F_loc - P_j|)."""
import collections

import numpy as np

LD = np.longdouble
PSF = collections.namedtuple("PSF", "counts norm field bound margin hits")
TWO_PI = 2 * LD("3.14159265358979323846264338327950288")  # (np.pi is a double)


def _cis(cycles):
    """exp(2 pi i frac(cycles)) of longdouble cycles, as (cos, sin)."""
    a = TWO_PI * (cycles - np.floor(cycles))
    return np.cos(a), np.sin(a)


def psf_reference(o, d, length, intensity, n_index, pathlength, ray, M, origin, half_width, half_height, axes, kind, local, grid, ny, nz, wavelength,
                  amplitude_mode=0, valid=None):
    """o, d: [n, 3]; length, intensity, n_index, pathlength: [n]; ray: [n] ints; M: 9 doubles (row-major 3 x 3, columns = the local
    axes), origin: 3; axes: 6 doubles (a_y, a_z); kind 0 / 1 with local = F_loc / u_loc; grid = (y0, dy, z0, dz); wavelength: a float
    or an array indexed by `ray`; amplitude_mode 0 sqrt(intensity), 1 intensity, 2 one; valid: [n] bools or None.  Returns PSF:
    counts (used, skipped, aliased), norm, field (complex128 [ny, nz]), bound (a float: on |U_device - U_exact| of every sample),
    margin (inf when no decision was taken), hits (the indices of the segments that hit, ascending)."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    length = np.asarray(length, dtype=np.float64).ravel()
    n = len(length)
    valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).ravel()
    M, origin, axes = np.asarray(M, dtype=np.float64).reshape(3, 3), np.asarray(origin, dtype=np.float64), np.asarray(axes, dtype=np.float64).ravel()
    # the decisions, in double as the device takes them (tests/wavefront_reference.py: the same test)
    r = o - origin
    lo = np.stack([M[0, k] * r[:, 0] + M[1, k] * r[:, 1] + M[2, k] * r[:, 2] for k in range(3)], axis=1)
    ld = np.stack([M[0, k] * d[:, 0] + M[1, k] * d[:, 1] + M[2, k] * d[:, 2] for k in range(3)], axis=1)
    margin = np.inf
    with np.errstate(all="ignore"):
        ld = ld * (1.0 / np.sqrt(ld[:, 0] * ld[:, 0] + ld[:, 1] * ld[:, 1] + ld[:, 2] * ld[:, 2]))[:, None]
        moving = valid & (ld[:, 0] != 0.0)
        t = -lo[:, 0] / ld[:, 0]
        crosses = moving & ~((np.abs(t) < 1e-9) | (t < 0.0) | (t > length))
        P = lo + t[:, None] * ld
        hit = crosses & (np.abs(P[:, 1]) <= half_width) & (np.abs(P[:, 2]) <= half_height)
        known = moving & np.isfinite(t)
        if known.any():
            margin = min(margin, np.abs(t[known] - length[known]).min(), np.abs(np.abs(t[known]) - 1e-9).min())
        if crosses.any():
            margin = min(margin, np.abs(np.abs(P[crosses, 1]) - half_width).min(), np.abs(np.abs(P[crosses, 2]) - half_height).min())
    index = np.nonzero(hit)[0]
    field = np.zeros((ny, nz), dtype=np.complex128)
    if not len(index):
        return PSF(np.zeros(3, dtype=np.int64), 0.0, field, 0.0, float(margin), index)
    # ... and what the hits contribute, in extended precision from the segments' doubles
    Ml, rl, dl = M.astype(LD), (o[index].astype(LD) - origin.astype(LD)), d[index].astype(LD)
    lo = np.stack([Ml[0, k] * rl[:, 0] + Ml[1, k] * rl[:, 1] + Ml[2, k] * rl[:, 2] for k in range(3)], axis=1)
    ld = np.stack([Ml[0, k] * dl[:, 0] + Ml[1, k] * dl[:, 1] + Ml[2, k] * dl[:, 2] for k in range(3)], axis=1)
    ld = ld / np.sqrt((ld * ld).sum(axis=1))[:, None]
    t = -lo[:, 0] / ld[:, 0]
    P = lo + t[:, None] * ld
    ni, pl, I = (np.asarray(v, dtype=np.float64).ravel()[index].astype(LD) for v in (n_index, pathlength, intensity))
    rays = np.asarray(ray).ravel()[index]
    if np.ndim(wavelength) == 0:
        lam, known = np.full(len(index), float(wavelength)), np.ones(len(index), dtype=bool)
    else:
        table = np.asarray(wavelength, dtype=np.float64).ravel()
        known = (rays >= 0) & (rays < len(table))
        lam = np.where(known, table[np.clip(rays, 0, len(table) - 1)], np.nan)
    known = known & np.isfinite(lam) & (lam > 0.0)
    lam = lam.astype(LD)
    F, ay, az = np.asarray(local, dtype=np.float64).astype(LD), axes[:3].astype(LD), axes[3:].astype(LD)
    L = t * ni + pl
    with np.errstate(all="ignore"):
        if kind == 0:
            W, gy, gz = L + ni * ((F - P) * ld).sum(axis=1), ni * (ld @ ay), ni * (ld @ az)
            size = np.abs(L) + ni * np.sqrt(((F - P) ** 2).sum(axis=1))
        else:
            W, gy, gz = L - ni * (P @ F), -ni * (P @ ay), -ni * (P @ az)
            size = np.abs(L) + ni * np.sqrt((P * P).sum(axis=1))
        x0, gy, gz = W / lam, gy / lam, gz / lam
        used = known & np.isfinite(W) & np.isfinite(gy) & np.isfinite(gz)
    y0, dy, z0, dz = (LD(float(v)) for v in grid)
    a = (np.sqrt(I), I, np.ones_like(I))[amplitude_mode][used]
    x0, gy, gz, lam, size = x0[used], gy[used], gz[used], lam[used], size[used]
    aliased = int(((np.abs(gy * dy) > 0.5) | (np.abs(gz * dz) > 0.5)).sum())
    counts = np.array([int(used.sum()), len(index) - int(used.sum()), aliased], dtype=np.int64)
    if not counts[0]:
        return PSF(counts, 0.0, field, 0.0, float(margin), index)
    yk, zl = y0 + np.arange(ny).astype(LD) * dy, z0 + np.arange(nz).astype(LD) * dz
    c = _cis(x0)
    A = _cis(gy[:, None] * yk[None, :])
    B = _cis(gz[:, None] * zl[None, :])
    Ar, Ai = a[:, None] * (c[0][:, None] * A[0] - c[1][:, None] * A[1]), a[:, None] * (c[0][:, None] * A[1] + c[1][:, None] * A[0])
    re, im = Ar.T @ B[0] - Ai.T @ B[1], Ar.T @ B[1] + Ai.T @ B[0]
    norm = a.sum()
    E = 16 * 2.0**-53 * float(size.max()) / float(lam.min())
    bound = float(norm) * (2 * np.pi * E + 2.0**-38)
    return PSF(counts, float(norm), re.astype(np.float64) + 1j * im.astype(np.float64), bound, float(margin), index)


def airy(v):
    """(2 J1(v) / v)^2, 1 at v = 0."""
    from scipy.special import j1

    v = np.asarray(v, dtype=np.float64)
    safe = np.where(v == 0.0, 1.0, v)
    return np.where(v == 0.0, 1.0, (2 * j1(safe) / safe) ** 2)


def disc_grid(n, radius):
    """The points of an n x n grid over [-radius, radius]^2 that lie inside the disc of that radius: [k, 2]."""
    g = np.linspace(-radius, radius, n)
    y, z = np.meshgrid(g, g, indexing="ij")
    keep = y * y + z * z <= radius * radius * (1 + 1e-12)
    return np.stack([y[keep], z[keep]], axis=1)


def plane_wave_sum(ty, tz, W, wavelength, y, z, weights=None):
    """The definition for rays given directly by their direction cosines (ty, tz), optical paths W and amplitudes `weights` (1) in
    a medium of index 1: U[k, l] = sum_j a_j exp(2 pi i (W_j + ty_j y_k + tz_j z_l) / wavelength), in extended precision."""
    ty, tz, W = (np.asarray(v, dtype=np.float64).astype(LD) for v in (ty, tz, W))
    a = np.ones_like(ty) if weights is None else np.asarray(weights, dtype=np.float64).astype(LD)
    lam = LD(float(wavelength))
    c = _cis(W / lam)
    A = _cis(ty[:, None] * np.asarray(y, dtype=np.float64).astype(LD)[None, :] / lam)
    B = _cis(tz[:, None] * np.asarray(z, dtype=np.float64).astype(LD)[None, :] / lam)
    Ar, Ai = a[:, None] * (c[0][:, None] * A[0] - c[1][:, None] * A[1]), a[:, None] * (c[0][:, None] * A[1] + c[1][:, None] * A[0])
    re, im = Ar.T @ B[0] - Ai.T @ B[1], Ar.T @ B[1] + Ai.T @ B[0]
    return re.astype(np.float64) + 1j * im.astype(np.float64), float(a.sum())
