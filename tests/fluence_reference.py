"""The fluence map of include/optable_hip.h (ot_fluence_map) in plain numpy, double precision: the yardstick of the rasteriser.

For every segment: project on the view's axes, renormalise the direction, clip the parameter interval [0, length] to the box,
collect the crossing parameters (edge - o) / dh of BOTH edge tables that lie strictly inside the clipped interval, sort them, and
walk the pieces between consecutive parameters — the pixel of a piece follows from the pixel of the one before by the integer
steps of the crossings between them (never by binning a midpoint).  The start pixel is counted from the same parameters: moving
up, the edges whose parameter is <= t_a lie behind; moving down, those whose parameter is > t_a lie ahead; a coordinate at rest is
binned as np.histogram bins it (half-open, the last bin closed).

Tolerance (tests/test_gpu_fluence.py): every crossing parameter is (e - o) / dh with e and o exact doubles; the subtraction, the
division and the renormalised dh (three products, two sums, a square root, a reciprocal, a product) give at most 16 U relative
error a side, U = 2^-53; a piece has two ends and there are two sides, kernel and reference: |I| 64 U t_b a piece.  Two summation
orders of c terms differ by at most 2 c U sum |I| l (the bound of tests/test_gpu_image.py).
"""
from collections import namedtuple

import numpy as np

U = 2.0**-53
Fluence = namedtuple("Fluence", "counts fluence abs_fluence bound pieces skipped clipped")


def _project(x, a):
    return x[:, 0] * a[0] + x[:, 1] * a[1] + x[:, 2] * a[2]


def _clip(lo, hi, o, dh, t_a, t_b, inside):
    """One axis of the clip, with the comparisons of the definition: a NaN parameter changes nothing."""
    rest = dh == 0.0
    inside &= ~rest | ((o >= lo) & (o <= hi))
    with np.errstate(all="ignore"):
        t_lo, t_hi = (lo - o) / dh, (hi - o) / dh
    t_in, t_out = np.where(dh > 0.0, t_lo, t_hi), np.where(dh > 0.0, t_hi, t_lo)
    t_a = np.where(~rest & (t_in > t_a), t_in, t_a)
    t_b = np.where(~rest & (t_out < t_b), t_out, t_b)
    return t_a, t_b, inside


def _axis(e, o, dh, t_a, t_b):
    """Crossing parameters of one table (inf where not strictly inside (t_a, t_b)), the step of a crossing, the start pixel."""
    nb = len(e) - 1
    moving = dh != 0.0
    with np.errstate(all="ignore"):
        t = (e[None, :] - o[:, None]) / np.where(moving, dh, 1.0)[:, None]
    up = (dh > 0.0)[:, None]
    behind_or_ahead = np.where(up, t <= t_a[:, None], t > t_a[:, None])  # moving up: edges behind; moving down: edges ahead
    first = np.clip(behind_or_ahead.sum(axis=1) - 1, 0, nb - 1)
    at_rest = np.clip(np.searchsorted(e, o, side="right") - 1, 0, nb - 1)  # (o == e[nb]: the last bin, closed)
    first = np.where(moving, first, at_rest)
    crossing = moving[:, None] & (t > t_a[:, None]) & (t < t_b[:, None])
    return np.where(crossing, t, np.inf), np.where(dh > 0.0, 1, -1), first


def fluence_reference(o, d, length, intensity, axes, u_edges, v_edges, w_lo, w_hi, valid=None):
    """o, d: [n, 3]; length: [n]; intensity: [n] or None (weight 1); axes: [3, 3] (a_u, a_v, a_w); valid: [n] bools or None.
    Returns Fluence: counts (int64 [nu, nv]), fluence = sum I l, abs_fluence = sum |I| l, bound (the tolerance of the module's
    docstring) — all [nu, nv] —, pieces (every positive piece length, one array), skipped, clipped (sum of t_b - t_a over the
    segments that deposit)."""
    o, d, length = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3), np.asarray(length, dtype=np.float64).ravel()
    axes, u_edges, v_edges = np.asarray(axes, dtype=np.float64), np.asarray(u_edges, dtype=np.float64), np.asarray(v_edges, dtype=np.float64)
    n, nu, nv = len(o), len(u_edges) - 1, len(v_edges) - 1
    weight = np.ones(n) if intensity is None else np.asarray(intensity, dtype=np.float64).ravel()
    valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).ravel()
    with np.errstate(all="ignore"):
        ou, ov, ow = (_project(o, a) for a in axes)
        du, dv, dw = (_project(d, a) for a in axes)
        norm = np.sqrt(du * du + dv * dv + dw * dw)
        inv = 1.0 / norm
        du, dv, dw = du * inv, dv * inv, dw * inv
    numbers = ~(np.isnan(ou) | np.isnan(ov) | np.isnan(ow) | np.isnan(du) | np.isnan(dv) | np.isnan(dw) | np.isnan(length)) & (norm > 0.0)
    t_a, t_b, inside = np.zeros(n), length.copy(), valid & numbers
    t_a, t_b, inside = _clip(u_edges[0], u_edges[-1], ou, du, t_a, t_b, inside)
    t_a, t_b, inside = _clip(v_edges[0], v_edges[-1], ov, dv, t_a, t_b, inside)
    t_a, t_b, inside = _clip(w_lo, w_hi, ow, dw, t_a, t_b, inside)
    inside &= t_a <= t_b
    endless = inside & ~(t_b < np.inf)
    skipped = int((valid & ~numbers).sum() + endless.sum())
    keep = np.flatnonzero(inside & ~endless)
    ou, ov, du, dv, t_a, t_b, weight = ou[keep], ov[keep], du[keep], dv[keep], t_a[keep], t_b[keep], weight[keep]
    m = len(keep)
    tu, su, ku = _axis(u_edges, ou, du, t_a, t_b)
    tv, sv, kv = _axis(v_edges, ov, dv, t_a, t_b)
    t = np.concatenate([tu, tv], axis=1)
    step_u = np.concatenate([np.broadcast_to(su[:, None], tu.shape), np.zeros(tv.shape, dtype=np.int64)], axis=1)
    step_v = np.concatenate([np.zeros(tu.shape, dtype=np.int64), np.broadcast_to(sv[:, None], tv.shape)], axis=1)
    order = np.argsort(t, axis=1, kind="stable")
    t = np.take_along_axis(t, order, axis=1)
    live = np.isfinite(t)  # (the crossings of a row come first, the masked ones are inf)
    step_u = np.where(live, np.take_along_axis(step_u, order, axis=1), 0)
    step_v = np.where(live, np.take_along_axis(step_v, order, axis=1), 0)
    # piece j runs from bounds[j] to bounds[j + 1], in the start pixel stepped by the crossings 0 .. j - 1
    ends = np.where(live, t, t_b[:, None])
    bounds = np.concatenate([t_a[:, None], ends, t_b[:, None]], axis=1)
    pu = ku[:, None] + np.concatenate([np.zeros((m, 1), dtype=np.int64), np.cumsum(step_u, axis=1)], axis=1)
    pv = kv[:, None] + np.concatenate([np.zeros((m, 1), dtype=np.int64), np.cumsum(step_v, axis=1)], axis=1)
    piece = bounds[:, 1:] - bounds[:, :-1]
    positive = piece > 0.0
    assert ((pu >= 0) & (pu < nu) & (pv >= 0) & (pv < nv))[positive].all(), "a piece of positive length outside the grid"
    pixel = (pu * nv + pv)[positive]
    lengths = piece[positive]
    w = np.broadcast_to(weight[:, None], piece.shape)[positive]
    t_end = bounds[:, 1:][positive]
    shape, size = (nu, nv), nu * nv
    counts = np.bincount(pixel, minlength=size).astype(np.int64)
    fluence = np.bincount(pixel, weights=w * lengths, minlength=size)
    abs_fluence = np.bincount(pixel, weights=np.abs(w) * lengths, minlength=size)
    ends_term = np.bincount(pixel, weights=np.abs(w) * 64.0 * U * np.abs(t_end), minlength=size)
    bound = ends_term + 2.0 * counts * U * abs_fluence
    return Fluence(counts.reshape(shape), fluence.reshape(shape), abs_fluence.reshape(shape), bound.reshape(shape), lengths, skipped,
                   float((t_b - t_a).sum()))
