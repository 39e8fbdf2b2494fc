"""The spot statistics of include/optable_hip.h (ot_monitor_spots_many) in plain numpy, double precision: the yardstick of
k_mon_spots.

For every segment and every plane j: the segment in the monitor's frame (local = M^T (x - origin), direction renormalised), the
local origin's x less offsets[j], the crossing t = -ox / dx of the plane x = 0, the tests dx == 0, |t| < 1e-9 || t < 0 ||
t > length, the rectangle |Py| <= half_width, |Pz| <= half_height, and for a hit y = P . a_y - c_y, z = P . a_z - c_z and the six
sums W, Wy, Wz, Wyy, Wzz, Wyz of its weight w — summed with math.fsum, so the reference's own sums are correctly rounded.

MARGIN: the smallest distance of any decision taken to its boundary — | |Py| - half_width | and | |Pz| - half_height | for every
crossing that passes the tests on t, and |t - length|, ||t| - 1e-9| and |t - 0| for every segment that moves along the normal.
Counts are compared for equality only where the margin is far above the rounding of P and t (the tests ask for 1e-7).

TOLERANCE of the sums (U = 2^-53), derived from the operations and returned per cell as `bound`:
  - the local origin is one subtraction and a three-term dot product on components of magnitude <= |r|_1 (r = x - origin, |M| <= 1):
    4 U |r|_1; the direction a three-term dot product, its norm (squares, sums, a root, a reciprocal) and a product: 8 U on
    components <= 1;
  - t = -ox / dx: (4 U |r|_1 + 8 U |t|) / |dx| + U |t|;  P = o + t d: 4 U |r|_1 + (error of t) + 8 U |t| + 2 U (|r|_1 + |t|):
    at most 27 U (|r|_1 + |t|) / |dx| a component;
  - y = P . a - c with |a|_1 <= sqrt 3: sqrt 3 times that, and 4 U (|P|_1 + |c|) for the dot product and the subtraction: at most
    64 U S with S = (|r|_1 + |t|) / |dx| + |c_y| + |c_z|.  Kernel and reference may each be that far from the exact value (one
    fuses multiply-adds, the other does not): d = 128 U S, S the largest of the cell's hits;
  - a term of Wy is w y: |w| d + U |w y|; of Wyy, (w y) y: |w| (2 |y| d + d^2) + 2 U |w y^2|; of Wyz: |w| ((|y| + |z|) d + d^2) +
    2 U |w y z|; w itself is exact (single precision is widened exactly);
  - the kernel sums c terms in an order of its own, (c - 1) U sum |term| to first order, and fsum rounds once: (c + 2) U sum |term|.
"""
import math
from collections import namedtuple

import numpy as np

U = 2.0**-53
Spots = namedtuple("Spots", "counts sums bound margin hits")


def spots_reference(o, d, length, weights, M, origin, half_width, half_height, axes, centre, offsets, valid=None):
    """o, d: [n, 3]; length: [n]; weights: [n] or None (1); M: 9 doubles (row-major 3 x 3, columns = the local axes), origin: 3;
    axes: 6 doubles (a_y, a_z); centre: (c_y, c_z); offsets: [J]; valid: [n] bools or None.
    Returns Spots: counts (int64 [J]), sums and bound (float64 [J, 6]: W, Wy, Wz, Wyy, Wzz, Wyz and the tolerance of each), margin
    (a float; inf when no decision was taken), hits (per plane the indices of the segments that hit)."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    length = np.asarray(length, dtype=np.float64).ravel()
    n = len(length)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
    valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).ravel()
    M, origin, axes = np.asarray(M, dtype=np.float64).reshape(3, 3), np.asarray(origin, dtype=np.float64), np.asarray(axes, dtype=np.float64).ravel()
    offsets = np.asarray(offsets, dtype=np.float64).ravel()
    o, d, length, w, index = o[valid], d[valid], length[valid], w[valid], np.nonzero(valid)[0]
    r = o - origin
    lo = np.stack([M[0, k] * r[:, 0] + M[1, k] * r[:, 1] + M[2, k] * r[:, 2] for k in range(3)], axis=1)
    ld = np.stack([M[0, k] * d[:, 0] + M[1, k] * d[:, 1] + M[2, k] * d[:, 2] for k in range(3)], axis=1)
    with np.errstate(all="ignore"):
        ld = ld * (1.0 / np.sqrt(ld[:, 0] * ld[:, 0] + ld[:, 1] * ld[:, 1] + ld[:, 2] * ld[:, 2]))[:, None]
    r1 = np.abs(r).sum(axis=1)
    counts, sums, bound, hits = np.zeros(len(offsets), dtype=np.int64), np.zeros((len(offsets), 6)), np.zeros((len(offsets), 6)), []
    margin = np.inf
    for j, off in enumerate(offsets):
        ox = lo[:, 0] - off
        moving = ld[:, 0] != 0.0  # (a NaN direction "moves" and fails every comparison below, as on the device)
        with np.errstate(all="ignore"):
            t = -ox / ld[:, 0]
            refused = (np.abs(t) < 1e-9) | (t < 0.0) | (t > length)
            crosses = moving & ~refused
            Px, Py, Pz = ox + t * ld[:, 0], lo[:, 1] + t * ld[:, 1], lo[:, 2] + t * ld[:, 2]
            hit = crosses & (np.abs(Py) <= half_width) & (np.abs(Pz) <= half_height)
            tm = t[moving & np.isfinite(t)]
            lm = length[moving & np.isfinite(t)]
            if len(tm):
                margin = min(margin, np.abs(tm - lm).min(), np.abs(np.abs(tm) - 1e-9).min(), np.abs(tm).min())
            if crosses.any():
                margin = min(margin, np.abs(np.abs(Py[crosses]) - half_width).min(), np.abs(np.abs(Pz[crosses]) - half_height).min())
        hits.append(index[hit])
        c = int(hit.sum())
        counts[j] = c
        if not c:
            continue
        Px, Py, Pz, wh = Px[hit], Py[hit], Pz[hit], w[hit]
        y = Px * axes[0] + Py * axes[1] + Pz * axes[2] - centre[0]
        z = Px * axes[3] + Py * axes[4] + Pz * axes[5] - centre[1]
        S = ((r1[hit] + np.abs(t[hit])) / np.abs(ld[hit, 0])).max() + abs(centre[0]) + abs(centre[1])
        dl = 128 * U * S
        aw, ay, az = np.abs(wh), np.abs(y), np.abs(z)
        terms = (wh, wh * y, wh * z, wh * y * y, wh * z * z, wh * y * z)
        own = (0.0, aw * dl + U * aw * ay, aw * dl + U * aw * az, aw * (2 * ay * dl + dl * dl) + 2 * U * aw * ay * ay,
               aw * (2 * az * dl + dl * dl) + 2 * U * aw * az * az, aw * ((ay + az) * dl + dl * dl) + 2 * U * aw * ay * az)
        for k, (term, err) in enumerate(zip(terms, own)):
            sums[j, k] = math.fsum(term)
            bound[j, k] = math.fsum(np.broadcast_to(err, term.shape)) + (c + 2) * U * math.fsum(np.abs(term))
    return Spots(counts, sums, bound, float(margin), hits)


def variance_bound(sums, bound):
    """(var_r, its tolerance) of one plane: var_r = var_y + var_z from `sums` (6 values), and how far sums within `bound` of them
    can move it, to first order in the bounds: var_y = Wyy / W - (Wy / W)^2 moves by at most
    (dWyy + |Wyy / W| dW) / W + 2 |Wy / W| (dWy + |Wy / W| dW) / W, and 4 U (|Wyy / W| + (Wy / W)^2) for its own roundings."""
    W, Wy, Wz, Wyy, Wzz, _ = (float(v) for v in sums)
    dW, dWy, dWz, dWyy, dWzz, _ = (float(v) for v in bound)
    var, err = 0.0, 0.0
    for first, second, d1, d2 in ((Wy, Wyy, dWy, dWyy), (Wz, Wzz, dWz, dWzz)):
        mean, square = first / W, second / W
        var += max(square - mean * mean, 0.0)
        err += (d2 + abs(square) * dW) / abs(W) + 2 * abs(mean) * (d1 + abs(mean) * dW) / abs(W) + 4 * U * (abs(square) + mean * mean)
    return var, err


def radius_interval(sums, bound):
    """[lowest, highest] rms radius sqrt(var_r) that sums within `bound` of `sums` allow (`variance_bound`)."""
    var, err = variance_bound(sums, bound)
    return math.sqrt(max(var - err, 0.0)), math.sqrt(var + err)
