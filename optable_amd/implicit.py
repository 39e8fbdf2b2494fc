"""Device form of a user's implicit surface: a verified 3-D Chebyshev series of f over its local box.

The reference traces any `Surface` subclass through four methods — `f(P) = 0`, `normal(P)`, `within_boundary(P)`,
`get_bbox_local()` (surfaces.py:5-65) — with a 10-point sign scan of f along the ray inside the local box and brentq
(optical_component.py:126-134, 198-233).  The kernels cannot call Python, so with `implicit_surfaces=True` the scene
compiler MEASURES such a surface (non-planar only) and hands the device

  * a tensor Chebyshev series of f over the box (padded by a relative 1e-9: the scan samples just outside it), fitted at
    Chebyshev nodes axis by axis and VERIFIED against the user's f on points the fit has not seen, to REL_TOL of max|f|;
  * the series of df/dx, df/dy, df/dz (chebder on the host): the normal (the root polish is derivative-free);
  * the sign s with which the user's `normal(P)` equals s grad f / |grad f|, checked on surface points;
  * which of four aperture families the user's `within_boundary` is on those surface points (the box, the disc
    inscribed in the box's yz face, the rectangle of that face, |P| <= R as `Circle` has it).

Anything else is refused with the measured reason; there is no host fallback.  Sampling limit of the aperture
measurement: N_SURFACE surface points see a hole or notch that covers more than about 1/N_SURFACE of the surface in the
box; a smaller feature (a round hole of radius ~1 % of the aperture) can go unseen.  `OpticalTable.ray_tracing` checks
every hit on such a surface against the user's `within_boundary` and `f` and raises when they disagree; `trace_batch`
does not check, and opting in is the user's acceptance there.

Cost on the device: one evaluation of f is nx * ny * nz fused multiply-adds (three nested Clenshaw recurrences); the ten
scan samples and the false-position polish evaluate f alone, the normal of a hit the three gradient blocks.
"""
import numpy as np

from . import cheb, shapes

HEADER = 20                     # == OT_IMPLICIT_HEADER (include/optable_hip.h)
APERTURE_BOX, APERTURE_DISC, APERTURE_RECT, APERTURE_BALL = range(4)  # == ot_implicit_aperture
APERTURE_NAMES = ("box", "disc", "rectangle", "ball")
# The 1-D fits hold 5e-14 of the range (cheb.REL_TOL); a tensor fit of f in fp64 is limited by the rounding of f itself at
# the n^3 nodes, ~1e-14 for a quartic.  1e-12 of max|f| moves a root by 1e-12 of max|f| / |grad f| — about 1e-12 of the box
# size for a surface that crosses its box — a thousand times inside the 1e-9 of the fp64 parity tests.
REL_TOL = 1e-12
DEGREES = (8, 12, 16, 24, 32, 48)  # terms per axis, grown axis by axis
MAX_TERMS = 48
MAX_COEFFS = 16384              # per block
PAD = 1e-9                      # relative padding of the fit box
N_VERIFY = 4096                 # random box points of the verification
N_SURFACE = 2048                # surface points of the normal and aperture measurements
NORMAL_TOL = 2e-7               # |normal(P) - s grad f / |grad f||, unit vectors (as the measured surfaces of adapter.py)
APERTURE_SLACK = 1e-12          # relative widening of the box / disc / ball apertures (the reference's 1e-12, surfaces.py:300-378)


class ImplicitError(NotImplementedError):
    pass


class Fit:
    """The measured device form (`record()` is the aux record) and what was measured."""

    def __init__(self, coef, lo, hi, err, fmax):
        self.coef, self.lo, self.hi, self.err, self.fmax = coef, lo, hi, err, fmax
        self.sign, self.aperture, self.radius = 1.0, APERTURE_BOX, 0.0
        self.box = None

    @property
    def degrees(self):
        return tuple(n - 1 for n in self.coef.shape)

    @property
    def rel_err(self):
        return self.err / self.fmax

    def gradient_blocks(self):
        half = 0.5 * (self.hi - self.lo)
        out = []
        for a in range(3):
            d = np.polynomial.chebyshev.chebder(self.coef, axis=a) / half[a] if self.coef.shape[a] > 1 else np.zeros_like(self.coef)
            pad = [(0, 0)] * 3
            pad[a] = (0, self.coef.shape[a] - d.shape[a])
            out.append(np.pad(d, pad))
        return out

    def evaluate(self, P, block=0):
        """Host evaluation of block `block` (0: f, 1..3: df/dx..dz) at P of shape (3, M)."""
        c = self.coef if block == 0 else self.gradient_blocks()[block - 1]
        t = [(np.asarray(P[a], dtype=float) - 0.5 * (self.lo[a] + self.hi[a])) / (0.5 * (self.hi[a] - self.lo[a])) for a in range(3)]
        return np.polynomial.chebyshev.chebval3d(t[0], t[1], t[2], c)

    def record(self):
        centre, half = 0.5 * (self.lo + self.hi), 0.5 * (self.hi - self.lo)
        nx, ny, nz = self.coef.shape
        slack = APERTURE_SLACK * max(1.0, float(np.abs(self.box).max()))
        abox = self.box + slack * np.array([-1, 1, -1, 1, -1, 1])
        r2 = (self.radius * (1 + APERTURE_SLACK) + slack) ** 2 if self.aperture in (APERTURE_DISC, APERTURE_BALL) else 0.0
        head = [nx, ny, nz, *centre, *(1.0 / half), self.sign, self.aperture, r2, *abox, self.rel_err, self.fmax]
        assert len(head) == HEADER
        blocks = [self.coef] + self.gradient_blocks()
        return [float(v) for v in head] + [float(v) for b in blocks for v in np.ravel(b)]


def _nodes(n):
    return np.cos(np.pi * (np.arange(n) + 0.5) / n)


def _fit_matrix(n):
    """c = A @ values at the n Chebyshev nodes (discrete orthogonality of T_k on those nodes)."""
    A = (2.0 / n) * np.polynomial.chebyshev.chebvander(_nodes(n), n - 1).T
    A[0] *= 0.5
    return A


def _sampler(surf, what):
    """f on points of shape (3, M).  Vectorised when the user's f takes arrays and agrees with its own scalar calls on 16
    points; point by point otherwise (user functions need not take arrays, cheb._sample)."""
    def scalar(P):
        out = np.empty(P.shape[1])
        for k in range(P.shape[1]):
            out[k] = float(surf.f(np.array(P[:, k])))
        return out

    def guarded(fn):
        def call(P):
            try:
                return fn(P)
            except ImplicitError:
                raise
            except Exception as exc:  # noqa: BLE001 - the user's f failed: that is the message
                raise ImplicitError(f"{what}: f raised {type(exc).__name__}: {exc}") from exc
        return call

    def probe(P):
        try:
            v = np.asarray(surf.f(P), dtype=float)
        except Exception:  # noqa: BLE001
            return None
        return v if v.shape == (P.shape[1],) else None

    def choose(P):
        v = probe(P)
        if v is None:
            return guarded(scalar)
        ref = scalar(P[:, :16])
        ok = np.allclose(v[:16], ref, rtol=1e-13, atol=1e-13 * max(1e-300, float(np.nanmax(np.abs(ref)))), equal_nan=True)
        return guarded((lambda Q: np.asarray(surf.f(Q), dtype=float).reshape(Q.shape[1])) if ok else scalar)

    state = {}

    def sample(P):
        if "fn" not in state:
            state["fn"] = choose(P) if P.shape[1] >= 16 else guarded(scalar)
        return state["fn"](P)

    return sample


def _grid(lo, hi, ns):
    axes = [0.5 * (lo[a] + hi[a]) + 0.5 * (hi[a] - lo[a]) * _nodes(ns[a]) for a in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()])


def _coefficients(vals, ns):
    c = vals.reshape(ns)
    for a in range(3):  # separable: one 1-D fit matrix per axis
        c = np.moveaxis(np.tensordot(_fit_matrix(ns[a]), c, axes=([1], [a])), 0, a)
    return c


def _tail(c, a, k=2):
    """Largest coefficient among the last k along axis a."""
    n = c.shape[a]
    return float(np.abs(np.take(c, range(max(0, n - k), n), axis=a)).max())


def _trim(c, floor):
    for a in range(3):
        keep = c.shape[a]
        while keep > 1 and float(np.abs(np.take(c, [keep - 1], axis=a)).max()) <= floor:
            keep -= 1
        c = np.take(c, range(keep), axis=a)
    return c


def fit(surf, box, what="implicit surface", rel_tol=REL_TOL, seed=20261016):
    """Fit and verify the series of surf.f over `box` (x0, x1, y0, y1, z0, z1).  Returns a Fit, or raises ImplicitError."""
    box = np.asarray(box, dtype=float)
    lo, hi = box[0::2].copy(), box[1::2].copy()
    width = hi - lo
    if not np.all(np.isfinite(box)) or np.any(width <= 0):
        raise ImplicitError(f"{what}: its local box {tuple(box.tolist())} is degenerate (a non-planar surface needs a box "
                            "of positive width on every axis)")
    pad = PAD * max(float(width.max()), float(np.abs(box).max()))
    lo, hi = lo - pad, hi + pad
    sample = _sampler(surf, what)
    rng = np.random.default_rng(seed)
    ns, prev_tail = [DEGREES[0]] * 3, None
    while True:
        vals = sample(_grid(lo, hi, ns))
        if not np.all(np.isfinite(vals)):
            raise ImplicitError(f"{what}: f is not finite everywhere in its box (a pole or a point where it is undefined)")
        fmax = max(float(np.abs(vals).max()), 1e-300)
        c = _coefficients(vals, ns)
        floor = 0.05 * rel_tol * fmax
        tails = [_tail(c, a) for a in range(3)]
        grow = [a for a in range(3) if tails[a] > floor]
        if not grow:
            break
        nxt = list(ns)
        for a in grow:
            later = [n for n in DEGREES if n > ns[a]]
            if not later:
                kink = prev_tail is not None and any(tails[a] > 0.05 * prev_tail[a] for a in grow)
                cause = ("the coefficients decay only algebraically: a kink or a jump of f or of a derivative in the box"
                         if kink else f"the degree cap of {MAX_TERMS} terms per axis")
                raise ImplicitError(f"{what}: no tensor Chebyshev series reproduces f over its box ({cause}; trailing "
                                    f"coefficients {max(tails) / fmax:.1e} of max|f|, needed {rel_tol:.0e})")
            nxt[a] = later[0]
        if int(np.prod(nxt)) > MAX_COEFFS:
            raise ImplicitError(f"{what}: f needs more than {MAX_COEFFS} coefficients ({nxt[0]} x {nxt[1]} x {nxt[2]} terms): "
                                "the degree cap; a smaller box or a smoother f")
        prev_tail, ns = tails, nxt
    c = _trim(c, floor)
    out = Fit(c, lo, hi, 0.0, fmax)
    out.box = box
    # verification on points the fit has not seen: random box points, and points near the surface (below)
    P = lo[:, None] + (hi - lo)[:, None] * rng.random((3, N_VERIFY))
    fv = sample(P)
    if not np.all(np.isfinite(fv)):
        raise ImplicitError(f"{what}: f is not finite everywhere in its box (a pole or a point where it is undefined)")
    out.fmax = fmax = max(fmax, float(np.abs(fv).max()))
    err = float(np.abs(out.evaluate(P) - fv).max())
    S = surface_points(out, rng, N_SURFACE // 4)
    if S.shape[1]:
        near = S + (1e-3 * width)[:, None] * rng.standard_normal(S.shape)
        near = np.clip(near, lo[:, None], hi[:, None])
        err = max(err, float(np.abs(out.evaluate(near) - sample(near)).max()))
    out.err = err
    if not err <= rel_tol * fmax:
        raise ImplicitError(f"{what}: the series of f misses f by {err / fmax:.1e} of max|f| on points between the nodes "
                            f"(needed {rel_tol:.0e}): f is not smooth enough for a device form (a kink or a steep feature)")
    return out


def surface_points(fit_, rng, n, chords=None):
    """Up to n points on the series' zero set: a vectorised sign scan of the series along random chords of the box (through
    two uniform points), each crossing polished by bisection."""
    lo, hi = fit_.lo, fit_.hi
    pts, tries = [], 0
    total = 0
    while total < n and tries < 8:
        tries += 1
        m = chords or max(256, n)
        a = lo[:, None] + (hi - lo)[:, None] * rng.random((3, m))
        b = lo[:, None] + (hi - lo)[:, None] * rng.random((3, m))
        s = np.linspace(-1.0, 2.0, 33)  # along a + s (b - a): the chord through a and b, well past both
        Q = a[:, :, None] + (b - a)[:, :, None] * s[None, None, :]
        inside = np.all((Q >= lo[:, None, None]) & (Q <= hi[:, None, None]), axis=0)
        g = fit_.evaluate(Q.reshape(3, -1)).reshape(m, len(s))
        cross = (g[:, :-1] * g[:, 1:] < 0) & inside[:, :-1] & inside[:, 1:]
        ci, cj = np.nonzero(cross)
        if not len(ci):
            continue
        sl, sr, gl = s[cj].copy(), s[cj + 1].copy(), g[ci, cj]
        A, D = a[:, ci], (b - a)[:, ci]
        for _ in range(60):
            sm = 0.5 * (sl + sr)
            gm = fit_.evaluate(A + D * sm)
            left = np.sign(gm) == np.sign(gl)
            sl, gl = np.where(left, sm, sl), np.where(left, gm, gl)
            sr = np.where(left, sr, sm)
        pts.append(A + D * (0.5 * (sl + sr)))
        total += len(ci)
    if not pts:
        return np.zeros((3, 0))
    return np.concatenate(pts, axis=1)[:, :n]


def _vector_calls(fn, P, width):
    out = np.empty((P.shape[1], width) if width else P.shape[1])
    for k in range(P.shape[1]):
        out[k] = np.asarray(fn(np.array(P[:, k])), dtype=float) if width else bool(fn(np.array(P[:, k])))
    return out


def measure(surf, what="implicit surface"):
    """Fit, then measure normal sign and aperture family on surface points.  Returns the Fit, or raises ImplicitError."""
    try:
        box = np.array([float(v) for v in surf.get_bbox_local()])
    except Exception as exc:  # noqa: BLE001
        raise ImplicitError(f"{what}: get_bbox_local() failed ({exc})") from exc
    if box.shape != (6,):
        raise ImplicitError(f"{what}: its local box is not six numbers")
    out = fit(surf, box, what)
    rng = np.random.default_rng(7)
    S = surface_points(out, rng, N_SURFACE)
    if S.shape[1] < N_SURFACE // 4:
        raise ImplicitError(f"{what}: its zero set barely crosses its local box ({S.shape[1]} points found on random chords)")
    try:
        fu = np.array([float(surf.f(np.array(S[:, k]))) for k in range(S.shape[1])])
        nu = _vector_calls(surf.normal, S, 3)
        inside = _vector_calls(surf.within_boundary, S, 0).astype(bool)
    except Exception as exc:  # noqa: BLE001
        raise ImplicitError(f"{what}: probing it on its surface failed ({type(exc).__name__}: {exc})") from exc
    if not np.all(np.abs(fu) <= 4 * REL_TOL * out.fmax):
        raise ImplicitError(f"{what}: f is not small at the series' roots ({float(np.abs(fu).max()) / out.fmax:.1e} of max|f|)")
    # normal: the user's normal(P) against s grad f / |grad f|, one sign s for every point
    g = np.stack([out.evaluate(S, b) for b in (1, 2, 3)], axis=1)
    gn = np.linalg.norm(g, axis=1)
    if not np.all(gn > 1e-9 * out.fmax / float(np.max(out.hi - out.lo))):
        raise ImplicitError(f"{what}: grad f vanishes on its surface (a singular point): the normal is undefined there")
    unit = g / gn[:, None]
    dots = np.einsum("ij,ij->i", nu, unit)
    sign = 1.0 if dots[0] >= 0 else -1.0
    off = np.linalg.norm(nu - sign * unit, axis=1)
    if not np.all(off <= NORMAL_TOL):
        k = int(np.argmax(off))
        raise ImplicitError(f"{what}: its normal(P) is not {'+' if sign > 0 else '-'}grad f / |grad f| with one sign for the "
                            f"whole surface (off by {off[k]:.1e} at P = {S[:, k].round(6).tolist()})")
    out.sign = sign
    # aperture: one of four families, equal to the user's within_boundary on every surface point
    bx = box
    slack = APERTURE_SLACK * max(1.0, float(np.abs(bx).max()))
    cy, cz = 0.5 * (bx[2] + bx[3]), 0.5 * (bx[4] + bx[5])
    R = 0.5 * min(bx[3] - bx[2], bx[5] - bx[4])
    x, y, z = S
    in_rect = (y >= bx[2] - slack) & (y <= bx[3] + slack) & (z >= bx[4] - slack) & (z <= bx[5] + slack)
    candidates = [
        (APERTURE_BOX, in_rect & (x >= bx[0] - slack) & (x <= bx[1] + slack)),
        (APERTURE_DISC, (y - cy) ** 2 + (z - cz) ** 2 <= (R + slack) ** 2),
        (APERTURE_RECT, in_rect),
        (APERTURE_BALL, x * x + y * y + z * z <= (R + slack) ** 2),
    ]
    for kind, mask in candidates:
        if np.array_equal(mask, inside):
            out.aperture, out.radius = kind, (R if kind in (APERTURE_DISC, APERTURE_BALL) else 0.0)
            return out
    raise ImplicitError(f"{what}: its within_boundary is none of the aperture families (the box, the disc inscribed in the "
                        f"box's yz face, the rectangle of that face, |P| <= R) on {S.shape[1]} surface points (features "
                        f"covering less than about 1/{S.shape[1]} of the surface are not resolved)")


def lower(surf):
    """shapes.Lowered for a non-planar user surface, or ImplicitError."""
    what = f"user-defined surface {type(surf).__name__}"
    return shapes.Lowered(shapes.IMPLICIT_CHEB, aux=measure(surf, what).record(), planar=False)


def record_gradient(rec, P):
    """grad f of an aux record (Fit.record layout) at the local point P, on the host: the run-time check of ray_tracing."""
    nx, ny, nz = (int(v) for v in rec[:3])
    centre, inv = np.asarray(rec[3:6], dtype=float), np.asarray(rec[6:9], dtype=float)
    t = (np.asarray(P, dtype=float) - centre) * inv
    n = nx * ny * nz
    return np.array([np.polynomial.chebyshev.chebval3d(t[0], t[1], t[2],
                                                       np.asarray(rec[HEADER + b * n:HEADER + (b + 1) * n]).reshape(nx, ny, nz))
                     for b in (1, 2, 3)])
