"""Shared test support: the fixtures and helpers the GPU and CPU test modules have in common.  Importing it touches neither the
device nor the built library; everything that does runs when a test calls it.  Bounds, references and each entry point's own
`_call` stay in the module that tests them."""
import ctypes as C

import numpy as np
import pytest
import torch

import optable_amd as oa
import scenes
from optable_amd import abi
from optable_amd.batch import RayBatch, SegmentBatch

# -- 1: scenes, monitors, rays ---------------------------------------------------------------------------------------------------
Q = 1j * np.pi * scenes.W0**2 / scenes.WL


def table_of(components):
    t = oa.OpticalTable()
    t.add_components(components)
    return t


def cfg2_table():
    return table_of(scenes.cfg2_components(oa))


def six_monitors():
    return [oa.Monitor([7.5, 0, 0], 6, 6),             # the one tests/test_gpu_append.py shows is hit
            oa.Monitor([6.5, 0, 0], 6, 6),
            oa.Monitor([7.5, 40, 0], 6, 6),            # where no segment passes: an empty list, an all-zero image
            oa.Monitor([8.5, 0, 0], 6, 6),
            oa.Monitor([7.5, 0, 0], 6, 6).RotZ(0.3),
            oa.Monitor([7.5, 0, 0], 0.5, 0.5)]         # clips


def eight_monitors():
    return six_monitors() + [oa.Monitor([7.5, 0, 0], 0.4, 6).RotX(0.5),  # the lab-tangent projection leaves the image range: the drop rule runs
                             oa.Monitor([7.5, 0, 0], 2, 2)]              # the beam over some 430 bins instead of 60


def half_mirror(ns):
    return [ns.Lens([5, 0, 0], focal_length=5, radius=1.0), ns.MirrorPair([10, 0, 0], 4, 4, reflectivity_1=0.5)]


def lattice(k_max=3):
    """The compiled scene of `k_max` cells of two beam splitters and a mirror: bushy ray trees."""
    comps = []
    for k in range(k_max):
        comps.append(oa.BeamSplitter([2.0 * (k + 1), 0, 0], width=6, height=2, eta=0.5).RotZ(np.pi / 4))
        comps.append(oa.Mirror([2.0 * (k + 1), 3.0 + 0.1 * k, 0], radius=2).RotZ(-np.pi / 2))
        comps.append(oa.BeamSplitter([2.0 * (k + 1) + 1.0, 1.5, 0], width=6, height=2, eta=0.3).RotZ(-np.pi / 4))
    return table_of(comps).compile()


def weighted_batch(o, d, precision="f64", seed=7, device="cuda"):
    """The rays with per-ray intensities 0.25 + 0.75 u: the weight channel is no copy of the counts."""
    intensity = 0.25 + 0.75 * np.random.default_rng(seed).random(len(o))
    return RayBatch.from_arrays(o, d, wavelength=scenes.WL, intensity=intensity, q=Q, precision=precision, device=device)


def waisted_batch(o, d, precision="f64", seed=7):
    """The rays with per-ray intensities 0.25 + 0.75 u and per-ray waists w0 log-uniform in [0.005, 2]."""
    rng = np.random.default_rng(seed)
    intensity = 0.25 + 0.75 * rng.random(len(o))
    w0 = np.exp(rng.uniform(np.log(0.005), np.log(2.0), len(o)))
    return RayBatch.from_arrays(o, d, wavelength=scenes.WL, intensity=intensity, q=1j * np.pi * w0**2 / scenes.WL, precision=precision, device="cuda")


def batch(o, d, precision="f64", **kw):
    kw.setdefault("wavelength", scenes.WL)
    kw.setdefault("q", Q)
    return RayBatch.from_arrays(o, d, precision=precision, device="cuda", **kw)


def short_rays(n):
    """cfg 2's rays (seed 0) with the rays of wave 0 and every other ray of wave 1 aimed past the lens: they miss everything (1
    segment) or meet the roof mirrors alone (2 or 3).  Wave 0 is a whole wave of short rays, wave 1 a mixed one, the rest goes the
    whole path.  Returns (o, d, the indices of the short rays)."""
    o, d = scenes.cfg2_rays(n, 0)
    idx = np.concatenate([np.arange(0, 64), np.arange(64, 128, 2)])
    idx = idx[idx < n]
    tan = np.linspace(0.21, 0.6, idx.size)  # past the lens's rim (radius 1 at x = 5) from tan = 0.2 on
    d[idx] = np.stack([np.ones(idx.size), tan, np.zeros(idx.size)], axis=1)
    d[idx[::4]] = [0.0, 1.0, 0.0]  # and straight up: nothing there
    return o, d, idx


def around(edges):
    """Every edge, and the doubles just below and above every one of them (the outer edges' outer neighbours lie outside)."""
    return np.unique(np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)]))


def host(t):
    return t.double().cpu().numpy()


def hit_wavelengths(wavelength, h):
    """The wavelength of every hit of `h` (reference order): a float, or the traced RayBatch's by the hits' ray."""
    if isinstance(wavelength, RayBatch):
        return host(wavelength.wavelength)[h.ray_index(None).cpu().numpy()]
    return np.full(len(h), float(wavelength))


# -- 2: compiled-scene cache -----------------------------------------------------------------------------------------------------
_compiled = {}


def engine_for(components_fn, key):
    """The engine with the scene `components_fn(oa)` uploaded; compiled once per `key`."""
    from optable_amd.engine import get_engine

    if key not in _compiled:
        _compiled[key] = table_of(components_fn(oa)).compile()
    eng = get_engine()
    eng.upload(_compiled[key])
    return eng


# -- 3: record views -------------------------------------------------------------------------------------------------------------
ALL_FIELDS = abi.SEG_FIELDS + ("ray", "surface")


def bits(t):
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def planes(segs, n, K, fields=ALL_FIELDS):
    """every field as bit patterns [K, n], `count`, and which slots hold records"""
    s = segs.to_slots()
    out = {f: bits(s.field(f)[: K * n]).view(K, n).clone() for f in fields}
    count = segs.count.clone()
    return out, count, torch.arange(K, device=count.device)[:, None] < count.abs()[None, :]


def valid_records(segs, n, K):
    """every field of the valid slots as bit patterns, plus count"""
    out, count, valid = planes(segs, n, K)
    out = {f: plane[valid] for f, plane in out.items()}
    out["count"] = count
    return out


def host_records(segs, *extra):
    """The valid segment records of a batch, copied from the device: (o [n, 3], d [n, 3], length, intensity) as doubles (single
    precision widens exactly), then the fields named in `extra`: doubles too, `ray` as int64."""
    h = segs.to_host(reference_order=False)
    col = lambda f: np.asarray(h[f], dtype=np.int64 if f == "ray" else np.float64)  # noqa: E731
    return (np.stack([col("ox"), col("oy"), col("oz")], 1), np.stack([col("dx"), col("dy"), col("dz")], 1), col("length"), col("intensity"),
            *(col(f) for f in extra))


def same_records(got, want, what, fields=ALL_FIELDS):
    (g, gc, valid), (w, wc, wvalid) = got, want
    assert torch.equal(gc, wc), (what, "count", gc.cpu().tolist(), wc.cpu().tolist())
    assert torch.equal(valid, wvalid), (what, "slots in use")
    for f in fields:
        assert torch.equal(g[f][valid], w[f][valid]), (what, f)


# -- 4: outputs and poison -------------------------------------------------------------------------------------------------------
POISON_BYTE = 0xA5
POISON_REAL, POISON_INT = 123.0, -7


def new_out(n, K, precision, layout, poison_byte=None, zero_count=False):
    """a fresh output; with `poison_byte` every byte of it, a tile's padding included, is poisoned (a write torch sees: there is no
    token yet); with `zero_count`, for calls through the C ABI, it says that it holds no old records"""
    out = SegmentBatch(n * K, precision, "cuda", tiled=(layout == "tiled"))
    if poison_byte is not None:
        if out.tiled:
            out.block.fill_(poison_byte)
        else:
            for f in ALL_FIELDS:
                out.field(f).view(torch.uint8).fill_(poison_byte)
    if zero_count:
        out.count, out.n_rays = torch.zeros(n, dtype=torch.int32, device="cuda"), n
    return out


def byte_poison(plane):
    return bits(torch.full((plane.element_size(),), POISON_BYTE, dtype=torch.uint8, device=plane.device).view(plane.dtype))


def value_poison(plane, f):
    dt = torch.int32 if f in ("ray", "surface") else {torch.int64: torch.float64, torch.int32: torch.float32}[plane.dtype]
    return bits(torch.full((1,), POISON_INT if dt == torch.int32 else POISON_REAL, dtype=dt, device=plane.device))


def poison_behind_torch(out, fields=ALL_FIELDS):
    """through .data: torch does not see the write, the tokens of a reused output stay"""
    for f in fields:
        out.field(f).data.fill_(POISON_INT if f in ("ray", "surface") else POISON_REAL)


def untouched_beyond_the_counts(out, n, K, what, fields=ALL_FIELDS):
    """an output poisoned byte by byte before its first trace: slots k >= |count| and a tiled block's padding hold the poison"""
    valid = (torch.arange(K, device="cuda")[:, None] < out.count.abs()[None, :]).reshape(-1)
    for f in fields:
        flat = bits(out.field(f).reshape(-1))
        poison = byte_poison(flat)
        assert bool((flat[: K * n][~valid] == poison).all()), (what, f, "a slot past a ray's count was written")
        if out.tiled:
            assert out.capacity % 64 == 0 and flat.numel() == out.capacity
            assert bool((flat[K * n:] == poison).all()), (what, f, "the last tile's padding was written")


class Sentinel:
    """Device outputs for a call through the C ABI, filled with a sentinel: `name=(dtype, shape)` gives the view `self.name`, with
    `guard` more sentinel elements on either side of it."""

    def __init__(self, guard=0, fill=-7, **specs):
        self.fill, self._guard, self._whole = fill, guard, []
        for name, (dtype, shape) in specs.items():
            size = int(np.prod(shape))
            whole = torch.full((size + 2 * guard,), fill, dtype=dtype, device="cuda")
            self._whole.append(whole)
            setattr(self, name, whole[guard:guard + size].view(shape))

    def untouched(self):
        return all(bool((t == self.fill).all()) for t in self._whole)

    def guards_untouched(self):
        G = self._guard
        return all(bool((t[:G] == self.fill).all()) and bool((t[t.numel() - G:] == self.fill).all()) for t in self._whole)


# -- 5: hand-made segment lists --------------------------------------------------------------------------------------------------
def list_segments(n, /, **fields):
    """A list of n double-precision segments on the device: every field zero except those given (an array or one value for all),
    `ray` = 0 .. n - 1."""
    segs = SegmentBatch(n, "f64", "cuda")
    for f in abi.SEG_FIELDS:
        segs.field(f).zero_()
    for f, v in fields.items():
        if np.ndim(v) == 0:
            segs.field(f).fill_(float(v))
        else:
            segs.field(f).copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)))
    segs.ray.copy_(torch.arange(n, dtype=torch.int32))
    segs.n_valid = n
    assert segs.layout == "list"
    return segs


def list_batch(o, d, length, intensity):
    return list_segments(len(o), ox=o[:, 0], oy=o[:, 1], oz=o[:, 2], dx=d[:, 0], dy=d[:, 1], dz=d[:, 2], length=length, intensity=intensity)


# -- 6: the C ABI ----------------------------------------------------------------------------------------------------------------
ERR_INVALID = -1


@pytest.fixture()
def ctx():
    lib = abi.load()
    c = C.c_void_p()
    assert lib.ot_ctx_create(0, None, C.byref(c)) == 0
    yield lib, c
    assert lib.ot_ctx_destroy(c) == 0


def image_tables(mons, nby, nbz):
    """(axes [M, 6], edges [M, nby + nbz + 2]) of the monitors' images, as ot_monitor_image_many and its kin read them"""
    from optable_amd.monitors import image_edges

    axes = np.array([np.concatenate([m.tangent_Y, m.tangent_Z]) for m in mons], dtype=float)
    edges = np.array([np.concatenate(image_edges(m, nby, nbz)) for m in mons], dtype=float)
    return axes, edges


def altered(src, **fields):
    """a copy of the OtSegmentSource `src` with the given members set"""
    other = abi.OtSegmentSource.from_buffer_copy(src)
    for k, v in fields.items():
        setattr(other, k, v)
    return other


def expect_invalid(lib, status, needle):
    msg = lib.ot_last_error().decode()
    assert status == ERR_INVALID and needle in msg, (status, msg, needle)


def trace_call(eng, family, batch, K, out, layout, *masks):
    """ot_trace[_tiled]_<family>_f64/_f32 on `out`, straight through the C ABI; returns the status"""
    rs = batch.c_struct()
    if layout == "tiled":
        where = (out.block.data_ptr(), out.capacity)
        fn = eng._fn("ot_trace_tiled_" + family, batch.precision)
    else:
        ss = out.c_struct()
        where = (C.byref(ss),)
        fn = eng._fn("ot_trace_" + family, batch.precision)
    return fn(eng._ctx, C.byref(rs), batch.n, K, *where, out.count.data_ptr(), None, 0, *masks)


# -- 7: traced-case cache --------------------------------------------------------------------------------------------------------
def traced(table, make_batch, K, derive):
    """get(layout, precision="f64") -> (segs, derive(segs)): `make_batch(precision)` traced through `table` with `K` segments a ray
    on first use, and kept."""
    made = {}

    def get(layout, precision="f64"):
        if (layout, precision) not in made:
            segs = table.trace_batch(make_batch(precision), max_segments=K, layout=layout)
            assert segs.layout == layout and segs.precision == precision
            made[layout, precision] = (segs, derive(segs))
        return made[layout, precision]

    return get


# -- 8: the CPU side -------------------------------------------------------------------------------------------------------------
def host_segments(n_rays=4, k=2, precision="f64"):
    segs = SegmentBatch(n_rays * k, precision, "cpu")
    segs.count, segs.n_rays = torch.full((n_rays,), k, dtype=torch.int32), n_rays
    return segs


def host_rays(n, **kw):
    o = np.zeros((n, 3))
    d = np.tile([1.0, 0.0, 0.0], (n, 1))
    return RayBatch.from_arrays(o, d, wavelength=780e-7, device="cpu", **kw)


def host_out(n, K, precision="f64", tiled=False):
    """a host output that says it holds K records of each of n rays"""
    out = SegmentBatch(n * K, precision, "cpu", tiled=tiled)
    out.count = torch.full((n,), K, dtype=torch.int32)
    out.n_rays = n
    return out
