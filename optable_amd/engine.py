"""Python handle on the HIP trace engine (one `ot_ctx` per device).

Everything that touches rays goes through liboptable_hip.so; this module only moves
pointers.  If the library or a GPU is missing the constructor raises — there is no CPU path.
"""
import contextlib
import ctypes as C
import threading
import time

import numpy as np
import torch

from . import abi
from .batch import RayBatch, SegmentBatch

_engines = {}


# -- how large an append-layout block has to be: every rule in one place, plain integers in and out -------------------
# Per-wave lists: every wave claims `chunk` slots at a time (OT_OPT_APPEND_CHUNK) and may leave the tail of its last chunk
# unused.  Block pool (bit 4 of `pair_queue`): a workgroup fills one chunk of `_wg_chunk(chunk)` slots at a time, loses at most
# 63 slots where a pass crosses into the next chunk (`_pool_holes`) and leaves the tail of its last chunk unused.
def _wg_chunk(chunk):
    return min(16 * chunk, 1 << 19)


def _pool_holes(n_records, wg_chunk):
    return 64 * (n_records // (wg_chunk - 64) + 1)


def _round64(slots):
    return (slots + 63) // 64 * 64


def append_slots(n_records, launch, chunk=512):
    """Slots an append-layout block needs for `n_records` segment records written by a launch of shape `launch`
    (`Engine.last_launch()`), holes included, per-wave lists or block pool as the launch was.  A multiple of 64."""
    n_records, chunk = int(n_records), int(chunk)
    if launch["kernel"] == 2 and launch["pair_queue"] & 16:
        wg_chunk = _wg_chunk(chunk)
        slots = n_records + _pool_holes(n_records, wg_chunk) + (wg_chunk + 64) * max(launch["workgroups"], 1)
    else:
        waves = max(launch["workgroups"] * launch["threads"] // 64, 1) if launch["kernel"] == 2 else 256 * 16
        slots = n_records + chunk * waves
    return _round64(slots)


def append_worst_case(n, K, chunk, max_waves, pool=True):
    """Slots that hold the records of ANY trace of n rays capped at K records each, holes included, before the launch shape is
    known.  `max_waves`: most waves the launch can have.  pool=True (ot_trace_append_*, which picks per-wave lists or the block
    pool itself): the tail of every wave's last chunk (one wave per ticket of 64 rays at most) or, with the pool (curved
    scenes, fp32), 63 slots per workgroup chunk and the last chunk of every workgroup, whichever is more.  pool=False
    (ot_trace_trees_append_*): per-wave lists only, and `max_waves` is the launch's own wave count (`Engine.trees_plan`)."""
    if not pool:
        return n * K + chunk * max_waves
    wg_chunk = _wg_chunk(chunk)
    waves = min(max_waves, (n + 63) // 64 + 1)
    return n * K + _pool_holes(n * K, wg_chunk) + max(chunk * waves, (wg_chunk + 64) * min((n + 1023) // 1024, 512))


def append_estimate(n, K, records_per_ray, chunk, max_waves, pool=True):
    """Slots for a trace of n rays that a sample says writes `records_per_ray`: 15 % over that, plus the slack of a full launch
    (pool=True: one more slot per 128 records for the pool's crossings), never more than the worst case.  A multiple of 64."""
    records = int(n * records_per_ray * 1.15)
    slack = records // 128 + max(chunk * max_waves, (_wg_chunk(chunk) + 64) * 256) if pool else chunk * max_waves
    return _round64(min(records + slack, append_worst_case(n, K, chunk, max_waves, pool)))


def _width(precision):
    return 8 if precision == "f64" else 4


# the first-segment fields Engine.trace flags of its own accord (Engine._launch says why `n` and `intensity` are left out)
_ENGINE_FIRST = abi.FIRST_FIELDS & ~(abi.UNIFORM_BIT["n"] | abi.UNIFORM_BIT["intensity"])


def _keeps_bits(bits, precision):
    """`bits` (the pattern of a uniform intensity, or None) if x * 1 gives back exactly that pattern on the device: not a
    subnormal, which a kernel built to flush them would turn into zero (NaN never carries a hint)."""
    if bits is None:
        return None
    exponent = (bits >> 52) & 0x7ff if precision == "f64" else (bits >> 23) & 0xff
    mantissa = bits & ((1 << 52) - 1) if precision == "f64" else bits & ((1 << 23) - 1)
    return None if (exponent == 0 and mantissa != 0) else bits


def _counts_table(scene, counts, columns, device):
    """The interact-count table of a launch as (table, its address, its columns): the caller's, else a zeroed one of `columns`
    columns when the scene has count-limited surfaces, else none."""
    if counts is None:
        if not scene.limited:
            return None, None, 0
        counts = torch.zeros((len(scene.limited), columns), dtype=torch.int32, device=device)
    return counts, counts.data_ptr(), counts.shape[1]


def segment_source(segs):
    """(ot_segment_source, n_segments, seg_count, n_rays) for a SegmentBatch AS IT LIES IN MEMORY, any layout, either precision
    (include/optable_hip.h: ot_monitor_record_many).  The tiled fields are strided [tiles, 64] views of one block: their
    address is the field's first tile and their row stride the tile size; every other field is a plain array (64-slot "tiles"
    back to back).  n_segments / seg_count / n_rays as ot_monitor_record_f64 wants them: all whole [k][ray] planes with the
    counts for slots and tiles, the first n_valid slots for lists (n_rays = -1: with holes).  Addresses only: no library call."""
    src = abi.OtSegmentSource()
    for k, f in enumerate(abi.MON_FIELDS):
        src.base[k] = segs.field(f).data_ptr()
    src.ray = segs.ray.data_ptr()
    src.width = _width(segs.precision)

    def tile_bytes(field):  # (of a tiled field: SegTiles<T>::TILE_BYTES of csrc/kernels.h, read off the view's row stride)
        return (field.stride(0) if field.dim() == 2 else 64) * field.element_size()

    src.tile_stride, src.ray_stride, src.capacity = tile_bytes(segs.ox), tile_bytes(segs.ray), segs.capacity
    if segs.layout in ("slots", "tiled"):
        n_rays = int(segs.n_rays)
        return src, (segs.capacity // n_rays * n_rays if n_rays else 0), segs.count, n_rays
    return src, int(segs.n_valid), None, (-1 if segs.append else 0)


# -- detector images (ot_monitor_image_many): how the library walks the monitors, in plain integers ---------------------------
IMAGE_LDS_BINS = (65536 - 32 * 4) // 12  # misc_kernels.h MON_IMG_LDS_BINS: 64 KB of LDS a workgroup, less the hit tally, at 12 bytes a bin
IMAGE_MAX_BINS = 1 << 24                 # MON_IMG_MAX_BINS: nby * nbz of one monitor
IMAGE_MAX_MONITORS = 32                  # MON_MAX: monitors of one launch


FIELD_LDS_BINS = (65536 - 32 * 4) // 20  # MON_FIELD_LDS_BINS: the same LDS at 20 bytes a bin (re, im, count) — ot_monitor_field_many
BEAM_LDS_BINS = (65536 - 32 * 4 - 4 * 128 * 8) // 12  # MON_BEAM_LDS_BINS: 12 bytes a bin (power, count) next to four waves' erf tables — ot_monitor_beam_many
WAVE_LDS_BINS = (65536 - 32 * 4 - 4 * 256 * 8) // 20  # MON_WAVE_LDS_BINS: 20 bytes a bin (re, im, count) next to four waves' strips of 256 doubles — ot_monitor_wave_many


def image_plan(n_monitors, nby, nbz, budget=IMAGE_LDS_BINS):
    """How ot_monitor_image_many bins `n_monitors` monitors of nby x nbz bins (optable_hip.hip image_plan, the same rule):
    {"path": "lds" when the images of a launch fit a workgroup's LDS (`budget` bins), "global" when one monitor's alone does not
    and every hit is a global atomic; "per_pass": monitors of a launch, as even as the most that fit allows; "passes": launches}."""
    n_monitors, bins = int(n_monitors), int(nby) * int(nbz)
    if n_monitors < 1 or nby < 1 or nbz < 1 or bins > IMAGE_MAX_BINS:
        raise ValueError(f"no image of {n_monitors} monitors x {nby} x {nbz} bins")
    lds = bins <= budget
    most = min(IMAGE_MAX_MONITORS, budget // bins) if lds else IMAGE_MAX_MONITORS
    passes = -(-n_monitors // most)
    return {"path": "lds" if lds else "global", "per_pass": -(-n_monitors // passes), "passes": passes}


def field_plan(n_monitors, nby, nbz):
    """`image_plan` for ot_monitor_field_many: the same rule with FIELD_LDS_BINS (three monitors of 30 x 30 a launch)."""
    return image_plan(n_monitors, nby, nbz, FIELD_LDS_BINS)


def beam_plan(n_monitors, nby, nbz):
    """`image_plan` for ot_monitor_beam_many: the same rule with BEAM_LDS_BINS (five monitors of 30 x 30 a launch; six go 3 + 3)."""
    return image_plan(n_monitors, nby, nbz, BEAM_LDS_BINS)


def wave_plan(n_monitors, nby, nbz):
    """`image_plan` for ot_monitor_wave_many: the same rule with WAVE_LDS_BINS (three monitors of 30 x 30 a launch; four go 2 + 2)."""
    return image_plan(n_monitors, nby, nbz, WAVE_LDS_BINS)


# -- fluence maps (ot_fluence_map) ---------------------------------------------------------------------------------------
FLUENCE_MAX_PIXELS = 1 << 24  # misc_kernels.h SEG_RASTER_MAX_PIXELS: nu * nv


def fluence_plan(nu, nv):
    """How ot_fluence_map deposits into nu x nv pixels (optable_hip.hip ot_fluence_map, the same rule): {"path": "lds" when the
    image fits a workgroup's LDS at 12 bytes a pixel (IMAGE_LDS_BINS), "global" when every piece is a global atomic}."""
    nu, nv = int(nu), int(nv)
    if nu < 1 or nv < 1 or nu * nv > FLUENCE_MAX_PIXELS:
        raise ValueError(f"no fluence map of {nu} x {nv} pixels")
    return {"path": "lds" if nu * nv <= IMAGE_LDS_BINS else "global"}


# -- the reductions of k_mon_spots (ot_monitor_spots_many, ot_monitor_spot_groups_many, ot_monitor_wavefront_many) -----------------------------------------------
def _cell_plan(cells, most):
    """How optable_hip.hip reduce_call walks a list of `cells` cells (the same rule): the launches as (first cell, cells), `most`
    at a time — every launch one pass over the segments."""
    return [(first, min(most, cells - first)) for first in range(0, cells, most)]


# -- spot statistics (ot_monitor_spots_many) --------------------------------------------------------------------------------
SPOT_CELLS = 256          # misc_kernels.h MON_SPOT_CELLS: cells (monitor, plane) of one launch, 224 bytes of LDS each
SPOT_MAX_CELLS = 1 << 20  # n_monitors * n_offsets of one call


def spots_plan(n_monitors, n_offsets):
    """How ot_monitor_spots_many walks the cells (monitor m, plane j) of `n_monitors` monitors x `n_offsets` planes: `_cell_plan`
    over the list [m][j], SPOT_CELLS cells at a time."""
    n_monitors, n_offsets = int(n_monitors), int(n_offsets)
    if n_monitors < 1 or n_offsets < 1 or n_monitors * n_offsets > SPOT_MAX_CELLS:
        raise ValueError(f"no spot statistics of {n_monitors} monitors x {n_offsets} planes")
    return _cell_plan(n_monitors * n_offsets, SPOT_CELLS)


# -- spot statistics per ray group (ot_monitor_spot_groups_many) -------------------------------------------------------------
SPOT_GROUPS_MAX = 256  # optable_hip.h OT_SPOT_GROUPS_MAX: groups of one call, a pair (monitor, plane) of them the least a launch takes


def spot_groups_plan(n_monitors, n_offsets, n_groups):
    """How ot_monitor_spot_groups_many walks the cells (monitor m, plane j, group g) of the list [m][j][g]: `_cell_plan` with whole
    pairs (m, j) a launch, (SPOT_CELLS // n_groups) * n_groups cells at a time — one hit test serves all groups of a pair."""
    n_monitors, n_offsets, n_groups = int(n_monitors), int(n_offsets), int(n_groups)
    if n_monitors < 1 or n_offsets < 1 or not 1 <= n_groups <= SPOT_GROUPS_MAX or n_monitors * n_offsets * n_groups > SPOT_MAX_CELLS:
        raise ValueError(f"no spot statistics of {n_monitors} monitors x {n_offsets} planes x {n_groups} groups")
    return _cell_plan(n_monitors * n_offsets * n_groups, SPOT_CELLS // n_groups * n_groups)


# -- wavefront error (ot_monitor_wavefront_many) -----------------------------------------------------------------------------
WAVEFRONT_MONITORS = 28           # optable_hip.h OT_WAVEFRONT_MONITORS: monitors of one launch, 4 waves x 63 doubles of LDS each
WAVEFRONT_SUMS = 61               # optable_hip.h OT_WAVEFRONT_SUMS: S (45), T (15), Q
WAVEFRONT_MAX_MONITORS = 1 << 20  # n_monitors of one call


def wavefront_plan(n_monitors):
    """How ot_monitor_wavefront_many walks `n_monitors` monitors: `_cell_plan` with a monitor a cell, WAVEFRONT_MONITORS at a time."""
    n_monitors = int(n_monitors)
    if n_monitors < 1 or n_monitors > WAVEFRONT_MAX_MONITORS:
        raise ValueError(f"no wavefront of {n_monitors} monitors")
    return _cell_plan(n_monitors, WAVEFRONT_MONITORS)


# -- wavefront error per ray group (ot_monitor_wavefront_groups_many) ----------------------------------------------------------
WAVEFRONT_GROUP_CELLS_MAX = 4096  # optable_hip.h OT_WAVEFRONT_GROUP_CELLS_MAX: n_monitors * n_groups of one call


def wavefront_groups_plan(n_monitors, n_groups):
    """How ot_monitor_wavefront_groups_many walks the cells (monitor m, group g) of the list [m][g]: `_cell_plan` with
    WAVEFRONT_MONITORS consecutive cells a launch, wherever in a monitor they begin and end — ceil(M G / 28) passes."""
    n_monitors, n_groups = int(n_monitors), int(n_groups)
    if n_monitors < 1 or not 1 <= n_groups <= SPOT_GROUPS_MAX or n_monitors * n_groups > WAVEFRONT_GROUP_CELLS_MAX:
        raise ValueError(f"no wavefront of {n_monitors} monitors x {n_groups} groups")
    return _cell_plan(n_monitors * n_groups, WAVEFRONT_MONITORS)


# -- diffraction PSF (ot_monitor_psf_many) -------------------------------------------------------------------------------------
PSF_MAX_SAMPLES = 512             # optable_hip.h OT_PSF_MAX_SAMPLES: ny, nz of one call
PSF_CHUNK_MIN = 512               # misc_kernels.h MON_PSF_CHUNK_MIN: hits of a chunk before a monitor gets another one
PSF_MAX_CHUNKS = 256              # MON_PSF_MAX_CHUNKS: hit chunks of one monitor
PSF_PARTIAL_ROWS = 1024           # MON_PSF_PARTIAL_ROWS: workgroups of one launch
PSF_ROW = 2 * 64 * 64 + 8         # MON_PSF_ROW: doubles of a workgroup's partial image (a 64 x 64 tile, re and im, and the tallies)
PSF_SCRATCH_BYTES = PSF_PARTIAL_ROWS * PSF_ROW * 8  # optable_hip.h OT_PSF_SCRATCH_BYTES
PSF_AMPLITUDES = ("sqrt", "linear", "unit")  # amplitude_mode 0, 1, 2


def _psf_parts(samples):
    """The pixel tiles along an axis of `samples` samples as (first sample, samples): the ceil(samples / 16) subtiles of 16 split as
    evenly as it goes into ceil(subtiles / 4) parts (misc_kernels.h mon_psf_part, the same rule)."""
    subtiles = -(-samples // 16)
    parts = -(-subtiles // 4)
    cuts = [i * subtiles // parts for i in range(parts + 1)]
    return [(16 * a, min(16 * b, samples) - 16 * a) for a, b in zip(cuts, cuts[1:])]


def psf_plan(ny, nz, hits=()):
    """How ot_monitor_psf_many walks an image of ny x nz samples whose monitors have `hits` hits each (optable_hip.hip, the same
    rule): {"tiles": the pixel tiles as (first row, rows, first column, columns), at most 64 x 64; "chunks": per monitor, the
    workgroups a tile's hits are split over — ceil(hits / PSF_CHUNK_MIN), 1 .. PSF_MAX_CHUNKS, a function of the hit count alone;
    "chunk_hits": per monitor, the hits of a chunk; "pairs_a_launch", "launches": the (monitor, tile) pairs one launch takes so that
    its partial images stay within PSF_PARTIAL_ROWS rows (PSF_SCRATCH_BYTES), and the launches that makes}."""
    ny, nz, hits = int(ny), int(nz), [int(h) for h in hits]
    if not 1 <= ny <= PSF_MAX_SAMPLES or not 1 <= nz <= PSF_MAX_SAMPLES or any(h < 0 for h in hits):
        raise ValueError(f"no PSF of {ny} x {nz} samples (1 .. {PSF_MAX_SAMPLES})")
    tiles = [(r0, r, c0, c) for r0, r in _psf_parts(ny) for c0, c in _psf_parts(nz)]
    chunks = [min(max(-(-h // PSF_CHUNK_MIN), 1), PSF_MAX_CHUNKS) for h in hits]
    pairs = len(hits) * len(tiles)
    a_launch = min(pairs, max(1, PSF_PARTIAL_ROWS // max(chunks, default=1)))
    return {"tiles": tiles, "chunks": chunks, "chunk_hits": [-(-h // c) for h, c in zip(hits, chunks)], "pairs_a_launch": a_launch,
            "launches": -(-pairs // a_launch) if pairs else 0}


# -- diffraction PSF per ray group (ot_monitor_psf_groups_many) ------------------------------------------------------------
PSF_PART_TILE = 2048          # misc_kernels.h MON_PSF_PART_TILE: consecutive hits of one monitor a workgroup of the partition takes
PSF_GROUP_CELLS_MAX = 4096    # optable_hip.h OT_PSF_GROUP_CELLS_MAX: n_monitors x n_groups of one call
PSF_GROUP_SAMPLES_MAX = 1 << 27  # n_monitors x n_groups x ny x nz of one call


def psf_groups_plan(ny, nz, cell_hits, tile=PSF_PART_TILE):
    """How ot_monitor_psf_groups_many walks an image of ny x nz samples whose cells have `cell_hits` hits: an [M][G] nested list
    (or array) of the GROUPED hits of every cell (monitor, group), masked hits left out (optable_hip.hip, the same rule).
    {"partition_tiles": per monitor, the workgroups of each of the two partition passes — ceil(hits / tile) over the monitor's
    hits, 1 for a monitor without a hit (the plan knows the grouped hits only: a monitor with masked hits has ceil((grouped +
    ungrouped) / tile)); "chunks": per cell [M][G], `psf_plan`'s chunks with the cell in a monitor's place; "pairs_a_launch",
    "launches": `psf_plan`'s over the M x G cells}."""
    rows = [[int(h) for h in row] for row in cell_hits]
    G = len(rows[0]) if rows else 0
    tile = int(tile)
    if (any(len(row) != G for row in rows) or (rows and not 1 <= G <= SPOT_GROUPS_MAX) or len(rows) * G > PSF_GROUP_CELLS_MAX
            or len(rows) * G * int(ny) * int(nz) > PSF_GROUP_SAMPLES_MAX or tile < 1):
        raise ValueError(f"no PSF of {len(rows)} monitors x {G} groups of {ny} x {nz} samples")
    plan = psf_plan(ny, nz, [h for row in rows for h in row])
    return {"partition_tiles": [max(1, -(-sum(row) // tile)) for row in rows], "chunks": [plan["chunks"][m * G:(m + 1) * G] for m in range(len(rows))],
            "pairs_a_launch": plan["pairs_a_launch"], "launches": plan["launches"]}


# -- what the private halves of monitor_*_many and fluence_map share: arguments in, outputs out -------------------------------
def _doubles(array):
    return array.ctypes.data_as(C.POINTER(C.c_double))


def _float64_tables(error, *tables):
    """Every (array, shape) of `tables` as the contiguous float64 array of that shape the library reads (None in a shape: any
    length).  ValueError `error` when one has another shape."""
    out = [np.ascontiguousarray(array, dtype=np.float64) for array, _ in tables]
    if any(t.ndim != len(shape) or any(n is not None and n != have for have, n in zip(t.shape, shape)) for t, (_, shape) in zip(out, tables)):
        raise ValueError(error)
    return out


def _image_tables(M, nby, nbz, axes, edges):
    """axes and edges of M monitors as the [M, 6] and [M, nby + 1 + nbz + 1] arrays the library reads."""
    return _float64_tables(f"axes must be [{M}, 6] and edges [{M}, {nby + nbz + 2}]", (axes, (M, 6)), (edges, (M, nby + nbz + 2)))


def _wavelength_arg(wavelength, dev):
    """`wavelength` as the library takes it: (device pointer or None, entries, the one value for all rays)."""
    if not torch.is_tensor(wavelength):
        return None, 0, float(wavelength)
    if wavelength.dtype != torch.float64 or wavelength.dim() != 1 or not wavelength.is_contiguous() or wavelength.device.type != dev.type:
        raise ValueError(f"wavelength: a float or a contiguous float64 vector on {dev}")
    return (wavelength.data_ptr() if wavelength.numel() else None), int(wavelength.numel()), 0.0


_TALLY = (torch.int64, (1,))  # a one-element counter next to a call's images


def _image_specs(shape, planes, tallies):
    """The outputs of an image call: int64 counts and `planes` float64 images of `shape`, then `tallies` tallies."""
    return [(torch.int64, shape)] + [(torch.float64, shape)] * planes + [_TALLY] * tallies


def _outputs(dev, specs, into, alloc, error, tally_error=None):
    """The tensors a call adds to, one per (dtype, shape) of `specs` — new from `alloc`, or `into`, which must be exactly those
    (ValueError `error` for the first that is not, `tally_error` where that one is a tally and the caller has a message for it)."""
    if into is None:
        return tuple(alloc(sh, dtype=dt, device=dev) for dt, sh in specs)
    outs = tuple(into)
    if len(outs) != len(specs):
        raise ValueError(error)
    for t, spec in zip(outs, specs):
        if (t.dtype, tuple(t.shape)) != spec or not t.is_contiguous() or t.device.type != dev.type:
            raise ValueError(tally_error if tally_error and spec is _TALLY else error)
    return outs


def _untouched(outs, into):
    """What a call with nothing to add returns (zero-size tensors have no address to hand over): new outputs zeroed, `into` as it is."""
    return tuple(t.zero_() for t in outs) if into is None else outs


def _address(tensor):
    return None if tensor is None else tensor.data_ptr()


# What a whole-trace launch writes, by library call: (the SegmentBatch made when the caller passes none, what makes a passed
# one of the right precision unusable for `slots` = n x cap records, how the error says so)
_APPEND_OUT = ({"block": True}, lambda out, slots: out.block is None or out.tiled,
               "append layout needs a SegmentBatch(block=True) of the rays' precision")
_OUT = {
    "ot_trace": ({}, lambda out, slots: out.capacity < slots, "output SegmentBatch too small or of the wrong precision"),
    "ot_trace_tiled": ({"tiled": True}, lambda out, slots: not out.tiled or out.capacity < slots,
                       "tiled layout needs a SegmentBatch(tiled=True) of the rays' precision with max_segments * n slots"),
    "ot_trace_append": _APPEND_OUT,
    "ot_trace_trees": ({}, lambda out, slots: out.capacity < slots or out.tiled or out.block is not None,
                       "out: plain slot arrays of max_trace_num * n_rays slots in the rays' precision"),
    "ot_trace_trees_append": _APPEND_OUT,
}


class Engine:
    def __init__(self, device=0):
        self.lib = abi.load()
        if not torch.cuda.is_available():
            raise abi.EngineUnavailable("no GPU visible: optable_amd traces only on an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self._ctx = C.c_void_p()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        abi.check(self.lib.ot_ctx_create(device, C.c_void_p(stream), C.byref(self._ctx)), self.lib)
        self._stream = stream       # the stream the launches go to (part of an output's resident-plane token)
        self._resident_plans = {}   # (precision, uniform mask, n, K) -> planes ot_trace_resident_plan reported for the uploaded scene
        self._first_plans = {}      # the same key -> first-segment fields ot_trace_reuse_plan reported
        self.scene = None
        self.append_chunk = 512  # OT_OPT_APPEND_CHUNK as last set through set_option (the library's default)
        self.trees_refill_at = 16  # OT_OPT_TREES_REFILL_AT likewise
        self._records_per_ray = {}  # (scene, cap, precision) -> records per ray seen in a sample trace (append capacity estimates)
        self._layout_choice = {}    # (scene, precision) -> "slots" | "tiled" measured on the workload itself (tune_layout)
        # An ot_ctx holds one scene and one set of scratch buffers: calls on it are serialised (include/
        # optable_hip.h).  The table-level entry points hold this lock across their upload + trace sequence so that
        # Python threads sharing the engine cannot interleave them (ctypes releases the GIL during a call).
        self.lock = threading.RLock()

    def use_stream(self, stream=None):
        """Launch on `stream` (a torch.cuda.Stream; default: torch's current stream) from now on."""
        handle = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        abi.check(self.lib.ot_ctx_set_stream(self._ctx, C.c_void_p(handle)), self.lib)
        self._stream = handle

    def close(self):
        if self._ctx:
            self.lib.ot_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    # -- scene -----------------------------------------------------------------------------
    def upload(self, scene):
        if scene is self.scene:  # the very object already on the device (a CompiledScene is immutable)
            return
        desc = scene.desc()
        abi.check(self.lib.ot_scene_upload(self._ctx, C.byref(desc)), self.lib)
        self.scene = scene
        self._records_per_ray = {}
        self._layout_choice = {}
        self._resident_plans = {}
        self._first_plans = {}

    def _refuse_hooks(self):
        """Whole-trace launches cannot call back into Python: a scene with user-defined `interact_local` leaves
        (CompiledScene.hooks) is traced generation by generation by `table.ray_tracing` (table.py: _trace_hooked), where
        the device finds the hits and the user's method says what they emit."""
        if self.scene is not None and getattr(self.scene, "hooks", None):
            from .scene import SceneError

            names = sorted({type(c).__name__ for c in self.scene.hooks.values()})
            raise SceneError(f"{', '.join(names)}: a user-defined interact_local runs on the host; trace such a scene with "
                             "table.ray_tracing (Ray objects) — the batch entry points are whole-trace device launches")

    def _check_wavelengths(self, rays):
        """Scenes with a dispersion SERIES (Material(n = callable), fitted over a wavelength interval: materials.py) say
        nothing outside that interval; the reference would call the function there.  Refuse rather than extrapolate."""
        rng = getattr(self.scene, "wavelength_range", None)
        if rng is None or rays.n == 0:
            return
        wl = rays.wavelength.double() * self.scene.unit
        lo, hi = float(wl.min().item()), float(wl.max().item())
        tol = 1e-12 if rays.precision == "f64" else 1e-6  # (a single-precision wavelength exactly at an edge of the interval has moved by its rounding)
        if lo < rng[0] * (1 - tol) or hi > rng[1] * (1 + tol):
            raise ValueError(f"ray wavelengths {lo:.4g} .. {hi:.4g} m leave the interval {rng[0]:.4g} .. {rng[1]:.4g} m on which the "
                             "scene's dispersion functions have their device form (Material(..., wavelength_range=(lo, hi)) widens it)")

    def plan(self, precision, n_rays, max_segments):
        """What the library would launch for the uploaded scene and such a batch, and the output layout its kernels write
        fastest (include/optable_hip.h: ot_trace_plan).  The first call for a light scene measures the device's stream rate in
        both slot layouts (ot_probe_layouts: ~15 ms, once per engine and precision)."""
        info = (C.c_int32 * 8)()
        abi.check(self.lib.ot_trace_plan(self._ctx, _width(precision), int(n_rays), int(max_segments), C.byref(info)), self.lib)
        return {"kernel": int(info[0]), "tiled_ok": bool(info[1]), "append_limit": 1 << int(info[2]),
                "layout": ("slots", "tiled", "append")[int(info[3])], "probe_us": (info[5] / 100.0, info[6] / 100.0)}

    def tune_layout(self, rays, max_segments, launches=20):
        """Measure THIS workload in both slot layouts and keep the faster one for the uploaded scene: `layout="auto"` then
        takes it instead of the generic stream probe (which times a copy-like kernel on buffers of its own; the real trace on
        the caller's buffers can come out the other way round — the two layouts differ by how their streams fall on the
        memory channels, and that depends on the box and on where the buffers lie).  Light scenes only (heavy ones have one
        dense layout); returns {"slots": us per launch, "tiled": us per launch, "rounds": ..., "chosen": ...}.  Needs room for
        both layouts' outputs at once (2 x n x K records).  A caller who times particular output buffers measures on THOSE
        (bench.py does): where the buffers lie is part of what is being measured."""
        K = int(max_segments)
        plan = self.plan(rays.precision, rays.n, K)
        if plan["kernel"] != 1 or not plan["tiled_ok"] or rays.n == 0:
            return {"chosen": plan["layout"]}
        # Both layouts' buffers live side by side and the rounds alternate, after a pre-load that brings the chip to its steady
        # clocks: measured one after the other from cold, the first layout pays for the clocks (a bench run chose tiles at 119
        # against 130 us that way and then ran 125 against 119 in its timed region).  The best round of a layout counts.
        outs = {lay: SegmentBatch(rays.n * K, rays.precision, rays.device, tiled=(lay == "tiled")) for lay in ("slots", "tiled")}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for it in range(2000):  # ~60 ms of load, at most 2000 launches
            self.trace(rays, K, out=outs["slots"], layout="slots")
            if it % 4 == 3:
                ev1.record()
                ev1.synchronize()
                if ev0.elapsed_time(ev1) > 60.0:
                    break
        rounds = {"slots": [], "tiled": []}
        for rnd in range(3):
            for layout in (("slots", "tiled") if rnd % 2 == 0 else ("tiled", "slots")):
                for _ in range(3):
                    self.trace(rays, K, out=outs[layout], layout=layout)
                ev0.record()
                for _ in range(launches):
                    self.trace(rays, K, out=outs[layout], layout=layout)
                ev1.record()
                torch.cuda.synchronize()
                rounds[layout].append(ev0.elapsed_time(ev1) / launches * 1e3)
        del outs
        res = {"slots": min(rounds["slots"]), "tiled": min(rounds["tiled"]), "rounds": rounds}
        res["chosen"] = "tiled" if res["tiled"] < res["slots"] else "slots"
        self._layout_choice = {(id(self.scene), rays.precision): res["chosen"]}
        return res

    def probe_layouts(self, precision="f64"):
        """(microseconds per launch into the 14 slot arrays, into 64-slot tiles) of cfg 2's streams on this device."""
        a, b = C.c_double(), C.c_double()
        abi.check(self.lib.ot_probe_layouts(self._ctx, _width(precision), C.byref(a), C.byref(b)), self.lib)
        return a.value, b.value

    # -- whole traces: one launch preparation for trace and trace_trees ---------------------------
    def _fn(self, name, precision):
        return getattr(self.lib, name + ("_f64" if precision == "f64" else "_f32"))

    def _out_for(self, name, rays, K, out, capacity, reuse_count):
        """The SegmentBatch the library call `name` writes for `rays` capped at K: a new one (append layout: of `capacity` slots),
        or the caller's if it is of the kind, size and precision the call takes; with `count`, `n_rays` and the layout flags set."""
        kind, unfit, message = _OUT[name]
        n = rays.n
        if out is None:
            out = SegmentBatch(capacity if "block" in kind else n * K, rays.precision, rays.device, **kind)
        elif out.precision != rays.precision or unfit(out, n * K):
            raise ValueError(message)
        if not reuse_count or out.count is None or out.count.numel() != n:
            out.count = torch.empty(n, dtype=torch.int32, device=rays.device)
        out.n_rays = n
        if "block" in kind:
            out.append, out.n_valid = True, 0
            out.tiled = False  # (forced, though the check above has just refused a tiled `out` and a new block is not tiled)
        return out

    def resident_plan(self, precision, uniform_mask, n_rays, max_segments):
        """abi.RESIDENT_* planes every record of a lane-per-ray launch of such a batch holds one known value in on the uploaded
        scene (ot_trace_resident_plan: the library's rule, asked once per scene and call shape); 0: not that kernel."""
        key = (precision, int(uniform_mask), int(n_rays), int(max_segments))
        planes = self._resident_plans.get(key)
        if planes is None:
            got = C.c_int32()
            abi.check(self.lib.ot_trace_resident_plan(self._ctx, _width(precision), key[1], key[2], key[3], C.byref(got)), self.lib)
            if len(self._resident_plans) > 64:
                self._resident_plans = {}
            planes = self._resident_plans[key] = int(got.value)
        return planes

    def first_plan(self, precision, uniform_mask, n_rays, max_segments):
        """abi.FIRST_FIELD bits of the record fields a lane-per-ray launch of such a batch would leave unwritten at segment 0 when
        told to (ot_trace_reuse_plan: the library's rule, asked once per scene and call shape); 0: not that kernel, or switched off."""
        key = (precision, int(uniform_mask), int(n_rays), int(max_segments))
        fields = self._first_plans.get(key)
        if fields is None:
            planes, got = C.c_int32(), C.c_uint32()
            abi.check(self.lib.ot_trace_reuse_plan(self._ctx, _width(precision), key[1], key[2], key[3], C.byref(planes), C.byref(got)), self.lib)
            if len(self._first_plans) > 64:
                self._first_plans = {}
            fields = self._first_plans[key] = int(got.value)
        return fields

    def _launch(self, name, rays, K, out, counts_ptr, n_classes, skip=False):
        """The library call `name`_f64 / _f32 on the whole batch, `out` handed over the way its layout wants.  skip: everything
        but the call itself (the append cursor is still made, zeroed and attached).
        Resident planes (SegmentBatch): whatever token `out` carries is read and cleared before the call; the calls that can land on
        the lane-per-ray kernel pass what it allows and leave a new one.  The first-segment token likewise: the fields whose one bit
        pattern in `rays` is the token's go out as first_mask.  `n` and `intensity` are never among them (_ENGINE_FIRST): where their
        planes are resident the plane mask covers segment 0 already, and where the scene changes them a reused output gets those
        planes rewritten whole, segment 0 included (tests/test_gpu_resident.py pins it); the library itself takes the two bits
        from a caller of ot_trace_reuse_*."""
        kind = _OUT[name][0]
        rs = rays.c_struct()
        if "block" in kind:
            cursor = torch.zeros(1, dtype=torch.int64, device=rays.device)
            blk = out.block_struct()
            where = (C.byref(blk), cursor.data_ptr())
        elif "tiled" in kind:
            where = (out.block.data_ptr(), out.capacity)
        else:
            ss = out.c_struct()
            where = (C.byref(ss),)
        if skip:
            out.forget_resident()
        else:
            hint, planes = (), 0
            if name in ("ot_trace", "ot_trace_tiled"):  # the calls that can land on the lane-per-ray kernel take the batch's uniform-field hint
                layout = "tiled" if "tiled" in kind else "slots"
                um = rays.uniform_mask
                planes = self.resident_plan(rays.precision, um, rays.n, K)
                firsts = rays.uniform_values()  # {field: the batch's one bit pattern in it}, the hint checked once
                values = {abi.RESIDENT_N: firsts.get("n"), abi.RESIDENT_INTENSITY: _keeps_bits(firsts.get("intensity"), rays.precision)}
                resident = out.resident_mask(rays.n, layout, values, self, self._stream) & planes
                first = out.first_mask(rays.n, layout, firsts, self, self._stream) & self.first_plan(rays.precision, um, rays.n, K) & _ENGINE_FIRST
                name, hint = name + "_reuse", (um, resident, first)
            out.forget_resident()
            abi.check(self._fn(name, rays.precision)(self._ctx, C.byref(rs), rays.n, K, *where, out.count.data_ptr(), counts_ptr, n_classes, *hint),
                      self.lib)
            if planes:
                out._set_resident(planes, rays.n, layout, values, self, self._stream)
                out._set_first(firsts, rays.n, layout, self, self._stream)
        if "block" in kind:
            out.cursor, out.n_valid = cursor, None  # device scalar: read lazily (n_valid) so that back-to-back launches do not synchronise

    def _until_it_fits(self, launch, capacity, internal_bound_ends, forget_rate):
        """An append trace into an ESTIMATED block: `launch(capacity)` -> SegmentBatch; its cursor (one 8-byte read-back) says what
        the launch needed, and a launch that needed more is repeated into that x 1.02 + 2^20 slots (room for the holes to fall
        differently: which wave claims which chunk is not the same from run to run), three times at most; the last launch is
        handed back unread (its `n_valid` raises if even that did not fit).  What the two callers do differently is passed in:
        internal_bound_ends: a cursor of 2^62 or more (the kernel stopped at an internal bound: `n_valid` says so) ends the loop
        instead of sizing the next block; forget_rate: `_records_per_ray` is cleared before a repeat (the next batch samples anew)."""
        out = launch(capacity)
        for _ in range(3):
            need = int(out.cursor.item())
            if need <= out.capacity or (internal_bound_ends and need >= 1 << 62):
                break
            if forget_rate:
                self._records_per_ray = {}
            del out  # (the block that was too small goes before the larger one is made)
            out = launch(_round64(int(need * 1.02) + (1 << 20)))
        return out

    # -- non-branching trace ---------------------------------------------------------------
    def trace(self, rays: RayBatch, max_segments, out: SegmentBatch = None, counts=None, layout="slots", capacity=None):
        """All segments of every ray in one launch; returns the SegmentBatch.
        layout="slots": [k][ray] slots (ot_trace_*).  layout="tiled": the same slots in 64-slot tiles (ot_trace_tiled_*): light
        scenes, the layout the HBM streams like best.  layout="auto": what the library recommends for this scene, batch and
        device (`plan`): "append" for scenes that take the rolling-list / block-pool kernels, for light ones "tiled" or
        "slots", whichever this device streams faster — every reader of a SegmentBatch (to_host, monitors, exports,
        final_state) takes all layouts.  layout="append": a dense list in append order (ot_trace_append_*,
        include/optable_hip.h) — `capacity` slots; default: estimated from a 1 % sample of the batch (`append_estimate`; the
        rare batch that needs more is traced again into a block of the size the first launch reported); pass what the job
        needs to skip the estimate: if that turns out too small a RuntimeError names the size that fits."""
        self._refuse_hooks()
        if self.scene is None:
            raise RuntimeError("upload a scene first")
        n, K = rays.n, int(max_segments)
        self._check_wavelengths(rays)
        if layout == "auto":  # what this scene's kernels write fastest ON THIS DEVICE: a measurement of this very workload
            # (tune_layout) where there is one, else the library's own rule (ot_trace_plan: a generic stream probe for light scenes)
            tuned = self._layout_choice.get((id(self.scene), rays.precision))
            plan = self.plan(rays.precision, n, K) if n else None
            layout = "slots" if plan is None else (tuned if (tuned and plan["kernel"] == 1 and plan["tiled_ok"]) else plan["layout"])
        if layout not in ("slots", "tiled", "append"):
            raise ValueError(f"unknown layout {layout!r}")
        if layout != "append" or out is not None or capacity is not None:
            return self._trace("ot_trace" if layout == "slots" else "ot_trace_" + layout, rays, K, out, counts, capacity)
        capacity, rpr = self._append_estimate(rays, K, counts)
        if rpr is None:
            return self._trace("ot_trace_append", rays, K, None, counts, capacity)
        # an estimated block can be too small.  (The table of a scene with limited surfaces is made here, once: a repeated launch
        # goes on counting in the table the launch before it left, as it always has.)
        counts = _counts_table(self.scene, counts, n, rays.device)[0]
        return self._until_it_fits(lambda slots: self._trace("ot_trace_append", rays, K, None, counts, slots), capacity,
                                   internal_bound_ends=True, forget_rate=True)

    def _trace(self, name, rays, K, out, counts, capacity):
        # (a `count` of the right length is written over, not replaced: a caller who passes `out` again and again allocates nothing)
        out = self._out_for(name, rays, K, out, capacity, reuse_count=True)
        out.counts_table = counts
        if rays.n == 0:  # nothing to launch (zero-size tensors have no address to hand over); `counts_table` is then what the caller
            return out   # passed, None included: the zeroed table of a scene with limited surfaces is made for a launch only
        counts, counts_ptr, n_classes = _counts_table(self.scene, counts, rays.n, rays.device)
        self._launch(name, rays, K, out, counts_ptr, n_classes)
        out.counts_table = counts
        return out

    def append_capacity(self, n_records):
        """Slots an append-layout block needs for `n_records` segment records on this device (`append_slots` for the shape of the
        last launch and the chunk in force).  Call after a trace of the same scene (the launch shape is taken from it);
        `sum(|count|)` of that trace is the record count."""
        return append_slots(n_records, self.last_launch(), self.append_chunk)

    MAX_WAVES = 256 * 32  # most waves a launch can have resident (256 CUs x 8 per SIMD): each may leave one chunk's tail unused

    def _append_worst_case(self, n, K):
        return append_worst_case(n, K, self.append_chunk, self.MAX_WAVES)

    def _append_estimate(self, rays, K, counts):
        """(capacity, records per ray) for an append trace without tracing the batch twice: records per ray from a strided 1 %
        sample (its own small trace) into `append_estimate`; remembered per scene and cap, so the next batch skips the sample.
        (worst case, None) where no estimate is made."""
        n = rays.n
        if n * K <= 1 << 22 or counts is not None:  # small: the worst case costs nothing; count tables: one ray per id per launch, never sampled
            return self._append_worst_case(n, K), None
        key = (id(self.scene), K, rays.precision)
        rpr = self._records_per_ray.get(key)
        if rpr is None:
            m = max(n // 100, 4096)
            idx = torch.arange(0, n, max(n // m, 1), device=rays.device)
            sample = self.trace(rays.take(idx), K, layout="append", capacity=self._append_worst_case(int(idx.numel()), K))
            rpr = float(sample.count.abs().sum().item()) / float(idx.numel())
            self._records_per_ray = {key: rpr}  # (one scene at a time)
        return append_estimate(n, K, rpr, self.append_chunk, self.MAX_WAVES), rpr

    # -- branching trace: breadth-first, one generation per launch ------------------------------
    def trees_plan(self, precision, max_trace_num, n_rays=0):
        """ot_trace_trees_plan: does the uploaded scene have a lane-per-tree kernel (k_trace_trees), how many queue entries
        per lane would a cap of `max_trace_num` get for a batch of `n_rays` trees (0: one that fills the device), and is that
        enough for every possible tree."""
        info = (C.c_int32 * 8)()
        abi.check(self.lib.ot_trace_trees_plan(self._ctx, _width(precision), int(max_trace_num), int(n_rays), info), self.lib)
        return {"kernel": bool(info[0] & 1), "slots": bool(info[0] & 2), "queue": int(info[1]), "full": bool(info[2]), "lds_entries": int(info[3]),
                "chunk": int(info[4]), "waves": int(info[5])}

    def trace_trees(self, rays: RayBatch, max_trace_num, out: SegmentBatch = None, counts=None, layout="slots", capacity=None):
        """Whole ray trees in one launch, a lane per tree with its FIFO on the chip (ot_trace_trees_*).
        layout "slots": a SegmentBatch in the `slots` layout — slot k * n + i = the k-th ray of tree i in the reference's order;
        layout "append": the dense list of ot_trace_append_* (`capacity` slots, default: what any trace of the batch can need) —
        a stable sort by `ray` is the reference's order; the layout for batches whose trees differ widely in size.
        count[i] = rays of tree i (negative: the tree's queue overflowed, possible only when `trees_plan()["full"]` is False;
        take trace_tree then); `capped` as trace_tree reports it.  `counts`: the interact-count table of scenes with limited
        surfaces ([surfaces, classes], rays.id = column; default: a zeroed column per ray) — exact when no two trees of the
        call share a column."""
        self._refuse_hooks()
        if self.scene is None:
            raise RuntimeError("upload a scene first")
        self._check_wavelengths(rays)
        n, K = rays.n, int(max_trace_num)
        # (a column per tree, one for a batch of none: unlike `trace`, a call for no trees makes and returns a table)
        counts, counts_ptr, n_classes = _counts_table(self.scene, counts, max(n, 1), rays.device)
        if layout not in ("slots", "append"):
            raise ValueError("layout: 'slots' or 'append'")
        name = "ot_trace_trees" if layout == "slots" else "ot_trace_trees_append"
        if layout == "append" and out is None and capacity is None:  # every tree at its cap + the tail of every wave's last chunk
            plan = self.trees_plan(rays.precision, K, n)
            capacity = append_worst_case(n, K, plan["chunk"], plan["waves"], pool=False)
        out = self._out_for(name, rays, K, out, capacity, reuse_count=False)  # (unlike `trace`: a new `count` per call, whatever `out` brings)
        # (the slots call is made for a batch of no trees too; the append call is not, it only leaves a zeroed cursor)
        self._launch(name, rays, K, out, counts_ptr, n_classes, skip=(n == 0 and layout == "append"))
        out.capped = out.count >= K
        out.timed_out = False
        out.counts_table = counts
        out.trees = True
        return out

    LANE_PER_TREE = True  # False: trace_branching always takes the generation loop (A/B measurements)
    HINT_SECONDS = 1.0  # MIN_HINTING_TIME of the reference's loop (optical_table.py:85): a longer trace reports its progress at this interval

    # A lane-per-tree launch whose queues may overflow (caps beyond ~170 in double precision) is a speculation on small trees:
    # small batches only, and it may allocate this many slots at most.
    TREES_SMALL_BATCH = 64 * 256
    TREES_SPECULATIVE_SLOTS = 1 << 22  # (440 MB of records in double precision; 40 rays under the reference's largest example's cap of 1e5)

    def _trees_estimate(self, rays, K):
        """(rays per tree of a large batch, how its waves should refill) from a strided 1 % sample (a lane-per-tree launch of
        its own), remembered per scene, cap and precision.  Rays per tree sizes the append block (`append_estimate` instead of
        every tree at its cap).  The spread of the tree sizes picks OT_OPT_TREES_REFILL_AT (set by the caller: `_refill_at`):
        trees that differ moderately (standard deviation below 0.35 of the mean: cfg 4 with R = 0.2 without a binding cap, 13-30
        rays) are traced 64 to a wave, in step — 1.9 instead of 2.6 ms on 3.2e6 of them; batches of mostly tiny trees, or of trees of
        every size up to the cap, keep their lanes busy one by one (1.33 vs 2.13 and 3.2 vs 3.8 ms) (kernels.h)."""
        n = rays.n
        key = ("trees", id(self.scene), K, rays.precision)
        known = self._records_per_ray.get(key)
        if known is None:
            m = max(n // 100, 4096)
            sample = rays.take(torch.arange(0, n, max(n // m, 1), device=rays.device))
            sizes = self.trace_trees(sample, K, layout="append").count.abs().double()
            rpr = float(sizes.mean().item())
            even = float(sizes.std(unbiased=False).item()) < 0.35 * rpr
            known = (rpr, 64 if even else 16)
            self._records_per_ray = {key: known}  # (one scene at a time)
        return known

    @contextlib.contextmanager
    def _refill_at(self, value):
        """OT_OPT_TREES_REFILL_AT = `value` while one batch of `trace_branching` is traced (its own choice for that batch), then
        again what the caller last asked for through `set_option` (the default for calls that do not sample)."""
        abi.check(self.lib.ot_set_option(self._ctx, abi.OPT_TREES_REFILL_AT, value), self.lib)
        try:
            yield
        finally:
            self.set_option(abi.OPT_TREES_REFILL_AT, self.trees_refill_at)

    def trace_branching(self, rays: RayBatch, max_trace_num, counts=None, max_trace_time=None, distinct_ids=None):
        """Ray trees by whichever path the scene and the cap allow: ONE launch with a lane per tree (`trace_trees`) when the
        scene has such a kernel and its queues hold every possible tree — or, for larger caps, speculatively when the batch
        is small (a tree that overflows its queue sends the call to the generations) — else the generation loop
        (`trace_tree`: a list in generation order).  The lane-per-tree launch writes [k][tree] slots (the reference's order
        as they lie) for small batches of planar scenes and the dense append list otherwise (whole lines per field however
        much the trees differ in size; its block sized from a 1 % sample of a large batch, traced again into what the launch
        asked for should that be too small); readers take all layouts; `capped` / `timed_out` are set either way.
        Scenes with count-limited surfaces: the lane-per-tree kernel meets them in each tree's FIFO order, which is the
        reference's as long as no two trees of the call share a column of `counts` (`distinct_ids=True`: the caller vouches
        for it, as the host API's rounds do; default: such scenes take the generations)."""
        self._refuse_hooks()
        n, K = rays.n, int(max_trace_num)
        gates_ok = not self.scene.limited or bool(distinct_ids)
        if n and gates_ok and self.LANE_PER_TREE and (max_trace_time is None or max_trace_time > 1.0):
            plan = self.trees_plan(rays.precision, K, n)
            small = n <= self.TREES_SMALL_BATCH
            if plan["kernel"] and (plan["full"] or (small and n * K <= self.TREES_SPECULATIVE_SLOTS)):
                before = counts.clone() if (counts is not None and not plan["full"]) else None  # a speculation must not leave counts behind
                if plan["slots"] and small:
                    segs = self.trace_trees(rays, K, counts=counts, layout="slots")
                elif n * K <= 1 << 22 or self.scene.limited:  # small: the worst case costs nothing; count tables are never sampled
                    segs = self.trace_trees(rays, K, counts=counts, layout="append")
                else:
                    rpr, refill_at = self._trees_estimate(rays, K)
                    with self._refill_at(refill_at):
                        if plan["slots"] and rays.precision == "f32" and rpr >= 0.9 * K:
                            # nearly every tree runs into the cap: lanes stay in step, [k][tree] rows are whole lines and cost no claims — in
                            # single precision, where a step is short: 0.29 vs 0.42 ms on 1e6 bushy trees under a cap of 12 (double: 0.57
                            # either way, cfg 4 R = 0.2 4.29 vs 4.07 for the dense list)
                            return self.trace_trees(rays, K, layout="slots")
                        segs = self._until_it_fits(lambda slots: self.trace_trees(rays, K, layout="append", capacity=slots),
                                                   append_estimate(n, K, rpr, plan["chunk"], plan["waves"], pool=False),
                                                   internal_bound_ends=False, forget_rate=False)
                if plan["full"] or not bool((segs.count < 0).any()):
                    return segs
                del segs
                if before is not None:
                    counts.copy_(before)
        return self.trace_tree(rays, K, counts=counts, max_trace_time=max_trace_time)

    def trace_tree(self, rays: RayBatch, max_trace_num, counts=None, out_capacity=None, max_trace_time=None):
        """Full ray trees (beam splitters, partial reflections, any cap).  Returns a flat
        SegmentBatch in generation order plus, per tree, whether a cap cut it short.
        `max_trace_time` (seconds): the reference's wall-clock cap (optical_table.py:84-97, `perfomance_limit
        ["max_trace_time"]`), honoured at generation granularity — the clock is read after every generation of
        the whole batch, and once it has run out the rays still queued are dropped, as the reference drops a
        tree's queue (`:138-144`); the trees they belonged to are reported in `capped` (`timed_out` says why)."""
        self._refuse_hooks()
        t_start = time.time()
        if self.scene is None:
            raise RuntimeError("upload a scene first")
        prec = rays.precision
        self._check_wavelengths(rays)
        dev, n = rays.device, rays.n
        if n == 0:
            out = SegmentBatch(0, prec, dev)
            out.n_valid, out.counts_table = 0, counts
            out.capped = torch.zeros(0, dtype=torch.bool, device=dev)
            out.timed_out = False
            return out
        fan = max(self.scene.max_children, 1)
        if out_capacity is None:
            out_capacity = max(4 * n, 1024)
        out = SegmentBatch(out_capacity, prec, dev)
        budget = torch.full((n,), int(max_trace_num), dtype=torch.int32, device=dev)
        state = torch.zeros(2, dtype=torch.int64, device=dev)  # [segment cursor, rays in the next generation]
        tree = torch.arange(n, dtype=torch.int32, device=dev)
        counts, counts_ptr, n_classes = _counts_table(self.scene, counts, n, dev)
        # The generation loop runs inside the library (ot_trace_tree_*: one 16-byte read-back per generation); it comes back
        # when the queue is empty, when the time is up, or when the pending generation needs more room — then the
        # buffers are grown here and the call repeated with that generation as input.
        tree_fn = self._fn("ot_trace_tree", prec)

        def buffer_pair(cap):  # two generations' rays and the tree of each ray
            return ([RayBatch(cap, prec, dev, initialise=False) for _ in range(2)],
                    [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2)])

        bufs, trees = buffer_pair(max(n * fan, 1024))
        result = (C.c_int64 * 5)()
        cur, cur_n, written = rays, n, 0
        timed_out = None
        # The library comes back at least once per HINT seconds: a trace that runs longer says so once per second, as the
        # reference does per input ray (optical_table.py:99-111; here the clock is the batch's and the counts are the batch's).
        HINT = self.HINT_SECONDS
        while cur_n > 0:
            left_total = None if max_trace_time is None else max(max_trace_time - (time.time() - t_start), 0.0)
            left = HINT * 1.01 if left_total is None else min(left_total, HINT * 1.01)  # (just over the interval: chains of small generations need max_seconds > 1)
            rs, ss, sa, sb = cur.c_struct(), out.c_struct(), bufs[0].c_struct(), bufs[1].c_struct()
            abi.check(tree_fn(self._ctx, C.byref(rs), tree.data_ptr(), cur_n, budget.data_ptr(), C.byref(ss), out.capacity,
                              state.data_ptr(), C.byref(sa), trees[0].data_ptr(), C.byref(sb), trees[1].data_ptr(), bufs[0].n,
                              counts_ptr, n_classes, left, result), self.lib)
            written, cur_n, where, _, reason = (int(x) for x in result)
            if where:  # the pending generation sits in one of the buffers
                cur, tree = bufs[where - 1].slice(0, cur_n), trees[where - 1][:cur_n]
                if where == 1:  # a call writes its first generation into buf_a: the pending one must be in the other buffer
                    bufs.reverse()
                    trees.reverse()
            if cur_n == 0:
                break
            if reason == 3:
                elapsed = time.time() - t_start
                if max_trace_time is None or elapsed < max_trace_time:  # a hint interval ended, not the caller's time
                    print("Tracing... Time elapsed: {:.2f} s, Trace num: {}, Alive rays: {}, Dead rays: {}".format(elapsed, written, cur_n, written))
                    continue
                timed_out = torch.zeros(n, dtype=torch.bool, device=dev)
                timed_out[tree.long()] = True  # trees with rays still queued
                break
            if reason == 1:
                out = _grow(out, max(written + cur_n, 2 * out.capacity), written)
            elif reason == 2:  # new, larger buffers; the pending generation stays where it is until the next call has read it
                keep = (cur, tree)  # noqa: F841 - holds the old buffer alive across the call
                bufs, trees = buffer_pair(max(cur_n * fan, 2 * bufs[0].n))
        out.n_valid = int(written)
        out.counts_table = counts
        out.capped = budget <= 0  # cap reached: queued rays were dropped (optical_table.py:138-144)
        out.timed_out = timed_out is not None
        if timed_out is not None:
            out.capped = out.capped | timed_out
        return out

    def generation_step(self, rays: RayBatch, counts=None, tree=None):
        """ONE generation of the breadth-first trace: every input ray is processed once (nearest hit,
        interaction).  Returns (segments, children, parent): a SegmentBatch with one record per input ray
        (slot i = ray i), the emitted rays as a RayBatch in parent order then child order, and for each of them
        the index of its parent.  This is `component.interact(ray)` for a batch (optical_component.py:337-378).
        `tree` (int32 per ray, ascending: a generation lists its rays tree by tree): which rays belong to one ray tree — the
        rays of a tree meet a count-limited surface one after the other in input order, as the reference's FIFO makes them
        (optical_component.py:140-149, 359-362); default: every ray a tree of its own."""
        if self.scene is None:
            raise RuntimeError("upload a scene first")
        prec = rays.precision
        self._check_wavelengths(rays)
        dev, n = rays.device, rays.n
        out = SegmentBatch(n, prec, dev)
        out.n_valid = 0
        if n == 0:
            return out, RayBatch(0, prec, dev), torch.zeros(0, dtype=torch.int32, device=dev)
        fan = max(self.scene.max_children, 1)
        state = torch.zeros(2, dtype=torch.int64, device=dev)
        if tree is None:
            tree = torch.arange(n, dtype=torch.int32, device=dev)
            budget = torch.full((n,), 2, dtype=torch.int32, device=dev)  # (one ray per tree, room for one more: the children are wanted)
        else:
            tree = torch.as_tensor(tree, dtype=torch.int32, device=dev).contiguous()
            if tree.numel() != n or (n > 1 and bool((tree[1:] < tree[:-1]).any())) or int(tree[0]) < 0:
                raise ValueError("tree: one non-negative id per ray, ascending")
            budget = torch.full((int(tree[-1]) + 1,), n + 1, dtype=torch.int32, device=dev)  # (every ray processed, children wanted)
        nxt = RayBatch(n * fan, prec, dev, initialise=False)
        nxt_tree = torch.empty(n * fan, dtype=torch.int32, device=dev)
        counts, counts_ptr, n_classes = _counts_table(self.scene, counts, n, dev)
        rs, ss, ns = rays.c_struct(), out.c_struct(), nxt.c_struct()
        self.set_option(abi.OPT_GEN_PARENT_INDEX, 1)  # nxt_tree = the parent's index, whatever `tree` groups
        try:
            abi.check(self._fn("ot_trace_generation", prec)(
                self._ctx, C.byref(rs), tree.data_ptr(), n, budget.data_ptr(), C.byref(ss), out.capacity,
                state.data_ptr(), C.byref(ns), nxt_tree.data_ptr(), nxt.n, state.data_ptr() + 8,
                counts_ptr, n_classes), self.lib)
        finally:
            self.set_option(abi.OPT_GEN_PARENT_INDEX, 0)
        written, n_next = state.tolist()
        out.n_valid, out.counts_table = int(written), counts
        kids = nxt.slice(0, int(n_next))
        # bits 8.. of the flags name the node a child starts on IN THIS SCENE (include/optable_hip.h); the batch is handed to
        # the caller, who may trace it through any scene: drop them (the start-plane rule then falls back to the |t| guard)
        kids.flags.bitwise_and_(0xff)
        return out, kids, nxt_tree[: int(n_next)]

    # -- monitors -------------------------------------------------------------------------------
    def monitor_record(self, monitor_struct, segs: SegmentBatch, n_segments=None):
        """Device pass of Monitor.record over a SegmentBatch.  Returns (slot index, P_local [h,3], t)
        in ascending slot order.  For the [k][ray] layout every slot is scanned and unused ones
        are skipped on the device."""
        with self.lock:
            return self._monitor_record(monitor_struct, segs, n_segments)

    def _monitor_record(self, monitor_struct, segs, n_segments):
        dev = segs.device
        segs = segs.to_slots()  # (a tiled history: one copy into slot arrays)
        if segs.precision != "f64":  # the monitor pass is fp64: widen an fp32 history once
            segs = segs.astype("f64")
        if segs.layout == "slots":
            n_segments, count_ptr, n_rays = segs.capacity // segs.n_rays * segs.n_rays, segs.count.data_ptr(), segs.n_rays
        else:
            n_segments = segs.n_valid if n_segments is None else n_segments
            count_ptr, n_rays = None, (-1 if segs.append else 0)
        idx = torch.empty(n_segments, dtype=torch.int64, device=dev)
        P = [torch.empty(n_segments, dtype=torch.float64, device=dev) for _ in range(3)]
        t = torch.empty(n_segments, dtype=torch.float64, device=dev)
        nh = torch.zeros(1, dtype=torch.int64, device=dev)
        ss = segs.c_struct()
        abi.check(self.lib.ot_monitor_record_f64(self._ctx, C.byref(monitor_struct), C.byref(ss), n_segments, count_ptr, n_rays,
                                                 idx.data_ptr(), P[0].data_ptr(), P[1].data_ptr(), P[2].data_ptr(),
                                                 t.data_ptr(), nh.data_ptr()), self.lib)
        k = int(nh.item())
        return idx[:k], torch.stack([p[:k] for p in P], dim=1), t[:k]

    def monitor_record_many(self, monitor_structs, segs: SegmentBatch, capacity=None):
        """Device pass of Monitor.record for a list of monitors over a SegmentBatch read as it lies (any layout, either
        precision: no `to_slots`, no `astype`): ot_monitor_record_many, the segments read once per pass whatever the number of
        monitors.  Returns one (slot index, P_local [h,3], t) per monitor, ascending slot order.  `capacity`: entries of the
        concatenated output (default: the slots scanned); a pass that finds more is repeated once, whole, with exactly what it
        found — the usual case for a stack of monitors that every ray crosses (M monitors x n rays hits against the slots of
        the history): pass `capacity` >= the hits expected to spare the first pass."""
        with self.lock:
            return self._monitor_record_many(list(monitor_structs), segs, capacity)

    def _monitor_record_many(self, mons, segs, capacity):
        dev, M = segs.device, len(mons)
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:  # (zero-size tensors have no address to hand over)
            none = torch.empty(0, dtype=torch.float64, device=dev)
            return [(torch.empty(0, dtype=torch.int64, device=dev), none.reshape(0, 3), none) for _ in range(M)]
        table = (abi.OtMonitor * M)(*mons)
        capacity = max(n_segments if capacity is None else int(capacity), 1)
        for _ in range(2):
            idx = torch.empty(capacity, dtype=torch.int64, device=dev)
            out = torch.empty((4, capacity), dtype=torch.float64, device=dev)  # Px, Py, Pz, t
            first = torch.empty(M + 2, dtype=torch.int64, device=dev)          # first[0 .. M], then the total
            abi.check(self.lib.ot_monitor_record_many(self._ctx, table, M, C.byref(src), n_segments, None if count is None else count.data_ptr(),
                                                      n_rays, capacity, first.data_ptr(), idx.data_ptr(), *(out[k].data_ptr() for k in range(4)),
                                                      first.data_ptr() + 8 * (M + 1)), self.lib)
            first = first.tolist()  # (synchronises)
            if first[M + 1] <= capacity:
                break
            capacity = first[M + 1]
        return [(idx[a:b], out[:3, a:b].T, out[3, a:b]) for a, b in zip(first[:M], first[1:M + 1])]

    def monitor_image_many(self, monitor_structs, axes, edges, bins, segs: SegmentBatch, into=None):
        """Detector images of a list of monitors over a SegmentBatch read as it lies (ot_monitor_image_many: the hits of
        `monitor_record_many`, binned on the device with no hit list).  axes: [M, 6] doubles (a_y, a_z per monitor); edges:
        [M, nby + 1 + nbz + 1] doubles; bins = (nby, nbz).  Returns (counts, intensity): int64 / float64 [M, nby, nbz] device
        tensors, zeroed by the call — or `into`, such a pair from an earlier call, with this call's hits added to it."""
        with self.lock:
            return self._monitor_image_many(list(monitor_structs), axes, edges, bins, segs, into)

    def _monitor_image_many(self, mons, axes, edges, bins, segs, into):
        dev, M, (nby, nbz) = segs.device, len(mons), bins
        axes, edges = _image_tables(M, nby, nbz, axes, edges)
        outs = _outputs(dev, _image_specs((M, nby, nbz), 1, 0), into, torch.empty,  # (the call zeroes them)
                        f"into: contiguous int64 counts and float64 intensity of shape [{M}, {nby}, {nbz}] on {dev}")
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:
            return _untouched(outs, into)
        abi.check(self.lib.ot_monitor_image_many(self._ctx, (abi.OtMonitor * M)(*mons), M, _doubles(axes), _doubles(edges), nby, nbz, C.byref(src),
                                                 segs.field("intensity").data_ptr(), n_segments, _address(count), n_rays,
                                                 *(t.data_ptr() for t in outs), 0 if into is None else 1), self.lib)
        return outs

    def fluence_map(self, axes, u_edges, v_edges, depth, segs: SegmentBatch, weighted=True, into=None):
        """Fluence map of a SegmentBatch read as it lies (ot_fluence_map): every segment rasterised into the view axes = (a_u,
        a_v, a_w) ([3, 3] doubles) over the pixels u_edges x v_edges (numpy) within depth = (w_lo, w_hi).  weighted: every
        piece weighs its segment's intensity; False: 1 (plain path length).  Returns (counts, fluence, skipped): int64 / float64
        [nu, nv] and a one-element int64 device tensor, zeroed by the call — or `into`, such a triple from an earlier call, with
        this call's segments added to it."""
        with self.lock:
            return self._fluence_map(axes, u_edges, v_edges, depth, segs, weighted, into)

    def _fluence_map(self, axes, u_edges, v_edges, depth, segs, weighted, into):
        dev = segs.device
        axes, u_edges, v_edges = _float64_tables("axes must be [3, 3], u_edges and v_edges one-dimensional", (axes, (3, 3)), (u_edges, (None,)),
                                                 (v_edges, (None,)))
        nu, nv = len(u_edges) - 1, len(v_edges) - 1
        fluence_plan(nu, nv)
        outs = _outputs(dev, _image_specs((nu, nv), 1, 1), into, torch.zeros,  # (zeros: the library is not called for nothing)
                        f"into: contiguous int64 counts and float64 fluence of shape [{nu}, {nv}] and one int64 on {dev}")
        src, n_segments, count, n_rays = segment_source(segs)
        if n_segments == 0:  # (zero-size tensors have no address to hand over; nothing to add)
            return outs
        abi.check(self.lib.ot_fluence_map(self._ctx, _doubles(axes), _doubles(u_edges), nu, _doubles(v_edges), nv, float(depth[0]), float(depth[1]),
                                          C.byref(src), segs.field("intensity").data_ptr() if weighted else None, n_segments, _address(count),
                                          n_rays, *(t.data_ptr() for t in outs), 0 if into is None else 1), self.lib)
        return outs

    def monitor_spots_many(self, monitor_structs, axes, centre, offsets, segs: SegmentBatch, weighted=True, into=None):
        """Spot statistics of a list of monitors over a SegmentBatch read as it lies (ot_monitor_spots_many): the moments of the
        hits of every monitor on itself and on the planes displaced by `offsets` (numpy, J) along its normal.  axes: [M, 6] doubles
        (a_y, a_z per monitor); centre: [M, 2] doubles (c_y, c_z, subtracted from every hit's coordinates).  weighted: every hit
        weighs its segment's intensity; False: 1.  Returns (counts, sums): int64 [M, J] and float64 [M, J, 6] (W, Wy, Wz, Wyy,
        Wzz, Wyz) device tensors, zeroed by the call — or `into`, such a pair from an earlier call, with this call's hits added
        to it.  The sums are the same bits every run."""
        with self.lock:
            return self._monitor_spots_many(list(monitor_structs), axes, centre, offsets, segs, weighted, into)

    def _monitor_spots_many(self, mons, axes, centre, offsets, segs, weighted, into):
        M = len(mons)
        axes, centre, offsets = _float64_tables(f"axes must be [{M}, 6], centre [{M}, 2] and offsets one-dimensional", (axes, (M, 6)), (centre, (M, 2)),
                                                (offsets, (None,)))
        J = len(offsets)
        if M:
            spots_plan(M, J)
        return self._reduce_many("ot_monitor_spots_many", mons, (_doubles(axes), _doubles(centre), _doubles(offsets), J), segs, weighted, (),
                                 [(torch.int64, (M, J)), (torch.float64, (M, J, 6))], into,
                                 f"into: contiguous int64 counts of shape [{M}, {J}] and float64 sums of shape [{M}, {J}, 6] on {segs.device}")

    def monitor_spot_groups_many(self, monitor_structs, axes, centre, offsets, groups, n_groups, segs: SegmentBatch, weighted=True, into=None):
        """Spot statistics per ray group (ot_monitor_spot_groups_many): `monitor_spots_many` with a group axis — a hit of a segment
        of input ray r belongs to group groups[r].  groups: a contiguous int32 vector on the segments' device, one id per input
        ray; ids outside 0 .. n_groups - 1 (and rays beyond the table) are masked.  Returns (counts, sums): int64 [M, J, G] and
        float64 [M, J, G, 6] device tensors, zeroed by the call — or `into`, such a pair from an earlier call, with this call's
        hits added to it.  The sums are the same bits every run."""
        with self.lock:
            return self._monitor_spot_groups_many(list(monitor_structs), axes, centre, offsets, groups, int(n_groups), segs, weighted, into)

    def _monitor_spot_groups_many(self, mons, axes, centre, offsets, groups, G, segs, weighted, into):
        M = len(mons)
        axes, centre, offsets = _float64_tables(f"axes must be [{M}, 6], centre [{M}, 2] and offsets one-dimensional", (axes, (M, 6)), (centre, (M, 2)),
                                                (offsets, (None,)))
        J = len(offsets)
        spot_groups_plan(max(M, 1), J, G)
        if (not torch.is_tensor(groups) or groups.dtype != torch.int32 or groups.dim() != 1 or not groups.is_contiguous() or groups.numel() < 1
                or groups.device.type != segs.device.type):
            raise ValueError(f"groups: a contiguous int32 vector of one id per input ray on {segs.device}")
        tables = (_doubles(axes), _doubles(centre), _doubles(offsets), J, groups.data_ptr(), int(groups.numel()), G)
        return self._reduce_many("ot_monitor_spot_groups_many", mons, tables, segs, weighted, (),
                                 [(torch.int64, (M, J, G)), (torch.float64, (M, J, G, 6))], into,
                                 f"into: contiguous int64 counts of shape [{M}, {J}, {G}] and float64 sums of shape [{M}, {J}, {G}, 6] on {segs.device}")

    def _reduce_many(self, call, mons, tables, segs, weighted, fields, specs, into, error):
        """What monitor_spots_many, monitor_spot_groups_many and monitor_wavefront_many do alike once their tables are checked: the outputs of `specs`, and the
        library's `call` with the mode's `tables` behind the monitors and its segment `fields` behind the intensity."""
        M = len(mons)
        outs = _outputs(segs.device, specs, into, torch.zeros, error)  # (zeros: the library is not called for nothing)
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:  # (zero-size tensors have no address to hand over; nothing to add)
            return outs
        abi.check(getattr(self.lib, call)(self._ctx, (abi.OtMonitor * M)(*mons), M, *tables, C.byref(src),
                                          segs.field("intensity").data_ptr() if weighted else None, *(segs.field(f).data_ptr() for f in fields),
                                          n_segments, _address(count), n_rays, *(t.data_ptr() for t in outs), 0 if into is None else 1), self.lib)
        return outs

    def monitor_wavefront_many(self, monitor_structs, axes, reference_kind, reference, coordinates, pupil, piston, segs: SegmentBatch,
                               weighted=True, into=None):
        """The wavefront sums of a list of monitors over a double-precision SegmentBatch read as it lies
        (ot_monitor_wavefront_many).  axes: [M, 6] doubles (a_y, a_z per monitor); reference_kind 0: reference [M, 3] is the focus in
        every monitor's frame, 1: the plane wave's unit direction there; coordinates 0: direction, 1: position; pupil: [M, 3]
        (c_y, c_z, R); piston: [M].  weighted: every hit weighs its segment's intensity; False: 1.  Returns (counts, sums): int64
        [M, 2] (inside, outside the pupil) and float64 [M, 61] (S, T, Q in the header's order) device tensors, zeroed by the call —
        or `into`, such a pair from an earlier call, with this call's hits added to it.  The sums are the same bits every run."""
        with self.lock:
            return self._monitor_wavefront_many(list(monitor_structs), axes, reference_kind, reference, coordinates, pupil, piston, segs, weighted, into)

    def _monitor_wavefront_many(self, mons, axes, reference_kind, reference, coordinates, pupil, piston, segs, weighted, into):
        M = len(mons)
        axes, reference, pupil, piston = _float64_tables(f"axes must be [{M}, 6], reference and pupil [{M}, 3] and piston [{M}]", (axes, (M, 6)),
                                                         (reference, (M, 3)), (pupil, (M, 3)), (piston, (M,)))
        if segs.precision != "f64":
            raise ValueError("a wavefront needs double-precision segments")
        if M:
            wavefront_plan(M)
        tables = (_doubles(axes), int(reference_kind), _doubles(reference), int(coordinates), _doubles(pupil), _doubles(piston))
        return self._reduce_many("ot_monitor_wavefront_many", mons, tables, segs, weighted, ("n", "pathlength"),
                                 [(torch.int64, (M, 2)), (torch.float64, (M, WAVEFRONT_SUMS))], into,
                                 f"into: contiguous int64 counts of shape [{M}, 2] and float64 sums of shape [{M}, {WAVEFRONT_SUMS}] on {segs.device}")

    def monitor_wavefront_groups_many(self, monitor_structs, axes, reference_kind, reference, coordinates, pupil, piston, groups, n_groups,
                                      segs: SegmentBatch, weighted=True, into=None):
        """The wavefront sums per ray group (ot_monitor_wavefront_groups_many): `monitor_wavefront_many` with a group axis — a hit
        of a segment of input ray r belongs to group groups[r], and reference [M, G, 3], pupil [M, G, 3] and piston [M, G] are per
        (monitor, group); axes stay [M, 6].  groups: a contiguous int32 vector on the segments' device, one id per input ray; ids
        outside 0 .. n_groups - 1 (and rays beyond the table) are masked.  Returns (counts, sums): int64 [M, G, 2] and float64
        [M, G, 61] device tensors, zeroed by the call — or `into`, such a pair from an earlier call, with this call's hits added
        to it.  The sums are the same bits every run."""
        with self.lock:
            return self._monitor_wavefront_groups_many(list(monitor_structs), axes, reference_kind, reference, coordinates, pupil, piston, groups,
                                                       int(n_groups), segs, weighted, into)

    def _monitor_wavefront_groups_many(self, mons, axes, reference_kind, reference, coordinates, pupil, piston, groups, G, segs, weighted, into):
        M = len(mons)
        wavefront_groups_plan(max(M, 1), G)
        axes, reference, pupil, piston = _float64_tables(f"axes must be [{M}, 6], reference and pupil [{M}, {G}, 3] and piston [{M}, {G}]", (axes, (M, 6)),
                                                         (reference, (M, G, 3)), (pupil, (M, G, 3)), (piston, (M, G)))
        if segs.precision != "f64":
            raise ValueError("a wavefront needs double-precision segments")
        if (not torch.is_tensor(groups) or groups.dtype != torch.int32 or groups.dim() != 1 or not groups.is_contiguous() or groups.numel() < 1
                or groups.device.type != segs.device.type):
            raise ValueError(f"groups: a contiguous int32 vector of one id per input ray on {segs.device}")
        tables = (_doubles(axes), int(reference_kind), _doubles(reference), int(coordinates), _doubles(pupil), _doubles(piston), groups.data_ptr(),
                  int(groups.numel()), G)
        return self._reduce_many("ot_monitor_wavefront_groups_many", mons, tables, segs, weighted, ("n", "pathlength"),
                                 [(torch.int64, (M, G, 2)), (torch.float64, (M, G, WAVEFRONT_SUMS))], into,
                                 f"into: contiguous int64 counts of shape [{M}, {G}, 2] and float64 sums of shape [{M}, {G}, {WAVEFRONT_SUMS}] on {segs.device}")

    def monitor_psf_many(self, monitor_structs, axes, reference_kind, reference, grid, pixels, segs: SegmentBatch, wavelength, amplitude_mode=0,
                         into=None):
        """The diffraction PSF of a list of monitors over a double-precision SegmentBatch read as it lies (ot_monitor_psf_many): the
        plane waves of every monitor's hits summed over its grid of samples.  axes: [M, 6] doubles (a_y, a_z per monitor);
        reference_kind 0: reference [M, 3] is the focus in every monitor's frame, 1: the plane wave's unit direction there; grid:
        [M, 4] doubles (y0, dy, z0, dz); pixels = (ny, nz).  wavelength: a float for all rays, or a float64 device tensor indexed by
        the segments' `ray`; amplitude_mode: 0 = sqrt(intensity), 1 = intensity, 2 = 1.  Returns (counts, norm, re, im): int64 [M, 3]
        (used, skipped, aliased), float64 [M] (the summed amplitudes) and float64 [M, ny, nz] twice, device tensors zeroed by the
        call — or `into`, such a tuple from an earlier call, with this call's hits added to it.  The same bits every run."""
        with self.lock:
            return self._monitor_psf_many(list(monitor_structs), axes, reference_kind, reference, grid, pixels, segs, wavelength, amplitude_mode, into)

    def _monitor_psf_many(self, mons, axes, reference_kind, reference, grid, pixels, segs, wavelength, amplitude_mode, into, groups=None):
        """Both PSF calls: groups None, or (ids, G) — then every output has a group axis behind the monitors' and `ungrouped` follows."""
        dev, M, (ny, nz) = segs.device, len(mons), pixels
        axes, reference, grid = _float64_tables(f"axes must be [{M}, 6], reference [{M}, 3] and grid [{M}, 4]", (axes, (M, 6)), (reference, (M, 3)),
                                                (grid, (M, 4)))
        if segs.precision != "f64":
            raise ValueError("a PSF needs double-precision segments")
        psf_plan(ny, nz)
        cell, call, tables, tail, shapes = (M,), "ot_monitor_psf_many", (), [], f"[{M}, 3], float64 norm of shape [{M}] and float64 re, im of shape [{M}, {ny}, {nz}]"
        if groups is not None:
            ids, G = groups
            psf_groups_plan(ny, nz, [[0] * G] * max(M, 1))
            if (not torch.is_tensor(ids) or ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous() or ids.numel() < 1
                    or ids.device.type != dev.type):
                raise ValueError(f"groups: a contiguous int32 vector of one id per input ray on {dev}")
            cell, call, tables, tail = (M, G), "ot_monitor_psf_groups_many", (ids.data_ptr(), int(ids.numel()), G), [(torch.int64, (M,))]
            shapes = f"[{M}, {G}, 3], float64 norm of shape [{M}, {G}], float64 re, im of shape [{M}, {G}, {ny}, {nz}] and int64 ungrouped of shape [{M}]"
        wavelength = _wavelength_arg(wavelength, dev)
        outs = _outputs(dev, [(torch.int64, cell + (3,)), (torch.float64, cell), (torch.float64, cell + (ny, nz)), (torch.float64, cell + (ny, nz))] + tail, into,
                        torch.zeros,  # (zeros: the library is not called for nothing)
                        f"into: contiguous int64 counts of shape {shapes} on {dev}")
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:  # (zero-size tensors have no address to hand over; nothing to add)
            return outs
        abi.check(getattr(self.lib, call)(self._ctx, (abi.OtMonitor * M)(*mons), M, _doubles(axes), int(reference_kind), _doubles(reference),
                                          _doubles(grid), ny, nz, *tables, C.byref(src), segs.field("intensity").data_ptr(), segs.field("n").data_ptr(),
                                          segs.field("pathlength").data_ptr(), *wavelength, int(amplitude_mode), n_segments, _address(count), n_rays,
                                          *(t.data_ptr() for t in outs), 0 if into is None else 1), self.lib)
        return outs

    def monitor_psf_groups_many(self, monitor_structs, axes, reference_kind, reference, grid, pixels, groups, n_groups, segs: SegmentBatch, wavelength,
                                amplitude_mode=0, into=None):
        """The diffraction PSF per ray group (ot_monitor_psf_groups_many): `monitor_psf_many` with a group axis — a hit of a segment
        of input ray r belongs to group groups[r], and the fields of different groups are never added.  groups: a contiguous int32
        vector on the segments' device, one id per input ray; ids outside 0 .. n_groups - 1 (and rays beyond the table) are masked
        and tallied.  Returns (counts, norm, re, im, ungrouped): int64 [M, G, 3], float64 [M, G], float64 [M, G, ny, nz] twice and
        int64 [M] (the masked hits) device tensors, zeroed by the call — or `into`, such a tuple from an earlier call, with this
        call's hits added to it.  The same bits every run; with G = 1 and every id 0, `monitor_psf_many`'s."""
        with self.lock:
            return self._monitor_psf_many(list(monitor_structs), axes, reference_kind, reference, grid, pixels, segs, wavelength, amplitude_mode, into,
                                          groups=(groups, int(n_groups)))

    def monitor_field_many(self, monitor_structs, axes, edges, bins, segs: SegmentBatch, wavelength, amplitude_mode=0, into=None):
        """Coherent detector images of a list of monitors over a double-precision SegmentBatch read as it lies
        (ot_monitor_field_many: `monitor_image_many` with the phasor a exp(i phi) of every hit in place of its intensity).  axes,
        edges, bins as there.  wavelength: a float for all rays, or a float64 device tensor indexed by the segments' `ray`;
        amplitude_mode: 0 = sqrt(intensity), 1 = intensity.  Returns (counts, re, im, skipped): int64 / float64 / float64
        [M, nby, nbz] device tensors and an int64 device tensor of one element (hits left out because their ray or wavelength
        was unusable), zeroed by the call — or `into`, such a tuple from an earlier call, with this call's hits added to it."""
        with self.lock:
            return self._monitor_field_many(list(monitor_structs), axes, edges, bins, segs, wavelength, amplitude_mode, into)

    def _monitor_field_many(self, mons, axes, edges, bins, segs, wavelength, amplitude_mode, into):
        dev, M, (nby, nbz) = segs.device, len(mons), bins
        axes, edges = _image_tables(M, nby, nbz, axes, edges)
        if segs.precision != "f64":
            raise ValueError("a field needs double-precision segments")
        wavelength = _wavelength_arg(wavelength, dev)
        outs = _outputs(dev, _image_specs((M, nby, nbz), 2, 1), into, torch.empty,  # (the call zeroes them)
                        f"into: contiguous int64 counts and float64 re, im of shape [{M}, {nby}, {nbz}] on {dev}", f"into: skipped is one int64 on {dev}")
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:
            return _untouched(outs, into)
        abi.check(self.lib.ot_monitor_field_many(self._ctx, (abi.OtMonitor * M)(*mons), M, _doubles(axes), _doubles(edges), nby, nbz, C.byref(src),
                                                 segs.field("intensity").data_ptr(), segs.field("n").data_ptr(), segs.field("pathlength").data_ptr(),
                                                 *wavelength, int(amplitude_mode), n_segments, _address(count), n_rays,
                                                 *(t.data_ptr() for t in outs), 0 if into is None else 1), self.lib)
        return outs

    def monitor_beam_many(self, monitor_structs, axes, edges, bins, segs: SegmentBatch, wavelength, into=None):
        """Gaussian-beam detector images of a list of monitors over a SegmentBatch read as it lies, either precision
        (ot_monitor_beam_many: `monitor_image_many` with every hit's intensity spread over its Gaussian spot, from the segments'
        q, n and the wavelength).  axes, edges, bins as there.  wavelength: a float for all rays, or a float64 device tensor indexed
        by the segments' `ray`.  Returns (counts, power, skipped): int64 / float64 [M, nby, nbz] device tensors and an int64 device
        tensor of one element (hits left out: no q, or an unusable ray, wavelength or index), zeroed by the call — or `into`, such
        a tuple from an earlier call, with this call's hits added to it."""
        with self.lock:
            return self._monitor_beam_many(list(monitor_structs), axes, edges, bins, segs, wavelength, into)

    def _monitor_beam_many(self, mons, axes, edges, bins, segs, wavelength, into):
        dev, M, (nby, nbz) = segs.device, len(mons), bins
        axes, edges = _image_tables(M, nby, nbz, axes, edges)
        wavelength = _wavelength_arg(wavelength, dev)
        outs = _outputs(dev, _image_specs((M, nby, nbz), 1, 1), into, torch.empty,  # (the call zeroes them)
                        f"into: contiguous int64 counts and float64 power of shape [{M}, {nby}, {nbz}] on {dev}", f"into: skipped is one int64 on {dev}")
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:
            return _untouched(outs, into)
        abi.check(self.lib.ot_monitor_beam_many(self._ctx, (abi.OtMonitor * M)(*mons), M, _doubles(axes), _doubles(edges), nby, nbz, C.byref(src),
                                                segs.field("intensity").data_ptr(), segs.field("q_re").data_ptr(), segs.field("q_im").data_ptr(),
                                                segs.field("n").data_ptr(), *wavelength, n_segments, _address(count), n_rays,
                                                *(t.data_ptr() for t in outs), 0 if into is None else 1), self.lib)
        return outs

    def monitor_wave_many(self, monitor_structs, axes, edges, bins, segs: SegmentBatch, wavelength, amplitude_mode=0, gouy=0, into=None):
        """Coherent Gaussian-beam detector images of a list of monitors over a double-precision SegmentBatch read as it lies
        (ot_monitor_wave_many: `monitor_field_many` with every hit a Gaussian beam — envelope, wavefront curvature and tilt from the
        segments' q, n and direction — sampled at the bin centres).  axes, edges, bins, wavelength, amplitude_mode as there; gouy: 1
        subtracts atan2(Re q, Im q) from every hit's phase.  Returns (counts, re, im, skipped, aliased): int64 / float64 / float64
        [M, nby, nbz] device tensors and two int64 device tensors of one element (hits left out: no q, or an unusable ray, wavelength
        or index; hits whose phase turns more than half a cycle a bin somewhere on their footprint, deposited all the same), zeroed
        by the call — or `into`, such a tuple from an earlier call, with this call's hits added to it."""
        with self.lock:
            return self._monitor_wave_many(list(monitor_structs), axes, edges, bins, segs, wavelength, amplitude_mode, gouy, into)

    def _monitor_wave_many(self, mons, axes, edges, bins, segs, wavelength, amplitude_mode, gouy, into):
        dev, M, (nby, nbz) = segs.device, len(mons), bins
        axes, edges = _image_tables(M, nby, nbz, axes, edges)
        if segs.precision != "f64":
            raise ValueError("a beam field needs double-precision segments")
        wavelength = _wavelength_arg(wavelength, dev)
        outs = _outputs(dev, _image_specs((M, nby, nbz), 2, 2), into, torch.empty,  # (the call zeroes them)
                        f"into: contiguous int64 counts and float64 re, im of shape [{M}, {nby}, {nbz}] on {dev}",
                        f"into: skipped and aliased are one int64 each on {dev}")
        src, n_segments, count, n_rays = segment_source(segs)
        if M == 0 or n_segments == 0:
            return _untouched(outs, into)
        abi.check(self.lib.ot_monitor_wave_many(self._ctx, (abi.OtMonitor * M)(*mons), M, _doubles(axes), _doubles(edges), nby, nbz, C.byref(src),
                                                segs.field("intensity").data_ptr(), segs.field("n").data_ptr(), segs.field("pathlength").data_ptr(),
                                                segs.field("q_re").data_ptr(), segs.field("q_im").data_ptr(), *wavelength, int(amplitude_mode),
                                                int(gouy), n_segments, _address(count), n_rays, *(t.data_ptr() for t in outs),
                                                0 if into is None else 1), self.lib)
        return outs

    # -- measurement ---------------------------------------------------------------------------
    def timing(self, enabled=True):
        abi.check(self.lib.ot_timing_enable(self._ctx, int(enabled)), self.lib)
        abi.check(self.lib.ot_timing_reset(self._ctx), self.lib)

    def timing_reset(self):
        abi.check(self.lib.ot_timing_reset(self._ctx), self.lib)

    def timing_read(self):
        ms, cnt = C.c_double(), C.c_int64()
        abi.check(self.lib.ot_timing_read(self._ctx, C.byref(ms), C.byref(cnt)), self.lib)
        return ms.value, cnt.value

    def set_option(self, option, value):
        self._resident_plans = {}
        self._first_plans = {}
        abi.check(self.lib.ot_set_option(self._ctx, option, value), self.lib)
        if option == abi.OPT_APPEND_CHUNK:
            self.append_chunk = int(value)  # (the capacity estimates of the append layout count holes in chunks)
        if option == abi.OPT_TREES_REFILL_AT:
            self.trees_refill_at = int(value)  # (what the caller asked for: trace_branching's own choice for a batch, `_refill_at`, does not come through here)

    def stream_ceiling(self, rays: RayBatch, max_segments, out: SegmentBatch):
        """Same bytes as `trace` with no tracing (roofline companion), in the layout of `out` (slots or tiled): fields the batch
        knows to be uniform are read once per wave here too."""
        out.forget_resident()  # (the ceiling writes whole records of its own into `out`)
        if out.count is None or out.count.numel() != rays.n:
            out.count = torch.empty(rays.n, dtype=torch.int32, device=rays.device)
        if out.tiled:
            rs = rays.c_struct()
            abi.check(self._fn("ot_bench_stream_tiled_uniform", rays.precision)(self._ctx, C.byref(rs), rays.n, int(max_segments), out.block.data_ptr(), out.capacity, out.count.data_ptr(), rays.uniform_mask), self.lib)
            return
        rs, ss = rays.c_struct(), out.c_struct()
        abi.check(self._fn("ot_bench_stream_uniform", rays.precision)(self._ctx, C.byref(rs), rays.n, int(max_segments), C.byref(ss),
                                                                      out.count.data_ptr(), rays.uniform_mask), self.lib)

    def last_launch(self):
        """Shape of the last trace launch (include/optable_hip.h: ot_debug_last_launch) as a dict."""
        info = (C.c_int32 * 8)()
        abi.check(self.lib.ot_debug_last_launch(self._ctx, C.byref(info)), self.lib)
        keys = ("kernel", "threads", "workgroups_per_cu", "workgroups", "lds_bytes", "list_cap", "mixed", "pair_queue")  # pair_queue: bit flags, see the header
        return dict(zip(keys, (int(v) for v in info)))

    def generation_mismatches(self):
        """Diagnostic counter of the two-pass generation kernels (include/optable_hip.h); expected 0."""
        v = C.c_int64()
        abi.check(self.lib.ot_debug_generation_mismatches(self._ctx, C.byref(v)), self.lib)
        return v.value

    def synchronize(self):
        abi.check(self.lib.ot_ctx_synchronize(self._ctx), self.lib)


def _grow(segs, capacity, n_keep):
    big = SegmentBatch(capacity, segs.precision, segs.device)
    for f in abi.SEG_FIELDS + ("ray", "surface"):
        big.field(f)[:n_keep].copy_(segs.field(f)[:n_keep])
    return big


def get_engine(device=None) -> Engine:
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _engines:
        _engines[device] = Engine(device)
    return _engines[device]
