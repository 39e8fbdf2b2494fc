"""OpticalTable: scene container whose `ray_tracing` runs on the MI355X engine.

Drop-in for optable/optical_table.py:9-147 (`add_components`, `add_monitors`, `ray_tracing`
with the misspelt `perfomance_limit` kwarg, `.rays` accumulating across calls, a deep copy
returned).  What changes is where the work happens: the component list is compiled to flat
tables (scene.py), the rays are packed structure-of-arrays into HBM (batch.py) and
liboptable_hip.so traces every ray tree; `Ray` objects are rebuilt from the segment stream
only at the end.  `trace_batch` is the same path without Python objects, for 1e6+ rays.

The wall-clock cap (`perfomance_limit["max_trace_time"]`, 600 s by default, optical_table.py:84-97) is honoured
where a trace takes more than one launch: ray trees that go generation by generation read the clock after each
(engine.trace_tree), and say where they are once per second as the reference's loop does (optical_table.py:99-111).  A
non-branching scene, and a batch of ray trees whose queues fit the chip (engine.trace_trees), is ONE launch bounded by
`max_trace_num`: milliseconds, nothing can be cut inside it.  Render / GUI are out of scope.
"""
import copy
from typing import List, Union

import numpy as np

from . import abi
from .assemblies import *  # noqa: F401,F403  (reference re-exports, optical_table.py:1-3)
from .components import *  # noqa: F401,F403
from .components import OpticalComponent
from .geometry import base_merge_bboxs, _NO_BOX, out_of_scope
from .monitors import Monitor, check_weight
from .rays import Ray
from .scene import compile_scene

MAX_TRACE_NUM = 2000  # optical_table.py:87
MAX_TRACE_TIME = 600.0  # seconds, optical_table.py:86
_FUSED_MAX_SEGMENTS = 64


def _engine():
    from .engine import get_engine  # imports torch + the HIP library lazily

    return get_engine()


class OpticalTable:
    render = out_of_scope("render")
    gather_components = out_of_scope("gather_components")
    export_components_csv = out_of_scope("export_components_csv")
    add_wavelength_legend = out_of_scope("add_wavelength_legend")

    def __init__(self, **kwargs):
        self.components = []
        self.rays = []
        self.monitors = []
        self.norender_set = set()
        self._bbox = _NO_BOX
        self.unit = kwargs.get("unit", 1e-2)

    # -- scene building (optical_table.py:25-43) ------------------------------------------------
    def add_components(self, component: Union[OpticalComponent, List]):
        self._collect(component, self.components, OpticalComponent)

    def add_monitors(self, monitor: Union[Monitor, List]):
        self._collect(monitor, self.monitors, Monitor)

    @staticmethod
    def _collect(item, sink, cls):
        if isinstance(item, cls):
            sink.append(item)
        elif isinstance(item, list):
            for entry in item:
                if isinstance(entry, cls):
                    sink.append(entry)
                elif isinstance(entry, list):
                    sink.extend(entry)

    @property
    def bbox(self):
        if self._bbox[0] is None:
            self.get_bbox()
        return self._bbox

    def get_bbox(self):
        self._bbox = base_merge_bboxs([c.bbox for c in self.components])
        return self._bbox

    accelerate = True  # attach the acceleration grids (scene.py); results do not depend on it
    # trace non-planar user surfaces that no built-in shape reproduces as verified 3-D Chebyshev series of their f (implicit.py)
    # instead of refusing them.  ray_tracing checks every hit on such a surface against the user's within_boundary and f;
    # trace_batch does not, and opting in is the user's acceptance of the measured aperture there.
    implicit_surfaces = False

    def compile(self):
        """Flatten the current components into device tables (poses are read now)."""
        return compile_scene(self.components, self.unit, accelerate=self.accelerate, implicit_surfaces=self.implicit_surfaces)

    # -- the hot path ---------------------------------------------------------------------------
    def ray_tracing(self, rays: Union[Ray, List[Ray]], perfomance_limit=None):
        """Trace `rays`; append the finished segments to `self.rays`; return a deep copy of
        everything accumulated so far (optical_table.py:57-72)."""
        if isinstance(rays, Ray):
            rays = [rays]
        cap, max_time = MAX_TRACE_NUM, MAX_TRACE_TIME
        if perfomance_limit is not None and "max_trace_num" in perfomance_limit:
            cap = int(perfomance_limit["max_trace_num"])
        if perfomance_limit is not None and "max_trace_time" in perfomance_limit:
            max_time = float(perfomance_limit["max_trace_time"])
        if len(rays) and cap > 0 and max_time > 0:  # the reference's loop does not start on an exhausted limit
            traced, capped = self._trace_objects(list(rays), cap, max_time)
            if capped:
                # the reference prints the number of traces its loop got through (optical_table.py:138-143): `cap` when
                # the count limit cut a tree, what was done by then when the clock did (the clock here runs over the
                # whole call and is read after every generation of the batch, not per input ray)
                done = min(cap, self._last_trace_num) if getattr(self, "_last_trace_num", None) else cap
                print(f"Ray tracing time exceeds the maximum tracing time after {done} traces. "
                      f"({capped} ray tree(s) truncated)")
            self.rays.extend(traced)
        elif len(rays):  # an exhausted limit: the reference's loop does not start, nothing is archived, the message is printed
            print(f"Ray tracing time exceeds the maximum tracing time after 0 traces. ({len(rays)} ray tree(s) truncated)")
        return _clone_rays(self.rays)

    def trace_batch(self, batch, max_segments=None, counts=None, scene=None, layout="auto", capacity=None):
        """Scalable entry: `RayBatch` in, `SegmentBatch` out, no Python objects.  Non-branching
        scenes run as one launch with [segment][ray] output slots; branching scenes run generation by
        generation; both in the batch's precision.
        `scene`: a `table.compile()` result to reuse when the components have not changed since (flattening
        a few hundred components in Python costs milliseconds — 10 ms for cfg 5 — and the engine skips the
        upload when it already holds that very scene); default: compile now, poses are read at call time.
        `layout`: "auto" (the default: what the scene's kernels write fastest on this device, Engine.plan — the dense
        "append" list for heavy scenes, "tiled" or "slots" for light ones, whichever the device streams faster), "slots"
        ([segment][ray] slots), "tiled" (the same slots in 64-slot tiles) or "append" (a dense list in append order,
        `capacity` slots: see Engine.trace) for the non-branching launch; ray trees come back as [k][tree] slots when one
        launch takes them (Engine.trace_branching: light scenes, caps whose queues fit the LDS) and as a list in generation
        order otherwise.  Every reader of a SegmentBatch takes all of them."""
        eng = _engine()
        if scene is None:
            scene = self.compile()
        with eng.lock:
            eng.upload(scene)
            cap = MAX_TRACE_NUM if max_segments is None else int(max_segments)
            if scene.limited:
                return self._trace_batch_limited(eng, scene, batch, cap, max_segments is not None, counts)
            speculate = scene.max_children == 2 and not scene.always_branches
            if max_segments is not None and (scene.max_children <= 1 or speculate):
                # max_children == 2: speculate that no tree actually branches (e.g. mirror-coated
                # interfaces only split on total internal reflection); fall back when one does.
                segs = eng.trace(batch, cap, layout=layout, capacity=capacity)
                if scene.max_children <= 1 or not bool((segs.count < 0).any()):
                    return segs
            return eng.trace_branching(batch, cap)

    def _trace_batch_limited(self, eng, scene, batch, cap, fused_ok, counts):
        """`trace_batch` for scenes with `max_interact_count` surfaces.  Their counters are keyed by ray id
        (optical_component.py:140-149): the device table has one column per DISTINCT id of the batch
        (`segs.count_ids` names the columns, ascending), and rays that share an id — copies made by
        `multiplexed_in_wavelength`, explicit duplicates — must see each other's updates in input order,
        as the reference finishes one input ray before it starts the next (optical_table.py:66-70).  Rays
        of one id are therefore traced in successive rounds (round r = the r-th ray of every id) over the
        same table; rays with different ids never interact, so a round is one ordinary launch."""
        import torch
        from .batch import SegmentBatch

        n, dev = batch.n, batch.device
        uniq, inverse = torch.unique(batch.id, return_inverse=True)
        n_classes, n_slots = int(uniq.numel()), len(scene.limited)
        if counts is None:
            counts = torch.zeros((n_slots, max(n_classes, 1)), dtype=torch.int32, device=dev)
        elif tuple(counts.shape) != (n_slots, n_classes):
            raise ValueError(f"counts must be [{n_slots}, {n_classes}] (limited surfaces x distinct ray ids)")
        work = batch.with_ids(inverse)
        fused = fused_ok and scene.max_children <= 1

        def run(sub):
            # (a run holds every id once: the lane-per-tree kernel's FIFO order per tree is the reference's)
            return eng.trace(sub, cap, counts=counts) if fused else eng.trace_branching(sub, cap, counts=counts, distinct_ids=True)

        if n_classes == n:
            segs = run(work)
            segs.count_ids = uniq
            return segs
        order = torch.argsort(inverse, stable=True)
        grouped = inverse[order]
        rounds = torch.empty(n, dtype=torch.int64, device=dev)
        rounds[order] = torch.arange(n, device=dev) - torch.searchsorted(grouped, grouped)
        parts = []
        for r in range(int(rounds.max()) + 1):
            idx = torch.nonzero(rounds == r).flatten()  # ascending: input order inside a round
            parts.append((idx, run(work.take(idx))))
        if fused:  # [k][ray] slots of the whole batch
            out = SegmentBatch(n * cap, batch.precision, dev)
            out.count, out.n_rays = torch.empty(n, dtype=torch.int32, device=dev), n
            for idx, part in parts:
                m = int(idx.numel())
                out.count[idx] = part.count
                for f in abi.SEG_FIELDS + ("surface",):
                    out.field(f).view(cap, n)[:, idx] = part.field(f).view(cap, m)
                out.ray.view(cap, n)[:, idx] = idx.to(torch.int32).unsqueeze(0).expand(cap, m)
        else:  # flat lists: concatenate, tree indices back to positions in `batch`
            def valid(part):  # slots a round's trace filled: the first n_valid of a list; of [k][tree] slots (lane-per-tree launch) row by
                if part.count is None:  # row, which keeps every tree's rays in their FIFO order
                    return slice(0, part.n_valid), part.n_valid
                keep = part.valid_mask()
                return keep, int(keep.sum().item())

            picks = [valid(part) for _, part in parts]
            total = sum(v for _, v in picks)
            out = SegmentBatch(total, batch.precision, dev)
            out.capped = torch.zeros(n, dtype=torch.bool, device=dev)
            at = 0
            for (idx, part), (keep, v) in zip(parts, picks):
                for f in abi.SEG_FIELDS + ("surface",):
                    out.field(f)[at:at + v] = part.field(f)[keep]
                out.ray[at:at + v] = idx[part.ray[keep].long()].to(torch.int32)
                out.capped[idx] = part.capped
                at += v
            out.n_valid = total
        out.counts_table, out.count_ids = counts, uniq
        return out

    def trace_host(self, origin, direction, **kwargs):
        """Host numpy rays in, host numpy results out, PCIe copies overlapped with the trace (stream.py)."""
        from .stream import trace_host

        return trace_host(self, origin, direction, **kwargs)

    def record_batch(self, monitor, segs):
        """Monitor.record over a SegmentBatch without Python objects: a `MonitorHits` (device tensors
        + the Monitor accessors: yList, tYList, IList, ... with the reference's sort orders)."""
        from .monitors import MonitorHits

        segs = segs.to_slots()  # a tiled history: as slot arrays (the accessors index segments by slot)
        slot, P, t = _engine().monitor_record(monitor_struct(monitor), segs)
        return MonitorHits(monitor, segs, slot, P, t)

    def record_all(self, segs, monitors=None):
        """`record_batch` for every monitor of the table (optical_table.py:145-146), or for those given: one `MonitorHits` per
        monitor, in their order, from ONE pass over the segments read as they lie (any layout, either precision)."""
        from .monitors import MonitorHits

        monitors = list(self.monitors if monitors is None else monitors)
        found = _engine().monitor_record_many([monitor_struct(m) for m in monitors], segs)
        return [MonitorHits(m, segs, slot, P, t) for m, (slot, P, t) in zip(monitors, found)]

    def _images_all(self, cls, mode, segs, bins, monitors, into, *args, left_out=None, **kwargs):
        """What image_all, field_all, beam_all and wave_all do alike once their own arguments are checked: the monitors' edge and
        axes tables, `into` (the list an earlier call of the same mode returned) as that call's tensors, the engine's
        monitor_<mode>_many with `args`, and one `cls` per monitor.  A mode that counts hits left out (its tensor follows the
        images) raises for them, `left_out` naming the causes.  Returns (the list, the engine's tensors — None where `into` had no
        monitors to ask for)."""
        from .monitors import image_edges

        nby, nbz = bins
        monitors = list(self.monitors if monitors is None else monitors)
        edges = [image_edges(m, nby, nbz) for m in monitors]
        stack = None
        if into is not None:
            into, stack = _into_stack(into, len(monitors), lambda k, im: isinstance(im, cls) and im.monitor is monitors[k] and im.bins == bins,
                                      f"into: the list an earlier {mode}_all returned for the same monitors and bins")
            if not monitors:
                return into, None
        axes = _monitor_axes(monitors)
        table = np.array([np.concatenate(e) for e in edges], dtype=float).reshape(len(monitors), nby + nbz + 2)
        outs = getattr(_engine(), f"monitor_{mode}_many")([monitor_struct(m) for m in monitors], axes, table, bins, segs, *args, into=stack, **kwargs)
        images = 1 + len(cls.PLANES)  # counts and the planes; then the tallies, the hits left out first
        n_left_out = int(outs[images].item()) if left_out else 0
        if n_left_out:
            raise ValueError(f"{mode}_all: {n_left_out} hits left out — {left_out}")
        if into is None:
            into = [cls(m, *(t[k] for t in outs[:images]), ey, ez, stack=(*outs, k)) for k, (m, (ey, ez)) in enumerate(zip(monitors, edges))]
        return into, outs

    def image_all(self, segs, bins=30, monitors=None, into=None):
        """Every monitor of the table (or those given) as an image: one `MonitorImage` per monitor, in their order — the hits
        of `record_all` binned on the device in the same pass that finds them, with no hit list (ot_monitor_image_many).  The
        image of a monitor is np.histogram2d of its `yList` / `zList` with `bins` (an int or (nby, nbz)) equal bins over
        +-width / 2, +-height / 2, weighted by `IList` (Monitor.render_hist: bins=30).  `into`: the list an earlier call with the
        same monitors and bins returned; this call's hits are added to those images (a detector summed over the chunks of a
        streamed trace)."""
        from .monitors import MonitorImage, image_bins

        return self._images_all(MonitorImage, "image", segs, image_bins(bins), monitors, into)[0]

    def image_batch(self, monitor, segs, bins=30):
        """One monitor as an image (`image_all` for it alone): a `MonitorImage`."""
        return self.image_all(segs, bins=bins, monitors=[monitor])[0]

    def fluence_map(self, segs, view="Z", roi=None, pixels=256, weight="intensity", into=None):
        """The segments as an image of a projected view — `render(type=view, roi=roi)` as numbers: a `FluenceMap` whose pixels
        hold the number of segment pieces inside them and the intensity-weighted path length of those pieces, rasterised on the
        device from the segments as they lie (any layout, either precision; ot_fluence_map).  view: "Z", "X" or "Y" — the image
        axes are the lab axes (x, y), (y, z), (z, x) and the third is the depth; roi = (x0, x1, y0, y1, z0, z1) as `render` takes
        it (default: the table's `get_bbox()`), a depth bound may be infinite; pixels: an int or (nu, nv) equal pixels over the
        roi's image ranges; weight: "intensity" or "none" (plain path length).  A segment that runs on without end inside the
        box — the unbounded last segment of a ray, with an infinite depth range — deposits nothing and is counted in `skipped`.
        `into`: the `FluenceMap` an earlier call with the same view, roi, pixels and weight returned; this call's segments are
        added to it (the chunks of a streamed trace)."""
        from .fluence import FluenceMap, fluence_view

        check_weight(weight)
        if roi is None:
            if not self.components:
                raise ValueError("roi=None takes the table's get_bbox(), and this table has no components: pass roi")
            roi = self.get_bbox()
        axes, u_edges, v_edges, depth, roi = fluence_view(view, roi, pixels)
        stack = None
        if into is not None:
            if not isinstance(into, FluenceMap) or (into.view, into.roi, into.pixels, into.weight) != (view, roi, (len(u_edges) - 1, len(v_edges) - 1), weight):
                raise ValueError("into: the FluenceMap an earlier fluence_map returned for the same view, roi, pixels and weight")
            stack = (into.counts, into.fluence, into._skipped)
        counts, fluence, skipped = _engine().fluence_map(axes, u_edges, v_edges, depth, segs, weighted=weight == "intensity", into=stack)
        if into is not None:
            return into
        return FluenceMap(view, roi, weight, counts, fluence, skipped, u_edges, v_edges)

    def spots_all(self, segs, offsets=(0.0,), monitors=None, weight="intensity", centre=None, into=None):
        """Every monitor of the table (or those given) as SPOT STATISTICS: one `MonitorSpots` per monitor, in their order — the
        count, the power and the first and second moments of the hits of `record_all`, on the monitor and on every plane displaced
        by one of `offsets` along its normal (a through-focus scan from one trace), summed on the device in the pass that finds the
        hits, with no hit list and no image (ot_monitor_spots_many).  A plane is tested as a monitor of the same size built at
        the displaced pose would be.  The coordinates are the images': the local hit point on the monitor's lab tangents, less
        `centre`.  weight: "intensity" or "none" (every hit weighs 1).  centre: None, one (y, z) for all monitors or one per
        monitor — a point near the spot, which keeps a small spot far from the monitor's centre from losing its variance to
        cancellation; `MonitorSpots.centroid()` adds it back.  Counts are exact and the sums the same bits every run.  `into`: the
        list an earlier call with the same monitors, offsets, weight and centre returned; this call's hits are added to it (the
        chunks of a streamed trace)."""
        from .spots import MonitorSpots, spot_centres, spot_offsets

        check_weight(weight)
        monitors = list(self.monitors if monitors is None else monitors)
        offsets, centres = spot_offsets(offsets), spot_centres(centre, len(monitors))
        stack = None
        if into is not None:
            into, stack = _into_stack(into, len(monitors), lambda k, sp: isinstance(sp, MonitorSpots) and sp.monitor is monitors[k] and sp.weight == weight
                                      and sp.centre == tuple(centres[k]) and np.array_equal(sp.offsets, offsets),
                                      "into: the list an earlier spots_all returned for the same monitors, offsets, weight and centre")
            if not monitors:
                return into
        counts, sums = _engine().monitor_spots_many([monitor_struct(m) for m in monitors], _monitor_axes(monitors), centres, offsets, segs,
                                                    weighted=weight == "intensity", into=stack)
        if into is None:
            into = [MonitorSpots(m, offsets, counts[k], sums[k], weight, centres[k], stack=(counts, sums, k)) for k, m in enumerate(monitors)]
        return into

    def spots_batch(self, monitor, segs, offsets=(0.0,), weight="intensity", centre=None):
        """One monitor as spot statistics (`spots_all` for it alone): a `MonitorSpots`."""
        return self.spots_all(segs, offsets=offsets, monitors=[monitor], weight=weight, centre=centre)[0]

    def spots_grouped_all(self, segs, groups, n_groups=None, offsets=(0.0,), monitors=None, weight="intensity", centre=None, into=None, labels=None):
        """`spots_all` PER RAY GROUP: one `MonitorSpotGroups` per monitor, in their order — the count and the six moments of the hits
        of every (plane, group), from one pass over the segments (ot_monitor_spot_groups_many).  groups: one integer id per INPUT
        ray of the trace (an array or tensor; `RayBatch.groups_by_wavelength()` gives one group per wavelength); a hit belongs to
        the group of the ray its segment descends from, whatever the layout and wherever in a ray tree.  n_groups = G, 1 .. 256
        (None: max id + 1); rays whose id is outside 0 .. G - 1 are in no group, so -1 masks a ray.  offsets, monitors, weight and
        centre as for `spots_all`; labels: what the groups stand for, one per group, kept on the results.  One trace of a batch
        multiplexed in wavelength gives the chromatic focal shift (`MonitorSpotGroups.best_focus()`), one of several field points
        the field curvature.  Counts are exact and the sums the same bits every run.  `into`: the list an earlier call with the
        same monitors, offsets, weight, centre and G returned; this call's hits are added to it, with this call's `groups` (the
        chunks of a streamed trace each bring their own table)."""
        from .spots import MonitorSpotGroups, spot_centres, spot_group_ids, spot_offsets

        check_weight(weight)
        monitors = list(self.monitors if monitors is None else monitors)
        offsets, centres = spot_offsets(offsets), spot_centres(centre, len(monitors))
        ids, G = spot_group_ids(groups, segs.n_rays, n_groups, device=segs.device)
        if labels is not None and len(labels) != G:
            raise ValueError(f"labels: one per group ({G}), not {len(labels)}")
        stack = None
        if into is not None:
            into, stack = _into_stack(into, len(monitors), lambda k, sp: isinstance(sp, MonitorSpotGroups) and sp.monitor is monitors[k]
                                      and sp.weight == weight and sp.centre == tuple(centres[k]) and np.array_equal(sp.offsets, offsets)
                                      and sp.n_groups == G,
                                      "into: the list an earlier spots_grouped_all returned for the same monitors, offsets, weight, centre and n_groups")
            if not monitors:
                return into
        counts, sums = _engine().monitor_spot_groups_many([monitor_struct(m) for m in monitors], _monitor_axes(monitors), centres, offsets, ids, G, segs,
                                                          weighted=weight == "intensity", into=stack)
        if into is None:
            into = [MonitorSpotGroups(m, offsets, counts[k], sums[k], weight, centres[k], labels=labels, stack=(counts, sums, k))
                    for k, m in enumerate(monitors)]
        return into

    def spots_grouped_batch(self, monitor, segs, groups, n_groups=None, offsets=(0.0,), weight="intensity", centre=None, labels=None):
        """One monitor as spot statistics per ray group (`spots_grouped_all` for it alone): a `MonitorSpotGroups`."""
        return self.spots_grouped_all(segs, groups, n_groups=n_groups, offsets=offsets, monitors=[monitor], weight=weight, centre=centre, labels=labels)[0]

    def wavefront_all(self, segs, focus=None, direction=None, pupil=None, coordinates=None, monitors=None, weight="intensity", piston=None,
                      into=None):
        """Every monitor of the table (or those given) as a WAVEFRONT: one `MonitorWavefront` per monitor, in their order — the
        optical path W of every hit of `record_all` against an ideal wave, reduced on the device, in the pass that finds the hits
        and with no hit list, to the moments a Zernike fit up to radial order 4 and the rms wavefront error need
        (ot_monitor_wavefront_many).  Exactly one of `focus` (a point F: the spherical wave that converges on F or diverges from
        it; W is the optical path at the foot of the perpendicular from F onto the ray — the reference sphere at infinity, which
        differs from a sphere of radius R_s by n e^2 / (2 R_s), e the ray's miss distance at F) or `direction` (a vector u: the
        plane wave along it), in the lab frame, one for all monitors or one per monitor.  `pupil` = (c_y, c_z, R), one for all or
        one per monitor: the hits with (p, q) = ((y - c_y) / R, (z - c_z) / R) inside the unit disc take part, the others are
        counted in `outside`; (y, z) are the hit's `yList` / `zList` (coordinates "position" or 1, the default with `direction`,
        where `pupil` defaults to (0, 0, min(width, height) / 2)) or its `tYList` / `tZList` ("direction" or 0, the default with
        `focus`, where `pupil` is required).  weight: "intensity" or "none".  `piston`: a number, or one per monitor, subtracted
        from W before it is summed; None: one extra pass — the call reduces with piston 0 and again with the mean it finds (0 for a
        monitor without a hit).  The value is kept on the result.  `into`: the list an earlier call with the same monitors,
        reference, pupil, coordinates and weight returned; this call's hits are added to it with ITS piston (the chunks of a
        streamed trace use the first chunk's), which an explicit `piston` must equal.  `segs` must be double precision."""
        from .wavefront import COORDINATES, MonitorWavefront, wavefront_coordinates, wavefront_piston, wavefront_pupil, wavefront_reference

        check_weight(weight)
        monitors = list(self.monitors if monitors is None else monitors)
        M = len(monitors)
        kind, lab, local = wavefront_reference(focus, direction, monitors)
        pupils, coords = wavefront_pupil(pupil, kind, monitors), wavefront_coordinates(coordinates, kind)
        pistons = None if piston is None else wavefront_piston(piston, M)
        if segs.precision != "f64":
            raise ValueError("wavefront_all needs a double-precision SegmentBatch: a path length in single precision is a hundredth of a wave wrong at table scale")
        name = ("focus", "direction")[kind]
        stack = None
        if into is not None:
            into, stack = _into_stack(into, M, lambda k, wf: isinstance(wf, MonitorWavefront) and wf.monitor is monitors[k] and wf.weight == weight
                                      and wf.reference == (name, tuple(lab[k])) and wf.pupil == tuple(pupils[k]) and wf.coordinates == COORDINATES[coords],
                                      "into: the list an earlier wavefront_all returned for the same monitors, reference, pupil, coordinates and weight")
            if pistons is not None and any(wf.piston != float(v) for wf, v in zip(into, pistons)):
                raise ValueError("into: piston must be None or the piston of the earlier call")
            if not monitors:
                return into
            pistons = np.array([wf.piston for wf in into], dtype=np.float64)
        axes, structs = _monitor_axes(monitors), [monitor_struct(m) for m in monitors]

        def reduce(p, out):
            return _engine().monitor_wavefront_many(structs, axes, kind, local, coords, pupils, p, segs, weighted=weight == "intensity", into=out)

        if pistons is None:  # the mean of W with piston 0, then the sums about it
            _, first = reduce(np.zeros(M), None)
            first = first.cpu().numpy()
            with np.errstate(all="ignore"):
                pistons = np.where(first[:, 0] != 0.0, first[:, 45] / first[:, 0], 0.0)
            pistons = np.ascontiguousarray(np.where(np.isfinite(pistons), pistons, 0.0))
        counts, sums = reduce(pistons, stack)
        if into is None:
            into = [MonitorWavefront(m, counts[k, 0], counts[k, 1], sums[k], (name, lab[k]), pupils[k], COORDINATES[coords], pistons[k], weight,
                                     stack=(counts, sums, k)) for k, m in enumerate(monitors)]
        return into

    def wavefront_batch(self, monitor, segs, focus=None, direction=None, pupil=None, coordinates=None, weight="intensity", piston=None):
        """One monitor as a wavefront (`wavefront_all` for it alone): a `MonitorWavefront`."""
        return self.wavefront_all(segs, focus=focus, direction=direction, pupil=pupil, coordinates=coordinates, monitors=[monitor], weight=weight,
                                  piston=piston)[0]

    def wavefront_grouped_all(self, segs, groups, n_groups=None, focus=None, direction=None, pupil=None, coordinates=None, monitors=None,
                              weight="intensity", piston=None, into=None, labels=None):
        """`wavefront_all` PER RAY GROUP: one `MonitorWavefrontGroups` per monitor, in their order — the 61 sums, and so the Zernike
        fit, the rms wavefront error and Marechal's Strehl ratio, of every group of input rays from one trace
        (ot_monitor_wavefront_groups_many): each colour's defocus from a batch multiplexed in wavelength, each field point's coma and
        astigmatism from one multiplexed in field.  groups, n_groups (G, 1 .. 256, with monitors x G <= 4096) and labels as for
        `spots_grouped_all`: one integer id per INPUT ray, a hit belongs to the group of the ray its segment descends from, ids
        outside 0 .. G - 1 are in no group and in no tally (-1 masks a ray).  Every field point has its own image point and pupil
        centre, so `focus` / `direction`, `pupil` and `piston` are taken PER (monitor, group), each in one of these shapes: one for
        all; one per monitor [M, ...]; one per group [G, ...] — only when M != G: a shape that could be either is read as per
        MONITOR; or [M, G, ...].  coordinates, weight and the meaning of every argument as for `wavefront_all`; `piston=None` is
        its two-call scheme per cell (the mean of W of every (monitor, group), 0 for an empty one).  A call is ceil(M G / 28) passes
        over the segments.  Counts are exact and the sums the same bits every run; group g equals `wavefront_all` over the rays of
        group g alone with that group's reference, pupil and piston, bit for bit.  `into`: the list an earlier call with the same
        monitors, G, references, pupils, coordinates and weight returned; this call's hits are added to it with ITS pistons and
        this call's `groups` (the chunks of a streamed trace each bring their own table).  `segs` must be double precision."""
        from .spots import spot_group_ids
        from .wavefront import (COORDINATES, MonitorWavefrontGroups, wavefront_coordinates, wavefront_group_piston, wavefront_group_pupil,
                                wavefront_group_reference)

        check_weight(weight)
        monitors = list(self.monitors if monitors is None else monitors)
        M = len(monitors)
        ids, G = spot_group_ids(groups, segs.n_rays, n_groups, device=segs.device)
        if labels is not None and len(labels) != G:
            raise ValueError(f"labels: one per group ({G}), not {len(labels)}")
        if M:
            from .engine import wavefront_groups_plan

            wavefront_groups_plan(M, G)
        kind, lab, local = wavefront_group_reference(focus, direction, monitors, G)
        pupils, coords = wavefront_group_pupil(pupil, kind, monitors, G), wavefront_coordinates(coordinates, kind)
        pistons = None if piston is None else wavefront_group_piston(piston, M, G)
        if segs.precision != "f64":
            raise ValueError("wavefront_all needs a double-precision SegmentBatch: a path length in single precision is a hundredth of a wave wrong at table scale")
        name = ("focus", "direction")[kind]
        stack = None
        if into is not None:
            into, stack = _into_stack(into, M, lambda k, wf: isinstance(wf, MonitorWavefrontGroups) and wf.monitor is monitors[k] and wf.weight == weight
                                      and wf.n_groups == G and wf.reference[0] == name and np.array_equal(wf.reference[1], lab[k])
                                      and np.array_equal(wf.pupil, pupils[k]) and wf.coordinates == COORDINATES[coords],
                                      "into: the list an earlier wavefront_grouped_all returned for the same monitors, n_groups, references, pupils, coordinates and weight")
            if pistons is not None and any(not np.array_equal(wf.piston, row) for wf, row in zip(into, pistons)):
                raise ValueError("into: piston must be None or the pistons of the earlier call")
            if not monitors:
                return into
            pistons = np.ascontiguousarray(np.array([wf.piston for wf in into], dtype=np.float64).reshape(M, G))
        axes, structs = _monitor_axes(monitors), [monitor_struct(m) for m in monitors]

        def reduce(p, out):
            return _engine().monitor_wavefront_groups_many(structs, axes, kind, local, coords, pupils, p, ids, G, segs, weighted=weight == "intensity",
                                                           into=out)

        if pistons is None:  # the mean of W of every cell with piston 0, then the sums about it
            _, first = reduce(np.zeros((M, G)), None)
            first = first.cpu().numpy()
            with np.errstate(all="ignore"):
                pistons = np.where(first[..., 0] != 0.0, first[..., 45] / first[..., 0], 0.0)
            pistons = np.ascontiguousarray(np.where(np.isfinite(pistons), pistons, 0.0)).reshape(M, G)
        counts, sums = reduce(pistons, stack)
        if into is None:
            into = [MonitorWavefrontGroups(m, counts[k, :, 0], counts[k, :, 1], sums[k], (name, lab[k]), pupils[k], COORDINATES[coords], pistons[k], weight,
                                           labels=labels, stack=(counts, sums, k)) for k, m in enumerate(monitors)]
        return into

    def wavefront_grouped_batch(self, monitor, segs, groups, n_groups=None, focus=None, direction=None, pupil=None, coordinates=None,
                                weight="intensity", piston=None, labels=None):
        """One monitor as a wavefront per ray group (`wavefront_grouped_all` for it alone): a `MonitorWavefrontGroups`."""
        return self.wavefront_grouped_all(segs, groups, n_groups=n_groups, focus=focus, direction=direction, pupil=pupil, coordinates=coordinates,
                                          monitors=[monitor], weight=weight, piston=piston, labels=labels)[0]

    def psf_all(self, segs, wavelength, focus=None, direction=None, step=None, pixels=65, centre=(0.0, 0.0), monitors=None, amplitude="sqrt",
                into=None):
        """Every monitor of the table (or those given) as a DIFFRACTION IMAGE: one `MonitorPSF` per monitor, in their order — the
        plane waves of the hits of `record_all`, every hit on every sample, summed over a grid of `pixels` samples (an int or
        (ny, nz), 1 .. 512) `step` apart (a number or (dy, dz), required) on the device (ot_monitor_psf_many).  Exactly one of
        `focus` (a point F, lab frame: the samples are the points F + y a_y + z a_z of the plane through F parallel to the monitor,
        `step` is a length, and every ray counts as the plane wave it locally is) or `direction` (a vector u: the samples are the
        directions u + y a_y + z a_z, `step` is in direction cosines — the far field of an afocal system), one for all monitors or
        one per monitor; the optical path of a hit is `wavefront_all`'s W against the same reference.  Sample k of an axis of n lies
        at c + (k - (n - 1) / 2) x step, c from `centre` = (y, z): an odd count puts a sample on the reference itself.
        `wavelength`: one float for all rays, or the `RayBatch` that was traced, as for `field_all`.  amplitude: "sqrt"
        (sqrt(intensity): intensity is a power), "linear" or "unit" (every hit 1).  The model: each ray is a plane-wave sample, so
        the result is the diffraction PSF when the rays sample the direction cosines (`focus`) or the pupil positions
        (`direction`) uniformly, with the intensity as weight, and that distribution's weighted sum for any other; no pi on
        reflection; every hit of a monitor adds to ONE field, whatever its wavelength or field point (`psf_grouped_all` keeps a field per
        group of rays); the image repeats with the period wavelength / (n x ray spacing).  Hits whose phase turns more than half a cycle from one sample to the next are summed all the same, counted in
        `MonitorPSF.aliased` and announced by one RuntimeWarning.  The result is the same bits every run.  `segs` must be double
        precision.  `into`: the list an earlier call with the same monitors, reference, grid and amplitude returned; this call's
        hits are added to it (a field is linear: the chunks of a streamed trace add)."""
        import warnings
        from .psf import MonitorPSF, psf_amplitude, psf_grid
        from .wavefront import wavefront_reference

        monitors = list(self.monitors if monitors is None else monitors)
        M = len(monitors)
        kind, lab, local = wavefront_reference(focus, direction, monitors)
        grid, pixels, step, centres = psf_grid(step, pixels, centre, M)
        mode = psf_amplitude(amplitude)
        if segs.precision != "f64":
            raise ValueError("psf_all needs a double-precision SegmentBatch: a path length in single precision is a hundredth of a wave wrong at table scale")
        wavelength = _wavelengths_of(wavelength, segs, "a PSF")
        name = ("focus", "direction")[kind]
        stack = None
        if into is not None:
            into, stack = _into_stack(into, M, lambda k, p: isinstance(p, MonitorPSF) and p.monitor is monitors[k] and p.amplitude == amplitude
                                      and p.reference == (name, tuple(lab[k])) and p.step == step and p.centre == tuple(centres[k])
                                      and tuple(p.re.shape) == pixels,
                                      "into: the list an earlier psf_all returned for the same monitors, reference, grid and amplitude")
            if not monitors:
                return into
        before = 0 if stack is None else int(stack[0][:, 2].sum().item())
        counts, norm, re, im = _engine().monitor_psf_many([monitor_struct(m) for m in monitors], _monitor_axes(monitors), kind, local, grid, pixels, segs,
                                                          wavelength, amplitude_mode=mode, into=stack)
        if into is None:
            into = [MonitorPSF(m, counts[k], norm[k], re[k], im[k], (name, lab[k]), grid[k], step, centres[k], amplitude, stack=(counts, norm, re, im, k))
                    for k, m in enumerate(monitors)]
        aliased = (int(counts[:, 2].sum().item()) if M else 0) - before
        if aliased > 0:
            warnings.warn(f"psf_all: {aliased} hits are aliased — their phase turns more than half a cycle from one sample to the next, and the "
                          "sampled image means nothing for them: use a smaller step", RuntimeWarning, stacklevel=2)
        return into

    def psf_batch(self, monitor, segs, wavelength, focus=None, direction=None, step=None, pixels=65, centre=(0.0, 0.0), amplitude="sqrt"):
        """One monitor as a diffraction image (`psf_all` for it alone): a `MonitorPSF`."""
        return self.psf_all(segs, wavelength, focus=focus, direction=direction, step=step, pixels=pixels, centre=centre, monitors=[monitor],
                            amplitude=amplitude)[0]

    def psf_grouped_all(self, segs, wavelength, groups, n_groups=None, focus=None, direction=None, step=None, pixels=65, centre=(0.0, 0.0),
                        monitors=None, amplitude="sqrt", labels=None, into=None):
        """`psf_all` PER RAY GROUP: one `MonitorPSFGroups` per monitor, in their order — one diffraction image per group of input
        rays from one trace and one pass over the segments (ot_monitor_psf_groups_many).  The fields of different groups are never
        added: a batch multiplexed in wavelength gives the image of every wavelength, whose INTENSITIES an instrument adds
        (`MonitorPSFGroups.intensity()`, `.strehl()`, `.mtf()`: the polychromatic PSF, Strehl ratio and MTF), one of several field
        points the image of every field point.  groups, n_groups and labels as for `spots_grouped_all`: one integer id per INPUT
        ray (`RayBatch.groups_by_wavelength()` gives one group per wavelength), G = 1 .. 256 (None: max id + 1), and rays whose id
        is outside 0 .. G - 1 are in no group — their hits are in no image and are counted in `MonitorPSFGroups.ungrouped`.  A hit
        belongs to the group of the ray its segment descends from, whatever the layout and wherever in a ray tree.  Every other
        argument, the model, the aliasing warning and the requirement of double precision are `psf_all`'s; monitors x G may not
        exceed 4096, monitors x G x samples not 2^27.  Group g of the result is bit for bit `psf_all` of that group's rays traced
        alone in the same order, the same bits every run.  `into`: the list an earlier call with the same monitors, reference,
        grid, amplitude and G returned; this call's hits are added to it, with this call's `groups` (the chunks of a streamed trace
        each bring their own table)."""
        import warnings
        from .psf import MonitorPSFGroups, psf_amplitude, psf_grid
        from .spots import spot_group_ids
        from .wavefront import wavefront_reference

        monitors = list(self.monitors if monitors is None else monitors)
        M = len(monitors)
        kind, lab, local = wavefront_reference(focus, direction, monitors)
        grid, pixels, step, centres = psf_grid(step, pixels, centre, M)
        mode = psf_amplitude(amplitude)
        ids, G = spot_group_ids(groups, segs.n_rays, n_groups, device=segs.device)
        if labels is not None and len(labels) != G:
            raise ValueError(f"labels: one per group ({G}), not {len(labels)}")
        if segs.precision != "f64":
            raise ValueError("psf_grouped_all needs a double-precision SegmentBatch: a path length in single precision is a hundredth of a wave wrong at table scale")
        wavelength = _wavelengths_of(wavelength, segs, "a PSF")
        name = ("focus", "direction")[kind]
        stack = None
        if into is not None:
            into, stack = _into_stack(into, M, lambda k, p: isinstance(p, MonitorPSFGroups) and p.monitor is monitors[k] and p.amplitude == amplitude
                                      and p.reference == (name, tuple(lab[k])) and p.step == step and p.centre == tuple(centres[k])
                                      and tuple(p.re.shape) == (G,) + pixels,
                                      "into: the list an earlier psf_grouped_all returned for the same monitors, reference, grid, amplitude and n_groups")
            if not monitors:
                return into
        before = 0 if stack is None else int(stack[0][:, :, 2].sum().item())
        counts, norm, re, im, ungrouped = _engine().monitor_psf_groups_many([monitor_struct(m) for m in monitors], _monitor_axes(monitors), kind, local, grid,
                                                                            pixels, ids, G, segs, wavelength, amplitude_mode=mode, into=stack)
        if into is None:
            into = [MonitorPSFGroups(m, counts[k], norm[k], re[k], im[k], ungrouped[k], (name, lab[k]), grid[k], step, centres[k], amplitude, labels=labels,
                                     stack=(counts, norm, re, im, ungrouped, k)) for k, m in enumerate(monitors)]
        aliased = (int(counts[:, :, 2].sum().item()) if M else 0) - before
        if aliased > 0:
            warnings.warn(f"psf_grouped_all: {aliased} hits are aliased — their phase turns more than half a cycle from one sample to the next, and the "
                          "sampled image means nothing for them: use a smaller step", RuntimeWarning, stacklevel=2)
        return into

    def psf_grouped_batch(self, monitor, segs, wavelength, groups, n_groups=None, focus=None, direction=None, step=None, pixels=65, centre=(0.0, 0.0),
                          amplitude="sqrt", labels=None):
        """One monitor as diffraction images per ray group (`psf_grouped_all` for it alone): a `MonitorPSFGroups`."""
        return self.psf_grouped_all(segs, wavelength, groups, n_groups=n_groups, focus=focus, direction=direction, step=step, pixels=pixels, centre=centre,
                                    monitors=[monitor], amplitude=amplitude, labels=labels)[0]

    def field_all(self, segs, wavelength=0.0, bins=30, monitors=None, into=None, amplitude="sqrt"):
        """Every monitor of the table (or those given) as a COHERENT image: one `MonitorField` per monitor, in their order — per
        bin of `image_all`'s images the count of hits and the complex sum of a exp(i phi) over them, summed on the device in the
        pass that finds the hits, with no hit list (ot_monitor_field_many).  phi is `Ray.phase(t)` at the monitor,
        2 pi frac((pathlength + t n) / wavelength), and a = sqrt(intensity) (amplitude="sqrt": intensity is a power) or the
        intensity as it stands (amplitude="linear": scenes built on amplitude-style splitting ratios).  It is the model's phase and
        nothing more: no pi on reflection, no Gaussian envelope.  `MonitorField.intensity()` is what an optical table shows.
        `wavelength`: one float for all rays, or the `RayBatch` that was traced (its wavelengths by the segments' `ray`; children
        of a ray tree inherit theirs).  `segs` must be double precision: single-precision path lengths carry some 0.02 cycle of
        phase noise at table scale.  `into`: as for `image_all`."""
        from .monitors import MonitorField, image_bins

        bins = image_bins(bins)
        if amplitude not in ("sqrt", "linear"):
            raise ValueError(f"amplitude must be 'sqrt' or 'linear', not {amplitude!r}")
        if segs.precision != "f64":
            raise ValueError("field_all needs a double-precision SegmentBatch: a field from single-precision path lengths is refused, not approximated")
        wavelength = _wavelengths_of(wavelength, segs, "a field")
        return self._images_all(MonitorField, "field", segs, bins, monitors, into, wavelength, amplitude_mode=("sqrt", "linear").index(amplitude),
                                left_out="their `ray` is no index into the wavelengths given, or its wavelength is not finite and > 0")[0]

    def field_batch(self, monitor, segs, wavelength=0.0, bins=30, amplitude="sqrt"):
        """One monitor as a coherent image (`field_all` for it alone): a `MonitorField`."""
        return self.field_all(segs, wavelength, bins=bins, monitors=[monitor], amplitude=amplitude)[0]

    def beam_all(self, segs, wavelength=0.0, bins=30, monitors=None, into=None):
        """Every monitor of the table (or those given) as the image its GAUSSIAN BEAMS make: one `MonitorBeam` per monitor, in
        their order — per bin of `image_all`'s images the count of hit centres and the power the bin receives when every hit is
        spread over its spot, I 2 / (pi w^2) exp(-2 r^2 / w^2) integrated over the bin, w = `Ray.spot_size(t)` at the monitor from
        the segment's q, n and the wavelength; summed on the device in the pass that finds the hits, with no hit list
        (ot_monitor_beam_many).  It is `Monitor.render_scatter(gaussian_beam=True)`'s circle made quantitative: the beam is taken
        at normal incidence in the monitor's (y, z), so a tilted beam's spot is not stretched, and a spot that reaches over the
        monitor's rim loses that part (the sum of `power` is at most the hits' intensity).  A hit whose centre lies outside the
        edges is counted nowhere and still deposits its tails.  `wavelength`: one float for all rays, or the `RayBatch` that was
        traced, as for `field_all`.  `segs` in either precision (all arithmetic is double).  A hit without q (a batch traced
        without a Gaussian beam) or with an unusable index raises ValueError.  `into`: as for `image_all`."""
        from .monitors import MonitorBeam, image_bins

        bins = image_bins(bins)
        wavelength = _wavelengths_of(wavelength, segs, "a beam image")
        return self._images_all(MonitorBeam, "beam", segs, bins, monitors, into, wavelength, left_out=_NO_BEAM)[0]

    def beam_batch(self, monitor, segs, wavelength=0.0, bins=30):
        """One monitor as a Gaussian-beam image (`beam_all` for it alone): a `MonitorBeam`."""
        return self.beam_all(segs, wavelength, bins=bins, monitors=[monitor])[0]

    def wave_all(self, segs, wavelength=0.0, bins=30, monitors=None, into=None, amplitude="sqrt", gouy=False):
        """Every monitor of the table (or those given) as the COHERENT image its GAUSSIAN BEAMS make: one `MonitorWave` per monitor,
        in their order — per bin of `image_all`'s images the count of hit centres and the complex sum over the hits of the beam's
        field SAMPLED AT THE BIN CENTRE (yc, zc),
            u = a sqrt(2 / (pi w^2)) exp(-(Dy^2 + Dz^2) / w^2) exp(i (2 pi frac(cycles) - g)),     Dy = yc - y0, Dz = zc - z0,
            cycles = (pathlength + t n) / wavelength + n (ty Dy + tz Dz) / wavelength + n Re(q) (Dy^2 + Dz^2) / (2 wavelength |q|^2):
        `Ray.phase(t)` as in `field_all`, the beam's tilt (`MonitorHits.tYList` / `tZList`) and its wavefront curvature
        (`radiusList`), under the envelope of `beam_all`'s spot w (`spotsizeList`); summed on the device in the pass that finds the
        hits, with no hit list (ot_monitor_wave_many).  a = sqrt(intensity) (amplitude="sqrt") or the intensity as it stands
        ("linear"), as in `field_all`.  Two traced rays give an interferometer's fringes; `MonitorWave.irradiance()` is what a
        camera shows.  gouy=True subtracts g = atan2(Re q, Im q) from every hit's phase (`gouyList`); the tracer's q does not
        accumulate the Gouy phase across lenses, so g is exact only for a beam that has met no focusing element since its waist
        (default False: g = 0).  Limits: the envelope is taken at normal incidence (a tilted spot is not stretched), q is not advanced
        across the tilt, bin centres more than 6 w from the hit's along an axis are left out (below exp(-36) of the peak), no pi
        on reflection.  A field sampled at bin centres means nothing where the phase turns more than half a cycle from one bin to
        the next: hits for which it does somewhere on their footprint are deposited all the same, counted in `MonitorWave.aliased`
        and announced by one RuntimeWarning.  `wavelength`, `into` and the double-precision `segs` as for `field_all` (a field is
        linear: chunks add).  A hit without q or with an unusable index raises ValueError, as in `beam_all`."""
        import warnings
        from .monitors import MonitorWave, image_bins

        bins = image_bins(bins)
        if amplitude not in ("sqrt", "linear"):
            raise ValueError(f"amplitude must be 'sqrt' or 'linear', not {amplitude!r}")
        if not isinstance(gouy, (bool, np.bool_)):
            raise ValueError(f"gouy must be True or False, not {gouy!r}")
        if segs.precision != "f64":
            raise ValueError("wave_all needs a double-precision SegmentBatch: a field from single-precision path lengths is refused, not approximated")
        wavelength = _wavelengths_of(wavelength, segs, "a beam field")
        waves, outs = self._images_all(MonitorWave, "wave", segs, bins, monitors, into, wavelength, amplitude_mode=("sqrt", "linear").index(amplitude),
                                       gouy=int(gouy), left_out=_NO_BEAM)
        if outs is None:
            return waves
        # the call's aliased counter runs on through every call that adds `into` it: what the images knew before is the earlier calls'
        before, total = (waves[0].aliased if waves else 0), int(outs[4].item())
        if total > before:
            warnings.warn(f"wave_all: {total - before} hits are aliased — somewhere on their footprint the phase of their beam turns more than half "
                          "a cycle from one bin centre to the next, and the sampled field means nothing there: use a smaller monitor or more bins",
                          RuntimeWarning, stacklevel=2)
        for f in waves:
            f.aliased = total
        return waves

    def wave_batch(self, monitor, segs, wavelength=0.0, bins=30, amplitude="sqrt", gouy=False):
        """One monitor as a coherent Gaussian-beam image (`wave_all` for it alone): a `MonitorWave`."""
        return self.wave_all(segs, wavelength, bins=bins, monitors=[monitor], amplitude=amplitude, gouy=gouy)[0]

    # -- ABCD extraction (optical_table.py:211-297), a caller of the hot path ----------------------
    def calculate_abcd_matrix(self, mon0, mon1, rays, disp=1e-5, rot=1e-5, debugaxs=None):
        """Per-ray 2x2 ABCD matrix between two monitors by finite differences: three traces
        (nominal, displaced along mon0's Y tangent, rotated about mon0's Z tangent at the nominal
        hit point).  Each trace is one device batch.  The reference's in-place biasing is kept:
        the angular probe is applied to the already displaced rays (optical_table.py:272-284)."""
        y_axis, z_axis = mon0.tangent_Y, mon0.tangent_Z

        def simulate(batch):
            self.rays = []
            mon0.clear()
            mon1.clear()
            self.ray_tracing(batch)

        assert len(rays) > 0, "No rays to trace in ABCD calculation."
        ids = [r._id for r in rays]
        assert len(set(ids)) == len(rays), "Redundant ray ids in ABCD calculation."
        probe = [copy.deepcopy(rays[i]) for i in np.argsort(ids)]
        simulate(probe)
        for mon, label in ((mon0, "mon0"), (mon1, "mon1")):
            assert set(ids) == {r._id for r in mon.get_rays(sort="ID")}, f"Rays at {label} do not match the input rays."
        pivots = mon0.get_PList(sort="ID")
        y0, ty0 = mon1.get_yList(sort="ID"), mon1.get_tYList(sort="ID")
        simulate([r._Translate(y_axis * disp) for r in probe])
        y1, ty1 = mon1.get_yList(sort="ID"), mon1.get_tYList(sort="ID")
        simulate([r._RotAround(z_axis, pivots[k], rot) for k, r in enumerate(probe)])
        y2, ty2 = mon1.get_yList(sort="ID"), mon1.get_tYList(sort="ID")
        Ms = np.zeros((len(rays), 2, 2))
        Ms[:, 0, 0], Ms[:, 1, 0] = (y1 - y0) / disp, (ty1 - ty0) / disp
        Ms[:, 0, 1], Ms[:, 1, 1] = (y2 - y0) / rot, (ty2 - ty0) / rot
        return Ms

    def abcd_batch(self, mon0, mon1, batch, disp=1e-5, rot=1e-5, max_segments=64):
        """`calculate_abcd_matrix` for a RayBatch, entirely on the device: three traces, monitor
        passes and the finite differences are tensor operations; returns a [N, 2, 2] tensor (ray i of
        the batch = row i).  Same biasing sequence as the object version (the angular probe acts on
        the already displaced rays and pivots about mon0's LOCAL hit point used as a lab point,
        optical_table.py:259-284).  Every ray must cross each monitor exactly once."""
        import torch
        from .geometry import rotation_matrix

        scene = self.compile()  # the components do not move between the three traces

        def probe(b):
            segs = self.trace_batch(b, max_segments=max_segments, scene=scene)
            h0, h1 = self.record_batch(mon0, segs), self.record_batch(mon1, segs)
            for h, label in ((h0, "mon0"), (h1, "mon1")):
                if len(h) != b.n or not torch.equal(h.ray_index("ID"), torch.arange(b.n, device=b.device)):
                    raise AssertionError(f"Rays at {label} do not match the input rays.")
            return h0, h1

        work = batch.clone()
        h0, h1 = probe(work)
        pivots = h0.PList("ID")
        y0, ty0 = h1.yList("ID"), h1.tYList("ID")
        work.translate_(np.asarray(mon0.tangent_Y, dtype=float) * disp)
        _, h1 = probe(work)
        y1, ty1 = h1.yList("ID"), h1.tYList("ID")
        work.rotate_around_(rotation_matrix(mon0.tangent_Z, rot), pivots)
        _, h1 = probe(work)
        y2, ty2 = h1.yList("ID"), h1.tYList("ID")
        Ms = torch.empty((batch.n, 2, 2), dtype=y0.dtype, device=batch.device)
        Ms[:, 0, 0], Ms[:, 1, 0] = (y1 - y0) / disp, (ty1 - ty0) / disp
        Ms[:, 0, 1], Ms[:, 1, 1] = (y2 - y0) / rot, (ty2 - ty0) / rot
        return Ms

    @staticmethod
    def calibrate_symmetric_4f(lens, rays, F10, F20, criterion="M=-I", debugaxs=None, optimize=True, display_M=False):
        """Tune the distances of mon0 - F1 - lens - 2 F2 - lens(turned) - F1 - mon1 with Nelder-Mead
        (optical_table.py:299-422).  A caller of the hot path: every cost evaluation is one
        `ray_tracing` + one `calculate_abcd_matrix` (4 device traces)."""
        def simulate(F1, F2):
            first = lens.copy()._Translate(np.array([F1, 0, 0]) - lens.origin)
            second = lens.copy()._Translate(np.array([F1 + 2 * F2, 0, 0]) - lens.origin).RotZ(np.pi)
            mon0 = Monitor(origin=[0, 0, 0], width=5, height=5)
            mon1 = Monitor(origin=[2 * F1 + 2 * F2, 0, 0], width=5, height=5)
            table = OpticalTable()
            table.add_components([first, second])
            table.add_monitors([mon0, mon1])
            table.ray_tracing(rays)
            y, ty = mon1.get_yList(), mon1.get_tYList()
            Ms = table.calculate_abcd_matrix(mon0, mon1, rays)
            if display_M:
                for M in Ms:
                    print(M)
            return Ms, y, ty

        costs = {
            "M=-I": lambda Ms, ty: np.mean([np.linalg.norm(M + np.eye(2)) for M in Ms]),
            "flat_field": lambda Ms, ty: np.mean([abs((1.5 * M[0, 0] - M[0, 1]) / (M[1, 1] - M[1, 0] * 1.5) - 1.5) for M in Ms]),
            "min_stdtY": lambda Ms, ty: float(np.std(ty)),
        }
        if criterion not in costs:
            raise ValueError(f"Unknown criterion: {criterion}")
        if not optimize:
            return simulate(F10, F20)
        from scipy.optimize import minimize

        def cost(x):
            Ms, _, ty = simulate(x[0], x[1])
            return costs[criterion](Ms, ty)

        res = minimize(cost, x0=[F10, F20], method="Nelder-Mead", options={"disp": True, "xatol": 1e-5, "maxiter": 50})
        return res.x[0], res.x[1]

    # -- exports (optical_table.py:447-500), written from columns (export.py) ---------------------------
    def gather_rays_csv(self):
        from . import export

        cols, has_q = export.columns_of_rays(self.rays)
        return [dict(zip(export.HEADER, row)) for row in export.rays_csv_rows(cols, has_q)]

    def export_rays_csv(self, filename: str):
        from . import export

        cols, has_q = export.columns_of_rays(self.rays)
        export.write_rays_csv(filename, cols, has_q)

    def export_batch_csv(self, segs, filename: str, rays=None):
        """`export_rays_csv` for a SegmentBatch, straight from its columns: no Ray objects.  `rays`: the traced
        RayBatch (tells which rays carry a Gaussian q, ray.py:98-104); without it every segment prints its q."""
        segs.export_rays_csv(filename, rays)

    def materialize(self, segs, sources, select=None):
        """SegmentBatch -> List[Ray] for the input rays in `select` only (all when None), in the
        reference's order; `sources` are the input Ray objects (ids, wavelengths, custom attributes
        are inherited from them as upstream copies do).  Lets plotting code consume a device trace
        without building millions of objects."""
        host = segs.to_host(reference_order=True)
        keep = np.ones(len(host["ray"]), dtype=bool) if select is None else np.isin(host["ray"], np.asarray(list(select)))
        host = {k: (v[keep] if k != "count" else v) for k, v in host.items()}
        per_ray = [None] * len(sources)
        _scatter_segments(host, sources, np.arange(len(sources)), per_ray)
        return [seg for chunk in per_ray if chunk for seg in chunk]

    # -- List[Ray] plumbing ------------------------------------------------------------------------
    def _trace_objects(self, rays, cap, max_time=MAX_TRACE_TIME):
        with _engine().lock:  # upload + every trace of this call as one unit (see Engine.lock)
            return OpticalTable._trace_objects_locked(self, rays, cap, max_time)  # (`self` may be the reference package's table: adapter.install)

    def _trace_objects_locked(self, rays, cap, max_time=MAX_TRACE_TIME):
        import torch

        eng = _engine()
        scene = self.compile()
        eng.upload(scene)
        n = len(rays)
        ids = [r._id for r in rays]
        class_of = {}
        cls = np.array([class_of.setdefault(i, len(class_of)) for i in ids], dtype=np.int32)
        n_classes = len(class_of)
        # rays sharing an _id share interact counters and must see each other's updates in
        # input order (optical_component.py:140-149): trace them in successive rounds.
        rounds = np.zeros(n, dtype=np.int64)
        if scene.limited and n_classes < n:
            seen = {}
            for k, c in enumerate(cls):
                rounds[k] = seen.get(c, 0)
                seen[c] = rounds[k] + 1
        counts = None
        if scene.limited:
            host = np.zeros((len(scene.limited), n_classes), dtype=np.int32)
            for s, comp in enumerate(scene.limited):
                for rid, c in class_of.items():
                    host[s, c] = comp._interact_count.get(rid, 0)
            counts = torch.from_numpy(host).to(eng.device)
        per_ray = [None] * n
        total_capped = 0
        for rnd in range(int(rounds.max()) + 1):
            pick = np.nonzero(rounds == rnd)[0]
            sub = [rays[k] for k in pick]
            if scene.hooks:  # leaves whose interact_local is the user's Python: generation by generation, device search + host physics
                chunks, capped = OpticalTable._trace_hooked(self, eng, scene, sub, cls[pick], cap, counts, max_time)
                total_capped += capped
                for k, chunk in zip(pick, chunks):
                    per_ray[k] = chunk
                continue
            batch = _pack(sub, cls[pick], eng.device, scene.unit)
            if scene.max_children <= 1 and cap <= _FUSED_MAX_SEGMENTS:
                segs = eng.trace(batch, cap, counts=counts)
                host_segs = segs.to_host(reference_order=True)
                capped = _fused_capped(host_segs, cap)
            else:
                segs = eng.trace_branching(batch, cap, counts=counts, max_trace_time=max_time, distinct_ids=True)  # (a round holds every id once)
                host_segs = segs.to_host(reference_order=True)
                capped = int(segs.capped.sum().item())
                if capped:  # traces done by the largest truncated tree (what the cap message reports)
                    per_tree = np.bincount(host_segs["ray"], minlength=len(sub))
                    self._last_trace_num = int(per_tree[segs.capped.cpu().numpy()].max())
            total_capped += capped
            check_implicit_hits(scene, host_segs)
            _scatter_segments(host_segs, sub, pick, per_ray)
        if scene.limited:
            host = counts.cpu().numpy()
            for s, comp in enumerate(scene.limited):
                for rid, c in class_of.items():
                    if host[s, c] or rid in comp._interact_count:
                        comp._interact_count[rid] = int(host[s, c])
        traced = [seg for chunk in per_ray for seg in chunk]
        for mon in self.monitors:
            record_monitor_hits(mon, traced)
        return traced, total_capped


    def _trace_hooked(self, eng, scene, sources, cls, cap, counts, max_time):
        """Ray trees through a scene with USER-DEFINED components (subclasses that override `interact_local`,
        optical_component.py:235-240).  The trees advance generation by generation: the device finds every queued ray's
        nearest hit among ALL leaves (boxes, grids, count gates, the strict first minimum: `Engine.generation_step`, the
        kernels of every other trace) and emits the children of the built-in leaves; for a ray whose winner is a hooked leaf
        the user's method gets the ray in the leaf's frame and its return is taken to the lab frame — the statements of
        optical_component.py:354-372.  Within a tree, generation order is the reference's FIFO order (optical_table.py:
        115-134): a hit contributes [truncated ray, its dead children ...] to the output and its live children to the queue;
        the cap counts pops per tree and drops what is still queued (:93-98, :138-144).  Deviation, by design: the reference
        calls `interact_local` on every component a ray geometrically hits and discards all results but the nearest's (:119-
        123); here only the nearest hit's is called, which is the same for a method without side effects.
        Returns (per-tree lists of finished rays, number of trees the cap or the clock cut)."""
        import time

        t0 = time.time()
        n = len(sources)
        done = [[] for _ in range(n)]
        pops, cut = [0] * n, [False] * n
        queue = [(r, t) for t, r in enumerate(sources)]
        while queue:
            if time.time() - t0 >= max_time:
                for _, t in queue:
                    cut[t] = True
                break
            live = []
            for r, t in queue:
                if pops[t] < cap:
                    pops[t] += 1
                    live.append((r, t))
            if not live:
                break
            m = len(live)
            eng.upload(scene)  # (a hook may have used the engine for a scene of its own: intersect_point_local)
            batch = _pack([r for r, _ in live], np.asarray(cls)[[t for _, t in live]], eng.device, scene.unit)
            segs, kids, parent = eng.generation_step(batch, counts, tree=[t for _, t in live])  # (a tree's rays meet a count gate in FIFO order)
            surface = segs.surface[:m].cpu().numpy()
            length = segs.length[:m].cpu().numpy()
            kid = {f: kids.field(f).cpu().numpy() for f in abi.RAY_FIELDS} if kids.n else None
            first = np.searchsorted(parent.cpu().numpy(), np.arange(m + 1))  # children come in parent order
            queue = []
            for i, (r, t) in enumerate(live):
                if surface[i] < 0:  # escaped, or dead on input: archived as it is (optical_table.py:133-134)
                    done[t].append(_clone_rays([r])[0])
                    continue
                stub = _clone_rays([r])[0]
                stub.length, stub.alive = float(length[i]), False
                done[t].append(stub)
                comp = scene.hooks.get(int(surface[i]))
                if comp is None:
                    children = [_child_ray(r, kid, j) for j in range(first[i], first[i + 1])]
                else:  # (the children the device emitted for a hooked leaf are its class's built-in physics: the hook may ask for them)
                    children = _call_hook(comp, r, length[i], (lambda r=r, a=first[i], b=first[i + 1]: [_child_ray(r, kid, j) for j in range(a, b)]))
                for c in children:
                    if c.alive:
                        queue.append((c, t))
                    else:
                        done[t].append(c)
        capped = [cut[t] or pops[t] >= cap for t in range(n)]
        if any(capped):
            self._last_trace_num = max(pops[t] for t in range(n) if capped[t])
        return done, int(sum(capped))


# What the device already knows about the ray a hook is being called for: id(local ray) -> (component, local origin, local
# direction, t, built-in children in the lab frame or None).  A hook that starts with `P, t = self.intersect_point_local(ray)`
# (every interact_local upstream does: optical_component.py:543, 624, 936) or calls `super().interact_local(ray)` asks for
# exactly that hit again; answering from here saves a one-ray launch per question (0.6 ms each: 126 -> 50 ms per call on the
# scene of fixture g25).  Only for the very ray object handed to the hook, and only while it still has the origin and direction
# it was handed over with; any other question goes to the device.
_HOOK_MEMO = {}


# (what leaves a hit out of beam_all and wave_all)
_NO_BEAM = ("they carry no q (a batch traced without a Gaussian beam), or their wavelength or refractive index is not finite and > 0, or their "
            "`ray` is no index into the wavelengths given")


def _monitor_axes(monitors):
    """The [M, 6] table of the monitors' lab tangents (a_y, a_z) that every monitor_*_many call takes."""
    return np.array([np.concatenate([m.tangent_Y, m.tangent_Z]) for m in monitors], dtype=float).reshape(len(monitors), 6)


def _into_stack(into, n, same, error):
    """`into=` of a *_all call over `n` monitors: (it as a list, the engine's tensors it adds to — None for no monitors).  It must be
    the list an earlier call returned for the same arguments (`same(k, item)` of every item; ValueError `error`), whole, in its order."""
    into = list(into)
    if len(into) != n or not all(same(k, item) for k, item in enumerate(into)):
        raise ValueError(error)
    if any(item._stack is None or item._stack[0] is not into[0]._stack[0] or item._stack[-1] != k or len(item._stack[0]) != n for k, item in enumerate(into)):
        raise ValueError("into: the whole list of one earlier call, in its order")
    return into, into[0]._stack[:-1] if into else None


def _wavelengths_of(wavelength, segs, what):
    """The `wavelength` argument of `field_all` / `beam_all` / `wave_all` as the engine takes it: a float > 0, or the double wavelengths of the
    `RayBatch` that was traced (one per input ray of `segs`); anything else is a ValueError that names `what` needs it."""
    import torch
    from .batch import RayBatch

    if isinstance(wavelength, RayBatch):
        if segs.n_rays is not None and wavelength.n != int(segs.n_rays):
            raise ValueError(f"wavelength: a RayBatch of {wavelength.n} rays for segments of {int(segs.n_rays)}")
        wavelength = wavelength.wavelength.double().contiguous()
        if not bool(((wavelength > 0) & torch.isfinite(wavelength)).all()):
            raise ValueError("wavelength: every ray of the batch needs a finite wavelength > 0")
        return wavelength
    try:
        value = float(wavelength)
    except (TypeError, ValueError):
        raise ValueError(f"wavelength must be a float or the RayBatch that was traced, not {wavelength!r}") from None
    if not (np.isfinite(value) and value > 0):
        raise ValueError(f"wavelength={wavelength!r}: {what} needs a finite wavelength > 0 (pass it, or the RayBatch that was traced)")
    return value


def _memo_for(comp, ray_local):
    memo = _HOOK_MEMO.get(id(ray_local))
    if memo is None or memo[0] is not comp:
        return None
    if not (np.array_equal(memo[1], ray_local.origin) and np.array_equal(memo[2], ray_local.direction)):
        return None
    return memo


def _call_hook(comp, ray, t=None, builtin_children=None):
    """The user's `interact_local` on a lab-frame ray the device found to hit `comp` first: local frame in, lab frame out
    (optical_component.py:354, 366-372).  `t`: the hit distance the device found; `builtin_children`: a callable giving the
    lab-frame rays the class's own physics emits for this hit (or None)."""
    local = comp.ray_to_local_coordinates(ray)
    if t is not None:
        _HOOK_MEMO[id(local)] = (comp, local.origin.copy(), local.direction.copy(), float(t), builtin_children)
    try:
        out = comp.interact_local(local)
    finally:
        _HOOK_MEMO.pop(id(local), None)
    if out is None:
        return []
    return [comp.ray_to_lab_coordinates(c) for c in out]


def _child_ray(parent, kid, j):
    """Ray object of child `j` of a generation step's output: the parent's clone (it keeps _id, wavelength, unit and user
    attributes, like the copy chain upstream) with the traced fields replaced."""
    from .materials import Material

    child = _clone_rays([parent])[0]
    d = child.__dict__
    d["origin"] = np.array([kid["ox"][j], kid["oy"][j], kid["oz"][j]])
    d["_direction"] = np.array([kid["dx"][j], kid["dy"][j], kid["dz"][j]])
    d["intensity"] = float(kid["intensity"][j])
    d["length"], d["alive"] = None, True
    if parent.qo is not None:
        d["qo"] = complex(kid["q_re"][j], kid["q_im"][j])
    d["_n"] = Material("Constant", n=float(kid["n"][j]))
    d["_pathlength"] = float(kid["pathlength"][j])
    return child


def _clone_rays(rays):
    """What `copy.deepcopy(self.rays)` (optical_table.py:72) yields for ordinary rays, without
    walking every object graph: the arrays are copied, scalars and the (immutable) material are
    shared.  ~20x cheaper than deepcopy, which is the reference's own bottleneck here."""
    out = []
    new = object.__new__
    for r in rays:
        c = new(type(r))
        d = c.__dict__
        d.update(r.__dict__)
        d["origin"] = r.origin.copy()
        d["_direction"] = r._direction.copy()
        out.append(c)
    return out


def _pack(rays, cls, device, scene_unit=1e-2):
    """List[Ray] -> RayBatch (fp64).  The reference evaluates materials at `ray.wavelength * ray.unit`
    — the RAY's unit (optical_component.py:627-628, base.py:31) — while the kernel multiplies by the
    scene's; the wavelength column is rescaled so that both give the same metres for every ray."""
    from .batch import RayBatch

    n = len(rays)
    origin = np.array([r.origin for r in rays], dtype=float).reshape(n, 3)
    direction = np.array([r.direction for r in rays], dtype=float).reshape(n, 3)
    has_q = np.array([r.qo is not None for r in rays])
    q = np.array([complex(r.qo) if r.qo is not None else 0j for r in rays], dtype=np.complex128)
    b = RayBatch.from_arrays(origin, direction,
                             wavelength=[r.wavelength * (getattr(r, "unit", scene_unit) / scene_unit) for r in rays],
                             intensity=[r.intensity for r in rays],
                             q=q, n_index=[r.n for r in rays], pathlength=[r._pathlength for r in rays],
                             ids=cls, device=device, normalize=False)
    import torch

    flags = np.where(has_q, abi.RAY_HAS_Q, 0) | np.where([bool(r.alive) for r in rays], 0, abi.RAY_DEAD)
    b.flags.copy_(torch.from_numpy(flags.astype(np.int32)))
    if any(r.length is not None for r in rays):
        lengths = np.array([np.inf if r.length is None else r.length for r in rays], dtype=float)
        b.length = torch.from_numpy(lengths).to(device)
    return b


def _fused_capped(host_segs, cap):
    """Trees for which the reference prints its cap message: the loop ran `cap` iterations that
    each processed a ray, so `exit_flag` was never set (optical_table.py:93-98, 138-143) — i.e.
    the tree filled all `cap` slots, whether or not a queued ray was actually dropped."""
    return int(np.sum(host_segs["count"] >= cap))


def check_implicit_hits(scene, segs):
    """Run-time check of the surfaces traced as 3-D series (scene.implicit): every segment that ends on one is taken into the
    leaf's frame and asked of the user's own methods — within_boundary must hold and |f| must be within what a hit point off
    by 1e-7 of the scene scale along grad f gives.  The aperture family was measured on a few thousand surface points at
    compile time (implicit.py); a feature smaller than that sampling resolves (a hole of ~1 % of the aperture) shows here."""
    from . import implicit
    from .scene import SceneError

    leaves = getattr(scene, "implicit", None)
    if not leaves:
        return
    surface = np.asarray(segs["surface"])
    for s in np.nonzero(np.isin(surface, list(leaves)))[0]:
        comp, rec = leaves[int(surface[s])]
        P = (np.array([segs["ox"][s], segs["oy"][s], segs["oz"][s]], dtype=float)
             + float(segs["length"][s]) * np.array([segs["dx"][s], segs["dy"][s], segs["dz"][s]], dtype=float))
        loc = np.asarray(comp.transform_matrix, dtype=float).T @ (P - np.asarray(comp.origin, dtype=float))
        surf = comp.surface
        inside, fv = bool(surf.within_boundary(loc)), float(surf.f(loc))
        tol = float(np.linalg.norm(implicit.record_gradient(rec, loc))) * 1e-7 * max(1.0, float(np.abs(loc).max())) + 4 * implicit.REL_TOL * rec[19]
        if not inside or not abs(fv) <= tol:
            what = "its within_boundary(P) is False" if not inside else f"its f(P) = {fv:.3e} (allowed {tol:.1e})"
            raise SceneError(f"{type(comp).__name__} with implicit surface {type(surf).__name__}: the device hit it at local "
                             f"P = {loc.tolist()}, but {what}: the aperture or surface measured at compile time does not hold "
                             "there (a feature finer than the measurement's sampling)")


def _scatter_segments(host_segs, sources, pick, per_ray):
    """Rebuild Ray objects, grouped by input ray, in the reference's order.  Every segment starts as a
    shallow clone of its input ray (it inherits _id, wavelength, unit and any user attribute, like the copy
    chain upstream) with the traced fields replaced.  Columns are converted to Python lists once and the
    clone is `__new__` + a dict update: ~2 us per segment instead of ~10 with copy.copy and per-field numpy
    scalars."""
    from .materials import Material

    tree = host_segs["ray"].tolist()
    surface = host_segs["surface"].tolist()
    length = host_segs["length"].tolist()
    intensity = host_segs["intensity"].tolist()
    q_re, q_im = host_segs["q_re"].tolist(), host_segs["q_im"].tolist()
    index, path = host_segs["n"].tolist(), host_segs["pathlength"].tolist()
    origin = np.stack([host_segs["ox"], host_segs["oy"], host_segs["oz"]], axis=1)
    direction = np.stack([host_segs["dx"], host_segs["dy"], host_segs["dz"]], axis=1)
    inf = float("inf")
    constants = {}  # one shared constant Material per distinct index value (Materials are immutable)
    for k in pick:
        per_ray[k] = []
    new = object.__new__
    for s, t in enumerate(tree):
        src = sources[t]
        seg = new(type(src))
        d = seg.__dict__
        d.update(src.__dict__)
        d["origin"] = origin[s].copy()
        d["_direction"] = direction[s].copy()
        d["intensity"] = intensity[s]
        d["length"] = None if length[s] == inf else length[s]
        d["alive"] = surface[s] == -1
        if d.get("qo") is not None:
            d["qo"] = complex(q_re[s], q_im[s])
        n = index[s]
        mat = constants.get(n)
        if mat is None:
            mat = constants[n] = Material("Constant", n=n)
        d["_n"] = mat  # what the RefractiveIndex descriptor would store for a float
        d["_pathlength"] = path[s]
        per_ray[pick[t]].append(seg)


def interact_component(comp, ray, call_hooks=True):
    """`component.interact(ray)` (optical_component.py:337-378; component_group.py:93-122 for groups) through
    the engine: one generation step over a scene made of this component alone.  Returns `(t, [truncated,
    *children])` or `(None, None)`; interact counters of the component (and of a group's children: every
    geometric hit consumes one) are read from and written back to the objects."""
    from .scene import compile_scene as _compile

    if not ray.alive:
        return None, None
    import torch

    eng = _engine()
    scene = _compile([comp])
    batch = _pack([ray], np.zeros(1, dtype=np.int32), eng.device, scene.unit)
    counts = None
    if scene.limited:
        host = np.array([[c._interact_count.get(ray._id, 0)] for c in scene.limited], dtype=np.int32)
        counts = torch.from_numpy(host).to(eng.device)
    with eng.lock:
        eng.upload(scene)
        segs, kids, _ = eng.generation_step(batch, counts)
    if scene.limited:
        after = counts.cpu().numpy()
        for s, c in enumerate(scene.limited):
            if after[s, 0] or ray._id in c._interact_count:
                c._interact_count[ray._id] = int(after[s, 0])
    if int(segs.surface[0].item()) < 0:
        return None, None
    t = float(segs.length[0].item())
    truncated = _clone_rays([ray])[0]
    truncated.length, truncated.alive = t, False
    out = [truncated]
    hook = scene.hooks.get(int(segs.surface[0].item())) if call_hooks else None
    if hook is not None:  # the leaf's physics is the user's Python (a group is asked for the leaf that was hit)
        return t, out + _call_hook(hook, ray, t)
    if kids.n:
        k = {f: kids.field(f).cpu().numpy() for f in abi.RAY_FIELDS}
        for j in range(kids.n):
            child = _clone_rays([ray])[0]
            child.origin = np.array([k["ox"][j], k["oy"][j], k["oz"][j]])
            child._direction = np.array([k["dx"][j], k["dy"][j], k["dz"][j]])
            child.intensity = float(k["intensity"][j])
            child.length, child.alive = None, True
            if ray.qo is not None:
                child.qo = complex(k["q_re"][j], k["q_im"][j])
            child._n = float(k["n"][j])
            child._pathlength = float(k["pathlength"][j])
            out.append(child)
    return t, out


def _pose_free_copy(comp):
    if hasattr(comp, "components"):
        raise NotImplementedError("local-frame calls are defined for leaf components")
    probe = copy.copy(comp)
    probe.origin, probe.transform_matrix = np.zeros(3), np.identity(3)
    probe._bbox, probe.max_interact_count, probe._interact_count = _NO_BOX, None, {}
    return probe


def interact_leaf_local(comp, ray_local):
    """`leaf.interact_local(ray_local)` (optical_component.py:536-570, 617-717, 930-948): the rays a hit emits,
    in the leaf's frame; an empty list when the local ray misses (upstream would fail on `P is None` there)."""
    memo = _memo_for(comp, ray_local)
    if memo is not None and memo[4] is not None:  # asked from inside a hook about the hit the device has just found
        return [comp.ray_to_local_coordinates(c) for c in memo[4]()]
    probe = _pose_free_copy(comp)
    probe._builtin_physics = True  # a user's override that calls super().interact_local() gets the class's own physics here
    _, rays = interact_component(probe, ray_local)
    return [] if rays is None else rays[1:]


def intersect_leaf_local(comp, ray_local):
    """`leaf.intersect_point_local(ray_local)` (optical_component.py:151-233): the ray is already in the
    leaf's frame, so the leaf is traced with an identity pose; count gates do not apply here."""
    memo = _memo_for(comp, ray_local)
    if memo is not None:  # asked from inside a hook about the hit the device has just found
        t = memo[3]
        return np.asarray(ray_local.origin, dtype=float) + t * np.asarray(ray_local.direction, dtype=float), t
    probe = _pose_free_copy(comp)
    t, rays = interact_component(probe, ray_local, call_hooks=False)  # (a user's interact_local asks for the hit point: no recursion)
    if t is None:
        return None, None
    return np.asarray(ray_local.origin, dtype=float) + t * np.asarray(ray_local.direction, dtype=float), t


def monitor_struct(monitor):
    """ot_monitor for a Monitor's current pose."""
    mon = abi.OtMonitor()
    mon.M[:] = np.asarray(monitor.transform_matrix, dtype=float).ravel().tolist()
    mon.origin[:] = np.asarray(monitor.origin, dtype=float).tolist()
    mon.half_width, mon.half_height = monitor.width / 2, monitor.height / 2
    return mon


def record_monitor_hits(monitor, rays):
    """Monitor.record (monitor.py:183-193) through `ot_monitor_record_f64`."""
    if not rays:
        monitor._updated = True
        return
    import torch
    from .batch import SegmentBatch

    eng = _engine()
    n = len(rays)
    segs = SegmentBatch(n, "f64", eng.device)
    cols = {
        "ox": [r.origin[0] for r in rays], "oy": [r.origin[1] for r in rays], "oz": [r.origin[2] for r in rays],
        "dx": [r.direction[0] for r in rays], "dy": [r.direction[1] for r in rays], "dz": [r.direction[2] for r in rays],
        "length": [np.inf if r.length is None else r.length for r in rays],
        "intensity": [r.intensity for r in rays],
    }
    for name, values in cols.items():
        segs.field(name).copy_(torch.tensor(values, dtype=torch.float64))
    segs.n_valid = n
    idx, P, t = eng.monitor_record(monitor_struct(monitor), segs)
    idx, P, t = idx.cpu().numpy(), P.cpu().numpy(), t.cpu().numpy()
    monitor._data_raw.extend([(P[k].copy(), rays[int(i)].intensity, float(t[k]), rays[int(i)]) for k, i in enumerate(idx)])
    monitor._updated = True
