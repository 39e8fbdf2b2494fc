#!/usr/bin/env python3
"""Coherent against incoherent detector images: `table.field_all` (ot_monitor_field_many: per bin a count and the complex sum of
the hits' phasors) and `table.image_all` (ot_monitor_image_many: a count and the sum of their intensities) on the same segments
and monitors, in one process, alternating round by round; `table.record_all` beside them, for the record mode of the kernel all
three share.

Workload: cfg 2 at 1e6 rays x 5 segments, fp64, slots; M monitors of a through-focus stack (default 6), bins 30.  A time is that
of the whole public call between two events on the engine's stream, after a warm-up; reported: the median of the rounds and
their spread.  field_all reads its `skipped` counter back before it returns (8 bytes, one synchronisation); image_all returns
without reading anything.

    python tools/bench_field.py [--rays 1000000] [--rounds 21] [--monitors 6] [--out profiles/field_image.json]
    env: OT_LIB = another build of the library (an older one without the field mode: the field_all column is left out)"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import optable_amd as oa
from optable_amd import workloads as W
from optable_amd import abi
from optable_amd.batch import RayBatch
from optable_amd.engine import field_plan, image_plan

if os.environ.get("OT_LIB"):  # an A/B build of the library, e.g. the parent commit's for image_all and record_all against themselves
    abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
    import ctypes

    for newer in ("ot_monitor_field_many", "ot_monitor_beam_many", "ot_monitor_wave_many"):
        if not hasattr(ctypes.CDLL(abi.LIB_PATH), newer):
            del abi.SYMBOLS[newer]

BINS = 30


def timed(fn, ev):
    ev[0].record()
    out = fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--monitors", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_image.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_field.py measures on an MI355X"
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mons = [oa.Monitor([6.0 + 3.0 * k / 32, 0, 0], 6, 6) for k in range(args.monitors)]  # the stack of tools/bench_monitors.py
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = table.trace_batch(batch, max_segments=5, layout="slots")
    paths = {"image_all": lambda: table.image_all(segs, bins=BINS, monitors=mons),
             "record_all": lambda: table.record_all(segs, monitors=mons)}
    if "ot_monitor_field_many" in abi.SYMBOLS:
        paths["field_all"] = lambda: table.field_all(segs, W.WL, bins=BINS, monitors=mons)
        paths["field_all_per_ray"] = lambda: table.field_all(segs, batch, bins=BINS, monitors=mons)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for fn in paths.values():  # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    times = {k: [] for k in paths}
    for rnd in range(args.rounds):
        for k in (sorted(paths) if rnd % 2 else sorted(paths, reverse=True)):
            ms, found = timed(paths[k], ev)
            times[k].append(ms)
            del found
    binned = sum(int(im.counts.sum()) for im in paths["image_all"]())
    row = {"workload": "cfg2 fp64 slots", "monitors": args.monitors, "bins": [BINS, BINS], "binned": binned,
           "image_plan": image_plan(args.monitors, BINS, BINS), "field_plan": field_plan(args.monitors, BINS, BINS)}
    for k, t in times.items():
        row[k] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
        print(f"M={args.monitors} bins={BINS}  {k:18s} {row[k]['ms_median']:8.3f} ms ({row[k]['ms_min']:.3f} .. {row[k]['ms_max']:.3f})", flush=True)
    record = {"tool": "tools/bench_field.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "rounds": args.rounds, "rows": [row]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
