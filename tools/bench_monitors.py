#!/usr/bin/env python3
"""Monitor.record on a through-focus stack of M monitors: `table.record_all` (one pass over the segments for all of them,
ot_monitor_record_many) against the same M `table.record_batch` calls (ot_monitor_record_f64 each) and against
`table.image_all` (the same hits binned on the device into 30 x 30 images, ot_monitor_image_many: no hit list), in one process,
the paths alternating round by round.  Device-resident: the history is traced once and stays where the trace left it.

Workloads: cfg 2 at 1e6 rays x 5 segments, fp64, in slots and in tiles; cfg 3 at 1e6 rays, cap 20, fp32, append layout.
M in 1, 2, 8, 32.  A time is that of the whole public call (the device passes, the read-back of the hit counts, the
MonitorHits built from them) between two events on the engine's stream, after a warm-up; reported: the median of the rounds
and their spread (min .. max).  Bytes are each path's own arithmetic from the shapes (`moved`), the rate is bytes over the
median of the whole call — an end-to-end figure, not a kernel's — as a fraction of the 8 TB/s HBM3E peak.

image_all's bytes: one pass of 7 reals per valid slot + validity, 8 bytes of intensity per hit, the images themselves (16 bytes
a bin, zeroed and added to); its row also names the plan of passes (optable_amd.engine.image_plan).

    python tools/bench_monitors.py [--rays 1000000] [--rounds 7] [--workloads cfg2-slots,cfg2-tiled,cfg3-append] [--stacks 1,2,8,32]
                                   [--out profiles/monitors_image.json]
    env: OT_LIB = another build of the library (an older one without image mode: the image_all column is left out)"""
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
from optable_amd.engine import image_plan, segment_source

if os.environ.get("OT_LIB"):  # an A/B build of the library, e.g. the parent commit's for record_all against itself
    abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
    import ctypes

    for newer in ("ot_monitor_image_many", "ot_monitor_field_many", "ot_monitor_beam_many", "ot_monitor_wave_many", "ot_fluence_map"):
        if not hasattr(ctypes.CDLL(abi.LIB_PATH), newer):
            del abi.SYMBOLS[newer]

HBM_PEAK = 8.0e12  # bytes per second (spec)
STACKS = (1, 2, 8, 32)
BINS = 30


def moved(segs, hits, n_monitors, passes):
    """Bytes each path moves for `n_monitors` monitors with `hits` hits in all, by its own arithmetic.  record_all: `passes`
    pairs of (count, emit) (2 when the first output was too small), each pass 7 reals per valid slot + the slot's validity (an
    int32 per slot in lists with holes; the counts of [k][ray] slots are n_rays words, left out), the emit pass also 40 bytes
    per hit it writes — an upper bound: emit leaves workgroups without hits unread.  record_batch, per monitor: the
    conversion copies (tiles -> slot arrays: 14 fields read and written; fp32 -> fp64: 12 reals read at 4, written at 8),
    the test (7 doubles per valid slot, a 4-byte flag per slot, 32 bytes per hit), the scan (the flags read twice, an
    8-byte offset written) and the compaction (flag + offset per slot, 32 bytes read and 40 written per hit).  Third: the bytes
    of ONE pass over the segments (what an image_all pass reads of them)."""
    _, slots, _, _ = segment_source(segs)
    valid = int(segs.count.abs().sum().item())
    w = 8 if segs.precision == "f64" else 4
    holes = 4 * slots if segs.layout == "append" else 0
    all_ = passes * 2 * (valid * 7 * w + holes) + passes * 40 * hits
    convert = (slots * 2 * (12 * w + 8) if segs.layout == "tiled" else 0) + (slots * 12 * (4 + 8) if w == 4 else 0)
    each = convert + valid * 7 * 8 + holes + slots * (4 + 2 * 4 + 8 + 4 + 8)
    return all_, n_monitors * each + hits * (32 + 32 + 40), valid * 7 * w + holes


def timed(fn, ev):
    ev[0].record()
    out = fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]), out


def run(label, table, segs, monitors, rounds, stacks=STACKS):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    rows = []
    for M in stacks:
        mons = monitors[:M]
        paths = {"record_all": lambda: table.record_all(segs, monitors=mons),
                 "record_batch": lambda: [table.record_batch(m, segs) for m in mons]}
        if "ot_monitor_image_many" in abi.SYMBOLS:
            paths["image_all"] = lambda: table.image_all(segs, bins=BINS, monitors=mons)
        for fn in paths.values():  # warm-up: code objects, the allocator's blocks
            fn()
            fn()
        times = {k: [] for k in paths}
        for rnd in range(rounds):
            for k in (sorted(paths) if rnd % 2 else sorted(paths, reverse=True)):
                ms, found = timed(paths[k], ev)
                times[k].append(ms)
                if k == "image_all":
                    binned = sum(int(im.counts.sum()) for im in found)  # (read back after the clock stopped)
                else:
                    hits = sum(len(h) for h in found)
                del found
        slots = segment_source(segs)[1]
        b_all, b_each, b_pass = moved(segs, hits, M, passes=2 if hits > slots else 1)
        row = {"workload": label, "monitors": M, "slots": slots, "hits": hits}
        for k, b in (("record_all", b_all), ("record_batch", b_each)):
            med = statistics.median(times[k])
            row[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "bytes": b,
                      "fraction_of_hbm_peak": round(b / (med * 1e-3) / HBM_PEAK, 4)}
        line = ""
        if "image_all" in paths:
            plan = image_plan(M, BINS, BINS)
            b = plan["passes"] * b_pass + 8 * hits + 3 * 16 * M * BINS * BINS
            med = statistics.median(times["image_all"])
            row["image_all"] = {"ms_median": round(med, 4), "ms_min": round(min(times["image_all"]), 4), "ms_max": round(max(times["image_all"]), 4),
                                "bytes": b, "fraction_of_hbm_peak": round(b / (med * 1e-3) / HBM_PEAK, 4), "bins": [BINS, BINS], "binned": binned,
                                "plan": plan}
            line = f"   image_all {med:8.3f} ms ({row['image_all']['ms_min']:.3f} .. {row['image_all']['ms_max']:.3f}, {plan['passes']} x {plan['path']})"
        rows.append(row)
        print(f"{label:28s} M={M:2d}  record_all {row['record_all']['ms_median']:8.3f} ms ({row['record_all']['ms_min']:.3f} .. {row['record_all']['ms_max']:.3f})"
              f"   {M} x record_batch {row['record_batch']['ms_median']:8.3f} ms ({row['record_batch']['ms_min']:.3f} .. {row['record_batch']['ms_max']:.3f})"
              f"{line}   {hits} hits", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--workloads", default="cfg2-slots,cfg2-tiled,cfg3-append")
    ap.add_argument("--stacks", default=",".join(str(m) for m in STACKS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitors_image.json"))
    args = ap.parse_args()
    workloads, stacks = args.workloads.split(","), tuple(int(m) for m in args.stacks.split(","))
    assert torch.cuda.is_available(), "bench_monitors.py measures on an MI355X"
    q = 1j * np.pi * W.W0**2 / W.WL
    rows = []

    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    stack = [oa.Monitor([6.0 + 3.0 * k / 32, 0, 0], 6, 6) for k in range(32)]  # between the lens (x = 5) and the mirrors (x = 10)
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=q, precision="f64")
    for layout in ("slots", "tiled"):
        if f"cfg2-{layout}" not in workloads:
            continue
        segs = table.trace_batch(batch, max_segments=5, layout=layout)
        rows += run(f"cfg2 fp64 {layout}", table, segs, stack, args.rounds, stacks)
        del segs
    del batch

    table = oa.OpticalTable()
    table.add_components(W.cfg3_components(oa))
    stack = [oa.Monitor([1.0 + 2.0 * k / 32, 0, 0], 12, 2) for k in range(32)]  # in front of the first column of components (x = 4)
    if "cfg3-append" in workloads:
        batch = RayBatch.from_arrays(*W.cfg3_rays(args.rays, 2), wavelength=W.WL, q=q, precision="f32")
        segs = table.trace_batch(batch, max_segments=20, layout="append")
        rows += run("cfg3 fp32 append", table, segs, stack, args.rounds, stacks)

    record = {"tool": "tools/bench_monitors.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0),
              "rays": args.rays, "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
