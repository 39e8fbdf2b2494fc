#!/usr/bin/env python3
"""Fluence maps (`table.fluence_map`, ot_fluence_map, k_seg_raster: one lane walks one segment through the pixel grid) at two image
sizes and in two segment layouts, with `table.image_all` on the same segments beside each for scale (one monitor of 30 x 30 bins:
one pass over the segments with one test and at most one deposit a slot).

Workload: cfg 2 at 1e6 rays x 5 segments, fp64, view "Z" over the table between the source and the mirrors;
  64 x 64     4,096 pixels: the workgroup's image in LDS
  512 x 512   262,144 pixels: every piece a global atomic
each in the `slots` layout (neighbouring lanes hold the same segment index of neighbouring rays: walks of like length) and in the
`append` layout (records in the order the waves wrote them).  A time is that of the whole public call between two events on the
engine's stream, after a warm-up; reported: the median of the rounds and their spread, the pieces deposited and the rate in
pieces per second.  All eight figures come from one run, one process, the paths alternating round by round.

    python tools/bench_fluence.py [--rays 1000000] [--rounds 11] [--out profiles/fluence.json]
    env: OT_LIB = another build of the library (the parent commit's, for an A/B in one job)"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ROI = (-1.03, 12.9, -3.01, 2.97, -2.83, 3.07)
SIZES = (64, 512)
LAYOUTS = ("slots", "append")


def timed(fn, ev):
    ev[0].record()
    out = fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fluence.json"))
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import fluence_plan

    if os.environ.get("OT_LIB"):  # an A/B build of the library, e.g. the parent commit's against this tree's
        abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
    assert torch.cuda.is_available(), "bench_fluence.py measures on an MI355X"
    assert args.rounds >= 5
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}
    paths = {}
    for layout in LAYOUTS:
        for size in SIZES:
            paths[f"fluence_map {size} x {size} {layout}"] = lambda s=segs[layout], p=size: table.fluence_map(s, view="Z", roi=ROI, pixels=p)
            # (one image_all beside every fluence figure: the same call twice a layout, measured twice)
            paths[f"image_all beside {size} x {size} {layout}"] = lambda s=segs[layout]: table.image_all(s, bins=30, monitors=[mon])
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
    rows = []
    for k, t in times.items():
        row = {"path": k, "ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
        if k.startswith("fluence_map"):
            fm = paths[k]()
            row["pieces"], row["skipped"] = int(fm.counts.sum()), fm.skipped
            row["plan"] = fluence_plan(*fm.pixels)
            row["pieces_per_s"] = round(row["pieces"] / (row["ms_median"] * 1e-3), 1)
        else:
            row["hits"] = int(paths[k]()[0].counts.sum())
        rows.append(row)
        extra = f"{row['pieces']} pieces, {row['pieces_per_s']:.3g} / s, {row['plan']['path']}" if "pieces" in row else f"{row['hits']} hits"
        print(f"{k:42s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})   {extra}", flush=True)
    record = {"tool": "tools/bench_fluence.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds, "view": "Z", "roi": list(ROI),
              "note": "one run: 2 sizes x 2 layouts, image_all (one monitor, 30 x 30 bins) beside each; one process, alternating rounds",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
