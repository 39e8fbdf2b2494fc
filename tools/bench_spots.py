#!/usr/bin/env python3
"""Spot statistics (`table.spots_all`, ot_monitor_spots_many, k_mon_spots: the moments of a monitor's hits on J planes displaced
along its normal, reduced on the device with no floating-point atomic) at four sizes and in two segment layouts, beside the two
ways to the same numbers the package had before:
  image_all of one monitor (30 x 30 bins)      the same loads and one test a slot: the floor for J = 1
  record_all over 32 displaced monitors,       what a through-focus scan took: 32 hit lists, then count, W, Wy, Wz, Wyy, Wzz, Wyz
  then the moments with torch                  of each on the device (`slots` only)

Workload: cfg 2 at 1e6 rays x 5 segments, fp64; one 6 x 6 monitor at x = 7.5 with J = 1, 32 and 256 planes over +-0.9, and eight
monitors between x = 6.6 and 8.4 with J = 32.  A time is that of the whole public call between two events on the engine's stream,
after a warm-up; reported: the median of the rounds and their spread.  All figures come from one run, one process, the paths
alternating round by round.

    python tools/bench_spots.py [--rays 1000000] [--rounds 11] [--out profiles/spots.json]"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spots.json"))
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import spots_plan

    assert torch.cuda.is_available(), "bench_spots.py measures on an MI355X"
    assert args.rounds >= 9
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    eight = [oa.Monitor([x, 0, 0], 6, 6) for x in np.linspace(6.6, 8.4, 8)]
    scan = {J: (np.linspace(-0.9, 0.9, J) if J > 1 else np.zeros(1)) for J in (1, 32, 256)}
    displaced = [oa.Monitor([7.5 + off, 0, 0], 6, 6) for off in scan[32]]
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}

    def by_hit_lists(s):
        out = []
        for h in table.record_all(s, monitors=displaced):
            y, z, w = h.yList(None), h.zList(None), h.IList(None)
            out.append(torch.stack([w.sum(), (w * y).sum(), (w * z).sum(), (w * y * y).sum(), (w * z * z).sum(), (w * y * z).sum()]))
        return torch.stack(out)

    paths = {}
    for layout in LAYOUTS:
        s = segs[layout]
        for J in scan:
            paths[f"spots_all 1 monitor J = {J} {layout}"] = lambda s=s, J=J: table.spots_all(s, offsets=scan[J], monitors=[mon])
        paths[f"spots_all 8 monitors J = 32 {layout}"] = lambda s=s: table.spots_all(s, offsets=scan[32], monitors=eight)
        paths[f"image_all 1 monitor {layout}"] = lambda s=s: table.image_all(s, bins=30, monitors=[mon])
    paths["record_all 32 monitors + torch moments slots"] = lambda: by_hit_lists(segs["slots"])
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for fn in paths.values():  # warm-up: code objects, the allocator's blocks, the library's scratch
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
        if k.startswith("spots_all"):
            found = paths[k]()
            row["cells"] = sum(len(sp.offsets) for sp in found)
            row["launches"] = len(spots_plan(len(found), len(found[0].offsets)))
            row["hits"] = int(sum(int(sp.counts.sum()) for sp in found))
        rows.append(row)
        extra = f"{row['cells']} cells in {row['launches']} launches, {row['hits']} hits" if "cells" in row else ""
        print(f"{k:48s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})   {extra}", flush=True)
    # the two routes give the same numbers
    ours, theirs = table.spots_all(segs["slots"], offsets=scan[32], monitors=[mon])[0].sums, by_hit_lists(segs["slots"])
    agree = float(((ours - theirs).abs().amax(dim=0) / theirs.abs().amax(dim=0)).max())  # (per sum, against its largest plane)
    print(f"largest difference between spots_all and the hit-list route, J = 32, relative to the sum's largest plane: {agree:.3g}")
    record = {"tool": "tools/bench_spots.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds,
              "note": "one run, one process, alternating rounds; whole public calls between events",
              "largest_relative_difference_J32": agree, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
