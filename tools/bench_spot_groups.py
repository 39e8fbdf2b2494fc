#!/usr/bin/env python3
"""Spot statistics per ray group (`table.spots_grouped_all`, ot_monitor_spot_groups_many, the group mode of k_mon_spots: the
moments of a monitor's hits per plane and per group of input rays, reduced on the device with no floating-point atomic) in two
segment layouts and two arrangements of the ids, beside the ways to the same numbers the package had before:
  spots_grouped_all, G = 8, group-major ids    every wave of the slot layout holds one group: one butterfly set per (plane, wave)
  spots_grouped_all, G = 8, random ids         every wave holds all eight groups: the in-wave walk, eight butterfly sets
  spots_all                                    the ungrouped call on the same segments: what one group alone costs
  8 x spots_all                                eight ungrouped calls: what eight separately traced batches would take to reduce
                                               (each over the whole segments here, as W traces of the whole pupil would be)
  record_all over 32 displaced monitors,       32 hit lists, then the seven sums of every (plane, group) with index_add_ by the
  then torch index_add_ by the hits' group     id of each hit's ray (spread over 1,024 rows a group, which are then summed), on the device (`slots` only)

Workload: cfg 2 at 1e6 rays x 5 segments, fp64; one 6 x 6 monitor at x = 7.5 with J = 32 planes over +-0.9.  A time is that of the
whole public call between two events on the engine's stream, after a warm-up; reported: the median of the rounds and their
spread.  All figures come from one run, one process, the paths alternating round by round.

    python tools/bench_spot_groups.py [--rays 1000000] [--rounds 11] [--out profiles/spot_groups.json]"""
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
G, J, SPREAD = 8, 32, 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spot_groups.json"))
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import spot_groups_plan

    assert torch.cuda.is_available(), "bench_spot_groups.py measures on an MI355X"
    assert args.rounds >= 9
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    scan = np.linspace(-0.9, 0.9, J)
    displaced = [oa.Monitor([7.5 + off, 0, 0], 6, 6) for off in scan]
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}
    ids = {"group-major": torch.from_numpy((np.arange(args.rays) * G // args.rays).astype(np.int32)).cuda(),
           "random": torch.from_numpy(np.random.default_rng(0).integers(0, G, args.rays).astype(np.int32)).cuda()}

    def by_hit_lists(s, table_of_ids):
        out = []
        for h in table.record_all(s, monitors=displaced):
            y, z, w, g = h.yList(None), h.zList(None), h.IList(None), table_of_ids[h.ray_index(None).long()].long()
            terms = torch.stack([torch.ones_like(w), w, w * y, w * z, w * y * y, w * z * z, w * y * z], dim=1)
            # SPREAD rows a group, then their sum: index_add_ is atomic adds, and two million hits on G rows would queue on G x 7 addresses
            rows = g * SPREAD + torch.arange(len(g), device=g.device) % SPREAD
            out.append(torch.zeros((G * SPREAD, 7), dtype=torch.float64, device=w.device).index_add_(0, rows, terms.double()).view(G, SPREAD, 7).sum(dim=1))
        return torch.stack(out)

    paths = {}
    for layout in LAYOUTS:
        s = segs[layout]
        for name, t in ids.items():
            paths[f"spots_grouped_all G = {G} {name} ids J = {J} {layout}"] = lambda s=s, t=t: table.spots_grouped_all(s, t, n_groups=G, offsets=scan, monitors=[mon])
        paths[f"spots_all J = {J} {layout}"] = lambda s=s: table.spots_all(s, offsets=scan, monitors=[mon])
        paths[f"{G} x spots_all J = {J} {layout}"] = lambda s=s: [table.spots_all(s, offsets=scan, monitors=[mon]) for _ in range(G)]
    paths[f"record_all {J} monitors + torch index_add_ slots"] = lambda: by_hit_lists(segs["slots"], ids["random"])
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for k, fn in paths.items():  # warm-up: code objects, the allocator's blocks, the library's scratch
        fn()
        print(f"warm-up {k}: {timed(fn, ev)[0]:.3f} ms", flush=True)
    times = {k: [] for k in paths}
    for rnd in range(args.rounds):
        for k in (sorted(paths) if rnd % 2 else sorted(paths, reverse=True)):
            ms, found = timed(paths[k], ev)
            times[k].append(ms)
            del found
    rows = []
    for k, t in times.items():
        row = {"path": k, "ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
        if k.startswith("spots_grouped_all"):
            found = paths[k]()
            row["cells"] = int(found[0].counts.numel())
            row["launches"] = len(spot_groups_plan(1, J, G))
            row["hits"] = int(found[0].counts.sum())
        rows.append(row)
        extra = f"{row['cells']} cells in {row['launches']} launches, {row['hits']} hits" if "cells" in row else ""
        print(f"{k:58s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})   {extra}", flush=True)
    # the routes give the same numbers
    ours = table.spots_grouped_all(segs["slots"], ids["random"], n_groups=G, offsets=scan, monitors=[mon])[0]
    theirs = by_hit_lists(segs["slots"], ids["random"])
    assert torch.equal(ours.counts, theirs[..., 0].long()), "the two routes count differently"
    agree = float(((ours.sums - theirs[..., 1:]).abs().amax(dim=(0, 1)) / theirs[..., 1:].abs().amax(dim=(0, 1))).max())
    print(f"largest difference between spots_grouped_all and the hit-list route, relative to the sum's largest cell: {agree:.3g}")
    by = {r["path"]: r for r in rows}
    verdict = {}
    for layout in LAYOUTS:
        one, eight = by[f"spots_grouped_all G = {G} group-major ids J = {J} {layout}"], by[f"{G} x spots_all J = {J} {layout}"]
        verdict[layout] = {"grouped_ms": one["ms_median"], "ungrouped_calls_ms": eight["ms_median"], "grouped_is_cheaper": one["ms_median"] < eight["ms_median"]}
        print(f"{layout}: one grouped call {one['ms_median']:.3f} ms against {G} ungrouped calls {eight['ms_median']:.3f} ms")
    record = {"tool": "tools/bench_spot_groups.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds, "groups": G, "planes": J,
              "note": "one run, one process, alternating rounds; whole public calls between events",
              "largest_relative_difference": agree, "group_major_against_ungrouped_calls": verdict, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
