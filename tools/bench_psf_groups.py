#!/usr/bin/env python3
"""The diffraction PSF per ray group (`table.psf_grouped_all`, ot_monitor_psf_groups_many: the hit list of record_all split by group
on the device by the two partition passes of k_mon_psf, then its sum over the cells (monitor, group)) on one monitor, in two segment
layouts, with G = 8 and G = 64 groups, ids in contiguous blocks and at random, at 65 and 129 samples squared — beside, on the same
rays:
  psf_all                      the ungrouped call: every hit into one field (what the sum alone costs)
  G x (take, trace, psf_all)   the way without the feature: the rays of every group gathered (`RayBatch.take`), traced alone and
                               summed alone, G times

Workload: cfg 2 at 1e6 rays x 5 segments, fp64; the 6 x 6 monitor in the collimated beam (x = 7.5) against the plane wave along x,
samples 4e-6 apart in direction cosines (tools/bench_psf.py's).  A time is that of the whole public call(s) between two events on
the engine's stream, after a warm-up; reported: the median of the rounds and their spread.  All figures come from one run, one
process, the paths alternating round by round.  Every group of a grouped call must equal the group traced alone, bit for bit
(checked for the slot layout at 65 x 65).

    python tools/bench_psf_groups.py [--rays 1000000] [--rounds 11] [--out profiles/psf_groups.json]"""
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
PIXELS = (65, 129)
GROUPS = (8, 64)
STEP = 4e-6


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psf_groups.json"))
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import psf_groups_plan

    assert torch.cuda.is_available(), "bench_psf_groups.py measures on an MI355X"
    assert args.rounds >= 9
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    kw = dict(direction=(1.0, 0.0, 0.0), step=STEP, monitors=[mon])
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}
    ids = {(G, "blocks"): torch.from_numpy((np.arange(args.rays) * G // args.rays).astype(np.int32)).cuda() for G in GROUPS}
    ids.update({(G, "random"): torch.from_numpy(np.random.default_rng(0).integers(0, G, args.rays).astype(np.int32)).cuda() for G in GROUPS})
    members = {G: [torch.nonzero(ids[G, "random"] == g).ravel() for g in range(G)] for G in GROUPS}

    def one_by_one(G, layout, n):
        return [table.psf_all(table.trace_batch(batch.take(index), max_segments=5, layout=layout), W.WL, pixels=n, **kw)[0] for index in members[G]]

    paths = {}
    for layout in LAYOUTS:
        for n in PIXELS:
            paths[f"psf_all {n:3d} x {n:3d} {layout}"] = lambda s=segs[layout], n=n: table.psf_all(s, W.WL, pixels=n, **kw)
            for G in GROUPS:
                for order in ("blocks", "random"):
                    paths[f"psf_grouped_all G = {G:2d} {order} ids {n:3d} x {n:3d} {layout}"] = (
                        lambda s=segs[layout], n=n, t=ids[G, order], G=G: table.psf_grouped_all(s, W.WL, t, n_groups=G, pixels=n, **kw))
                paths[f"{G:2d} x (take, trace, psf_all) {n:3d} x {n:3d} {layout}"] = lambda G=G, layout=layout, n=n: one_by_one(G, layout, n)
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
        if k.startswith("psf_grouped_all"):
            p = paths[k]()[0]
            plan = psf_groups_plan(p.re.shape[1], p.re.shape[2], [(p.counts + p.skipped).tolist()])
            row.update(hits=int(p.counts.sum()), groups=p.n_groups, partition_tiles=plan["partition_tiles"][0], most_chunks=max(plan["chunks"][0]),
                       pairs_a_launch=plan["pairs_a_launch"], launches=plan["launches"])
        rows.append(row)
        print(f"{k:58s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})", flush=True)
    by = {r["path"]: r["ms_median"] for r in rows}
    summary = []
    for layout in LAYOUTS:
        for n in PIXELS:
            plain = by[f"psf_all {n:3d} x {n:3d} {layout}"]
            for G in GROUPS:
                line = {"layout": layout, "pixels": n, "groups": G, "psf_all_ms": plain, "one_by_one_ms": by[f"{G:2d} x (take, trace, psf_all) {n:3d} x {n:3d} {layout}"]}
                line.update({f"grouped_{order}_ms": by[f"psf_grouped_all G = {G:2d} {order} ids {n:3d} x {n:3d} {layout}"] for order in ("blocks", "random")})
                summary.append(line)
                print(f"{layout} {n} x {n} G = {G}: grouped {line['grouped_blocks_ms']:.3f} (blocks) / {line['grouped_random_ms']:.3f} (random) ms, "
                      f"psf_all {plain:.3f} ms, {G} x (take, trace, psf_all) {line['one_by_one_ms']:.3f} ms")
    # a group of the grouped call is the group traced alone, bit for bit
    G = GROUPS[0]
    grouped = table.psf_grouped_all(segs["slots"], W.WL, ids[G, "random"], n_groups=G, pixels=65, **kw)[0]
    for g, alone in enumerate(one_by_one(G, "slots", 65)):
        assert torch.equal(grouped.re[g], alone.re) and torch.equal(grouped.im[g], alone.im) and int(grouped.counts[g]) == int(alone.counts), g
    print(f"every group of the grouped call (G = {G}, random ids, slots, 65 x 65) equals the group traced alone, bit for bit")
    record = {"tool": "tools/bench_psf_groups.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds, "step": STEP,
              "note": "one run, one process, alternating rounds; whole public calls between events", "summary": summary, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):  # (the file also keeps the lines of tools/bench_psf.py on the parent and on this commit: see DESIGN.md 4.6g)
        with open(args.out) as fh:
            kept = json.load(fh)
        record = {**{k: v for k, v in kept.items() if k == "psf_all_against_the_parent"}, **record}
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
