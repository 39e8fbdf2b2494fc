#!/usr/bin/env python3
"""Wavefront error per ray group (`table.wavefront_grouped_all`, ot_monitor_wavefront_groups_many, the wavefront mode's group mode
of k_mon_spots: the 61 moments of a monitor's hits per group of input rays, with a reference, pupil and piston per group) in two
segment layouts and two arrangements of the ids, beside the ways to the same numbers the package had before:
  wavefront_grouped_all, G = 8, block ids      every wave of the slot layout holds one group: one set of 61 butterflies a wave
  wavefront_grouped_all, G = 8, random ids     every wave holds all eight groups: the in-wave walk, eight sets
  wavefront_grouped_all, G = 64, random ids    ceil(64 / 28) = 3 passes over the segments
  wavefront_all                                the ungrouped call on the same segments: what one group alone costs
  8 x (take, trace, wavefront_all)             every group's rays taken out of the batch, traced alone and reduced alone
  record_all + torch per group                 one hit list, then the 61 sums of every group by masked sums on the device (`slots` only)
`--lib PATH` measures another build of the library (same ABI version); where that library has no
ot_monitor_wavefront_groups_many (an older build: the symbol is looked for in the file itself) the entry is left unbound, the
grouped rows are skipped and the comparison routes alone are timed.

Workload: cfg 2 at 1e6 rays x 5 segments, fp64; one 6 x 6 monitor at x = 7.5 against the plane wave along x, pupil radius 0.8.  A
time is that of the whole public call between two events on the engine's stream, after a warm-up; reported: the median of the
rounds and their spread.  All figures come from one run, one process, the paths alternating round by round.

    python tools/bench_wavefront_groups.py [--rays 1000000] [--rounds 11] [--lib PATH] [--out profiles/wavefront_groups_bench.json]"""
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
G, G_WIDE = 8, 64
PUPIL, PISTON = (0.0, 0.0, 0.8), 10.0


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavefront_groups_bench.json"))
    ap.add_argument("--lib", default=None, help="another build of liboptable_hip.so to measure")
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.wavefront import N_SUMS, N_S, MONOMIALS

    assert torch.cuda.is_available(), "bench_wavefront_groups.py measures on an MI355X"
    assert args.rounds >= 9
    entry = "ot_monitor_wavefront_groups_many"
    if args.lib:
        abi.LIB_PATH = os.path.abspath(args.lib)
    with open(abi.LIB_PATH, "rb") as fh:  # (the dynamic symbol's name, without loading anything)
        have = entry.encode() + b"\0" in fh.read()
    if not have:
        abi.SYMBOLS.pop(entry, None)  # abi.load() binds every declared symbol: this library has one fewer
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}
    rng = np.random.default_rng(0)
    ids = {"block": torch.from_numpy((np.arange(args.rays) * G // args.rays).astype(np.int32)).cuda(),
           "random": torch.from_numpy(rng.integers(0, G, args.rays).astype(np.int32)).cuda()}
    wide = torch.from_numpy(rng.integers(0, G_WIDE, args.rays).astype(np.int32)).cuda()
    members = [torch.nonzero(ids["block"] == g).flatten() for g in range(G)]
    kw = dict(direction=(1.0, 0.0, 0.0), pupil=PUPIL, piston=PISTON, monitors=[mon])

    def traced_alone(layout):
        return [table.wavefront_all(table.trace_batch(batch.take(rows), max_segments=5, layout=layout), **kw) for rows in members]

    def by_hit_list(s, table_of_ids, n_groups):
        (h,) = table.record_all(s, monitors=[mon])
        Wl, w = h.wavefrontList(sort=None, direction=(1.0, 0.0, 0.0)) - PISTON, h.IList(None).double()
        p, q = (h.yList(None) - PUPIL[0]) / PUPIL[2], (h.zList(None) - PUPIL[1]) / PUPIL[2]
        g = table_of_ids[h.ray_index(None).long()].long()
        inside = (p * p + q * q <= 1.0) & torch.isfinite(Wl)
        S = [(a - b, b) for a in range(9) for b in range(a + 1)]
        terms = torch.stack([w * p**a * q**b for a, b in S] + [w * Wl * p**a * q**b for a, b in MONOMIALS] + [w * Wl * Wl], dim=1)
        assert terms.shape[1] == N_SUMS and len(S) == N_S
        return torch.stack([(terms * (inside & (g == k))[:, None]).sum(dim=0) for k in range(n_groups)])

    paths = {}
    for layout in LAYOUTS:
        s = segs[layout]
        if have:
            for name, t in ids.items():
                paths[f"wavefront_grouped_all G = {G} {name} ids {layout}"] = lambda s=s, t=t: table.wavefront_grouped_all(s, t, n_groups=G, **kw)
            paths[f"wavefront_grouped_all G = {G_WIDE} random ids {layout}"] = lambda s=s: table.wavefront_grouped_all(s, wide, n_groups=G_WIDE, **kw)
        paths[f"wavefront_all {layout}"] = lambda s=s: table.wavefront_all(s, **kw)
        paths[f"{G} x (take, trace, wavefront_all) {layout}"] = lambda layout=layout: traced_alone(layout)
    paths[f"record_all + torch per group G = {G} slots"] = lambda: by_hit_list(segs["slots"], ids["random"], G)
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
        if k.startswith("wavefront_grouped_all"):
            from optable_amd.engine import wavefront_groups_plan

            found = paths[k]()[0]
            row["cells"], row["launches"] = found.n_groups, len(wavefront_groups_plan(1, found.n_groups))
            row["hits"] = int(found.counts.sum() + found.outside.sum())
        rows.append(row)
        extra = f"{row['cells']} cells in {row['launches']} launches, {row['hits']} hits" if "cells" in row else ""
        print(f"{k:58s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})   {extra}", flush=True)
    agree = None
    if have:  # the routes give the same numbers
        ours = table.wavefront_grouped_all(segs["slots"], ids["random"], n_groups=G, **kw)[0]
        theirs = by_hit_list(segs["slots"], ids["random"], G)
        scale = theirs.abs().amax(dim=0).clamp_min(1e-300)
        agree = float(((ours.sums - theirs).abs().amax(dim=0) / scale).max())
        print(f"largest difference between wavefront_grouped_all and the hit-list route, relative to the sum's largest cell: {agree:.3g}")
    else:
        print("this library has no wavefront_grouped_all: the comparison routes alone were timed")
    record = {"tool": "tools/bench_wavefront_groups.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds, "groups": G,
              "groups_wide": G_WIDE, "grouped_entry": have, "note": "one run, one process, alternating rounds; whole public calls between events",
              "largest_relative_difference": agree, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
