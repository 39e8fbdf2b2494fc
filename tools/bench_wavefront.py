#!/usr/bin/env python3
"""Wavefront error (`table.wavefront_all`, ot_monitor_wavefront_many, the wavefront mode of k_mon_spots: 61 moments of the optical
path difference per monitor, reduced on the device with no floating-point atomic) in two segment layouts, on one and on eight
monitors, beside what stands next to it:
  wavefront_all, explicit piston        one pass over the segments
  wavefront_all, piston=None            two passes: the mean of W, then the sums about it
  spots_all, J = 1                      the same kernel's seven values a cell on the same segments
  record_all + torch least squares      the route a user had before: hit lists (wavefrontList, yList, zList, IList), the 15 Noll
                                        terms hit by hit and their weighted normal equations with torch (`slots`, one monitor)

Workload: cfg 2 at 1e6 rays x 5 segments, fp64; 6 x 6 monitors in the collimated beam (x = 7.5; eight between 6.6 and 8.4) against
the plane wave along x, pupil radius 0.8 in position coordinates.  A time is that of the whole public call between two events on
the engine's stream, after a warm-up; reported: the median of the rounds and their spread.  All figures come from one run, one
process, the paths alternating round by round.

    python tools/bench_wavefront.py [--rays 1000000] [--rounds 11] [--out profiles/wavefront.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavefront.json"))
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import wavefront_plan
    from optable_amd.wavefront import MONOMIALS, noll_matrix

    assert torch.cuda.is_available(), "bench_wavefront.py measures on an MI355X"
    assert args.rounds >= 9
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    eight = [oa.Monitor([x, 0, 0], 6, 6) for x in np.linspace(6.6, 8.4, 8)]
    direction, pupil, piston = (1.0, 0.0, 0.0), (0.0, 0.0, 0.8), 6.0
    batch = RayBatch.from_arrays(*W.cfg2_rays(args.rays, 0), wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}
    A = torch.as_tensor(noll_matrix(), device="cuda")

    def by_hit_lists(s):
        (h,) = table.record_all(s, monitors=[mon])
        Wl, w = h.wavefrontList(direction=direction, sort=None), h.IList(None).double()
        p, q = (h.yList(None).double() - pupil[0]) / pupil[2], (h.zList(None).double() - pupil[1]) / pupil[2]
        inside = p * p + q * q <= 1.0
        Wl, w, p, q = Wl[inside], w[inside], p[inside], q[inside]
        mean = (w * Wl).sum() / w.sum()
        Z = A @ torch.stack([p**a * q**b for a, b in MONOMIALS])
        G, rhs = (Z * w) @ Z.T, (Z * w) @ (Wl - mean)  # the normal equations on the device, their 15 x 15 solve on the host
        return torch.linalg.solve(G.cpu(), rhs.cpu()).to(G.device), mean

    paths = {}
    for layout in LAYOUTS:
        s = segs[layout]
        for name, mons in (("1 monitor", [mon]), ("8 monitors", eight)):
            paths[f"wavefront_all {name} piston given {layout}"] = lambda s=s, mons=mons: table.wavefront_all(s, direction=direction, pupil=pupil, monitors=mons, piston=piston)
            paths[f"wavefront_all {name} piston=None {layout}"] = lambda s=s, mons=mons: table.wavefront_all(s, direction=direction, pupil=pupil, monitors=mons)
            paths[f"spots_all {name} J = 1 {layout}"] = lambda s=s, mons=mons: table.spots_all(s, monitors=mons)
    paths["record_all 1 monitor + torch least squares slots"] = lambda: by_hit_lists(segs["slots"])
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
        if k.startswith("wavefront_all"):
            found = paths[k]()
            row["monitors"], row["launches"] = len(found), len(wavefront_plan(len(found)))
            row["inside"], row["outside"] = int(sum(int(wf.counts) for wf in found)), int(sum(int(wf.outside) for wf in found))
        rows.append(row)
        extra = f"{row['launches']} launch(es) a pass, {row['inside']} hits inside, {row['outside']} outside" if "inside" in row else ""
        print(f"{k:52s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})   {extra}", flush=True)
    # the two routes give the same numbers
    wf = table.wavefront_batch(mon, segs["slots"], direction=direction, pupil=pupil)
    theirs, mean = by_hit_lists(segs["slots"])
    ours = wf.coefficients()
    ours[0] -= float(mean)
    agree = float((ours - theirs).abs().max())
    print(f"largest difference between coefficients() and the hit-list route: {agree:.3g} (rms wavefront error {float(wf.rms()):.3g})")
    record = {"tool": "tools/bench_wavefront.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds,
              "note": "one run, one process, alternating rounds; whole public calls between events",
              "largest_coefficient_difference": agree, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
