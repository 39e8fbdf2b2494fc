#!/usr/bin/env python3
"""The diffraction PSF (`table.psf_all`, ot_monitor_psf_many: the hit list of record_all, then k_mon_psf — per-axis phasor tables in
LDS and a complex product on the fp64 matrix cores, no transcendental per pixel and no floating-point atomic) on one monitor, in two
segment layouts, at 33, 65, 129 and 257 samples squared, beside the two routes a user had before on the same segments:
  wave_all, 30 x 30 bins, wide beams   every hit's Gaussian beam on every bin: a sincospi and an fp64 atomic per hit and bin
  record_all + torch                   hit lists, then chunked torch.exp and a complex matmul per chunk of hits

Workload: cfg 2 at 1e6 rays x 5 segments, fp64; the 6 x 6 monitor in the collimated beam (x = 7.5: every ray crosses it on its way
to the mirrors and on its way back) against the plane wave along x, samples 4e-6 apart in direction cosines.  A time is that of the
whole public call between two events on the engine's stream, after a warm-up; reported: the median of the rounds and their spread.
All figures come from one run, one process, the paths alternating round by round.  The torch route's field must agree with
psf_all's within the accuracy contract's bound (include/optable_hip.h), which the tool computes from the hit lists.

    python tools/bench_psf.py [--rays 1000000] [--rounds 11] [--out profiles/psf.json]"""
import argparse
import datetime
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

LAYOUTS = ("slots", "append")
PIXELS = (33, 65, 129, 257)
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
    ap.add_argument("--torch-pixels", type=int, default=65, help="samples squared of the torch route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psf.json"))
    args = ap.parse_args()
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import psf_plan

    assert torch.cuda.is_available(), "bench_psf.py measures on an MI355X"
    assert args.rounds >= 9
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mon = oa.Monitor([7.5, 0, 0], 6, 6)
    direction = (1.0, 0.0, 0.0)
    rays = W.cfg2_rays(args.rays, 0)
    batch = RayBatch.from_arrays(*rays, wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision="f64")
    wide = RayBatch.from_arrays(*rays, wavelength=W.WL, q=1j * np.pi * 1.5**2 / W.WL, precision="f64")  # tools/bench_wave.py: every hit reaches every bin
    segs = {layout: table.trace_batch(batch, max_segments=5, layout=layout) for layout in LAYOUTS}
    segs_wide = table.trace_batch(wide, max_segments=5, layout="slots")

    def by_torch(s, n, chunk=1 << 15):
        """U[k, l] = sum_j a_j exp(2 pi i (x0_j + gy_j y_k + gz_j z_l)) from record_all's hit lists: per chunk of hits the two
        phasor tables by torch.exp and one complex matmul.  Returns (U, the contract's bound for these hits)."""
        (h,) = table.record_all(s, monitors=[mon])
        Wl = h.wavefrontList(direction=direction, sort=None)
        y, z, a = h.yList(None).double(), h.zList(None).double(), h.IList(None).double().sqrt()
        x0, gy, gz = Wl / W.WL, -y / W.WL, -z / W.WL  # (n = 1 at the monitor)
        k = (torch.arange(n, device=Wl.device, dtype=torch.float64) - (n - 1) / 2) * STEP
        U = torch.zeros((n, n), dtype=torch.complex128, device=Wl.device)
        for j in range(0, len(Wl), chunk):
            e = slice(j, j + chunk)
            A = a[e, None] * torch.exp(2j * math.pi * (torch.frac(x0[e, None]) + torch.frac(gy[e, None] * k[None, :])))
            B = torch.exp(2j * math.pi * torch.frac(gz[e, None] * k[None, :]))
            U += A.T @ B
        size = float((Wl.abs() + (y * y + z * z).sqrt()).max())
        return U, float(a.sum()) * (2 * math.pi * 16 * 2.0**-53 * size / W.WL + 2.0**-38)

    paths = {}
    for layout in LAYOUTS:
        for n in PIXELS:
            paths[f"psf_all {n:3d} x {n:3d} {layout}"] = lambda s=segs[layout], n=n: table.psf_all(s, W.WL, direction=direction, step=STEP, pixels=n, monitors=[mon])
    paths["wave_all 30 x 30 wide beams slots"] = lambda: table.wave_all(segs_wide, W.WL, bins=30, monitors=[mon])
    paths[f"record_all + torch {args.torch_pixels} x {args.torch_pixels} slots"] = lambda: by_torch(segs["slots"], args.torch_pixels)
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
        found = paths[k]()
        if k.startswith("psf_all"):
            hits, n = int(found[0].counts), found[0].re.shape[0]
            plan = psf_plan(n, n, [hits])
            row.update(hits=hits, pixels=n * n, tiles=len(plan["tiles"]), chunks=plan["chunks"][0], launches=plan["launches"],
                       hit_pixels_per_s=round(hits * n * n / (row["ms_median"] * 1e-3), -6))
        elif k.startswith("wave_all"):
            hits = int(found[0].counts.sum())
            row.update(hits=hits, pixels=900, hit_pixels_per_s=round(hits * 900 / (row["ms_median"] * 1e-3), -6))
        else:
            hits = int(table.psf_all(segs["slots"], W.WL, direction=direction, step=STEP, pixels=args.torch_pixels, monitors=[mon])[0].counts)
            row.update(hits=hits, pixels=args.torch_pixels**2, hit_pixels_per_s=round(hits * args.torch_pixels**2 / (row["ms_median"] * 1e-3), -6))
        rows.append(row)
        print(f"{k:44s} {row['ms_median']:9.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f})   {row['hits']} hits x {row['pixels']} = "
              f"{row['hit_pixels_per_s']:.3g} hit-pixels/s", flush=True)
    # table building against product: a call costs hits x (t_hit + pixels t_pixel); the 33- and the 257-squared case give the two
    by = {(r["path"].split()[-1], r["pixels"]): r for r in rows if r["path"].startswith("psf_all")}
    shares = {}
    for layout in LAYOUTS:
        small, large = by[(layout, 33 * 33)], by[(layout, 257 * 257)]
        t_pixel = (large["ms_median"] - small["ms_median"]) / (large["pixels"] - small["pixels"])
        shares[layout] = {f"{n} x {n}": round(1.0 - t_pixel * n * n / by[(layout, n * n)]["ms_median"], 3) for n in PIXELS}
        print(f"{layout}: share of a call that does not grow with the pixels (hit pass, tables, partials): {shares[layout]}")
    # the two routes give the same field
    n = args.torch_pixels
    ours = table.psf_all(segs["slots"], W.WL, direction=direction, step=STEP, pixels=n, monitors=[mon])[0]
    theirs, bound = by_torch(segs["slots"], n)
    agree = float((ours.field - theirs).abs().max())
    print(f"largest difference between psf_all and the torch route at {n} x {n}: {agree:.3g} (bound {bound:.3g}, norm {float(ours.norm):.4g})")
    assert agree <= bound, (agree, bound)
    record = {"tool": "tools/bench_psf.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "segments": 5 * args.rays, "rounds": args.rounds, "step": STEP,
              "note": "one run, one process, alternating rounds; whole public calls between events",
              "largest_difference_to_the_torch_route": agree, "bound": bound, "share_not_growing_with_pixels": shares, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
