#!/usr/bin/env python3
"""Gaussian-beam detector images against point images: `table.beam_all` (ot_monitor_beam_many: every hit spread over its spot
size, fy + fz + 2 erf evaluations and fy * fz atomic adds a hit) beside `table.image_all` (one add a hit) and `table.field_all`
(two) on the same monitors, in one process, alternating round by round.

Workload: cfg 2 at 1e6 rays x 5 segments, fp64, slots; M monitors of a through-focus stack (default 6), bins 30, two beam widths:
  narrow  cfg 2's own waist (W0 = 61 um: w some 0.02 at the monitors, a tenth of a bin — at most 4 bins a hit)
  wide    a waist of 1.5 (w some 1.2 .. 1.5 behind the lens: a quarter of the 6 x 6 monitor — every hit reaches every bin)
A time is that of the whole public call between two events on the engine's stream, after a warm-up; reported: the median of the
rounds and their spread.  beam_all and field_all read their `skipped` counter back before they return (8 bytes, one
synchronisation); image_all returns without reading anything.

    python tools/bench_beam.py [--rays 1000000] [--rounds 21] [--monitors 6] [--out profiles/beam_image.json]
    env: OT_LIB = another build of the library (the parent commit's, for an A/B in one job)
    python tools/bench_beam.py --probe     the device math library's double erf against scipy.special.erf, in ulp of erf, on 1e5
                                           arguments in [-8, 8]: a one-line kernel of its own in a process of its own (what the
                                           bound of tests/test_gpu_beam.py takes for E_DEV, doubled)"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

BINS = 30
PROBE = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void k_probe(const double* x, double* y, int n) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) y[i] = erf(x[i]); }
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    fseek(in, 0, SEEK_END); const int n = (int)(ftell(in) / 8); fseek(in, 0, SEEK_SET);
    std::vector<double> x(n), y(n);
    if (fread(x.data(), 8, n, in) != (size_t)n) return 2;
    fclose(in);
    double *dx, *dy;
    if (hipMalloc((void**)&dx, 8 * n) != hipSuccess || hipMalloc((void**)&dy, 8 * n) != hipSuccess) return 3;
    if (hipMemcpy(dx, x.data(), 8 * n, hipMemcpyHostToDevice) != hipSuccess) return 3;
    hipLaunchKernelGGL(k_probe, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n);
    if (hipMemcpy(y.data(), dy, 8 * n, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(y.data(), 8, n, out) != (size_t)n) return 4;
    fclose(out);
    return 0;
}
"""


def probe():
    """Largest |device erf - scipy erf| in ulp of the value over 1e5 arguments in [-8, 8] (half of them uniform, half dense around 0)."""
    from scipy.special import erf

    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-8, 8, 50_000), rng.normal(0, 1.5, 50_000).clip(-8, 8)])
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, f) for f in ("probe.hip", "probe", "x.bin", "y.bin"))
        open(src, "w").write(PROBE)
        x.tofile(fin)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", src, "-o", exe], timeout=300)
        subprocess.check_call([exe, fin, fout], timeout=120)
        y = np.fromfile(fout, dtype=np.float64)
    ref = erf(x)
    ulp = np.spacing(np.abs(ref))
    err = np.abs(y - ref) / ulp
    at = int(np.argmax(err))
    result = {"arguments": len(x), "range": [-8, 8], "max_ulp": float(err[at]), "at": float(x[at]), "mean_ulp": float(err.mean()),
              "differing": int((err > 0).sum())}
    print(f"device erf against scipy.special.erf: largest difference {err[at]:.3g} ulp at x = {x[at]:.17g}, mean {err.mean():.3g} ulp, "
          f"{result['differing']} of {len(x)} differ", flush=True)
    return result


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
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_image.json"))
    args = ap.parse_args()
    if args.probe:
        found = probe()
        out = os.path.splitext(args.out)[0] + "_erf_probe.json"
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump({"tool": "tools/bench_beam.py --probe", "date": datetime.date.today().isoformat(), **found}, fh, indent=1)
        print("wrote", out)
        return
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import beam_plan, field_plan, image_plan

    if os.environ.get("OT_LIB"):  # an A/B build of the library, e.g. the parent commit's against this tree's
        abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
    assert torch.cuda.is_available(), "bench_beam.py measures on an MI355X"
    table = oa.OpticalTable()
    table.add_components(W.cfg2_components(oa))
    mons = [oa.Monitor([6.0 + 3.0 * k / 32, 0, 0], 6, 6) for k in range(args.monitors)]  # the stack of tools/bench_monitors.py
    o, d = W.cfg2_rays(args.rays, 0)
    segs, spots = {}, {}
    for name, w0 in (("narrow", W.W0), ("wide", 1.5)):
        batch = RayBatch.from_arrays(o, d, wavelength=W.WL, q=1j * np.pi * w0**2 / W.WL, precision="f64")
        segs[name] = table.trace_batch(batch, max_segments=5, layout="slots")
        w = table.record_all(segs[name], monitors=mons[:1])[0].spotsizeList(W.WL, None)
        spots[name] = [float(w.min()), float(w.median()), float(w.max())]
        print(f"{name}: w0 = {w0:g}, w at the first monitor {spots[name][0]:.4g} .. {spots[name][2]:.4g} (bin {6 / BINS:g})", flush=True)
    paths = {"image_all": lambda: table.image_all(segs["narrow"], bins=BINS, monitors=mons),
             "field_all": lambda: table.field_all(segs["narrow"], W.WL, bins=BINS, monitors=mons),
             "beam_all_narrow": lambda: table.beam_all(segs["narrow"], W.WL, bins=BINS, monitors=mons),
             "beam_all_wide": lambda: table.beam_all(segs["wide"], W.WL, bins=BINS, monitors=mons)}
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
    hits = sum(int(im.counts.sum()) for im in paths["image_all"]())
    caught = {k: float(sum(b.power.sum() for b in paths[k]())) for k in ("beam_all_narrow", "beam_all_wide")}
    row = {"workload": "cfg2 fp64 slots", "monitors": args.monitors, "bins": [BINS, BINS], "hits": hits, "spot_size_min_median_max": spots,
           "power_on_the_monitors": caught, "image_plan": image_plan(args.monitors, BINS, BINS), "field_plan": field_plan(args.monitors, BINS, BINS),
           "beam_plan": beam_plan(args.monitors, BINS, BINS)}
    for k, t in times.items():
        row[k] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
        print(f"M={args.monitors} bins={BINS}  {k:18s} {row[k]['ms_median']:9.3f} ms ({row[k]['ms_min']:.3f} .. {row[k]['ms_max']:.3f})", flush=True)
    record = {"tool": "tools/bench_beam.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "rounds": args.rounds, "rows": [row]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
