#!/usr/bin/env python3
"""Coherent Gaussian-beam detector images against the two modes they combine: `table.wave_all` (ot_monitor_wave_many, k_mon_wave:
every hit a complex Gaussian sampled at the bin centres — fy + fz exp / sincospi pairs and 2 fy fz atomic adds a hit) beside
`table.beam_all` (fy + fz + 2 erf, fy fz adds) and `table.field_all` (one phasor, two adds) on the SAME segments, monitors and bins,
in one process, alternating round by round.

Workload: cfg 2 at 1e6 rays x 5 segments, fp64, slots; M monitors of a through-focus stack (default 8), bins 30, two beam widths:
  narrow  cfg 2's own waist (W0 = 61 um: w some 0.02 at the monitors, a tenth of a bin — most hits reach no bin centre or one)
  wide    a waist of 1.5 (w some 1.2 .. 1.5 behind the lens: a quarter of the 6 x 6 monitor — every hit reaches every bin)
A time is that of the whole public call between two events on the engine's stream, after a warm-up; reported: the median of the
rounds and their spread.  All three read a device counter back before they return (8 or 16 bytes, one synchronisation).  At 780 nm
on a 6 x 6 monitor of 30 bins nearly every hit is aliased (wave_all says so; the count is in the record): the timing is that of
the arithmetic, the image is not physics.

    python tools/bench_wave.py [--rays 1000000] [--rounds 11] [--monitors 8] [--out profiles/wave_image.json]
    env: OT_LIB = another build of the library (the parent commit's, for an A/B in one job)
    python tools/bench_wave.py --probe     the device math library's double exp and sincospi against np.longdouble on 1e5 arguments
                                           each over the ranges k_mon_wave uses (exp on [-37, 0]; sincospi(2 f), f in [0, 1), half of
                                           them dense around the zeros), in a kernel of its own in a process of its own: what the
                                           bound of tests/test_gpu_wave.py takes for E_EXP and E_SC, doubled"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

BINS = 30
PROBE = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void k_probe(const double* x, double* y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    y[i] = exp(x[i]);
    double s, c;
    sincospi(2.0 * x[n + i], &s, &c);
    y[n + i] = s, y[2 * n + i] = c;
}
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    fseek(in, 0, SEEK_END); const int n = (int)(ftell(in) / 16); fseek(in, 0, SEEK_SET);
    std::vector<double> x(2 * n), y(3 * n);
    if (fread(x.data(), 8, 2 * n, in) != (size_t)(2 * n)) return 2;
    fclose(in);
    double *dx, *dy;
    if (hipMalloc((void**)&dx, 16 * n) != hipSuccess || hipMalloc((void**)&dy, 24 * n) != hipSuccess) return 3;
    if (hipMemcpy(dx, x.data(), 16 * n, hipMemcpyHostToDevice) != hipSuccess) return 3;
    hipLaunchKernelGGL(k_probe, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n);
    if (hipMemcpy(y.data(), dy, 24 * n, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(y.data(), 8, 3 * n, out) != (size_t)(3 * n)) return 4;
    fclose(out);
    return 0;
}
"""


def probe():
    """Largest |device - np.longdouble| of exp in ulp of the value over 1e5 arguments in [-37, 0], and of sin and cos of 2 pi f in
    units of 2^-53 (the phasor has magnitude 1) and in ulp of the value over 1e5 f in [0, 1)."""
    rng = np.random.default_rng(0)
    n = 100_000
    xe = np.concatenate([rng.uniform(-37, 0, n // 2), -rng.exponential(1.0, n // 2).clip(0, 37)])
    f = np.concatenate([rng.random(n // 2), (rng.integers(0, 4, n // 2) / 4 + rng.normal(0, 1e-3, n // 2)) % 1.0])
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, name) for name in ("probe.hip", "probe", "x.bin", "y.bin"))
        open(src, "w").write(PROBE)
        np.concatenate([xe, f]).tofile(fin)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", src, "-o", exe], timeout=300)
        subprocess.check_call([exe, fin, fout], timeout=120)
        y = np.fromfile(fout, dtype=np.float64)
    dev_exp, dev_sin, dev_cos = y[:n], y[n:2 * n], y[2 * n:]
    L = np.longdouble
    ref_exp = np.exp(xe.astype(L))
    # sin, cos of pi t, t = 2 f, reduced exactly: t = m + d with m a multiple of 1 / 2 and |d| <= 1 / 4 (both exact in double)
    t = 2.0 * f
    m = np.round(2.0 * t) / 2.0
    d = (t - m).astype(L)
    pi = 4 * np.arctan(L(1))
    q = (np.round(2.0 * m).astype(np.int64)) % 4  # pi m = q pi / 2
    sm, cm = np.array([0, 1, 0, -1], dtype=L)[q], np.array([1, 0, -1, 0], dtype=L)[q]
    ref_sin, ref_cos = sm * np.cos(pi * d) + cm * np.sin(pi * d), cm * np.cos(pi * d) - sm * np.sin(pi * d)

    def ulps(dev, ref):
        err = np.abs(dev.astype(L) - ref)
        return (err / np.spacing(np.abs(ref.astype(np.float64))).astype(L)).astype(np.float64), (err / L(2.0**-53)).astype(np.float64)

    e_ulp, _ = ulps(dev_exp, ref_exp)
    s_ulp, s_abs = ulps(dev_sin, ref_sin)
    c_ulp, c_abs = ulps(dev_cos, ref_cos)
    result = {"arguments": n, "exp_range": [-37, 0], "exp_max_ulp": float(e_ulp.max()), "exp_at": float(xe[int(np.argmax(e_ulp))]),
              "exp_mean_ulp": float(e_ulp.mean()), "sincospi_f_range": [0, 1],
              "sincospi_max_abs_in_2^-53": float(max(s_abs.max(), c_abs.max())), "sincospi_max_ulp": float(max(s_ulp.max(), c_ulp.max())),
              "sincospi_mean_abs_in_2^-53": float(0.5 * (s_abs.mean() + c_abs.mean())), "reference": "np.longdouble (64-bit significand)"}
    print(f"device exp against np.longdouble: largest difference {result['exp_max_ulp']:.3g} ulp at x = {result['exp_at']:.17g}, mean "
          f"{result['exp_mean_ulp']:.3g} ulp; sincospi(2 f): largest {result['sincospi_max_abs_in_2^-53']:.3g} x 2^-53 absolute, "
          f"{result['sincospi_max_ulp']:.3g} ulp of the value", flush=True)
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
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--monitors", type=int, default=8)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_image.json"))
    args = ap.parse_args()
    if args.probe:
        found = probe()
        out = os.path.splitext(args.out)[0] + "_probe.json"
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump({"tool": "tools/bench_wave.py --probe", "date": datetime.date.today().isoformat(), **found}, fh, indent=1)
        print("wrote", out)
        return
    import torch

    import optable_amd as oa
    from optable_amd import abi
    from optable_amd import workloads as W
    from optable_amd.batch import RayBatch
    from optable_amd.engine import beam_plan, field_plan, wave_plan

    if os.environ.get("OT_LIB"):  # an A/B build of the library, e.g. the parent commit's against this tree's
        abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
    assert torch.cuda.is_available(), "bench_wave.py measures on an MI355X"
    assert args.rounds >= 5
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

    def wave(name):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (the aliased count is reported below)
            return table.wave_all(segs[name], W.WL, bins=BINS, monitors=mons)

    paths = {"field_all": lambda: table.field_all(segs["narrow"], W.WL, bins=BINS, monitors=mons),
             "beam_all_narrow": lambda: table.beam_all(segs["narrow"], W.WL, bins=BINS, monitors=mons),
             "beam_all_wide": lambda: table.beam_all(segs["wide"], W.WL, bins=BINS, monitors=mons),
             "wave_all_narrow": lambda: wave("narrow"), "wave_all_wide": lambda: wave("wide")}
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
    hits = sum(int(f.counts.sum()) for f in paths["field_all"]())
    aliased = {k: int(paths[k]()[0].aliased) for k in ("wave_all_narrow", "wave_all_wide")}
    row = {"workload": "cfg2 fp64 slots", "monitors": args.monitors, "bins": [BINS, BINS], "hits": hits, "spot_size_min_median_max": spots,
           "aliased": aliased, "field_plan": field_plan(args.monitors, BINS, BINS), "beam_plan": beam_plan(args.monitors, BINS, BINS),
           "wave_plan": wave_plan(args.monitors, BINS, BINS)}
    for k, t in times.items():
        row[k] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
        print(f"M={args.monitors} bins={BINS}  {k:18s} {row[k]['ms_median']:9.3f} ms ({row[k]['ms_min']:.3f} .. {row[k]['ms_max']:.3f})", flush=True)
    record = {"tool": "tools/bench_wave.py", "library": os.path.relpath(abi.LIB_PATH, ROOT), "date": datetime.date.today().isoformat(),
              "device": torch.cuda.get_device_name(0), "rays": args.rays, "rounds": args.rounds,
              "note": "all five figures come from this one run, one process, alternating rounds; beam_all and field_all are the parent's code",
              "rows": [row]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
