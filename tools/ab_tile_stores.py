#!/usr/bin/env python3
"""One side of an A/B on the lane-per-ray kernel's segment stores (DESIGN.md 4.1 "Tile stores"; profiles/tile_stores_cfg2.json):
cfg 2 (1e6 rays, cap 5) and cfg 4 (N4 base rays x 64 wavelengths, cap 3) with the output layout FORCED, steady reuse (batch s into
output s, four rotating for cfg 2), library hipEvent time per launch.  Prints one JSON line per case with the time of every round.
One process per side; a job alternates the sides:
    [OT_LIB=<another build's liboptable_hip.so>] [PAIR=0|1] python tools/ab_tile_stores.py <label>
    env: CASES (comma list of workload:precision:layout, default cfg2:f64:tiled,cfg2:f64:slots), ROUNDS (18), LAUNCHES (50; cfg 4: ROUNDS4 (3) x
    LAUNCHES4 (10)), N4 (500000), WARM (400), FORGET (1: forget_resident() before every launch — whole records, what a fresh output gets)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import optable_amd as oa
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch, SegmentBatch

if os.environ.get("OT_LIB"):
    abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
from optable_amd.engine import get_engine  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "this tree"
eng = get_engine()
if os.environ.get("PAIR"):
    eng.set_option(abi.OPT_PAIR_STORES, int(os.environ["PAIR"]))
Q = 1j * np.pi * W.W0**2 / W.WL
FORGET = bool(int(os.environ.get("FORGET", 0)))


def batches_of(workload, prec):
    if workload == "cfg2":
        return [RayBatch.from_arrays(*W.cfg2_rays(1_000_000, 1000 * s), wavelength=W.WL, q=Q, precision=prec) for s in range(4)], 5
    o, d, _ = W.cfg4_rays(int(os.environ.get("N4", 500_000)), 4, n_wavelengths=1)
    base = RayBatch.from_arrays(o, d, wavelength=W.WL, q=Q, precision=prec)
    return [base.multiplexed_in_wavelength(np.linspace(400e-7, 1100e-7, W.CFG4_WAVELENGTHS))], 3


for case in os.environ.get("CASES", "cfg2:f64:tiled,cfg2:f64:slots").split(","):
    workload, prec, layout = case.split(":")
    table = oa.OpticalTable()
    table.add_components((W.cfg2_components if workload == "cfg2" else W.cfg4_components)(oa))
    eng.upload(table.compile())
    batches, K = batches_of(workload, prec)
    n = batches[0].n
    outs = [SegmentBatch(n * K, prec, b.device, tiled=(layout == "tiled")) for b in batches]
    light = workload == "cfg2"
    rounds = int(os.environ.get("ROUNDS", 18)) if light else int(os.environ.get("ROUNDS4", 3))
    launches = int(os.environ.get("LAUNCHES", 50)) if light else int(os.environ.get("LAUNCHES4", 10))
    for s in range(int(os.environ.get("WARM", 400)) if light else 8):  # clocks up; every output holds its batch's records (resident planes)
        eng.trace(batches[s % len(batches)], K, out=outs[s % len(batches)], layout=layout)
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        eng.timing(True)
        for s in range(launches):
            out = outs[s % len(batches)]
            eng.trace(batches[s % len(batches)], K, out=out.forget_resident() if FORGET else out, layout=layout)
        torch.cuda.synchronize()
        ms, cnt = eng.timing_read()
        eng.timing(False)
        per.append(round(ms / cnt, 5))
    segs = int(outs[0].count.abs().sum().item())
    print(json.dumps({"label": label, "case": case, "pair": os.environ.get("PAIR", "default"), "whole_records": FORGET, "rays": n, "segments": segs,
                      "kernel": eng.last_launch()["kernel"], "ms_per_launch_by_round": per, "min": min(per), "median": float(np.median(per)),
                      "max": max(per)}), flush=True)
    del outs, batches
    torch.cuda.empty_cache()
