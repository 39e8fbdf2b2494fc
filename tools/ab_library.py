#!/usr/bin/env python3
"""One side of an A/B of two builds of the library on the trace kernels: cfg 3 and cfg 5 in fp32 (5e5 rays, append layout) and
cfg 2 (1e6 rays, fp64, tiled), library hipEvent time per launch, min / median / max over ROUNDS x 5 launches, with the number of
segments written (the same on both sides when the records are the same).  One process per build; a job alternates them:
    OT_LIB=<the other build's liboptable_hip.so> python tools/ab_library.py <label>      env: ROUNDS (12)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import optable_amd as oa
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch

if os.environ.get("OT_LIB"):
    abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
from optable_amd.engine import get_engine  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "this tree"
rounds = int(os.environ.get("ROUNDS", 12))
eng = get_engine()
Q = 1j * np.pi * W.W0**2 / W.WL
CASES = [("cfg3 fp32 append", W.cfg3_components, W.cfg3_rays(500_000, 2), "f32", 20, "append"),
         ("cfg5 fp32 append", W.cfg5_components, W.cfg5_rays(500_000, 3), "f32", 50, "append"),
         ("cfg2 fp64 tiled", W.cfg2_components, W.cfg2_rays(1_000_000, 0), "f64", 5, "tiled")]
for name, comps, (o, d), prec, cap, layout in CASES:
    table = oa.OpticalTable()
    table.add_components(comps(oa))
    eng.upload(table.compile())
    batch = RayBatch.from_arrays(o, d, wavelength=W.WL, q=Q, precision=prec)
    segs = eng.trace(batch, cap, layout=layout)  # warm
    nseg = int(segs.n_valid) if segs.count is None else int(segs.count.abs().sum().item())
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        eng.timing(True)
        for _ in range(5):
            segs = eng.trace(batch, cap, layout=layout)
        torch.cuda.synchronize()
        ms, launches = eng.timing_read()
        eng.timing(False)
        per.append(ms / 5)
    per = np.array(per)
    print(f"{label:10s} {name:18s} {nseg:9d} segments  ms per launch: min {per.min():.4f}  median {np.median(per):.4f}  max {per.max():.4f}"
          f"  (kernel {eng.last_launch()['kernel']})", flush=True)
    del segs, batch
