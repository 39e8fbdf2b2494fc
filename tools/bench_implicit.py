#!/usr/bin/env python3
"""Cost of user-defined implicit surfaces (OT_SHAPE_IMPLICIT_CHEB, optable_amd/implicit.py) on the device: 1e6 rays, fp64 and
fp32, library hipEvent time, on three one-mirror scenes —
    sphere    the built-in Sphere cap (closed-form search)
    isphere   the same cap as a user's implicit surface |P|^2 - R^2 (a (2,2,2) series, scan + polish)
    torus     a toroidal mirror section (a (4,4,4) series)
each behind a plane mirror that sends every ray back through it once (two hits per ray, cap 4).
    python tools/bench_implicit.py [n_rays]      env: ONLY=f32|f64, OT_LIB"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import implicit_scenes
import optable_amd as oa
from optable_amd import abi
from optable_amd import workloads as W
from optable_amd.batch import RayBatch
from optable_amd.engine import get_engine

if os.environ.get("OT_LIB"):
    abi.LIB_PATH = os.path.abspath(os.environ["OT_LIB"])
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
K = 4
eng = get_engine()
U = implicit_scenes.implicit_surface_classes(oa)
R = 20.0
SURFACES = {
    "sphere": lambda: oa.Sphere(R, 0.2),
    "isphere": lambda: U["ImplicitSphere"](R, 0.2),
    "torus": lambda: U["Torus"](10.0, 4.0, 1.5),
}


def scene(name):
    surf = SURFACES[name]()
    # the sphere caps sit at local x in [R - h, R]: put their vertex where the torus vertex is
    origin = [8 + R, 0, 0] if name != "torus" else [8, 0, 0]
    mirror = U["CurvedMirror"](origin, surf, reflectivity=1.0).RotZ(np.pi)
    t = oa.OpticalTable()
    t.implicit_surfaces = True
    t.add_components([oa.Mirror([0, 0, 0], radius=4.0).RotZ(0.0), mirror])
    return t


rng = np.random.default_rng(11)
o = np.stack([np.full(n, 1.0), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)], 1)
d = np.stack([np.ones(n), rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n)], 1)
for prec in ("f64", "f32"):
    if os.environ.get("ONLY") and os.environ["ONLY"] != prec:
        continue
    batch = RayBatch.from_arrays(o, d, wavelength=W.WL, q=1j * np.pi * W.W0**2 / W.WL, precision=prec)
    for name in SURFACES:
        table = scene(name)
        sc = table.compile()
        best = None
        for rep in range(4):  # the first is warm-up (scratch, code objects)
            torch.cuda.synchronize()
            eng.timing(True)
            t0 = time.perf_counter()
            segs = table.trace_batch(batch, max_segments=K, scene=sc)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ms, launches = eng.timing_read()
            eng.timing(False)
            if rep:
                best = ms if best is None else min(best, ms)
        nseg = int(segs.n_valid) if segs.count is None else int(segs.count.abs().sum().item())
        print(f"{prec} {name}: {n} rays -> {nseg} segments; device best of 3 {best:.3f} ms ({launches} timed regions), "
              f"wall {wall:.1f} ms; launch {eng.last_launch()}", flush=True)
        del segs
