#!/usr/bin/env python3
"""Times of one update of the calibration and mode statistics (csrc/diagnostics.hip): 64, 10 000 and 50 000 scores
into a ``CalibrationStats`` and 10 000 samples x 25 modes into a ``ModeStats``, HIP events around back-to-back updates; and beside each the
host path it replaces -- the same device tensor copied to the host and put through the numpy state function -- by the wall clock.

Every GPU step is a child process of its own under its own time limit; the first step that fails or runs out of time ends the run.

    python tools/diagnostics_timing.py [--rounds 5] [--limit 120]
"""
import argparse
import os
import subprocess
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ["cal,64", "cal,10000", "cal,50000", "mode,10000"]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
ap.add_argument("--step", default=None, help="(internal) the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for step in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", step], timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no result within {args.limit} s; stopping")
        if rc != 0:
            sys.exit(f"step {step}: exit status {rc}; stopping")
    sys.exit(0)

import numpy as np
import torch
from cgs_amd import metrics as M


def events(fn, n=50, warm=5):
    """us per call by HIP events around n back-to-back calls"""
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def wall(fn, n=20, warm=3):
    """us per call by the wall clock (the host path ends on the host)"""
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): fn()
    return (time.perf_counter() - t0) * 1e6 / n


kind, n = args.step.split(",")
n = int(n)
dev = torch.device("cuda:0")
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, {kind}, n = {n}", flush=True)
g = torch.Generator().manual_seed(1)
if kind == "cal":
    p = torch.sigmoid(torch.randn(n, generator=g)).to(dev)
    cs = M.CalibrationStats(dev)
    ours = lambda: cs.update(p, 1)
    host = lambda: M.calibration_state_of(p.cpu().numpy(), 1)
else:
    side = np.linspace(-2.0, 2.0, 5)
    c = np.array([(a, b) for a in side for b in side])
    x = (torch.from_numpy(c[np.random.RandomState(1).randint(25, size=n)]).float() + 0.05 * torch.randn((n, 2), generator=g)).to(dev)
    ms = M.ModeStats(c, 0.2, dev)
    ours = lambda: ms.update(x)
    host = lambda: M.mode_state_of(x.cpu().numpy(), c, 0.2)
ta, tb = [], []
for r in range(args.rounds):
    ta.append(events(ours)); tb.append(wall(host))
    print(f"   round {r}: device update {ta[-1]:9.1f} us   copy to the host + numpy {tb[-1]:9.1f} us", flush=True)
print(f"{kind} n={n}: device update median {np.median(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f}; two launches, event-chained)   "
      f"copy + numpy median {np.median(tb):.1f} us (min {min(tb):.1f}, max {max(tb):.1f})", flush=True)
