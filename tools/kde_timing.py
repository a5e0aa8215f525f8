#!/usr/bin/env python3
"""Times of one update of a density map (csrc/kde2d.hip): 64, 10 000 and 50 000 samples into a ``DensityMap`` on the
reference's 100 x 100 grid and 10 000 samples on 256 x 256, HIP events around back-to-back updates; and beside each the host path it
replaces -- scipy.stats.gaussian_kde with the reference's bandwidth on the same pool and grid -- by the wall clock (one evaluation: it
takes seconds).

Every GPU step is a child process of its own under its own time limit; the first step that fails or runs out of time ends the run.

    python tools/kde_timing.py [--rounds 5] [--limit 180] [--no-scipy]
"""
import argparse
import os
import subprocess
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ["64,100", "10000,100", "50000,100", "10000,256"]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=180, help="seconds per GPU step")
ap.add_argument("--no-scipy", action="store_true", help="leave the host column out")
ap.add_argument("--step", default=None, help="(internal) the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", step] + (["--no-scipy"] if args.no_scipy else [])
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
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


n, nbins = (int(v) for v in args.step.split(","))
dev = torch.device("cuda:0")
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, n = {n}, grid {nbins} x {nbins}", flush=True)
rs = np.random.RandomState(1)
side = np.array([-2.0, 0.0, 2.0])
c = np.array([(a, b) for a in side for b in side])
x = (c[rs.randint(9, size=n)] + 0.05 * rs.randn(n, 2)).astype(np.float32)          # nine tight modes, scale 4
axis = M.kde_axes(4.0, nbins)
whiten, norm = M.kde_whiten(np.cov(x.astype(np.float64), rowvar=False), n)
xd = torch.from_numpy(x).to(dev)
dm = M.DensityMap(axis, axis, whiten, dev)
ta = []
for r in range(args.rounds):
    ta.append(events(lambda: dm.update(xd)))
    print(f"   round {r}: device update {ta[-1]:9.1f} us", flush=True)
line = f"n={n} grid={nbins}x{nbins}: device update median {np.median(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f}; two launches, event-chained)"
if not args.no_scipy:
    from scipy.stats import gaussian_kde
    x64 = x.astype(np.float64)
    t0 = time.perf_counter()
    k = gaussian_kde([x64[:, 0], x64[:, 1]])
    k.set_bandwidth(bw_method=k.factor / 2.)
    xi, yi = np.mgrid[-4.0:4.0:nbins * 1j, -4.0:4.0:nbins * 1j]
    want = k(np.vstack([xi.flatten(), yi.flatten()])).reshape(xi.shape)
    t1 = time.perf_counter()
    got = M.DensityMap(axis, axis, whiten, dev).update(xd).values(norm)
    line += f"   scipy gaussian_kde {t1 - t0:.3f} s (one evaluation, wall clock)   worst |delta| / max = {np.abs(got - want).max() / want.max():.3g}"
print(line, flush=True)
