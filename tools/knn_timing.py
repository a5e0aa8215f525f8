#!/usr/bin/env python3
"""Times of the nearest-neighbour ops and of the manifold metrics (csrc/knn.hip) on two pools of n rows each at
n x d = 10 000 x 2, 10 000 x 512 and 50 000 x 512:

  nn_min / knn_radii (k = 5, a pool against itself) / ball_count    HIP events around back-to-back launches
  manifold_metrics (k = 5)                                          a host clock around the call: five launches, four sums, one read-back
  host                                                              metrics.manifold_metrics_host, the float64 numpy restatement, at 10 000 x 2
                                                                    (and at 10 000 x 512 with --host-512: minutes of host time)

The pools are seeded Gaussians.  Medians over --rounds rounds.  Every GPU step is a child process of its own under its own time limit;
the first step that fails or runs out of time ends the run.

    python tools/knn_timing.py [--rounds 5] [--limit 240] [--no-host] [--host-512]
"""
import argparse
import os
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ["10000x2", "10000x512", "50000x512"]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
ap.add_argument("--host-512", action="store_true", help="run the host restatement at 10 000 x 512 too")
ap.add_argument("--step", default=None, help="(internal) n x d of the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for size in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", size]
        cmd += (["--no-host"] if args.no_host else []) + (["--host-512"] if args.host_512 else [])
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step {size}: no result within {args.limit} s; stopping")
        if rc != 0:
            sys.exit(f"step {size}: exit status {rc}; stopping")
    sys.exit(0)

import numpy as np
import torch
from cgs_amd import knn
from cgs_amd.metrics import manifold_metrics, manifold_metrics_host


def events(fn, n, warm=2):
    """ms per call by HIP events around n back-to-back calls"""
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


n, d = (int(v) for v in args.step.split("x"))
k = 5
dev = torch.device("cuda:0")
plan = knn.plan(n, n, d)
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, two pools of {n} x {d}, k = {k}, plan {plan}", flush=True)
rs = np.random.RandomState(2019)
real_h, fake_h = rs.randn(n, d).astype(np.float32), (rs.randn(n, d) * 1.1 + 0.1).astype(np.float32)
real, fake = torch.from_numpy(real_h).to(dev), torch.from_numpy(fake_h).to(dev)
r2 = knn.knn_radii(real, k)
reps = 20 if n * d <= 20000 else 5 if n <= 10000 else 2
ops = {"nn_min": lambda: knn.nn_min(real, fake), "knn_radii": lambda: knn.knn_radii(real, k), "ball_count": lambda: knn.ball_count(fake, real, r2)}
times = {name: [] for name in ops}
tm = []
for r in range(args.rounds):
    for name, fn in ops.items():
        times[name].append(events(fn, reps))
    ms, got = wall(lambda: manifold_metrics(real, fake, k=k))
    tm.append(ms)
    print(f"   round {r}: " + "   ".join(f"{name} {times[name][-1]:9.3f} ms" for name in ops) + f"   manifold_metrics {ms:9.3f} ms", flush=True)
pairs = float(n) * n
line = f"{n}x{d}: " + "   ".join(f"{name} median {np.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f}; {pairs * d / (np.median(t) * 1e-3) / 1e12:.2f} T coordinate "
                                 f"pairs/s)" for name, t in times.items())
line += f"   manifold_metrics median {np.median(tm):.3f} ms (min {min(tm):.3f}, max {max(tm):.3f})   {got}"
if not args.no_host and (d <= 2 or (args.host_512 and n <= 10000)):
    t0 = time.perf_counter()
    host = manifold_metrics_host(real_h, fake_h, k)
    th = (time.perf_counter() - t0) * 1e3
    line += f"   host restatement {th:.0f} ms (one run), equal to the device's: {host == got}"
else:
    line += "   host restatement not run"
print(line, flush=True)
