#!/usr/bin/env python3
"""Times of the Frechet distance from two pools' moment states at d = 512, 1024 and 2048:

  device   metrics.frechet_device on two PoolMoments (csrc/frechet.hip: covariances, two Newton-Schulz roots, traces; one 64-byte read-back)
  host     today's route: PoolMoments.state() twice (d + d^2 doubles each to the host), moments_mean_cov, metrics.frechet_from_moments
           (scipy.linalg.sqrtm of S_r S_f) -- a host clock around it, it ends on the host
  product  one cgs_f64_matmul against float64 torch.matmul on the same operands, HIP events around back-to-back launches

The pools are full-rank feature clouds (n = 4 d rows) as in tests/frechet_cases.py.  Medians over --rounds alternating rounds.
Every GPU step is a child process of its own under its own time limit; the first step that fails or runs out of time ends the run.

    python tools/frechet_timing.py [--rounds 5] [--limit 240] [--no-host]
"""
import argparse
import os
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [512, 1024, 2048]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
ap.add_argument("--no-host", action="store_true", help="skip the host route (sqrtm takes about a minute per call at d = 2048)")
ap.add_argument("--step", default=None, help="(internal) d of the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for d in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", str(d)] + (["--no-host"] if args.no_host else [])
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step d={d}: no result within {args.limit} s; stopping")
        if rc != 0:
            sys.exit(f"step d={d}: exit status {rc}; stopping")
    sys.exit(0)

import warnings

import numpy as np
import torch
import frechet_cases as FC
from cgs_amd import kernels as K
from cgs_amd.metrics import PoolMoments, frechet_device, frechet_from_moments, moments_mean_cov


def events(fn, n=20, warm=3):
    """us per call by HIP events around n back-to-back calls"""
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


d = int(args.step)
dev = torch.device("cuda:0")
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, d = {d}, n = {4 * d} per pool", flush=True)
pools = [PoolMoments(d, dev).update(torch.from_numpy(FC.cloud(90 + i, 4 * d, d)).to(dev)) for i in range(2)]


def host_route():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return frechet_from_moments(*moments_mean_cov(pools[0].state()), *moments_mean_cov(pools[1].state()))


rec = frechet_device(*pools, details=True)                      # warm-up: code objects, the workspace
td, th = [], []
for r in range(args.rounds):
    ms, fd = wall(lambda: frechet_device(*pools))
    td.append(ms)
    line = f"   round {r}: device {ms:9.2f} ms"
    if not args.no_host and (d < 2048 or r == 0):               # one host round at 2048
        ms, fh = wall(host_route)
        th.append(ms)
        line += f"   host route {ms:10.1f} ms   |device - host| / e_norm = {abs(fd - fh) / (rec['tr_r'] + rec['tr_f'] + rec['dmu2']):.2e}"
    print(line, flush=True)
a = torch.randn((d, d), dtype=torch.float64, device=dev)
b = torch.randn((d, d), dtype=torch.float64, device=dev)
o1, o2 = torch.empty_like(a), torch.empty_like(a)
ta, tb = [], []
for r in range(args.rounds):
    ta.append(events(lambda: K.f64_matmul(a, b, out=o1)))
    tb.append(events(lambda: torch.matmul(a, b, out=o2)))
flop = 2.0 * d ** 3
ma, mb = float(np.median(ta)), float(np.median(tb))
launches = 2 * (2 + 4 * FC.MAX_ITERS) + 7
print(f"d={d}: frechet_device median {np.median(td):.2f} ms (min {min(td):.2f}, max {max(td):.2f}; iterations {rec['iters_r']} / {rec['iters_m']}, status "
      f"{rec['status']}, {launches} launches queued)   host route " + (f"median {np.median(th):.1f} ms ({len(th)} runs)" if th else "not run")
      + f"   cgs_f64_matmul median {ma:.1f} us (min {min(ta):.1f}, max {max(ta):.1f}; {flop / (ma * 1e-6) / 1e12:.2f} TFLOP/s)   float64 torch.matmul median "
      f"{mb:.1f} us (min {min(tb):.1f}, max {max(tb):.1f}; {flop / (mb * 1e-6) / 1e12:.2f} TFLOP/s)", flush=True)
