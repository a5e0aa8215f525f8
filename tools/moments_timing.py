#!/usr/bin/env python3
"""Times of the pool-moments accumulation (cgs_pool_moments_accumulate, csrc/moments.hip) at
(m = 32768, d = 512) and (m = 8192, d = 2048), and beside each the yardstick: torch.matmul of the same product A^T A on float64
device tensors (the conversion and the shift subtraction NOT included: the yardstick starts from a ready float64 matrix).
HIP events around back-to-back launches, several rounds, the two alternating.

Every GPU step is a child process of its own under its own time limit; the first step that fails or runs out of time ends the run.

    python tools/moments_timing.py [--rounds 5] [--limit 120]
"""
import argparse
import os
import subprocess
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32768, 512), (8192, 2048)]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
ap.add_argument("--step", default=None, help="(internal) m,d of the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for m, d in SHAPES:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", f"{m},{d}"],
                                timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step m={m} d={d}: no result within {args.limit} s; stopping")
        if rc != 0:
            sys.exit(f"step m={m} d={d}: exit status {rc}; stopping")
    sys.exit(0)

import numpy as np
import torch
from cgs_amd import kernels as K


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


m, d = (int(v) for v in args.step.split(","))
dev = torch.device("cuda:0")
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, m = {m}, d = {d}", flush=True)
g = torch.Generator().manual_seed(1)
x = (100.0 + torch.randn((m, d), generator=g)).to(dev)
shift = x.mean(0).contiguous()
s, gram = torch.zeros(d, dtype=torch.float64, device=dev), torch.zeros((d, d), dtype=torch.float64, device=dev)
a64 = x.double() - shift.double()
out = torch.empty((d, d), dtype=torch.float64, device=dev)
ours = lambda: K.pool_moments(x, s, gram, shift=shift)
yard = lambda: torch.matmul(a64.t(), a64, out=out)
ta, tb = [], []
for r in range(args.rounds):
    ta.append(events(ours)); tb.append(events(yard))
    print(f"   round {r}: pool_moments {ta[-1]:9.1f} us   float64 matmul {tb[-1]:9.1f} us", flush=True)
flop = 2.0 * m * d * d
ma, mb = float(np.median(ta)), float(np.median(tb))
print(f"m={m} d={d}: pool_moments median {ma:.1f} us (min {min(ta):.1f}, max {max(ta):.1f}; {flop / 2 / (ma * 1e-6) / 1e12:.2f} TFLOP/s on the "
      f"upper triangle it computes, {flop / (ma * 1e-6) / 1e12:.2f} counted as the full product)   float64 matmul median {mb:.1f} us "
      f"(min {min(tb):.1f}, max {max(tb):.1f}; {flop / (mb * 1e-6) / 1e12:.2f} TFLOP/s)   pool_moments / matmul = {ma / mb:.2f}", flush=True)
