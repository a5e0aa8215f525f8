#!/usr/bin/env python3
"""Times of the rejection-sampling kernels (csrc/drs.hip): one ``decide`` at 64, 2048 (32 batches of 64) and 10 000
scores, one ``compact`` of 2048 x 784 and 1024 x 12 288 floats with every second row accepted, HIP events around back-to-back calls;
and beside each the host route it replaces by the wall clock -- copy the scores (and the rows) to the host, ``Rejector.sampling`` per
batch (index the rows with the mask).

Every GPU step is a child process of its own under its own time limit; the first step that fails or runs out of time ends the run.

    python tools/drs_timing.py [--rounds 5] [--limit 120]
"""
import argparse
import os
import subprocess
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ["decide,64,1", "decide,64,32", "decide,10000,1", "compact,2048,784", "compact,1024,12288"]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
ap.add_argument("--step", default=None, help="(internal) the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", step]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no result within {args.limit} s; stopping")
        if rc != 0:
            sys.exit(f"step {step}: exit status {rc}; stopping")
    sys.exit(0)

import numpy as np
import torch
from cgs_amd import kernels as K
from cgs_amd.sampling import Rejector


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
    """us per call by the wall clock (the host route ends in a synchronising copy)"""
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): fn()
    return (time.perf_counter() - t0) * 1e6 / n


what, a, b = args.step.split(",")
a, b = int(a), int(b)
dev = torch.device("cuda:0")
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, {args.step}", flush=True)
rs = np.random.RandomState(1)
td, th = [], []
if what == "decide":
    batch, groups = a, b
    n = batch * groups
    sig = torch.from_numpy(rs.uniform(0.01, 0.99, (n, 1)).astype(np.float32)).to(dev)
    u = torch.from_numpy(rs.rand(n)).to(dev)
    state = torch.zeros(1, dtype=torch.float64, device=dev)
    rows = np.arange(n)

    def host():
        s = sig.cpu().numpy()
        r = Rejector()
        return [r.sampling(rows[g * batch:(g + 1) * batch], s[g * batch:(g + 1) * batch], shift_percent=100.0) for g in range(groups)]
    for q, tag in ((100.0, "q=100"), (60.0, "q=60 (radix select)")):
        td = [events(lambda: K.drs_decide(sig, u, state, groups, q)) for _ in range(args.rounds)]
        print(f"decide {groups} x {batch}, {tag}: device median {np.median(td):.1f} us (min {min(td):.1f}, max {max(td):.1f}; two launches and four "
              f"small allocations per call)", flush=True)
    th = [wall(host) for _ in range(args.rounds)]
    print(f"decide {groups} x {batch}: host route (scores to the host, Rejector.sampling per batch) median {np.median(th):.1f} us", flush=True)
else:
    n, row = a, b
    src = torch.from_numpy(rs.randn(n, row).astype(np.float32)).to(dev)
    mask_h = (np.arange(n) % 2).astype(np.uint8)
    mask = torch.from_numpy(mask_h).to(dev)
    dst = torch.empty((n, row), dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    pinned = torch.empty((n, row), dtype=torch.float32).pin_memory()

    def host():
        pinned.copy_(src)                                             # every row crosses, the rejected ones too
        return pinned.numpy()[mask_h.astype(bool)]
    td = [events(lambda: K.compact_rows(src, mask, dst, 0, total=total)) for _ in range(args.rounds)]
    th = [wall(host) for _ in range(args.rounds)]
    moved = 2 * (n // 2) * row * 4
    print(f"compact {n} x {row}, half accepted: device median {np.median(td):.1f} us (min {min(td):.1f}, max {max(td):.1f}) = "
          f"{moved / np.median(td) / 1e3:.0f} GB/s read + written; host route (rows to pinned memory, index) median {np.median(th):.1f} us", flush=True)
