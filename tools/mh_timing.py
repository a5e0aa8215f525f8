#!/usr/bin/env python3
"""Times of the Metropolis-Hastings chain kernels (csrc/mh.hip): one ``walk`` of 64, 2048 (32 batches of 64), 10 000
and 50 000 scores at T = 20 (uniform scores; the 50 000 also constant, where every proposal moves: the longest serial path), one
``gather`` of 2048 x 784 and 1024 x 12 288 floats from a list with repeats, HIP events around back-to-back calls; beside each the host
route it replaces by the wall clock -- copy the scores (and the rows) to the host, ``IndependenceSampler.walk`` per batch, index the rows,
upload the result; and ``fill``: ``evaluate.hastings_fill_fused`` against ``evaluate.collaborate_fused`` on the MNIST net (batch 64,
G = 32, K = 50 refinement steps, T = 20, 5 000 samples), wall time, host-chain seconds and device-wait seconds of each.

Every GPU step is a child process of its own under its own time limit; the first step that fails or runs out of time ends the run.

    python tools/mh_timing.py [--rounds 5] [--limit 120] [--steps walk,64,1 ...]
"""
import argparse
import os
import subprocess
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ["walk,64,1", "walk,64,32", "walk,10000,1", "walk,50000,1", "gather,2048,784", "gather,1024,12288", "fill,5000,32"]
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
ap.add_argument("--steps", nargs="*", default=STEPS)
ap.add_argument("--step", default=None, help="(internal) the one step this process runs")
args = ap.parse_args()

if args.step is None:
    for step in args.steps:
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
from cgs_amd.sampling import DeviceIndependenceSampler, IndependenceSampler


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
T = 20
if what == "walk":
    batch, groups = a, b
    n = batch * groups
    kinds = [("uniform", rs.uniform(0.01, 0.99, (n, 1)).astype(np.float32))]
    if batch >= 50000:
        kinds.append(("constant: every proposal moves", np.full((n, 1), 0.37, dtype=np.float32)))
    u_h = rs.uniform(0, 1, n)
    u = torch.from_numpy(u_h).to(dev)
    for tag, sig_h in kinds:
        sig = torch.from_numpy(sig_h).to(dev)
        src = torch.from_numpy(rs.randn(n, 2).astype(np.float32)).to(dev)
        state = torch.tensor([0.5, 1.0], dtype=torch.float64, device=dev)

        def device():
            state[0] = 0.5                                            # every call walks from the same state
            return K.mh_walk(sig, u, state, T, 0, groups)

        def host():
            s = sig.cpu().numpy()
            x = src.cpu().numpy()
            h = IndependenceSampler(T=T)
            h.set_score_curr(0.5)
            out = [x[g * batch:(g + 1) * batch][h.walk(s[g * batch:(g + 1) * batch].copy(), u_h[g * batch:(g + 1) * batch])] for g in range(groups)]
            return torch.from_numpy(np.concatenate(out)).to(dev)
        few = 10 if n >= 10000 else 50
        td = [events(device, n=few) for _ in range(args.rounds)]
        rows, counts, span = device()
        listed = rows.cpu().numpy()[:int(span.cpu()[1])]
        th = [wall(host, n=5 if n >= 10000 else 20) for _ in range(args.rounds)]
        print(f"walk {groups} x {batch}, T = {T}, {tag}: device median {np.median(td):.1f} us (min {min(td):.1f}, max {max(td):.1f}; one launch, one state "
              f"write and three small allocations per call; {len(listed)} rows emitted, {len(np.unique(listed))} distinct); host route (scores and 2-float rows to "
              f"the host, IndependenceSampler.walk per batch, index, upload) median {np.median(th):.1f} us", flush=True)
elif what == "gather":
    n, row = a, b
    src = torch.from_numpy(rs.randn(n, row).astype(np.float32)).to(dev)
    picks_h = np.sort(rs.randint(n, size=n // 2)).astype(np.int32)     # half as many rows as the source holds, with repeats, in chain order
    picks = torch.from_numpy(picks_h).to(dev)
    span = torch.tensor([0, n // 2], dtype=torch.int64, device=dev)
    dst = torch.empty((n, row), dtype=torch.float32, device=dev)
    pinned = torch.empty((n, row), dtype=torch.float32).pin_memory()

    def host():
        pinned.copy_(src)                                             # every row crosses, the ones never emitted too
        return torch.from_numpy(pinned.numpy()[picks_h]).to(dev)
    td = [events(lambda: K.gather_rows(src, picks, span, dst)) for _ in range(args.rounds)]
    th = [wall(host) for _ in range(args.rounds)]
    moved = 2 * (n // 2) * row * 4
    print(f"gather {n} x {row}, {n // 2} rows listed: device median {np.median(td):.1f} us (min {min(td):.1f}, max {max(td):.1f}) = "
          f"{moved / np.median(td) / 1e3:.0f} GB/s read + written; host route (rows to pinned memory, index, upload) median {np.median(th):.1f} us", flush=True)
else:
    from cgs_amd.evaluate import MIN_EFFICIENCY, FusedProposer, collaborate_fused, hastings_fill_fused
    from cgs_amd.model import GAN
    from cgs_amd.nets import init_params
    eval_size, G = a, b
    gan = GAN("mnist", batch_size=64, device=dev, params=init_params("mnist", dev, 2019))
    prop = FusedProposer(gan, 50, 0.1, batch=64, groups=G, depth=2)
    for r in range(args.rounds):
        for name in ("collaborate_fused", "hastings_fill_fused"):
            stats = {}
            np.random.seed(7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "collaborate_fused":
                out, eff = collaborate_fused(prop, IndependenceSampler(T=T), eval_size, np.float32(0.5), min_efficiency=MIN_EFFICIENCY, stats=stats)
            else:
                out, eff = hastings_fill_fused(prop, DeviceIndependenceSampler(T=T, device=dev), eval_size, np.float32(0.5), min_efficiency=MIN_EFFICIENCY,
                                               stats=stats)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"fill {eval_size} of 64 x {G} per round, round {r}: {name} wall {dt:.3f} s, proposed {stats['proposed']}, eff {eff:.4f}, host_chain_s "
                  f"{stats['host_chain_s']:.4f}, device_wait_s {stats['device_wait_s']:.4f}", flush=True)
