#!/usr/bin/env python3
"""Wall time of the wide 2-D generator's G step (WideGStep.step) at 128 x 6 and 256 x 6 and of one whole train iteration at the
reference's 25-Gaussians widths: 10 warm-up calls, then 200 timed calls between two device synchronisations.
The forward alone (WideMLPGenerator.generate, training mode) is timed beside the step, which contains it.  The matrix work of a step
is 3 (nl - 2) products of 2 B nh^2 FLOP: forward, adjoint, weight gradient.

    python tools/gstep_wide_timing.py
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o gstep -- python tools/gstep_wide_timing.py     # per-kernel times
"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cgs_amd.datasets import NoiseDataset, ToyDataset
from cgs_amd.synthetic import Gan2DTrainer, MLPDiscriminator, WideMLPGenerator, g_stepper

PEAK = 157.3e12          # fp32 matrix peak of the MI355X, FLOP/s

def timeit(fn, n=200):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6

print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs")
for nh in (128, 256):
    for B in (1000, 10000):
        G = WideMLPGenerator.init(0, nh, 6)
        step = g_stepper(G, 5e-3)
        rs = np.random.RandomState(B + nh)
        z = torch.from_numpy(rs.randn(B, 2).astype(np.float32)).to("cuda:0")
        gp = torch.from_numpy((1e-3 * rs.randn(B, 2)).astype(np.float32)).to("cuda:0")
        t_f = timeit(lambda: G.generate(z))
        t = timeit(lambda: step.step(z, gp))
        print(f"B={B:5d} nh={nh:3d} nl=6: {type(step).__name__}.step {t:8.1f} us (forward alone {t_f:7.1f} us)"
              f"   fp32 matrix peak: {3 * 4 * 2.0 * B * nh * nh / (t * 1e-6) / PEAK:6.1%}", flush=True)

np.random.seed(0)
data = ToyDataset("25Gaussians", scale=1.0)
tr = Gan2DTrainer(WideMLPGenerator.init(0, 256, 6), MLPDiscriminator.init(1, 256, 6), data, NoiseDataset(), 1000)
print(f"one train iteration at 256 x 6, B=1000 (host RNG + uploads + G fwd + D step + G fwd + saliency + G step): "
      f"{timeit(lambda: tr.iteration('train')):.1f} us", flush=True)
