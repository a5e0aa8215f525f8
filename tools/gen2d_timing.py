#!/usr/bin/env python3
"""Wall time of the 2-D generator's calls and of one train iteration: 10 warm-up calls, then N timed calls between two
device synchronisations.  Default G (nhidden 64, nlayers 6).

    python tools/gen2d_timing.py
"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cgs_amd.synthetic import MLPGenerator, MLPDiscriminator, GStep, GanTrainer
from cgs_amd.datasets import ToyDataset, NoiseDataset

def timeit(fn, n):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6

G = MLPGenerator.init(0)
for B in (1000, 10000):
    z = torch.randn(B, 2, device="cuda:0")
    gp = 1e-3 * torch.randn(B, 2, device="cuda:0")
    st = GStep(G)
    print(f"B={B}: forward(train) {timeit(lambda: G.generate(z), 200):.1f} us, forward(infer) {timeit(lambda: G.generate(z, is_training=False), 200):.1f} us, "
          f"g_step {timeit(lambda: st.grads(z, gp), 200):.1f} us", flush=True)
np.random.seed(0)
tr = GanTrainer(MLPGenerator.init(0), MLPDiscriminator.init(1), ToyDataset("Imbal-8Gaussians", 10.0, 0.9), NoiseDataset(), 1000)
print(f"one train iteration at B=1000 (host RNG + uploads + D step + G fwd + saliency + G step): {timeit(lambda: tr.iteration('train'), 300):.1f} us", flush=True)
