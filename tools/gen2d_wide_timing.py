#!/usr/bin/env python3
"""Wall time of the wide 2-D generator's forward and of one calibrate / shape iteration at the reference's 25-Gaussians width (DESIGN.md
section 13): 10 warm-up calls, then N timed calls between two device synchronisations.

    python tools/gen2d_wide_timing.py
"""
import os
import sys
import time
import types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cgs_amd.synthetic import Gan, MLPDiscriminator, Refiner, WideGanTrainer, WideMLPGenerator
from cgs_amd.datasets import ToyDataset, NoiseDataset

def timeit(fn, n):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6

for nh in (128, 256):
    G = WideMLPGenerator.init(0, nh, 6)
    for B in (1000, 10000):
        z = torch.randn(B, 2, device="cuda:0")
        print(f"{nh} x 6, B={B}: forward(train) {timeit(lambda: G.generate(z), 200):.1f} us, "
              f"forward(infer) {timeit(lambda: G.generate(z, is_training=False), 200):.1f} us", flush=True)
np.random.seed(0)
data = ToyDataset("25Gaussians", scale=1.0)
D = MLPDiscriminator.init(1, 256, 6)
refiner = Refiner(types.SimpleNamespace(rollout_steps=50, rollout_rate=0.1, rollout_method="ladam"))
refiner.set_env(Gan(D), None, data)
tr = WideGanTrainer(WideMLPGenerator.init(0, 256, 6), D, data, NoiseDataset(), 1000, refiner=refiner)
print(f"one calibrate iteration at 256 x 6, B=1000 (host RNG + uploads + G fwd + D step): {timeit(lambda: tr.iteration('calibrate'), 200):.1f} us", flush=True)
print(f"one shape iteration at 256 x 6, B=1000, K=50 (+ real scores, the 50-step refiner, the step pick): {timeit(lambda: tr.iteration('shape'), 200):.1f} us", flush=True)
