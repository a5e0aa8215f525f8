#!/usr/bin/env python3
"""Wall time of scoring (sigmoid_and_saliency) and refining (the fused K-step loop) with 2-D discriminators of 64, 128 and 256 hidden units
(DESIGN.md section 11): 10 warm-up calls, then 200 timed calls between two device synchronisations.  K = 50, ladam, rate 0.05 is the
reference's 25-Gaussians command line; (64, 6) at K = 10 ties the table to the config-1 numbers.  For the wide rows the achieved fraction
of the fp32 matrix peak counts 2 B nh^2 FLOP per hidden->hidden layer and direction (the padded units and the VALU layers are not counted).

    python tools/refine2d_wide_timing.py
"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cgs_amd.synthetic import MLPDiscriminator

PEAK = 157.3e12          # fp32 matrix peak of the MI355X, FLOP/s

def timeit(fn, n=200):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6

def gemm_flop(B, nh, nl, evals):
    return evals * 2 * (nl - 2) * 2.0 * B * nh * nh

print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs")
for B in (1000, 10000):
    x = torch.from_numpy((1.5 * np.random.RandomState(B).randn(B, 2)).astype(np.float32)).to("cuda:0")
    for nh, nl, K in ((64, 6, 10), (64, 6, 50), (128, 6, 50), (256, 6, 50)):
        D = MLPDiscriminator.init(1, nhidden=nh, nlayers=nl)
        t_sal = timeit(lambda: D.sigmoid_and_saliency(x))
        t_ref = timeit(lambda: D.refine(x, 0.5, K, 0.05, "ladam"))
        line = f"B={B:5d} nh={nh:3d} nl={nl} K={K:2d}: sigmoid_and_saliency {t_sal:8.1f} us   refine {t_ref:9.1f} us"
        if nh > 64:
            line += (f"   fp32 matrix peak: {gemm_flop(B, nh, nl, 1) / (t_sal * 1e-6) / PEAK:6.1%} (saliency) "
                     f"{gemm_flop(B, nh, nl, K + 1) / (t_ref * 1e-6) / PEAK:6.1%} (refine)")
        print(line, flush=True)
