#!/usr/bin/env python3
"""Wall time of the 2-D net's D step (DShaper.step / WideDShaper.step) at 64, 128 and 256 hidden units and of one whole shaping iteration
at 256 x 6: 10 warm-up calls, then 200 timed calls between two device synchronisations.  The shaping iteration is
shape_step with the reference's 25-Gaussians command line (K = 50, ladam, rate 0.05, batch 1000): refiner call + D step + the host work
between them.  The matrix work of a wide step is 3 (nl - 2) products of 2 B nh^2 FLOP: forward, adjoint, weight gradient.

    python tools/dstep_wide_timing.py
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o dstep -- python tools/dstep_wide_timing.py     # per-kernel times of passes A, B, C
"""
import os
import sys
import time
import types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cgs_amd.datasets import ToyDataset
from cgs_amd.synthetic import Gan, MLPDiscriminator, Refiner, d_shaper, shape_step

PEAK = 157.3e12          # fp32 matrix peak of the MI355X, FLOP/s

def timeit(fn, n=200):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6

print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs")
data = ToyDataset("25Gaussians", scale=1.0)
for B, nh, nl in ((1000, 64, 6), (1000, 128, 6), (1000, 256, 6), (10000, 256, 6)):
    rs = np.random.RandomState(B + nh)
    real = torch.from_numpy(data.next_batch(B).astype(np.float32)).to("cuda:0")
    fake = torch.from_numpy((1.5 * rs.randn(B, 2)).astype(np.float32)).to("cuda:0")
    sh = d_shaper(MLPDiscriminator.init(1, nhidden=nh, nlayers=nl), 1e-2)
    t = timeit(lambda: sh.step(real, fake))
    line = f"B={B:5d}+{B:<5d} nh={nh:3d} nl={nl}: {type(sh).__name__}.step {t:8.1f} us"
    if nh > 64:
        line += f"   fp32 matrix peak: {3 * (nl - 2) * 2.0 * (2 * B) * nh * nh / (t * 1e-6) / PEAK:6.1%}"
    print(line, flush=True)

D = MLPDiscriminator.init(1, nhidden=256, nlayers=6)
sh = d_shaper(D, 1e-2)
ref = Refiner(types.SimpleNamespace(rollout_steps=50, rollout_rate=0.05, rollout_method="ladam"))
ref.set_env(Gan(D), None, data)
noise = (1.5 * np.random.RandomState(3).randn(1000, 2)).astype(np.float32)
real = data.next_batch(1000)
t_it = timeit(lambda: shape_step(ref, sh, noise, real))
t_ref = timeit(lambda: ref.manipulate_sample(noise, 'probabilistic'))
print(f"shaping iteration (shape_step, 256 x 6, batch 1000, K = 50, ladam 0.05): {t_it / 1e3:7.2f} ms, of which manipulate_sample {t_ref / 1e3:7.2f} ms", flush=True)
