#!/usr/bin/env python3
"""Times of the D step on the PatchGAN of BASELINE config 5 (cyclegan256, batch 8), one process:

  1. shaping.DShaper.step, and one shaping.shape_step at K = 20 next to the refinement call alone: 5 warm-up calls, then timed calls
     between two device synchronisations;
  2. every layer's weight-gradient launch on its own, by HIP events around a batch of launches;
  3. an alternating A/B on d_c5's shape (x [8,32,32,512], dy [8,32,32,1], 4x4, stride 1): the one-output-channel entry
     (cgs_conv2d_nhwc_bwd_weight_cout1) against the generic GEMM entry (cgs_conv2d_nhwc_bwd_weight), several rounds each, the rounds
     interleaved, with the largest difference of the two results.

    python tools/dstep_patchgan_timing.py [--batch 8] [--steps 20] [--rounds 5]
"""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cgs_amd import kernels as K
from cgs_amd.engine import RefineEngine, _Conv
from cgs_amd.nets import ARCHS, init_params
from cgs_amd.shaping import DShaper, shape_step

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="cyclegan256")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()


def timeit(fn, n, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6


def events(fn, n=50, warm=5):
    """us per launch by HIP events around n back-to-back launches"""
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


dev = torch.device("cuda:0")
arch, B = args.arch, args.batch
A = ARCHS[arch]
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, {arch} batch {B}", flush=True)
P = init_params(arch, dev)
g = torch.Generator().manual_seed(1)
src = (torch.rand((B,) + tuple(A["g_in"]), generator=g) * 2 - 1).to(dev)
real = torch.tanh(torch.randn((B,) + tuple(A["img"]), generator=g)).to(dev)
eng = RefineEngine(arch, P, B, dev)
sh = DShaper(arch, P, B, dev, learning_rate=1e-5)
idx = np.random.RandomState(0).randint(args.steps + 1, size=B)
fake = eng.refine_from_z(src, args.steps, 0.1, mode="probabilistic", indices=idx)[0].clone()

# 1. the step, and a shaping iteration next to its refinement call
t_d = timeit(lambda: sh.step(real, fake), 30)
t_ref = timeit(lambda: eng.refine_from_z(src, args.steps, 0.1, mode="probabilistic", indices=idx), 5, warm=2)
t_it = timeit(lambda: shape_step(eng, sh, src, real, args.steps, 0.1, indices=idx), 5, warm=2)
print(f"DShaper.step {t_d / 1e3:7.3f} ms   refine K={args.steps} {t_ref / 1e3:8.3f} ms ({B / (t_ref * 1e-6):6.1f} samples/s)   "
      f"shape_step {t_it / 1e3:8.3f} ms ({B / (t_it * 1e-6):6.1f} samples/s)", flush=True)

# 2. every layer's weight-gradient launch
sh.loss_and_grads(real, fake)
for st in sh.tape.stages:
    if isinstance(st, _Conv):
        x, dy = st.x_in, torch.randn_like(st.out)
        kh, kw, Cin, Cout = st.w.shape
        fn = ((lambda: K.conv2d_bwd_weight_cout1(x, dy, kh, kw, st.s, st.s, out=st.g_w)) if st.wgrad_cout1
              else (lambda: K.conv2d_bwd_weight(x, dy, kh, kw, st.s, st.s, out=st.g_w)))
        t_w = events(fn)
        flop = 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * Cout * kh * kw * Cin
        print(f"   conv wgrad {tuple(x.shape[1:])} -> {tuple(st.out.shape[1:])} k={kh} s={st.s} [{'cout1' if st.wgrad_cout1 else 'generic'}]: "
              f"{t_w:8.1f} us  {flop / (t_w * 1e-6) / 1e12:6.2f} TFLOP/s  x {x.numel() * 4 / (t_w * 1e-6) / 1e12:5.2f} TB/s", flush=True)

# 3. the A/B on the logit head's shape
head = sh.tape.stages[-1]
x, dy = head.x_in, torch.randn_like(head.out)
kh, kw, Cin, Cout = head.w.shape
if Cout == 1 and K.conv_wgrad_cout1_ok(tuple(x.shape), kh, kw, head.s, head.s):
    ga, gb = torch.empty_like(head.w), torch.empty_like(head.w)
    new = lambda: K.conv2d_bwd_weight_cout1(x, dy, kh, kw, head.s, head.s, out=ga)
    old = lambda: K.conv2d_bwd_weight(x, dy, kh, kw, head.s, head.s, out=gb)
    ta, tb = [], []
    for r in range(args.rounds):
        ta.append(events(new)); tb.append(events(old))
        print(f"   A/B round {r}: cout1 {ta[-1]:8.1f} us   generic {tb[-1]:8.1f} us", flush=True)
    diff = float((ga - gb).abs().max()) / float(gb.abs().max())
    xb = x.numel() * 4
    print(f"A/B {tuple(x.shape)} k={kh} s={head.s}: cout1 median {np.median(ta):.1f} us (min {min(ta):.1f}, max {max(ta):.1f}; x at "
          f"{xb / (np.median(ta) * 1e-6) / 1e12:.2f} TB/s)   generic median {np.median(tb):.1f} us (min {min(tb):.1f}, max {max(tb):.1f})   "
          f"ratio {np.median(tb) / np.median(ta):.2f}   max|cout1 - generic| / max|generic| = {diff:.2e}", flush=True)
