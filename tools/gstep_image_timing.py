#!/usr/bin/env python3
"""Wall time of the image GAN's generator step (training.GStepper.step) and of one whole train iteration (training.GanTrainer.iteration)
at the reference's batch 64, for mnist and dcgan64: 10 warm-up calls, then 100 timed calls between two device
synchronisations.  The D step (shaping.DShaper.step) is timed beside them for scale, and the weight gradient of every transposed
convolution of G on its own (kernels.deconv2d_bwd_weight), the last layer's Cout = 1 / 3 launch among them.

    python tools/gstep_image_timing.py
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o gstep -- python tools/gstep_image_timing.py     # per-kernel times
"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cgs_amd import kernels as K
from cgs_amd.engine import _Deconv
from cgs_amd.nets import ARCHS, init_params
from cgs_amd.training import GanTrainer

def timeit(fn, n=100):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e6

dev = torch.device("cuda:0")
B = 64
print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, batch {B}")
for arch in ("mnist", "dcgan64"):
    A = ARCHS[arch]
    P = init_params(arch, dev)
    tr = GanTrainer(arch, P, B, dev)
    g = torch.Generator().manual_seed(1)
    z = (torch.rand((B, A["z_dim"]), generator=g) * 2 - 1).to(dev)
    real = torch.tanh(torch.randn((B,) + tuple(A["img"]), generator=g)).to(dev)
    fake = tr.gstepper.forward(z).clone()
    t_fwd = timeit(lambda: tr.gstepper.forward(z))
    t_g = timeit(lambda: tr.gstepper.step(z))
    t_d = timeit(lambda: tr.dshaper.step(real, fake))
    t_it = timeit(lambda: tr.iteration(real, z))
    print(f"{arch:8s}: G step {t_g / 1e3:7.3f} ms (its training-mode forward alone {t_fwd / 1e3:6.3f} ms)   D step {t_d / 1e3:6.3f} ms   "
          f"iteration {t_it / 1e3:7.3f} ms", flush=True)
    for idx, st in enumerate(tr.gstepper.g.stages):
        if isinstance(st, _Deconv):
            x, dy = tr.gstepper.x_in[idx], torch.randn_like(st.out)
            kh, kw, Cout, Cin = st.w.shape
            t_w = timeit(lambda: K.deconv2d_bwd_weight(x, dy, kh, kw, st.s, st.s, out=st.g_w))
            flop = 2.0 * x.shape[0] * x.shape[1] * x.shape[2] * Cin * kh * kw * Cout
            print(f"          deconv wgrad {tuple(x.shape[1:])} -> {tuple(st.out.shape[1:])} k={kh}: {t_w:7.1f} us  ({flop / (t_w * 1e-6) / 1e12:5.2f} TFLOP/s)", flush=True)
