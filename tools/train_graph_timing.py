#!/usr/bin/env python3
"""Same-process A/B of the image GAN's train iteration (training.GanTrainer.iteration) issued eagerly and replayed as a captured hipGraph
(``use_graph=True``), at the reference's batch 64 for mnist and dcgan64.

Two trainers on copies of one checkpoint; 10 warm-up iterations each (the graph trainer's first is its eager warm-up, its second captures), then
100 timed iterations each in alternating windows of 10, the device synchronised around every window.  The yardstick of the replayed form is the
eager form of the SAME process.  Launch counts: the C-ABI entry calls one eager iteration makes and the calls the captured program recorded (an
entry launches 1 to 3 kernels; the torch launches beside them are not counted).

Every net runs in a child process of its own under a time limit; the first child that fails ends the run.

    python tools/train_graph_timing.py [--nets mnist dcgan64] [--limit 300]
"""
import argparse
import collections
import copy
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, WARMUP, WINDOWS, PER_WINDOW = 64, 10, 10, 10


def child(arch):
    import torch
    from cgs_amd import lib as L
    from cgs_amd.nets import ARCHS, init_params
    from cgs_amd.training import GanTrainer
    dev = torch.device("cuda:0")
    A = ARCHS[arch]
    P = init_params(arch, dev)
    g = torch.Generator().manual_seed(1)
    z = (torch.rand((B, A["z_dim"]), generator=g) * 2 - 1).to(dev)
    real = torch.tanh(torch.randn((B,) + tuple(A["img"]), generator=g)).to(dev)

    def trainer(use_graph):
        return GanTrainer(arch, {k: v.clone() for k, v in P.items()}, B, dev, use_graph=use_graph)
    forms = {"eager": trainer(False), "graph": trainer(True)}
    for tr in forms.values():
        for _ in range(WARMUP):
            tr.iteration(real, z)
    torch.cuda.synchronize()
    if forms["graph"].path != "graph":
        print(f"{arch}: the capture was refused ({forms['graph'].graph_fallback}); nothing to compare", flush=True)
        return 1
    windows = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for name, tr in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(PER_WINDOW):
                tr.iteration(real, z)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / PER_WINDOW * 1e3)
    same = all(torch.equal(forms["eager"].P[k], forms["graph"].P[k]) for k in P if "moving_" not in k)
    ms = {k: sum(v) / len(v) for k, v in windows.items()}
    print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, {arch}, batch {B}, "
          f"{WINDOWS} alternating windows of {PER_WINDOW} iterations after {WARMUP} warm-ups")
    for k in forms:
        print(f"  {k:5s}: {ms[k]:7.3f} ms / iteration   (windows {min(windows[k]):.3f} .. {max(windows[k]):.3f})")
    print(f"  eager / graph = {ms['eager'] / ms['graph']:.2f}; variables bit-equal after {WARMUP + WINDOWS * PER_WINDOW} iterations each: {same}", flush=True)

    # ---- launch counts (after the timing: the counter costs host time)
    calls = collections.Counter()
    plain = L.call

    def counting(name, *args):
        calls[name] += 1
        return plain(name, *args)
    L.call = counting
    try:
        forms["eager"].iteration(real, z)
        eager_calls = copy.copy(calls)
        calls.clear()
        fresh = trainer(True)
        fresh.iteration(real, z)
        calls.clear()
        fresh.iteration(real, z)            # records the program (the replay itself makes no entry call)
        recorded = copy.copy(calls)
    finally:
        L.call = plain
    torch.cuda.synchronize()
    for what, c in (("one eager iteration", eager_calls), ("the recorded program", recorded)):
        adam = c["cgs_adam_step"] + c["cgs_adam_multi"]
        print(f"  entry calls of {what}: {sum(c.values())} (Adam {adam}, bn_moving_update {c['cgs_bn_moving_update']})")
    print("  a replayed iteration costs the host: 2 input copies, 2 lr_t fills, 1 graph launch, 2 loss clones", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["mnist", "dcgan64"])
    ap.add_argument("--limit", type=int, default=300, help="seconds a net's child process may take")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    for arch in a.nets:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", arch]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"{arch}: the child ended with status {rc}; nothing more is started")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
