#!/usr/bin/env python3
"""Generate tests/golden/g11_pairwise_distance.npz by RUNNING THE REFERENCE'S OWN ``pairwise_distance`` (sampling/utils_sampling.py:126-130,
imported from /root/reference) in the build container; never on the GPU box.  Nothing of the reference is copied: the fixture holds the
inputs this script draws and the outputs the reference returns.

    python tests/golden/make_knn_golden.py

  near_*   two seeded 24 x 2 Gaussian pools: another point is nearer than the 10 the identity adds
  far_*    a pool against itself on a grid 25 apart: the self term (0 + 10) wins every column
  wide_*   two seeded 16 x 33 Gaussian pools in fp32 (cdist widens them)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

import numpy as np

for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.gridspec", "sklearn", "sklearn.metrics"):      # drawing / brier: not what runs here
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
        if name == "sklearn.metrics":
            sys.modules[name].brier_score_loss = None
sys.path.insert(0, os.path.join(REF, "sampling"))
import utils_sampling as U      # noqa: E402


def main():
    rs = np.random.RandomState(2019)
    near_real, near_model = rs.randn(24, 2), rs.randn(24, 2)
    g = 25.0 * np.stack(np.meshgrid(np.arange(4.0), np.arange(3.0)), axis=-1).reshape(-1, 2)
    wide_real, wide_model = rs.randn(16, 33).astype(np.float32), rs.randn(16, 33).astype(np.float32)
    out = {"near_real": near_real, "near_model": near_model, "near_out": U.pairwise_distance(near_real, near_model),
           "far_real": g, "far_model": g.copy(), "far_out": U.pairwise_distance(g, g.copy()),
           "wide_real": wide_real, "wide_model": wide_model, "wide_out": U.pairwise_distance(wide_real, wide_model)}
    np.savez(os.path.join(HERE, "g11_pairwise_distance.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
