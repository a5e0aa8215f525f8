"""Record tests/golden/calibration_golden.npz and mode_golden.npz from the REFERENCE's own functions (CPU only, never on the GPU box):

    python tests/golden/make_calibration_golden.py <path to the reference checkout>

Nothing of the reference is copied: its sampling/utils_sampling.py and synthetic/Datasets.py are imported, and the two row writers
(save_metrics of synthetic/main.py, GAN.write of nsgan/GAN.py -- modules that import TensorFlow) are cut out of their files with ``ast``
and executed as they stand, writing one row each to a temporary file.  Only inputs and recorded outputs are saved.

calibration_golden.npz -- calibration_diagnostic / calibration_bins (n_bins = 20) on float64 holders of fp32 scores, as nsgan/GAN.py:287-301
fills them:
  c1: 1000 fake + 1500 real sigmoids; RandomState(2019): fake logits = randn(1000) - 1, real logits = randn(1500) + 1, sigmoid in
      float64, rounded to fp32.
  c2: c1 plus, for each of the 21 double edges, its fp32 neighbours (the largest fp32 below it and the smallest fp32 at or above it)
      and 0.0, 1.0 and the smallest positive denormal; the neighbours go to the fake set, the three extras to the real set.  Two neighbours
      are left out because the reference itself cannot take them: the fp32 below edge 0 is negative (np.bincount raises) and the fp32
      at or above the last edge is above 1 (sklearn's brier_score_loss raises).
  c3: 8 fake + 8 real scores, all 0.5.
mode_golden.npz -- 25Gaussians and Imbal-8Gaussians (scale 10, ratio 0.9): centeroids, std, a real pool of 1000 dataset samples and a
  model pool of 1000 (750 dataset samples + N(0, 0.05) jitter, 250 from N(0, 4^2)), both fp32; the reference's metrics_distance,
  freq_category, metrics_diversity and metrics_distribution at thres = 4 std; and what cgs_amd.metrics' functions of the same names
  returned on the commit before their count-to-frequency tail was factored out (``proj_*``: pinned bit for bit by the CPU test).
rows (in calibration_golden.npz): the bytes the two writers append for the recorded arguments.
"""
import ast
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2019


def reference_function(path, name):
    """The function (or method) ``name`` of a reference file, executed from its own source without importing the module."""
    with open(path) as fh:
        tree = ast.parse(fh.read())
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            ns = {}
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
            return ns[name]
    raise KeyError(name)


def row_of(fn, *args):
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "row.txt")
        fn(*((None, f) if fn.__name__ == "write" else (f,)), *args)
        with open(f, "rb") as fh:
            return np.frombuffer(fh.read(), dtype=np.uint8)


def main(ref):
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(ref, "sampling"))
    sys.path.insert(0, os.path.join(ref, "synthetic"))
    sys.path.insert(0, ROOT)
    import Datasets
    import utils_sampling as U

    rs = np.random.RandomState(SEED)
    sig = lambda t: (1.0 / (1.0 + np.exp(-t))).astype(np.float32)
    fake, real = sig(rs.randn(1000) - 1.0), sig(rs.randn(1500) + 1.0)
    assert (fake.astype(np.float64) * (1 - fake.astype(np.float64))).sum() + (real.astype(np.float64) * (1 - real.astype(np.float64))).sum() > 400
    edges = np.linspace(0., 1. + 1e-8, 21)
    nb = []
    for e in edges:
        hi = np.float32(e)
        if float(hi) < e:
            hi = np.nextafter(hi, np.float32(np.inf))
        lo = np.nextafter(hi, np.float32(-np.inf))
        assert float(lo) < e <= float(hi)
        nb += [v for v in (lo, hi) if 0.0 <= float(v) <= 1.0]
    nb = np.asarray(nb, dtype=np.float32)
    extra = np.asarray([0.0, 1.0, np.nextafter(np.float32(0), np.float32(1))], dtype=np.float32)
    cases = {"c1": (fake, real), "c2": (np.concatenate([fake, nb]), np.concatenate([real, extra])),
             "c3": (np.full(8, 0.5, np.float32), np.full(8, 0.5, np.float32))}
    out = dict(seed=np.array([SEED]), edges=edges,
               recipe=np.array("RandomState(seed): fake = f32(sigmoid(randn(1000) - 1)), real = f32(sigmoid(randn(1500) + 1))"))
    for name, (f, r) in cases.items():
        f64, r64 = np.empty((f.size, 1)), np.empty((r.size, 1))           # float64 holders of the fp32 values (nsgan/GAN.py:287,294)
        f64[:, 0], r64[:, 0] = f, r
        z, brier, ece, mce = U.calibration_diagnostic(f64, r64)
        y_pred = np.concatenate([f64, r64])
        y_true = np.concatenate([np.zeros_like(f64), np.ones_like(r64)])
        pt, pp, w = U.calibration_bins(y_true, y_pred, n_bins=20)
        out.update({f"{name}_fake": f, f"{name}_real": r, f"{name}_diag": np.array([z, brier, ece, mce], dtype=np.float64),
                    f"{name}_prob_true": pt, f"{name}_prob_pred": pp, f"{name}_weights": w})
    args_syn = (7, 1500, 0.12345, 0.98765, 0.0123449, 0.25, 0.3333333, -1.23456789, 0.12995, 0.049951, 0.5)
    args_ns = (7, 1500, 8.76543, 12.00005, 1.0, -1.23456789, 0.12995, 0.049951, 0.5)
    out["row_synthetic_args"], out["row_nsgan_args"] = np.array(args_syn), np.array(args_ns)
    out["row_synthetic"] = row_of(reference_function(os.path.join(ref, "synthetic", "main.py"), "save_metrics"), *args_syn)
    out["row_nsgan"] = row_of(reference_function(os.path.join(ref, "nsgan", "GAN.py"), "write"), *args_ns)
    np.savez_compressed(os.path.join(OUT, "calibration_golden.npz"), **out)

    from cgs_amd import metrics as M
    out = {}
    for tag, d in (("g25", Datasets.ToyDataset(distr="25Gaussians")), ("imb8", Datasets.ToyDataset(distr="Imbal-8Gaussians", scale=10.0, ratio=0.9))):
        np.random.seed(SEED)
        real = d.next_batch(1000).astype(np.float32)
        rs = np.random.RandomState(SEED + 1)
        model = np.concatenate([d.next_batch(750)[::-1] + rs.randn(750, 2) * 0.05, rs.randn(250, 2) * 4.0]).astype(np.float32)
        c, thres = np.asarray(d.centeroids, dtype=np.float64), float(d.std * 4)
        out.update({f"{tag}_centeroids": c, f"{tag}_std": np.array([d.std]), f"{tag}_thres": np.array([thres]), f"{tag}_real": real, f"{tag}_model": model})
        for fam, mod in (("ref", U), ("proj", M)):
            for pool, x in (("real", real), ("model", model)):
                md, good = mod.metrics_distance(x, c, thres)
                fv, fa = mod.freq_category(x, c, thres)
                out.update({f"{tag}_{fam}_{pool}_dist": np.array([md, good], dtype=np.float64), f"{tag}_{fam}_{pool}_freqs_valid": fv,
                            f"{tag}_{fam}_{pool}_freqs_all": fa})
            out[f"{tag}_{fam}_kl_js"] = np.array([mod.metrics_diversity(real, model, c, thres), mod.metrics_distribution(real, model, c, thres)],
                                                 dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "mode_golden.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
