"""``synthetic.evaluate_collaborative(manifold=...)`` and ``synthetic.evaluate_calibrated(manifold=...)`` on the small
seeded 2-D setup of tests/test_gpu_density_maps.py: the rows gain precision / recall / density / coverage of their pool against the target
batch, equal to ``metrics.manifold_metrics_host`` of the kept pools, and nothing else moves -- every other entry and the numpy stream's
end are those of ``manifold=None``."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampling_ref as S

NEW = ("precision", "recall", "density", "coverage")
_GAN = {}


def _setup_2d():
    """The data and D of tests/test_gpu_density_maps.py: Imbal-8Gaussians at scale 10, a 64-unit D shaped for 200 calibrate iterations
    against the modes blurred by a 0.8-sigma Gaussian."""
    if "2d" not in _GAN:
        from cgs_amd.datasets import ToyDataset
        from cgs_amd.synthetic import DShaper, MLPDiscriminator
        Ws, bs = S.mlp_init(64, 6, seed=2019, scale=1.0)
        D = MLPDiscriminator.from_lists([w.numpy() for w in Ws], [b.numpy() for b in bs], "cuda:0")
        data = ToyDataset("Imbal-8Gaussians", 10.0, 0.9)
        sh = DShaper(D, lrd=1e-2)
        np.random.seed(2019)
        train_rs = np.random.RandomState(3)
        for _ in range(200):
            sh.step(data.next_batch(1000), (data.centeroids[train_rs.randint(8, size=1000)] + 0.8 * train_rs.randn(1000, 2)).astype(np.float32))
        _GAN["2d"] = (D, data)
    return _GAN["2d"]


def _host(pool):
    return pool.cpu().numpy() if isinstance(pool, torch.Tensor) else np.asarray(pool)


def _check(plain, full, ends, rows, pools, target, k):
    from cgs_amd import metrics as M
    assert np.array_equal(ends[0], ends[1])                               # the numpy stream is where it was
    assert set(plain) == set(full) == set(rows) | {"pools"}
    for row in rows:
        assert set(full[row]) == set(plain[row]) | set(NEW), row
        for key, v in plain[row].items():
            assert full[row][key] == v, (row, key)                        # every metric and eff, identical
    for name in plain["pools"]:
        assert np.array_equal(_host(plain["pools"][name]), _host(full["pools"][name])), name
    for row, pool in pools.items():
        want = M.manifold_metrics_host(target.astype(np.float32), _host(pool).astype(np.float32), k)     # (the device takes the pools as fp32)
        got = {key: full[row][key] for key in NEW}
        print(f"\n[manifold= {row}] {got}")
        assert got == {key: want[key] for key in NEW}, row
        assert all(0.0 <= got[key] <= 1.0 for key in ("precision", "recall", "coverage")) and got["density"] >= 0.0


def test_evaluate_collaborative_with_manifold_adds_four_numbers_per_row_and_moves_nothing_else():
    from cgs_amd.synthetic import Gan, Refiner, evaluate_collaborative
    D, data = _setup_2d()
    n, k = 500, 3
    args = types.SimpleNamespace(rollout_steps=20, rollout_rate=0.1, rollout_method="ladam")
    outs, ends, batches = [], [], []
    for manifold in (None, dict(k=k)):
        ref = Refiner(args)
        ref.set_env(Gan(D), None, data)
        gen_rs = np.random.RandomState(5)
        generate = lambda: (data.centeroids[gen_rs.randint(8, size=n)] + 0.8 * gen_rs.randn(n, 2)).astype(np.float32)
        np.random.seed(11)
        eval_batch, target = generate(), data.next_batch(n)
        outs.append(evaluate_collaborative(ref, D, generate, eval_batch, target, data.centeroids, data.std, keep_pools=True,
                                           **({} if manifold is None else dict(manifold=manifold))))
        ends.append(np.random.get_state()[1].copy())
        batches.append((eval_batch, target))
    plain, full = outs
    eval_batch, target = batches[1]
    _check(plain, full, ends, ("standard", "refinement", "collaborate"),
           {"standard": eval_batch, "refinement": full["pools"]["refinement"], "collaborate": full["pools"]["collaborate"]}, target, k)
    for bad in (dict(), dict(k=0), dict(k=9), dict(k=3, scale=1.0)):
        with pytest.raises(ValueError):
            evaluate_collaborative(ref, D, generate, eval_batch, target, data.centeroids, data.std, manifold=bad)


def test_evaluate_calibrated_with_manifold_adds_four_numbers_per_row_and_moves_nothing_else():
    from cgs_amd.sampling import DeviceIndependenceSampler
    from cgs_amd.synthetic import evaluate_calibrated
    D, data = _setup_2d()
    n, k = 500, 3
    outs, ends, batches = [], [], []
    for manifold in (None, dict(k=k)):
        gen_rs = np.random.RandomState(5)
        generate = lambda: (data.centeroids[gen_rs.randint(8, size=n)] + 0.8 * gen_rs.randn(n, 2)).astype(np.float32)
        np.random.seed(11)
        eval_batch, target = generate(), data.next_batch(n)
        outs.append(evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, keep_pools=True,
                                        mh_sampler=DeviceIndependenceSampler(T=20, device=torch.device("cuda:0")),
                                        **({} if manifold is None else dict(manifold=manifold))))
        ends.append(np.random.get_state()[1].copy())
        batches.append((eval_batch, target))
    plain, full = outs
    eval_batch, target = batches[1]
    assert isinstance(full["pools"]["hastings"], torch.Tensor)            # the device pools go to the kernels as they are
    _check(plain, full, ends, ("standard", "rejection", "hastings"),
           {"standard": eval_batch, "rejection": full["pools"]["rejection"], "hastings": full["pools"]["hastings"]}, target, k)
