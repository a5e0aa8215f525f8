"""The host surface of the density maps on the device: ``metrics.kde_grid`` against live scipy with the reference's
bandwidth, ``metrics.DensityMap`` fed from two streams, and ``synthetic.evaluate_collaborative(maps=...)``.  The bar is the kernel's: every
cell within 1e-4 of the map's maximum (tests/test_gpu_kde2d.py)."""
import types

import numpy as np
import pytest
import torch

import kde_cases as KC

pytestmark = pytest.mark.gpu

from oracle import sampling_ref as S

DEV = torch.device("cuda:0")
BAR = 1e-4


def test_kde_grid_gives_scipys_map_of_a_25_mode_pool_and_draw_kdes_colour_limits():
    from scipy.stats import gaussian_kde
    from cgs_amd import metrics as M
    x = KC.pool("modes25", 2000)
    scale, nbins = 2.4, 40
    x64 = x.astype(np.float64)
    k = gaussian_kde([x64[:, 0], x64[:, 1]])
    k.set_bandwidth(bw_method=k.factor / 2.)
    xi, yi = np.mgrid[-scale:scale:nbins * 1j, -scale:scale:nbins * 1j]
    want = k(np.vstack([xi.flatten(), yi.flatten()])).reshape(xi.shape)
    for samples in (x, torch.from_numpy(np.array(x)).to(DEV)):           # a host array and a device tensor
        zi, (vmin, vmax) = M.kde_grid(samples, scale, nbins, device=DEV)
        ratio = np.abs(zi - want).max() / want.max()
        print(f"\n[kde_grid vs scipy] worst |delta| / max = {ratio:.3g} (bar {BAR:g})")
        assert zi.shape == (nbins, nbins) and zi.dtype == np.float64 and ratio <= BAR
        wmin, wmax = KC.colour_limits(want)
        assert (vmin, vmax) == (zi.min(), max(0.2 * zi.max(), zi.min()))
        assert abs(vmin - wmin) <= BAR * want.max() and abs(vmax - wmax) <= BAR * want.max()
    with pytest.raises(ValueError):
        M.kde_grid(x[:1], scale, nbins, device=DEV)
    with pytest.raises(ValueError):
        M.kde_grid(np.stack([x[:, 0], x[:, 0]], 1), scale, nbins, device=DEV)                   # a collinear pool
    with pytest.raises(ValueError):
        M.DensityMap(M.kde_axes(1.0, 5), M.kde_axes(1.0, 5), [1.0, 0.0, 1.0], "cpu")


def test_density_map_in_batches_of_64_from_two_streams_equals_one_update():
    from cgs_amd import metrics as M
    x = KC.pool("modes9", 2000)
    ax, ay = M.kde_axes(4.0, 50), M.kde_axes(3.0, 31)
    whiten, norm = M.kde_whiten(np.cov(x.astype(np.float64), rowvar=False), len(x))
    xd = torch.from_numpy(np.array(x)).to(DEV)
    one = M.DensityMap(ax, ay, whiten, DEV).update(xd)
    many = M.DensityMap(ax, ay, whiten, DEV)
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    torch.cuda.synchronize()
    for i, a in enumerate(range(0, len(x), 64)):
        with torch.cuda.stream(streams[i % 2]):
            many.update(xd[a:a + 64])
    s1, sm = one.state(), many.state()
    ref = M.density_state_of(x, ax, ay, whiten)
    top = ref["sums"].max()
    assert s1["n"] == sm["n"] == 2000 and sm["sums"].shape == (50, 31) and np.array_equal(sm["whiten"], whiten)
    print(f"\n[DensityMap] batches vs one update {np.abs(sm['sums'] - s1['sums']).max() / top:.3g}, batches vs float64 "
          f"{np.abs(sm['sums'] - ref['sums']).max() / top:.3g} of the maximum (bar {BAR:g})")
    assert np.abs(sm["sums"] - s1["sums"]).max() <= BAR * top and np.abs(sm["sums"] - ref["sums"]).max() <= BAR * top
    want = KC.density(x, ax, ay)
    for got in (many.values(), many.values(norm)):
        assert np.abs(got - want).max() <= BAR * want.max()
    assert M.all_reduce_density(many)["n"] == 2000                        # no process group: the identity


def test_evaluate_collaborative_with_maps_adds_the_maps_and_moves_nothing_else(monkeypatch):
    """The data, generator and refiner of tests/test_gpu_synthetic.py's end-to-end evaluation (Imbal-8Gaussians at scale 10, the modes blurred
    by a 0.8-sigma Gaussian as the generator, ladam, 20 steps, rate 0.1) with 500 rows and a D trained for 200 calibrate iterations only:
    what is checked here is that the maps are those of the pools and that nothing else moves, not the quality of the samples."""
    from cgs_amd import metrics as M
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.synthetic import DShaper, Gan, MLPDiscriminator, Refiner, evaluate_collaborative, landscape_grid
    Ws, bs = S.mlp_init(64, 6, seed=2019, scale=1.0)
    D = MLPDiscriminator.from_lists([w.numpy() for w in Ws], [b.numpy() for b in bs], "cuda:0")
    data = ToyDataset("Imbal-8Gaussians", 10.0, 0.9)
    n = 500
    args = types.SimpleNamespace(rollout_steps=20, rollout_rate=0.1, rollout_method="ladam")
    sh = DShaper(D, lrd=1e-2)
    np.random.seed(2019)
    train_rs = np.random.RandomState(3)
    for _ in range(200):
        sh.step(data.next_batch(1000), (data.centeroids[train_rs.randint(8, size=1000)] + 0.8 * train_rs.randn(1000, 2)).astype(np.float32))
    pools = []
    real_kde_grid = M.kde_grid

    def recording_kde_grid(samples, *a, **kw):
        pools.append(np.array(samples.cpu() if isinstance(samples, torch.Tensor) else samples))
        return real_kde_grid(samples, *a, **kw)
    monkeypatch.setattr(M, "kde_grid", recording_kde_grid)
    region, nbins = 8.0, 30
    outs, ends, batches = [], [], []
    for maps in (None, dict(scale=region, nbins=nbins, grid_scale=10.0)):
        ref = Refiner(args)
        ref.set_env(Gan(D), None, data)
        gen_rs = np.random.RandomState(5)
        generate = lambda: (data.centeroids[gen_rs.randint(8, size=n)] + 0.8 * gen_rs.randn(n, 2)).astype(np.float32)
        np.random.seed(11)
        eval_batch, target = generate(), data.next_batch(n)
        outs.append(evaluate_collaborative(ref, D, generate, eval_batch, target, data.centeroids, data.std, **({} if maps is None else dict(maps=maps))))
        ends.append(np.random.get_state()[1].copy())
        batches.append((eval_batch, target))
    plain, full = outs
    assert np.array_equal(ends[0], ends[1])                               # the numpy stream is where it was
    assert set(plain) == {"standard", "refinement", "collaborate"} and set(full) == set(plain) | {"maps"}
    for part in plain:
        assert full[part] == plain[part], part                            # every metric and eff, identical
    maps = full["maps"]
    assert set(maps) == {"standard", "refinement", "collaborate", "target", "landscape"} and len(pools) == 4
    eval_batch, target = batches[1]
    assert np.array_equal(pools[0], eval_batch) and np.array_equal(pools[3], target) and pools[1].shape == pools[2].shape == (n, 2)
    assert not np.array_equal(pools[1], pools[0]) and not np.array_equal(pools[2], pools[1])
    axis = KC.axes32(region, nbins)
    for name, pool in zip(("standard", "refinement", "collaborate", "target"), pools):
        want = KC.density(pool.astype(np.float32), axis, axis)            # (the device takes the pool as fp32)
        got = maps[name]
        ratio = np.abs(got - want).max() / want.max()
        print(f"\n[evaluate_collaborative maps, {name}] worst |delta| / max = {ratio:.3g} (bar {BAR:g})")
        assert got.shape == (nbins, nbins) and got.dtype == np.float64 and ratio <= BAR, name
    grid, sig = maps["landscape"]
    assert np.array_equal(grid, landscape_grid(10.0, 21)) and np.array_equal(grid, KC.landscape_loop(10.0, 21))
    assert np.array_equal(sig, D.sigmoid_and_saliency(grid, want_saliency=False)[0].cpu().numpy()) and sig.shape == (441, 1)
    with pytest.raises(ValueError):
        evaluate_collaborative(ref, D, generate, eval_batch, target, data.centeroids, data.std, maps=dict(nbins=10))
