"""The density map without a device: the float64 definition of tests/kde_cases.py against live scipy.stats.gaussian_kde with the
reference's bandwidth (set_bandwidth(k.factor / 2.), sampling/utils_sampling.py:106-107), the pure-numpy functions of cgs_amd.metrics
against that definition, the state algebra, the landscape grid, the C ABI surface of csrc/kde2d.hip and the all-reduce over gloo."""
import os
import re
import socket

import numpy as np
import pytest

import kde_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cgs_kde2d_ws_bytes", "cgs_kde2d_accumulate"]


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("kind", ["iso", "corr", "modes9"])
def test_the_float64_definition_equals_scipy_with_the_halved_scott_factor_on_the_double_grid(kind):
    from scipy.stats import gaussian_kde
    x = KC.pool(kind, 2000).astype(np.float64)
    scale, nbins = 4.0, 50
    k = gaussian_kde([x[:, 0], x[:, 1]])
    k.set_bandwidth(bw_method=k.factor / 2.)
    xi, yi = np.mgrid[-scale:scale:nbins * 1j, -scale:scale:nbins * 1j]
    want = k(np.vstack([xi.flatten(), yi.flatten()])).reshape(xi.shape)
    got = KC.density(x, xi[:, 0], yi[0, :])
    ratio = np.abs(got - want).max() / want.max()
    print(f"\n[kde_cases vs scipy, {kind}] worst |delta| / max = {ratio:.3g} (bar 1e-12)")
    assert got.shape == (nbins, nbins) and ratio <= 1e-12
    if kind == "corr":                                                  # the pool is what it says: w10 matters
        W, _ = KC.bandwidth(x)
        assert abs(np.corrcoef(x.T)[0, 1] - 0.95) < 0.01 and abs(W[1, 0]) > 2 * W[0, 0]


def test_metrics_functions_equal_the_definition_on_the_fp32_grid():
    from cgs_amd import metrics as M
    x = KC.pool("modes9", 1500)
    ax, ay = M.kde_axes(4.0, 40), M.kde_axes(3.0, 23)
    whiten, norm = M.kde_whiten(np.cov(x.astype(np.float64), rowvar=False), len(x))
    W, sqrt_det = KC.bandwidth(x)
    assert np.abs(whiten - [W[0, 0], W[1, 0], W[1, 1]]).max() <= 1e-12 * np.abs(W).max() and W[0, 1] == 0.0
    assert abs(norm - len(x) * 2 * np.pi * sqrt_det) <= 1e-13 * norm
    st = M.density_state_of(x, ax, ay, whiten)
    want = KC.density(x, ax, ay)
    assert st["n"] == 1500 and st["sums"].shape == (40, 23)
    for got in (M.density_values(st), M.density_values(st, norm)):      # the state's own divisor and kde_whiten's
        assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert KC.colour_limits(want) == (want.min(), max(0.2 * want.max(), want.min()))


@pytest.mark.parametrize("scale,nbins", [(4.0, 100), (2.4, 100), (0.8, 7), (13.0, 33)])
def test_kde_axes_is_the_mgrid_axis_rounded_to_fp32(scale, nbins):
    from cgs_amd.metrics import kde_axes
    xi, yi = np.mgrid[-scale:scale:nbins * 1j, -scale:scale:nbins * 1j]
    a = kde_axes(scale, nbins)
    assert a.dtype == np.float32 and a.shape == (nbins,)
    assert np.array_equal(a, xi[:, 0].astype(np.float32)) and np.array_equal(a, yi[0, :].astype(np.float32))
    assert np.array_equal(a, KC.axes32(scale, nbins)) and np.array_equal(xi, np.broadcast_to(xi[:, :1], xi.shape))     # [i, j] = (x_i, y_j)


def test_rounding_the_axes_moves_the_map_by_a_few_1e7_of_its_maximum():
    x = KC.pool("modes9", 2000)
    a64, a32 = KC.axes64(4.0, 50), KC.axes32(4.0, 50)
    z64, z32 = KC.density(x, a64, a64), KC.density(x, a32, a32)
    shift = np.abs(z64 - z32).max() / z64.max()
    print(f"\n[fp32 axes] worst |delta| / max = {shift:.3g}")
    assert 0 < shift < 1e-5


def test_density_merge_is_additive_and_refuses_another_grid_or_bandwidth():
    from cgs_amd import metrics as M
    x = KC.pool("corr", 900)
    ax = M.kde_axes(4.0, 17)
    whiten, _ = M.kde_whiten(np.cov(x.astype(np.float64), rowvar=False), len(x))
    whole = M.density_state_of(x, ax, ax, whiten)
    parts = M.density_merge(M.density_merge(M.density_state_of(x[:1], ax, ax, whiten), M.density_state_of(x[1:500], ax, ax, whiten)),
                            M.density_state_of(x[500:], ax, ax, whiten))
    assert parts["n"] == whole["n"] == 900 and np.abs(parts["sums"] - whole["sums"]).max() <= 1e-13 * whole["sums"].max()
    empty = M.density_state_of(x[:0], ax, ax, whiten)
    assert empty["n"] == 0 and not empty["sums"].any() and np.array_equal(M.density_merge(whole, empty)["sums"], whole["sums"])
    with pytest.raises(ValueError):
        M.density_merge(whole, M.density_state_of(x, ax, ax[:-1], whiten))
    with pytest.raises(ValueError):
        M.density_merge(whole, M.density_state_of(x, ax, ax, whiten * 2.0))


def test_kde_whiten_raises_on_one_sample_and_on_a_collinear_pool():
    from cgs_amd.metrics import kde_whiten
    with pytest.raises(ValueError):
        kde_whiten(np.eye(2), 1)
    t = np.random.RandomState(3).randn(500)
    for line in (np.stack([t, t], 1), np.stack([t, 2.0 * t + 1.0], 1), np.stack([0.3 * t - 2.0, -1.7 * t], 1), np.stack([t, 0 * t], 1)):
        with pytest.raises(ValueError):
            kde_whiten(np.cov(line, rowvar=False), 500)
    with pytest.raises(ValueError):
        KC.bandwidth(np.zeros((1, 2)))
    with pytest.raises(ValueError):
        KC.bandwidth(np.stack([t, 0 * t], 1))
    with pytest.raises(ValueError):
        kde_whiten(np.eye(3), 10)
    w, norm = kde_whiten(np.eye(2), 64)                                  # f = 0.5 * 64^(-1/6) = 0.25
    assert np.allclose(w, [4.0, 0.0, 4.0], rtol=1e-15) and abs(norm - 64 * 2 * np.pi / 16) <= 1e-12


@pytest.mark.parametrize("region,ngrids", [(1.0, 21), (2.5, 21), (10.0 * 2.5, 21), (0.3, 5)])
def test_landscape_grid_equals_the_reference_loop_bit_for_bit(region, ngrids):
    from cgs_amd.synthetic import landscape_grid
    got = landscape_grid(region, ngrids)
    assert got.dtype == np.float64 and got.shape == (ngrids * ngrids, 2)
    assert np.array_equal(got, KC.landscape_loop(region, ngrids))
    assert got[1, 0] == got[0, 0] and got[1, 1] > got[0, 1]             # i major


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_bindings_and_library_agree_on_the_new_entry_points():
    import ctypes
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    l = lib.load()
    for name in NEW:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert lib.SIGNATURES["cgs_kde2d_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert l.cgs_version() >= 113
    assert "kde2d.hip" in open(os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc", "Makefile")).read()
    assert lib.built_from() == lib.source_hash()                        # cgs_source_sha covers the new file


def plan(n, cells):
    """csrc/kde2d.hip, kde_plan restated: 1024 cells per block; as many sample slices as bring tiles x slices to 512, of whole multiples
    of 64 samples.  -> (tiles, samples per slice, slices)"""
    tiles = -(-cells // 1024)
    want = min(-(-512 // tiles), max(n // 64, 1))
    size = -(-(-(-n // want)) // 64) * 64
    return tiles, size, -(-n // size)


@pytest.mark.parametrize("n,gx,gy,slices", [(1, 1, 1, 1), (64, 1, 7, 1), (65, 3, 5, 1), (128, 3, 5, 2), (129, 3, 5, 2), (193, 3, 5, 2), (4099, 100, 100, 33),
                                            (10000, 100, 100, 40), (50000, 100, 100, 49), (10000, 256, 256, 8), (10000, 1024, 1024, 1), (1 << 30, 1, 1, 512)])
def test_workspace_query_follows_the_restated_plan_and_bad_arguments_launch_nothing(n, gx, gy, slices):
    from cgs_amd import lib
    l = lib.load()
    tiles, size, ns = plan(n, gx * gy)
    assert ns == slices and size % 64 == 0 and (ns - 1) * size < n <= ns * size
    assert int(l.cgs_kde2d_ws_bytes(n, gx, gy)) == ns * gx * gy * 8
    assert int(l.cgs_kde2d_ws_bytes(0, gx, gy)) == 0
    for bad in ((n, 0, gy), (n, gx, 0), (n, -1, gy), (n, 1025, 1024), (n, 1 << 20, 2), (n, 1 << 16, 1 << 16), (-1, gx, gy), ((1 << 30) + 1, gx, gy)):
        assert int(l.cgs_kde2d_ws_bytes(*bad)) == 0
        b_n, b_gx, b_gy = bad
        assert l.cgs_kde2d_accumulate(None, b_n, None, b_gx, None, b_gy, None, None, None, 0, None) == lib.EINVAL     # the check comes before any pointer
    assert l.cgs_kde2d_accumulate(None, n, None, gx, None, gy, None, None, None, 0, None) == lib.EINVAL                # n samples of a null x
    assert l.cgs_kde2d_accumulate(None, 0, None, gx, None, gy, None, None, None, 0, None) == lib.OK                    # no sample: a no-op


# ---------------------------------------------------------------------------------------------------------------- ranks
def test_all_reduce_without_a_process_group_is_the_identity():
    from cgs_amd import metrics as M
    ax = M.kde_axes(4.0, 9)
    st = M.density_state_of(KC.pool("iso", 200), ax, ax, [1.0, 0.2, 1.5])
    assert M.all_reduce_density(st) is st


def _rank_state(rank):
    from cgs_amd import metrics as M
    x = KC.pool("modes9", 1000)
    ax, ay = M.kde_axes(4.0, 12), M.kde_axes(4.0, 9)
    whiten, _ = M.kde_whiten(np.cov(x.astype(np.float64), rowvar=False), len(x))      # the whole pool's bandwidth on both ranks
    return M.density_state_of(x[:400] if rank == 0 else x[400:], ax, ay, whiten)


def _gloo_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    from cgs_amd.metrics import all_reduce_density
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.save(all_reduce_density(_rank_state(rank)), out + f".{rank}")
    dist.destroy_process_group()


def test_all_reduce_over_gloo_equals_the_merge_of_the_two_host_states(tmp_path):
    import torch
    import torch.multiprocessing as mp
    from cgs_amd import metrics as M
    out = str(tmp_path / "state")
    with socket.socket() as so:                                   # a free rendezvous port on the loopback interface
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, out), nprocs=2, join=True)
    want = M.density_merge(_rank_state(0), _rank_state(1))
    x = KC.pool("modes9", 1000)
    whole = KC.density(x, M.kde_axes(4.0, 12), M.kde_axes(4.0, 9))
    for r in range(2):
        got = torch.load(out + f".{r}", weights_only=False)
        assert got["n"] == want["n"] == 1000 and got["sums"].shape == (12, 9) and np.array_equal(got["whiten"], want["whiten"])
        assert np.abs(got["sums"] - want["sums"]).max() <= 1e-15 * want["sums"].max()
        assert np.abs(M.density_values(got) - whole).max() <= 1e-12 * whole.max()      # the ranks together are the one-pool map
