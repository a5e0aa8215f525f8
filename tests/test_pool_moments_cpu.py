"""The pool-moments feature without a device: the C ABI surface and the slab / tile plan of csrc/moments.hip restated, the pure-numpy
state algebra of cgs_amd.metrics (rebase, merge, finalise, the Frechet tail), and the all-reduce of states over gloo."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cgs_pool_moments_ws_bytes", "cgs_pool_moments_accumulate", "cgs_spatial_mean"]


def test_header_bindings_and_library_agree_on_the_new_entry_points():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    l = lib.load()
    for name in NEW:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        nargs = len(decl.group(1).split(","))
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert lib.SIGNATURES["cgs_pool_moments_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert len(lib.SIGNATURES["cgs_pool_moments_accumulate"][1]) == 11
    assert l.cgs_version() >= 110


def plan(m, d):
    """csrc/moments.hip, mom_plan: T = ceil(d / 64) column tiles, P = T (T + 1) / 2 tile pairs on or above the diagonal; aim at 1024
    blocks, at least 128 samples per slab, at most 32 slabs, samples per slab rounded up to the 32-sample tile.
    Returns (T, P, samples per slab, slabs, workspace bytes): per slab P tiles of 64 x 64 doubles and T x 64 column sums."""
    T = -(-d // 64)
    P = T * (T + 1) // 2
    slabs = min(-(-1024 // P), max(1, m // 128), 32)
    sps = -(-(-(-m // slabs)) // 32) * 32
    slabs = -(-m // sps)
    return T, P, sps, slabs, slabs * (P * 64 * 64 + T * 64) * 8


@pytest.mark.parametrize("m,d,slabs,last", [
    (100, 64, 1, 100),           # one slab
    (1, 1, 1, 1),                # d = 1
    (450, 17, 3, 130),           # three slabs of 160, a short last one (the GPU test's slab shape)
    (1000, 130, 7, 40),          # T = 3: six tile pairs
    (300, 2048, 2, 140),         # the widest d: 528 tile pairs; the block target allows 2 slabs
    (8192, 2048, 2, 4096),
    (32768, 512, 29, 512),       # below the cap: ceil(1024 / 36) = 29
    (100000, 16, 32, 2784),      # the slab cap
])
def test_workspace_query_against_the_restated_plan(m, d, slabs, last):
    from cgs_amd import lib
    T, P, sps, n_slabs, nbytes = plan(m, d)
    assert n_slabs == slabs and m - (slabs - 1) * sps == last and sps % 32 == 0
    assert int(lib.load().cgs_pool_moments_ws_bytes(m, d)) == nbytes


def test_unsupported_shapes_are_refused_before_anything_is_dereferenced():
    from cgs_amd import lib
    l = lib.load()
    for m, d in [(10, 0), (10, 2049), (-1, 16)]:
        assert int(l.cgs_pool_moments_ws_bytes(m, d)) == 0
        # null device pointers throughout: the shape check comes first (rows == NULL: the n rows of x)
        assert l.cgs_pool_moments_accumulate(None, max(m, 0), d, None, m, None, None, None, None, 0, None) == lib.EINVAL
    assert l.cgs_pool_moments_accumulate(None, 1 << 20, 1024, None, 0, None, None, None, None, 0, None) == lib.EINVAL      # x of 4 GiB
    assert int(l.cgs_pool_moments_ws_bytes(0, 16)) == 0
    assert l.cgs_pool_moments_accumulate(None, 0, 16, None, 0, None, None, None, None, 0, None) == lib.OK                   # no sample: a no-op
    rows = (ctypes.c_int * 1)()
    assert l.cgs_pool_moments_accumulate(None, 5, 16, ctypes.cast(rows, ctypes.c_void_p), 0, None, None, None, None, 0, None) == lib.OK
    assert l.cgs_pool_moments_accumulate(None, 5, 16, None, 0, None, None, None, None, 0, None) == lib.EINVAL               # 5 rows of a null x


def _cloud(n, d, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(n, d) * rs.uniform(0.5, 3.0, d) + rs.uniform(-100.0, 100.0, d)


@pytest.mark.parametrize("n", [600, 5000])
@pytest.mark.parametrize("d", [3, 64])
def test_merged_chunks_with_three_shifts_finalise_to_numpy_mean_and_cov(n, d):
    from cgs_amd.metrics import frechet_distance, frechet_from_moments, moments_mean_cov, moments_merge, moments_of, moments_rebase
    x = _cloud(n, d, n + d)
    cuts = [0, n // 7, n // 2, n]
    shifts = [x[:5].mean(0), np.zeros(d), x.mean(0) + 1.0]
    st = None
    for (a, b), c in zip(zip(cuts[:-1], cuts[1:]), shifts):
        part = moments_of(x[a:b], c)
        st = part if st is None else moments_merge(st, part)
    assert st["n"] == n and np.array_equal(st["shift"], shifts[0])
    mean, cov = moments_mean_cov(st)
    ref = np.cov(x, rowvar=False)
    assert np.abs(mean - x.mean(0)).max() <= 1e-10 * np.abs(ref).max()
    assert np.abs(cov - ref).max() <= 1e-10 * np.abs(ref).max()
    # a rebase there and back is the identity to rounding, and ddof is np.cov's
    back = moments_rebase(moments_rebase(st, shifts[2]), shifts[0])
    assert np.abs(back["gram"] - st["gram"]).max() <= 1e-10 * np.abs(st["gram"]).max()
    assert np.abs(moments_mean_cov(st, ddof=0)[1] - np.cov(x, rowvar=False, ddof=0)).max() <= 1e-10 * np.abs(ref).max()
    # the Frechet tail on two such states against the cloud form
    y = _cloud(n // 2, d, 7 * n + d) * 0.9 + 0.5
    sy = moments_merge(moments_of(y[:100], y[0]), moments_of(y[100:], y[-1]))
    fd = frechet_from_moments(*moments_mean_cov(st), *moments_mean_cov(sy))
    want = frechet_distance(x, y)
    assert abs(fd - want) <= 1e-8 * abs(want)


def test_frechet_distance_returns_the_value_it_returned_before_the_split():
    """The literal is what cgs_amd.metrics.frechet_distance returned on the parent commit for this seed."""
    from cgs_amd.metrics import frechet_distance
    rs = np.random.RandomState(1234)
    a = rs.randn(400, 12) * rs.uniform(0.5, 2, 12) + rs.uniform(-3, 3, 12)
    b = rs.randn(300, 12) @ rs.randn(12, 12) * 0.5 + rs.uniform(-3, 3, 12)
    assert frechet_distance(a, b) == float.fromhex("0x1.e76482d5cf7b4p+6") == 121.84815534666888


def test_all_reduce_moments_without_a_process_group_is_the_identity():
    from cgs_amd.metrics import all_reduce_moments, moments_of
    st = moments_of(_cloud(50, 4, 1), np.ones(4))
    assert all_reduce_moments(st) is st


def _gloo_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    from cgs_amd.metrics import all_reduce_moments, moments_of
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x = _cloud(300 + 50 * rank, 6, 40 + rank)
    got = all_reduce_moments(moments_of(x, x[rank]))              # the ranks start from different shifts
    torch.save(got, out + f".{rank}")
    dist.destroy_process_group()


def test_all_reduce_moments_over_gloo_equals_the_merge(tmp_path):
    import torch
    import torch.multiprocessing as mp
    from cgs_amd.metrics import moments_merge, moments_of
    out = str(tmp_path / "state")
    with socket.socket() as so:                                   # a free rendezvous port on the loopback interface
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, out), nprocs=2, join=True)
    xs = [_cloud(300 + 50 * r, 6, 40 + r) for r in range(2)]
    want = moments_merge(moments_of(xs[0], xs[0][0]), moments_of(xs[1], xs[1][1]))
    for r in range(2):
        got = torch.load(out + f".{r}", weights_only=False)
        assert got["n"] == want["n"] == 650 and np.array_equal(got["shift"], want["shift"])
        assert np.abs(got["sum"] - want["sum"]).max() <= 1e-12 * np.abs(want["sum"]).max()
        assert np.abs(got["gram"] - want["gram"]).max() <= 1e-12 * np.abs(want["gram"]).max()
