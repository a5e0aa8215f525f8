"""cgs_pool_moments_accumulate (csrc/moments.hip) against numpy float64 of the same definition:

    a_i = double(x[r_i]) - double(shift)        sum[j] += sum_i a_ij        gram[j][k] += sum_i a_ij a_ik

The bar is derived, not measured.  Every term is ONE double product and every sum a double sum, so for any
summation order an entry that starts from g0 ends within gamma_{m+1} <= 2 (m + 2) u of (|g0| + sum_i |a_ij a_ik|), u = 2^-53; the same with
|a_ij| for ``sum``.  The reference (numpy's float64 product) carries the same kind of error, hence the factor 2 on top.  The worst
observed ratio to the bound is printed per case (and recorded in DESIGN.md).

Shapes: one sample / one column; d below, at and just above the 16-column MFMA tile and the 64-column block tile (5, 16, 17, 64, 130);
m below, at and above the 32-sample tile (3, 64, 65); 2 slabs (257 x 64) and 7 slabs (1000 x 130) with a short last one; the widest d (2048:
528 tile pairs); and 450 x 17 -- three slabs of 160 samples, the last one 130 (the plan restated in tests/test_pool_moments_cpu.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SHAPES = [(1, 1), (3, 5), (64, 16), (65, 17), (257, 64), (1000, 130), (300, 2048), (450, 17)]
WORST = {}


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(n, d):
    """(x fp32 [n, d] = 100 + N(0, 1); its fp32 column mean; unrelated symmetric non-zero start contents) -- computed once per shape."""
    rs = np.random.RandomState(1000 * n + d)
    x = (100.0 + rs.randn(n, d)).astype(np.float32)
    shift = x.mean(0).astype(np.float32)
    s0 = rs.randn(d) * 50.0
    g0 = rs.randn(d, d) * 50.0
    g0 = g0 + g0.T
    for v in (x, shift, s0, g0):
        v.setflags(write=False)
    return x, shift, s0, g0


def _reference(x, shift, rows, s0, g0):
    """numpy float64 of the definition -> (sum, gram, bound on sum, bound on gram)."""
    a = x.astype(np.float64) if rows is None else x[np.asarray(rows, dtype=np.int64)].astype(np.float64)
    if shift is not None:
        a = a - shift.astype(np.float64)
    m = a.shape[0]
    aa = np.abs(a)
    s = s0 + a.sum(0)
    g = g0 + a.T.dot(a)
    bs = 2.0 * (m + 2) * U * (np.abs(s0) + aa.sum(0))
    bg = 2.0 * (m + 2) * U * (np.abs(g0) + aa.T.dot(aa))
    return s, g, bs, bg


def _run(x_dev, shift_dev, rows, s0, g0):
    from cgs_amd import kernels as K
    s = torch.from_numpy(np.array(s0)).to(_dev())
    g = torch.from_numpy(np.array(g0)).to(_dev())
    K.pool_moments(x_dev, s, g, shift=shift_dev, rows=rows)
    return s, g


def _check(tag, s, g, ref):
    rs, rg, bs, bg = ref
    sh, gh = s.cpu().numpy(), g.cpu().numpy()
    ratio_s = float((np.abs(sh - rs) / np.maximum(bs, 1e-300)).max())
    ratio_g = float((np.abs(gh - rg) / np.maximum(bg, 1e-300)).max())
    WORST[tag] = (ratio_s, ratio_g)
    print(f"\n[pool_moments {tag}] worst |delta| / bound: sum {ratio_s:.3g}, gram {ratio_g:.3g} (bar 2)")
    assert np.isfinite(sh).all() and np.isfinite(gh).all()
    assert ratio_s <= 2.0 and ratio_g <= 2.0, (tag, ratio_s, ratio_g)
    assert np.array_equal(gh, gh.T), tag                      # exactly symmetric


@pytest.mark.parametrize("onto", ["zeros", "contents"])
@pytest.mark.parametrize("shifted", [False, True], ids=["noshift", "shift"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_update_meets_the_derived_bound_is_symmetric_and_reruns_bit_equal(n, d, shifted, onto):
    from cgs_amd import kernels as K
    x, shift, s0, g0 = _case(n, d)
    if onto == "zeros":
        s0, g0 = np.zeros(d), np.zeros((d, d))
    xd = torch.from_numpy(np.array(x)).to(_dev())
    sd = torch.from_numpy(np.array(shift)).to(_dev()) if shifted else None
    s, g = _run(xd, sd, None, s0, g0)
    _check(f"{n}x{d} {'shift' if shifted else 'noshift'} {onto}", s, g, _reference(x, shift if shifted else None, None, s0, g0))
    # a NaN-filled workspace does not leak, and the rerun is bit-equal
    for ws in K._mom_ws.values():
        ws.fill_(float("nan"))
    s2, g2 = _run(xd, sd, None, s0, g0)
    assert torch.equal(s, s2) and torch.equal(g, g2)


@pytest.mark.parametrize("n,d", SHAPES)
def test_row_subsets_unsorted_unique_one_all_but_one_and_none(n, d):
    x, shift, s0, g0 = _case(n, d)
    xd, sd = torch.from_numpy(np.array(x)).to(_dev()), torch.from_numpy(np.array(shift)).to(_dev())
    perm = np.random.RandomState(7).permutation(n)
    for m in sorted({1, n - 1, max(1, n // 2)} - {0}):
        rows = perm[:m]
        s, g = _run(xd, sd, rows, s0, g0)
        _check(f"{n}x{d} rows m={m}", s, g, _reference(x, shift, rows, s0, g0))
    s, g = _run(xd, sd, np.zeros(0, dtype=np.int64), s0, g0)            # m = 0: bit-unchanged
    assert np.array_equal(s.cpu().numpy(), s0) and np.array_equal(g.cpu().numpy(), g0)


@pytest.mark.parametrize("n,d", [s for s in SHAPES if s[0] >= 3])
def test_two_successive_updates_and_one_update_of_the_concatenation_both_meet_the_bound(n, d):
    from cgs_amd import kernels as K
    x, shift, s0, g0 = _case(n, d)
    cut = n // 3
    sd = torch.from_numpy(np.array(shift)).to(_dev())
    ref = _reference(x, shift, None, s0, g0)
    s, g = _run(torch.from_numpy(np.array(x)).to(_dev()), sd, None, s0, g0)
    _check(f"{n}x{d} whole", s, g, ref)
    s, g = _run(torch.from_numpy(x[:cut].copy()).to(_dev()), sd, None, s0, g0)
    K.pool_moments(torch.from_numpy(x[cut:].copy()).to(_dev()), s, g, shift=sd)
    _check(f"{n}x{d} two updates", s, g, ref)


def test_the_wrapper_refuses_bad_rows_layouts_and_types():
    from cgs_amd import kernels as K
    from cgs_amd import lib as L
    x = torch.ones((6, 8), dtype=torch.float32, device=_dev())
    s = torch.zeros(8, dtype=torch.float64, device=_dev())
    g = torch.zeros((8, 8), dtype=torch.float64, device=_dev())
    for rows in ([0, 6], [-1], [1.5]):
        with pytest.raises(L.CgsError):
            K.pool_moments(x, s, g, rows=np.asarray(rows))
    with pytest.raises(L.CgsError):
        K.pool_moments(torch.ones((8, 6), dtype=torch.float32, device=_dev()).t(), s, g)       # non-contiguous
    with pytest.raises(L.CgsError):
        K.pool_moments(x.double(), s, g)
    with pytest.raises(L.CgsError):
        K.pool_moments(x.cpu(), s, g)
    with pytest.raises(L.CgsError):
        K.pool_moments(x, s.float(), g)
    with pytest.raises(L.CgsError):
        K.pool_moments(torch.ones((2, 2049), dtype=torch.float32, device=_dev()), torch.zeros(2049, dtype=torch.float64, device=_dev()),
                       torch.zeros((2049, 2049), dtype=torch.float64, device=_dev()))
    torch.cuda.synchronize()
    assert not s.any() and not g.any()                       # nothing was launched


def test_pool_moments_object_streams_batches_and_fixes_its_shift_on_the_first():
    """metrics.PoolMoments: three unequal batches, the second through a row list; shift = the first batch's fp32 column mean; the
    finalised mean / covariance against np.mean / np.cov of the rows it saw (1e-10 of max|cov|, the bar of the CPU merge test)."""
    from cgs_amd.metrics import PoolMoments, moments_mean_cov
    x, _, _, _ = _case(1000, 130)
    pm = PoolMoments(130, _dev())
    rows = np.random.RandomState(3).permutation(400)[:250]
    pm.update(torch.from_numpy(x[:300].copy()).to(_dev()))
    pm.update(torch.from_numpy(x[300:700].copy()).to(_dev()), rows)
    pm.update(torch.from_numpy(x[700:].copy()).to(_dev()))
    seen = np.concatenate([x[:300], x[300:700][rows], x[700:]]).astype(np.float64)
    st = pm.state()
    assert st["n"] == pm.n == 850
    assert np.allclose(st["shift"], x[:300].mean(0), rtol=1e-6)
    mean, cov = moments_mean_cov(st)
    ref_cov = np.cov(seen, rowvar=False)
    assert np.abs(mean - seen.mean(0)).max() < 1e-10 * np.abs(seen.mean(0)).max()
    assert np.abs(cov - ref_cov).max() < 1e-10 * np.abs(ref_cov).max()


def test_all_reduce_moments_on_rccl_world1_is_the_local_state():
    """metrics.all_reduce_moments under "nccl" at the one world size a 1-GPU box holds: broadcast + all-reduce of device tensors."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    code = (
        "import os, sys, numpy as np, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from cgs_amd.metrics import PoolMoments, all_reduce_moments, moments_of\n"
        f"os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='{port}', RANK='0', WORLD_SIZE='1')\n"
        "dev = torch.device('cuda:0'); torch.cuda.set_device(dev)\n"
        "x = (3 + np.random.RandomState(0).randn(200, 20)).astype(np.float32)\n"
        "pm = PoolMoments(20, dev).update(torch.from_numpy(x).to(dev))\n"
        "local = all_reduce_moments(pm)\n"                      # no process group: the identity
        "dist.init_process_group('nccl', device_id=dev)\n"
        "st = all_reduce_moments(pm)\n"
        "assert st['n'] == 200 and all(np.array_equal(st[k], local[k]) for k in ('shift', 'sum', 'gram'))\n"
        "ref = moments_of(x, local['shift'])\n"
        "assert np.abs(st['gram'] - ref['gram']).max() < 1e-10 * np.abs(ref['gram']).max()\n"
        "dist.destroy_process_group(); print('RCCL_OK')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "RCCL_OK" in out.stdout, out.stderr[-3000:]
