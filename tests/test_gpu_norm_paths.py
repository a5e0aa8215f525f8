"""Every form of every norm (+ lrelu) entry point of csrc/bn.hip against the float64 definitions of tests/norm_cases.py, on inputs
that pin the form: each case first asserts the path name the entry point left in cgs_last_kernel (include/cgs_hip.h: norm_small,
norm_passes, norm_fa, norm_finalize, norm_sliced, + _fwd / _bwd), then compares with the reference by test_gpu_ops.close().

From x the bars are the project's own for these ops: statistics and y 1e-5, dx 5e-5.  One channel of every case is constant: its
dx is ~1/sqrt(eps) = 316 times the other channels', so close() -- relative to the largest reference value -- is applied to that channel and to
the others separately; one bar over both would be 300 times laxer for the ordinary channels.
From partial rows the statistics are the float64 sum of the same float32 rows and one rounding to float32: 1e-6 relative per channel.
The rows are synthetic (not sums of x) with NaN in every row no group owns: a mis-addressed row changes the statistics or leaves NaN."""
import numpy as np
import pytest
import torch

import norm_cases as NC
from test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu


def rel_close(got, want, tol):
    got, want = got.detach().cpu().double(), want.double()
    err = ((got - want).abs() / want.abs()).max().item()
    assert err <= tol, f"max relative delta {err:.3e} (tol {tol})"


def no_nan(*tensors):
    for t in tensors:
        assert not bool(t.isnan().any())


def nan_stats(groups, C, d, flat):
    shape = (C,) if flat else (groups, C)
    return torch.full(shape, float("nan"), device=d), torch.full(shape, float("nan"), device=d)


def close_split(got, want, tol, c0):
    """close() on the constant channel and on the other channels separately (module docstring)."""
    C = want.shape[-1]
    reg = torch.tensor([c for c in range(C) if c != c0])
    close(got.detach().cpu()[..., reg], want[..., reg], tol)
    close(got.detach().cpu()[..., c0], want[..., c0], tol)


def x_params():
    return [pytest.param(kind, groups, M, C, path, leak, id=f"{kind}-{groups}x{M}x{C}-{path}-leak{leak}")
            for kind, groups, M, C, path, leaks in NC.FROM_X for leak in leaks]


@pytest.mark.parametrize("kind,groups,M,C,path,leak", x_params())
def test_norm_from_x(kind, groups, M, C, path, leak):
    from cgs_amd import kernels as K, lib
    d = dev()
    inp = NC.build_inputs(groups, M, C, leak)
    flat = kind == "bn"
    shape = (M, C) if flat else (groups, M, C)
    x, dy, gam, bet = inp.x.reshape(shape).to(d), inp.dy.reshape(shape).to(d), inp.gamma.to(d), inp.beta.to(d)
    fwd = K.bn_train_lrelu_fwd if flat else K.instnorm_lrelu_fwd
    bwd = K.bn_train_lrelu_bwd_data if flat else K.instnorm_lrelu_bwd_data
    c0 = inp.const_c
    reg = torch.tensor([c for c in range(C) if c != c0])

    # forward
    y, mean, invstd = fwd(x, gam, bet, leak, stats=nan_stats(groups, C, d, flat))
    assert lib.last_kernel() == path + "_fwd", lib.last_kernel()
    no_nan(y, mean, invstd)                                          # (the saved statistics are written for every group)
    mean64, _, invstd64 = NC.stats_from_x(inp.x)
    want_y = NC.ref_fwd(inp.x, inp.gamma, inp.beta, mean64, invstd64, leak)
    gm, gi, gy = mean.cpu().reshape(groups, C), invstd.cpu().reshape(groups, C), y.cpu().reshape(groups, M, C)
    if C > 1 and reg.numel():
        close(gm[:, reg], mean64[:, reg], 1e-5)
        close(gi[:, reg], invstd64[:, reg], 1e-5)
        close(gy[..., reg], want_y[..., reg], 1e-5)
    # the constant channel: float32 sums of 0.5 and 0.25 are exact, so mean == 0.5 and var == 0 exactly and invstd is 1/sqrt(eps) rounded once
    assert bool((gm[:, c0] == NC.CONST).all())
    rel_close(gi[:, c0], invstd64[:, c0], 2.0 ** -23)
    # ... and y = lrelu(beta) up to the rounding of shift = beta - mean * scale, |shift| ~ 0.5 * gamma * invstd ~ 158: half an ulp of it,
    # plus the roundings of the results themselves (|y| < 1: 2^-24 each for the fma and the leak product)
    half_ulp = float(np.spacing(np.float32(0.5 * abs(float(inp.gamma[c0])) * float(invstd64[0, c0]) + abs(float(inp.beta[c0]))))) / 2
    err = (gy[..., c0].double() - want_y[..., c0]).abs().max().item()
    assert err <= half_ulp + 2.0 ** -23, (err, half_ulp)

    # backward, from the float32 mean / invstd of the case (the rounded float64 statistics of x), not from the forward above
    mean32, invstd32 = inp.mean.reshape(mean.shape).to(d), inp.invstd.reshape(mean.shape).to(d)
    dx = bwd(dy, x, gam, bet, mean32, invstd32, leak)
    assert lib.last_kernel() == path + "_bwd", lib.last_kernel()
    no_nan(dx)
    want_dx = NC.ref_bwd(inp.dy, inp.x, inp.gamma, inp.beta, inp.mean, inp.invstd, leak)
    close_split(dx.reshape(groups, M, C), want_dx, 5e-5, c0)

    # bit-identical over two runs
    y2, mean2, invstd2 = fwd(x, gam, bet, leak)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(invstd, invstd2)
    assert torch.equal(dx, bwd(dy, x, gam, bet, mean32, invstd32, leak))


def p_params():
    return [pytest.param(*case[:7], leak, id="g{}-r{}x{}s{}-{}x{}-{}-leak{}".format(*case[:7], leak)) for case in NC.FROM_PARTIALS for leak in case[7]]


@pytest.mark.parametrize("groups,rows,nseg,stride,M,C,path,leak", p_params())
def test_norm_fwd_from_partials(groups, rows, nseg, stride, M, C, path, leak):
    from cgs_amd import kernels as K, lib
    d = dev()
    inp = NC.build_inputs(groups, M, C, leak)
    p = NC.build_partials(groups, rows, nseg, stride, C, M)
    x, gam, bet, part = inp.x.to(d), inp.gamma.to(d), inp.beta.to(d), p.part.to(d)
    mean64, invstd64 = NC.stats_from_partials(p)
    want_y = NC.ref_fwd(inp.x, inp.gamma, inp.beta, mean64, invstd64, leak)

    def check(y, mean, invstd, name):
        assert lib.last_kernel() == name, (lib.last_kernel(), name)
        no_nan(y, mean, invstd)                                      # a gap row read, or a group's statistics not written
        rel_close(mean.reshape(groups, C), mean64, 1e-6)
        rel_close(invstd.reshape(groups, C), invstd64, 1e-6)
        close(y.reshape(groups, M, C), want_y, 1e-5)

    # the group form never slices: one-stage finalize whatever the row count
    name = (path if path != "norm_sliced" else "norm_finalize") + "_fwd"
    run = lambda: K.groupnorm_lrelu_fwd_from_partials(x, part, p.layout, groups, gam, bet, leak, stats=nan_stats(groups, C, d, False))
    got = run()
    check(*got, name)
    assert all(torch.equal(a, b) for a, b in zip(got, run()))
    if groups == 1 and nseg == 1:                                    # the batch-norm form of the same rows
        run = lambda: K.bn_train_lrelu_fwd_from_partials(x.reshape(M, C), part, gam, bet, leak, stats=nan_stats(1, C, d, True))
        got = run()
        check(*got, path + "_fwd")
        assert all(torch.equal(a, b) for a, b in zip(got, run()))


@pytest.mark.parametrize("groups,rows,nseg,stride,M,C,path,leak", p_params())
def test_norm_bwd_from_partials(groups, rows, nseg, stride, M, C, path, leak):
    from cgs_amd import kernels as K, lib
    d = dev()
    inp = NC.build_inputs(groups, M, C, leak)
    p = NC.build_partials(groups, rows, nseg, stride, C, M, seed=1)
    x, dy, gam, bet, part = inp.x.to(d), inp.dy.to(d), inp.gamma.to(d), inp.beta.to(d), p.part.to(d)
    m1, m2 = NC.partial_sums(p)
    nstat = K.NormBwdStats(x, inp.mean.to(d), inp.invstd.to(d), gam, bet, leak, 1, part, p.layout)
    dx = K.norm_lrelu_bwd_from_partials(dy, x, nstat, groups)
    assert lib.last_kernel() == path + "_bwd", lib.last_kernel()
    no_nan(dx)
    want = NC.ref_bwd(inp.dy, inp.x, inp.gamma, inp.beta, inp.mean, inp.invstd, leak, m1, m2)
    close_split(dx, want, 5e-5, inp.const_c)
    # in place (dx is dy), which is also the second run: bit-identical
    buf = dy.clone()
    out = K.norm_lrelu_bwd_from_partials(buf, x, nstat, groups, out=buf)
    assert out is buf and torch.equal(buf, dx)

    # m1 / m2 themselves, read through dx: with dy = 0, gamma = invstd = 1, mean = 0 the kernel returns dx = -(m1 + x * m2), so the row
    # x = 0 holds -m1 exactly and the row x = 1 holds -(m1 + m2) rounded once: m2 to 2^-24 * (|m1| + |m2|) / |m2| < 2e-7 (|m1| <= 1, m2 >= 0.5)
    xp = torch.zeros((groups, M, C), device=d)
    xp[:, 1] = 1.0
    one, zero = torch.ones(C, device=d), torch.zeros((groups, C), device=d)
    probe = K.NormBwdStats(xp, zero, torch.ones((groups, C), device=d), one, one, leak, 1, part, p.layout)
    dp = K.norm_lrelu_bwd_from_partials(torch.zeros_like(xp), xp, probe, groups).cpu().double()
    assert lib.last_kernel() == path + "_bwd", lib.last_kernel()
    no_nan(dp)
    rel_close(-dp[:, 0], m1, 1e-6)
    rel_close(dp[:, 0] - dp[:, 1], m2, 1e-6)
