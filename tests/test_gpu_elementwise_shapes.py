"""The element-wise kernels of csrc/elementwise.hip at the sizes their launch plan turns on, and the row selects on the scalar branch of
copy_row.

Every GRID_STRIDE kernel is launched with at most 8192 blocks of 256 threads (ew_blocks): 2 097 152 = 2^21 threads, so a thread takes a
second element only from n = 2^21 + 1 on.  BIG = 2 * 2^21 + 3 elements: the second turn whole, a third turn of 3 elements.

    kernel                              big case                                              bar (the one in force for the op, file named)
    unary_kernel<0,1>  lrelu fwd / bwd  n = BIG                                               bit-equal (the product is the only rounding)
    unary_kernel<2,3>  tanh fwd / bwd   n = BIG                                               1e-5 max|ref|   (test_gpu_ops.py)
    affine_relu_kernel<0,1>             M = ceil(BIG / C) rows, C in {1, 12, 64}              1e-5 max|ref|   (test_gpu_ops.py)
    affine_kernel<0,1>                  the same shapes                                       1e-6 max|ref|   (test_gpu_train_kernels.py)
    loss_unary_kernel<0,1> bce_ones     n = BIG                                               1e-6 max|ref|   (test_gpu_train_kernels.py)
    loss_unary_kernel<2>   clip         n = BIG                                               bit-equal
    gan_loss_kernel<lsq, hinge, linear> n = BIG, with and without dloss                       3 U max|ref| / bit-equal (test_gpu_loss_seed.py)
    add_kernel                          n = BIG                                               bit-equal
    refine_update_kernel                n = BIG, first / not first, with clip                 bit-equal       (test_gpu_ops.py)
    refine_update_ladam_kernel<true>    B x F = 4099 x 4096: 2 * 2^21 + 3072 float4           loss_cases.ladam_bound (test_gpu_ladam_update.py)
    refine_update_ladam_kernel<false>   B x F = 4101 x 1023 (F % 4 != 0): > BIG floats        the same

copy_row's scalar branch (F % 4 != 0, or a base that is not 16-byte aligned) under refine_select, refine_select_rows and
refine_select2 with and without tickets: rows of 75 and 63 floats, and rows of 100 and 64 floats whose source, destination or both
start one float past an aligned address; deterministic and forced mode; bit-equal to the torch.where statement, tickets back at zero.
"""
import numpy as np
import pytest
import torch

import loss_cases as LC
from test_gpu_train_kernels import close, planted_logits, rnd

pytestmark = pytest.mark.gpu

F32 = np.float32
BIG = 2 * (1 << 21) + 3
SIZES = [1, 255, 257, BIG]
NAN = float("nan")


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nans(shape):
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), NAN, dtype=torch.float32, device=dev())


def same_bits(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    assert torch.equal(got, want), (what, int((got != want).sum()), int((got != want).flatten().nonzero()[0]) if (got != want).any() else -1)


@pytest.mark.parametrize("n", SIZES)
def test_lrelu_and_tanh(n):
    from cgs_amd import kernels as K
    d = dev()
    x, dy = planted_logits(n, 80 + n % 7), rnd((n,), 81)
    leak = float(F32(0.2))
    yl = K.lrelu_fwd(x.to(d), out=nans(n))
    same_bits(yl, torch.maximum(x.double(), leak * x.double()).float(), f"lrelu_fwd n={n}")
    same_bits(K.lrelu_bwd(dy.to(d), yl, out=nans(n)), (dy.double() * torch.where(yl.cpu() > 0, 1.0, leak).double()).float(), f"lrelu_bwd n={n}")
    yt = K.tanh_fwd(x.to(d), out=nans(n))
    close(yt, torch.tanh(x.double()), 1e-5, f"tanh_fwd n={n}")
    close(K.tanh_bwd(dy.to(d), yt, out=nans(n)), dy.double() * (1.0 - yt.cpu().double() ** 2), 1e-5, f"tanh_bwd n={n}")


@pytest.mark.parametrize("C", [1, 12, 64])
@pytest.mark.parametrize("n", SIZES)
def test_affine_relu_and_affine(n, C):
    """M = ceil(n / C) rows, so that the big case passes 2 * 2^21 elements at every C."""
    from cgs_amd import kernels as K
    d = dev()
    M = -(-n // C)
    x = planted_logits(M * C, 90 + C).reshape(M, C)
    a, b, dy = rnd((C,), 91), rnd((C,), 92), rnd((M, C), 93)
    xd, ad, bd, dyd = x.to(d), a.to(d), b.to(d), dy.to(d)
    y = K.affine_relu_fwd(xd, ad, bd, out=nans((M, C)))
    close(y, torch.relu(a.double() * x.double() + b.double()), 1e-5, f"affine_relu_fwd {M}x{C}")
    close(K.affine_relu_bwd(dyd, y, ad, out=nans((M, C))), dy.double() * (y.cpu() > 0) * a.double(), 1e-5, f"affine_relu_bwd {M}x{C}")
    close(K.affine_fwd(xd, ad, bd, out=nans((M, C))), a.double() * x.double() + b.double(), 1e-6, f"affine_fwd {M}x{C}")
    close(K.affine_bwd(dyd, ad, out=nans((M, C))), dy.double() * a.double(), 1e-6, f"affine_bwd {M}x{C}")


@pytest.mark.parametrize("huge", [True, False])
def test_bce_ones_past_the_second_turn(huge):
    """(n = 1, 255, 257 and 2^20: tests/test_gpu_train_kernels.py::test_bce_ones_fwd_and_bwd, whose bar and inputs these are.)"""
    from cgs_amd import kernels as K
    d = dev()
    l, dy = planted_logits(BIG, 60, huge), rnd((BIG,), 61)
    ld = l.to(d)
    close(K.bce_ones_fwd(ld, out=nans(BIG)), torch.nn.functional.softplus(-l.double()), 1e-6, "bce_ones_fwd")
    close(K.bce_ones_bwd(dy.to(d), ld, out=nans(BIG)), -dy.double() * torch.sigmoid(-l.double()), 1e-6, "bce_ones_bwd")


@pytest.mark.parametrize("n", SIZES)
def test_gan_loss_clip_and_add(n):
    from cgs_amd import kernels as K
    d = dev()
    l = LC.make_logits((n,), 7 + n % 11)
    up = (np.random.RandomState(n % 13).randn(n)).astype(F32)
    lg, upd = torch.from_numpy(l).to(d), torch.from_numpy(up).to(d)
    for kind, target in (("lsq", 1.0), ("lsq", 0.0), ("hinge", 1.0), ("hinge", 0.0), ("linear", 1.0)):
        want = LC.d_loss(kind, l, target)
        e = K.gan_loss(lg, kind, target, out=nans(n)).cpu().numpy()
        assert np.isfinite(e).all() and np.abs(e - want).max() <= 3 * LC.U * max(np.abs(want).max(), 1e-30), (kind, target)
        t = F32(target)
        dd = {"lsq": lambda: F32(2.0) * (l - t),
              "hinge": lambda: (np.where(l < 1, F32(-1), F32(0)) if target == 1.0 else np.where(l > -1, F32(1), F32(0))).astype(F32),
              "linear": lambda: np.full_like(l, -1.0)}[kind]()
        same_bits(K.gan_loss(lg, kind, target, dloss=upd, out=nans(n)), torch.from_numpy(up * dd), f"gan_loss {kind} t={target} with dloss n={n}")
    x, y = planted_logits(n, 31), rnd((n,), 32, 50.0)
    same_bits(K.clip(x.to(d), -0.75, 2.5, out=nans(n)), torch.clamp(x, -0.75, 2.5), f"clip n={n}")
    same_bits(K.add(x.to(d), y.to(d), out=nans(n)), x + y, f"add n={n}")


@pytest.mark.parametrize("n", SIZES)
def test_refine_update(n):
    """first / not first, with and without the clip: bit-equal to the reference's separately rounded operations (policy.py:33-36)."""
    from cgs_amd import kernels as K
    d = dev()
    rs = np.random.RandomState(n % 17)
    th0, m0, g = (rs.randn(n).astype(F32) for _ in range(3))
    rate, alpha = F32(0.1), F32(0.9)
    for first, clip in ((True, False), (False, False), (True, True), (False, True)):
        th, m = torch.from_numpy(th0.copy()).to(d), (nans(n) if first else torch.from_numpy(m0.copy()).to(d))      # the first step must not use m
        K.refine_update(th, m, torch.from_numpy(g).to(d), 0.1, 0.9, first, *((0.05, 1.5) if clip else ()))
        mv = rate * g if first else alpha * m0 + rate * g
        want = th0 - mv
        if clip:
            want = np.minimum(np.maximum(want, F32(0.05)), F32(1.5))
        assert mv.dtype == F32 and want.dtype == F32
        same_bits(m, torch.from_numpy(mv), f"refine_update m n={n} first={first}")
        same_bits(th, torch.from_numpy(want), f"refine_update theta n={n} first={first} clip={clip}")


@pytest.mark.parametrize("B,F,first", [(4099, 4096, False), (4101, 1023, True), (4101, 1023, False)])
def test_ladam_update_past_the_second_turn(B, F, first):
    """The float4 form counts n / 4, so it needs 4 x as many floats (its float64 reference takes seconds on the host: only the step that
    reads m and v is run at that size); the sample index of an element ((i << 2) / F, i / F) is checked by a gain that differs per
    sample.  Bound and state bars: tests/test_gpu_ladam_update.py."""
    from cgs_amd import kernels as K
    d = dev()
    assert (B * F // 4 if F % 4 == 0 else B * F) > 2 * (1 << 21)
    rs = np.random.default_rng(B)
    theta = rs.standard_normal((B, F), dtype=F32)
    m, v = F32(0.1) * rs.standard_normal((B, F), dtype=F32), F32(0.01) * rs.random((B, F), dtype=F32)
    g = F32(0.1) * rs.standard_normal((B, F), dtype=F32)
    gain = (rs.random(B) * 2.0).astype(F32)
    gain[1], gain[B - 1] = 0.0, 1e8
    clip = not first
    vmin, vmax = (float(F32(0.05)), 1.5) if clip else (None, None)
    t, mm, vv = (torch.from_numpy(a).to(d) for a in (theta, m, v))
    if first:
        mm, vv = nans((B, F)), nans((B, F))
    K.refine_update_ladam(t, mm, vv, torch.from_numpy(g).to(d), torch.from_numpy(gain).to(d), 0.1, first, vmin, vmax)
    rate = float(F32(0.1))
    want, wm, wv = LC.ladam_step(theta, m, v, g, gain, rate, first, vmin, vmax)
    bound = LC.ladam_bound(theta, m, v, g, gain, rate, first)
    got = t.cpu().numpy()
    assert np.isfinite(got).all()
    frac = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print(f"ladam update B={B} F={F} first={first} clip={clip}: max |err| / bound = {frac:.3f}")
    assert frac <= 1.0
    assert np.abs(mm.cpu().numpy() - wm).max() <= 3 * LC.U * (np.abs(wm).max() + np.abs(g).max())
    assert np.abs(vv.cpu().numpy() - wv).max() <= 3 * LC.U * np.abs(wv).max()
    if not clip:
        assert np.array_equal(got[1], theta[1])                     # gain 0: the sample stands still, wherever the loop reaches it
    else:
        assert got.min() >= F32(0.05) and got.max() <= F32(1.5)


def _place(t, off):
    """A copy of ``t`` on the device that starts ``off`` floats past an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev())
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


SELECT_CASES = {"odd_rows": ((5, 5, 3), (3, 3, 7), 0, 0), "source_off": ((5, 5, 4), (4, 4, 4), 1, 0),
                "destination_off": ((5, 5, 4), (4, 4, 4), 0, 1), "both_off": ((5, 5, 4), (4, 4, 4), 1, 1)}


@pytest.mark.parametrize("mode", ["deterministic", "forced"])
@pytest.mark.parametrize("case", sorted(SELECT_CASES))
def test_row_selects_on_the_scalar_copy(case, mode):
    from cgs_amd import kernels as K
    d = dev()
    rshape, tshape, soff, doff = SELECT_CASES[case]
    B, step = 77, 2
    Fr, F = int(np.prod(rshape)), int(np.prod(tshape))
    assert (Fr % 4 != 0 and F % 4 != 0) or soff or doff            # copy_row's vec4 condition fails for both tensors
    rows, theta, logit, best = rnd((B,) + rshape, 4), rnd((B,) + tshape, 5), rnd((B,), 6), rnd((B,), 7)
    old_rows, old_theta = rnd((B,) + rshape, 8), rnd((B,) + tshape, 9)
    forced = torch.randint(0, 4, (B,), dtype=torch.int32, generator=torch.Generator().manual_seed(10)) if mode == "forced" else None
    upd = (forced == step) if forced is not None else (logit > best)
    assert upd.any() and not upd.all()
    want = [torch.where(upd.view(-1, 1, 1, 1), rows, old_rows), torch.where(upd.view(-1, 1, 1, 1), theta, old_theta),
            torch.where(upd, logit, best), torch.where(upd, torch.full_like(best, step + 1.0), torch.ones_like(best))]
    rows_d, theta_d, logit_d = _place(rows, soff), _place(theta, soff), logit.to(d)
    forced_d = None if forced is None else forced.to(d)

    def fresh():
        return [_place(old_rows, doff), _place(old_theta, doff), best.to(d), torch.ones(B, device=d)]

    def check(state, what):
        for got, w, name in zip(state, want, ("rows", "theta", "best_logit", "best_step")):
            same_bits(got, w, f"{case} {mode} {what}: {name}")
    a = fresh()
    K.refine_select_rows(rows_d, logit_d, forced_d, step, a[0], a[2])
    K.refine_select(theta_d, logit_d, forced_d, step, a[1], a[2], a[3])
    check(a, "select_rows + select")
    c = fresh()
    K.refine_select2(rows_d, c[0], theta_d, c[1], logit_d, forced_d, step, c[2], c[3])
    check(c, "select2")
    e = fresh()
    tickets = torch.zeros(B, dtype=torch.int32, device=d)
    for _ in range(2):          # (the second call selects nothing new in deterministic mode, the same rows in forced mode)
        K.refine_select2(rows_d, e[0], theta_d, e[1], logit_d, forced_d, step, e[2], e[3], tickets)
        check(e, "select2 with tickets")
        assert not tickets.any()
    for t, w in ((rows_d, rows), (theta_d, theta)):
        assert torch.equal(t.cpu(), w)                              # the sources are untouched
