"""The loss seeds of the fused refiner and of the D / G training steps, shape by shape: cgs_refine_loss_seed, cgs_linear_out1_seed,
cgs_gan_logits_grad, cgs_gan_loss (csrc/elementwise.hip, api.hip, wgrad.hip)."""
import math

import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED_SHAPES = [(B, P) for B in (1, 3, 4, 5, 129) for P in (1, 5, 63, 64, 65, 900)]


def dev():
    return torch.device("cuda:0")


def seed_dlogits_f32(kind, l):
    """The kernel's own float32 expression (lsq, linear)."""
    return {"lsq": lambda: F32(2.0) * (l - F32(1.0)), "linear": lambda: np.full_like(l, -1.0)}[kind]()


def ladam_state_f32(s_real, sig, avg, first):
    """ladam_seed1 in numpy float32, operation by operation."""
    loss = F32(s_real) - sig
    avg = loss if first else F32(0.5) * avg + F32(0.5) * loss
    c = np.minimum(np.maximum(avg + F32(0.5), F32(0.0)), F32(10000.0))
    return avg, c * c


@pytest.mark.parametrize("B,P", SEED_SHAPES)
def test_refine_loss_seed(B, P):
    from cgs_amd import kernels as K
    d = dev()
    l = LC.make_logits((B, P), 100 * B + P)
    lg = torch.from_numpy(l).to(d)
    dl0, lm0 = K.bce_ones_grad_rowmean(lg)
    sig0 = K.sigmoid_rowmean(lg).reshape(B)
    for kind in LC.REFINE_KINDS:
        dl, lm = K.refine_loss_seed(lg, kind)
        assert torch.equal(lm, lm0), kind                                   # the selection does not depend on the loss
        if kind == "bce":
            assert torch.equal(dl, dl0)
        else:
            assert np.array_equal(dl.cpu().numpy(), seed_dlogits_f32(kind, l)), kind
        # float64: 3 roundings at most (bce: exp, sum, quotient, each correctly rounded or within 2 ulp)
        want = LC.refine_dlogits(kind, l)
        assert np.abs(dl.cpu().numpy() - want).max() <= 6 * LC.U * max(np.abs(want).max(), 1e-30), kind
        # with the ladam state: the same dlogits and mean, the state from the score of cgs_sigmoid_rowmean, two steps
        st = K.LadamState(B, d)
        st.set_real(0.6)
        avg = None
        for first, s_real in ((True, 0.6), (False, torch.tensor(0.25, device=d))):
            st.set_real(s_real)
            dl2, lm2 = K.refine_loss_seed(lg, kind, ladam=st, first=first)
            assert torch.equal(dl2, dl) and torch.equal(lm2, lm0), kind
            avg, gain = ladam_state_f32(float(s_real), sig0.cpu().numpy(), avg, first)
            assert np.array_equal(st.loss_avg.cpu().numpy(), avg) and np.array_equal(st.gain.cpu().numpy(), gain), (kind, first)
        dl3, lm3 = K.refine_loss_seed(lg, kind)                             # reruns are bit-equal
        assert torch.equal(dl3, dl) and torch.equal(lm3, lm)


def test_refine_loss_seed_refuses_bad_arguments():
    from cgs_amd import kernels as K, lib
    lg = torch.zeros(2, 3, device=dev())
    with pytest.raises(lib.CgsError):
        K.refine_loss_seed(lg, "hinge")
    with pytest.raises(lib.CgsError):
        lib.call("cgs_refine_loss_seed", lg.data_ptr(), 7, lg.data_ptr(), lg.data_ptr(), 2, 3, None, None)


@pytest.mark.parametrize("B", (1, 4, 5))
@pytest.mark.parametrize("Kin", (1024, 1030))
def test_linear_out1_seed_equals_its_parts(B, Kin):
    from cgs_amd import kernels as K
    d = dev()
    rs = np.random.RandomState(B * Kin)
    x = torch.from_numpy(rs.randn(B, Kin).astype(F32)).to(d)
    w = torch.from_numpy((0.1 * rs.randn(Kin, 1)).astype(F32)).to(d)
    b = torch.from_numpy(rs.randn(1).astype(F32)).to(d)
    y = K.linear_fwd(x, w, b)
    for kind in LC.REFINE_KINDS:
        for with_ladam in (False, True):
            sa, sb = (K.LadamState(B, d), K.LadamState(B, d)) if with_ladam else (None, None)
            for st in (sa, sb):
                if st is not None:
                    st.set_real(0.7)
                    st.loss_avg.copy_(torch.linspace(-2.0, 2.0, B, device=d))
            dl, lm = K.refine_loss_seed(y, kind, ladam=sa, first=False)
            y2, dl2, lm2 = torch.empty_like(y), torch.empty_like(y), torch.empty(B, device=d)
            K.linear_out1_seed(x, w, b, y2, dl2, lm2, kind, ladam=sb, first=False)
            assert torch.equal(y, y2) and torch.equal(dl, dl2) and torch.equal(lm, lm2), (kind, with_ladam)
            if with_ladam:
                assert torch.equal(sa.loss_avg, sb.loss_avg) and torch.equal(sa.gain, sb.gain), kind


def loss_sum_bound(kind, l, target, scale):
    """|loss_sum - float64| of cgs_gan_logits_grad: each thread adds ceil(n / 256) terms in turn, the block's tree
    adds 8 levels: A = ceil(n / 256) - 1 + 8 additions on any path, each at most U of the partial sum, which sum |e_i| bounds.  A term
    carries at most 3 U of its own ((l - t) rounded, then squared: 2 U, and the square's rounding; hinge 1, linear 0), the final product
    with scale 2 U (scale's own rounding, the product)."""
    n = l.size
    A = math.ceil(n / 256) - 1 + 8
    return 1.001 * (A + 3 + 2) * LC.U * scale * np.abs(LC.d_loss(kind, l, target)).sum()


@pytest.mark.parametrize("n", (1, 255, 256, 257, 7200))
def test_gan_logits_grad(n):
    from cgs_amd import kernels as K
    d = dev()
    l = LC.make_logits((n,), n)
    lg = torch.from_numpy(l).to(d)
    scale = 1.0 / n
    for kind, target in (("lsq", 1.0), ("lsq", 0.0), ("hinge", 1.0), ("hinge", 0.0), ("linear", 1.0), ("bce", 1.0), ("bce", 0.0)):
        loss = torch.zeros(1, device=d)
        dl = K.gan_logits_grad(lg, kind, target, scale, loss=loss)
        if kind == "bce":
            loss0 = torch.zeros(1, device=d)
            assert torch.equal(dl, K.bce_logits_grad(lg, target, scale, loss=loss0)) and torch.equal(loss, loss0)
            continue
        s, t = F32(scale), F32(target)
        want = {"lsq": lambda: s * (F32(2.0) * (l - t)),
                "hinge": lambda: s * (np.where(l < 1, F32(-1), F32(0)) if target == 1.0 else np.where(l > -1, F32(1), F32(0))).astype(F32),
                "linear": lambda: np.full_like(l, -s)}[kind]()
        assert np.array_equal(dl.cpu().numpy(), want), (kind, target)
        ref = scale * LC.d_loss(kind, l, target).sum()
        err, bound = abs(float(loss.item()) - ref), loss_sum_bound(kind, l, target, scale)
        print(f"gan_logits_grad {kind} t={target} n={n}: |loss_sum - f64| = {err:.3e}, bound {bound:.3e}, fraction {err / max(bound, 1e-300):.3f}")
        assert err <= bound, (kind, target, err, bound)
        # unreduced twin (ops.least_squares_loss / hinge_loss): the same formulas per logit, forward and backward
        e = K.gan_loss(lg, kind, target)
        assert np.abs(e.cpu().numpy() - LC.d_loss(kind, l, target)).max() <= 3 * LC.U * max(np.abs(LC.d_loss(kind, l, target)).max(), 1e-30)
        up = torch.full_like(lg, scale)
        assert torch.equal(K.gan_loss(lg, kind, target, dloss=up), dl), (kind, target)
        loss2 = torch.zeros(1, device=d)
        assert torch.equal(K.gan_logits_grad(lg, kind, target, scale, loss=loss2), dl) and torch.equal(loss, loss2)      # reruns
    from cgs_amd import lib
    with pytest.raises(lib.CgsError):
        K.gan_logits_grad(lg, "hinge", 0.5, scale)


def test_operator_losses_have_autograd():
    from cgs_amd import ops
    d = dev()
    l = LC.make_logits((6, 9), 4)
    for fn, kind, target in ((lambda t: ops.least_squares_loss(t, 1.0), "lsq", 1.0), (lambda t: ops.least_squares_loss(t, 0.0), "lsq", 0.0),
                             (lambda t: ops.hinge_loss(t, True), "hinge", 1.0), (lambda t: ops.hinge_loss(t, False), "hinge", 0.0),
                             (lambda t: ops.hinge_loss(t), "linear", 1.0)):
        t = torch.from_numpy(l).to(d).requires_grad_(True)
        out = fn(t)
        assert tuple(out.shape) == l.shape
        (g,) = torch.autograd.grad(out.sum(), t)
        want_e, want_g = LC.d_loss(kind, l, target), LC.d_dlogits(kind, l, target)
        assert np.abs(out.detach().cpu().numpy() - want_e).max() <= 3 * LC.U * np.abs(want_e).max()
        assert np.abs(g.cpu().numpy() - want_g).max() <= 2 * LC.U * np.abs(want_g).max()
