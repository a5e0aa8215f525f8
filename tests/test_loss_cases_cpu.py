"""The float64 definitions of tests/loss_cases.py against float64 torch autograd and the oracle's Policy (no GPU)."""
import numpy as np
import pytest
import torch

import loss_cases as LC
from oracle import sampling_ref as S


def test_logit_builder_keeps_clear_of_the_hinge_kinks():
    for shape in ((1, 1), (5, 63), (129, 900)):
        l = LC.make_logits(shape, 3)
        assert l.dtype == np.float32 and l.shape == shape
        assert np.abs(np.abs(l.astype(np.float64)) - 1.0).min() >= LC.KINK_MARGIN
        if l.size >= 2:
            assert l.max() == 40.0 and l.min() == -40.0


@pytest.mark.parametrize("kind", LC.REFINE_KINDS)
def test_refine_losses_against_autograd(kind):
    l = torch.from_numpy(LC.make_logits((7, 33), 11).astype(np.float64)).requires_grad_(True)
    loss = {"bce": lambda: torch.nn.functional.softplus(-l), "lsq": lambda: (l - 1.0) ** 2, "linear": lambda: -l}[kind]()
    (g,) = torch.autograd.grad(loss.sum(), l)
    np.testing.assert_allclose(LC.refine_loss(kind, l.detach().numpy()), loss.detach().numpy(), rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(LC.refine_dlogits(kind, l.detach().numpy()), g.numpy(), rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("target", (1.0, 0.0))
@pytest.mark.parametrize("kind", LC.D_KINDS + ("linear",))
def test_training_losses_against_autograd(kind, target):
    l = torch.from_numpy(LC.make_logits((257,), 5).astype(np.float64)).requires_grad_(True)
    t = torch.full_like(l, target)
    loss = {"bce": lambda: torch.nn.functional.binary_cross_entropy_with_logits(l, t, reduction="none"),
            "lsq": lambda: (l - t) ** 2,
            "hinge": lambda: torch.relu(1.0 - l) if target == 1.0 else torch.relu(1.0 + l),
            "linear": lambda: -l}[kind]()
    (g,) = torch.autograd.grad(loss.sum(), l)
    # (torch's cross entropy adds and subtracts |l| <= 40 around log1p: absolute error up to a few 40 * 2^-53)
    np.testing.assert_allclose(LC.d_loss(kind, l.detach().numpy(), target), loss.detach().numpy(), rtol=1e-12, atol=4e-14)
    np.testing.assert_allclose(LC.d_dlogits(kind, l.detach().numpy(), target), g.numpy(), rtol=1e-12, atol=1e-17)


def test_ladam_step_against_the_oracle_policy_and_autograd_free_formula():
    rs = np.random.RandomState(0)
    B, shape = 5, (5, 3, 2, 4)
    theta = rs.randn(*shape)
    pol = S.Policy(0.1, "ladam")
    m = v = avg = None
    th_ref = torch.from_numpy(theta.copy())
    for i in range(3):
        g = rs.randn(*shape) * 0.1
        loss = rs.randn(B) * 0.3 + (4e4 if i == 1 else 0.0) * (np.arange(B) == 2) - 3.0 * (np.arange(B) == 1)
        th_ref = pol.step(th_ref, torch.from_numpy(g), torch.from_numpy(loss))
        avg, gain = LC.ladam_state(loss, avg, i == 0)
        theta, m, v = LC.ladam_step(theta, m, v, g, gain, 0.1, i == 0, c1=1.0 - LC.B1, c2=1.0 - LC.B2)
        assert gain[1] == 0.0 and (i != 1 or gain[2] == 1e8)                  # both ends of the clamp are visited
        np.testing.assert_allclose(theta, th_ref.numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(avg, pol.l.numpy(), rtol=1e-14)
    # the clip of collaborator.py:69-70 and the fp32 (1 - beta) factors the kernel is handed
    out, _, _ = LC.ladam_step(theta, m, v, g, gain, 0.1, False, 0.05, 0.5)
    assert out.min() >= 0.05 and out.max() <= 0.5
    assert abs(LC.C1 - 0.1) < 2.0 ** -27 and LC.C2 == 0.5


def test_ladam_bound_is_positive_and_small():
    rs = np.random.RandomState(1)
    th, g = rs.randn(3, 7).astype(np.float32), rs.randn(3, 7).astype(np.float32)
    bound = LC.ladam_bound(th, None, None, g, np.ones(3), 0.1, True)
    assert (bound > 0).all() and bound.max() < 1e-5
