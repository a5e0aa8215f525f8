"""tests/mlp2d_cases.py checked without a device: the float64 definitions against the float32 torch-CPU oracle (oracle.sampling_ref), the
5 % caps on rows dropped for a ReLU kink on every case, and the reference side of every measured bar of tests/test_gpu_mlp2d_narrow.py --
printed (run with -s), and asserted inside the bar that is 4x the figure mlp2d_cases records."""
import numpy as np
import pytest
import torch

import mlp2d_cases as M
from oracle import sampling_ref as S


def _torch_net(Ws, bs):
    return [torch.from_numpy(w) for w in Ws], [torch.from_numpy(b) for b in bs]


def test_saliency_oracle_vs_float64_and_kink_cap():
    """The float32 oracle against ref64 over SALIENCY x SCALES: the reference side of SALIENCY_BAR.  Every case keeps >= 95 % of its rows and
    has a saliency to compare (the one-unit net is dead on part of the plane, not on all of it)."""
    worst_sig = worst_sal = worst_drop = 0.0
    for nh, nl, B in M.SALIENCY:
        for scale in M.SCALES:
            Ws, bs, x, (sig, sal, near) = M.saliency_case(nh, nl, B, scale)
            keep = ~near
            assert near.mean() <= M.KINK_CAP, (nh, nl, B, scale, near.mean())
            assert np.abs(sal[keep]).max() > 0
            o_sig, o_sal = S.mlp_sigmoid_and_saliency(*_torch_net(Ws, bs), x)
            ds = np.abs(o_sig[keep, 0] - sig[keep]).max()
            dg = np.abs(o_sal[keep] - sal[keep]).max() / np.abs(sal[keep]).max()
            print(f"saliency {(nh, nl, B, scale)}: dropped {near.mean():.4f}  oracle max|d sigmoid| {ds:.3e}  max|d saliency|/max|saliency| {dg:.3e}")
            worst_sig, worst_sal, worst_drop = max(worst_sig, ds), max(worst_sal, dg), max(worst_drop, near.mean())
    print(f"SALIENCY: worst dropped {worst_drop:.4f}, oracle's worst |d sigmoid| {worst_sig:.3e}, saliency {worst_sal:.3e} "
          f"(recorded {M.ORACLE_SALIENCY:.1e}, bar {M.SALIENCY_BAR:.1e})")
    assert worst_sig <= M.SIGMOID_BAR and worst_sal <= M.SALIENCY_BAR


def test_ref64_saliency_is_the_gradient_of_the_mean_loss():
    """ref64's hand-written backward against float64 torch autograd of mean softplus(-logit) (synthetic/GAN.py:105-111)."""
    Ws, bs, x, (sig, sal, near) = M.saliency_case(33, 4, 1000, 2.0)
    Wd, bd = [torch.from_numpy(w).double() for w in Ws], [torch.from_numpy(b).double() for b in bs]
    xt = torch.from_numpy(x).double().requires_grad_(True)
    h = xt
    for i, (W, b) in enumerate(zip(Wd, bd)):
        h = h @ W + b
        if i + 1 < len(Wd):
            h = torch.relu(h)
    g = torch.autograd.grad(torch.nn.functional.softplus(-h, threshold=500.0).mean(), xt)[0].numpy()
    assert np.abs(torch.sigmoid(h).detach().numpy()[:, 0] - sig).max() <= 1e-14
    assert np.abs(g[~near] - sal[~near]).max() <= 1e-13 * np.abs(sal).max()
    np.testing.assert_allclose(M.ref64(Ws, bs, x, 0.25)[1], sal * 250.0, rtol=1e-14, atol=0)       # inv_batch replaces the 1 / B


@pytest.mark.parametrize("case", M.REFINE, ids=M.case_id)
def test_teacher_forced_states_the_refiner_rule(case):
    """The float32 restatement of refine2d_kernel on the oracle D, put through teacher_forced: every step within STEP_BAR of the float64
    prediction from its own previous point (a wrong constant, a state off from step 2 on, or a rule applied to the wrong method would
    miss it by orders of magnitude), at most 5 % of the rows near a kink along the trajectory, the recorded best point a minimum of
    the float64 losses up to the sigmoid's error."""
    nh, nl, B, K, method, rate, scale = case
    Ws, bs, x, base = M.refine_case(*case)
    traj, best, step = M.refine_f32(Ws, bs, x, base, K, rate, method)
    pred, loss64, near = M.teacher_forced(Ws, bs, traj, base, rate, method)
    keep = ~near
    assert near.mean() <= M.KINK_CAP, (case, near.mean())
    err = np.abs(traj[keep, 1:].astype(np.float64) - pred[keep, 1:]).max()
    moved = np.abs(traj[:, 1:] - traj[:, :1]).max(axis=(1, 2))
    print(f"refine {case}: dropped {near.mean():.4f}  oracle's worst one-step error {err:.3e} (bar {M.STEP_BAR:.1e})  "
          f"median / max distance moved {np.median(moved):.3e} / {moved.max():.3e}  rows with best_step > 0: {(step > 0).mean():.3f}")
    assert err <= M.STEP_BAR
    assert np.median(moved) > 100 * M.STEP_BAR          # the samples do move: the bar binds
    assert np.array_equal(best, traj[np.arange(B), step.astype(np.int64)])
    picked = loss64[np.arange(B), step.astype(np.int64)]
    assert (picked[keep] <= loss64[keep].min(axis=1) + 2 * M.DEVICE_SIGMOID).all()


@pytest.mark.parametrize("wrong", ["rate", "beta", "state", "gain"])
def test_teacher_forced_notices_a_wrong_rule(wrong):
    """The comparison has the power the issue asks of it: a float32 loop whose rule is off in one constant misses STEP_BAR."""
    nh, nl, B, K, method, rate, scale = case = M.REFINE[4]             # (33, 4, 1000, 10, ladam)
    Ws, bs, x, base = M.refine_case(*case)
    traj, _, _ = M.refine_f32(Ws, bs, x, base, K, rate, method)
    bad = {"rate": lambda: M.teacher_forced(Ws, bs, traj, base, rate * 1.001, method),
           "gain": lambda: M.teacher_forced(Ws, bs, traj, base + 1e-3, rate, method),
           "beta": lambda: M.teacher_forced(Ws, bs, traj, base, rate, "momentum"),
           "state": lambda: M.teacher_forced(Ws, bs, np.concatenate([traj[:, 1:2], traj[:, 1:]], axis=1), base, rate, method)}[wrong]()
    pred, _, near = bad
    lo = 2 if wrong == "state" else 1                   # ("state": the first point replaced, so every later state differs by a few 1e-4 ...)
    err = np.abs(traj[~near, lo:].astype(np.float64) - pred[~near, lo:]).max()
    print(f"wrong {wrong}: worst one-step error {err:.3e} against the bar {M.STEP_BAR:.1e}")
    assert err > M.STEP_BAR


def test_d_step64_vs_float32_oracle_and_kink_cap():
    """d_step64 against S.mlp_d_loss_and_grads (float32 torch autograd) over DSTEP: the reference side of DLOSS_BAR / DGRAD_BAR; no row of
    the batches handed out is near a kink, and at most 5 % of the candidates were."""
    worst_loss = worst_grad = 0.0
    for case in M.DSTEP:
        nl, nh, Br, Bf = case
        Ws, bs, real, fake, dropped = M.dstep_case(*case)
        assert real.shape == (Br, 2) and fake.shape == (Bf, 2) and dropped <= M.KINK_CAP, (case, dropped)
        lr, lf, dW, db, near_r, near_f = M.d_step64(Ws, bs, real, fake)
        assert not near_r.any() and not near_f.any()
        (olr, olf), ogW, ogb = S.mlp_d_loss_and_grads(*_torch_net(Ws, bs), real, fake)
        el = max(abs(olr - lr) / lr, abs(olf - lf) / lf)
        eg = max(np.abs(o.numpy() - w).max() / np.abs(w).max() for o, w in zip(ogW + ogb, dW + db))
        print(f"d step {case}: dropped {dropped:.4f}  oracle |d loss|/loss {el:.3e}  worst max|d grad|/max|grad| {eg:.3e}")
        worst_loss, worst_grad = max(worst_loss, el), max(worst_grad, eg)
    print(f"DSTEP: oracle's worst loss {worst_loss:.3e} (recorded {M.ORACLE_DLOSS:.1e}, bar {M.DLOSS_BAR:.1e}), "
          f"gradient {worst_grad:.3e} (recorded {M.ORACLE_DGRAD:.1e}, bar {M.DGRAD_BAR:.1e})")
    assert worst_loss <= M.DLOSS_BAR and worst_grad <= M.DGRAD_BAR
    assert M.DLOSS_BAR <= 2e-5 and M.DGRAD_BAR <= 2e-4


def test_d_step64_is_the_gradient_of_the_loss():
    """The explicit backward against float64 torch autograd."""
    Ws, bs, real, fake, _ = M.dstep_case(3, 63, 77, 130)
    lr, lf, dW, db, _, _ = M.d_step64(Ws, bs, real, fake)
    Wd, bd = [torch.from_numpy(w).double() for w in Ws], [torch.from_numpy(b).double() for b in bs]
    Wp, bp = [w.clone().requires_grad_(True) for w in Wd], [b.clone().requires_grad_(True) for b in bd]

    def logits(x):
        h = torch.from_numpy(x).double()
        for i, (W, b) in enumerate(zip(Wp, bp)):
            h = h @ W + b
            if i + 1 < len(Wp):
                h = torch.relu(h)
        return h
    a, b = logits(real), logits(fake)
    F = torch.nn.functional.binary_cross_entropy_with_logits
    l1, l2 = F(a, torch.ones_like(a)), F(b, torch.zeros_like(b))
    grads = torch.autograd.grad(l1 + l2, Wp + bp)
    assert abs(l1.item() - lr) <= 1e-14 and abs(l2.item() - lf) <= 1e-14
    for got, want in zip(dW + db, grads):
        assert np.abs(got - want.numpy()).max() <= 1e-13 * float(want.abs().max())
