"""The 64-unit 2-D discriminator kernels of csrc/mlp2d.hip -- the ones BASELINE config 1 runs -- shape by shape against the float64
definitions of tests/mlp2d_cases.py: mlp_saliency_kernel, refine2d_kernel (teacher-forced: one step deep, K times) and the D step
(mlp_train_fwdbwd_kernel / mlp_train_grad_kernel) through DShaper.  The generator's shapes are in tests/test_gpu_synthetic_train.py.

Bars: 4x what the float32 torch-CPU oracle shows against the same float64 definitions over the same tables (tests/mlp2d_cases.py records
it, tests/test_mlp2d_cases_cpu.py measures it); beside them what an MI355X measured, worst over each table:

    quantity                                      oracle      bar         device
    rows dropped for a ReLU kink                  <= 4.0 %    5 %         (the same rows: the float64 definition decides)
    |d sigmoid|                                   1.9e-6      2e-5        1.75e-6  at (64, 6, 4097) scale 2
    max|d saliency| / max|saliency|               2.39e-6     9.6e-6      1.68e-6  at (64, 6, 1) scale 1
    one refiner step, |d x|                       5.6e-6      2.2e-5      3.06e-6  at (64, 6, 1000, K = 10, ladam)
    D step |d loss| / loss                        2.2e-6      8.8e-6      1.63e-7  at (3, 63, 77, 130)
    D step max|d grad| / max|grad|, per tensor    3.1e-6      1.2e-5      5.53e-6  at (6, 64, 4100, 4097)
    loss of the refiner's pick above the least    0           3.6e-6      1.83e-7  (bar: twice the device's |d sigmoid|, rounded up to 1.8e-6)

Paths, and the case that enters each:
    the sample loop's second and third turn (256 blocks x 16 waves = 4096 samples a turn)
        saliency (64, 6, 4097) and (16, 6, 8200); refiner (64, 6, 4097, K = 5) and (16, 6, 8200, K = 3); both parts of the D step
        (6, 64, 4100, 4097), whose second part also writes its rows at row0 = 4100; rows 4096.. compared bit for bit with a batch of
        their own in test_a_rows_sigmoid_does_not_depend_on_its_batch
    padding to 64 lanes, nh in {1, 7, 16, 33, 63}
        saliency (1, 2, 64), (7, 5, 15), (16, 6, 8200), (33, 4, 1000), (63, 3, 333); the same without nh = 1 in the refiner;
        D step (2, 1, 5, 3), (4, 7, 64, 1), (5, 33, 1, 64), (3, 63, 77, 130)
    nlayers = 2 (no hidden -> hidden layer) .. 6
        saliency / refiner (64, 2, 17), (63, 3, 333), (33, 4, 1000), (7, 5, 15), (64, 6, ...); D step nl = 2, 3, 4, 5, 6
    steps = 0, rate = 0, want_traj = False for sgd / momentum / ladam, the device-scalar baseline at nh = 33
        the tests of those names below
"""
import numpy as np
import pytest
import torch

import mlp2d_cases as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def _D(Ws, bs):
    from cgs_amd.synthetic import MLPDiscriminator
    return MLPDiscriminator.from_lists(Ws, bs, DEV)


def _saliency_nan_filled(D, x, want_saliency=True):
    """cgs_mlp2d_sigmoid_saliency into NaN-filled outputs (MLPDiscriminator.sigmoid_and_saliency allocates its own, so the entry point is
    called as that method calls it)."""
    from cgs_amd import lib as L
    xd = D._x(x)
    B = xd.shape[0]
    sig = torch.full((B,), NAN, dtype=torch.float32, device=D.dev)
    sal = torch.full((B, 2), NAN, dtype=torch.float32, device=D.dev) if want_saliency else None
    L.call("cgs_mlp2d_sigmoid_saliency", D._wp, D._bp, D.nlayers, D.nhidden, xd.data_ptr(), sig.data_ptr(), None if sal is None else sal.data_ptr(),
           B, 1.0 / B, torch.cuda.current_stream(D.dev).cuda_stream)
    return sig, sal


@pytest.mark.parametrize("scale", M.SCALES)
@pytest.mark.parametrize("nh,nl,B", M.SALIENCY)
def test_sigmoid_and_saliency_vs_float64(nh, nl, B, scale):
    Ws, bs, x, (want_sig, want_sal, near) = M.saliency_case(nh, nl, B, scale)
    keep = ~near
    assert near.mean() <= M.KINK_CAP
    D = _D(Ws, bs)
    sig, sal = _saliency_nan_filled(D, x)
    sig_h, sal_h = sig.cpu().numpy().astype(np.float64), sal.cpu().numpy().astype(np.float64)
    assert np.isfinite(sig_h).all() and np.isfinite(sal_h).all()
    ds = np.abs(sig_h[keep] - want_sig[keep]).max()
    dg = np.abs(sal_h[keep] - want_sal[keep]).max() / np.abs(want_sal[keep]).max()
    print(f"{(nh, nl, B, scale)}: dropped {near.mean():.4f}  max|d sigmoid| {ds:.3e}  max|d saliency|/max|saliency| {dg:.3e}")
    assert ds <= M.SIGMOID_BAR and dg <= M.SALIENCY_BAR, (ds, dg)
    sig_only, none = _saliency_nan_filled(D, x, want_saliency=False)
    assert none is None and torch.equal(sig_only, sig)
    sig2, sal2 = D.sigmoid_and_saliency(x)                              # the class surface: the same bits, [B, 1] and [B, 2]
    assert sig2.shape == (B, 1) and sal2.shape == (B, 2) and torch.equal(sig2[:, 0], sig) and torch.equal(sal2, sal)


def test_a_rows_sigmoid_does_not_depend_on_its_batch():
    """Three turns of the sample loop against batches that take one: a row's sigmoid bits depend neither on the batch around it nor on the
    turn that reaches it.  (The saliency carries 1 / B: another function at another B, left out.)"""
    Ws, bs = M.net(64, 6, 11, 2.0)
    D = _D(Ws, bs)
    x = torch.from_numpy((3.0 * np.random.RandomState(9).randn(8200, 2)).astype(np.float32)).to(DEV)
    big = _saliency_nan_filled(D, x)[0]
    for lo, hi in ((0, 1000), (4096, 4200), (8199, 8200)):
        assert torch.equal(big[lo:hi], _saliency_nan_filled(D, x[lo:hi].contiguous())[0]), (lo, hi)


def _refine(D, x, base, K, rate, method, want_traj):
    best, step, traj = D.refine(x, base, K, rate, method, want_traj=want_traj)
    return best.cpu().numpy(), step.cpu().numpy(), None if traj is None else traj.cpu().numpy()


@pytest.mark.parametrize("case", M.REFINE, ids=M.case_id)
def test_refiner_teacher_forced_vs_float64(case):
    nh, nl, B, K, method, rate, scale = case
    Ws, bs, x, base = M.refine_case(*case)
    D = _D(Ws, bs)
    best, step, traj = _refine(D, x, base, K, rate, method, True)
    assert traj.shape == (B, K + 1, 2) and np.isfinite(traj).all()
    assert np.array_equal(traj[:, 0], x)
    pred, loss64, near = M.teacher_forced(Ws, bs, traj, base, rate, method)
    keep = ~near
    assert near.mean() <= M.KINK_CAP, near.mean()
    err = np.abs(traj[keep, 1:].astype(np.float64) - pred[keep, 1:]).max()
    idx = step.astype(np.int64)
    picked = loss64[np.arange(B), idx]
    excess = (picked[keep] - loss64[keep].min(axis=1)).max()
    print(f"refine {case}: dropped {near.mean():.4f}  worst one-step error {err:.3e} (bar {M.STEP_BAR:.1e})  "
          f"loss of the picked step above the least {excess:.3e} (bar {2 * M.DEVICE_SIGMOID:.1e})  rows with best_step > 0: {(idx > 0).mean():.3f}")
    assert err <= M.STEP_BAR
    assert np.array_equal(step, idx) and idx.min() >= 0 and idx.max() <= K
    assert np.array_equal(best, traj[np.arange(B), idx])                # best is a recorded point, at the recorded step, for every row
    assert excess <= 2 * M.DEVICE_SIGMOID
    best2, step2, none = _refine(D, x, base, K, rate, method, False)
    assert none is None and np.array_equal(best2, best) and np.array_equal(step2, step)


@pytest.mark.parametrize("method", ["sgd", "momentum", "ladam"])
def test_refiner_without_the_trajectory_returns_the_same_bits(method):
    """want_traj = False for every method, where the sample loop takes three turns."""
    Ws, bs = M.net(16, 6, 5, 2.0)
    D = _D(Ws, bs)
    x = (3.0 * np.random.RandomState(6).randn(8200, 2)).astype(np.float32)
    rate = {"sgd": 2000.0, "momentum": 600.0, "ladam": 0.05}[method]
    a, b = _refine(D, x, 0.4, 4, rate, method, True), _refine(D, x, 0.4, 4, rate, method, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] > 0).mean() > 0.5


def test_device_scalar_baseline_equals_the_host_float_on_a_padded_net():
    nh, nl, B, K, method, rate, scale = case = M.REFINE[4]             # (33, 4, 1000, 10, ladam)
    Ws, bs, x, base = M.refine_case(*case)
    D = _D(Ws, bs)
    a = D.refine(x, torch.tensor(base, dtype=torch.float32, device=DEV), K, rate, method, want_traj=True)
    b = D.refine(x, base, K, rate, method, want_traj=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("method", ["sgd", "momentum", "ladam"])
def test_zero_steps_and_zero_rate(method):
    """steps = 0: nothing but the input comes back.  rate = 0: every recorded point is the input, and best_step stays 0 -- the update test is
    strict (bl - loss > 0), so a tie keeps the earlier step."""
    Ws, bs, x, base = M.refine_case(*M.REFINE[3])                       # (63, 3, 333)
    D = _D(Ws, bs)
    best, step, traj = _refine(D, x, base, 0, 60.0, method, True)
    assert traj.shape == (333, 1, 2) and np.array_equal(traj[:, 0], x) and np.array_equal(best, x) and not step.any()
    best, step, none = _refine(D, x, base, 0, 60.0, method, False)
    assert none is None and np.array_equal(best, x) and not step.any()
    best, step, traj = _refine(D, x, base, 3, 0.0, method, True)
    assert traj.shape == (333, 4, 2) and all(np.array_equal(traj[:, i], x) for i in range(4))
    assert np.array_equal(best, x) and not step.any()


@pytest.mark.parametrize("case", M.DSTEP, ids=M.case_id)
def test_d_step_vs_float64(case):
    from cgs_amd.synthetic import DShaper
    nl, nh, Br, Bf = case
    Ws, bs, real, fake, dropped = M.dstep_case(*case)
    assert real.shape == (Br, 2) and fake.shape == (Bf, 2) and dropped <= M.KINK_CAP
    lr64, lf64, dW, db, near_r, near_f = M.d_step64(Ws, bs, real, fake)
    assert not near_r.any() and not near_f.any()
    D = _D(Ws, bs)
    sh = DShaper(D, lrd=8e-3)
    for t in sh.gw + sh.gb + [sh.loss]:
        t.fill_(NAN)
    loss, gW, gb = sh.loss_and_grads(real, fake)
    loss_h = loss.cpu().numpy().astype(np.float64)
    el = max(abs(loss_h[0] - lr64) / lr64, abs(loss_h[1] - lf64) / lf64)
    errs = []
    for got, want in zip(gW + gb, dW + db):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape and np.isfinite(got).all()
        errs.append(np.abs(got - want).max() / np.abs(want).max())
    print(f"d step {case}: dropped {dropped:.4f}  |d loss|/loss {el:.3e} (bar {M.DLOSS_BAR:.1e})  "
          f"worst max|d grad|/max|grad| {max(errs):.3e} (bar {M.DGRAD_BAR:.1e})")
    assert el <= M.DLOSS_BAR and max(errs) <= M.DGRAD_BAR, (el, errs)
    for t, w in zip(D.w + D.b, Ws + bs):
        assert torch.equal(t.cpu(), torch.from_numpy(w))                               # lr = 0 left the weights alone
    g_first = [t.clone() for t in gW + gb]
    before = [t.clone() for t in D.w + D.b]
    loss_first = loss.clone()
    assert torch.equal(sh.step(real, fake), loss_first)
    for t, w0, g in zip(D.w + D.b, before, g_first):
        assert torch.equal(t, w0 - torch.tensor(8e-3, dtype=torch.float32) * g)        # var -= lr * grad, two roundings, bit-exact
    assert any(not torch.equal(t, w0) for t, w0 in zip(D.w + D.b, before))
    D2 = _D(Ws, bs)
    DShaper(D2, lrd=8e-3).step(real, fake)
    for a, b in zip(D.w + D.b, D2.w + D2.b):
        assert torch.equal(a, b)                                                       # two runs are bit-equal
