"""cgs_refine_update_ladam / cgs_ladam_gain and PolicyAdaptive("ladam") on device maps against the float64 step of tests/loss_cases.py.
The bound is loss_cases.ladam_bound: derived from the operation count of the formula, not from measurements."""
import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 4), (3, 7), (4, 12544), (5, 12546)]          # 3x7 and 5x12546: the scalar form; the others 16-byte accesses


def dev():
    return torch.device("cuda:0")


def case(B, F, seed):
    rs = np.random.RandomState(seed)
    theta = rs.randn(B, F).astype(F32)
    m, v = (0.1 * rs.randn(B, F)).astype(F32), (0.01 * rs.rand(B, F)).astype(F32)
    g = (0.1 * rs.randn(B, F)).astype(F32)
    g[0, F // 2] = 0.0                                      # theta must not move where g (and, on later steps, m and v) is exactly zero
    m[0, F // 2] = v[0, F // 2] = 0.0
    gain = (rs.rand(B) * 2.0).astype(F32)
    return theta, m, v, g, gain


@pytest.mark.parametrize("clip", (False, True))
@pytest.mark.parametrize("first", (True, False))
@pytest.mark.parametrize("B,F", SHAPES)
def test_ladam_update_against_float64(B, F, first, clip):
    from cgs_amd import kernels as K
    d = dev()
    theta, m, v, g, gain = case(B, F, 7 * B + F)
    if B >= 3:
        gain[1], gain[2] = 0.0, 1e8                          # the two ends of the clamp (gain 0: the sample stands still)
    vmin, vmax = (float(F32(0.05)), 1.5) if clip else (None, None)      # (the clip values as the kernel gets them; a clip moves no two values apart)
    t, mm, vv = (torch.from_numpy(a.copy()).to(d) for a in (theta, m, v))
    if first:                                               # the first step must not read m and v
        mm.fill_(float("nan")); vv.fill_(float("nan"))
    K.refine_update_ladam(t, mm, vv, torch.from_numpy(g).to(d), torch.from_numpy(gain).to(d), 0.1, first, vmin, vmax)
    rate = float(F32(0.1))
    want, wm, wv = LC.ladam_step(theta, m, v, g, gain, rate, first, vmin, vmax)
    bound = LC.ladam_bound(theta, m, v, g, gain, rate, first)
    err = np.abs(t.cpu().numpy().astype(np.float64) - want)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print(f"ladam update B={B} F={F} first={first} clip={clip}: max |err| / bound = {frac:.3f}")
    assert frac <= 1.0
    assert np.abs(mm.cpu().numpy() - wm).max() <= 3 * LC.U * (np.abs(wm).max() + np.abs(g).max())
    assert np.abs(vv.cpu().numpy() - wv).max() <= 3 * LC.U * np.abs(wv).max()
    got = t.cpu().numpy()
    if not clip:
        assert got[0, F // 2] == theta[0, F // 2]
        if B >= 3:
            assert np.array_equal(got[1], theta[1])
    else:
        assert got.min() >= F32(0.05) and got.max() <= F32(1.5)
    t2, m2, v2 = (torch.from_numpy(a.copy()).to(d) for a in (theta, m, v))
    K.refine_update_ladam(t2, m2, v2, torch.from_numpy(g).to(d), torch.from_numpy(gain).to(d), 0.1, first, vmin, vmax)
    assert torch.equal(t2, t)                               # reruns are bit-equal


def test_ladam_gain_state():
    from cgs_amd import kernels as K
    d = dev()
    loss = np.array([0.3, -3.0, 4e4, -0.5, 0.0], dtype=F32)       # -3: loss_avg + 0.5 < 0 -> gain 0; 4e4: above the clamp
    avg_d, gain_d = torch.empty(5, device=d), torch.empty(5, device=d)
    avg = None
    for first in (True, False, False):
        K.ladam_gain(torch.from_numpy(loss).to(d), avg_d, gain_d, first)
        avg = loss if first else F32(0.5) * avg + F32(0.5) * loss
        c = np.minimum(np.maximum(avg + F32(0.5), F32(0)), F32(1e4))
        assert np.array_equal(avg_d.cpu().numpy(), avg) and np.array_equal(gain_d.cpu().numpy(), c * c)
        want_avg, want_gain = LC.ladam_state(loss, None, True)            # (a constant loss: its running average stays the loss)
        assert np.allclose(avg, want_avg, rtol=1e-6) and np.allclose(c * c, want_gain, rtol=1e-6)
    assert gain_d[1].item() == 0.0 and gain_d[2].item() == 1e8


def test_policy_ladam_on_a_device_map():
    """PolicyAdaptive("ladam") on a CUDA map tensor over 3 calls against its own result on the CPU copy, each step from the same theta,
    within the per-step bound; after reset_moving_average the first-step form again."""
    from cgs_amd.sampling.policy import PolicyAdaptive
    d = dev()
    rs = np.random.RandomState(5)
    shape = (4, 7, 7, 16)
    dp, cp = PolicyAdaptive(0.1, "ladam"), PolicyAdaptive(0.1, "ladam")
    theta = torch.from_numpy(rs.randn(*shape).astype(F32))
    for rounds in range(2):
        m = v = avg = None
        for i in range(3):
            g = torch.from_numpy((0.1 * rs.randn(*shape)).astype(F32))
            loss = torch.from_numpy((0.3 * rs.randn(4)).astype(F32))
            got = dp.apply_gradient(theta.to(d), g.to(d), loss.to(d))
            want = cp.apply_gradient(theta, g, loss)
            assert got.is_cuda and got.shape == theta.shape and not torch.equal(got.cpu(), theta)
            rate = float(F32(0.1))
            avg, gain = LC.ladam_state(loss.numpy(), avg, i == 0)
            bound = LC.ladam_bound(theta.numpy().reshape(4, -1), m, v, g.numpy().reshape(4, -1), gain, rate, i == 0)
            _, m, v = LC.ladam_step(theta.numpy().reshape(4, -1), m, v, g.numpy().reshape(4, -1), gain, rate, i == 0)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want.numpy().astype(np.float64)).reshape(4, -1)
            print(f"policy ladam round {rounds} step {i}: max |device - cpu| / bound = {(err / bound).max():.3f}")
            assert (err <= bound).all()
            if i == 0:
                assert torch.equal(dp.momentum.cpu(), g)            # the first-step form: m = g
            theta = want
        dp.reset_moving_average(); cp.reset_moving_average()
        assert dp.momentum is None and dp.loss is None
    # CPU tensors and numpy arrays keep their own branches
    assert not cp.apply_gradient(theta, g, loss).is_cuda
