"""The D step of the 2-D net at 65..256 hidden units (WideDShaper -> cgs_mlp2d_wide_d_step, csrc/mlp2d_wide_train.hip): both loss terms and
every gradient against a float64 restatement of the same float32 weights, the in-place update and its determinism, an embedded 64-unit
net against the shipped narrow step, five carried steps, the class surface, and a D that learns.

Tile sizes: pass A picks T = 32 or 64 samples per workgroup per part from that part's rows and the CU count; on the MI355X's 256 CUs a
part of up to 8192 rows runs T = 32 and 8193..16384 rows T = 64, hence the 8200-row parts.  Pass B sums the samples in chunks of
CHUNK(B_total) = 128 ceil(B_total / 2048) rows, whatever the device."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampling_ref as S

DEV = "cuda:0"


def CHUNK(B_total):
    """samples per partial tile of the weight-gradient pass (mlpw_chunk of mlp2d_wide_train.hip)"""
    return 128 * -(-B_total // 2048)


def _net(nh, nl, seed, scale):
    Ws, bs = S.mlp_init(nh, nl, seed=seed, scale=scale)
    return [w.numpy() for w in Ws], [b.numpy() for b in bs]


def _D(Ws, bs):
    from cgs_amd.synthetic import MLPDiscriminator
    return MLPDiscriminator.from_lists(Ws, bs, DEV)


def ref64(Ws, bs, real, fake):
    """float64 forward, ReLU masks, backward and h^T d sums of the float32 weights for
    d_loss = mean BCE(D(real), 1) + mean BCE(D(fake), 0) -> ((loss_real, loss_fake), [dW...], [db...], near [Br + Bf]);
    near[b]: some pre-activation of row b lies within 1e-6 max|z| (max over its layer) of zero (ref64 of mlp2d_cases.py)."""
    W = [w.astype(np.float64) for w in Ws]
    b = [v.astype(np.float64) for v in bs]
    Br, Bf = len(real), len(fake)
    x = np.concatenate([np.asarray(real, np.float64), np.asarray(fake, np.float64)])
    tgt = np.concatenate([np.ones(Br), np.zeros(Bf)])
    scale = np.concatenate([np.full(Br, 1.0 / Br), np.full(Bf, 1.0 / Bf)])
    hs, zs, near = [x], [], np.zeros(len(x), bool)
    for i in range(len(W) - 1):
        z = hs[-1] @ W[i] + b[i]
        near |= (np.abs(z) < 1e-6 * np.abs(z).max()).any(axis=1)
        zs.append(z)
        hs.append(np.maximum(z, 0.0))
    logit = (hs[-1] @ W[-1] + b[-1])[:, 0]
    bce = np.maximum(logit, 0.0) - logit * tgt + np.log1p(np.exp(-np.abs(logit)))
    losses = np.array([(scale * bce)[:Br].sum(), (scale * bce)[Br:].sum()])
    d = (scale * (1.0 / (1.0 + np.exp(-logit)) - tgt))[:, None]
    gW, gb = [None] * len(W), [None] * len(W)
    for i in range(len(W) - 1, -1, -1):
        gW[i], gb[i] = hs[i].T @ d, d.sum(axis=0)
        if i:
            d = (d @ W[i].T) * (zs[i - 1] > 0)
    return losses, gW, gb, near


SPARE = 64      # spare rows per part, drawn after the case's own rows, for the cases that must keep their row counts


def _batches(nh, Br, Bf):
    """The case's own rows, then SPARE more of each part from the same stream (the first Br / Bf rows do not depend on the spares)."""
    rs = np.random.RandomState(Br + nh)
    real = S.toy_next_batch("25Gaussians", 1.0, 0.9, max(Br, 64), rs)[:Br]
    fake = 1.5 * rs.randn(Bf, 2)
    real = np.concatenate([real, S.toy_next_batch("25Gaussians", 1.0, 0.9, SPARE, rs)])
    fake = np.concatenate([fake, 1.5 * rs.randn(SPARE, 2)])
    return real.astype(np.float32), fake.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(nh, nl, Br, Bf, scale, refill=False):
    """Weights, the two batches with the rows near a ReLU kink dropped (at most 5 % of either part, before anything is computed from them),
    and the float64 reference on the kept rows.  refill: the dropped rows are replaced by spare rows that are not near a kink either, so
    that the parts keep exactly Br and Bf rows -- for the cases whose row count is what they are about."""
    Ws, bs = _net(nh, nl, 7 + nh + nl, scale)
    real, fake = _batches(nh, Br, Bf)
    if not refill:
        real, fake = real[:Br], fake[:Bf]
    near = ref64(Ws, bs, real, fake)[3]
    nr, nf = near[:len(real)], near[len(real):]
    dropped = (nr[:Br].mean(), nf[:Bf].mean())
    assert max(dropped) <= 0.05, ("rows near a ReLU kink", dropped)
    real, fake = real[~nr][:Br], fake[~nf][:Bf]
    if refill:
        assert len(real) == Br and len(fake) == Bf
    losses, gW, gb, _ = ref64(Ws, bs, real, fake)
    return Ws, bs, real, fake, losses, gW, gb, dropped


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _grad_errs(gw, gb, want_W, want_b):
    """per tensor: max|got - want| / max|want| (the bar is 2e-4 max|want| + 1e-9)"""
    errs = []
    for got, want in list(zip(gw, want_W)) + list(zip(gb, want_b)):
        got = got.astype(np.float64).reshape(want.shape)
        assert np.abs(got - want).max() <= 2e-4 * np.abs(want).max() + 1e-9, (got.shape, np.abs(got - want).max(), np.abs(want).max())
        errs.append(np.abs(got - want).max() / np.abs(want).max())
    return errs


CASES = [(65, 2, 33, 31),        # one unit past a 32-granule; no hidden -> hidden layer; tail tiles of 1 and 31 rows
         (96, 3, 65, 130),       # three tiles; a tail tile of one row
         (200, 4, 333, 100),     # nh not a multiple of the weight slab
         (129, 6, 64, 1),        # a part of one row; a whole tile exactly
         (256, 2, 31, 77),       # no hidden -> hidden layer at full width
         (256, 6, 1000, 1000),   # the workload's own net
         (96, 3, 8200, 100),     # the T = 64 form of pass A for one part (on 256 CUs); refilled to 8200 rows after the drop
         (256, 3, 100, 8200),    # ... for the other part, at full width; refilled likewise
         (128, 3, 200, 57)]      # B_total = 257 = 2 CHUNK(257) + 1: the last chunk of pass B holds one sample; refilled likewise
REFILL = set(CASES[-3:])


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("nh,nl,Br,Bf", CASES)
def test_loss_and_gradients_vs_float64(nh, nl, Br, Bf, scale):
    """Bars (the project's own for this step, test_mlp_d_step_gradients_and_sgd_vs_autograd): each loss term rtol 2e-5, each gradient
    tensor 2e-4 max|want| + 1e-9.  For scale, the float32 torch-CPU oracle (S.mlp_d_loss_and_grads) against the same float64 restatement on
    these inputs, measured on the CPU: worst gradient error 9.4e-6 max|g|, worst loss error 4.7e-7 (2.4e-5 on the batches without the refill).
    Measured on an MI355X over these 18 cases (this test prints them): loss relative error 2.3e-8 .. 4.7e-7; worst gradient tensor
    max|d g| / max|g| 4.5e-7 .. 2.1e-5 (the largest at (96, 3, 8200, 100), scale 1)."""
    Ws, bs, real, fake, want_loss, want_W, want_b, dropped = _case(nh, nl, Br, Bf, scale, (nh, nl, Br, Bf) in REFILL)
    if max(Br, Bf) == 8200:
        assert max(len(real), len(fake)) > 8192                       # the part that is to run T = 64 still does after the drop
    if (nh, nl, Br, Bf) == CASES[-1]:
        assert (len(real) + len(fake)) % CHUNK(len(real) + len(fake)) == 1
    from cgs_amd.synthetic import WideDShaper
    D = _D(Ws, bs)
    sh = WideDShaper(D, lrd=1e-2)
    loss, gw, gb = sh.loss_and_grads(real, fake)
    assert loss.shape == (2,) and loss.device.type == "cuda"
    loss = loss.cpu().numpy().astype(np.float64)
    lerr = np.abs(loss - want_loss) / np.abs(want_loss)
    print(f"{(nh, nl, Br, Bf, scale)}: dropped {dropped[0]:.4f} / {dropped[1]:.4f}  loss rel err {lerr.max():.3e}")
    np.testing.assert_allclose(loss, want_loss, rtol=2e-5, atol=0)
    for t, w in zip(gw + gb, want_W + want_b):
        assert t.numel() == w.size
    errs = _grad_errs(_np(gw), _np(gb), want_W, want_b)
    print(f"{(nh, nl, Br, Bf, scale)}: max over tensors of max|d g| / max|g| {max(errs):.3e}")
    for t, w0 in zip(D.w + D.b, Ws + bs):                              # lr = 0: nothing moved
        np.testing.assert_array_equal(t.cpu().numpy(), w0)


@pytest.mark.parametrize("nh,nl,Br,Bf", [(256, 6, 1000, 1000), (65, 2, 33, 31)])
def test_update_is_two_roundings_and_deterministic(nh, nl, Br, Bf):
    from cgs_amd.synthetic import WideDShaper
    Ws, bs, real, fake = _case(nh, nl, Br, Bf, 1.0, False)[:4]
    lrd = 1e-2
    D1, D2 = _D(Ws, bs), _D(Ws, bs)
    s1, s2 = WideDShaper(D1, lrd), WideDShaper(D2, lrd)
    _, gw, gb = s1.loss_and_grads(real, fake)
    g = _np(gw) + _np(gb)
    _, gw, gb = s1.loss_and_grads(real, fake)
    for a, b in zip(g, _np(gw) + _np(gb)):
        np.testing.assert_array_equal(a, b)
    l1 = s1.step(real, fake).cpu().numpy()
    l2 = s2.step(real, fake).cpu().numpy()
    np.testing.assert_array_equal(l1, l2)
    moved = 0
    for t1, t2, w0, gi in zip(D1.w + D1.b, D2.w + D2.b, Ws + bs, g):
        want = w0 - np.float32(lrd) * gi.reshape(w0.shape)             # float32 numpy: the product rounds, then the difference
        assert want.dtype == np.float32
        np.testing.assert_array_equal(t1.cpu().numpy(), want)
        assert torch.equal(t1, t2)
        moved += int((want != w0).sum())
    assert moved > 0


@pytest.mark.parametrize("wide", [96, 256])
def test_embedded_64_unit_net_vs_the_narrow_step(wide):
    """The 64 x 6 net at a seeded permutation of `wide` positions (the other units: zero weights in and out, zero bias), 333 + 200 rows:
    losses and the gradient entries at the embedded positions against DShaper's, the bars of the float64 test; every other entry of
    every dW and db exactly 0.0 (a silent unit's pre-activation is exactly 0, its mask bit 0, its activation 0)."""
    from cgs_amd.synthetic import DShaper, WideDShaper
    Ws, bs = _net(64, 6, 11, 2.0)
    n = len(Ws)
    pos = np.random.RandomState(wide).permutation(wide)[:64]
    We, be, sel_w, sel_b = [], [], [], []
    for i, (w, b) in enumerate(zip(Ws, bs)):
        din, dout = (2 if i == 0 else wide), (1 if i == n - 1 else wide)
        E, e = np.zeros((din, dout), np.float32), np.zeros(dout, np.float32)
        ix = np.ix_(np.arange(2) if i == 0 else pos, np.arange(1) if i == n - 1 else pos)
        E[ix] = w
        e[ix[1][0]] = b
        We.append(E); be.append(e); sel_w.append(ix); sel_b.append(ix[1][0])
    rs = np.random.RandomState(5)
    real = S.toy_next_batch("25Gaussians", 1.0, 0.9, 333, rs).astype(np.float32)
    fake = (1.5 * rs.randn(200, 2)).astype(np.float32)
    ln, gwn, gbn = DShaper(_D(Ws, bs)).loss_and_grads(real, fake)
    lw, gww, gbw = WideDShaper(_D(We, be)).loss_and_grads(real, fake)
    np.testing.assert_allclose(lw.cpu().numpy(), ln.cpu().numpy(), rtol=2e-5, atol=0)
    gww, gbw = _np(gww), _np(gbw)
    errs = _grad_errs([g[ix] for g, ix in zip(gww, sel_w)], [g[ix] for g, ix in zip(gbw, sel_b)],
                      [g.astype(np.float64) for g in _np(gwn)], [g.astype(np.float64) for g in _np(gbn)])
    print(f"embedded in {wide}: loss rel err {np.abs(lw.cpu().numpy() / ln.cpu().numpy() - 1).max():.3e}  max|d g| / max|g| {max(errs):.3e}")
    for g, ix in zip(gww, sel_w):
        rest = np.ones(g.shape, bool)
        rest[ix] = False
        assert (g[rest] == 0.0).all()
    for g, ix in zip(gbw, sel_b):
        rest = np.ones(g.shape, bool)
        rest[ix] = False
        assert (g[rest] == 0.0).all()


def five_step_batches(k):
    rs = np.random.RandomState(100 + k)
    real = S.toy_next_batch("25Gaussians", 1.0, 0.9, 500, rs).astype(np.float32)
    return real, (1.5 * rs.randn(500, 2)).astype(np.float32)


def five_steps_float64(Ws, bs, lr):
    W, b = [w.astype(np.float64) for w in Ws], [v.astype(np.float64) for v in bs]
    for k in range(5):
        real, fake = five_step_batches(k)
        _, gW, gb, _ = ref64(W, b, real, fake)
        W = [w - lr * g for w, g in zip(W, gW)]
        b = [v - lr * g for v, g in zip(b, gb)]
    return W, b


FIVE_STEP_ORACLE = 2.24e-4     # five float32 torch-CPU steps (S.mlp_d_sgd_step) against the float64 run, worst tensor (a 128 x 128 kernel whose
FIVE_STEP_BAR = 4 * FIVE_STEP_ORACLE       # total movement, 1.3e-4, is some 2000 float32 roundings of its entries); the other tensors: 7.6e-7 .. 1.8e-4


def test_five_carried_steps_vs_float64():
    """(128, 4, 500, 500), lr 1e-2, fresh seeded batches per step: the weights after five step() calls against five float64 steps of the
    restatement, per tensor max|w5 - want5| / max|want5 - w0| (the error relative to the tensor's total movement).
    The bar is 4 x what five steps of the float32 torch-CPU oracle S.mlp_d_sgd_step measure against the same float64 run on the same
    batches: FIVE_STEP_ORACLE (worst tensor), measured on the CPU; the seed is the first tried."""
    from cgs_amd.synthetic import WideDShaper
    Ws, bs = _net(128, 4, 21, 1.0)
    lr = float(np.float32(1e-2))
    W64, b64 = five_steps_float64(Ws, bs, lr)
    D = _D(Ws, bs)
    sh = WideDShaper(D, lrd=1e-2)
    for k in range(5):
        sh.step(*five_step_batches(k))
    worst = 0.0
    for t, w0, want in zip(D.w + D.b, Ws + bs, W64 + b64):
        got = t.cpu().numpy().astype(np.float64).reshape(want.shape)
        move = np.abs(want - w0.reshape(want.shape)).max()
        worst = max(worst, np.abs(got - want).max() / move)
    print(f"five steps: worst max|w5 - want5| / max|want5 - w0| {worst:.3e} (bar {FIVE_STEP_BAR:.1e}, float32 oracle {FIVE_STEP_ORACLE:.1e})")
    assert worst <= FIVE_STEP_BAR


def test_class_surface():
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.lib import CgsError
    from cgs_amd.synthetic import DShaper, Gan, MLPDiscriminator, Refiner, WideDShaper, d_shaper, shape_step
    D64, D65 = MLPDiscriminator.init(1), MLPDiscriminator.init(1, nhidden=65, nlayers=3)
    assert type(d_shaper(D64, 1e-2)) is DShaper and type(d_shaper(D65, 1e-2)) is WideDShaper
    with pytest.raises(CgsError, match="DShaper"):
        WideDShaper(D64)
    args = types.SimpleNamespace(rollout_steps=5, rollout_rate=0.05, rollout_method="ladam")
    rs = np.random.RandomState(1)
    fake = (1.5 * rs.randn(300, 2)).astype(np.float32)
    probe = (2.0 * rs.randn(64, 2)).astype(np.float32)
    data = ToyDataset("25Gaussians", scale=1.0)
    after = {}
    for nh in (64, 256):
        D = _D(*_net(nh, 6, 2019, 1.0))
        sh = d_shaper(D, 1e-2)
        assert sh.loss.shape == (2,) and sh.loss.device.type == "cuda" and len(sh.gw) == len(sh.gb) == 6
        ref = Refiner(args)
        ref.set_env(Gan(D), None, data)
        w0 = [t.clone() for t in D.w + D.b]
        sig0, sal0 = D.sigmoid_and_saliency(probe)
        np.random.seed(2019)
        real = data.next_batch(300)
        loss, refined = shape_step(ref, sh, fake, real)
        after[nh] = np.random.randint(1 << 30, size=4)
        assert refined.shape == (300, 2) and refined.dtype == np.float64 and np.isfinite(refined).all()
        assert loss is sh.loss and torch.isfinite(loss).all()
        assert all(not torch.equal(a, b) for a, b in zip(w0, D.w + D.b))          # every tensor moved, in place
        sig1, sal1 = D.sigmoid_and_saliency(probe)
        assert not torch.equal(sig0, sig1) and not torch.equal(sal0, sal1)
    np.testing.assert_array_equal(after[64], after[256])                          # the host RNG consumption does not depend on the width


def trains_batches():
    rs = np.random.RandomState(6)
    real = S.toy_next_batch("25Gaussians", 1.0, 0.9, 1000, rs).astype(np.float32)
    modes = np.array([(x, y) for x in range(-2, 3) for y in range(-2, 3)], np.float64)
    fake = (modes[rs.randint(25, size=1000)] + 0.8 * rs.randn(1000, 2)).astype(np.float32)
    return real, fake


def test_it_trains():
    """A 256 x 6 D, one fixed pair of batches (25-Gaussians real; fake: the modes blurred by a 0.8-sigma Gaussian), 50 steps at lr 1e-2:
    d_loss before the last step is below d_loss before the first.  The float64 restatement alone shows this drop for this seed
    (DESIGN.md section 12)."""
    from cgs_amd.synthetic import WideDShaper
    real, fake = trains_batches()
    sh = WideDShaper(_D(*_net(256, 6, 2019, 1.0)), lrd=1e-2)
    first = sh.step(real, fake).sum().item()
    for _ in range(49):
        last = sh.step(real, fake).sum().item()
    print(f"d_loss {first:.5f} -> {last:.5f}")
    assert np.isfinite(last) and last < first
