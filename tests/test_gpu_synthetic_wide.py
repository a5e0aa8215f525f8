"""The 2-D discriminator at 65..256 hidden units (the 25-Gaussians D: 256 x 6) on the sample-tile MFMA kernels of mlp2d_wide.hip: sigmoid and
saliency against a float64 restatement of the same float32 weights, against the shipped 64-unit kernel on an embedded net, row
independence across tile sizes, the fused refiner against oracle.sampling_ref.refine_2d, and the class surface.

Tile sizes: the library picks T = 32 or 64 samples per workgroup from B and the CU count; on the MI355X's 256 CUs every B <= 8192 runs
T = 32 and 8193 <= B <= 16384 runs T = 64, hence the B = 8200 cases."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlp2d_cases import ref64          # the float64 forward / backward and the rows near a ReLU kink, stated once for both widths
from oracle import sampling_ref as S

DEV = "cuda:0"


def _net(nh, nl, seed, scale):
    Ws, bs = S.mlp_init(nh, nl, seed=seed, scale=scale)
    return [w.numpy() for w in Ws], [b.numpy() for b in bs]


def _D(Ws, bs):
    from cgs_amd.synthetic import MLPDiscriminator
    return MLPDiscriminator.from_lists(Ws, bs, DEV)


def _check_vs(sig, sal, want_sig, want_sal, keep, tag):
    """The bars of the issue: |d sigmoid| <= 2e-5 (the project's device-score bar; the float32 torch-CPU oracle measures <= 4.0e-6 against
    float64) and max|d saliency| <= 3e-6 max|saliency| (4x the 7.7e-7 of that oracle)."""
    assert keep.mean() >= 0.95, (tag, "rows near a ReLU kink", 1.0 - keep.mean())
    ds = np.abs(sig[keep] - want_sig[keep]).max()
    dg = np.abs(sal[keep] - want_sal[keep]).max() / np.abs(want_sal[keep]).max()
    print(f"{tag}: dropped {1.0 - keep.mean():.4f}  max|d sigmoid| {ds:.3e}  max|d saliency|/max|saliency| {dg:.3e}")
    assert ds <= 2e-5 and dg <= 3e-6, (tag, ds, dg)


CASES = [(65, 2, 33), (96, 3, 65), (128, 6, 1000), (200, 4, 333), (256, 6, 1000), (256, 6, 1), (256, 2, 31), (129, 6, 64),
         (96, 3, 8200), (256, 3, 8200)]            # the last two: T = 64 tiles, the tail tile 8 rows


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("nh,nl,B", CASES)
def test_sigmoid_and_saliency_vs_float64(nh, nl, B, scale):
    """Rows near a ReLU kink (ref64) are dropped before the device is called, at most 5 % of them.
    Measured on an MI355X over these cases: 0 - 1.6 % of rows dropped, max|d sigmoid| 1.9e-8 .. 1.6e-6 (bar 2e-5),
    max|d saliency| / max|saliency| 8.9e-8 .. 1.2e-6 (bar 3e-6; the largest at (256, 6, 1000), scale 2)."""
    Ws, bs = _net(nh, nl, 7 + nh + nl, scale)
    x = (3.0 * np.random.RandomState(B + nh).randn(B, 2)).astype(np.float32)
    want_sig, want_sal, near = ref64(Ws, bs, x)
    D = _D(Ws, bs)
    sig, sal = D.sigmoid_and_saliency(x)
    assert sig.shape == (B, 1) and sal.shape == (B, 2)
    _check_vs(sig.cpu().numpy()[:, 0].astype(np.float64), sal.cpu().numpy().astype(np.float64), want_sig, want_sal, ~near, (nh, nl, B, scale))
    sig_only, none = D.sigmoid_and_saliency(x, want_saliency=False)
    assert none is None and torch.equal(sig_only, sig)


@pytest.mark.parametrize("wide", [96, 256])
def test_wide_kernel_equals_narrow_kernel_on_an_embedded_net(wide):
    """A 64-unit net placed at a seeded permutation of `wide` positions (the other units: zero weights in and out, zero bias) is the same
    function: the new kernel against the shipped one, no oracle in between, no row excluded.
    Measured on an MI355X: max|d sigmoid| 8.0e-7 / 1.2e-6, max|d saliency| / max|saliency| 7.9e-7 / 5.3e-7 (96 / 256 wide)."""
    Ws, bs = _net(64, 6, 11, 2.0)
    pos = np.random.RandomState(wide).permutation(wide)[:64]
    We, be = [], []
    for i, (w, b) in enumerate(zip(Ws, bs)):
        din, dout = (2 if i == 0 else wide), (1 if i == len(Ws) - 1 else wide)
        E, e = np.zeros((din, dout), np.float32), np.zeros(dout, np.float32)
        E[np.ix_(np.arange(2) if i == 0 else pos, np.arange(1) if i == len(Ws) - 1 else pos)] = w
        e[np.arange(1) if i == len(Ws) - 1 else pos] = b
        We.append(E); be.append(e)
    x = (3.0 * np.random.RandomState(5).randn(333, 2)).astype(np.float32)
    sig_n, sal_n = _D(Ws, bs).sigmoid_and_saliency(x)
    sig_w, sal_w = _D(We, be).sigmoid_and_saliency(x)
    _check_vs(sig_w.cpu().numpy()[:, 0].astype(np.float64), sal_w.cpu().numpy().astype(np.float64),
              sig_n.cpu().numpy()[:, 0].astype(np.float64), sal_n.cpu().numpy().astype(np.float64), np.ones(333, bool), ("embedded", wide))


def test_rows_are_independent_and_calls_reproducible():
    """A row's bits depend neither on the batch around it nor on the tile size that batch gets."""
    Ws, bs = _net(256, 6, 3, 2.0)
    D = _D(Ws, bs)
    x = torch.from_numpy((3.0 * np.random.RandomState(9).randn(8200, 2)).astype(np.float32)).to(DEV)
    sig, sal = D.sigmoid_and_saliency(x[:1000])
    for lo, hi in ((0, 33), (999, 1000)):
        assert torch.equal(D.sigmoid_and_saliency(x[lo:hi].contiguous())[0], sig[lo:hi])
    big, _ = D.sigmoid_and_saliency(x)                               # T = 64 tiles against the T = 32 tiles of the calls above
    assert torch.equal(big[:1000], sig) and torch.equal(big[8192:], D.sigmoid_and_saliency(x[8192:].contiguous())[0])
    a = D.refine(x[:1000], 0.4, 10, 0.1, "ladam", want_traj=True)
    b = D.refine(x[:1000], 0.4, 10, 0.1, "ladam", want_traj=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    real = torch.from_numpy(np.random.RandomState(4).randn(512, 2).astype(np.float32)).to(DEV)
    base = D.sigmoid_and_saliency(real, want_saliency=False)[0].mean()
    c = D.refine(x[:512], base, 10, 0.1, "ladam")
    d = D.refine(x[:512], float(base.item()), 10, 0.1, "ladam")
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])
    e = D.refine(x, 0.4, 3, 0.1, "ladam")                            # T = 64 tiles (the saliency carries 1/B, so other B: another function)
    f = D.refine(x, 0.4, 3, 0.1, "ladam")
    assert torch.equal(e[0], f[0]) and torch.equal(e[1], f[1])


REFINE = {"a": (96, 2, 65, 5, "sgd", 200.0, 2.0), "b": (200, 4, 333, 5, "momentum", 60.0, 2.0), "c": (128, 3, 333, 5, "ladam", 0.05, 2.0),
          "d": (256, 6, 1000, 10, "ladam", 0.1, 1.0), "e": (256, 6, 1000, 50, "ladam", 0.05, 1.0),
          "f": (96, 3, 8200, 3, "ladam", 0.05, 2.0)}            # (a)-(e): the issue's cases; (f): the refiner's T = 64 form, bars of (a)-(d)


@pytest.mark.parametrize("case", sorted(REFINE))
def test_fused_refiner_vs_oracle(case):
    """best, best_step and the trajectory of the one-launch K-step loop against oracle.sampling_ref.refine_2d on the float32 oracle D.
    best_step agrees on > 98 % of the samples (the float32 oracle against a float64 D: 99.1 - 100 %); on those the 99th percentile of
    |d best| < 1e-4; (a)-(d) max < 5e-3; (e), 50 ladam steps dividing by sqrt(v) + 1e-8, no max bar (the float32 oracle alone is 2.6e-3
    from float64 there) but at most 1 % of the agreeing samples above 1e-4."""
    nh, nl, B, K, method, rate, scale = REFINE[case]
    Ws, bs = _net(nh, nl, 2019, scale)
    Wt, bt = [torch.from_numpy(w) for w in Ws], [torch.from_numpy(b) for b in bs]
    rs = np.random.RandomState(3)
    real = S.toy_next_batch("25Gaussians", 1.0, 0.9, B, rs)
    fake = (1.5 * rs.randn(B, 2)).astype(np.float32)
    d_fn = lambda x: S.mlp_sigmoid_and_saliency(Wt, bt, x)
    want, want_step, _ = S.refine_2d(fake, real, d_fn, K, rate, method, "deterministic")
    base = float(np.mean(d_fn(real)[0]))
    best, step, traj = _D(Ws, bs).refine(fake, base, K, rate, method, want_traj=True)
    best, step, traj = best.cpu().numpy(), step.cpu().numpy(), traj.cpu().numpy()
    agree = step == want_step
    err = np.abs(best[agree].astype(np.float64) - want[agree])
    print(f"({case}) best_step agrees {agree.mean():.4f}  p99|d best| {np.percentile(err, 99):.3e}  max {err.max():.3e}  "
          f"above 1e-4: {(err.max(axis=1) > 1e-4).mean():.4f}")
    assert agree.mean() > 0.98
    assert np.percentile(err, 99) < 1e-4
    if case == "e":
        assert (err.max(axis=1) > 1e-4).mean() <= 0.01
    else:
        assert err.max() < 5e-3
    np.testing.assert_array_equal(traj[:, 0, :], fake)
    np.testing.assert_array_equal(traj[np.arange(B), step.astype(np.int64)], best)       # best is a recorded point, at the recorded step


def test_refiner_class_on_a_256_unit_d():
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.synthetic import Gan, Refiner
    args = types.SimpleNamespace(rollout_steps=10, rollout_rate=0.05, rollout_method="ladam")
    fake0 = (1.5 * np.random.RandomState(1).randn(500, 2)).astype(np.float32)
    after = {}
    for nh in (64, 256):
        D = _D(*_net(nh, 6, 2019, 1.0))
        for mode in ("deterministic", "probabilistic"):
            ref = Refiner(args)
            ref.set_env(Gan(D), None, ToyDataset("25Gaussians", scale=1.0))
            np.random.seed(2019)
            fake = fake0.copy()
            out = ref.manipulate_sample(fake, mode)
            np.testing.assert_array_equal(fake, fake0)
            assert out.shape == (500, 2) and out.dtype == (np.float32 if mode == "deterministic" else np.float64) and np.isfinite(out).all()
            assert ref.optimal_step.shape == (500,)
            after[nh, mode] = np.random.randint(1 << 30, size=4)
    for mode in ("deterministic", "probabilistic"):
        np.testing.assert_array_equal(after[64, mode], after[256, mode])        # the host RNG consumption does not depend on the width


def test_evaluate_collaborative_runs_on_a_256_unit_d():
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.synthetic import Gan, Refiner, evaluate_collaborative
    D = _D(*_net(256, 6, 2019, 1.0))
    data = ToyDataset("25Gaussians", scale=1.0)
    ref = Refiner(types.SimpleNamespace(rollout_steps=5, rollout_rate=0.05, rollout_method="ladam"))
    ref.set_env(Gan(D), None, data)
    rs = np.random.RandomState(2)
    np.random.seed(2019)
    gen = lambda: (1.5 * rs.randn(500, 2)).astype(np.float32)
    out = evaluate_collaborative(ref, D, gen, gen(), data.next_batch(500), data.centeroids, data.std)
    assert set(out) == {"standard", "refinement", "collaborate"}
    for q in out.values():
        assert all(np.isfinite(v) for v in q.values()), out
    assert 0.0 < out["collaborate"]["eff"] <= 1.0


def test_construction_limits():
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.lib import CgsError
    from cgs_amd.synthetic import DShaper, GanTrainer, MLPDiscriminator, MLPGenerator
    with pytest.raises(CgsError, match="256"):
        MLPDiscriminator.init(1, nhidden=257, nlayers=3)
    D256 = MLPDiscriminator.init(1, nhidden=256, nlayers=6)
    assert set(D256.params()) == set(MLPDiscriminator.init_params(1, 256, 6)) and D256.nhidden == 256
    with pytest.raises(CgsError, match="64-unit"):
        DShaper(D256)
    with pytest.raises(CgsError, match="64-unit"):
        GanTrainer(MLPGenerator.init(1), D256, ToyDataset("25Gaussians", scale=1.0))
    with pytest.raises(CgsError):
        MLPGenerator.init(1, nhidden=256)
    DShaper(MLPDiscriminator.init(1))                                # 64 units: as before
