"""The 2-D generator on the GPU (csrc/mlp2d.hip: cgs_mlp2d_gen_fwd, cgs_mlp2d_g_step) and the train mode of synthetic/main.py built on it,
against the float64 torch restatement in test_synthetic_train_cpu.py."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_synthetic_train_cpu as R

DEV = "cuda:0"


def perturbed_params(seed, nhidden=64, nlayers=6):
    """Seeded init with every G variable moved off its TF default, so that biases, gamma, beta and the moving statistics all matter."""
    from cgs_amd.synthetic import MLPGenerator
    P = MLPGenerator.init_params(seed, nhidden, nlayers)
    rs = np.random.RandomState(seed + 1)
    for k, v in P.items():
        if k.endswith("/bias") or k.endswith("/beta") or k.endswith("/moving_mean"):
            P[k] = (0.5 * rs.randn(*v.shape)).astype(np.float32)
        elif k.endswith("/gamma") or k.endswith("/moving_variance"):
            P[k] = rs.uniform(0.5, 1.5, v.shape).astype(np.float32)
    return P


def host(t):
    return t.detach().cpu().double()


def rel_err(out, ref):
    return ((host(out) - ref).abs().max() / ref.abs().max()).item()


# gen_plan's edges (<= 256 waves of >= 8 contiguous samples, none empty): B = 9 -> waves of 5 and 4; B = 2041 -> 256 waves of 8, the last
# with ONE sample (its M2 partial is 0, its mean sum / 1); B = 2049, just past the cap -> chunk 9 and 228 waves
@pytest.mark.parametrize("B", [2, 7, 1000, 10000, 9, 2041, 2049])
def test_training_forward_and_moving_averages_vs_float64(B):
    check_training_forward(B, 64, 6)


@pytest.mark.parametrize("nhidden,nlayers,B", [(1, 2, 9), (63, 3, 2041), (7, 6, 2049), (1, 2, 2041)])
def test_training_forward_on_padded_and_shallow_nets(nhidden, nlayers, B):
    """lane < nh throughout the generator kernels, at one unit, at 63 and at 7; no hidden -> hidden layer at nlayers = 2.  Same float64
    reference and bars as the 64 x 6 cases."""
    check_training_forward(B, nhidden, nlayers)


def check_training_forward(B, nhidden, nlayers):
    from cgs_amd.synthetic import MLPGenerator, _bn_name
    P = perturbed_params(B, nhidden, nlayers)
    G = MLPGenerator(P, DEV)
    Q = R.to_torch(P, torch.float64)
    rs = np.random.RandomState(B)
    for call in range(3):
        z = rs.randn(B, 2).astype(np.float32)
        x, st = G.generate(z, batch_stats=True)
        stats = []
        ref = R.g_forward(Q, torch.as_tensor(z, dtype=torch.float64), stats=stats)
        # (B = 2: the variance of two samples is a difference of two rounded pre-activations, measured 1.6e-5 relative)
        tol = 1e-4 if B == 2 else 1e-5
        assert rel_err(x, ref) < tol, (call, rel_err(x, ref))
        for k, (m, v) in enumerate(stats):
            scale = (m.abs() + v.sqrt()).max()
            assert ((host(st[k, 0]) - m).abs().max() / scale).item() < tol
            assert ((host(st[k, 1]) - v).abs().max() / v.max()).item() < tol
        if call in (0, 2):                      # after 1 and after 3 training-mode calls: v -= (v - value) * 0.1, Bessel-corrected variance
            for k in range(G.nlayers - 1):
                for name, dev_t in (("moving_mean", G.moving_mean[k]), ("moving_variance", G.moving_variance[k])):
                    want = Q[f"{_bn_name(k)}/{name}"]
                    assert ((host(dev_t) - want).abs().max() / want.abs().max()).item() < 1e-5, (call, k, name)
    # inference mode (gan.fake_samples): the moving statistics, and no variable moves
    before = {k: v.clone() for k, v in G.params().items()}
    z = rs.randn(B, 2).astype(np.float32)
    x = G.generate(z, is_training=False)
    ref = R.g_forward(Q, torch.as_tensor(z, dtype=torch.float64), training=False)
    assert rel_err(x, ref) < 1e-5
    after = G.params()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_bessel_rule_is_the_recorded_one():
    """Moving variance after one call on a batch of 2 from moving_variance = 0: 0.1 * the UNBIASED variance, twice the biased one."""
    from cgs_amd.synthetic import MLPGenerator
    P = perturbed_params(5, 16, 2)
    P["generator/BatchNorm/moving_variance"][:] = 0
    G = MLPGenerator(P, DEV)
    z = np.random.RandomState(0).randn(2, 2).astype(np.float32)
    _, st = G.generate(z, batch_stats=True)
    np.testing.assert_allclose(G.moving_variance[0].cpu().numpy(), 0.1 * 2 * st[0, 1].cpu().numpy(), rtol=1e-6, atol=1e-12)


# (one unit at B = 2041, not at B = 9: with these seeds no sample of 9 passes the unit's ReLU, and every gradient below it is exactly zero)
@pytest.mark.parametrize("nhidden,nlayers,B", [(64, 6, 1000), (16, 3, 37), (64, 6, 9), (64, 6, 2041), (64, 6, 2049), (1, 2, 2041), (63, 3, 2049), (7, 6, 9)])
def test_g_step_vs_float64_autograd(nhidden, nlayers, B):
    from cgs_amd.synthetic import GStep, MLPGenerator
    P = perturbed_params(11, nhidden, nlayers)
    rs = np.random.RandomState(12)
    z = rs.randn(B, 2).astype(np.float32)
    gp = (1e-3 * rs.randn(B, 2)).astype(np.float32)
    G = MLPGenerator(P, DEV)
    step = GStep(G, lrg=5e-3)
    before = {k: v.detach().clone() for k, v in G.params().items()}          # snapshot BEFORE the lr = 0 call
    gw, gb = step.grads(z, gp)
    Q = R.to_torch(P, torch.float64)
    ref = R.g_step(Q, torch.as_tensor(z, dtype=torch.float64), torch.as_tensor(gp, dtype=torch.float64), 0.0)
    for i in range(nlayers):
        rw = ref[f"generator/g_fc{i + 1}/kernel"]
        rb = ref[f"generator/g_fc{i + 1}/bias"]
        assert rel_err(gw[i], rw) < 1e-3, (i, rel_err(gw[i], rw))                # 0.1 % of the step's own size
        if i < nlayers - 1:                     # feeds a training-mode BN: zero in exact arithmetic, computed by the formula
            # (measured: 1.2e-6 of the layer's largest kernel gradient -- the rounding of 1000 summed terms)
            assert host(gb[i]).abs().max().item() < 1e-5 * rw.abs().max().item(), (i, host(gb[i]).abs().max().item())
        else:
            assert rel_err(gb[i], rb) < 1e-3
    # lr = 0: every weight bit-unchanged against the snapshot taken before the call (the moving statistics did move: the forward ran)
    for i in range(nlayers):
        assert torch.equal(G.w[i], before[f"generator/g_fc{i + 1}/kernel"]) and torch.equal(G.b[i], before[f"generator/g_fc{i + 1}/bias"])
    assert not torch.equal(G.moving_mean[0], before[f"{R.bn_name(0)}/moving_mean"])
    # the step itself: w - lr * g from the pre-call weights, rounded twice (same batch -> the same gradient, the calls are deterministic)
    gw = [t.clone() for t in gw]
    step.step(z, gp)
    lr = torch.tensor(5e-3, dtype=torch.float32)
    for i in range(nlayers):
        assert torch.equal(G.w[i], before[f"generator/g_fc{i + 1}/kernel"] - lr * gw[i])
        assert not torch.equal(G.w[i], before[f"generator/g_fc{i + 1}/kernel"])
    # gamma and beta (not in g_vars) bit-unchanged since before the first call
    for k in range(nlayers - 1):
        assert torch.equal(G.gamma[k], before[f"{R.bn_name(k)}/gamma"]) and torch.equal(G.beta[k], before[f"{R.bn_name(k)}/beta"])


def test_forward_and_g_step_are_deterministic():
    from cgs_amd.synthetic import GStep, MLPGenerator
    P = perturbed_params(21)
    rs = np.random.RandomState(22)
    z = rs.randn(10000, 2).astype(np.float32)
    gp = (1e-3 * rs.randn(10000, 2)).astype(np.float32)
    runs = []
    for _ in range(2):
        G = MLPGenerator(P, DEV)
        x = G.generate(z)
        GStep(G).step(z, gp)
        GStep(G).step(z[:1000], gp[:1000])
        runs.append((x, G.params()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_twenty_train_iterations_vs_float64():
    """GanTrainer 'train' from one init and one host RNG stream against the float64 restatement (test_synthetic_train_cpu.train_iteration).
    Bound: the same 20 iterations of the restatement in float32 on the CPU drift from float64 by at most 8.1e-4 of a tensor's largest
    entry (seeds 0-3, worst: discriminator/d_fc2/bias; G's own worst 1.5e-4), and the BN-fed biases of G reach 1e-10 where float64 keeps
    them at ~1e-18.  Held here: 5e-3 of the largest entry (6x that fp32 drift) and 1e-8 absolute for the BN-fed biases."""
    from cgs_amd.datasets import NoiseDataset, ToyDataset
    from cgs_amd.synthetic import GanTrainer, MLPDiscriminator, MLPGenerator
    seed = 0
    P0 = {**MLPGenerator.init_params(seed), **MLPDiscriminator.init_params(seed + 100)}
    np.random.seed(seed)
    tr = GanTrainer(MLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV), ToyDataset("Imbal-8Gaussians", 10.0, 0.9), NoiseDataset(), 1000)
    for _ in range(20):
        tr.iteration("train")
    got = {k: v for k, v in {**tr.G.params(), **tr.D.params()}.items()}
    state_after = np.random.get_state()[1].copy()
    Q = R.to_torch(P0, torch.float64)
    np.random.seed(seed)
    data, noise = ToyDataset("Imbal-8Gaussians", 10.0, 0.9), NoiseDataset()
    for _ in range(20):
        R.train_iteration(Q, data, noise, 1000, torch.float64)
    assert np.array_equal(state_after, np.random.get_state()[1]), "the host RNG stream diverged from the reference's"
    bn_biases = [f"generator/g_fc{i}/bias" for i in range(1, 6)]
    worst = {}
    for k in got:
        if k in bn_biases:
            assert host(got[k]).abs().max().item() < 1e-8, k
        else:
            worst[k] = rel_err(got[k], Q[k])
    print("20 train iterations, max |fp32 GPU - fp64| / max|fp64|:", max(worst.values()), max(worst, key=worst.get))
    assert max(worst.values()) < 5e-3, worst


def test_paper_experiment_end_to_end(tmp_path):
    """synthetic/main.py on the device, BASELINE config 1: train the GAN (Imbal-8Gaussians, ratio 0.9, scale 10, B = 1000) for 1000
    iterations from a seeded init and save it (the "early terminated GAN", iteration 1000), load that checkpoint, shape D on refined
    samples with lrd = 8e-3 (run_shaping.sh), then the collaborative evaluation of main.py:215-263 with G in training mode as the proposer.
    Asserted: outcome-level facts, not the published numbers (a fp32 GAN run diverges from any other run).  The bars were checked on this
    same device pipeline over five seeds (gpu seeds table in DESIGN.md section 10; the float64 restatement takes minutes per seed on a CPU
    and was not run end to end).  The evaluation uses 5000 rows instead of the reference's eval_size = 10 000 to keep the test near a minute."""
    from cgs_amd.datasets import NoiseDataset, ToyDataset
    from cgs_amd.synthetic import Gan, GanTrainer, MLPDiscriminator, MLPGenerator, Refiner, evaluate_collaborative
    np.random.seed(2019)
    data, noise = ToyDataset("Imbal-8Gaussians", 10.0, 0.9), NoiseDataset()
    tr = GanTrainer(MLPGenerator.init(1), MLPDiscriminator.init(2), data, noise, 1000, lrd=1e-2, lrg=5e-3)
    paths = tr.run(1001, "train", save_every=1000, save_prefix=str(tmp_path / "Imbal-8Gaussians"))
    assert [p.rsplit("-", 1)[1] for p in paths] == ["1000.safetensors"]
    G, D = GanTrainer.load(paths[0], DEV)
    refiner = Refiner(types.SimpleNamespace(rollout_steps=50, rollout_rate=0.1, rollout_method="ladam"))
    refiner.set_env(Gan(D), None, data)
    GanTrainer(G, D, data, noise, 1000, lrd=8e-3, refiner=refiner).run(1000, "shape")
    E = 5000
    eval_batch = G.generate(noise.next_batch(E)).cpu().numpy()
    target = data.next_batch(E)
    out = evaluate_collaborative(refiner, D, G, eval_batch, target, data.centeroids, data.std)
    readme = {"standard": (0.20, 0.44), "refinement": (0.915, 0.042), "collaborate": (0.96, 0.018)}
    print("\n%-12s %8s %8s %8s %8s   %s" % ("", "good", "kl", "js", "eff", "README good / js"))
    for k in ("standard", "refinement", "collaborate"):
        o = out[k]
        print("%-12s %8.3f %8.3f %8.3f %8s   %.3f / %.3f" % (k, o["good"], o["kl"], o["js"], "%.3f" % o["eff"] if "eff" in o else "-", *readme[k]))
    s, r, c = out["standard"], out["refinement"], out["collaborate"]
    # bars that held on all five seeds; seed 1's shaped D barely helps (good 0.287 / 0.294 / 0.293), and
    # collaborative vs refined good-rate went either way (+0.09, -0.001, +0.08, +0.12, -0.002), so only a 0.01 slack is held there
    assert s["good"] < 0.6 and s["js"] > 0.1                        # the early-terminated GAN: many samples off the modes
    assert r["good"] > s["good"]                                     # refinement moves samples onto the modes
    assert c["good"] > s["good"] and c["good"] > r["good"] - 0.01    # collaboration keeps that ...
    assert c["js"] < r["js"] and c["js"] < s["js"] and c["kl"] < s["kl"]      # ... and matches the target distribution better
    assert 0.0 < c["eff"] <= 1.0
