"""The forward of the 2-D generator at 65..256 hidden units (csrc/mlp2d_wide_gen.hip: cgs_mlp2d_wide_gen_fwd) and the trainer built on it
(WideGanTrainer: calibrate | shape | test at 256 x 6, train while G is narrow), against the float64 torch restatement of
test_synthetic_train_cpu.py, which is width-agnostic.

Tile sizes: the library picks T = 32 or 64 samples per workgroup from B and the CU count (mlpw_tile, restated in TILE below); on the
MI355X's 256 CUs every B <= 8192 runs T = 32 and 8193 <= B <= 16384 runs T = 64, hence the B = 8200 cases.

The float32 figures quoted beside the bars are the same restatement run in float32 on the CPU on exactly the inputs of the case, against
its float64 run (max |difference| / max |float64| per tensor)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_synthetic_train_cpu as R
from test_gpu_synthetic_train import host, perturbed_params, rel_err

DEV = "cuda:0"


def TILE(B):
    """mlpw_tile of csrc/mlp2d_wide.h: T = 32 where the busiest CU then carries strictly less, T = 64 on a tie"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n64, n32 = -(-B // 64), -(-B // 32)
    return 32 if 2 * -(-n64 // cus) > -(-n32 // cus) else 64


def stat_errs(st, stats):
    """the narrow test's scaling: mean against max(|mean| + std), variance against max variance; worst over the BN layers"""
    em = max(((host(st[k, 0]) - m).abs().max() / (m.abs() + v.sqrt()).max()).item() for k, (m, v) in enumerate(stats))
    ev = max(((host(st[k, 1]) - v).abs().max() / v.max()).item() for k, (m, v) in enumerate(stats))
    return em, ev


def moving_err(G, Q):
    from cgs_amd.synthetic import _bn_name
    worst = 0.0
    for k in range(G.nlayers - 1):
        for name, dev_t in (("moving_mean", G.moving_mean[k]), ("moving_variance", G.moving_variance[k])):
            want = Q[f"{_bn_name(k)}/{name}"]
            worst = max(worst, ((host(dev_t) - want).abs().max() / want.abs().max()).item())
    return worst


def three_training_calls(nh, nl, B, tol_x, tol_stat, tol_moving):
    from cgs_amd.synthetic import WideMLPGenerator
    P = perturbed_params(B + nh, nh, nl)
    G = WideMLPGenerator(P, DEV)
    Q = R.to_torch(P, torch.float64)
    rs = np.random.RandomState(B)
    for call in range(3):
        z = rs.randn(B, 2).astype(np.float32)
        x, st = G.generate(z, batch_stats=True)
        assert x.shape == (B, 2) and st.shape == (nl - 1, 2, nh)
        stats = []
        ref = R.g_forward(Q, torch.as_tensor(z, dtype=torch.float64), stats=stats)
        ex, (em, ev) = rel_err(x, ref), stat_errs(st, stats)
        print(f"({nh}, {nl}, {B}) call {call}: x {ex:.2e}  mean {em:.2e}  variance {ev:.2e}")
        assert ex < tol_x and em < tol_stat and ev < tol_stat, (call, ex, em, ev)
        if call in (0, 2):                      # after 1 and after 3 training-mode calls
            e = moving_err(G, Q)
            print(f"({nh}, {nl}, {B}) call {call}: moving statistics {e:.2e}")
            assert e < tol_moving, (call, e)


SHAPES = [(65, 2, 33),          # first and last layer only
          (96, 3, 37),
          (129, 4, 65),         # nh just over a 32-column strip, B = two groups + 1
          (200, 6, 97),         # nh not a multiple of the slab
          (128, 6, 1000),
          (256, 6, 1000),
          (256, 6, 8200)]       # T = 64 tiles on 256 CUs


@pytest.mark.parametrize("nh,nl,B", SHAPES)
def test_training_forward_and_moving_averages_vs_float64(nh, nl, B):
    """The narrow test's bars: 1e-5 relative for x, for mean / variance as scaled there and for the moving statistics after calls 1 and 3.
    float32 on the CPU on these inputs: <= 2.4e-6 (x), 1.2e-6 (statistics), 1.5e-7 (moving statistics)."""
    if B == 8200 and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert TILE(8200) == 64 and TILE(1000) == 32
    three_training_calls(nh, nl, B, 1e-5, 1e-5, 1e-5)


# B = 2 at 256 x 6 is ill-conditioned: a unit's variance is a quarter of the squared difference of two rounded pre-activations, and
# (a - mean) * rstd is +-1 whatever that difference is, so a relative error of the variance passes through undamped, layer after layer.
# float32 on the CPU, on exactly these inputs (perturbed_params(258, 256, 6), RandomState(2)), worst of the three calls:
B2_F32_X, B2_F32_STAT, B2_F32_MOVING = 1.0e-4, 5.7e-5, 2.7e-5
B2_BARS = (4 * B2_F32_X, 4 * B2_F32_STAT, 4 * B2_F32_MOVING)


def test_training_forward_on_a_batch_of_two():
    three_training_calls(256, 6, 2, *B2_BARS)


@pytest.mark.parametrize("nh,nl,B", [(256, 6, 1000), (200, 6, 97)])
def test_inference_forward_vs_float64(nh, nl, B):
    """The moving statistics, and no variable moves.  float32 on the CPU on these inputs: <= 1.7e-6."""
    from cgs_amd.synthetic import WideMLPGenerator
    P = perturbed_params(B + nh, nh, nl)
    G = WideMLPGenerator(P, DEV)
    before = {k: v.clone() for k, v in G.params().items()}
    z = np.random.RandomState(B).randn(B, 2).astype(np.float32)
    x = G.generate(z, is_training=False)
    ref = R.g_forward(R.to_torch(P, torch.float64), torch.as_tensor(z, dtype=torch.float64), training=False)
    print(f"inference ({nh}, {nl}, {B}): x {rel_err(x, ref):.2e}")
    assert rel_err(x, ref) < 1e-5
    after = G.params()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_inference_rows_do_not_depend_on_the_batch():
    """A row's bits depend neither on the batch around it nor on the tile size that batch gets (8200: T = 64; 1000: T = 32)."""
    from cgs_amd.synthetic import WideMLPGenerator
    z = torch.from_numpy(np.random.RandomState(9).randn(8200, 2).astype(np.float32)).to(DEV)
    G = WideMLPGenerator(perturbed_params(7, 200, 6), DEV)
    assert torch.equal(G.generate(z[:97], is_training=False)[:33], G.generate(z[:33], is_training=False))
    G = WideMLPGenerator(perturbed_params(8, 256, 6), DEV)
    small = G.generate(z[:1000], is_training=False)
    assert torch.equal(G.generate(z, is_training=False)[:1000], small)
    assert torch.equal(G.generate(z[:97], is_training=False)[:33], G.generate(z[:33], is_training=False))


def test_bessel_rule_is_the_recorded_one():
    """Moving variance after one call on a batch of 2 from moving_variance = 0: 0.1 * the UNBIASED variance, twice the biased one."""
    from cgs_amd.synthetic import WideMLPGenerator
    P = perturbed_params(5, 96, 2)
    P["generator/BatchNorm/moving_variance"][:] = 0
    G = WideMLPGenerator(P, DEV)
    z = np.random.RandomState(0).randn(2, 2).astype(np.float32)
    _, st = G.generate(z, batch_stats=True)
    np.testing.assert_allclose(G.moving_variance[0].cpu().numpy(), 0.1 * 2 * st[0, 1].cpu().numpy(), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("wide", [96, 256])
def test_embedded_64_unit_net_vs_the_narrow_generator(wide):
    """The 64 x 6 net in the first 64 of `wide` units (the others: zero weights in and out, zero bias, gamma 1, beta 0) is the same function:
    the new kernels against the shipped ones on the same z.  Two float32 results, each within 1e-5 of float64: 2e-5."""
    from cgs_amd.synthetic import MLPGenerator, WideMLPGenerator
    P = perturbed_params(31)
    E = WideMLPGenerator.init_params(0, wide, 6)
    for k, v in P.items():
        e = np.zeros_like(E[k]) if k.endswith("/kernel") or k.endswith("/bias") else E[k]
        e[tuple(slice(0, n) for n in v.shape)] = v
        E[k] = e
    z = np.random.RandomState(32).randn(1000, 2).astype(np.float32)
    xn, sn = MLPGenerator(P, DEV).generate(z, batch_stats=True)
    xw, sw = WideMLPGenerator(E, DEV).generate(z, batch_stats=True)
    ex = rel_err(xw, host(xn))
    em, ev = stat_errs(sw[:, :, :64], [(host(sn[k, 0]), host(sn[k, 1])) for k in range(5)])
    print(f"embedded at {wide}: x {ex:.2e}  mean {em:.2e}  variance {ev:.2e}")
    assert ex < 2e-5 and em < 2e-5 and ev < 2e-5
    assert (sw[:, :, 64:] == 0).all()


def test_forward_is_deterministic():
    from cgs_amd.synthetic import WideMLPGenerator
    P = perturbed_params(21, 256, 6)
    z = np.random.RandomState(22).randn(3, 10000, 2).astype(np.float32)
    runs = []
    for _ in range(2):
        G = WideMLPGenerator(P, DEV)
        xs = [G.generate(z[i]) for i in range(3)] + [G.generate(z[i, :1000]) for i in range(3)]
        runs.append((xs, G.params()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


# ---- WideGanTrainer ---------------------------------------------------------------------------------------------------------
def gan_params(seed, g_shape, d_shape):
    from cgs_amd.synthetic import MLPDiscriminator
    return {**perturbed_params(seed, *g_shape), **MLPDiscriminator.init_params(seed + 100, *d_shape)}


def dataset():
    from cgs_amd.datasets import NoiseDataset, ToyDataset
    return ToyDataset("25Gaussians", scale=1.0), NoiseDataset()


def calibrate_iteration(P, data, noise, B, dtype, lrd=1e-2):
    """synthetic/main.py:352-365, mode calibrate, on the {G, D} tensors of P"""
    real = torch.as_tensor(data.next_batch(B), dtype=dtype)
    z = torch.as_tensor(noise.next_batch(B), dtype=dtype)
    with torch.no_grad():
        fake = R.g_forward(P, z)
    R.d_step(P, real, fake, lrd)


def restated(P0, seed, iters, B, dtype, train):
    """-> ({name: tensor} after `iters` iterations of the restatement from host RNG seed `seed`, the RNG state afterwards)"""
    Q = R.to_torch(P0, dtype)
    np.random.seed(seed)
    data, noise = dataset()
    for _ in range(iters):
        if train:
            R.train_iteration(Q, data, noise, B, dtype)
        else:
            calibrate_iteration(Q, data, noise, B, dtype)
    return Q, np.random.get_state()[1].copy()


def drift(got, Q):
    """worst tensor's max |difference| / max |float64|; tensors that float64 keeps at rounding level (the BN-fed biases of G in train
    mode, ~1e-18) are held to 1e-8 absolute instead, as in the narrow trainer's test"""
    worst = {}
    for k, v in got.items():
        want = Q[k].double()
        if want.abs().max().item() < 1e-12:
            assert host(v).abs().max().item() < 1e-8, k
        else:
            worst[k] = ((host(v) - want).abs().max() / want.abs().max()).item()
    k = max(worst, key=worst.get)
    return worst[k], k


# worst tensor's drift of the float32 CPU restatement from the float64 one over the case's own iterations
CALIBRATE_F32 = {(96, 3, 100): 2.9e-7,        # discriminator/d_fc2/bias
                 (256, 6, 256): 3.4e-3}       # discriminator/d_fc1/bias
TRAIN_F32 = 9.3e-6                            # 2 train iterations, 64 x 6 G and 128 x 3 D, B = 500: discriminator/d_fc3/bias


@pytest.mark.parametrize("nh,nl,B", sorted(CALIBRATE_F32))
def test_five_calibrate_iterations_vs_float64(nh, nl, B):
    from cgs_amd.synthetic import MLPDiscriminator, WideGanTrainer, WideMLPGenerator
    seed = nh
    P0 = gan_params(seed, (nh, nl), (nh, nl))
    np.random.seed(seed)
    data, noise = dataset()
    tr = WideGanTrainer(WideMLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV), data, noise, B)
    for _ in range(5):
        tr.iteration("calibrate")
    state = np.random.get_state()[1].copy()
    Q, want_state = restated(P0, seed, 5, B, torch.float64, train=False)
    assert np.array_equal(state, want_state), "the host RNG stream diverged from the reference's"
    err, name = drift({**tr.G.params(), **tr.D.params()}, Q)
    print(f"5 calibrate iterations at {nh} x {nl}, B = {B}: worst {err:.2e} ({name}); float32 CPU {CALIBRATE_F32[nh, nl, B]:.2e}")
    assert err < 4 * CALIBRATE_F32[nh, nl, B], (err, name)


def test_two_train_iterations_with_a_narrow_g_and_a_wide_d():
    from cgs_amd.synthetic import MLPDiscriminator, MLPGenerator, WideGanTrainer
    seed, B = 3, 500
    P0 = gan_params(seed, (64, 6), (128, 3))
    np.random.seed(seed)
    data, noise = dataset()
    tr = WideGanTrainer(MLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV), data, noise, B)
    for _ in range(2):
        tr.iteration("train")
    state = np.random.get_state()[1].copy()
    Q, want_state = restated(P0, seed, 2, B, torch.float64, train=True)
    assert np.array_equal(state, want_state)
    err, name = drift({**tr.G.params(), **tr.D.params()}, Q)
    print(f"2 train iterations, 64 x 6 G and 128 x 3 D, B = {B}: worst {err:.2e} ({name}); float32 CPU {TRAIN_F32:.2e}")
    assert err < 4 * TRAIN_F32, (err, name)
    for mode in ("calibrate", "test"):
        tr.iteration(mode)


def _refiner(D, data):
    from cgs_amd.synthetic import Gan, Refiner
    r = Refiner(types.SimpleNamespace(rollout_steps=10, rollout_rate=0.1, rollout_method="ladam"))
    r.set_env(Gan(D), None, data)
    return r


def test_three_shape_iterations_at_256_x_6():
    from cgs_amd.synthetic import GanTrainer, MLPDiscriminator, MLPGenerator, WideGanTrainer, WideMLPGenerator
    states = {}
    for nh, trainer, gen in ((256, WideGanTrainer, WideMLPGenerator), (64, GanTrainer, MLPGenerator)):
        P0 = gan_params(5, (nh, 6), (nh, 6))
        np.random.seed(5)
        data, noise = dataset()
        G, D = gen(P0, DEV), MLPDiscriminator(P0, DEV)
        tr = trainer(G, D, data, noise, 256, refiner=_refiner(D, data))
        before = {k: v.clone() for k, v in {**G.params(), **D.params()}.items()}
        for _ in range(3):
            tr.iteration("shape")
        states[nh] = np.random.get_state()[1].copy()
        if nh == 64:
            continue
        after = {**G.params(), **D.params()}
        for k in before:
            if k.startswith("discriminator/") or k.endswith("/moving_mean"):
                assert not torch.equal(before[k], after[k]), k
            elif not k.endswith("/moving_variance"):
                assert torch.equal(before[k], after[k]), k
        assert all(torch.isfinite(v).all() for v in after.values()) and torch.isfinite(tr.d_loss).all()
    assert np.array_equal(states[256], states[64])          # the draws do not depend on the width


def test_train_with_a_wide_g_is_refused_before_any_draw(tmp_path):
    from cgs_amd.lib import CgsError
    from cgs_amd.synthetic import MLPDiscriminator, MLPGenerator, WideGanTrainer, WideMLPGenerator, mlp_generator
    P0 = gan_params(6, (256, 6), (256, 6))
    np.random.seed(6)
    data, noise = dataset()
    tr = WideGanTrainer(WideMLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV), data, noise, 100)
    before = np.random.get_state()
    with pytest.raises(CgsError, match="G step"):
        tr.iteration("train")
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    tr.iteration("test")
    # checkpoint round trip: the classes by width, every tensor bit-equal
    path = str(tmp_path / "wide.safetensors")
    tr.save(path)
    G, D = WideGanTrainer.load(path, DEV)
    assert type(G) is WideMLPGenerator and isinstance(G, MLPGenerator) and D.nhidden == 256
    want = {**tr.G.params(), **tr.D.params()}
    got = {**G.params(), **D.params()}
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert type(mlp_generator(perturbed_params(1), DEV)) is MLPGenerator
    with pytest.raises(CgsError, match="MLPGenerator"):
        WideMLPGenerator.init(1, nhidden=64)
    with pytest.raises(CgsError):
        WideMLPGenerator.init(1, nhidden=257)


def test_evaluate_collaborative_takes_a_wide_generator():
    from cgs_amd.synthetic import MLPDiscriminator, WideMLPGenerator, evaluate_collaborative
    P0 = gan_params(8, (256, 6), (256, 6))
    np.random.seed(2019)
    data, noise = dataset()
    G, D = WideMLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV)
    eval_batch = G.generate(noise.next_batch(500)).cpu().numpy()
    out = evaluate_collaborative(_refiner(D, data), D, G, eval_batch, data.next_batch(500), data.centeroids, data.std)
    assert set(out) == {"standard", "refinement", "collaborate"}
    for q in out.values():
        assert all(np.isfinite(v) for v in q.values()), out
    assert 0.0 < out["collaborate"]["eff"] <= 1.0
