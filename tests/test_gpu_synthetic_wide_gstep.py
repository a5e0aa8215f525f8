"""The G step of the 2-D generator at 65..256 hidden units (csrc/mlp2d_wide_gstep.hip: cgs_mlp2d_wide_g_step) and the trainer built on it
(Gan2DTrainer: all four modes at any supported widths), against the float64 torch restatement of test_synthetic_train_cpu.py.

Bars: every bar is 4 x the error of the same restatement run in float32 on the CPU on the case's own inputs against its float64 run
(the device adds in group and chunk order and torch does not; 4 x is what the wide D step's and the wide forward's tests held).  The
float32-CPU figures are the constants beside each test; test_synthetic_wide_gstep_cpu.py holds the measures.

ReLU kinks: every gradient case's seed is the first one whose float64 forward has no BN output y = gamma xhat + beta closer to 0 than
m = 4 max |y_float32-CPU - y_float64| (W.kink_margin), asserted in the test: an entry inside that margin may take the other branch on
the device, and one flip moves a gradient by far more than rounding does."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_synthetic_train_cpu as R
import test_synthetic_wide_gstep_cpu as W
from test_gpu_synthetic_train import host, perturbed_params, rel_err

DEV = "cuda:0"


def TILE(B):
    """mlpw_tile of csrc/mlp2d_wide.h: T = 32 where the busiest CU then carries strictly less, T = 64 on a tie"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n64, n32 = -(-B // 64), -(-B // 32)
    return 32 if 2 * -(-n64 // cus) > -(-n32 // cus) else 64


def named(gw, gb):
    return {**{f"generator/g_fc{i + 1}/kernel": host(t) for i, t in enumerate(gw)},
            **{f"generator/g_fc{i + 1}/bias": host(t) for i, t in enumerate(gb)}}


# ---- 1. gradients against float64 autograd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nl,B,shift", sorted(W.GRAD_CASES))
def test_gradients_vs_float64_autograd(nh, nl, B, shift):
    """Measured on the MI355X (256 CUs), device / float32 CPU, kernels then BN-fed biases:
        (65, 2, 33, 0)      6.1e-7 / 6.5e-7    4.9e-8 / 5.7e-7
        (96, 3, 37, 0)      1.5e-6 / 1.0e-6    9.5e-8 / 3.5e-7
        (129, 4, 65, 0)     1.6e-6 / 1.4e-6    1.2e-7 / 6.6e-7
        (200, 6, 97, 0)     8.3e-6 / 2.9e-6    1.4e-7 / 1.7e-6
        (256, 4, 257, 0)    3.8e-6 / 3.0e-6    5.7e-7 / 6.4e-7
        (256, 2, 1000, 0)   1.7e-6 / 1.1e-6    3.6e-7 / 3.0e-7
        (96, 2, 8200, 0)    1.2e-6 / 4.7e-7    2.9e-7 / 3.6e-7
        (256, 6, 257, 8)    2.3e-4 / 9.4e-4    6.6e-7 / 2.6e-5
        (256, 6, 1000, 8)   2.2e-3 / 2.4e-3    7.1e-7 / 4.6e-6
        (96, 3, 8200, 8)    2.2e-5 / 4.8e-5    1.4e-6 / 2.2e-6
        (256, 6, 8200, 8)   4.2e-4 / 2.7e-4    3.2e-6 / 1.0e-5
    Before xhat was centred in the BN backward, (256, 2, 1000, 0) left 1.6e-6 in the biases and (96, 3, 8200, 8)
    4.4e-4 / 3.7e-5, both past their bars: the forward's mean(xhat) is not zero, and the sum of da over the batch carried it."""
    from cgs_amd.synthetic import WideGStep, WideMLPGenerator
    seed, f32_k, f32_b = W.GRAD_CASES[nh, nl, B, shift]
    if B == 8200 and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert TILE(8200) == 64 and TILE(1000) == 32
    P, z, gp = W.case_inputs(seed, nh, nl, B, shift)
    lo, m = W.kink_margin(P, z)
    assert lo >= m, f"seed {seed}: a BN output at {lo:.2e} lies inside the float32 margin {m:.2e}"
    gw, gb = WideGStep(WideMLPGenerator(P, DEV)).grads(z, gp)
    ref, _ = W.g_step_ref(P, z, gp, torch.float64)
    ek, eb = W.grad_errs(named(gw, gb), ref, nl)
    print(f"({nh}, {nl}, {B}, shift {shift}) seed {seed}: kernels {ek:.2e} (float32 CPU {f32_k:.1e})  BN-fed biases {eb:.2e} (float32 CPU {f32_b:.1e})")
    assert ek < 4 * f32_k and eb < 4 * f32_b, (ek, eb)


# ---- 2. lr = 0 and the update -----------------------------------------------------------------------------------------------------
def test_lr_zero_writes_nothing_and_the_step_is_two_roundings():
    from cgs_amd.synthetic import WideGStep, WideMLPGenerator
    nh, nl, B = 200, 6, 97
    P, z, gp = W.case_inputs(1, nh, nl, B)
    G = WideMLPGenerator(P, DEV)
    step = WideGStep(G, lrg=5e-3)
    before = {k: v.detach().clone() for k, v in G.params().items()}
    gw, gb = step.grads(z, gp)
    after = G.params()
    for k in before:
        if "moving_" in k:
            assert not torch.equal(before[k], after[k]), k          # the forward ran
        else:
            assert torch.equal(before[k], after[k]), k
    gw, gb = [t.clone() for t in gw], [t.clone() for t in gb]
    # x of the step's own forward: the bits of generate on the same z (same variables: the step's forward comes before its update)
    G2 = WideMLPGenerator(P, DEV)
    x = step.step(z, gp, want_x=True)
    assert torch.equal(x, G2.generate(z))
    lr = torch.tensor(5e-3, dtype=torch.float32, device=DEV)
    for i in range(nl):
        assert torch.equal(G.w[i], before[f"generator/g_fc{i + 1}/kernel"] - lr * gw[i]), i
        assert torch.equal(G.b[i], before[f"generator/g_fc{i + 1}/bias"] - lr * gb[i]), i
    assert all(torch.equal(a, b) for a, b in zip(step.gw, gw))       # same batch statistics, same gradient: the moving averages play no part
    after = G.params()
    for k in before:
        if k.endswith("/gamma") or k.endswith("/beta"):
            assert torch.equal(before[k], after[k]), k


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
def test_step_is_deterministic():
    from cgs_amd.synthetic import WideGStep, WideMLPGenerator
    P = perturbed_params(21, 256, 6)
    rs = np.random.RandomState(22)
    z, gp = rs.randn(10000, 2).astype(np.float32), (1e-3 * rs.randn(10000, 2)).astype(np.float32)
    runs = []
    for _ in range(2):
        G = WideMLPGenerator(P, DEV)
        step = WideGStep(G)
        step.step(z, gp)                       # T = 64 on 256 CUs, 16 chunks of 640 samples
        step.step(z[:1000], gp[:1000])         # T = 32, 8 chunks of 128
        runs.append({**G.params(), **{"g" + k: v for k, v in named(step.gw, step.gb).items()}})
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


# ---- 4. the 64 x 6 net embedded in 96 and in 256 units ----------------------------------------------------------------------------
# What the two float32 paths (the 64-unit net, the same net embedded) differ by on the CPU restatement, W.grad_errs of the embedded
# run's inner block against the 64-unit run: (0.0, 4.7e-7) at 96 units, (6.6e-7, 4.7e-7) at 256.  The extra units add exact zeros, so
# torch's two runs differ by its own blocking alone, and at 96 units not at all; the device's two steps are different kernels with
# different summation orders, and neither can be closer to the other than one float32 evaluation is to float64.  That error, the
# float32 CPU run of the 64 x 6 net against float64 on these inputs, is (1.0e-6, 4.7e-7): the figure is the larger of the two.
EMBED_F32 = {96: (1.0e-6, 4.7e-7), 256: (1.0e-6, 4.7e-7)}


@pytest.mark.parametrize("wide", [96, 256])
def test_embedded_64_unit_net_vs_the_narrow_g_step(wide):
    from cgs_amd.synthetic import GStep, MLPGenerator, WideGStep, WideMLPGenerator
    P, z, gp = W.case_inputs(W.EMBED_SEED, 64, 6, 1000)
    E = W.embed(P, wide)
    gn = named(*GStep(MLPGenerator(P, DEV)).grads(z, gp))
    gwide = named(*WideGStep(WideMLPGenerator(E, DEV)).grads(z, gp))
    inner = {k: v[tuple(slice(0, n) for n in gn[k].shape)] for k, v in gwide.items()}
    ek, eb = W.grad_errs(inner, gn, 6)
    # the BN-fed biases of the narrow step are rounding noise themselves: grad_errs' bias measure is the wide step's own
    f32_k, f32_b = EMBED_F32[wide]
    print(f"embedded at {wide}: kernels {ek:.2e} (float32 CPU {f32_k:.1e})  BN-fed biases {eb:.2e} (float32 CPU {f32_b:.1e})")
    assert ek < 4 * f32_k and eb < 4 * f32_b
    for k, v in gwide.items():                 # a silent unit's pre-activation, xhat, dxhat and da are exact zeros
        outer = v.clone()
        outer[tuple(slice(0, n) for n in gn[k].shape)] = 0
        assert (outer == 0).all(), k


# ---- 5. five carried steps --------------------------------------------------------------------------------------------------------
CARRIED_F32 = 4.2e-7         # worst tensor's drift of the float32 CPU restatement over the same five steps (W.CARRIED, W.CARRIED_SEED)


def drift(got, Q):
    """worst tensor's max |difference| / max |float64|; tensors that float64 keeps at rounding level (the BN-fed biases: their gradient
    is zero in exact arithmetic) are measured against their layer's kernel instead"""
    worst = {}
    for k, v in got.items():
        want = Q[k].double()
        scale = want.abs().max()
        if k.startswith("generator/g_fc") and k.endswith("/bias"):
            scale = max(scale, Q[k.replace("/bias", "/kernel")].double().abs().max())
        worst[k] = ((host(v) - want).abs().max() / scale).item()
    k = max(worst, key=worst.get)
    return worst[k], k


def test_five_carried_steps_vs_float64():
    from cgs_amd.synthetic import WideGStep, WideMLPGenerator
    nh, nl, B = W.CARRIED
    assert W.carried_kink_free(W.CARRIED_SEED)
    P = perturbed_params(W.CARRIED_SEED, nh, nl)
    G = WideMLPGenerator(P, DEV)
    step = WideGStep(G, lrg=5e-3)
    Q = R.to_torch(P, torch.float64)
    for z, gp in W.carried_batches(W.CARRIED_SEED):
        step.step(z, gp)
        R.g_step(Q, torch.as_tensor(z, dtype=torch.float64), torch.as_tensor(gp, dtype=torch.float64), 5e-3)
    err, name = drift(G.params(), Q)
    print(f"5 carried G steps at {W.CARRIED}: worst {err:.2e} ({name}); float32 CPU {CARRIED_F32:.2e}")
    assert err < 4 * CARRIED_F32, (err, name)


# ---- 6. it trains -----------------------------------------------------------------------------------------------------------------
# the float64 restatement alone, 50 steps at lr 0.05 on the same z and target: 1/2 mean |x - target|^2 before and after
TRAINS_F64 = (1.7012, 0.8553)


def trains_inputs():
    rs = np.random.RandomState(51)
    return perturbed_params(50, 96, 3), rs.randn(256, 2).astype(np.float32), rs.randn(256, 2).astype(np.float32)


def test_it_trains():
    from cgs_amd.synthetic import WideGStep, WideMLPGenerator
    assert TRAINS_F64[1] < TRAINS_F64[0]
    P, z, target = trains_inputs()
    G = WideMLPGenerator(P, DEV)
    step = WideGStep(G, lrg=0.05)
    zd, td = torch.as_tensor(z).to(DEV), torch.as_tensor(target).to(DEV)
    loss = lambda x: 0.5 * ((x - td) ** 2).sum(1).mean().item()
    first = loss(G.generate(zd))
    for _ in range(50):
        x = G.generate(zd)
        step.step(zd, (x - td) / z.shape[0])
    last = loss(G.generate(zd))
    print(f"50 steps: {first:.4f} -> {last:.4f}; float64 restatement {TRAINS_F64[0]:.4f} -> {TRAINS_F64[1]:.4f}")
    assert abs(first - TRAINS_F64[0]) < 1e-3 * TRAINS_F64[0] and last < first


# ---- 7. Gan2DTrainer --------------------------------------------------------------------------------------------------------------
def gan_params(seed, g_shape, d_shape):
    from cgs_amd.synthetic import MLPDiscriminator
    return {**perturbed_params(seed, *g_shape), **MLPDiscriminator.init_params(seed + 100, *d_shape)}


def dataset():
    from cgs_amd.datasets import NoiseDataset, ToyDataset
    return ToyDataset("25Gaussians", scale=1.0), NoiseDataset()


def restated_train(P0, seed, iters, B, dtype):
    Q = R.to_torch(P0, dtype)
    np.random.seed(seed)
    data, noise = dataset()
    for _ in range(iters):
        R.train_iteration(Q, data, noise, B, dtype)
    return Q, np.random.get_state()[1].copy()


def trainer_drift(got, Q):
    """test_gpu_synthetic_wide_gen.py's measure: tensors that float64 keeps at rounding level are held to 1e-8 absolute"""
    worst = {}
    for k, v in got.items():
        want = Q[k].double()
        if want.abs().max().item() < 1e-12:
            assert host(v).abs().max().item() < 1e-8, k
        else:
            worst[k] = ((host(v) - want).abs().max() / want.abs().max()).item()
    k = max(worst, key=worst.get)
    return worst[k], k


# worst tensor's drift of the float32 CPU restatement from the float64 one over the case's own two train iterations
TRAIN_F32 = {(96, 3, 100): 3.1e-6,         # discriminator/d_fc3/bias
             (256, 6, 256): 2.2e-4}        # discriminator/d_fc6/bias


@pytest.mark.parametrize("nh,nl,B", sorted(TRAIN_F32))
def test_two_train_iterations_vs_float64(nh, nl, B):
    from cgs_amd.synthetic import Gan2DTrainer, MLPDiscriminator, WideGStep, WideMLPGenerator
    seed = nh
    P0 = gan_params(seed, (nh, nl), (nh, nl))
    np.random.seed(seed)
    data, noise = dataset()
    tr = Gan2DTrainer(WideMLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV), data, noise, B)
    assert type(tr.gstep) is WideGStep
    for _ in range(2):
        tr.iteration("train")
    state = np.random.get_state()[1].copy()
    Q, want_state = restated_train(P0, seed, 2, B, torch.float64)
    assert np.array_equal(state, want_state), "the host RNG stream diverged from the reference's"
    err, name = trainer_drift({**tr.G.params(), **tr.D.params()}, Q)
    print(f"2 train iterations at {nh} x {nl}, B = {B}: worst {err:.2e} ({name}); float32 CPU {TRAIN_F32[nh, nl, B]:.2e}")
    assert err < 4 * TRAIN_F32[nh, nl, B], (err, name)


def test_other_modes_checkpoint_and_the_old_refusal(tmp_path):
    from cgs_amd.lib import CgsError
    from cgs_amd.synthetic import Gan, Gan2DTrainer, MLPDiscriminator, Refiner, WideGanTrainer, WideMLPGenerator
    P0 = gan_params(6, (256, 6), (256, 6))
    np.random.seed(6)
    data, noise = dataset()
    G, D = WideMLPGenerator(P0, DEV), MLPDiscriminator(P0, DEV)
    refiner = Refiner(types.SimpleNamespace(rollout_steps=10, rollout_rate=0.1, rollout_method="ladam"))
    refiner.set_env(Gan(D), None, data)
    old = WideGanTrainer(G, D, data, noise, 100)
    before = np.random.get_state()
    with pytest.raises(CgsError, match="G step"):
        old.iteration("train")
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    tr = Gan2DTrainer(G, D, data, noise, 100, refiner=refiner)
    for mode in ("calibrate", "shape", "test", "train"):
        tr.iteration(mode)
    assert all(torch.isfinite(v).all() for v in {**G.params(), **D.params()}.values()) and torch.isfinite(tr.d_loss).all()
    path = str(tmp_path / "gan2d.safetensors")
    tr.save(path)
    G2, D2 = Gan2DTrainer.load(path, DEV)
    assert type(G2) is WideMLPGenerator and D2.nhidden == 256
    want, got = {**G.params(), **D.params()}, {**G2.params(), **D2.params()}
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)


# ---- 8. class surface ---------------------------------------------------------------------------------------------------------------
def test_class_surface():
    from cgs_amd.lib import CgsError
    from cgs_amd.synthetic import GStep, MLPGenerator, WideGStep, WideMLPGenerator, g_stepper
    narrow, wide = MLPGenerator(perturbed_params(1), DEV), WideMLPGenerator(perturbed_params(2, 96, 3), DEV)
    assert type(g_stepper(narrow)) is GStep and type(g_stepper(wide)) is WideGStep and isinstance(g_stepper(wide), GStep)
    assert g_stepper(wide, 0.25).lrg == 0.25
    with pytest.raises(CgsError, match="GStep"):
        WideGStep(narrow)
    z = np.zeros((8, 2), np.float32)
    with pytest.raises(CgsError, match="not built"):
        GStep(wide).grads(z, z)
    with pytest.raises(CgsError, match="not built"):
        wide._ws_bytes(8, True)
    with pytest.raises(CgsError, match="grad_plugin shape"):
        WideGStep(wide).grads(z, np.zeros((7, 2), np.float32))
    step = WideGStep(wide)
    assert [t.shape for t in step.gw] == [t.shape for t in wide.w] and [t.shape for t in step.gb] == [t.shape for t in wide.b]
