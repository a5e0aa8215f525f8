"""The 2-D generator and its training loop, host side: the new C ABI entries, G's TF variable names and shapes, {G, D} checkpoints,
the seeded initialisers, and the 'g_' variable filter of synthetic/GAN.py:83-84.

This file also holds the torch restatement of G (synthetic/GAN.py:39-49, 83-101) and of one train iteration of synthetic/main.py:350-380
that the GPU tests (test_gpu_synthetic_train.py) compare against.  It runs in any float dtype: float64 is the reference, float32 on the CPU
measures how far plain fp32 arithmetic drifts from it."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, DECAY = 1.001e-5, 0.9          # epsilon: GAN.py's 1e-5 as TF 1.x's fused batch norm raises it (cuDNN minimum 1.001e-5)

NEW_SYMBOLS = ("cgs_mlp2d_gen_ws_bytes", "cgs_mlp2d_gen_fwd", "cgs_mlp2d_g_step")


# ---- restatement ------------------------------------------------------------------------------------------------------------
def bn_name(k):
    return "generator/BatchNorm" if k == 0 else f"generator/BatchNorm_{k}"


def gan_py_variables(nhidden, nlayers):
    """(name, shape, trainable) of every variable synthetic/GAN.py:28-49 creates, in creation order (build_model: D on the real input
    first, then G, GAN.py:57-63): tf.layers.dense -> <scope>/kernel, /bias; tf.contrib.layers.batch_norm(scale=True) -> BatchNorm[_k]/
    beta, gamma (trainable), moving_mean, moving_variance (not trainable)."""
    out = []
    dims = [2] + [nhidden] * (nlayers - 1) + [1]
    for i in range(nlayers):
        out += [(f"discriminator/d_fc{i + 1}/kernel", (dims[i], dims[i + 1]), True), (f"discriminator/d_fc{i + 1}/bias", (dims[i + 1],), True)]
    dims = [2] + [nhidden] * (nlayers - 1) + [2]
    for i in range(nlayers):
        out += [(f"generator/g_fc{i + 1}/kernel", (dims[i], dims[i + 1]), True), (f"generator/g_fc{i + 1}/bias", (dims[i + 1],), True)]
        if i < nlayers - 1:
            out += [(f"{bn_name(i)}/{v}", (nhidden,), v in ("beta", "gamma")) for v in ("beta", "gamma", "moving_mean", "moving_variance")]
    return out


def g_vars(nhidden, nlayers):
    """GAN.py:82-84: t_vars = tf.trainable_variables(); g_vars = [var for var in t_vars if 'g_' in var.name]."""
    return [n for n, _, trainable in gan_py_variables(nhidden, nlayers) if trainable and "g_" in n + ":0"]


def to_torch(P, dtype):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone() for k, v in P.items()}


def nlayers_of(P, prefix):
    n = 1
    while f"{prefix}{n + 1}/kernel" in P:
        n += 1
    return n


def g_forward(P, z, training=True, update=True, stats=None):
    """G(z) on the tensors of P.  Training mode: batch mean / biased variance, and (update) the moving averages move in place with
    v -= (v - value) * (1 - decay), value = the batch mean / the Bessel-corrected batch variance.  Inference mode: the moving statistics.
    ``stats``: a list that receives (mean, biased var) per BN layer."""
    n = nlayers_of(P, "generator/g_fc")
    h = z
    for i in range(n):
        a = h @ P[f"generator/g_fc{i + 1}/kernel"] + P[f"generator/g_fc{i + 1}/bias"]
        if i == n - 1:
            return a
        bn = bn_name(i)
        mm, mv = P[f"{bn}/moving_mean"], P[f"{bn}/moving_variance"]
        if training:
            mean, var = a.mean(0), a.var(0, unbiased=False)
            if stats is not None:
                stats.append((mean.detach().clone(), var.detach().clone()))
            if update:
                B = a.shape[0]
                with torch.no_grad():
                    mm -= (mm - mean.detach()) * (1 - DECAY)
                    mv -= (mv - var.detach() * (B / (B - 1))) * (1 - DECAY)
        else:
            mean, var = mm, mv
        h = torch.relu((a - mean) / torch.sqrt(var + EPS) * P[f"{bn}/gamma"] + P[f"{bn}/beta"])


def d_logits(P, x):
    n = nlayers_of(P, "discriminator/d_fc")
    h = x
    for i in range(n):
        h = h @ P[f"discriminator/d_fc{i + 1}/kernel"] + P[f"discriminator/d_fc{i + 1}/bias"]
        if i < n - 1:
            h = torch.relu(h)
    return h


def g_step(P, z, grad_plugin, lr):
    """g_optim (GAN.py:83-101): tf.gradients(generates, g_vars, grad_plugin) through a training-mode forward (which moves the moving
    averages), then w -= lr * g on the g_fc kernels and biases.  -> {name: gradient}."""
    n = nlayers_of(P, "generator/g_fc")
    names = [f"generator/g_fc{i + 1}/{v}" for i in range(n) for v in ("kernel", "bias")]
    leaves = {k: P[k].detach().clone().requires_grad_(True) for k in names}
    Q = dict(P, **leaves)
    x = g_forward(Q, z)
    grads = dict(zip(names, torch.autograd.grad(x, [leaves[k] for k in names], grad_plugin)))
    with torch.no_grad():
        for k in names:
            P[k] -= lr * grads[k]
    return grads


def d_step(P, real, fake, lr):
    """d_optim (GAN.py:69-74,98-99): mean BCE(D(real), 1) + mean BCE(D(fake), 0), GradientDescentOptimizer(lr) on every d_fc variable."""
    n = nlayers_of(P, "discriminator/d_fc")
    names = [f"discriminator/d_fc{i + 1}/{v}" for i in range(n) for v in ("kernel", "bias")]
    leaves = {k: P[k].detach().clone().requires_grad_(True) for k in names}
    Q = dict(P, **leaves)
    loss = torch.nn.functional.softplus(-d_logits(Q, real)).mean() + torch.nn.functional.softplus(d_logits(Q, fake)).mean()
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    with torch.no_grad():
        for k, g in zip(names, grads):
            P[k] -= lr * g


def train_iteration(P, data, noise, B, dtype, lrd=1e-2, lrg=5e-3):
    """synthetic/main.py:352-380, mode train, d_steps = g_steps = 1, on the {G, D} tensors of P (updated in place)."""
    real = torch.as_tensor(data.next_batch(B), dtype=dtype)
    z = torch.as_tensor(noise.next_batch(B), dtype=dtype)
    with torch.no_grad():
        fake = g_forward(P, z)
    d_step(P, real, fake, lrd)
    z = torch.as_tensor(noise.next_batch(B), dtype=dtype)
    with torch.no_grad():
        x = g_forward(P, z)
    x.requires_grad_(True)
    grad_default = torch.autograd.grad(torch.nn.functional.softplus(-d_logits(P, x)).mean(), x)[0]      # GAN.py:77-78,87
    g_step(P, z, grad_default, lrg)


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_typed():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        nargs = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
    l = lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    # the workspace: (pre-activations [+ their gradients]) per BN layer, plus the fixed partial / statistics rows
    ws = lambda B, nl, bwd: int(l.cgs_mlp2d_gen_ws_bytes(B, nl, bwd))
    assert ws(1000, 6, 1) - ws(1000, 6, 0) == 5 * 1000 * 64 * 4
    assert ws(2000, 6, 0) - ws(1000, 6, 0) == 5 * 1000 * 64 * 4
    assert ws(1000, 7, 0) == 0 and ws(0, 6, 0) == 0


def test_generator_limits_are_the_d_kernels_limits():
    """The 25-Gaussians G (nhidden = 256) and more than 6 layers are refused with CGS_EINVAL before anything is launched."""
    from cgs_amd import lib
    l = lib.load()
    for nl, nh in ((6, 256), (7, 64), (1, 64)):
        rc = l.cgs_mlp2d_gen_fwd(None, None, None, None, None, None, nl, nh, None, None, 1000, 1, 1e-5, None, None, 0, None)
        assert rc == lib.EINVAL and b"nlayers" in l.cgs_last_error()
        rc = l.cgs_mlp2d_g_step(None, None, None, None, None, None, nl, nh, None, None, 1000, 1e-5, 5e-3, None, None, None, None, 0, None)
        assert rc == lib.EINVAL


@pytest.mark.parametrize("nhidden,nlayers", [(64, 6), (16, 3)])
def test_generator_variable_names_and_shapes(nhidden, nlayers):
    from cgs_amd.synthetic import MLPDiscriminator, MLPGenerator
    want = {n: s for n, s, _ in gan_py_variables(nhidden, nlayers)}
    G = MLPGenerator.init_params(0, nhidden, nlayers)
    D = MLPDiscriminator.init_params(0, nhidden, nlayers)
    assert {k: v.shape for k, v in G.items()} == {k: s for k, s in want.items() if k.startswith("generator/")}
    assert {k: v.shape for k, v in D.items()} == {k: s for k, s in want.items() if k.startswith("discriminator/")}
    assert all(v.dtype == np.float32 for v in list(G.values()) + list(D.values()))


def test_seeded_init_is_reproducible_and_tf_default():
    from cgs_amd.synthetic import MLPDiscriminator, MLPGenerator
    for cls in (MLPGenerator, MLPDiscriminator):
        a, b, c = cls.init_params(7), cls.init_params(7), cls.init_params(8)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert any(not np.array_equal(a[k], c[k]) for k in a if k.endswith("kernel"))
        for k, v in a.items():
            if k.endswith("/kernel"):                                     # glorot-uniform: U(-l, l), l = sqrt(6 / (fan_in + fan_out))
                lim = np.sqrt(6.0 / sum(v.shape))
                assert np.abs(v).max() <= lim and np.abs(v).max() > 0.8 * lim and abs(v.mean()) < 0.2 * lim
            elif k.endswith("/bias") or k.endswith("/beta") or k.endswith("/moving_mean"):
                assert not v.any()
            else:                                                         # gamma, moving_variance
                assert (v == 1).all()


def test_checkpoint_round_trip_of_g_and_d(tmp_path):
    """{G, D} through checkpoint.save / load in both formats, and a TF variable dump (':0' suffixes) through clean_tf_names: no G
    variable is mistaken for an optimizer slot (BatchNorm/beta is not beta1_power)."""
    from cgs_amd import checkpoint as CK
    from cgs_amd.synthetic import MLPDiscriminator, MLPGenerator
    P = {**MLPGenerator.init_params(3, 16, 3), **MLPDiscriminator.init_params(4, 16, 3)}
    rs = np.random.RandomState(0)
    P = {k: (v + rs.randn(*v.shape)).astype(np.float32) for k, v in P.items()}
    for ext in (".safetensors", ".npz"):
        CK.save(str(tmp_path / ("gd" + ext)), P)
        Q = CK.load(str(tmp_path / ("gd" + ext)))
        assert Q.keys() == P.keys() and all(np.array_equal(Q[k], P[k]) for k in P)
    tf_dump = {k + ":0": v for k, v in P.items()}
    tf_dump["beta1_power:0"] = np.float32(0.9)                           # an optimizer slot, dropped
    assert CK.clean_tf_names(tf_dump).keys() == P.keys()


def test_g_vars_filter_matches_gan_py():
    """GAN.py:83-84 filters TRAINABLE variables by the substring 'g_': the g_fc kernels and biases.  gamma / beta are trainable but
    named BatchNorm*/gamma|beta, so G's BN affine stays at its initial value for ever; the moving statistics do contain 'g_'
    ('movin[g_]mean') but are not trainable.  d_vars ('d_') is D's dense variables only."""
    for nh, nl in ((64, 6), (16, 3)):
        allv = gan_py_variables(nh, nl)
        assert g_vars(nh, nl) == [f"generator/g_fc{i + 1}/{v}" for i in range(nl) for v in ("kernel", "bias")]
        assert [n for n, _, t in allv if "g_" in n and not t] == [f"{bn_name(k)}/{v}" for k in range(nl - 1) for v in ("moving_mean", "moving_variance")]
        assert [n for n, _, t in allv if t and "d_" in n] == [f"discriminator/d_fc{i + 1}/{v}" for i in range(nl) for v in ("kernel", "bias")]
        assert not [n for n in g_vars(nh, nl) if "BatchNorm" in n]


def test_restatement_bn_backward_matches_finite_differences():
    """The float64 restatement's g_step gradient (autograd through the batch norm) against central differences on a tiny G."""
    from cgs_amd.synthetic import MLPGenerator
    P = to_torch(MLPGenerator.init_params(1, 4, 3), torch.float64)
    rs = np.random.RandomState(2)
    z = torch.as_tensor(rs.randn(6, 2))
    gp = torch.as_tensor(rs.randn(6, 2))
    grads = g_step(dict(P), z, gp, 0.0)
    k = "generator/g_fc2/kernel"
    for idx in ((0, 1), (3, 2)):
        Pp, Pm = {n: t.clone() for n, t in P.items()}, {n: t.clone() for n, t in P.items()}
        Pp[k][idx] += 1e-6
        Pm[k][idx] -= 1e-6
        fd = ((g_forward(Pp, z, update=False) - g_forward(Pm, z, update=False)) * gp).sum() / 2e-6
        assert abs(fd.item() - grads[k][idx].item()) < 1e-6 * max(1.0, abs(fd.item()))
