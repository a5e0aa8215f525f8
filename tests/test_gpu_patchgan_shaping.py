"""The discriminator shaping step on the PatchGAN of BASELINE config 5 (``shaping.DShaper`` over instance norms and a logit MAP; the
instance-norm parameter gradients and the one-output-channel weight gradient of csrc/wgrad_dot.hip inside it), against float64 autograd
of the branch the device evaluated, as test_gpu_shaping.py does for the reference's nets; ``shape_step`` on an image-to-image net and
``calibrate_step``."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N
from oracle import ops_ref as R

T64 = "cyclegan_t64"        # the tiny topology at 64 pixels: d_in2 normalises 16 x 16 = 256 pixels per sample, the three-launch norm path
N_D_VARS = 16               # 5 convs x (w, biases) + 3 instance norms x (scale, offset)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def close(got, want, tol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs().max().item()
    ref = want.abs().max().item() + 1e-30
    print(f"{what}: max|delta|={err:.3e} max|ref|={ref:.3e} ratio={err / ref:.3e} bar={tol:.1e}")
    assert err <= tol * ref, f"{what}: max|delta|={err:.3e} vs max|ref|={ref:.3e}"


@pytest.fixture
def archs(monkeypatch):
    from cgs_amd import nets
    monkeypatch.setitem(nets.ARCHS, T64, nets.cyclegan(64, 2, ngf=16, ndf=16))
    monkeypatch.setitem(N.ARCHS, T64, N._cyclegan(64, 2, ngf=16, ndf=16))


def _oracle_d_with_lrelu_sides(arch, P, x, sides):
    """The oracle D in float64 with every LeakyReLU taking the side it is told (test_gpu_shaping.py: the gradient of the piecewise-linear
    branch the GPU's forward evaluated)."""
    sides = list(sides)
    for L in N.ARCHS[arch]["d"]:
        if L[0] == "lrelu":
            x = torch.where(sides.pop(0), x, R.LRELU_LEAK * x)
        else:
            x = N.run_layers([L], x, P, "discriminator", bn_training=True)
    assert not sides
    return x


def _slots_by_name(sh, Pd, names):
    out = {}
    for st in sh.tape.stages:
        for attr in ("w", "b", "scale", "offset"):
            if hasattr(st, "g_" + attr):
                out[[k for k in names if Pd[k] is getattr(st, attr)][0]] = getattr(st, "g_" + attr)
    return out


@pytest.mark.parametrize("arch,B", [("cyclegan_tiny", 4), (T64, 2)])
def test_patchgan_d_step_matches_autograd(archs, arch, B):
    from cgs_amd import lib as L
    from cgs_amd.engine import _Conv, _InstNormAct
    from cgs_amd.nets import to_device
    from cgs_amd.shaping import DShaper
    P = N.init_params(arch, 2019, True)
    img = tuple(N.ARCHS[arch]["img"])
    real = rnd((B,) + img, 1).clamp(-1, 1)
    fake = torch.tanh(rnd((B,) + img, 2))
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    d = dev()
    Pd = to_device(P, d)
    sh = DShaper(arch, Pd, B, d, learning_rate=1e-3)
    if arch == T64:
        assert isinstance(sh.tape.stages[2], _InstNormAct) and tuple(sh.tape.stages[2].out.shape[1:3]) == (16, 16)      # d_in2: HW = 256 > 128 rows
    head = sh.tape.stages[-1]
    assert isinstance(head, _Conv) and head.w.shape[3] == 1 and head.wgrad_cout1        # the logit head: the dot-product weight gradient

    def lrelu_sides(x):
        sh.tape.forward(x.to(d))
        return [(st.out > 0).cpu() for st in sh.tape.stages
                if (isinstance(st, _Conv) and st.epi == L.EPI_LRELU) or (isinstance(st, _InstNormAct) and st.leak != 1.0)]
    sides_r, sides_f = lrelu_sides(real), lrelu_sides(fake)
    assert len(sides_r) == 4
    Pg = {k: (v.clone().double().requires_grad_(True) if k.startswith("discriminator/") else v.double()) for k, v in P.items()}
    lr = _oracle_d_with_lrelu_sides(arch, Pg, real.double(), sides_r)
    lf = _oracle_d_with_lrelu_sides(arch, Pg, fake.double(), sides_f)
    assert lr.shape[1] > 1 and lr.shape[3] == 1                          # a logit MAP: the mean runs over every patch
    loss = bce(lr, torch.ones_like(lr)) + bce(lf, torch.zeros_like(lf))
    loss.backward()
    got_loss = sh.loss_and_grads(real.to(d), fake.to(d))
    print(f"d_loss {got_loss.item():.8f} vs float64 {loss.item():.8f}")
    assert abs(got_loss.item() - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    names = [k for k in Pg if Pg[k].requires_grad]
    grads = _slots_by_name(sh, Pd, names)
    assert len(names) == N_D_VARS and sorted(grads) == sorted(names) and len(sh.slots) == N_D_VARS
    for k in names:
        g_ref, got = Pg[k].grad, grads[k].cpu().double()
        if k.endswith("/biases") and k.split("/")[1] in ("d_c2", "d_c3", "d_c4"):
            # a bias in front of an instance norm: zero in exact arithmetic; bounded absolutely, as the bias in front of a batch norm is
            assert float(g_ref.abs().max()) < 1e-6 and float(got.abs().max()) < 1e-4, k
        else:
            close(got, g_ref, 2e-5, k)
    # one Adam step (tf.train.AdamOptimizer formula) from the step's OWN gradients, at test_gpu_shaping.py's tolerance
    before = {k: Pd[k].clone() for k in names}
    own = {k: g.clone() for k, g in grads.items()}
    sh.step(real.to(d), fake.to(d))
    lr_t = 1e-3 * math.sqrt(1 - 0.999) / (1 - 0.5)
    for k in names:
        g = own[k].cpu()
        want = before[k].cpu() - lr_t * (0.5 * g) / (torch.sqrt(0.001 * g * g) + 1e-8)
        assert (Pd[k].cpu() - want).abs().max().item() <= 1e-6 + 2e-3 * lr_t * 16, k
        assert not torch.equal(Pd[k], before[k]), k


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_shape_step_on_an_image_to_image_net(use_graph):
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device
    from cgs_amd.shaping import DShaper, shape_step
    arch, B, Ksteps = "cyclegan_tiny", 4, 3
    d = dev()
    Pd = to_device(N.init_params(arch, 2019, True), d)
    eng = RefineEngine(arch, Pd, B, d, use_graph=use_graph)
    sh = DShaper(arch, Pd, B, d, learning_rate=1e-3)
    src = (torch.rand((B, 32, 32, 3), generator=torch.Generator().manual_seed(5)) * 2 - 1).to(d)     # the image G translates
    real = rnd((B, 32, 32, 3), 1).clamp(-1, 1).to(d)
    idx = np.array([0, 3, 1, 2])
    kw = dict(mode="probabilistic", indices=idx)
    first = [t.clone() for t in eng.refine_from_z(src, Ksteps, 0.1, **kw)]
    before = {k: v.clone() for k, v in Pd.items()}
    loss = shape_step(eng, sh, src, real, Ksteps, 0.1, indices=idx)
    assert math.isfinite(float(loss))
    for k, v in Pd.items():
        if k.startswith("discriminator/"):
            assert not torch.equal(v, before[k]), k
        else:
            assert torch.equal(v, before[k]), k
    after = [t.clone() for t in eng.refine_from_z(src, Ksteps, 0.1, **kw)]
    fresh = [t.clone() for t in RefineEngine(arch, Pd, B, d, use_graph=use_graph).refine_from_z(src, Ksteps, 0.1, **kw)]
    assert not torch.equal(after[2], first[2])                              # the refiner sees the shaped D
    for a, b in zip(after, fresh):
        assert torch.equal(a, b)


def test_calibrate_step_is_the_hand_composition():
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device
    from cgs_amd.shaping import DShaper, calibrate_step
    arch, B = "mnist", 8
    d = dev()
    P = N.init_params(arch, 2019, True)
    z = rnd((B, 62), 2).clamp(-1, 1).to(d)
    real = rnd((B, 28, 28, 1), 1).clamp(-1, 1).to(d)
    probe = torch.tanh(rnd((B, 28, 28, 1), 3)).to(d)
    Pa, Pb = to_device(P, d), to_device(P, d)
    ea, sa = RefineEngine(arch, Pa, B, d), DShaper(arch, Pa, B, d, learning_rate=2e-3)
    s0 = ea.score(probe).clone()
    la = calibrate_step(ea, sa, z, real)
    eb, sb = RefineEngine(arch, Pb, B, d), DShaper(arch, Pb, B, d, learning_rate=2e-3)
    fake = eb.generate(z)                                                    # nsgan/GAN.py:274
    lb = sb.step(real, fake)                                                 # :275
    eb.refresh_weights()
    assert torch.equal(la, lb) and math.isfinite(float(la))
    for k in Pa:
        assert torch.equal(Pa[k], Pb[k]), k
    s1 = ea.score(probe).clone()
    assert s1.shape == s0.shape and not torch.equal(s0, s1)
    assert torch.equal(s1, eb.score(probe))
