"""The image GAN's generator step without a device: the two new entry points of the C ABI, the split plan of the transposed
convolution's weight gradient, and a hand-written restatement of one G step (nsgan/GAN.py:132-146, 211-223) held to torch.autograd on the
operator oracle.  The restatement (``GanRef``) is also what tests/test_gpu_training.py carries beside the device, in float64 and in float32."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import nets_ref as N
from oracle import ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cgs_deconv_wgrad_ws_bytes", "cgs_deconv2d_nhwc_bwd_weight")


# ----------------------------------------------------------------------------- the restatement
def conv_filter_grad(inp, dout, kh, kw, s):
    """Filter gradient [kh,kw,Ci,Co] of the 'SAME' stride-s conv inp[B,H,W,Ci] -> dout[B,ceil(H/s),ceil(W/s),Co], by patches."""
    pt, pb = R.same_pads(inp.shape[1], kh, s)
    pl, pr = R.same_pads(inp.shape[2], kw, s)
    cols = F.unfold(F.pad(inp.permute(0, 3, 1, 2), (pl, pr, pt, pb)), (kh, kw), stride=s)        # [B, Ci*kh*kw, L]
    B, Ho, Wo, Co = dout.shape
    assert cols.shape[2] == Ho * Wo, (cols.shape, dout.shape)
    dw = torch.einsum("bkl,blo->ko", cols, dout.reshape(B, Ho * Wo, Co))
    return dw.reshape(inp.shape[3], kh, kw, Co).permute(1, 2, 0, 3).contiguous()


def deconv_filter_grad(x, dy, kh, kw, s):
    """dw[kh,kw,Cout,Cin] of deconv2d(x[B,Hin,Win,Cin]) contracted with dy[B,Hout,Wout,Cout]: the filter is that of the conv dy -> x."""
    return conv_filter_grad(dy, x, kh, kw, s)


def forward_layers(layers, x, P, scope, tape, sides=None, stats=None):
    """The oracle's operators layer by layer in training mode, keeping what the hand-written backward needs.  ``sides``: one bool tensor
    per relu / lrelu, in layer order, telling it the side to take (the branch a device forward evaluated); None = its own decision."""
    for L in layers:
        kind, s = L[0], (L[4] if len(L) >= 5 else 2)
        if kind == "linear":
            tape.append(("linear", f"{scope}/{L[1]}", x))
            x = x @ P[f"{scope}/{L[1]}/Matrix"] + P[f"{scope}/{L[1]}/bias"]
        elif kind in ("reshape", "flatten"):
            tape.append(("view", x.shape))
            x = x.reshape((x.shape[0],) + tuple(L[1])) if kind == "reshape" else x.reshape(x.shape[0], -1)
        elif kind == "conv":
            tape.append(("conv", f"{scope}/{L[1]}", x, s))
            x = R.conv2d(x, P[f"{scope}/{L[1]}/w"], P[f"{scope}/{L[1]}/biases"], s, s)
        elif kind == "deconv":
            tape.append(("deconv", f"{scope}/{L[1]}", x, s))
            x = R.deconv2d(x, P[f"{scope}/{L[1]}/w"], P[f"{scope}/{L[1]}/biases"], (x.shape[0],) + tuple(L[2]), s, s)
        elif kind == "bn":
            red = tuple(range(x.dim() - 1))
            mean = x.mean(dim=red)
            var = ((x - mean) ** 2).mean(dim=red)
            rstd = 1.0 / torch.sqrt(var + R.BN_EPS)
            xhat = (x - mean) * rstd
            if stats is not None:
                stats[f"{scope}/{L[1]}"] = (mean, var)
            tape.append(("bn", f"{scope}/{L[1]}", xhat, rstd))
            x = P[f"{scope}/{L[1]}/gamma"] * xhat + P[f"{scope}/{L[1]}/beta"]
        elif kind in ("relu", "lrelu"):
            leak = 0.0 if kind == "relu" else R.LRELU_LEAK
            m = sides.pop(0) if sides is not None else x > 0
            tape.append(("act", m, leak))
            x = torch.where(m, x, leak * x)
        elif kind == "tanh":
            x = torch.tanh(x)
            tape.append(("tanh", x))
        else:
            raise KeyError(kind)
    return x


def backward_layers(tape, dy, P, grads):
    """The adjoint of ``forward_layers`` written out; leaves every parameter gradient in ``grads``; returns the input gradient."""
    for rec in reversed(tape):
        kind = rec[0]
        if kind == "linear":
            _, name, x = rec
            grads[name + "/Matrix"], grads[name + "/bias"] = x.t() @ dy, dy.sum(0)
            dy = dy @ P[name + "/Matrix"].t()
        elif kind == "view":
            dy = dy.reshape(rec[1])
        elif kind == "conv":
            _, name, x, s = rec
            w = P[name + "/w"]
            grads[name + "/w"], grads[name + "/biases"] = conv_filter_grad(x, dy, w.shape[0], w.shape[1], s), dy.sum((0, 1, 2))
            dy = R.deconv2d(dy, w, torch.zeros(w.shape[2], dtype=dy.dtype), x.shape, s, s)
        elif kind == "deconv":
            _, name, x, s = rec
            w = P[name + "/w"]
            grads[name + "/w"], grads[name + "/biases"] = deconv_filter_grad(x, dy, w.shape[0], w.shape[1], s), dy.sum((0, 1, 2))
            dy = R.conv2d(dy, w, torch.zeros(w.shape[3], dtype=dy.dtype), s, s)
        elif kind == "bn":
            _, name, xhat, rstd = rec
            red = tuple(range(dy.dim() - 1))
            grads[name + "/beta"], grads[name + "/gamma"] = dy.sum(red), (dy * xhat).sum(red)
            dxh = dy * P[name + "/gamma"]
            dy = rstd * (dxh - dxh.mean(dim=red) - xhat * (dxh * xhat).mean(dim=red))
        elif kind == "act":
            dy = torch.where(rec[1], dy, rec[2] * dy)
        elif kind == "tanh":
            dy = dy * (1.0 - rec[1] * rec[1])
    return dy


def is_var(name, scope):
    return name.startswith(scope + "/") and "moving" not in name


class GanRef:
    """nsgan/GAN.py:219-223 in one dtype on the CPU: Adam as tf.train.AdamOptimizer, G's moving averages as ops.bn moves them (decay 0.9,
    the biased batch variance), D at ``lr`` and G at ``5 lr``."""

    def __init__(self, arch, P, dtype, lr=2e-4, b1=0.5, b2=0.999, eps=1e-8):
        self.arch, self.A, self.dtype = arch, N.ARCHS[arch], dtype
        self.P = {k: v.detach().clone().to(dtype) for k, v in P.items()}
        self.lr, self.b1, self.b2, self.eps = lr, b1, b2, eps
        self.t = {"generator": 0, "discriminator": 0}
        self.m = {k: torch.zeros_like(v) for k, v in self.P.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.P.items()}

    def g_forward(self, z, tape=None, sides=None):
        """generator(z, is_training=True); the moving averages move once."""
        stats = {}
        x = forward_layers(self.A["g_head"] + self.A["g_tail"], z.to(self.dtype), self.P, "generator", [] if tape is None else tape, sides, stats)
        for name, (mean, var) in stats.items():
            self.P[name + "/moving_mean"] = 0.9 * self.P[name + "/moving_mean"] + 0.1 * mean
            self.P[name + "/moving_variance"] = 0.9 * self.P[name + "/moving_variance"] + 0.1 * var
        return x

    def g_loss_and_grads(self, z, g_sides=None, d_sides=None):
        """g_loss = mean BCE(D(G(z)), 1) and the gradient of every g_ variable, by the hand-written backward."""
        gt, dt, grads = [], [], {}
        x = self.g_forward(z, gt, g_sides)
        logits = forward_layers(self.A["d"], x, self.P, "discriminator", dt, d_sides)
        loss = F.softplus(-logits).mean()
        dl = (torch.sigmoid(logits) - 1.0) / logits.numel()
        backward_layers(gt, backward_layers(dt, dl, self.P, {}), self.P, grads)
        return loss, grads

    def adam(self, scope, grads, lr):
        self.t[scope] += 1
        t = self.t[scope]
        lr_t = lr * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
        for k, g in grads.items():
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * g * g
            self.P[k] = self.P[k] - lr_t * self.m[k] / (torch.sqrt(self.v[k]) + self.eps)

    def g_step(self, z):
        loss, grads = self.g_loss_and_grads(z)
        self.adam("generator", grads, 5 * self.lr)
        return loss

    def d_step(self, real, fake):
        """d_optim on d_loss = mean BCE(D(real), 1) + mean BCE(D(fake), 0), D in training mode (autograd on the oracle's D)."""
        names = [k for k in self.P if is_var(k, "discriminator")]
        Pd = dict(self.P)
        for k in names:
            Pd[k] = self.P[k].clone().requires_grad_(True)
        lr_, lf_ = N.discriminator(self.arch, Pd, real.to(self.dtype)), N.discriminator(self.arch, Pd, fake.detach())
        loss = F.softplus(-lr_).mean() + F.softplus(lf_).mean()
        gs = torch.autograd.grad(loss, [Pd[k] for k in names])
        self.adam("discriminator", dict(zip(names, gs)), self.lr)
        return loss.detach()

    def iteration(self, real, z):
        fake = self.g_forward(z)
        d_loss = self.d_step(real, fake)
        return d_loss, self.g_step(z)


# ----------------------------------------------------------------------------- tests
def test_header_bindings_and_library_agree_on_the_new_entry_points():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    declared = set(re.findall(r"\b(cgs_[a-z0-9_]+)\s*\(", header))
    l = lib.load()
    for name in NEW:
        assert name in declared and name in lib.SIGNATURES
        assert getattr(l, name) is not None
    import ctypes
    assert lib.SIGNATURES[NEW[0]] == (ctypes.c_size_t, [ctypes.c_int] * 11)
    assert len(lib.SIGNATURES[NEW[1]][1]) == 18
    assert l.cgs_version() >= 107


# (B, Hin, Win, Cin, Hout, Wout, Cout, kh, kw, sh, sw): the G layers of the shipped nets at batch 64, odd / non-square / stride-1 outputs, and
# both sides of the slab cap at Cin = Cout = 8 (32 641 = 255 * 128 + 1 pixels is the first count that asks for 256 slabs of >= 4 steps)
PLAN_SHAPES = [(64, 7, 7, 128, 14, 14, 64, 4, 4, 2, 2), (64, 14, 14, 64, 28, 28, 1, 4, 4, 2, 2), (64, 4, 4, 512, 8, 8, 256, 5, 5, 2, 2),
               (64, 32, 32, 64, 64, 64, 3, 5, 5, 2, 2), (2, 3, 3, 5, 5, 5, 3, 5, 5, 2, 2), (2, 3, 5, 4, 6, 10, 7, 3, 5, 2, 2),
               (1, 4, 4, 6, 4, 4, 7, 3, 3, 1, 1), (1, 3, 3, 5, 6, 6, 3, 4, 4, 2, 2), (3, 7, 7, 128, 14, 14, 64, 4, 4, 2, 2),
               (7, 1, 4663, 8, 2, 9326, 8, 4, 4, 2, 2), (1, 1, 32640, 8, 2, 65280, 8, 4, 4, 2, 2), (2, 2, 2, 130, 4, 4, 127, 5, 5, 2, 2)]


def test_deconv_wgrad_workspace_is_the_conv_plan_with_the_roles_swapped():
    from cgs_amd import lib
    from wgrad_plan import SPLIT_CAP, ceil_div, wgrad_plan
    l = lib.load()
    for (B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, sh, sw) in PLAN_SHAPES:
        p = wgrad_plan(B, Ho, Wo, Co, Ci, kh, kw, sh, sw)             # big = dy (Hout, Wout, Cout), small = x (Hin, Win, Cin)
        assert (p.Ho, p.Wo) == (Hi, Wi) and p.M == B * Hi * Wi and p.Kc == kh * kw * Co
        got = int(l.cgs_deconv_wgrad_ws_bytes(B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, sh, sw))
        assert got == p.splits * p.Kc * p.Csp * 4, ((B, Hi, Wi, Ci, Ho, Wo, Co), got, p)
        assert got == int(l.cgs_conv_wgrad_ws_bytes(B, Ho, Wo, Co, Ci, kh, kw, sh, sw))
        assert 1 <= p.splits <= SPLIT_CAP and p.splits * p.m_per_split >= p.M > (p.splits - 1) * p.m_per_split
    assert wgrad_plan(7, 2, 9326, 8, 8, 4, 4, 2, 2).splits == SPLIT_CAP and wgrad_plan(1, 2, 65280, 8, 8, 4, 4, 2, 2).splits == SPLIT_CAP - 1
    assert wgrad_plan(1, 6, 6, 3, 5, 4, 4, 2, 2).splits == 1 and wgrad_plan(3, 14, 14, 64, 128, 4, 4, 2, 2).m_per_split * 2 > 147   # one slab; a short last one
    # not a 'SAME' pre-image, or a non-positive argument: no plan
    assert int(l.cgs_deconv_wgrad_ws_bytes(2, 3, 3, 5, 7, 6, 3, 4, 4, 2, 2)) == 0
    assert int(l.cgs_deconv_wgrad_ws_bytes(2, 3, 3, 5, 6, 4, 3, 4, 4, 2, 2)) == 0
    assert int(l.cgs_deconv_wgrad_ws_bytes(0, 3, 3, 5, 6, 6, 3, 4, 4, 2, 2)) == 0
    assert int(l.cgs_deconv_wgrad_ws_bytes(2, 3, 3, 5, 6, 6, 3, 4, 4, 2, 0)) == 0
    assert ceil_div(7, 2) == 4


def test_filter_gradient_by_patches_matches_autograd():
    g = torch.Generator().manual_seed(0)
    for (B, Hi, Wi, Ci, Ho, Wo, Co, k, s) in [(2, 3, 3, 5, 6, 6, 3, 4, 2), (2, 3, 3, 5, 5, 5, 3, 5, 2), (1, 4, 4, 6, 4, 4, 7, 3, 1), (2, 3, 5, 4, 6, 10, 7, 5, 2)]:
        x = torch.randn((B, Hi, Wi, Ci), generator=g, dtype=torch.float64)
        w = torch.randn((k, k, Co, Ci), generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn((B, Ho, Wo, Co), generator=g, dtype=torch.float64)
        (R.deconv2d(x, w, torch.zeros(Co, dtype=torch.float64), (B, Ho, Wo, Co), s, s) * dy).sum().backward()
        got = deconv_filter_grad(x, dy, k, k, s)
        assert (got - w.grad).abs().max().item() <= 1e-12 * w.grad.abs().max().item()


def test_restated_g_step_matches_autograd_on_the_oracle():
    arch, B = "mnist", 4
    P = N.init_params(arch, 2019, True)
    g = torch.Generator().manual_seed(7)
    z = (torch.rand((B, 62), generator=g) * 2 - 1).double()
    ref = GanRef(arch, P, torch.float64)
    before = {k: v.clone() for k, v in ref.P.items()}
    loss, grads = ref.g_loss_and_grads(z)
    # torch.autograd through oracle/ops_ref.py's operators, both nets in training mode
    Pa = {k: (v.clone().requires_grad_(True) if is_var(k, "generator") else v.clone()) for k, v in before.items()}
    x = N.run_layers(N.ARCHS[arch]["g_head"] + N.ARCHS[arch]["g_tail"], z, Pa, "generator", bn_training=True)
    logits = N.discriminator(arch, Pa, x)
    want = F.binary_cross_entropy_with_logits(logits, torch.ones_like(logits))
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-10 * abs(want.item())
    names = [k for k in Pa if Pa[k].requires_grad]
    assert sorted(names) == sorted(grads) and len(names) == 14          # Matrix / bias x 2, w / biases x 2, gamma / beta x 3
    for k in names:
        ref_g = Pa[k].grad
        assert (grads[k] - ref_g).abs().max().item() <= 1e-10 * max(ref_g.abs().max().item(), 1e-300) or ref_g.abs().max().item() < 1e-12, k
    # a bias in front of a batch norm has no gradient in exact arithmetic
    assert grads["generator/g_fc1/bias"].abs().max().item() < 1e-12
    # one training-mode forward moved every moving average once, D's variables and moving averages not at all
    for k in before:
        if k.startswith("discriminator/"):
            assert torch.equal(ref.P[k], before[k]), k
    stats = {}
    forward_layers(N.ARCHS[arch]["g_head"] + N.ARCHS[arch]["g_tail"], z, before, "generator", [], None, stats)
    for name, (mean, var) in stats.items():
        assert torch.allclose(ref.P[name + "/moving_mean"], 0.9 * before[name + "/moving_mean"] + 0.1 * mean, rtol=0, atol=1e-15)
        assert torch.allclose(ref.P[name + "/moving_variance"], 0.9 * before[name + "/moving_variance"] + 0.1 * var, rtol=0, atol=1e-15)
    # the Adam step at 5 lr: the first step moves every entry by lr_t * g / (|g| sqrt(1 - b2) + eps)
    ref.adam("generator", grads, 5 * ref.lr)
    lr_t = 5 * 2e-4 * math.sqrt(1 - 0.999) / (1 - 0.5)
    k = "generator/g_dc4/w"
    want_w = before[k] - lr_t * 0.5 * grads[k] / (torch.sqrt(0.001 * grads[k] ** 2) + 1e-8)
    assert (ref.P[k] - want_w).abs().max().item() < 1e-15 and ref.t["generator"] == 1


@pytest.mark.parametrize("arch", ["mnist", "dcgan32", "dcgan64"])
def test_training_mode_generator_tape_folds_relu_into_the_norm_stage(arch):
    """bn + relu in training mode is one norm stage at leak 0 (stage construction only allocates: no device needed)."""
    from cgs_amd import engine as E, training
    from cgs_amd.nets import ARCHS, g_input_shape
    assert training.BN_DECAY == 0.9
    A = ARCHS[arch]
    P = N.init_params(arch, 2019, True)
    tape = E.Tape(A["g_head"] + A["g_tail"], g_input_shape(A), P, "generator", 2, A["k"], A["stride"], True, torch.device("cpu"))
    kinds = [type(st).__name__ for st in tape.stages]
    assert "_Unary" not in kinds and "_AffineRelu" not in kinds
    norms = [st for st in tape.stages if isinstance(st, E._BnTrainLrelu)]
    assert len(norms) == sum(1 for L in A["g_head"] + A["g_tail"] if L[0] == "bn") and all(st.leak == 0.0 for st in norms)
    assert tape.stages[-1].epi == 3 and tuple(tape.out_shape) == tuple(A["img"])          # deconv + tanh
