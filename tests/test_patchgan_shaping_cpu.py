"""The D step of the PatchGAN discriminator (BASELINE config 5), host side: the three C ABI entries of csrc/wgrad_dot.hip, the slab plan
of the one-output-channel weight gradient restated in Python, its refusals, and a float64 restatement of the whole step (hand-written
backward through the operators of oracle/ops_ref.py) checked against torch.autograd.  The GPU tests import the restatements."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import nets_ref as N
from oracle import ops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cgs_instnorm_param_grads", "cgs_conv_wgrad_cout1_ws_bytes", "cgs_conv2d_nhwc_bwd_weight_cout1")

# ---- the slab plan of cgs_conv2d_nhwc_bwd_weight_cout1 (csrc/wgrad_dot.hip, co1_plan) ----
CO1_THREADS, CO1_UNROLL, CO1_BLOCKS, CO1_MIN_PIX, CO1_MAX_SLABS = 256, 4, 1024, 32, 256


def ceil_div(a, b):
    return -(-a // b)


def co1_plan(B, H, W, Cin, kh, kw, sh, sw):
    """(slabs, pixels per slab, floats per partial dW) or None for a shape the entry refuses."""
    if min(B, H, W, Cin, kh, kw, sh, sw) <= 0 or Cin % 4 or kh * kw * Cin < 1024 or sh != sw:
        return None
    M = B * ceil_div(H, sh) * ceil_div(W, sw)
    K4 = kh * kw * Cin // 4
    colblocks = ceil_div(K4, CO1_THREADS)
    slabs = min(ceil_div(CO1_BLOCKS, colblocks), max(M // CO1_MIN_PIX, 1), CO1_MAX_SLABS)
    pps = ceil_div(ceil_div(M, slabs), CO1_UNROLL) * CO1_UNROLL
    return ceil_div(M, pps), pps, 4 * K4


# >= 3 slabs with a short last one, from the constants above: M = 2 * 9 * 9 = 162 pixels, K4 = 1024 -> 4 column blocks -> 256 slabs
# wanted, 162 // 32 = 5 allowed, 33 -> 36 pixels per slab: 5 slabs, the last one of 162 - 4 * 36 = 18 pixels
SHORT_LAST_SLAB = (2, 9, 9, 256, 4, 1)


def test_new_symbols_are_declared_typed_and_exported():
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
    assert l.cgs_version() >= 109


@pytest.mark.parametrize("shape,slabs", [
    ((1, 1, 1, 1024, 1, 1), 1),            # a single pixel: one slab
    ((4, 4, 4, 128, 4, 1), 2),             # the tiny net's d_c5: 64 pixels
    ((2, 6, 5, 256, 4, 1), 1),             # 60 pixels: one slab
    ((3, 9, 7, 64, 5, 2), 1),              # stride 2: 3 * 5 * 4 = 60 pixels
    ((2, 8, 8, 68, 4, 1), 4),              # Cin % 64 != 0: 272 float4 columns, two column blocks
    (SHORT_LAST_SLAB[:4] + (4, 4, 1, 1), 5),
    ((8, 32, 32, 512, 4, 4, 1, 1), 128),   # cyclegan256's d_c5 at batch 8: many slabs of 64 pixels
    ((64, 32, 32, 64, 4, 4, 1, 1), 256),   # the slab cap
])
def test_ws_query_equals_the_plan(shape, slabs):
    from cgs_amd import lib
    if len(shape) == 6:
        B, H, W, Cin, k, s = shape
        shape = (B, H, W, Cin, k, k, s, s)
    plan = co1_plan(*shape)
    assert plan is not None and plan[0] == slabs
    M = shape[0] * ceil_div(shape[1], shape[6]) * ceil_div(shape[2], shape[7])
    assert (plan[0] - 1) * plan[1] < M <= plan[0] * plan[1]                  # every slab holds a pixel, all pixels are covered
    assert int(lib.load().cgs_conv_wgrad_cout1_ws_bytes(*shape)) == plan[0] * plan[2] * 4


def test_short_last_slab_case_is_what_its_comment_says():
    B, H, W, Cin, k, s = SHORT_LAST_SLAB
    slabs, pps, _ = co1_plan(B, H, W, Cin, k, k, s, s)
    assert slabs >= 3 and 0 < B * H * W - (slabs - 1) * pps < pps


@pytest.mark.parametrize("shape", [
    (2, 8, 8, 6, 16, 16, 1, 1),            # Cin % 4 != 0 (K = 1536)
    (2, 8, 8, 130, 4, 4, 1, 1),            # Cin % 4 != 0
    (2, 8, 8, 32, 4, 4, 1, 1),             # K = 512 < 1024
    (2, 8, 8, 60, 4, 4, 1, 1),             # K = 960
    (2, 8, 8, 128, 4, 4, 1, 2),            # two strides
    (0, 8, 8, 128, 4, 4, 1, 1), (2, 0, 8, 128, 4, 4, 1, 1), (2, 8, -1, 128, 4, 4, 1, 1), (2, 8, 8, 0, 4, 4, 1, 1),
    (2, 8, 8, 128, 0, 4, 1, 1), (2, 8, 8, 128, 4, 0, 1, 1), (2, 8, 8, 128, 4, 4, 0, 0), (2, 8, 8, 128, 4, 4, -1, -1),
])
def test_ws_query_is_zero_and_the_entry_refuses(shape):
    from cgs_amd import lib
    l = lib.load()
    assert co1_plan(*shape) is None
    assert int(l.cgs_conv_wgrad_cout1_ws_bytes(*shape)) == 0
    # (refused on the shape, before anything is dereferenced or launched: the non-null pointers are never read)
    assert l.cgs_conv2d_nhwc_bwd_weight_cout1(16, 16, 16, *shape, 0, 16, 1 << 30, None) == lib.EINVAL


def test_instnorm_param_grads_refuses_bad_arguments():
    from cgs_amd import lib
    l = lib.load()
    for B, HW, C in [(0, 64, 16), (2, 0, 16), (2, 64, 0), (2, 64, 6), (70000, 64, 16)]:
        assert l.cgs_instnorm_param_grads(16, B, HW, C, 16, 16, 0, None) == lib.EINVAL
    assert l.cgs_instnorm_param_grads(None, 2, 64, 16, 16, 16, 0, None) == lib.EINVAL


# ---- float64 restatement of the PatchGAN D step ----
def conv_grads(x, w, dy, s):
    """(dx, dw, db) of R.conv2d(x, w, b, s, s) contracted with dy, written out: the weight gradient tap by tap over the 'SAME'-padded
    input, the data gradient as the transposed convolution R.deconv2d defines (the adjoint of that conv)."""
    kh, kw = w.shape[0], w.shape[1]
    pt, pb = R.same_pads(x.shape[1], kh, s)
    pl, pr = R.same_pads(x.shape[2], kw, s)
    xp = F.pad(x, (0, 0, pl, pr, pt, pb))
    Ho, Wo = dy.shape[1], dy.shape[2]
    dw = torch.zeros_like(w)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :]
            dw[ky, kx] = torch.einsum("bhwi,bhwo->io", win, dy)
    dx = R.deconv2d(dy, w, torch.zeros(w.shape[2], dtype=x.dtype), tuple(x.shape), s, s)
    return dx, dw, dy.sum(dim=(0, 1, 2))


def instnorm_grads(x, scale, dy):
    """(dx, dscale, doffset) of R.instance_norm(x, scale, offset) contracted with dy."""
    mean = x.mean(dim=(1, 2), keepdim=True)
    invstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=(1, 2), keepdim=True) + R.BN_EPS)
    xhat = (x - mean) * invstd
    m1, m2 = dy.mean(dim=(1, 2), keepdim=True), (dy * xhat).mean(dim=(1, 2), keepdim=True)
    return scale * invstd * (dy - m1 - xhat * m2), (dy * xhat).sum(dim=(0, 1, 2)), dy.sum(dim=(0, 1, 2))


def patchgan_d_pass(layers, P, x, target, sides=None):
    """One pass of D in float64 with its hand-written backward: (mean BCE(logits, target), {parameter name: gradient}).  ``sides``: one
    bool tensor per LeakyReLU in layer order -- the side each one takes (None: its own pre-activation decides)."""
    sides = list(sides) if sides is not None else None
    tape = []
    for Lr in layers:
        s_ = "discriminator/" + Lr[1] if len(Lr) > 1 else None
        if Lr[0] == "conv":
            st = Lr[4] if len(Lr) >= 5 else 2
            tape.append(("conv", s_, x, st))
            x = R.conv2d(x, P[s_ + "/w"], P[s_ + "/biases"], st, st)
        elif Lr[0] == "instnorm":
            tape.append(("instnorm", s_, x))
            x = R.instance_norm(x, P[s_ + "/scale"], P[s_ + "/offset"])
        elif Lr[0] == "lrelu":
            side = sides.pop(0) if sides is not None else x > 0
            tape.append(("lrelu", side))
            x = torch.where(side, x, R.LRELU_LEAK * x)
        else:
            raise KeyError(Lr[0])
    assert not sides
    n = x.numel()
    loss = (torch.clamp(x, min=0) - x * target + torch.log1p(torch.exp(-x.abs()))).sum() / n     # sigmoid_cross_entropy_with_logits, mean
    dy = (torch.sigmoid(x) - target) / n
    grads = {}
    for rec in reversed(tape):
        if rec[0] == "lrelu":
            dy = torch.where(rec[1], dy, R.LRELU_LEAK * dy)
        elif rec[0] == "instnorm":
            dy, grads[rec[1] + "/scale"], grads[rec[1] + "/offset"] = instnorm_grads(rec[2], P[rec[1] + "/scale"], dy)
        else:
            dy, grads[rec[1] + "/w"], grads[rec[1] + "/biases"] = conv_grads(rec[2], P[rec[1] + "/w"], dy, rec[3])
    return loss, grads


def patchgan_d_step(layers, P, real, fake, sides_real=None, sides_fake=None):
    """d_loss = mean BCE(D(real), 1) + mean BCE(D(fake), 0) (nsgan/GAN.py:126-131 on a logit map) and every D variable's gradient."""
    lr, gr = patchgan_d_pass(layers, P, real, 1.0, sides_real)
    lf, gf = patchgan_d_pass(layers, P, fake, 0.0, sides_fake)
    return lr + lf, {k: gr[k] + gf[k] for k in gr}


def test_f64_restatement_of_the_patchgan_d_step_matches_autograd():
    arch, B = "cyclegan_tiny", 2
    g = torch.Generator().manual_seed(7)
    P = {k: v.double() for k, v in N.init_params(arch, 2019, True).items()}
    real = (torch.rand((B,) + tuple(N.ARCHS[arch]["img"]), generator=g, dtype=torch.float64) * 2 - 1)
    fake = torch.tanh(torch.randn((B,) + tuple(N.ARCHS[arch]["img"]), generator=g, dtype=torch.float64))
    loss, grads = patchgan_d_step(N.ARCHS[arch]["d"], P, real, fake)
    Pg = {k: (v.clone().requires_grad_(True) if k.startswith("discriminator/") else v) for k, v in P.items()}
    bce = F.binary_cross_entropy_with_logits
    lr, lf = N.discriminator(arch, Pg, real), N.discriminator(arch, Pg, fake)
    want = bce(lr, torch.ones_like(lr)) + bce(lf, torch.zeros_like(lf))
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    names = [k for k in Pg if Pg[k].requires_grad]
    assert sorted(names) == sorted(grads) and len(names) == 16           # 5 convs x (w, biases) + 3 instance norms x (scale, offset)
    for k in names:
        ref = Pg[k].grad
        top = float(ref.abs().max())
        if k.endswith("/biases") and any(k.startswith(f"discriminator/d_c{i}/") for i in (2, 3, 4)):
            # a bias in front of an instance norm: zero in exact arithmetic, rounding noise in both evaluations
            assert float(grads[k].abs().max()) < 1e-12 and top < 1e-12, k
        else:
            assert float((grads[k] - ref).abs().max()) <= 1e-10 * top, (k, float((grads[k] - ref).abs().max()), top)
