"""``cgs_deconv2d_nhwc_bwd_weight`` (csrc/wgrad.hip): the weight gradient of the transposed convolution, against float64 on the CPU from the
same float32 inputs.  The bars are the project's own for the conv weight gradient: 3e-5 of max|ref| up to 1000 reduced
pixels, 2e-5 * sqrt(M / 1000) above; M = B * Hin * Win, the pixels of the deconv's INPUT."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_training_cpu import deconv_filter_grad
from wgrad_plan import SPLIT_CAP, wgrad_plan


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def wtol(M):
    return 3e-5 if M <= 1000 else 2e-5 * math.sqrt(M / 1000.0)


def close(got, want, tol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: inf / NaN in the result"
    err = (got - want).abs().max().item()
    ref = want.abs().max().item() + 1e-30
    print(f"{what} max|delta|={err:.3e} max|ref|={ref:.3e} ratio={err / ref:.3e} bar={tol:.3e}")
    assert err <= tol * ref, f"{what}: max|delta|={err:.3e} vs max|ref|={ref:.3e} (bar {tol:.1e})"


_REF = {}


def case(shape):
    """(x, dy, float64 reference, plan) of a shape (B, Hin, Win, Cin, Hout, Wout, Cout, kh, kw, s): computed once, never written to."""
    if shape not in _REF:
        B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s = shape
        x, dy = rnd((B, Hi, Wi, Ci), 21), rnd((B, Ho, Wo, Co), 22)
        _REF[shape] = (x, dy, deconv_filter_grad(x.double(), dy.double(), kh, kw, s), wgrad_plan(B, Ho, Wo, Co, Ci, kh, kw, s, s))
    return _REF[shape]


def run(shape, out=None, accumulate=False):
    from cgs_amd import kernels as K
    B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s = shape
    x, dy, want, p = case(shape)
    assert (p.Ho, p.Wo, p.M) == (Hi, Wi, B * Hi * Wi)
    return K.deconv2d_bwd_weight(x.to(dev()), dy.to(dev()), kh, kw, s, s, out=out, accumulate=accumulate), want, p


# (B, Hin, Win, Cin, Hout, Wout, Cout, kh, kw, s)
SHAPES = [(2, 3, 3, 5, 6, 6, 3, 4, 4, 2),
          (2, 3, 3, 5, 5, 5, 3, 5, 5, 2),               # odd output
          (3, 7, 7, 128, 14, 14, 64, 4, 4, 2),          # mnist g_dc3; M = 147 in two slabs of 96: a short last slab
          (2, 7, 7, 64, 14, 14, 1, 4, 4, 2),            # Cout = 1: 16 rows of one tile, the scalar gather
          (2, 8, 8, 64, 16, 16, 3, 5, 5, 2),            # Cout = 3: 75 rows
          (1, 4, 4, 6, 4, 4, 7, 3, 3, 1),               # stride 1
          (2, 2, 2, 130, 4, 4, 127, 5, 5, 2),           # both sides of a tile edge, off both 16-byte paths
          (2, 2, 2, 127, 4, 4, 130, 5, 5, 2),
          (2, 3, 5, 6, 6, 10, 5, 4, 4, 2),              # non-square
          (1, 3, 3, 5, 6, 6, 3, 4, 4, 2),               # M = 9: one slab
          (7, 1, 4663, 8, 2, 9326, 8, 4, 4, 2)]         # M = 32 641 = 255 * 128 + 1: the smallest pixel count that reaches the slab cap


@pytest.mark.parametrize("shape", SHAPES)
def test_deconv_weight_gradient_matches_float64(shape):
    B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s = shape
    out = torch.full((kh, kw, Co, Ci), float("nan"), device=dev())             # (a NaN left = an element skipped)
    got, want, p = run(shape, out=out)
    assert got is out
    close(got, want, wtol(p.M), f"deconv wgrad {shape} splits={p.splits}x{p.m_per_split}")


def test_the_split_cases_are_what_they_claim():
    one, short, cap = case(SHAPES[9])[3], case(SHAPES[2])[3], case(SHAPES[10])[3]
    assert (one.M, one.splits) == (9, 1)
    assert short.splits == 2 and short.M - short.m_per_split == 51 < short.m_per_split
    assert cap.splits == SPLIT_CAP and cap.tiles == 1 and wgrad_plan(1, 2, 65280, 8, 8, 4, 4, 2, 2).splits == SPLIT_CAP - 1
    from cgs_amd import lib
    for shape in SHAPES:
        B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s = shape
        p = case(shape)[3]
        assert int(lib.load().cgs_deconv_wgrad_ws_bytes(B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s, s)) == p.splits * p.Kc * p.Csp * 4


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]])
def test_accumulates_onto_unrelated_contents_and_overwrites_nan(shape):
    B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s = shape
    want, p = case(shape)[2], case(shape)[3]
    old = rnd((kh, kw, Co, Ci), 23, float(want.abs().max()))
    got, _, _ = run(shape, out=old.to(dev()), accumulate=True)
    # old + gradient: one more float32 addition of two numbers of the gradient's size on top of the gradient's own bar (as for the conv entry)
    close(got, old.double() + want, wtol(p.M), f"accumulate {shape}")
    assert not torch.equal(got.cpu(), old)
    got0, _, _ = run(shape, out=torch.full((kh, kw, Co, Ci), float("nan"), device=dev()), accumulate=False)
    assert torch.isfinite(got0).all()
    close(got0, want, wtol(p.M), f"overwrite {shape}")


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[10]])
def test_two_runs_are_bit_equal(shape):
    a = run(shape)[0].clone()
    b = run(shape)[0]
    assert torch.equal(a, b)


def test_refusals():
    from cgs_amd import lib
    d = dev()
    B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s = SHAPES[2]
    x, dy = case(SHAPES[2])[0].to(d), case(SHAPES[2])[1].to(d)
    dw = torch.zeros((kh, kw, Co, Ci), device=d)
    need = int(lib.load().cgs_deconv_wgrad_ws_bytes(B, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, s, s))
    ws = torch.empty(need // 4, device=d)
    args = (x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, Hi, Wi, Ci)
    tail = (Co, kh, kw, s, s, 0)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(lib.CgsError, match=r"deconv2d_nhwc_bwd_weight: workspace \d+ < \d+ bytes"):           # a short workspace
        lib.call("cgs_deconv2d_nhwc_bwd_weight", *args, Ho, Wo, *tail, ws.data_ptr(), need - 4, stream)
    with pytest.raises(lib.CgsError, match=r"workspace 0 < "):
        lib.call("cgs_deconv2d_nhwc_bwd_weight", *args, Ho, Wo, *tail, None, 0, stream)
    # an output that is no 'SAME' pre-image of the input: ceil(15 / 2) = 8 != 7, ceil(12 / 2) = 6 != 7
    with pytest.raises(lib.CgsError, match=r"'SAME' geometry mismatch: big 15x14 stride 2x2 needs small 8x7, got 7x7"):
        lib.call("cgs_deconv2d_nhwc_bwd_weight", *args, 15, 14, *tail, ws.data_ptr(), need, stream)
    with pytest.raises(lib.CgsError, match=r"'SAME' geometry mismatch"):
        lib.call("cgs_deconv2d_nhwc_bwd_weight", *args, 14, 12, *tail, ws.data_ptr(), need, stream)
    with pytest.raises(lib.CgsError, match=r"bad argument"):
        lib.call("cgs_deconv2d_nhwc_bwd_weight", None, dy.data_ptr(), dw.data_ptr(), B, Hi, Wi, Ci, Ho, Wo, *tail, ws.data_ptr(), need, stream)
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0.0                      # nothing was launched
    lib.call("cgs_deconv2d_nhwc_bwd_weight", *args, Ho, Wo, *tail, ws.data_ptr(), need, stream)             # and the exact size is enough
    close(dw, case(SHAPES[2])[2], wtol(B * Hi * Wi), "exact workspace")
