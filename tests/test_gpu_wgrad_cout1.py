"""``cgs_conv2d_nhwc_bwd_weight_cout1`` (csrc/wgrad_dot.hip): the weight gradient of a convolution to ONE output channel over a deep
reduction, against float64 autograd of ``oracle.ops_ref.conv2d`` on the same float32 inputs.  Bars: the conv weight gradient's own
(test_gpu_shaping.py, test_gpu_deconv_wgrad.py): 3e-5 of max|ref|, 2e-5 * sqrt(M / 1000) where M = B * Ho * Wo > 2250."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops_ref as R
from test_patchgan_shaping_cpu import SHORT_LAST_SLAB, co1_plan

# (B, H, W, Cin, k, s): the tiny net's d_c5, every tap crosses the border | non-square, asymmetric padding | stride 2, K = 1600 |
# Cin % 64 != 0 | a single pixel | five slabs, the last one short (test_patchgan_shaping_cpu.py)
SHAPES = [(4, 4, 4, 128, 4, 1), (2, 6, 5, 256, 4, 1), (3, 9, 7, 64, 5, 2), (2, 8, 8, 68, 4, 1), (1, 1, 1, 1024, 1, 1), SHORT_LAST_SLAB]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def wtol(M):
    return 3e-5 if M <= 2250 else 2e-5 * math.sqrt(M / 1000.0)


def close(got, want, tol, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs().max().item()
    ref = want.abs().max().item() + 1e-30
    print(f"{what}: max|delta|={err:.3e} max|ref|={ref:.3e} ratio={err / ref:.3e} bar={tol:.3e}")
    assert torch.isfinite(got).all() and err <= tol * ref, f"{what}: max|delta|={err:.3e} vs max|ref|={ref:.3e} (bar {tol:.1e})"


_cases = {}


def case(shape):
    """(x, dy, float64 dw, M) of a shape: computed once, shared, never written."""
    if shape not in _cases:
        B, H, W, Cin, k, s = shape
        x = rnd((B, H, W, Cin), 1)
        w = torch.zeros((k, k, Cin, 1), dtype=torch.float64, requires_grad=True)
        y = R.conv2d(x.double(), w, torch.zeros(1, dtype=torch.float64), s, s)
        dy = rnd(tuple(y.shape), 3)
        (y * dy.double()).sum().backward()
        _cases[shape] = (x.to(dev()), dy.to(dev()), w.grad.detach(), B * y.shape[1] * y.shape[2])
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_cout1_weight_grad_matches_float64(shape):
    from cgs_amd import kernels as K
    B, H, W, Cin, k, s = shape
    x, dy, want, M = case(shape)
    slabs, pps, _ = co1_plan(B, H, W, Cin, k, k, s, s)
    nan = torch.full((k, k, Cin, 1), float("nan"), device=dev())
    got = K.conv2d_bwd_weight_cout1(x, dy, k, k, s, s, out=nan)                    # NaN-filled output is overwritten
    assert got is nan
    close(got, want, wtol(M), f"cout1 wgrad {shape} slabs={slabs}x{pps}")
    again = K.conv2d_bwd_weight_cout1(x, dy, k, k, s, s)                           # a rerun is bit-identical
    assert torch.equal(got, again)
    generic = K.conv2d_bwd_weight(x, dy, k, k, s, s)                               # the generic GEMM kernel on the same inputs
    close(got, generic, 3e-5, f"cout1 vs generic {shape}")
    old = rnd((k, k, Cin, 1), 7, float(want.abs().max()))                          # accumulation onto unrelated contents
    acc = K.conv2d_bwd_weight_cout1(x, dy, k, k, s, s, out=old.to(dev()), accumulate=True)
    close(acc, old.double() + want, wtol(M), f"accumulate {shape}")
    assert not torch.equal(acc.cpu(), old)


def test_exact_size_workspace_and_one_byte_short():
    from cgs_amd import lib
    shape = SHORT_LAST_SLAB
    B, H, W, Cin, k, s = shape
    x, dy, want, M = case(shape)
    need = int(lib.load().cgs_conv_wgrad_cout1_ws_bytes(B, H, W, Cin, k, k, s, s))
    assert need > 0 and need % 16 == 0
    # the partials end exactly at a guard region that must stay as it is
    buf = torch.full((need // 4 + 64,), 123.0, device=dev())
    dw = torch.full((k, k, Cin, 1), 5.0, device=dev())
    tail = (B, H, W, Cin, k, k, s, s, 0, buf.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.load().cgs_conv2d_nhwc_bwd_weight_cout1(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *tail, need - 1, stream)
    assert rc == lib.EWORKSPACE and b"workspace" in lib.load().cgs_last_error()
    torch.cuda.synchronize()
    assert float((dw - 5.0).abs().max()) == 0.0 and float((buf - 123.0).abs().max()) == 0.0      # nothing was launched
    lib.call("cgs_conv2d_nhwc_bwd_weight_cout1", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *tail, need, stream)
    close(dw, want, wtol(M), "exact workspace")
    assert float((buf[need // 4:] - 123.0).abs().max()) == 0.0                                 # no store past the stated size


@pytest.mark.parametrize("B,H,W,Cin,k", [(2, 8, 8, 6, 16), (2, 8, 8, 32, 4)], ids=["Cin=6", "K=512"])
def test_refused_shapes_leave_the_output_untouched(B, H, W, Cin, k):
    from cgs_amd import lib
    x, dy = rnd((B, H, W, Cin), 1).to(dev()), rnd((B, H, W, 1), 2).to(dev())
    dw = torch.full((k, k, Cin, 1), 5.0, device=dev())
    ws = torch.zeros(1 << 20, device=dev())
    assert int(lib.load().cgs_conv_wgrad_cout1_ws_bytes(B, H, W, Cin, k, k, 1, 1)) == 0
    rc = lib.load().cgs_conv2d_nhwc_bwd_weight_cout1(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, Cin, k, k, 1, 1, 0, ws.data_ptr(),
                                                     ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    assert rc == lib.EINVAL
    torch.cuda.synchronize()
    assert float((dw - 5.0).abs().max()) == 0.0 and float(ws.abs().max()) == 0.0
    from cgs_amd import kernels as K
    with pytest.raises(lib.CgsError):
        K.conv2d_bwd_weight_cout1(x, dy, k, k, 1, 1, out=dw)
    assert float((dw - 5.0).abs().max()) == 0.0
