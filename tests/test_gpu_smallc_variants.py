"""The small-channel transposed-conv kernels variant by variant (csrc/convt_smalln.hip, csrc/convt_quad.hip: convt_smalln_kernel<N>,
convt_quad_mfma_kernel<4>, all 16 convt_quad_lds_kernel<N, TW, NYX> and the persistent form of the latter), and five forward variants no
other test names, against the float64 reference of tests/smallc_cases.py.  Every call first asserts that cgs_last_kernel() is the kernel
the restated dispatch predicts -- the table says which variant a shape is there for, so a dispatch change that sends it elsewhere fails
here instead of silently testing another kernel -- and then holds the result to the project's operator bar, unchanged:

    max|delta| <= 2e-5 max(1, sqrt(k k Cs / 1000)) max|ref|        (x 1.5 under the forward tanh; tests/test_gpu_fuzz.py, ktol)

over the whole tensor and, for the transposed direction, over every parity class (py, px) and output channel on its own (against the
same bar times the GLOBAL max|ref|), so that a failure names the class and channel that is wrong.  Each forward is called twice with the
same weight tensor (the second call takes the packed workspace as it is: bit-equal results), then the weights are scaled in place and the
result has to follow (the workspace cache re-packs; the kernels that pack nothing must not care).

The float32 torch-CPU oracle's own worst against the same reference is 5.0e-7 of max|ref| (0.017 of the bar) over the transposed table
and 1.2e-6 (0.040 of the bar) over the forward one (smallc_cases.ORACLE_*, tests/test_smallc_cases_cpu.py).

The device's measured worst max|delta| / max|ref| per variant (MI355X; every figure is printed before it is asserted, run with -s):
    convt_smalln_kernel                5.2e-7   0.026 of the bar   at 5x9x13x20x3x5 fwd lrelu
    convt_quad_mfma_kernel<4>          1.04e-6  0.034              at 2x4x6x48x4x7 bwd none
    convt_quad_lds_kernel<1, 16, 0>    4.4e-7   0.015              at 2x6x48x16x1x3 fwd tanh
    convt_quad_lds_kernel<1, 16, 3>    4.3e-7   0.022              at 2x6x48x16x1x5 fwd, weights x -2
    convt_quad_lds_kernel<1, 32, 0>    2.8e-7   0.014              at 2x8x64x16x1x3 fwd none
    convt_quad_lds_kernel<1, 32, 3>    4.3e-7   0.022              at 2x8x64x16x1x5 bwd relu_bwd_affine
    convt_quad_lds_kernel<2, 16, 0>    3.8e-7   0.019              at 2x7x9x32x2x3 fwd, weights x -2
    convt_quad_lds_kernel<2, 16, 3>    1.09e-6  0.036              at 1027x8x8x16x2x5 fwd tanh (persistent; 171x20x36x16x2x5: 9.0e-7)
    convt_quad_lds_kernel<2, 32, 0>    4.2e-7   0.014              at 2x8x32x16x2x3 fwd tanh
    convt_quad_lds_kernel<2, 32, 3>    5.4e-7   0.018              at 2x8x32x16x2x5 fwd tanh
    convt_quad_lds_kernel<3, 16, 0>    4.1e-7   0.014              at 2x9x34x16x3x3 fwd tanh
    convt_quad_lds_kernel<3, 16, 3>    4.7e-7   0.023              at 2x8x40x16x3x5 bwd relu_bwd_affine
    convt_quad_lds_kernel<3, 32, 0>    4.0e-7   0.013              at 2x8x64x16x3x3 fwd tanh
    convt_quad_lds_kernel<3, 32, 3>    6.6e-7   0.022              at 2x16x64x16x3x5 fwd tanh
    convt_quad_lds_kernel<4, 16, 0>    2.5e-7   0.012              at 2x5x5x16x4x3 bwd none
    convt_quad_lds_kernel<4, 16, 3>    7.0e-7   0.035              at 3x20x12x32x4x5 bwd relu_bwd_affine
    convt_quad_lds_kernel<4, 32, 0>    8.1e-7   0.027              at 1025x8x32x16x4x3 fwd tanh (persistent)
    convt_quad_lds_kernel<4, 32, 3>    6.4e-7   0.032              at 130x8x32x16x4x5 bwd none
    igemm_kernel (the calls handed on) 4.9e-7   0.025              at 5x9x13x20x3x5 bwd relu_bwd_affine
    conv_patch_kernel                  2.8e-7   0.014              at 2x16x32x1x32x5x2 fwd none
    conv_smalln_f_kernel               8.0e-7   0.027              at 2x256x256x16x2x3x1 fwd tanh
    conv_dot_kernel<2>                 2.6e-7   0.008              at 2x6x7x128x2x3x2 fwd tanh

All 353 figures lie within 0.036 of the bar, every kernel-name assertion holds, and the second call of every forward is bit-equal: no
variant needs more than the bar (fast_tanh of convt_quad.hip, documented at 2.4e-7 absolute, included), and no defect was found.
"""
import pytest
import torch

import smallc_cases as SC
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu


def hold(got, want, tol, what, classes=True):
    """Print max|delta| / max|ref|, then assert it per parity class and channel (transposed direction) and over the whole tensor."""
    err = (got.detach().cpu().double() - want).abs()
    ref = float(want.abs().max())
    worst = float(err.max())
    print(f"device {what}: max|delta|/max|ref| = {worst / ref:.3e} = {worst / ref / tol:.3f} of the bar {tol:.2e}")
    assert tuple(got.shape) == tuple(want.shape)
    if classes:
        for (py, px, n), e in SC.parity_slices(err):
            assert float(e.max()) <= tol * ref, f"{what}: parity class (py, px) = ({py}, {px}), channel {n}: max|delta| = {float(e.max()):.3e} " \
                                                f"vs {tol:.2e} x max|ref| = {tol * ref:.3e}"
    assert worst <= tol * ref, f"{what}: max|delta| = {worst:.3e} vs {tol:.2e} x max|ref| = {tol * ref:.3e}"


@pytest.fixture
def packed_flags(monkeypatch):
    """The ws_prepacked flag of every conv-family call of the test, as the workspace cache hands it out."""
    from cgs_amd import kernels as K
    seen, get = [], K.WS.get

    def spy(*args, **kwargs):
        ws, pre = get(*args, **kwargs)
        seen.append(pre)
        return ws, pre
    monkeypatch.setattr(K.WS, "get", spy)
    return seen


T_PARAMS = [pytest.param(want, shape, id=SC.tshape_id(shape)) for want, shape, _ in SC.TRANSPOSED]


@pytest.mark.parametrize("want,shape", T_PARAMS)
def test_transposed_forward(want, shape, packed_flags):
    """deconv2d [B,Hs,Ws,Cs] -> [B,2Hs,2Ws,N]: bias with none / lrelu / tanh, no bias; twice per call; weights scaled in place."""
    from cgs_amd import kernels as K, lib
    d = dev()
    B, Hs, Ws, Cs, N, k = shape
    inp = SC.t_inputs(shape)
    lin, _ = SC.t_reference(shape)
    x, w, bias = inp.x.to(d), inp.w.clone().to(d), inp.bias.to(d)
    for e in SC.FWD_EPILOGUES:
        pred = SC.predict(*SC.t_call(shape, SC.DECONV_FWD, e))
        assert pred.kernel == want
        got = K.deconv2d_fwd(x, w, bias, (2 * Hs, 2 * Ws), 2, 2, e)
        assert lib.last_kernel() == want, (lib.last_kernel(), want)
        again = K.deconv2d_fwd(x, w, bias, (2 * Hs, 2 * Ws), 2, 2, e)
        assert lib.last_kernel() == want and packed_flags[-1] == 1 and torch.equal(got, again)
        hold(got, SC.fwd_epilogue64(lin, inp.bias, e), SC.bar(k, Cs, e), f"{want} {SC.tshape_id(shape)} fwd {SC.EPI_NAMES[e]}")
    assert packed_flags[0] == 0 and all(packed_flags[1:])             # packed once, by the first call
    got = K.deconv2d_fwd(x, w, None, (2 * Hs, 2 * Ws), 2, 2)
    assert lib.last_kernel() == want
    hold(got, lin, SC.bar(k, Cs, SC.EPI_NONE), f"{want} {SC.tshape_id(shape)} fwd no bias")
    w.mul_(-2.0)                                                     # (exact in float32: the reference is -2 x the same float64 sums)
    got = K.deconv2d_fwd(x, w, bias, (2 * Hs, 2 * Ws), 2, 2)
    assert lib.last_kernel() == want and packed_flags[-1] == 0
    hold(got, SC.fwd_epilogue64(-2.0 * lin, inp.bias, SC.EPI_NONE), SC.bar(k, Cs, SC.EPI_NONE), f"{want} {SC.tshape_id(shape)} fwd weights x -2")


@pytest.mark.parametrize("want,shape", T_PARAMS)
def test_transposed_backward_data(want, shape):
    """The same contraction as the backward-data of the conv2d [B,2Hs,2Ws,N] -> [B,Hs,Ws,Cs] with the same weights viewed as [k,k,N,Cs],
    plain and with the three folded activation gradients.  The quad family serves them all; convt_smalln serves the plain call and
    hands the epilogues to the implicit GEMM, which one case says by name."""
    from cgs_amd import kernels as K, lib
    d = dev()
    B, Hs, Ws, Cs, N, k = shape
    inp = SC.t_inputs(shape)
    _, lin = SC.t_reference(shape)
    dy, w, a = inp.dy.to(d), inp.w.to(d), inp.a.to(d)
    for e in SC.BWD_EPILOGUES:
        pred = SC.predict(*SC.t_call(shape, SC.CONV_BWD_DATA, e))
        if want == SC.SMALLN_T and e != SC.EPI_NONE:
            assert pred.family == SC.FAMILY_IGEMM
            if shape != SC.SMALLN_BWD_EPILOGUE_SHAPE:
                continue
        else:
            assert pred.kernel == want
        aux = SC.bwd_aux(inp, e)
        got = K.conv2d_bwd_data(dy, w, (2 * Hs, 2 * Ws), 2, 2, epilogue=e, ep_a=a if e == SC.EPI_RELU_BWD_AFFINE else None,
                                ep_aux=None if aux is None else aux.to(d))
        assert SC.kernel_matches(pred, lib.last_kernel()), (lib.last_kernel(), pred)
        hold(got, SC.bwd_epilogue64(lin, e, a=inp.a, aux=aux), SC.bar(k, Cs, e),
             f"{pred.kernel if pred.family == SC.FAMILY_IGEMM else want} {SC.tshape_id(shape)} bwd {SC.EPI_NAMES[e]}")


@pytest.mark.parametrize("shape", SC.AFFINE_RELU_SHAPES, ids=SC.tshape_id)
def test_affine_relu_leaves_the_small_channel_families(shape):
    """relu(a v + b) is not an epilogue of the VALU and quad kernels: the call lands on the implicit GEMM, and still matches."""
    from cgs_amd import kernels as K, lib
    d = dev()
    B, Hs, Ws, Cs, N, k = shape
    inp = SC.t_inputs(shape)
    lin, _ = SC.t_reference(shape)
    pred = SC.predict(*SC.t_call(shape, SC.DECONV_FWD, SC.EPI_AFFINE_RELU))
    assert pred.family == SC.FAMILY_IGEMM and SC.predict(*SC.t_call(shape, SC.DECONV_FWD, SC.EPI_NONE)).family != SC.FAMILY_IGEMM
    got = K.deconv2d_fwd(inp.x.to(d), inp.w.to(d), inp.bias.to(d), (2 * Hs, 2 * Ws), 2, 2, SC.EPI_AFFINE_RELU, inp.a.to(d), inp.b.to(d))
    assert lib.last_kernel().startswith(SC.IGEMM_PREFIX), lib.last_kernel()
    hold(got, SC.fwd_epilogue64(lin, inp.bias, SC.EPI_AFFINE_RELU, inp.a, inp.b), SC.bar(k, Cs, SC.EPI_AFFINE_RELU),
         f"{SC.IGEMM_PREFIX} {SC.tshape_id(shape)} fwd affine_relu")


@pytest.mark.parametrize("want,shape", [pytest.param(w_, s, id=SC.tshape_id(s)) for w_, s in SC.FORWARD])
def test_forward_variants_by_name(want, shape):
    """conv2d forward on the general conv_patch_kernel (one and two input channels), conv_smalln_f_kernel at N = 2 and conv_dot_kernel<2>."""
    from cgs_amd import kernels as K, lib
    d = dev()
    B, H, W, Cin, Cout, k, s = shape
    inp = SC.f_inputs(shape)
    lin = SC.f_reference(shape)
    x, w, bias = inp.x.to(d), inp.w.to(d), inp.bias.to(d)
    for e in SC.FWD_EPILOGUES:
        assert SC.predict(*SC.f_call(shape, e)).kernel == want
        got = K.conv2d_fwd(x, w, bias, s, s, e)
        assert lib.last_kernel() == want, (lib.last_kernel(), want)
        hold(got, SC.fwd_epilogue64(lin, inp.bias, e), SC.bar(k, Cin, e), f"{want} {SC.tshape_id(shape)} fwd {SC.EPI_NAMES[e]}", classes=False)
