"""The split-bf16 contraction (csrc/igemm_bx6.hip) held to fp32-level accuracy product by product: all six igemm_bx6_kernel<BM, BN, PAR>
instantiations, from the big -> small and the transposed direction, pixel-major and per-XCD-decoded launches among them, on the cases,
inputs and float64 references of tests/bx6_cases.py.  tests/test_bx6_cases_cpu.py shows on a model of the kernel's arithmetic that
assertions (a) and (b) below cannot hold for a kernel that lost one of its six products (every mutant misses its bar by >= 3 x in every
group; the intact arithmetic keeps half / two thirds of the bar to spare).

Every case of the table runs as conv2d forward, conv2d backward-data, deconv2d forward and deconv2d backward-data, under "bx6_all" and
under "f32".  Every call first asserts cgs_last_kernel(): the exact instantiation the restated dispatch predicts, or -- where the split-bf16
form does not serve the direction -- the exact-fp32 kernel's prefix.  Then:

    operator bar   max|delta| <= 2e-5 max|ref64| on the random family, unchanged (it catches indexing faults)
    (a) random family: mean |got - ref64| / sum|a||b| per group (parity class of a stride-2 transposed direction x 32-channel band of N)
        <= 4 x the same mean of the float32 torch-CPU oracle over the whole tensor; both kernels are held to it
    (b) cancelling families (activation-hi / weight-hi: the result lives in the mid and lo planes of one operand's split):
        max|got - ref64| / max|ref64| <= 10 x the larger of the float32 oracle's and the exact-fp32 kernel's figure
    (c) the call repeated is bit-equal; after the weights are scaled in place by 1.5 the result follows the new reference (operator bar
        and (a)): a stale packed-plane cache would not
    (d) activations x 2^20 and weights x 2^-30 give the outputs x 2^-10 bit for bit, in both modes: the split and every fp32 operation
        commute with exact scaling

Every figure is printed before it is asserted (run with -s).  Measured on the MI355X, the worst share of its bar per instantiation
(the figure itself in brackets; (a) over 1.5-scaled weights too):

                                        (a) random                              (b) act-hi cancelling   (b) weight-hi cancelling   operator bar
    igemm_bx6_kernel<128, 256, false>   0.35  (1.94e-8, 2x9x7x32x256x3x1 dF)    0.12  (5.9e-5)          0.11  (5.6e-5)             0.077
    igemm_bx6_kernel<128, 256, true>    0.43  (1.89e-8, 2x9x8x256x96x3x2 dB)    0.10  (4.8e-5)          0.10  (5.2e-5)             0.061
    igemm_bx6_kernel<256, 128, false>   0.35  (1.91e-8, 8x16x16x32x128x3x1 dF)  0.15  (6.2e-5)          0.15  (6.0e-5)             0.057
    igemm_bx6_kernel<256, 128, true>    0.47  (1.85e-8, 2x12x12x128x128x3x2 dB) 0.12  (5.3e-5)          0.12  (5.3e-5)             0.058
    igemm_bx6_kernel<128, 64, false>    0.55  (1.86e-8, 3x7x9x64x192x3x2 dB)    0.16  (6.0e-5)          0.14  (5.5e-5)             0.058
    igemm_bx6_kernel<128, 64, true>     0.22  (1.84e-8, 2x18x16x32x64x4x2 cF)   0.11  (4.7e-5)          0.10  (3.6e-5)             0.036
    igemm_kernel (f32, and the unserved directions)   0.34  (1.20e-8, 4x16x16x32x64x3x1 cB)   --        --                         0.044

(cF / cB / dF / dB: conv / deconv forward / backward-data.)  The split-bf16 kernel's mean scaled error is 1.8 .. 2.2e-8 in every
instantiation, direction and 32-column band -- its share of bar (a) moves with the float32 oracle's own figure, 2.1e-8 for a conv forward
and down to 8.5e-9 for an autograd backward-data over K = 1728 -- where the model of the intact arithmetic gives 1.2 .. 1.4e-8 and the
weakest mutant 4.2 x the bar.  On the cancelling families it sits at 1.0 .. 1.6 x the exact-fp32 kernel's error.  All 216 tests hold every
name, bit-equality and scaling assertion: no bar was moved, and no defect was found.
"""
import pytest
import torch

import bx6_cases as BC
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu


def run(case, op, a, w):
    """The call of a direction through cgs_amd.kernels, no bias, no epilogue -> (result, cgs_last_kernel())."""
    from cgs_amd import kernels as K, lib
    c = BC.call_of(case, op)
    s, hw = c.s, tuple(c.out_shape[1:3])
    if op == BC.CONV_FWD:
        got = K.conv2d_fwd(a, w, None, s, s)
    elif op == BC.CONV_BWD_DATA:
        got = K.conv2d_bwd_data(a, w, hw, s, s)
    elif op == BC.DECONV_FWD:
        got = K.deconv2d_fwd(a, w, None, hw, s, s)
    else:
        got = K.deconv2d_bwd_data(a, w, hw, s, s)
    assert tuple(got.shape) == c.out_shape
    return got, lib.last_kernel()


def run_both(case, op, a, w):
    """-> (split-bf16 result, exact-fp32 result), the kernel name of each call asserted."""
    from cgs_amd import kernels as K
    want = BC.kernel_name(BC.call_of(case, op))
    with K.contraction("bx6_all"):
        got, name = run(case, op, a, w)
    assert BC.name_matches(want, name), f"{BC.call_id(case, op)}: ran {name}, the table is there for {want}"
    f32, name = run(case, op, a, w)
    assert name.startswith(BC.IGEMM_PREFIX), f"{BC.call_id(case, op)} under f32: ran {name}"
    return got, f32


def hold_operator_bar(got, ref, what):
    err = BC.max_error(got, ref)
    print(f"{what}: max|delta|/max|ref| = {err:.2e} = {err / BC.OPERATOR_BAR:.3f} of the operator bar")
    assert err <= BC.OPERATOR_BAR, f"{what}: max|delta| / max|ref| = {err:.3e} vs {BC.OPERATOR_BAR}"


def hold_random_bar(case, op, got, ref, what):
    """Assertion (a): every group's mean scaled error against 4 x the float32 oracle's."""
    bar = BC.random_bar(ref)
    e = BC.scaled_error(got, ref)
    means = {g: float(e[idx].mean()) for g, idx in BC.groups(case, op)}
    worst = max(means, key=means.get)
    print(f"{what}: (a) worst group (py, px, band) = {worst}: {means[worst]:.2e} = {means[worst] / bar:.3f} of the bar {bar:.2e}; "
          f"best {min(means.values()) / bar:.3f}, {len(means)} groups")
    for g, m in means.items():
        assert m <= bar, f"{what}: group (py, px, band) = {g}: mean|delta|/sum|a||b| = {m:.3e} vs 4 x the float32 oracle's = {bar:.3e}"


PARAMS = [pytest.param(case, op, id=BC.call_id(case, op)) for case, op in BC.CALLS]


@pytest.mark.parametrize("case,op", PARAMS)
def test_random_family(case, op):
    """The operator bar, (a), (c) and (d)."""
    from cgs_amd import kernels as K
    d = dev()
    name = BC.kernel_name(BC.call_of(case, op))
    what = f"{BC.call_id(case, op)} {name} random"
    a, w = BC.inputs(case, op, BC.RANDOM)
    ref = BC.reference(case, op, BC.RANDOM)
    a_d, w_d = a.to(d), w.clone().to(d)
    got, f32 = run_both(case, op, a_d, w_d)
    for res, which in ((got, what), (f32, f"{BC.call_id(case, op)} {BC.IGEMM_PREFIX} (f32) random")):
        hold_operator_bar(res, ref, which)
        hold_random_bar(case, op, res, ref, which)
    # (c) the packed planes are taken as they are: bit-equal; then the weights change in place and the planes must follow
    again, _ = run_both(case, op, a_d, w_d)
    assert torch.equal(got, again), f"{what}: the call repeated is not bit-equal"
    # (d) exact scaling, in both modes, on fresh tensors (packed anew)
    s_got, s_f32 = run_both(case, op, a_d * 2.0 ** 20, w_d * 2.0 ** -30)
    assert torch.equal(s_got, got * 2.0 ** -10), f"{what}: activations x 2^20, weights x 2^-30 is not the result x 2^-10 bit for bit"
    assert torch.equal(s_f32, f32 * 2.0 ** -10), f"{what} (f32): activations x 2^20, weights x 2^-30 is not the result x 2^-10 bit for bit"
    w_d.mul_(1.5)
    ref15 = BC.reference(case, op, BC.RANDOM, 1.5)
    with K.contraction("bx6_all"):
        got15, ran = run(case, op, a_d, w_d)
    assert BC.name_matches(name, ran), ran
    hold_operator_bar(got15, ref15, what + ", weights x 1.5 in place")
    hold_random_bar(case, op, got15, ref15, what + ", weights x 1.5 in place")


@pytest.mark.parametrize("family", [BC.ACT_CANCEL, BC.W_CANCEL])
@pytest.mark.parametrize("case,op", PARAMS)
def test_cancelling_families(case, op, family):
    """(b): what is left when the hi pieces of one operand cancel pairwise along the reduced axis."""
    d = dev()
    what = f"{BC.call_id(case, op)} {BC.kernel_name(BC.call_of(case, op))} {family}"
    a, w = BC.inputs(case, op, family)
    ref = BC.reference(case, op, family)
    got, f32 = run_both(case, op, a.to(d), w.to(d))
    oracle, e32, err = BC.max_error(ref.oracle32, ref), BC.max_error(f32, ref), BC.max_error(got, ref)
    bar = BC.CANCEL_BAR_X * max(oracle, e32)
    print(f"{what}: (b) max|delta|/max|ref| = {err:.2e} = {err / bar:.3f} of the bar {bar:.2e} (float32 oracle {oracle:.2e}, f32 kernel {e32:.2e})")
    assert err <= bar, f"{what}: max|delta| / max|ref| = {err:.3e} vs 10 x max(float32 oracle {oracle:.3e}, f32 kernel {e32:.3e})"
