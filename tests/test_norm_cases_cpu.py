"""The norm tests' own inputs and reference (tests/norm_cases.py), checked without a GPU: the float64 definitions against
torch.autograd in float64, the builder's kink condition on every backward case the device tests run, and the synthetic partial rows."""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC


@pytest.mark.parametrize("groups,M,C", [(1, 17, 40), (1, 129, 4), (3, 130, 40), (3, 128, 40)])
@pytest.mark.parametrize("leak", [0.2, 1.0, 0.0])
def test_reference_equals_float64_autograd(groups, M, C, leak):
    """groups == 1: batch norm + lrelu; groups > 1: instance norm + lrelu (a group = one sample).  Forward and input gradient."""
    inp = NC.build_inputs(groups, M, C, leak)
    x = inp.x.double().requires_grad_(True)
    g, b = inp.gamma.double(), inp.beta.double()
    xc = x.permute(0, 2, 1)                                              # [groups, C, M]: torch's channel-second layout
    if groups == 1:
        n = F.batch_norm(xc, None, None, g, b, training=True, eps=NC.EPS)
    else:
        n = F.instance_norm(xc, weight=g, bias=b, eps=NC.EPS)
    y = F.leaky_relu(n, leak).permute(0, 2, 1)
    (y * inp.dy.double()).sum().backward()
    mean, var, invstd = NC.stats_from_x(inp.x)
    want_y = NC.ref_fwd(inp.x, inp.gamma, inp.beta, mean, invstd, leak)
    want_dx = NC.ref_bwd(inp.dy, inp.x, inp.gamma, inp.beta, mean, invstd, leak)           # the unrounded statistics: the exact definition
    for want, got in ((want_y, y.detach()), (want_dx, x.grad)):        # per channel: the constant channel's dx is ~300 x the others'
        assert bool(((want - got).abs().amax((0, 1)) <= 1e-12 * got.abs().amax((0, 1))).all())
    # the constant channel: var == 0, invstd == 1/sqrt(eps), y == lrelu(beta) exactly
    c = inp.const_c
    assert bool((var[:, c] == 0).all()) and bool((mean[:, c] == NC.CONST).all())
    assert bool((want_y[:, :, c] == NC.lrelu(b[c], leak)).all())


def backward_shapes():
    return sorted({(g, M, C) for _, g, M, C, _, _ in NC.BWD_FROM_X} | {(g, M, C) for g, _, _, _, M, C, _, _ in NC.FROM_PARTIALS})


@pytest.mark.parametrize("groups,M,C", backward_shapes())
def test_no_backward_input_lies_near_the_kink(groups, M, C):
    inp = NC.build_inputs(groups, M, C)                    # (asserts the condition itself)
    assert NC.kink_count(inp) == 0
    assert bool((inp.x[:, :, inp.const_c] == NC.CONST).all())
    assert inp.beta.abs().min().item() >= NC.BETA_MIN * (1 - 1e-6)
    mean, _, invstd = NC.stats_from_x(inp.x)               # what the backward is handed is the float32 rounding of x's own statistics
    assert torch.equal(inp.mean, mean.float()) and torch.equal(inp.invstd, invstd.float())


@pytest.mark.parametrize("groups,rows_per_seg,nseg,seg_stride,M,C", sorted({c[:6] for c in NC.FROM_PARTIALS}))
def test_synthetic_partial_rows_partition_the_buffer(groups, rows_per_seg, nseg, seg_stride, M, C):
    p = NC.build_partials(groups, rows_per_seg, nseg, seg_stride, C, M)
    rows_total, R, S, stride = p.layout
    assert p.part.shape == (rows_total, 2, C) and rows_total == S * stride
    owned = p.owner >= 0
    nan_row = p.part.isnan().all(2).all(1)
    finite_row = p.part.isfinite().all(2).all(1)
    assert torch.equal(nan_row, ~owned) and torch.equal(finite_row, owned)          # NaN gap rows and owned rows partition the buffer
    assert int(owned.sum()) == groups * R * S and int((~owned).sum()) == S * (stride - groups * R)
    for gi, rows in enumerate(NC.owned_rows(groups, R, S, stride)):
        assert bool((p.owner[torch.tensor(rows)] == gi).all())
    own = p.part[owned].reshape(int(owned.sum()), 2 * C)
    assert own.unique(dim=0).shape[0] == own.shape[0]                                # distinct rows: a wrong row changes the sums ...
    for col in own.T:                                                                # ... in every channel (bar a float32 birthday collision)
        assert col.unique().numel() >= 0.99 * col.numel()
    mean, e2 = NC.partial_sums(p)
    assert bool((e2 > 0).all()) and bool((e2 - mean * mean >= 0.1 * e2).all())     # no cancellation in the float64 formula
    assert bool((mean.abs() >= 0.1 * (1 - 1e-6)).all())
