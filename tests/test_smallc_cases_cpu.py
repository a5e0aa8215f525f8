"""tests/smallc_cases.py checked without a device: the restated dispatch against the library's own cgs_conv_family, the coverage the case
tables claim (printed: run with -s), the float64 reference against float64 autograd of the oracle's conv2d, and the reference side of the
bar of tests/test_gpu_smallc_variants.py -- the float32 oracle's error against float64, normalised as that test normalises the device's."""
import numpy as np
import pytest
import torch

import smallc_cases as SC
from oracle import ops_ref as R

T_SHAPES = [shape for _, shape, _ in SC.TRANSPOSED]
ORACLE_SLACK = 2.0      # the recorded figures are one machine's: torch-CPU's float32 summation order changes with the thread count


@pytest.fixture(autouse=True)
def _plain_cpu_convolutions():
    """torch-CPU's oneDNN convolution backward corrupts the heap on some degenerate shapes (tests/test_gpu_fuzz.py); the native kernels are fine."""
    with torch.backends.mkldnn.flags(enabled=False):
        yield


def _all_calls():
    """Every call the GPU test makes, as the arguments of SC.predict."""
    for _, shape, _ in SC.TRANSPOSED:
        for e in SC.FWD_EPILOGUES + (SC.EPI_AFFINE_RELU,):
            yield SC.t_call(shape, SC.DECONV_FWD, e)
        for e in SC.BWD_EPILOGUES:
            yield SC.t_call(shape, SC.CONV_BWD_DATA, e)
    for _, shape in SC.FORWARD:
        for e in SC.FWD_EPILOGUES:
            yield SC.f_call(shape, e)


def test_restated_family_equals_the_librarys():
    """SC.predict's family against cgs_conv_family for every call the GPU test makes, and on a sweep around the tables' shapes."""
    from cgs_amd import lib
    l = lib.load()
    assert lib.get_contraction() == "f32"
    n = 0
    for call in _all_calls():
        assert SC.predict(*call).family == SC.lib_family(l, *call), call
        n += 1
    # ... and on a sweep around the tables' shapes, so that a condition restated wrongly but not binding on the tables shows too
    for B in (1, 3, 1030):
        for Hs, Ws in ((1, 1), (5, 7), (8, 32), (6, 48)):
            for Cs in (4, 12, 16, 48, 160, 512):
                for N in (1, 2, 3, 4, 5):
                    for k in (1, 2, 3, 4, 5, 6, 7):
                        for e in (SC.EPI_NONE, SC.EPI_AFFINE_RELU, SC.EPI_TANH, SC.EPI_LRELU_BWD):
                            for op in (SC.DECONV_FWD, SC.CONV_BWD_DATA):
                                if (op == SC.CONV_BWD_DATA) != (e in (SC.EPI_NONE, SC.EPI_LRELU_BWD)) and e != SC.EPI_NONE:
                                    continue
                                call = SC.t_call((B, Hs, Ws, Cs, N, k), op, e)
                                assert SC.predict(*call).family == SC.lib_family(l, *call), call
                                n += 1
    print(f"restated family == cgs_conv_family on {n} calls")


def test_tables_reach_what_they_claim():
    """Every row reaches the kernel it names in both directions and with every epilogue; the 16 + 1 + 4 variants are all there; the
    persistent plans, the global-load cases and the VALU cases have the properties their rows name.  Prints the coverage list."""
    assert len(set(T_SHAPES)) == len(T_SHAPES)
    names, smalln_n = {}, set()
    for want, shape, why in SC.TRANSPOSED:
        B, Hs, Ws, Cs, N, k = shape
        for op, epis in ((SC.DECONV_FWD, SC.FWD_EPILOGUES), (SC.CONV_BWD_DATA, SC.BWD_EPILOGUES)):
            for e in epis:
                p = SC.predict(*SC.t_call(shape, op, e))
                if want == SC.SMALLN_T and e >= SC.EPI_RELU_BWD_AFFINE:
                    assert p == SC.Prediction(SC.FAMILY_IGEMM, SC.IGEMM_PREFIX, None), (shape, e, p)      # handed on to the implicit GEMM
                    continue
                assert p.kernel == want, (shape, SC.EPI_NAMES[e], p)
                assert p.family == (SC.FAMILY_SMALLN_T if want == SC.SMALLN_T else SC.FAMILY_QUAD)
        assert SC.predict(*SC.t_call(shape, SC.DECONV_FWD, SC.EPI_AFFINE_RELU)).family == SC.FAMILY_IGEMM
        names.setdefault(want, []).append(shape)
        if want == SC.SMALLN_T:
            smalln_n.add(N)
    lds = {f"convt_quad_lds_kernel<{n}, {tw}, {yx}>" for n in (1, 2, 3, 4) for tw in (16, 32) for yx in (3, 0)}
    assert lds <= set(names) and SC.QUAD_MFMA in names and smalln_n == {1, 2, 3, 4}
    assert set(names) == lds | {SC.QUAD_MFMA, SC.SMALLN_T}
    for name in sorted(names):
        print(f"{name}: {', '.join(SC.tshape_id(s) for s in names[name])}")
    print(f"{SC.SMALLN_T}: N = {sorted(smalln_n)}")
    for s in SC.AFFINE_RELU_SHAPES + [SC.SMALLN_BWD_EPILOGUE_SHAPE] + SC.PERSISTENT + [SC.NOT_PERSISTENT]:
        assert s in T_SHAPES
    assert {SC.predict(*SC.t_call(s, SC.DECONV_FWD, SC.EPI_NONE)).family for s in SC.AFFINE_RELU_SHAPES} == {SC.FAMILY_QUAD, SC.FAMILY_SMALLN_T}
    assert SC.predict(*SC.t_call(SC.SMALLN_BWD_EPILOGUE_SHAPE, SC.DECONV_FWD, SC.EPI_NONE)).family == SC.FAMILY_SMALLN_T

    # the persistent launches: >= 4 tiles per block, a ragged last block; runs that cross an image boundary inside the run
    crossing = 0
    for shape in SC.PERSISTENT:
        for op in (SC.DECONV_FWD, SC.CONV_BWD_DATA):
            plan = SC.predict(*SC.t_call(shape, op, SC.EPI_NONE)).plan
            assert plan.tiles >= 1024 and plan.per >= 4 and 0 < plan.last < plan.per and plan.blocks == SC.ceil_div(plan.tiles, plan.per), plan
        runs = [(b * plan.per, min((b + 1) * plan.per, plan.tiles) - 1) for b in range(plan.blocks)]
        cross = sum(1 for t0, t1 in runs if t0 // plan.tiles_per_image != t1 // plan.tiles_per_image)
        mid = sum(1 for t0, t1 in runs if any(t % plan.tiles_per_image for t in range(t0 + 1, t1 + 1)) and t0 // plan.tiles_per_image != t1 // plan.tiles_per_image)
        crossing += cross
        print(f"persistent {SC.tshape_id(shape)}: {plan}; {cross} of {plan.blocks} runs cross an image boundary, {mid} of them with an image's tiles split over two runs")
    assert crossing > 0
    plan = SC.predict(*SC.t_call((171, 20, 36, 16, 2, 5), SC.DECONV_FWD, SC.EPI_NONE)).plan
    assert plan.tiles_per_image == 6 and plan.per % plan.tiles_per_image and plan.tiles_per_image % plan.per       # images split over runs
    plan = SC.predict(*SC.t_call(SC.NOT_PERSISTENT, SC.DECONV_FWD, SC.EPI_NONE)).plan
    assert plan.per == 1 and plan.blocks == plan.tiles == 130
    for want, shape, _ in SC.TRANSPOSED:                      # every other LDS case keeps one tile per block
        if shape not in SC.PERSISTENT and want.startswith("convt_quad_lds"):
            assert SC.predict(*SC.t_call(shape, SC.DECONV_FWD, SC.EPI_NONE)).plan.per == 1

    # what the global-load cases are there for
    mfma = {shape: why for want, shape, why in SC.TRANSPOSED if want == SC.QUAD_MFMA}
    quads = {s: s[0] * s[1] * s[2] for s in mfma}
    assert any(q % 256 and q > 256 for q in quads.values()) and 1 in quads.values()
    assert any(any((16 * j) // (s[1] * s[2]) != min(16 * j + 15, q - 1) // (s[1] * s[2]) for j in range(SC.ceil_div(q, 16))) for s, q in quads.items())
    nbh = {s: SC.neighbourhood(SC.t_layer(s)) for s in mfma}
    assert sum(1 for v in nbh.values() if (v[1], v[3]) == (4, 4)) == 2
    for s, v in nbh.items():                                 # each is off the LDS variant for the reason its row names
        assert (v[1] > 3 and v[3] > 3) or (2 * s[2] * s[4]) % 4 != 0, (s, v)
    # ... and the VALU cases: a block count above one with a ragged last block, images that end inside a block
    assert any(s[0] * s[1] * s[2] > 512 and (s[0] * s[1] * s[2]) % 256 and 256 % (s[1] * s[2]) for w_, s, _ in SC.TRANSPOSED if w_ == SC.SMALLN_T)

    for want, shape in SC.FORWARD:
        for e in SC.FWD_EPILOGUES:
            assert SC.predict(*SC.f_call(shape, e)).kernel == want, (shape, e)
    print("forward: " + ", ".join(f"{w_} {SC.tshape_id(s)}" for w_, s in SC.FORWARD))


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("shape", T_SHAPES, ids=SC.tshape_id)
def test_reference_is_the_adjoint_of_the_oracle_conv(shape):
    """transposed64 (the oracle's deconv2d in float64) against float64 autograd of the oracle's conv2d with the same weights viewed as
    [k,k,N,Cs], and the float64 epilogues against torch's own functions; then the float32 oracle's error against it, per epilogue."""
    B, Hs, Ws, Cs, N, k = shape
    inp = SC.t_inputs(shape)
    lin_x, lin_dy = SC.t_reference(shape)
    xb = torch.zeros((B, 2 * Hs, 2 * Ws, N), dtype=torch.float64, requires_grad=True)
    (R.conv2d(xb, inp.w.double(), torch.zeros(Cs, dtype=torch.float64), 2, 2) * inp.dy.double()).sum().backward()
    assert float((xb.grad - lin_dy).abs().max()) <= 1e-12 * float(lin_dy.abs().max())
    # the forward applies the same operator A^T to x: the adjoint identity <A^T x, g> = <x, A g> at one more point
    g = inp.aux_tanh.double()
    lhs = float((lin_x * g).sum())
    rhs = float((R.conv2d(g, inp.w.double(), torch.zeros(Cs, dtype=torch.float64), 2, 2) * inp.x.double()).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, float(lin_x.abs().max()) * g.numel() ** 0.5)
    assert float(inp.aux_sign.abs().min()) >= SC.AUX_MARGIN and inp.aux_sign.shape == lin_dy.shape
    assert bool((inp.aux_sign > 0).any()) and bool((inp.aux_sign < 0).any())

    v = lin_x + inp.bias.double()
    F = torch.nn.functional
    assert torch.equal(SC.fwd_epilogue64(lin_x, inp.bias, SC.EPI_NONE), v) and torch.equal(SC.fwd_epilogue64(lin_x, None, SC.EPI_NONE), lin_x)
    assert float((SC.fwd_epilogue64(lin_x, inp.bias, SC.EPI_LRELU) - F.leaky_relu(v, 0.2)).abs().max()) <= 1e-15 * float(v.abs().max())
    assert torch.equal(SC.fwd_epilogue64(lin_x, inp.bias, SC.EPI_TANH), v.tanh())
    assert torch.equal(SC.fwd_epilogue64(lin_x, inp.bias, SC.EPI_AFFINE_RELU, inp.a, inp.b), F.relu(inp.a.double() * v + inp.b.double()))
    # the backward epilogues are the gradients of those activations at the saved output: autograd through them
    u = lin_dy
    pre = inp.aux_sign.double().requires_grad_(True)
    (F.leaky_relu(pre, 0.2) * u).sum().backward()
    assert float((pre.grad - SC.bwd_epilogue64(lin_dy, SC.EPI_LRELU_BWD, aux=inp.aux_sign)).abs().max()) <= 1e-15 * float(u.abs().max())
    pre = inp.aux_sign.double().requires_grad_(True)             # relu(a x + b) seen from x, at a point where a x + b has the sign of aux
    (F.relu(inp.a.double() * pre) * u).sum().backward()
    assert float((pre.grad - SC.bwd_epilogue64(lin_dy, SC.EPI_RELU_BWD_AFFINE, a=inp.a, aux=inp.aux_sign)).abs().max()) <= 1e-15 * float(u.abs().max() * inp.a.max())
    pre = torch.atanh(inp.aux_tanh.double()).requires_grad_(True)
    (torch.tanh(pre) * u).sum().backward()
    assert float((pre.grad - SC.bwd_epilogue64(lin_dy, SC.EPI_TANH_BWD, aux=inp.aux_tanh)).abs().max()) <= 1e-12 * float(u.abs().max())

    # the float32 oracle, normalised as the GPU test normalises the device
    zeros = torch.zeros(N)
    with torch.no_grad():
        o_x = R.deconv2d(inp.x, inp.w, inp.bias, (B, 2 * Hs, 2 * Ws, N), 2, 2)
        o_dy = R.deconv2d(inp.dy, inp.w, zeros, (B, 2 * Hs, 2 * Ws, N), 2, 2)
    figs = {"none": _rel(o_x, v), "lrelu": _rel(R.lrelu(o_x), SC.fwd_epilogue64(lin_x, inp.bias, SC.EPI_LRELU)),
            "tanh": _rel(torch.tanh(o_x), v.tanh()),
            "affine_relu": _rel(torch.relu(inp.a * o_x + inp.b), SC.fwd_epilogue64(lin_x, inp.bias, SC.EPI_AFFINE_RELU, inp.a, inp.b)),
            "bwd none": _rel(o_dy, lin_dy),
            "relu_bwd_affine": _rel(torch.where(inp.aux_sign > 0, o_dy * inp.a, torch.zeros_like(o_dy)),
                                    SC.bwd_epilogue64(lin_dy, SC.EPI_RELU_BWD_AFFINE, a=inp.a, aux=inp.aux_sign)),
            "lrelu_bwd": _rel(o_dy * torch.where(inp.aux_sign > 0, 1.0, 0.2), SC.bwd_epilogue64(lin_dy, SC.EPI_LRELU_BWD, aux=inp.aux_sign)),
            "tanh_bwd": _rel(o_dy * (1 - inp.aux_tanh * inp.aux_tanh), SC.bwd_epilogue64(lin_dy, SC.EPI_TANH_BWD, aux=inp.aux_tanh))}
    worst = max(figs.values())
    share = max(f / SC.bar(k, Cs, SC.EPI_TANH if name == "tanh" else SC.EPI_NONE) for name, f in figs.items())
    print(f"oracle {SC.tshape_id(shape)}: " + "  ".join(f"{name} {f:.2e}" for name, f in figs.items()) + f"  | worst {worst:.2e} = {share:.3f} of the bar")
    assert worst <= ORACLE_SLACK * SC.ORACLE_T_WORST and share <= ORACLE_SLACK * SC.ORACLE_T_OF_BAR
    assert ORACLE_SLACK * SC.ORACLE_T_OF_BAR < 1.0 and 0.05 < float(v.abs().median()) < 2.0          # (sums of order one: the tanh is not saturated)


@pytest.mark.parametrize("shape", [s for _, s in SC.FORWARD], ids=SC.tshape_id)
def test_forward_reference_and_oracle(shape):
    """The forward cases: float64 ops_ref.conv2d against the direct-loop definition (with the case's kernel, stride and channels), and the float32 oracle's error."""
    B, H, W, Cin, Cout, k, s = shape
    inp = SC.f_inputs(shape)
    lin = SC.f_reference(shape)
    crop = inp.x[:1, :min(H, 8 * s), :min(W, 8 * s)].double()        # (the loops are slow: the operator on a corner of the case's input)
    loops = R.conv2d_loops(crop.numpy(), inp.w.double().numpy(), np.zeros(Cout), s)
    small = R.conv2d(crop, inp.w.double(), torch.zeros(Cout, dtype=torch.float64), s, s)
    assert loops.shape == tuple(small.shape) and np.abs(loops - small.numpy()).max() <= 1e-12 * float(small.abs().max())
    with torch.no_grad():
        o = R.conv2d(inp.x, inp.w, inp.bias, s, s)
    v = lin + inp.bias.double()
    figs = {"none": _rel(o, v), "lrelu": _rel(R.lrelu(o), SC.fwd_epilogue64(lin, inp.bias, SC.EPI_LRELU)), "tanh": _rel(torch.tanh(o), v.tanh())}
    share = max(f / SC.bar(k, Cin, SC.EPI_TANH if name == "tanh" else SC.EPI_NONE) for name, f in figs.items())
    print(f"oracle forward {SC.tshape_id(shape)}: " + "  ".join(f"{name} {f:.2e}" for name, f in figs.items()) + f"  | {share:.3f} of the bar")
    assert max(figs.values()) <= ORACLE_SLACK * SC.ORACLE_F_WORST and share <= ORACLE_SLACK * SC.ORACLE_F_OF_BAR < 1.0
