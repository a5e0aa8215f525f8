"""The kernels that TRAIN the discriminator (the shaping step of shaping.DShaper: csrc/wgrad.hip, the column sums and parameter
gradients of csrc/bn.hip, the loss kernels of csrc/elementwise.hip), one by one against a float64 restatement computed on the CPU from
the same float32 inputs: torch autograd on oracle/ops_ref.py in ``.double()``, or the closed formula.

Where a bar is not one the suite already uses for the operation (the file is named beside it), it is 4x the error a float32 torch-CPU
evaluation of the same formula shows against float64 on the same inputs; the measured figure stands beside the bar."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N
from oracle import ops_ref as R
from wgrad_plan import SPLIT_CAP, lib_splits, wgrad_plan


@pytest.fixture(autouse=True)
def _plain_cpu_convolutions():
    """The checker's convolutions run on torch-CPU's native kernels (see tests/test_gpu_fuzz.py: oneDNN's backward corrupts the heap
    on some degenerate shapes, and 1x1 kernels with one channel are among the cases here)."""
    with torch.backends.mkldnn.flags(enabled=False):
        yield


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def close(got, want, tol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: inf / NaN in the result"
    err = (got - want).abs().max().item()
    ref = want.abs().max().item() + 1e-30
    print(f"{what} max|delta|={err:.3e} max|ref|={ref:.3e} ratio={err / ref:.3e} bar={tol:.3e}")
    assert err <= tol * ref, f"{what}: max|delta|={err:.3e} vs max|ref|={ref:.3e} (bar {tol:.1e})"


def wtol(M):
    """The suite's bars for a weight gradient, relative to max|ref|: 3e-5 up to 1000 reduced pixels (tests/test_gpu_shaping.py), then the
    growth rule 2e-5 * sqrt(M / 1000) (tests/test_gpu_fuzz.py)."""
    return 3e-5 if M <= 1000 else 2e-5 * math.sqrt(M / 1000.0)


def coltol(M):
    """Column sums (bias gradient): tests/test_gpu_fuzz.py."""
    return 1e-5 * max(1.0, math.sqrt(M / 1000.0))


# ================================================================================================ weight gradients
def wgrad_ref(x, dy, kh, kw, sh, sw):
    """float64 autograd of the oracle's conv w.r.t. its filter."""
    w = torch.zeros((kh, kw, x.shape[3], dy.shape[3]), dtype=torch.float64, requires_grad=True)
    y = R.conv2d(x.double(), w, None, sh, sw)
    assert tuple(y.shape) == tuple(dy.shape)
    (y * dy.double()).sum().backward()
    return w.grad


def wgrad_inputs(B, H, W, Cin, Cout, kh, kw, sh, sw):
    p = wgrad_plan(B, H, W, Cin, Cout, kh, kw, sh, sw)
    return rnd((B, H, W, Cin), 11), rnd((B, p.Ho, p.Wo, Cout), 12), p


def check_wgrad(B, H, W, Cin, Cout, kh, kw, sh, sw):
    """One shape: the planner restatement against the library, then the gradient written over a NaN-filled destination."""
    from cgs_amd import kernels as K, lib
    d = dev()
    x, dy, p = wgrad_inputs(B, H, W, Cin, Cout, kh, kw, sh, sw)
    assert lib_splits(lib.load(), B, H, W, Cin, Cout, kh, kw, sh, sw) == p.splits, p
    want = wgrad_ref(x, dy, kh, kw, sh, sw)
    out = torch.full((kh, kw, Cin, Cout), float("nan"), device=d)
    got = K.conv2d_bwd_weight(x.to(d), dy.to(d), kh, kw, sh, sw, out=out)
    assert got is out
    close(got, want, wtol(p.M), f"wgrad {(B, H, W, Cin, Cout, kh, kw, sh, sw)} splits={p.splits}x{p.m_per_split}")      # (NaN left = an element skipped)
    return p


NONSQUARE = [(kh, kw, sh, sw, H, W) for (kh, kw) in [(3, 5), (5, 3), (1, 4), (4, 1)] for (sh, sw) in [(1, 2), (2, 1), (2, 2), (1, 1)]
             for (H, W) in [(7, 9), (9, 4), (1, 13)]]


@pytest.mark.parametrize("kh,kw,sh,sw,H,W", NONSQUARE)
def test_wgrad_nonsquare_kernels_strides_and_images(kh, kw, sh, sw, H, W):
    """Per-axis kernel, stride and padding: pt != pl and different bottom / right pads."""
    i = NONSQUARE.index((kh, kw, sh, sw, H, W))
    Cin, Cout = [(3, 5), (8, 12), (5, 8), (4, 3)][i % 4]             # the four (Cin % 4, Cout % 4) load-path combinations
    check_wgrad(3, H, W, Cin, Cout, kh, kw, sh, sw)


def test_wgrad_nonsquare_cases_do_have_unequal_pads():
    pads = {(wgrad_plan(3, H, W, 4, 4, kh, kw, sh, sw).pt, wgrad_plan(3, H, W, 4, 4, kh, kw, sh, sw).pl) for kh, kw, sh, sw, H, W in NONSQUARE}
    assert any(pt != pl for pt, pl in pads) and any(pt > pl for pt, pl in pads) and any(pt < pl for pt, pl in pads)


EDGE_K = [(1, 127), (1, 128), (1, 129), (1, 130), (1, 257), (3, 1), (3, 3), (3, 43)]       # (k, Cin): kh*kw*Cin = 127 .. 257, 9, 27, 387
EDGE_COUT = [1, 3, 4, 127, 128, 129, 130]


@pytest.mark.parametrize("Cout", EDGE_COUT)
@pytest.mark.parametrize("k,Cin", EDGE_K)
def test_wgrad_tile_and_vector_edges(k, Cin, Cout):
    """Channel counts at the 128-wide tile edge and on / off the 16-byte load paths of both operands."""
    check_wgrad(2, 5, 6, Cin, Cout, k, k, 1 if k == 1 else 2, 1)


def test_wgrad_edge_cases_reach_all_four_load_paths():
    combos = {(Cin % 4 == 0, Cout % 4 == 0) for _, Cin in EDGE_K for Cout in EDGE_COUT}
    assert len(combos) == 4


# (B, H, W, Cin, Cout, k, s) and what the plan must be there: (splits, m_per_split, pixels in the last slab)
SPLIT_CASES = [
    ((1, 3, 5, 8, 16, 3, 1), (1, 32, 15)),               # M = 15: less than one 32-pixel step
    ((2, 32, 32, 8, 16, 3, 1), (16, 128, 128)),          # M = 2048 = 16 * m_per_split exactly
    ((3, 1, 683, 8, 16, 3, 1), (17, 128, 1)),            # M = 2049: one pixel in the last slab
    ((33, 16, 16, 8, 16, 3, 1), (66, 128, 128)),         # M = 256 * 33: "four steps a block" holds the count at 66, not 256
    ((43, 16, 48, 4, 8, 3, 1), (207, 160, 64)),          # M = 256 * 129: 129 rounds up to 160 pixels -> 207 slabs, the last one short
    ((64, 64, 64, 3, 64, 5, 2), (256, 256, 256)),        # dcgan64's first layer: M = 65536, the cap
    ((8, 64, 64, 4, 32, 3, 1), (256, 128, 128)),         # stride 1, M = 32768, the cap
]


@pytest.mark.parametrize("shape,plan", SPLIT_CASES)
def test_wgrad_reduction_split(shape, plan):
    B, H, W, Cin, Cout, k, s = shape
    p = wgrad_plan(B, H, W, Cin, Cout, k, k, s, s)
    assert p.tiles == 1
    assert (p.splits, p.m_per_split, p.M - (p.splits - 1) * p.m_per_split) == plan, p
    if plan[0] == SPLIT_CAP:
        assert p.M >= 256 * 128
    check_wgrad(B, H, W, Cin, Cout, k, k, s, s)


@pytest.mark.parametrize("shape", [(3, 9, 4, 5, 3, 3, 5, 2, 1), (2, 5, 6, 128, 130, 1, 1, 1, 1), (43, 16, 48, 4, 8, 3, 3, 1, 1)])
def test_wgrad_accumulates_onto_unrelated_contents(shape):
    from cgs_amd import kernels as K
    d = dev()
    B, H, W, Cin, Cout, kh, kw, sh, sw = shape
    x, dy, p = wgrad_inputs(*shape)
    want = wgrad_ref(x, dy, kh, kw, sh, sw)
    old = rnd((kh, kw, Cin, Cout), 13, float(want.abs().max()))
    got = K.conv2d_bwd_weight(x.to(d), dy.to(d), kh, kw, sh, sw, out=old.to(d), accumulate=True)
    # old + gradient: one more float32 addition of two numbers of the gradient's size on top of the gradient's own bar
    close(got, old.double() + want, wtol(p.M), f"wgrad accumulate {shape}")
    assert not torch.equal(got.cpu(), old)


@pytest.mark.parametrize("shape", [(64, 64, 64, 3, 64, 5, 5, 2, 2), (1, 3, 5, 8, 16, 3, 3, 1, 1), (3, 7, 9, 3, 5, 3, 5, 1, 2)])
def test_wgrad_is_bit_reproducible(shape):
    """The slabs are added in a fixed order (csrc/wgrad.hip header): two runs on fresh outputs are bit-equal."""
    from cgs_amd import kernels as K
    d = dev()
    B, H, W, Cin, Cout, kh, kw, sh, sw = shape
    x, dy, _ = wgrad_inputs(*shape)
    xd, dyd = x.to(d), dy.to(d)
    a = K.conv2d_bwd_weight(xd, dyd, kh, kw, sh, sw, out=torch.full((kh, kw, Cin, Cout), 7.0, device=d))
    b = K.conv2d_bwd_weight(xd, dyd, kh, kw, sh, sw, out=torch.full((kh, kw, Cin, Cout), -3.0, device=d))
    assert torch.equal(a, b)


def test_wgrad_refuses_a_short_workspace_without_launching():
    from cgs_amd import lib
    l = lib.load()
    d = dev()
    B, H, W, Cin, Cout, k, s = 2, 8, 8, 8, 16, 3, 2
    x, dy, p = wgrad_inputs(B, H, W, Cin, Cout, k, k, s, s)
    xd, dyd = x.to(d), dy.to(d)
    need = int(l.cgs_conv_wgrad_ws_bytes(B, H, W, Cin, Cout, k, k, s, s))
    ws = torch.zeros(need // 4 + 4, device=d)
    stream = torch.cuda.current_stream().cuda_stream
    dw = torch.full((k, k, Cin, Cout), 5.0, device=d)
    rc = l.cgs_conv2d_nhwc_bwd_weight(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), B, H, W, Cin, Cout, k, k, s, s, 0, ws.data_ptr(), need - 1, stream)
    assert rc == lib.EWORKSPACE and "conv2d_nhwc_bwd_weight" in l.cgs_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), torch.full((k, k, Cin, Cout), 5.0)) and float(ws.abs().max()) == 0.0      # nothing ran
    # the linear form, and a null workspace
    xl, dl = rnd((5, 40), 1).to(d), rnd((5, 12), 2).to(d)
    need_l = int(l.cgs_conv_wgrad_ws_bytes(5, 1, 1, 40, 12, 1, 1, 1, 1))
    dwl = torch.full((40, 12), 5.0, device=d)
    rc = l.cgs_linear_bwd_weight(xl.data_ptr(), dl.data_ptr(), dwl.data_ptr(), 5, 40, 12, 0, ws.data_ptr(), need_l - 1, stream)
    assert rc == lib.EWORKSPACE and "linear_bwd_weight" in l.cgs_last_error().decode()
    rc = l.cgs_linear_bwd_weight(xl.data_ptr(), dl.data_ptr(), dwl.data_ptr(), 5, 40, 12, 0, None, need_l, stream)
    assert rc == lib.EWORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(dwl.cpu(), torch.full((40, 12), 5.0))
    # the exact size is enough
    assert l.cgs_conv2d_nhwc_bwd_weight(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), B, H, W, Cin, Cout, k, k, s, s, 0, ws.data_ptr(), need, stream) == lib.OK
    close(dw, wgrad_ref(x, dy, k, k, s, s), wtol(p.M), "wgrad exact workspace")


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("Nout", [1, 3, 40, 129])
@pytest.mark.parametrize("B", [1, 5, 33, 1024])
def test_linear_weight_grad(B, Nout, accumulate):
    from cgs_amd import kernels as K
    d = dev()
    Kin = 100 if Nout != 40 else 131
    x, dy = rnd((B, Kin), 21), rnd((B, Nout), 22)
    want = x.double().t() @ dy.double()
    old = rnd((Kin, Nout), 23, float(want.abs().max())) if accumulate else torch.full((Kin, Nout), float("nan"))
    got = K.linear_bwd_weight(x.to(d), dy.to(d), out=old.to(d), accumulate=accumulate)
    close(got, old.double() + want if accumulate else want, wtol(B), f"linear wgrad B={B} {Kin}->{Nout} acc={accumulate}")


# ================================================================================================ bias gradient
@pytest.mark.parametrize("mode", ["fresh", "accumulate", "over_nan"])
@pytest.mark.parametrize("M,C", [(1, 4), (7, 64), (640, 68), (65536, 64), (4096, 512), (33, 1), (640, 3)])
def test_bias_grad(M, C, mode):
    """C % 4 == 0: the two-stage column sum of csrc/bn.hip; C in {1, 3}: the wrapper's own sum for the one-logit head."""
    from cgs_amd import kernels as K
    d = dev()
    dy = rnd((M, C), 31)
    want = dy.double().sum(0)
    if mode == "fresh":
        got = K.bias_grad(dy.to(d))
    elif mode == "accumulate":
        old = rnd((C,), 32, float(want.abs().max()))
        got = K.bias_grad(dy.to(d), out=old.to(d), accumulate=True)
        want = want + old.double()
    else:
        got = K.bias_grad(dy.to(d), out=torch.full((C,), float("nan"), device=d))
    close(got, want, coltol(M), f"bias_grad {M}x{C} {mode}")


def test_bias_grad_of_a_4d_tensor_sums_every_axis_but_the_last():
    from cgs_amd import kernels as K
    dy = rnd((3, 5, 7, 8), 33)
    close(K.bias_grad(dy.to(dev())), dy.double().sum((0, 1, 2)), coltol(105), "bias_grad 4-D")


# ================================================================================================ batch norm parameter gradients
NORM_SMALL_MAX_ROWS = 128          # csrc/bn.hip: 16 row lanes x NS_ROWS = 8 rows; above it the three-kernel form runs
KINK_MARGIN = 1e-5                 # min|z| > 1e-5 * max|z|: ~100 float32 roundings between every pre-activation and the lrelu kink

# seed of x for every (M, C) at leak 0.2, chosen (on the CPU) so that no pre-activation lies within KINK_MARGIN of the kink;
# the test asserts it before the device is called
BN_SEEDS = {(2, 4): 40, (2, 64): 40, (2, 68): 40, (2, 512): 40, (128, 4): 40, (128, 64): 40, (128, 68): 40, (128, 512): 253,
            (129, 4): 40, (129, 64): 40, (129, 68): 42, (129, 512): 48}


def bn_inputs(M, C, seed):
    x = rnd((M, C), seed) * 1.3 + 0.4
    if M == 2:       # two rows: keep them apart (|x0 - x1| >= 1), or a channel's variance falls to the size of eps and invstd is ill-conditioned
        gap = rnd((C,), seed + 1)
        x[1] = x[0] + torch.where(gap >= 0, 1.0 + gap, gap - 1.0)
    gamma, beta, dy = rnd((C,), 42).abs() + 0.5, rnd((C,), 43, 0.3), rnd((M, C), 44)
    return x, gamma, beta, dy


def bn_ref(x, gamma, beta, dy, leak):
    xd, g, b = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = R.bn_train(xd, g, b)
    (R.lrelu(z, leak) * dy.double()).sum().backward()
    return z.detach(), xd.grad, g.grad, b.grad


def kink_clear(z):
    return float(z.abs().min()) > KINK_MARGIN * float(z.abs().max())


def bn_dx_tol(M):
    """2e-4: tests/test_gpu_fuzz.py::test_bn_random_shapes.  Two rows: xhat = +-1 and dx is a difference of nearly equal numbers;
    float32 torch-CPU autograd of the same expression is 9.6e-3 of max|ref| from float64 on these inputs (C = 512) -> 4x that."""
    return 2e-4 if M > 2 else 4 * 9.6e-3


def bn_param_tols(M):
    """dbeta is a column sum of dy' (the bias gradient's bar, tests/test_gpu_fuzz.py); dgamma a sum over the M rows of products with xhat,
    itself formed from the float32 mean / invstd (the weight gradient's bar: 2e-5, growing with sqrt(M / 1000) -- tests/test_gpu_shaping.py
    holds every gradient of the step, gamma and beta included, to 2e-5)."""
    grow = max(1.0, math.sqrt(M / 1000.0))
    return 2e-5 * grow, 1e-5 * grow


BN_SHAPES = [(M, C) for M in (2, NORM_SMALL_MAX_ROWS, NORM_SMALL_MAX_ROWS + 1) for C in (4, 64, 68, 512)]


def run_bn_pair(M, C, leak, accumulate, seed, then=None):
    from cgs_amd import kernels as K
    d = dev()
    x, gamma, beta, dy = bn_inputs(M, C, seed)
    z, dx_ref, dg_ref, db_ref = bn_ref(x, gamma, beta, dy, leak)
    if leak != 1.0:
        assert x.numel() <= 2 ** 18
        assert kink_clear(z), f"seed {seed} puts a pre-activation of ({M}, {C}) within {KINK_MARGIN} of the lrelu kink: pick another"
    xd, gd, bd = x.to(d), gamma.to(d), beta.to(d)
    _, mean, invstd = K.bn_train_lrelu_fwd(xd, gd, bd, leak)
    scale = float(max(dg_ref.abs().max(), db_ref.abs().max()))
    old_g, old_b = rnd((C,), 45, scale), rnd((C,), 46, scale)
    if accumulate:
        dgamma, dbeta = old_g.to(d), old_b.to(d)
        dg_ref, db_ref = dg_ref + old_g.double(), db_ref + old_b.double()
    else:
        dgamma, dbeta = torch.full((C,), float("nan"), device=d), torch.full((C,), float("nan"), device=d)
    dx = K.bn_train_lrelu_bwd_data(dy.to(d), xd, gd, bd, mean, invstd, leak)
    K.bn_train_param_grads(xd, dgamma, dbeta, accumulate)
    extra = then() if then is not None else None
    tg, tb = bn_param_tols(M)
    close(dx, dx_ref, bn_dx_tol(M), f"bn dx {M}x{C} leak={leak}")
    close(dgamma, dg_ref, tg, f"bn dgamma {M}x{C} leak={leak} acc={accumulate}")
    close(dbeta, db_ref, tb, f"bn dbeta {M}x{C} leak={leak} acc={accumulate}")
    return extra


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("leak", [0.2, 1.0])
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_param_grads(M, C, leak, accumulate):
    """Both producers of the statistics bn_train_param_grads reads: the one-launch form (M <= 128) and the three-kernel form."""
    run_bn_pair(M, C, leak, accumulate, BN_SEEDS[(M, C)])


@pytest.mark.parametrize("accumulate", [False, True])
def test_bn_param_grads_many_rows(accumulate):
    """M = 65536 rows (every stage-1 block busy); no lrelu, so no pre-activation can change sides."""
    run_bn_pair(65536, 64, 1.0, accumulate, 40)


@pytest.mark.parametrize("M", [NORM_SMALL_MAX_ROWS, NORM_SMALL_MAX_ROWS + 1])
def test_bn_param_grads_survive_a_bias_grad_of_the_same_width(M):
    """DShaper's order: the bias gradient of the layer below runs right after bn_train_param_grads and shares the workspace keyed by C."""
    from cgs_amd import kernels as K
    C = 64
    other = rnd((300, C), 47)

    def then():
        return K.bias_grad(other.to(dev()))
    db = run_bn_pair(M, C, 0.2, False, BN_SEEDS[(M, C)], then)
    close(db, other.double().sum(0), coltol(300), "bias_grad after the bn pair")


# ================================================================================================ loss kernels
PLANTED = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]


def planted_logits(n, seed, huge=True):
    """N(0, 3) with the edge values planted (as many as fit, starting at a seed-dependent one)."""
    l = rnd((n,), seed, 3.0)
    vals = PLANTED if huge else PLANTED[:-2]
    k = seed % len(vals)
    vals = (vals[k:] + vals[:k])[:n]
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))[:len(vals)]
    l[pos] = torch.tensor(vals, dtype=torch.float32)
    return l


def bce_terms64(l, t):
    l = l.double()
    return torch.clamp(l, min=0) - l * t + torch.log1p(torch.exp(-l.abs()))


# float32 torch-CPU evaluation of sum(max(l,0) - l*t + log1p(exp(-|l|))) against float64 on these inputs (n up to 100003, the +-1e4 plants
# included), summed in the kernel's order (256 strided partial sums, then the tree): at most 2.4e-7 relative -- below the 1e-5 bar, which therefore stands.
BCE_LOSS_TOL = 1e-5


@pytest.mark.parametrize("with_loss", [True, False])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 8192, 100003])
def test_bce_logits_grad(n, target, mean, with_loss):
    from cgs_amd import kernels as K
    d = dev()
    scale = 1.0 / n if mean else 1.0
    l = planted_logits(n, 50 + n % 97 + int(target * 10))
    t = float(np.float32(target))                       # the entry point takes a float: 0.9 is its float32 neighbour
    s = float(np.float32(scale))
    want = s * (torch.sigmoid(l.double()) - t)
    loss = torch.full((1,), float("nan"), device=d) if with_loss else None
    dl = torch.full((n,), float("nan"), device=d)
    got = K.bce_logits_grad(l.to(d), target, scale, dl, loss)
    assert got is dl
    got = got.cpu().double()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"bce_logits_grad n={n} t={target} scale={scale:.3e}: max|delta|={err:.3e} bar={1e-6 * s:.3e}")
    assert err <= 1e-6 * s, (err, 1e-6 * s, int((got - want).abs().argmax()))
    if with_loss:
        want_loss = s * float(bce_terms64(l, t).sum())
        got_loss = float(loss.cpu()[0])
        assert math.isfinite(got_loss)
        print(f"  loss {got_loss!r} vs {want_loss!r}: rel {abs(got_loss - want_loss) / abs(want_loss):.3e}")
        assert abs(got_loss - want_loss) <= BCE_LOSS_TOL * abs(want_loss)


@pytest.mark.parametrize("huge", [True, False])
@pytest.mark.parametrize("n", [1, 255, 257, 1 << 20])
def test_bce_ones_fwd_and_bwd(n, huge):
    """softplus(-l) and dy * (sigmoid(l) - 1); 1e-6 of max|ref| as tests/test_gpu_ops.py::test_elementwise_and_fold holds their
    neighbours.  Once with the +-1e4 plants (max|ref| = 1e4) and once without (max|ref| ~ 104), so the bar also binds the small values."""
    from cgs_amd import kernels as K
    d = dev()
    l = planted_logits(n, 60 + n % 13, huge)
    dy = rnd((n,), 61)
    ld = l.to(d)
    close(K.bce_ones_fwd(ld, out=torch.full((n,), float("nan"), device=d)), torch.nn.functional.softplus(-l.double()), 1e-6, f"bce_ones_fwd n={n}")
    close(K.bce_ones_bwd(dy.to(d), ld, out=torch.full((n,), float("nan"), device=d)), -dy.double() * torch.sigmoid(-l.double()), 1e-6,
          f"bce_ones_bwd n={n}")


@pytest.mark.parametrize("C", [1, 3, 12, 64])
@pytest.mark.parametrize("n", [1, 255, 257, 1 << 20])
def test_affine_fwd_and_bwd(n, C):
    from cgs_amd import kernels as K
    d = dev()
    M = max(1, n // C)
    x = planted_logits(M * C, 70 + C).reshape(M, C)
    a, b, dy = rnd((C,), 71), rnd((C,), 72), rnd((M, C), 73)
    close(K.affine_fwd(x.to(d), a.to(d), b.to(d), out=torch.full((M, C), float("nan"), device=d)), a.double() * x.double() + b.double(), 1e-6,
          f"affine_fwd {M}x{C}")
    close(K.affine_bwd(dy.to(d), a.to(d), out=torch.full((M, C), float("nan"), device=d)), dy.double() * a.double(), 1e-6, f"affine_bwd {M}x{C}")


# ================================================================================================ Adam
BETA1, BETA2, EPS = 0.5, 0.999, 1e-8
# One step of float32 torch-CPU arithmetic against the float64 restatement below, on adam_inputs (n = 4096*256 + 3, 8 carried steps),
# in the three scales the test uses (adam_ref64): w 2.3e-7, m 6.0e-8, v 1.7e-7 (measured maxima over the steps) -> bars of 4x that.
ADAM_W_TOL, ADAM_M_TOL, ADAM_V_TOL = 4 * 2.3e-7, 4 * 6.0e-8, 4 * 1.7e-7
V_FLOOR = 1e-36          # below float32's normal range (1.2e-38) v has absolute, not relative, precision: the scale of v never falls under this


def lr_at(lr, t, b1=BETA1, b2=BETA2):
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)              # tf.train.AdamOptimizer


def adam_grad(n, step):
    """Fresh gradient of a step: magnitudes from 1e-6 to 10, an exact zero at every 7th element."""
    g = torch.Generator().manual_seed(900 + step)
    mag = 10.0 ** (torch.rand(n, generator=g) * 7.0 - 6.0)
    out = (torch.randn(n, generator=g) * mag).float()
    out[::7] = 0.0
    return out


def adam_ref64(w, g, m, v, lr_t, b1=BETA1, b2=BETA2, eps=EPS):
    """One float64 step from float32 state, with the constants formed as the kernel forms them: beta, eps and lr_t are float32 arguments and
    ``1 - beta`` is subtracted in float32 (float64(1 - 0.999) differs from float32(1.f - 0.999f) by 6e-5 relative).
    Returns (w, m, v) and the scales the three errors are measured in."""
    f = np.float32
    b1f, b2f = f(b1), f(b2)
    c1, c2 = float(f(1) - b1f), float(f(1) - b2f)
    w, g, m, v = w.double(), g.double(), m.double(), v.double()
    m1 = float(b1f) * m + c1 * g
    v1 = float(b2f) * v + c2 * g * g
    upd = float(f(lr_t)) * m1 / (v1.sqrt() + float(f(eps)))
    m_scale = float(b1f) * m.abs() + c1 * g.abs()                      # not |m1|: the two terms cancel
    return (w - upd, m1, v1), (w.abs() + upd.abs(), m_scale, v1 + V_FLOOR)


def adam_errors(got, ref, scales):
    """max over the elements of |got - ref| / scale, per tensor (a zero scale demands an exact zero)."""
    out = []
    for a, b, s in zip(got, ref, scales):
        a = a.detach().cpu().double()
        assert torch.isfinite(a).all()
        e = (a - b).abs()
        assert bool((e[s == 0] == 0).all())
        out.append(float((e[s > 0] / s[s > 0]).max()) if bool((s > 0).any()) else 0.0)
    return out


def check_adam_state(got, before, g, lr_t, what):
    ref, scales = adam_ref64(before[0], g, before[1], before[2], lr_t)
    ew, em, ev = adam_errors(got, ref, scales)
    print(f"{what}: w {ew:.3e} (bar {ADAM_W_TOL:.1e})  m {em:.3e} (bar {ADAM_M_TOL:.1e})  v {ev:.3e} (bar {ADAM_V_TOL:.1e})")
    assert ew <= ADAM_W_TOL and em <= ADAM_M_TOL and ev <= ADAM_V_TOL, (what, ew, em, ev)


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3, 6272 * 1024])
def test_adam_kernel_eight_carried_steps(n):
    """Every step from the device's own float32 state before it, so errors do not compound into the bars; m and v are read back."""
    from cgs_amd import kernels as K
    d = dev()
    w = rnd((n,), 80, 0.05).to(d)
    m, v = torch.zeros(n, device=d), torch.zeros(n, device=d)
    idle = torch.arange(0, n, 7)
    for t in range(1, 9):
        g = adam_grad(n, t) if n > 1 else adam_grad(8, t)[1:2]
        before = (w.cpu(), m.cpu(), v.cpu())
        lr_t = lr_at(1e-3, t)
        K.adam_step(w, g.to(d), m, v, lr_t, BETA1, BETA2, EPS)
        check_adam_state((w, m, v), before, g, lr_t, f"adam n={n} t={t}")
        if n > 1:       # g == 0, m == 0, v == 0: nothing moves, bit for bit
            assert torch.equal(w.cpu()[idle], before[0][idle]) and float(m.cpu()[idle].abs().max()) == 0.0 and float(v.cpu()[idle].abs().max()) == 0.0
    assert not torch.equal(m.cpu(), v.cpu())


def test_adam_zero_gradient_from_zero_state_leaves_w_alone():
    from cgs_amd import kernels as K
    d = dev()
    w0 = rnd((1000,), 81)
    w, m, v = w0.to(d), torch.zeros(1000, device=d), torch.zeros(1000, device=d)
    K.adam_step(w, torch.zeros(1000, device=d), m, v, lr_at(1e-3, 1), BETA1, BETA2, EPS)
    assert torch.equal(w.cpu(), w0) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


# ================================================================================================ DShaper over several steps
@pytest.mark.parametrize("arch,B", [("mnist", 16), ("dcgan32", 8)])
def test_dshaper_five_steps_follow_a_float64_shadow(arch, B):
    """Five calls of step(): after each, every parameter / m / v tensor is one float64 Adam step (with the step's own gradients and the
    lr_t of ITS count) from the device state before it, at the kernel-level bars; and a float64 shadow of (m, v) carried from zero through
    all five steps is followed within the bound those bars imply by induction: a step multiplies the distance E to the shadow by beta and adds
    at most bar * scale, where the device's scale is within beta * E of the shadow's -- E_t = beta * (1 + bar) * E_(t-1) + bar * scale_t.
    Catches a wrong t or lr_t, a slot paired with another tensor's moments, moments that are not carried."""
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device
    from cgs_amd.shaping import DShaper
    d = dev()
    lr = 1e-3
    Pd = to_device(N.init_params(arch, 2019, True), d)
    img = tuple(N.ARCHS[arch]["img"])
    eng_before = RefineEngine(arch, Pd, B, d)
    z = rnd((B, N.ARCHS[arch]["z_dim"]), 5).clamp(-1, 1).to(d)
    f0 = eng_before.input_to_feature(z).clone()
    l_start = eng_before.compute_forward_logits_and_grad(f0)[0].clone()
    sh = DShaper(arch, Pd, B, d, learning_rate=lr)
    assert sh.t == 0 and all(float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 for _, _, m, v in sh.slots)
    assert len({p.data_ptr() for p, _, _, _ in sh.slots}) == len(sh.slots)
    shadow = [(torch.zeros(p.shape, dtype=torch.float64), torch.zeros(p.shape, dtype=torch.float64)) for p, _, _, _ in sh.slots]
    bound = [(torch.zeros(p.shape, dtype=torch.float64), torch.zeros(p.shape, dtype=torch.float64)) for p, _, _, _ in sh.slots]
    for t in range(1, 6):
        real = rnd((B,) + img, 100 + t).clamp(-1, 1).to(d)
        fake = torch.tanh(rnd((B,) + img, 200 + t)).to(d)
        before = [(p.cpu(), m.cpu(), v.cpu()) for p, _, m, v in sh.slots]
        loss = sh.step(real, fake)
        assert math.isfinite(float(loss)) and sh.t == t
        lr_t = lr_at(lr, t)
        for i, ((p, g, m, v), bef) in enumerate(zip(sh.slots, before)):
            gc = g.cpu()                                     # the gradients the step used are still in place
            assert torch.isfinite(gc).all()
            check_adam_state((p, m, v), bef, gc, lr_t, f"{arch} step {t} slot {i} {tuple(p.shape)}")
            (_, m64, v64), (_, m_scale, _) = adam_ref64(torch.zeros_like(gc), gc, shadow[i][0], shadow[i][1], lr_t)
            shadow[i] = (m64, v64)
            em = (m.cpu().double() - m64).abs()
            ev = (v.cpu().double() - v64).abs()
            bound[i] = (float(np.float32(BETA1)) * (1 + ADAM_M_TOL) * bound[i][0] + ADAM_M_TOL * m_scale,
                        float(np.float32(BETA2)) * (1 + ADAM_V_TOL) * bound[i][1] + ADAM_V_TOL * (v64 + V_FLOOR))
            assert bool((em <= bound[i][0]).all()), (arch, t, i, "m left the carried shadow", float((em - bound[i][0]).max()))
            assert bool((ev <= bound[i][1]).all()), (arch, t, i, "v left the carried shadow", float((ev - bound[i][1]).max()))
    # the refiner built before the steps, refreshed, reads the same weights as one built after them
    eng_before.refresh_weights()
    l_refreshed = eng_before.compute_forward_logits_and_grad(f0)[0].clone()
    l_fresh = RefineEngine(arch, Pd, B, d).compute_forward_logits_and_grad(f0)[0].clone()
    assert torch.equal(l_refreshed, l_fresh) and not torch.equal(l_refreshed, l_start)
