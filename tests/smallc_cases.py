"""The small-channel convolution kernels, variant by variant: the dispatch restated in plain Python integers, a float64 reference with every
fused epilogue, seeded inputs, and the case tables two tests share (tests/test_smallc_cases_cpu.py checks the restatement against the
library's own ``cgs_conv_family``, the tables' coverage and the reference without a device; tests/test_gpu_smallc_variants.py holds the
kernels to them).  Not a test module and not a conftest: the tests import it by name.

    predict        ``choose_family`` (csrc/api.hip) and, inside the family, the launcher's choice of kernel (``cgs_convt_quad_launch``,
                   ``cgs_conv_patch_launch``, ...) for a call (op, B, H, W, Cin, Ho, Wo, Cout, k, s, epilogue) at the workspace
                   ``kernels._WsCache`` hands it, every pointer aligned, the exact-fp32 contraction: the family number, the exact string
                   ``cgs_last_kernel()`` reports (for the implicit GEMM: the prefix "igemm_kernel<", its internals are not restated) and,
                   for ``convt_quad_lds_kernel``, the tiles / per / blocks plan of its persistent launch
    transposed64   the TF-'SAME' stride-2 transposed convolution in float64: oracle.ops_ref.deconv2d on float64 copies of the float32
                   inputs -- which is also the backward-data of the conv2d with the same weights viewed as [k,k,N,Cs] (the CPU test
                   checks that against float64 autograd of ops_ref.conv2d)
    fwd_epilogue64, bwd_epilogue64   bias + none / lrelu 0.2 / tanh / relu(a v + b), and none / aux > 0 ? v a[c] : 0 / lrelu' / tanh'

The bar is the project's operator bar, unchanged (``ktol`` of tests/test_gpu_fuzz.py): max|delta| <= 2e-5 max(1, sqrt(k k Cs / 1000)) max|ref|,
times 1.5 under the forward tanh.  Its reference side, the float32 torch-CPU oracle against the float64 reference over these very tables
and normalised the same way, is ORACLE_T_WORST / ORACLE_F_WORST below (tests/test_smallc_cases_cpu.py prints every figure and asserts it inside the bar);
the device's figures stand in the docstring of tests/test_gpu_smallc_variants.py.
"""
import collections
import functools

import torch

from oracle import ops_ref as R

# include/cgs_hip.h, cgs_amd/lib.py
CONV_FWD, CONV_BWD_DATA, DECONV_FWD, DECONV_BWD_DATA = 0, 1, 2, 3
EPI_NONE, EPI_LRELU, EPI_AFFINE_RELU, EPI_TANH, EPI_RELU_BWD_AFFINE, EPI_LRELU_BWD, EPI_TANH_BWD = 0, 1, 2, 3, 4, 5, 6
FAMILY_IGEMM, FAMILY_QUAD, FAMILY_SMALLN_T, FAMILY_SMALLN_F, FAMILY_PATCH, FAMILY_TAPS, FAMILY_DOT = 0, 1, 2, 3, 4, 5, 6
EPI_NAMES = {EPI_NONE: "none", EPI_LRELU: "lrelu", EPI_AFFINE_RELU: "affine_relu", EPI_TANH: "tanh", EPI_RELU_BWD_AFFINE: "relu_bwd_affine",
             EPI_LRELU_BWD: "lrelu_bwd", EPI_TANH_BWD: "tanh_bwd"}
FWD_EPILOGUES = (EPI_NONE, EPI_LRELU, EPI_TANH)
BWD_EPILOGUES = (EPI_NONE, EPI_RELU_BWD_AFFINE, EPI_LRELU_BWD, EPI_TANH_BWD)

IGEMM_PREFIX = "igemm_kernel<"
SMALLN_T = "convt_smalln_kernel"
QUAD_MFMA = "convt_quad_mfma_kernel<4>"

# The float32 oracle's worst max|delta| / max|ref| against the float64 reference over every case and epilogue of a table, and its worst
# share of the bar (tests/test_smallc_cases_cpu.py prints every figure and asserts it against these): the reference side of the bar.
ORACLE_T_WORST, ORACLE_T_OF_BAR = 5.0e-7, 0.017       # 4.98e-7 at 1025x8x32x16x4x3 under the forward tanh
ORACLE_F_WORST, ORACLE_F_OF_BAR = 1.2e-6, 0.040       # 1.18e-6 at 2x256x256x16x2x3x1 under tanh

AUX_MARGIN = 1e-3       # no element of a sign-deciding aux tensor lies closer to zero

Layer = collections.namedtuple("Layer", "kh kw sh sw Hb Wb Cb Hs Ws Cs dirT")
TilePlan = collections.namedtuple("TilePlan", "TW TH tiles_per_image tiles per blocks last")
Prediction = collections.namedtuple("Prediction", "family kernel plan")


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


def same_pad_before(size, k, s):
    """TF 'SAME': the smaller half of the total padding goes in front (cgs_same_pad_before)."""
    return max((ceil_div(size, s) - 1) * s + k - size, 0) // 2


def layer_of(op, H, W, Cin, Ho, Wo, Cout, k, s):
    """conv_call_of (csrc/api.hip): the big tensor, the small tensor and the direction of the contraction."""
    dirT = op in (CONV_BWD_DATA, DECONV_FWD)
    if op in (CONV_FWD, CONV_BWD_DATA):
        return Layer(k, k, s, s, H, W, Cin, ceil_div(H, s), ceil_div(W, s), Cout, dirT)
    return Layer(k, k, s, s, Ho, Wo, Cout, H, W, Cin, dirT)


def quad_range(k, pad):
    """The input-pixel offsets d = (parity + pad - tap) / 2 that feed a 2-pixel output pair (convt_quad.hip) -> (lo, hi)."""
    ds = [(par + pad - kk) // 2 for par in (0, 1) for kk in range(k) if (par + pad - kk) % 2 == 0]
    return min(ds), max(ds)


def neighbourhood(L):
    """-> (dmin_y, ny, dmin_x, nx) of the quad forms."""
    ly, hy = quad_range(L.kh, same_pad_before(L.Hb, L.kh, 2))
    lx, hx = quad_range(L.kw, same_pad_before(L.Wb, L.kw, 2))
    return ly, hy - ly + 1, lx, hx - lx + 1


def smalln_ok(L, epilogue):
    return L.Cb <= 4 and L.sh == 2 and L.sw == 2 and L.Hb == 2 * L.Hs and L.Wb == 2 * L.Ws and L.Cs % 4 == 0 and epilogue != EPI_AFFINE_RELU


def quad_fits(L):
    _, ny, _, nx = neighbourhood(L)
    return ny * nx * L.Cs * 16 * 4 <= 150 * 1024


def convt_taps_ok(L):
    return L.Cb == 1 and L.kh == 4 and L.kw == 4 and L.sh == 2 and L.sw == 2 and L.Hb == 2 * L.Hs and L.Wb == 2 * L.Ws and L.Ws <= 16 and \
        L.Cs in (16, 32, 64, 128)


def rows_mt(L):
    if L.Cb not in (1, 3) or L.kw * L.Cb > 16 or L.kw > 6 or L.Cs % 16 or (2 * L.Ws * L.Cb) % 4:
        return 0
    if L.kh * L.Cs * 16 * 4 > 64 * 1024 or L.Ws > 32:
        return 0
    return 1 if L.Ws <= 16 else 2


def quad_kernel(L, B, epilogue):
    """cgs_convt_quad_launch: taps form, rows form, LDS-patch variant, global-load fallback -> (name, TilePlan or None)."""
    bwd = "true" if epilogue >= EPI_RELU_BWD_AFFINE else "false"
    if convt_taps_ok(L):
        return f"convt_taps_kernel<{L.Cs // 16}>", None
    dmin_y, ny, dmin_x, nx = neighbourhood(L)
    mt = rows_mt(L)
    if mt:
        s5 = L.kh == 5 and L.Cs == 64 and same_pad_before(L.Hb, L.kh, 2) == 1 and dmin_y == -1 and ny == 3
        tall = s5 and L.Cb == 3 and L.Hs >= 8 and epilogue < EPI_RELU_BWD_AFFINE
        return f"convt_rows_kernel<{L.Cb}, {mt}, {'true' if s5 and L.Cb == 3 else 'false'}, {4 if tall else 2}, {bwd}>", None
    need = ny * nx * L.Cs * 16 * 4
    if ny <= 3 and nx <= 3 and (2 * L.Ws * L.Cb) % 4 == 0:
        wide = L.Ws % 32 == 0 and L.Hs % 8 == 0
        TW = 32 if wide else 16
        TH = 256 // TW
        PH, PW = TH + ny - 1, TW + nx - 1
        if need + 2 * PH * PW * 16 * 4 <= 160 * 1024 and 4 * 256 * L.Cb <= 2 * PH * PW * 16:
            tpi = ceil_div(L.Hs, TH) * ceil_div(L.Ws, TW)
            tiles = B * tpi
            per = ceil_div(tiles, 512)
            if per < 4:
                per = 4 if tiles >= 4 * 256 else 1
            blocks = ceil_div(tiles, per)
            plan = TilePlan(TW, TH, tpi, tiles, per, blocks, tiles - (blocks - 1) * per)
            return f"convt_quad_lds_kernel<{L.Cb}, {TW}, {3 if ny == 3 and nx == 3 else 0}>", plan
    return QUAD_MFMA, None


# ---- the forward direction: only what the forward cases below need (the eligibility of every family in front of the implicit GEMM) ----
ST = 16                     # conv_smalln_f.hip: tile side
TR, TC, PBN = 8, 16, 64     # conv_patch.hip: output tile, channels per block


def ws_floats_fwd(L):
    """cgs_conv_ws_bytes / 4 of a forward conv whose output channels are no multiple of 64 -- a lower bound of what _WsCache offers."""
    return round_up(L.kh * L.kw * L.Cb, 32) * round_up(L.Cs, 64)


def conv_smalln_f_ok(L, B, epilogue):
    return B * (L.Hb // ST) * (L.Wb // ST) >= 512 and L.Cs <= 4 and L.sh == 1 and L.sw == 1 and L.Cb % 16 == 0 and L.Hb % ST == 0 and \
        L.Wb % ST == 0 and L.kh <= 7 and L.kw <= 7 and epilogue in (EPI_NONE, EPI_TANH, EPI_LRELU)


def conv_taps_ok(L):
    return L.Cb == 1 and L.kh == 4 and L.kw == 4 and L.sh == 2 and L.sw == 2 and L.Cs % 32 == 0 and L.Cs <= 128


def conv_dot_ok(L, epilogue):
    return L.Cs <= 4 and L.Cb % 4 == 0 and L.kh * L.kw * L.Cb >= 1024 and epilogue < EPI_RELU_BWD_AFFINE and L.sh == L.sw


def conv_patch_ok(L):
    return L.Cb <= 4 and L.sh == L.sw and L.sh in (1, 2) and L.Hs % TR == 0 and L.Ws % TC == 0 and L.Cs % 4 == 0 and \
        L.kh * L.kw * L.Cb <= 160 and L.kh <= 7 and L.kw <= 7 and (L.sh * (TR - 1) + L.kh) * (L.sh * (TC - 1) + L.kw) * L.Cb <= 10 * 256


def patch_kernel(L, epilogue):
    """cgs_conv_patch_launch, forward direction: the 5x5x3 stride-2 form, the two fixed geometries, the general form."""
    if L.sh == 2 and L.sw == 2 and L.kh == 5 and L.kw == 5 and L.Cb == 3:
        return f"conv_patch2_kernel<5, 16, 15, 8, {1 if epilogue >= EPI_RELU_BWD_AFFINE else 0}>"
    K, run, pitch = L.kh * L.kw * L.Cb, L.kw * L.Cb, (L.sh * (TC - 1) + L.kw) * L.Cb + 1
    if (K, run, pitch) == (147, 21, 67):
        return "conv_patch_kernel<147, 21, 67>"
    if (K, run, pitch) == (48, 12, 103):
        return "conv_patch_kernel<48, 12, 103>"
    return "conv_patch_kernel"


def predict(op, B, H, W, Cin, Ho, Wo, Cout, k, s, epilogue):
    """-> Prediction(family, kernel, plan): see the module docstring."""
    L = layer_of(op, H, W, Cin, Ho, Wo, Cout, k, s)
    if L.dirT:
        if smalln_ok(L, epilogue):
            if L.Cs % 16 == 0 and quad_fits(L):
                return Prediction(FAMILY_QUAD, *quad_kernel(L, B, epilogue))
            if epilogue < EPI_RELU_BWD_AFFINE:
                return Prediction(FAMILY_SMALLN_T, SMALLN_T, None)
        assert not (L.Cs <= 4 and L.sh == 1), "the transposed stride-1 patch form is not restated here"
        return Prediction(FAMILY_IGEMM, IGEMM_PREFIX, None)
    if conv_smalln_f_ok(L, B, epilogue) and ws_floats_fwd(L) >= L.kh * L.kw * L.Cb * L.Cs:
        return Prediction(FAMILY_SMALLN_F, "conv_smalln_f_kernel", None)
    if conv_taps_ok(L):
        return Prediction(FAMILY_TAPS, f"conv_taps_kernel<{L.Cs // 32}, {1 if epilogue >= EPI_RELU_BWD_AFFINE else 0}>", None)
    if conv_dot_ok(L, epilogue):
        return Prediction(FAMILY_DOT, f"conv_dot_kernel<{L.Cs}>", None)
    if conv_patch_ok(L) and ws_floats_fwd(L) >= round_up(L.kh * L.kw * L.Cb, 2) * round_up(L.Cs, PBN):
        return Prediction(FAMILY_PATCH, patch_kernel(L, epilogue), None)
    return Prediction(FAMILY_IGEMM, IGEMM_PREFIX, None)


def kernel_matches(pred, name):
    """The implicit GEMM is predicted by its prefix, every other kernel by its exact name."""
    return name.startswith(IGEMM_PREFIX) if pred.kernel == IGEMM_PREFIX else name == pred.kernel


def lib_family(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s, epilogue):
    """cgs_conv_family asked as kernels._WsCache.plan asks it: at the workspace size cgs_conv_ws_bytes_for gives.  No device needed."""
    nbytes = max(int(lib.cgs_conv_ws_bytes_for(op, B, H, W, Cin, Cout, k, k, s, s)), 16)
    return int(lib.cgs_conv_family(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, epilogue, nbytes))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# Transposed direction: (kernel the shape must reach, (B, Hs, Ws, Cs, N, k), what the shape is there for); stride 2, output 2Hs x 2Ws x N.
# Each runs as a deconv2d forward [B,Hs,Ws,Cs] -> [B,2Hs,2Ws,N] and as the backward-data of the conv2d with the same weights viewed as
# [k,k,N,Cs].  256 quads (input-resolution pixels) make a block of convt_smalln_kernel and of convt_quad_mfma_kernel<4>.
def _lds(n, tw, yx):
    return f"convt_quad_lds_kernel<{n}, {tw}, {yx}>"


TRANSPOSED = [
    (SMALLN_T, (2, 5, 7, 24, 1, 5), "N=1; Cs = 24: six float4 chunks, odd grid"),
    (SMALLN_T, (2, 5, 7, 24, 2, 5), "N=2, the same"),
    (SMALLN_T, (2, 5, 7, 24, 4, 5), "N=4, the same"),
    (SMALLN_T, (5, 9, 13, 20, 3, 5), "N=3; 585 quads: three blocks, the last ragged, images inside one block"),
    (SMALLN_T, (1, 3, 4, 12, 3, 4), "4x4 kernel"),
    (SMALLN_T, (3, 6, 5, 8, 2, 3), "3x3 kernel: 2x2 neighbourhood"),
    (SMALLN_T, (1, 4, 5, 160, 3, 7), "Cs % 16 == 0, but the quad image does not fit LDS"),
    (SMALLN_T, (2, 4, 4, 512, 3, 5), "the same with a 5x5 kernel"),
    (SMALLN_T, (3, 1, 1, 4, 4, 1), "one quad per image, 1x1 kernel"),
    (QUAD_MFMA, (2, 6, 7, 32, 3, 5), "odd Ws, N=3"),
    (QUAD_MFMA, (3, 5, 9, 16, 1, 5), "odd Ws, N=1"),
    (QUAD_MFMA, (2, 3, 5, 64, 1, 3), "odd Ws, N=1, 3x3 kernel"),
    (QUAD_MFMA, (2, 8, 8, 16, 2, 7), "k=7: 4x4 neighbourhood, N=2"),
    (QUAD_MFMA, (2, 4, 6, 48, 4, 7), "k=7, N=4: all 16 columns, three 16-channel chunks"),
    (QUAD_MFMA, (2, 9, 7, 16, 3, 1), "1x1 kernel"),
    (QUAD_MFMA, (5, 9, 7, 16, 3, 5), "315 quads: two blocks, last wave tiles ragged, tiles straddling images"),
    (QUAD_MFMA, (1, 1, 1, 16, 3, 5), "a single quad"),
    (_lds(1, 32, 3), (2, 8, 64, 16, 1, 5), "whole 8x32 tiles"),
    (_lds(1, 32, 0), (2, 8, 64, 16, 1, 3), "whole 8x32 tiles, run-time neighbourhood"),
    (_lds(1, 16, 3), (2, 6, 48, 16, 1, 5), "16x16 tiles clipped at the bottom"),
    (_lds(1, 16, 0), (2, 6, 48, 16, 1, 3), "the same, run-time neighbourhood"),
    (_lds(2, 32, 3), (2, 8, 32, 16, 2, 5), ""),
    (_lds(2, 32, 0), (2, 8, 32, 16, 2, 3), ""),
    (_lds(2, 16, 3), (2, 20, 36, 16, 2, 5), "tiles hanging over both edges"),
    (_lds(2, 16, 0), (2, 7, 9, 32, 2, 3), "odd grid; two chunks"),
    (_lds(2, 16, 0), (2, 7, 9, 32, 2, 2), "2x2 kernel: a 1x1 neighbourhood"),
    (_lds(3, 32, 3), (2, 16, 64, 16, 3, 5), "wider than the rows form takes"),
    (_lds(3, 32, 0), (2, 8, 64, 16, 3, 3), "the same"),
    (_lds(3, 16, 3), (2, 8, 40, 16, 3, 5), ""),
    (_lds(3, 16, 3), (2, 6, 10, 16, 3, 6), "kw N = 18 > 16 keeps a narrow layer off the rows form"),
    (_lds(3, 16, 0), (2, 9, 34, 16, 3, 3), ""),
    (_lds(4, 32, 3), (2, 8, 32, 32, 4, 4), ""),
    (_lds(4, 32, 0), (2, 8, 32, 16, 4, 3), ""),
    (_lds(4, 16, 3), (3, 20, 12, 32, 4, 5), ""),
    (_lds(4, 16, 0), (2, 5, 5, 16, 4, 3), ""),
    (_lds(4, 16, 0), (2, 5, 5, 16, 4, 1), "1x1 kernel: the staging tile fills the patch buffer exactly"),
    (_lds(2, 16, 3), (1027, 8, 8, 16, 2, 5), "persistent: 1027 one-tile images, 4 tiles per block, 257 blocks, the last 3 tiles"),
    (_lds(2, 16, 3), (171, 20, 36, 16, 2, 5), "persistent: 6 clipped tiles per image, 1026 tiles, runs cross images mid-run, the last 2 tiles"),
    (_lds(4, 32, 0), (1025, 8, 32, 16, 4, 3), "persistent: wide form, run-time neighbourhood, last block one tile"),
    (_lds(4, 32, 3), (130, 8, 32, 16, 4, 5), "not persistent: 130 tiles, one per block"),
]
PERSISTENT = [(1027, 8, 8, 16, 2, 5), (171, 20, 36, 16, 2, 5), (1025, 8, 32, 16, 4, 3)]
NOT_PERSISTENT = (130, 8, 32, 16, 4, 5)

# the relu(a v + b) epilogue leaves both families by design, and convt_smalln hands the backward epilogues on: where the tests say so by name
AFFINE_RELU_SHAPES = [(2, 5, 7, 24, 4, 5), (2, 8, 32, 16, 2, 5)]       # one of the VALU family, one of the quad family
SMALLN_BWD_EPILOGUE_SHAPE = (5, 9, 13, 20, 3, 5)

# Forward variants no other test pins by name: (kernel, (B, H, W, Cin, Cout, k, s))
FORWARD = [
    ("conv_patch_kernel", (2, 8, 32, 1, 32, 3, 1)),          # the general patch form from one channel at stride 1
    ("conv_patch_kernel", (2, 16, 32, 1, 32, 5, 2)),         # ... with a 5x5 stride-2 kernel (the 4x4 one goes to the taps family)
    ("conv_patch_kernel", (3, 8, 16, 2, 20, 3, 1)),          # ... from two channels at stride 1; 20 of 64 columns
    ("conv_smalln_f_kernel", (2, 256, 256, 16, 2, 3, 1)),    # N = 2: 512 tiles, the least the VALU head kernel takes
    ("conv_dot_kernel<2>", (2, 6, 7, 128, 2, 3, 2)),         # a wave per pixel, two channels, stride 2, odd sizes
]


def tshape_id(shape):
    return "x".join(str(v) for v in shape)


def t_call(shape, op, epilogue):
    """A transposed-direction shape as the arguments of predict / cgs_conv_family for op = DECONV_FWD or CONV_BWD_DATA."""
    B, Hs, Ws, Cs, N, k = shape
    if op == DECONV_FWD:
        return (op, B, Hs, Ws, Cs, 2 * Hs, 2 * Ws, N, k, 2, epilogue)
    assert op == CONV_BWD_DATA
    return (op, B, 2 * Hs, 2 * Ws, N, 0, 0, Cs, k, 2, epilogue)


def t_layer(shape):
    B, Hs, Ws, Cs, N, k = shape
    return layer_of(DECONV_FWD, Hs, Ws, Cs, 2 * Hs, 2 * Ws, N, k, 2)


def f_call(shape, epilogue):
    B, H, W, Cin, Cout, k, s = shape
    return (CONV_FWD, B, H, W, Cin, 0, 0, Cout, k, s, epilogue)


def ktol(k, c):
    """tests/test_gpu_fuzz.py: 2e-5 for reductions up to 1000 terms, growing with the square root of the length beyond."""
    return 2e-5 * max(1.0, (k * k * c / 1000.0) ** 0.5)


def bar(k, c, epilogue):
    return (1.5 if epilogue == EPI_TANH else 1.0) * ktol(k, c)


# ---- inputs (seeded float32; computed once per process and shared, never written to) and the float64 reference -----------------------
def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _off_zero(t):
    """Shift every element closer than AUX_MARGIN to zero out to +-2 AUX_MARGIN (nothing is dropped)."""
    near = t.abs() < AUX_MARGIN
    return torch.where(near, torch.where(t < 0, -2 * AUX_MARGIN, 2 * AUX_MARGIN).to(t.dtype), t)


TInputs = collections.namedtuple("TInputs", "x dy w bias a b aux_sign aux_tanh")


@functools.lru_cache(maxsize=None)
def t_inputs(shape):
    """x: the forward's input, dy: the backward-data's; w [k,k,N,Cs] scaled so that the sums are of order one (tanh is not saturated);
    a > 0, b: the affine pair; aux_sign: the saved activation of the relu' / lrelu' epilogues, off zero; aux_tanh: a saved tanh output."""
    B, Hs, Ws, Cs, N, k = shape
    seed = 7919 * B + 131 * Hs + 17 * Ws + 5 * Cs + 3 * N + k
    out = (B, 2 * Hs, 2 * Ws, N)
    w = _randn((k, k, N, Cs), seed + 2, 0.7 / (max(1.0, k * k / 4.0) * Cs) ** 0.5)
    return TInputs(_randn((B, Hs, Ws, Cs), seed), _randn((B, Hs, Ws, Cs), seed + 1), w, _randn((N,), seed + 3, 0.2),
                   _randn((N,), seed + 4).abs() + 0.5, _randn((N,), seed + 5, 0.3), _off_zero(_randn(out, seed + 6)),
                   torch.tanh(_randn(out, seed + 7)))


def transposed64(x, w, N):
    """[B,Hs,Ws,Cs] float32, w [k,k,N,Cs] float32 -> [B,2Hs,2Ws,N] float64, no bias."""
    B, Hs, Ws, _ = x.shape
    return R.deconv2d(x.double(), w.double(), torch.zeros(N, dtype=torch.float64), (B, 2 * Hs, 2 * Ws, N), 2, 2)


def fwd_epilogue64(lin, bias, epilogue, a=None, b=None):
    v = lin if bias is None else lin + bias.double()
    if epilogue == EPI_LRELU:
        return torch.maximum(v, 0.2 * v)
    if epilogue == EPI_TANH:
        return torch.tanh(v)
    if epilogue == EPI_AFFINE_RELU:
        return torch.relu(a.double() * v + b.double())
    assert epilogue == EPI_NONE
    return v


def bwd_epilogue64(lin, epilogue, a=None, aux=None):
    if epilogue == EPI_RELU_BWD_AFFINE:
        return torch.where(aux > 0, lin * a.double(), torch.zeros_like(lin))
    if epilogue == EPI_LRELU_BWD:
        return torch.where(aux > 0, lin, 0.2 * lin)
    if epilogue == EPI_TANH_BWD:
        return lin * (1.0 - aux.double() ** 2)
    assert epilogue == EPI_NONE
    return lin


def bwd_aux(inp, epilogue):
    return inp.aux_tanh if epilogue == EPI_TANH_BWD else inp.aux_sign if epilogue != EPI_NONE else None


@functools.lru_cache(maxsize=None)
def t_reference(shape):
    """-> (float64 transposed convolution of x, of dy) with the case's weights: the linear parts of every forward / backward-data call."""
    inp = t_inputs(shape)
    N = shape[4]
    with torch.no_grad():
        return transposed64(inp.x, inp.w, N), transposed64(inp.dy, inp.w, N)


FInputs = collections.namedtuple("FInputs", "x w bias")


@functools.lru_cache(maxsize=None)
def f_inputs(shape):
    B, H, W, Cin, Cout, k, s = shape
    seed = 104729 + 7919 * B + 131 * H + 17 * W + 5 * Cin + 3 * Cout + k + s
    return FInputs(_randn((B, H, W, Cin), seed), _randn((k, k, Cin, Cout), seed + 1, 0.7 / (k * k * Cin) ** 0.5), _randn((Cout,), seed + 2, 0.2))


@functools.lru_cache(maxsize=None)
def f_reference(shape):
    """The forward conv2d in float64, no bias."""
    inp, s = f_inputs(shape), shape[6]
    with torch.no_grad():
        return R.conv2d(inp.x.double(), inp.w.double(), torch.zeros(shape[4], dtype=torch.float64), s, s)


def parity_slices(t):
    """[B,2Hs,2Ws,N] -> ((py, px, n), the [B,Hs,Ws] slice of that parity class and channel), in a fixed order."""
    for py in (0, 1):
        for px in (0, 1):
            for n in range(t.shape[3]):
                yield (py, px, n), t[:, py::2, px::2, n]
