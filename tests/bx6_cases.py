"""The split-bf16 contraction (csrc/igemm_bx6.hip) product by product: its split restated in numpy, a model of its arithmetic that can
lose one of the six products, the dispatch restated in plain integers, seeded inputs, the float64 reference and the case table two tests
share (tests/test_bx6_cases_cpu.py checks the restatements against the library, the table's coverage, the reference against autograd and
-- the point of the file -- that the assertions of tests/test_gpu_bx6_accuracy.py cannot hold for a kernel that lost a product).  Not a
test module and not a conftest: the tests import it by name.  Imports no GPU.

    split3         x = x0 + x1 + x2, three bf16 pieces by truncation: ``bx6_split2`` and ``pack_weights_bx6_kernel`` in four lines
    model          the six products a_i b_j (i + j <= 2) of a GEMM summed in an fp32 accumulator in K order, as the kernel issues them: per
                   16-deep K tile one v_mfma_f32_32x32x16_bf16 per product, in the order of the kernel's MM list; a tile's 16-term sum of
                   one product is taken exactly (tile=16; every term has 16 significant bits) and rounded once into the accumulator.
                   tile=1 is the plain chain that rounds after every term.  drop=(i, j) loses one product.  The model derives no result
                   the device is held to: it sizes the bars' headroom and proves that the tests have power.
    f32_chain      the exact-fp32 kernel's arithmetic: one fma per term in K order
    call_of        a table case in one of the four directions as the kernels see it: conv_call_of + cgs_geom_F / cgs_geom_T of csrc/api.hip
    bx6_ok, kernel_name   ``cgs_igemm_bx6_ok(any_size)`` and the string ``cgs_last_kernel()`` reports
    inputs         three families per (case, direction): random, activation-hi-cancelling, weight-hi-cancelling (below)
    reference      float64 oracle operator on the float32 inputs, the scale sum|a||b| (the operator on absolute values) and the float32
                   oracle's own result -- the measuring stick of the bars
    lower          the call as a GEMM over a sample of output pixels of one group, K in the kernel's order (32-channel chunk, tap, channel)

The metrics and bars (the GPU test's assertions (a) and (b); the CPU test holds the model and its mutants to the same functions):

    (a) random family: mean of |got - ref64| / sum|a||b| over a group -- a parity class (py, px) of a stride-2 transposed direction (else
        the whole tensor) times a 32-channel band of N (the kernel's 32-column MFMA tiles) -- <= 4 x the same mean of the float32
        oracle's result over the whole tensor (the oracle's blocking knows nothing of the kernel's groups).
    (b) cancelling families: max|got - ref64| / max|ref64| <= 10 x the larger of the float32 oracle's and the exact-fp32 kernel's
        (on the CPU: its model's, ``f32_chain``) figure on the same inputs.

The cancelling families are properties of the mathematical sum, whatever the K order, tap order, tiling or zero padding: along the reduced
channel axis, activation channel 2c+1 = -hi(channel 2c) with equal weights for both channels leaves sum (a1 + a2) w, which lives entirely
in the mid / lo planes of the in-kernel split (losing a1 b0 is a 100 % error, a1 b1 or a2 b0 one of 2^-8); the mirror image with the
weights paired isolates a0 b1, a1 b1 and a0 b2 of the pack-time split.
"""
import collections
import functools

import numpy as np
import torch

from oracle import ops_ref as R

# include/cgs_hip.h, cgs_amd/lib.py
CONV_FWD, CONV_BWD_DATA, DECONV_FWD, DECONV_BWD_DATA = 0, 1, 2, 3
OPS = (CONV_FWD, CONV_BWD_DATA, DECONV_FWD, DECONV_BWD_DATA)
OP_NAMES = {CONV_FWD: "conv_fwd", CONV_BWD_DATA: "conv_bwd_data", DECONV_FWD: "deconv_fwd", DECONV_BWD_DATA: "deconv_bwd_data"}
FAMILY_IGEMM, FAMILY_IGEMM_BX6 = 0, 7
IGEMM_PREFIX = "igemm_kernel<"
INSTANTIATIONS = [f"igemm_bx6_kernel<{bm}, {bn}, {p}>" for bm, bn in ((128, 256), (256, 128), (128, 64)) for p in ("false", "true")]

RANDOM, ACT_CANCEL, W_CANCEL = "random", "act_cancel", "w_cancel"
FAMILIES = (RANDOM, ACT_CANCEL, W_CANCEL)
# the kernel's MM list: hi x hi first, the two second-order cross products last
PRODUCTS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))
MUTANTS = PRODUCTS[1:]
DESIGNATED = {ACT_CANCEL: ((1, 0), (1, 1), (2, 0)), W_CANCEL: ((0, 1), (1, 1), (0, 2))}

OPERATOR_BAR = 2e-5         # the project's operator bar, max|delta| / max|ref| (tests/test_gpu_ops.py): kept, it catches indexing faults
RANDOM_BAR_X = 4.0          # (a)
CANCEL_BAR_X = 10.0         # (b)


# ---- the split and the arithmetic ------------------------------------------------------------------------------------------------------
def _hi(x):
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    """float32 array -> (x0, x1, x2) float32, each a bf16 value: mask the low 16 bits, subtract in fp32, repeat."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x0 = _hi(x)
    r = x - x0
    x1 = _hi(r)
    q = r - x1
    return x0, x1, _hi(q)


def _tile_products(A, W, tile):
    """{(i, j): [K / tile, M, N] float64}: every tile's exact sum of one product."""
    M, K = A.shape
    assert K % tile == 0 and W.shape[0] == K
    As = [p.astype(np.float64).reshape(M, K // tile, tile).transpose(1, 0, 2) for p in split3(A)]
    Ws = [p.astype(np.float64).reshape(K // tile, tile, W.shape[1]) for p in split3(W)]
    keep = np.array([bool(a.any()) for a in As[0]])          # (a tile of zero padding adds exact zeros: left out)
    return {(i, j): np.matmul(As[i][keep], Ws[j][keep]) for i, j in PRODUCTS}


def _accumulate(parts, shape, drop):
    acc = np.zeros(shape, dtype=np.float32)
    for t in range(len(parts[(0, 0)])):
        for ij in PRODUCTS:
            if ij != drop:
                acc = (acc + parts[ij][t]).astype(np.float32)       # (float32 + float64 is taken in float64: one rounding)
    return acc


def model(A, W, drop=None, tile=16):
    """A [M, K], W [K, N] float32 -> [M, N] float32: see the module docstring."""
    A, W = np.asarray(A, dtype=np.float32), np.asarray(W, dtype=np.float32)
    return _accumulate(_tile_products(A, W, tile), (A.shape[0], W.shape[1]), drop)


def model_and_mutants(A, W, tile=16):
    """{None: the intact model, (i, j): the model without that product} -- the tiles' products are computed once."""
    A, W = np.asarray(A, dtype=np.float32), np.asarray(W, dtype=np.float32)
    parts = _tile_products(A, W, tile)
    return {drop: _accumulate(parts, (A.shape[0], W.shape[1]), drop) for drop in (None,) + MUTANTS}


def f32_chain(A, W):
    """acc = fma(a_k, b_k, acc) over k in float32."""
    A64, W64 = np.asarray(A, dtype=np.float32).astype(np.float64), np.asarray(W, dtype=np.float32).astype(np.float64)
    acc = np.zeros((A64.shape[0], W64.shape[1]), dtype=np.float32)
    for k in range(A64.shape[1]):
        if A64[:, k].any():
            acc = (acc + A64[:, k:k + 1] * W64[k:k + 1, :]).astype(np.float32)      # (24 x 24 bits: exact in float64)
    return acc


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------------
Call = collections.namedtuple("Call", "op dirT B k s Hb Wb Cb Hs Ws Cs in_shape out_shape w_shape Cred N")


def ceil_div(a, b):
    return -(-a // b)


def case_id(case):
    return "x".join(str(v) for v in case)


def call_of(case, op):
    """case = (B, H, W, Cin, Cout, k, s[, Ho, Wo]): a conv2d [B,H,W,Cin] -> [B,H/s,W/s,Cout] with w [k,k,Cin,Cout], or a deconv2d
    [B,H,W,Cin] -> [B,Ho,Wo,Cout] (s H x s W unless the case says otherwise) with w [k,k,Cout,Cin], forward or backward-data.  The
    weights are [k,k,Cb,Cs] of the big and the small tensor either way; the transposed directions (conv backward-data, deconv
    forward) go small -> big and reduce over Cs, the others big -> small over Cb."""
    B, H, W, Cin, Cout, k, s = case[:7]
    if op in (CONV_FWD, CONV_BWD_DATA):
        Hb, Wb, Cb, Hs, Ws, Cs = H, W, Cin, ceil_div(H, s), ceil_div(W, s), Cout
    else:
        Ho, Wo = case[7:] if len(case) > 7 else (s * H, s * W)
        assert ceil_div(Ho, s) == H and ceil_div(Wo, s) == W
        Hb, Wb, Cb, Hs, Ws, Cs = Ho, Wo, Cout, H, W, Cin
    dirT = op in (CONV_BWD_DATA, DECONV_FWD)
    big, small = (B, Hb, Wb, Cb), (B, Hs, Ws, Cs)
    return Call(op, dirT, B, k, s, Hb, Wb, Cb, Hs, Ws, Cs, small if dirT else big, big if dirT else small, (k, k, Cb, Cs),
                Cs if dirT else Cb, Cb if dirT else Cs)


def lib_args(case, op):
    """The arguments of cgs_conv_family / cgs_conv_ws_bytes_for after the op: B, H, W, Cin, Ho, Wo, Cout, k, k, s, s of the OPERATOR."""
    B, H, W, Cin, Cout, k, s = case[:7]
    c = call_of(case, op)
    ho, wo = (c.Hb, c.Wb) if op in (DECONV_FWD, DECONV_BWD_DATA) else (0, 0)
    return (B, H, W, Cin, ho, wo, Cout, k, k, s, s)


def bx6_ok(c):
    """cgs_igemm_bx6_ok(L, dirT, B, any_size = true): whole 32-channel chunks of the reduction into whole 64-column wave tiles, at most
    16 taps per axis, stride <= 2 in the transposed direction, the packed planes of a class inside 32-bit byte offsets."""
    return c.Cred % 32 == 0 and c.N % 64 == 0 and c.k <= 16 and not (c.dirT and c.s > 2) and c.k * c.k * c.Cred * c.N * 6 <= 0x7fffffff


def tap_parity(c):
    """cgs_geom_F / cgs_geom_T: evens-then-odds tap order in the stride-2 big -> small direction on grids of more than 64 pixels."""
    return (not c.dirT) and c.s == 2 and c.Hs * c.Ws > 64


def kernel_name(c):
    """The string cgs_last_kernel() reports under "bx6_all": the exact instantiation, or the exact-fp32 kernel's prefix."""
    if not bx6_ok(c):
        return IGEMM_PREFIX
    bm, bn = (128, 256) if c.N % 256 == 0 else (256, 128) if c.N % 128 == 0 else (128, 64)
    return f"igemm_bx6_kernel<{bm}, {bn}, {'true' if tap_parity(c) else 'false'}>"


def name_matches(want, got):
    return got.startswith(IGEMM_PREFIX) if want == IGEMM_PREFIX else got == want


def tap_order(i, n, parity_first):
    """cgs_tap_order: the i-th tap visited along an axis of n taps."""
    if not parity_first:
        return i
    ne = (n + 1) >> 1
    return 2 * i if i < ne else 2 * (i - ne) + 1


def lib_family(lib, case, op):
    """cgs_conv_family asked as kernels._WsCache.plan asks it (the calling thread's contraction mode counts).  No device needed."""
    a = lib_args(case, op)
    nbytes = max(int(lib.cgs_conv_ws_bytes_for(op, a[0], a[1], a[2], a[3], a[6], a[7], a[8], a[9], a[10])), 16)
    return int(lib.cgs_conv_family(op, *a, 0, nbytes))


# ---- the cases: (B, H, W, Cin, Cout, k, s[, Ho, Wo]), what the case is there for ---------------------------------------------------------
# Each runs in all four directions; a direction the split-bf16 kernel does not serve (N % 64, Cred % 32) must land on igemm_kernel.
# M = GEMM rows of a launch (per parity class in the transposed directions).  The reduction stays short, K = k k Cred <= 1600 (1728 in
# one backward-data): the distance between the intact arithmetic and a mutant shrinks like 1 / sqrt(K), and so does the float32 oracle's
# own error -- the measuring stick -- where torch sums a backward-data in blocks (4 x 6.5e-9 at K = 2304 on one machine, 8.8e-9 on another:
# too close to the 1.2 .. 1.4e-8 of the intact model and the 1.9e-8 of the device).  That is why no served direction reduces over 256
# channels with 3 x 3 taps or more, and why some cases have a channel count that keeps their backward-datas on the exact-fp32 kernel.
TABLE = [
    ((2, 9, 7, 32, 256, 3, 1), "<128,256>: one ragged tile, M = 126"),
    ((3, 16, 16, 32, 256, 7, 2), "<128,256>: K = 1568 at stride 2, ragged second tile (M = 192)"),
    ((2, 6, 6, 64, 160, 3, 2), "the backward-datas reduce over 160 into 64: <128,64> from five chunks"),
    ((2, 8, 8, 96, 256, 3, 1), "<128,256> in both directions at stride 1, three chunks"),
    ((2, 9, 8, 256, 96, 3, 2), "<128,256> in both directions at stride 2 (the backward-datas); the deconv one has 72 > 64 pixels: parity order"),
    ((2, 18, 16, 32, 256, 4, 2), "<128,256,true> from a conv forward with one chunk (K = 512)"),
    ((3, 10, 10, 32, 128, 3, 1), "<256,128>: M = 300 = 256 + 44"),
    ((2, 12, 12, 128, 128, 3, 2), "<256,128> in both directions, the deconv backward-data with parity order"),
    ((2, 5, 5, 96, 384, 3, 1), "three n-tiles of <256,128>, three chunks, M = 50 (at M = 25 one machine's float32 oracle errs 10 x more on the cancelling inputs)"),
    ((2, 18, 16, 32, 64, 4, 2), "the one-wave <128,64> block, one n-tile; conv forward with parity order"),
    ((3, 7, 9, 64, 192, 3, 2), "<128,64>: three n-tiles, odd sizes; the backward-datas reduce over 192 into 64"),
    ((2, 6, 5, 64, 64, 3, 1), "<128,64> in both directions at stride 1"),
    ((1, 8, 8, 32, 64, 7, 1), "49 taps"),
    ((4, 16, 16, 32, 64, 3, 1), "M = 1024: eight m-tiles of 128, the per-XCD block decode"),
    ((8, 16, 16, 32, 128, 3, 1), "M = 2048: eight m-tiles of 256, the same"),
    ((128, 4, 4, 32, 64, 5, 2), "pixel-major: whole one-pixel tiles, zero-tap skipping, heaviest-first order"),
    ((130, 4, 4, 32, 256, 5, 2), "pixel-major with tiles straddling pixels"),
    ((3, 6, 5, 96, 128, 4, 2, 11, 10), "deconv to 11 x 10: parity classes of unequal size"),
]
CASES = [case for case, _ in TABLE]
CALLS = [(case, op) for case in CASES for op in OPS]


def call_id(case, op):
    return f"{case_id(case)}-{OP_NAMES[op]}"


# ---- inputs (seeded float32, computed once per process, never written to) and references ----------------------------------------------
def _seed(case, op, family):
    return (sum(p * v for p, v in zip((7919, 131, 17, 5, 3, 101, 211, 13, 29), case)) * 4 + op) * 3 + FAMILIES.index(family)


def _hi_t(t):
    return torch.from_numpy(_hi(np.ascontiguousarray(t.numpy())).copy())


def _small_residual(t):
    """hi(t) + (t - hi(t)) / 4: the part of the paired operand that survives the cancellation, a quarter of its natural size.  What the
    arithmetic drops by design (a1 b2 + a2 b1 + a2 b2, 2^-16 of the surviving sum) stays where it is relative to the result, while the
    rounding of any float32 summation -- the measuring stick of bar (b) -- grows fourfold relative to it: the intact arithmetic then sits
    at a tenth of the bar, not a third, and the mutants that lose a 2^-8 share of the result still miss it sixfold."""
    h = _hi_t(t)
    return h + (t - h) * 0.25


@functools.lru_cache(maxsize=None)
def inputs(case, op, family):
    """-> (a, w): the tensor the call contracts (the forward's x / the backward-data's dy) and the operator's weights [k,k,Cb,Cs].
    random: randn activations over several binades (x (1 + 3 rand), as tools/bx6_accuracy.py), 0.05 randn weights.
    act_cancel: activation channel 2c+1 = -hi(channel 2c) along the reduced axis, the weights of both channels equal.
    w_cancel: weight channel 2c+1 = -hi(channel 2c) along the reduced axis, the activations of both channels equal.
    (The even channels of the paired operand are the random family's with their residual quartered: _small_residual.)"""
    c = call_of(case, op)
    g = torch.Generator().manual_seed(_seed(case, op, family))
    a = (torch.randn(c.in_shape, generator=g) * (1 + 3 * torch.rand(c.in_shape, generator=g))).float()
    w = (torch.randn(c.w_shape, generator=g) * 0.05).float()
    red = 3 if c.dirT else 2                    # the reduced channel axis of the weights
    wr = w.movedim(red, -1).contiguous()
    if family == ACT_CANCEL:
        a[..., 0::2] = _small_residual(a[..., 0::2].contiguous())
        a[..., 1::2] = -_hi_t(a[..., 0::2].contiguous())
        wr[..., 1::2] = wr[..., 0::2]
    elif family == W_CANCEL:
        a[..., 1::2] = a[..., 0::2]
        wr[..., 0::2] = _small_residual(wr[..., 0::2].contiguous())
        wr[..., 1::2] = -_hi_t(wr[..., 0::2].contiguous())
    else:
        assert family == RANDOM
    return a.contiguous(), wr.movedim(-1, red).contiguous()


def operator(case, op, a, w):
    """The oracle operator of a direction in the dtype of its arguments: ops_ref.conv2d / deconv2d, autograd for the backward-datas."""
    c = call_of(case, op)
    s = c.s
    if op == CONV_FWD:
        with torch.no_grad():
            return R.conv2d(a, w, torch.zeros(c.Cs, dtype=a.dtype), s, s)
    if op == DECONV_FWD:
        with torch.no_grad():
            return R.deconv2d(a, w, torch.zeros(c.Cb, dtype=a.dtype), c.out_shape, s, s)
    x = torch.zeros(c.out_shape, dtype=a.dtype, requires_grad=True)
    with torch.backends.mkldnn.flags(enabled=False):          # (oneDNN's convolution backward is not safe on degenerate shapes: tests/test_gpu_fuzz.py)
        if op == CONV_BWD_DATA:
            y = R.conv2d(x, w, torch.zeros(c.Cs, dtype=a.dtype), s, s)
        else:
            y = R.deconv2d(x, w, torch.zeros(c.Cb, dtype=a.dtype), (c.B, c.Hb, c.Wb, c.Cb), s, s)
        (y * a).sum().backward()
    return x.grad.detach()


Reference = collections.namedtuple("Reference", "ref64 scale64 oracle32")


@functools.lru_cache(maxsize=None)
def reference(case, op, family, w_times=1.0):
    """float64 operator on the float32 inputs (weights scaled in float32 by w_times first), the same on absolute values, the float32 oracle."""
    a, w = inputs(case, op, family)
    if w_times != 1.0:
        w = w * w_times
    return Reference(operator(case, op, a.double(), w.double()), operator(case, op, a.double().abs(), w.double().abs()), operator(case, op, a, w))


def groups(case, op):
    """The groups of metric (a): ((py, px, band), index into [B,Hout,Wout,N]) -- parity classes only in a stride-2 transposed direction."""
    c = call_of(case, op)
    classes = [(py, px) for py in range(c.s) for px in range(c.s)] if c.dirT and c.s == 2 else [(0, 0)]
    step = c.s if c.dirT and c.s == 2 else 1
    for py, px in classes:
        for band in range(c.N // 32 if c.N % 32 == 0 else 1):
            cols = slice(32 * band, 32 * band + 32) if c.N % 32 == 0 else slice(None)
            yield (py, px, band), (slice(None), slice(py, None, step), slice(px, None, step), cols)


def scaled_error(got, ref):
    """|got - ref64| / sum|a||b|, elementwise (float64 tensor)."""
    return (got.detach().cpu().double() - ref.ref64).abs() / ref.scale64


def random_bar(ref):
    return RANDOM_BAR_X * float(scaled_error(ref.oracle32, ref).mean())


def max_error(got, ref):
    """max|got - ref64| / max|ref64|."""
    return float((got.detach().cpu().double() - ref.ref64).abs().max() / ref.ref64.abs().max())


# ---- the call as a GEMM --------------------------------------------------------------------------------------------------------------------
ROWS = 24       # sampled output pixels per parity class


def sample_rows(case, op, py, px):
    """[<= ROWS, 3] (b, oy, ox): output pixels of one parity class, evenly spaced from the first to the last, corners included."""
    c = call_of(case, op)
    step = c.s if c.dirT and c.s == 2 else 1
    _, Hout, Wout, _ = c.out_shape
    ys, xs = np.arange(py, Hout, step), np.arange(px, Wout, step)
    n = c.B * len(ys) * len(xs)
    pick = np.unique(np.linspace(0, n - 1, min(ROWS, n)).round().astype(np.int64))
    b, rem = pick // (len(ys) * len(xs)), pick % (len(ys) * len(xs))
    return np.stack([b, ys[rem // len(xs)], xs[rem % len(xs)]], axis=1)


def lower(case, op, a, w, rows):
    """-> A [len(rows), K], W [K, N] float32 with K = k k Cred in the kernel's order: 32-channel chunk, tap in visiting order (rows, then
    columns; evens first under the parity order), channel in chunk.  A tap outside the image, or -- in a transposed direction -- of
    another parity class than the row's, is a block of zeros."""
    c = call_of(case, op)
    a, w = a.numpy(), w.numpy()
    k, s = c.k, c.s
    pt, pl = R.same_pads(c.Hb, k, s)[0], R.same_pads(c.Wb, k, s)[0]
    par = tap_parity(c)
    taps = [(tap_order(i, k, par), tap_order(j, k, par)) for i in range(k) for j in range(k)]
    _, Hin, Win, _ = c.in_shape
    A = np.zeros((len(rows), c.Cred // 32, len(taps), 32), dtype=np.float32)
    Wm = np.zeros((c.Cred // 32, len(taps), 32, c.N), dtype=np.float32)
    b, oy, ox = rows[:, 0], rows[:, 1], rows[:, 2]
    for t, (ky, kx) in enumerate(taps):
        if c.dirT:      # out[oy] += in[iy] w[ky] where oy = s iy + ky - pt
            ny, nx = oy + pt - ky, ox + pl - kx
            ok = (ny % s == 0) & (nx % s == 0)
            iy, ix = ny // s, nx // s
            wt = w[ky, kx].T            # [Cs = Cred, Cb = N]
        else:           # out[oy] += in[s oy + ky - pt] w[ky]
            iy, ix = oy * s + ky - pt, ox * s + kx - pl
            ok = np.ones(len(rows), dtype=bool)
            wt = w[ky, kx]              # [Cb = Cred, Cs = N]
        ok = ok & (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
        A[ok, :, t, :] = a[b[ok], iy[ok], ix[ok]].reshape(-1, c.Cred // 32, 32)
        Wm[:, t] = wt.reshape(c.Cred // 32, 32, c.N)
    return A.reshape(len(rows), -1), Wm.reshape(-1, c.N)
