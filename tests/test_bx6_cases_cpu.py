"""tests/bx6_cases.py checked without a device: the split, the restated dispatch against the library's own cgs_conv_family, the coverage
the case table claims, the float64 reference against float64 autograd of the oracle's conv2d, and -- the point -- the POWER of
tests/test_gpu_bx6_accuracy.py: every call of the table is lowered to its GEMM and the model of the kernel's arithmetic is run on the very
inputs the GPU test uses, intact and with each of the five droppable products a0 b1, a1 b0, a1 b1, a0 b2, a2 b0 removed.  With the GPU
test's own metrics and bars (bx6_cases.random_bar, 10 x the float32 figures):

    random family        the intact model <= 1/2 of the bar and EACH of the five mutants >= 3 x the bar, in every group
    cancelling families  the intact model <= 1/3 of the bar and each of the family's three designated mutants >= 3 x the bar

so a kernel that lost a product -- in one instantiation, under one tap order, in one 32-column band, or through a wrong mid / lo plane
of the pack kernel -- cannot pass them.  Every figure is printed (run with -s)."""
import numpy as np
import pytest
import torch

import bx6_cases as BC
from oracle import ops_ref as R

CALL_PARAMS = [pytest.param(case, op, id=BC.call_id(case, op)) for case, op in BC.CALLS]


def _bf16(x):
    return not np.any(x.view(np.uint32) & np.uint32(0xffff))


def test_split_is_exact_and_every_piece_a_bf16():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(200000) * np.exp2(rng.uniform(-30, 30, 200000))).astype(np.float32)
    full = np.array([0x3fffffff, 0x3f800001, 0x3f80ffff, 0x3f8000ff, 0x3f808080], dtype=np.uint32).view(np.float32)   # all 24 bits set, one bit per piece, ...
    edge = np.concatenate([np.zeros(1, np.float32), np.exp2(np.arange(-30, 31)).astype(np.float32), full,
                           np.float32(1.9999999) * np.exp2(np.arange(-30, 31)).astype(np.float32)])
    assert (edge.view(np.uint32) & np.uint32(0x7fffff) == 0x7fffff).sum() >= 61
    for v in (x, edge, -edge):
        x0, x1, x2 = BC.split3(v)
        assert x0.dtype == x1.dtype == x2.dtype == np.float32
        nz = v != 0                                                                       # (-0 splits into -0 + 0 + 0 = +0)
        assert np.array_equal(((x0 + x1) + x2)[nz].view(np.uint32), v[nz].view(np.uint32)) and not ((x0 + x1) + x2)[~nz].any()      # bit for bit, in float32
        assert np.array_equal(v.astype(np.float64), x0.astype(np.float64) + x1 + x2)
        assert _bf16(x0) and _bf16(x1) and _bf16(x2)                                      # 8 significant bits each
        assert np.all(np.abs(x1) <= np.abs(x0) * 2.0 ** -7) and np.all(np.abs(x2) <= np.abs(x0) * 2.0 ** -15)
    # ... and the identity the kernel rests on: the six products are the product up to the three dropped terms a1 b2 + a2 b1 + a2 b2.
    # Truncation leaves |x1| < 2^-7 |x0| and |x2| < 2^-15 |x0| (8 significant bits are 7 below the leading one), so the bound that
    # holds for every operand is (2 * 2^-22 + 2^-30) |a b|; the 3 * 2^-24 |a b| of the kernel's header is the size for mid-binade operands.
    a, b = [p.astype(np.float64) for p in BC.split3(x[:100000])], [p.astype(np.float64) for p in BC.split3(x[100000:])]
    want = x[:100000].astype(np.float64) * x[100000:].astype(np.float64)
    six = sum(a[i] * b[j] for i, j in BC.PRODUCTS)
    rel = np.abs(six - want) / np.abs(want)
    print(f"dropped terms / |a b|: max {rel.max() * 2 ** 24:.2f} x 2^-24, mean {rel.mean() * 2 ** 24:.2f} x 2^-24")
    assert len(BC.PRODUCTS) == 6 and all(i + j <= 2 for i, j in BC.PRODUCTS) and rel.max() <= 2 * 2.0 ** -22 + 2.0 ** -30


def test_model_loses_what_it_is_told_to():
    rng = np.random.default_rng(6)
    A, W = rng.standard_normal((8, 64)).astype(np.float32), rng.standard_normal((64, 8)).astype(np.float32)
    As, Ws = [p.astype(np.float64) for p in BC.split3(A)], [p.astype(np.float64) for p in BC.split3(W)]
    both = BC.model_and_mutants(A, W)
    for drop in (None,) + BC.MUTANTS:
        want = sum(As[i] @ Ws[j] for i, j in BC.PRODUCTS if (i, j) != drop)
        for got in (BC.model(A, W, drop), BC.model(A, W, drop, tile=1), both[drop]):
            assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
        assert np.array_equal(BC.model(A, W, drop), both[drop])
    assert np.abs(BC.f32_chain(A, W) - A.astype(np.float64) @ W.astype(np.float64)).max() <= 1e-5


def test_restated_dispatch_equals_the_librarys():
    """bx6_ok against cgs_conv_family under "bx6_all" for every call of the table and on a sweep of channel counts, kernel sizes and
    strides; under "f32" no call of the table leaves the exact-fp32 implicit GEMM."""
    from cgs_amd import lib
    l = lib.load()
    assert lib.get_contraction() == "f32"
    for case, op in BC.CALLS:
        assert BC.lib_family(l, case, op) == BC.FAMILY_IGEMM, (case, op)
    lib.set_contraction("bx6_all")
    try:
        n = 0
        for case, op in BC.CALLS:
            want = BC.FAMILY_IGEMM_BX6 if BC.bx6_ok(BC.call_of(case, op)) else BC.FAMILY_IGEMM
            assert BC.lib_family(l, case, op) == want, (case, op)
            n += 1
        for B, H, W in ((2, 6, 5), (130, 4, 4)):
            for Cin in (3, 16, 32, 48, 64, 96, 128, 256):
                for Cout in (3, 32, 64, 96, 128, 192, 256, 384):
                    for k in (1, 3, 4, 5, 7, 16, 17):
                        for s in (1, 2, 3):
                            for op in BC.OPS:
                                case = (B, H, W, Cin, Cout, k, s)
                                c = BC.call_of(case, op)
                                if c.dirT and s > 2:
                                    assert not BC.bx6_ok(c)
                                    continue            # (the entry points refuse the call)
                                assert (BC.lib_family(l, case, op) == BC.FAMILY_IGEMM_BX6) == BC.bx6_ok(c), (case, op)
                                n += 1
        # the 2 GiB limit of the packed planes: 16 x 16 taps x 2048 x 1024 channels x 6 bytes
        for Cout, ok in ((512, True), (1024, False)):
            case = (1, 4, 4, 2048, Cout, 16, 1)
            assert BC.bx6_ok(BC.call_of(case, BC.CONV_FWD)) == ok == (BC.lib_family(l, case, BC.CONV_FWD) == BC.FAMILY_IGEMM_BX6)
    finally:
        lib.set_contraction("f32")
    print(f"bx6_ok == (cgs_conv_family == IGEMM_BX6) on {n} calls")


def test_table_reaches_what_it_claims():
    """All six instantiations, each from a big -> small and (parity order aside: the transposed geometry never sets it) from a transposed
    direction; the edges the rows name.  Prints the coverage list."""
    assert len(set(BC.CASES)) == len(BC.CASES)
    reach = {}
    for case, op in BC.CALLS:
        c = BC.call_of(case, op)
        reach.setdefault(BC.kernel_name(c), []).append((case, op, c))
    for name in BC.INSTANTIATIONS + [BC.IGEMM_PREFIX]:
        print(f"{name}: " + ", ".join(BC.call_id(case, op) for case, op, _ in reach.get(name, [])))
    assert set(reach) == set(BC.INSTANTIATIONS) | {BC.IGEMM_PREFIX}
    for name in BC.INSTANTIATIONS:
        dirs = {c.dirT for _, _, c in reach[name]}
        assert dirs == ({False} if name.endswith("true>") else {False, True}), name
    name_of = {(case, op): BC.kernel_name(BC.call_of(case, op)) for case, op in BC.CALLS}

    def rows(case, op):       # GEMM rows of the launch's largest class
        c = BC.call_of(case, op)
        step = c.s if c.dirT else 1
        return c.B * BC.ceil_div(c.out_shape[1], step) * BC.ceil_div(c.out_shape[2], step)

    F, CB, T, DB = BC.CONV_FWD, BC.CONV_BWD_DATA, BC.DECONV_FWD, BC.DECONV_BWD_DATA
    assert rows((2, 9, 7, 32, 256, 3, 1), F) == 126 and name_of[(2, 9, 7, 32, 256, 3, 1), F] == "igemm_bx6_kernel<128, 256, false>"
    assert rows((3, 16, 16, 32, 256, 7, 2), F) == 192 and name_of[(3, 16, 16, 32, 256, 7, 2), F] == "igemm_bx6_kernel<128, 256, false>"
    assert name_of[(2, 6, 6, 64, 160, 3, 2), CB] == name_of[(2, 6, 6, 64, 160, 3, 2), DB] == "igemm_bx6_kernel<128, 64, false>"
    assert name_of[(2, 8, 8, 96, 256, 3, 1), F] == name_of[(2, 8, 8, 96, 256, 3, 1), T] == "igemm_bx6_kernel<128, 256, false>"
    assert name_of[(2, 8, 8, 96, 256, 3, 1), CB] == name_of[(2, 8, 8, 96, 256, 3, 1), DB] == BC.IGEMM_PREFIX
    assert name_of[(2, 9, 8, 256, 96, 3, 2), DB] == "igemm_bx6_kernel<128, 256, true>" and name_of[(2, 9, 8, 256, 96, 3, 2), CB] == "igemm_bx6_kernel<128, 256, false>"
    assert name_of[(2, 18, 16, 32, 256, 4, 2), F] == "igemm_bx6_kernel<128, 256, true>"
    assert rows((3, 10, 10, 32, 128, 3, 1), F) == 300 and name_of[(2, 12, 12, 128, 128, 3, 2), DB] == "igemm_bx6_kernel<256, 128, true>"
    assert rows((2, 5, 5, 96, 384, 3, 1), F) == 50 and name_of[(2, 5, 5, 96, 384, 3, 1), F] == "igemm_bx6_kernel<256, 128, false>"
    assert name_of[(2, 18, 16, 32, 64, 4, 2), F] == "igemm_bx6_kernel<128, 64, true>"
    assert name_of[(3, 7, 9, 64, 192, 3, 2), F] == name_of[(3, 7, 9, 64, 192, 3, 2), CB] == "igemm_bx6_kernel<128, 64, false>"
    assert name_of[(1, 8, 8, 32, 64, 7, 1), F] == "igemm_bx6_kernel<128, 64, false>"
    # eight m-tiles: launch_bx6 decodes blocks per XCD when the m-tile count is a multiple of 8
    assert rows((4, 16, 16, 32, 64, 3, 1), F) == 8 * 128 and rows((8, 16, 16, 32, 128, 3, 1), F) == 8 * 256
    # the reductions stay short (see the table's header)
    for case, op in BC.CALLS:
        c = BC.call_of(case, op)
        if BC.bx6_ok(c):
            taps = BC.ceil_div(c.k, c.s) ** 2 if c.dirT else c.k * c.k         # (of the heaviest parity class)
            assert taps * c.Cred <= (1728 if (case, op) == ((3, 7, 9, 64, 192, 3, 2), DB) else 1600), (case, op)
    # pixel-major rows (igemm_pix_major: B >= 128, 1 < pixels <= 256): whole one-pixel tiles when B % 128 == 0, else straddling
    for case in ((128, 4, 4, 32, 64, 5, 2), (130, 4, 4, 32, 256, 5, 2)):
        for op in (F, T):
            c = BC.call_of(case, op)
            assert BC.bx6_ok(c) and c.B >= 128 and 1 < rows(case, op) // c.B <= 256
    assert BC.call_of((3, 6, 5, 96, 128, 4, 2, 11, 10), T).out_shape == (3, 11, 10, 128) and name_of[(3, 6, 5, 96, 128, 4, 2, 11, 10), T] == "igemm_bx6_kernel<256, 128, false>"
    # the families are what their names say: the hi pieces cancel pairwise along the reduced axis, the weights / activations are paired
    for case, op in ((BC.CASES[1], F), (BC.CASES[1], BC.CONV_BWD_DATA), (BC.CASES[-1], T), (BC.CASES[-1], DB)):
        c = BC.call_of(case, op)
        red = 3 if c.dirT else 2
        a, w = BC.inputs(case, op, BC.ACT_CANCEL)
        assert np.array_equal(BC.split3(a[..., 0::2].numpy())[0], -a[..., 1::2].numpy()) and a.shape[-1] == c.Cred == w.shape[red]
        assert torch.equal(w.movedim(red, -1)[..., 0::2], w.movedim(red, -1)[..., 1::2])
        a, w = BC.inputs(case, op, BC.W_CANCEL)
        wr = w.movedim(red, -1).contiguous()
        assert np.array_equal(BC.split3(wr[..., 0::2].contiguous().numpy())[0], -wr[..., 1::2].contiguous().numpy())
        assert torch.equal(a[..., 0::2], a[..., 1::2])


@pytest.mark.parametrize("case,op", CALL_PARAMS)
def test_reference_is_the_oracle_conv_and_its_adjoint(case, op):
    """Every direction is ops_ref.conv2d with the call's weights [k,k,Cb,Cs] or its adjoint: the float64 reference (ops_ref.deconv2d and
    autograd of it among them) against float64 autograd of ops_ref.conv2d / against ops_ref.conv2d itself; the scale bounds the result."""
    c = BC.call_of(case, op)
    a, w = BC.inputs(case, op, BC.RANDOM)
    ref = BC.reference(case, op, BC.RANDOM)
    assert tuple(ref.ref64.shape) == c.out_shape and ref.ref64.dtype == torch.float64 and ref.oracle32.dtype == torch.float32
    zeros = torch.zeros(c.Cs, dtype=torch.float64)
    if c.dirT:
        xb = torch.zeros((c.B, c.Hb, c.Wb, c.Cb), dtype=torch.float64, requires_grad=True)
        (R.conv2d(xb, w.double(), zeros, c.s, c.s) * a.double()).sum().backward()
        want = xb.grad
    else:
        with torch.no_grad():
            want = R.conv2d(a.double(), w.double(), zeros, c.s, c.s)
    assert float((ref.ref64 - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((ref.ref64.abs() <= ref.scale64 * (1 + 1e-12)).all()) and float(ref.scale64.min()) > 0
    # ... and the lowering to a GEMM reproduces it on the sampled pixels of every class
    for (py, px, band), _ in BC.groups(case, op):
        if band == 0 and c.Cred % 32 == 0:
            rows = BC.sample_rows(case, op, py, px)
            A, W = BC.lower(case, op, a, w, rows)
            at = ref.ref64[rows[:, 0], rows[:, 1], rows[:, 2]].numpy()
            assert np.abs(A.astype(np.float64) @ W.astype(np.float64) - at).max() <= 1e-12 * np.abs(at).max()
            assert (rows[:, 1] % (c.s if c.dirT else 1) == py % (c.s if c.dirT else 1)).all()


def _lowered(case, op, family):
    """-> [(class (py, px), rows, {drop: model result [rows, N]}, f32_chain result)] over the parity classes of the call."""
    c = BC.call_of(case, op)
    a, w = BC.inputs(case, op, family)
    out = []
    for (py, px, band), _ in BC.groups(case, op):
        if band == 0:
            rows = BC.sample_rows(case, op, py, px)
            A, W = BC.lower(case, op, a, w, rows)
            out.append(((py, px), rows, BC.model_and_mutants(A, W), None if family == BC.RANDOM else BC.f32_chain(A, W)))
    return out


BX6_PARAMS = [pytest.param(case, op, id=BC.call_id(case, op)) for case, op in BC.CALLS if BC.bx6_ok(BC.call_of(case, op))]


@pytest.mark.parametrize("case,op", BX6_PARAMS)
def test_power_random_family(case, op):
    """Metric (a) of the GPU test on the model: the intact arithmetic passes with half the bar to spare, every mutant misses it 3 x, in
    every group (parity class x 32-channel band; a sample of bx6_cases.ROWS output pixels per class)."""
    c = BC.call_of(case, op)
    ref = BC.reference(case, op, BC.RANDOM)
    bar = BC.random_bar(ref)
    worst = {drop: None for drop in (None,) + BC.MUTANTS}
    for (py, px), rows, results, _ in _lowered(case, op, BC.RANDOM):
        at = ref.ref64[rows[:, 0], rows[:, 1], rows[:, 2]].numpy()
        scale = ref.scale64[rows[:, 0], rows[:, 1], rows[:, 2]].numpy()
        for drop, got in results.items():
            e = np.abs(got.astype(np.float64) - at) / scale
            for band in range(c.N // 32):
                m = float(e[:, 32 * band:32 * band + 32].mean())
                if drop is None:
                    assert m <= 0.5 * bar, f"intact model, class ({py}, {px}) band {band}: {m:.2e} vs half the bar {0.5 * bar:.2e}"
                    worst[drop] = max(worst[drop] or 0.0, m)
                else:
                    assert m >= 3 * bar, f"mutant without a{drop[0]} b{drop[1]}, class ({py}, {px}) band {band}: {m:.2e} vs 3 x the bar {3 * bar:.2e}"
                    worst[drop] = min(worst[drop] or m, m)
    K = c.k * c.k * c.Cred // (c.s * c.s if c.dirT else 1)
    print(f"power {BC.call_id(case, op)} {BC.kernel_name(c)} K~{K}: bar {bar:.2e} | intact {worst[None] / bar:.2f} of it | weakest group of each mutant: "
          + "  ".join(f"-a{i}b{j} {worst[(i, j)] / bar:.1f}x" for i, j in BC.MUTANTS))


@pytest.mark.parametrize("family", [BC.ACT_CANCEL, BC.W_CANCEL])
@pytest.mark.parametrize("case,op", BX6_PARAMS)
def test_power_cancelling_families(case, op, family):
    """Assertion (b) on the model: max|delta| / max|ref64| over the sampled pixels against 10 x the larger of the float32 oracle's figure
    (whole tensor) and the exact-fp32 chain's (same pixels)."""
    ref = BC.reference(case, op, family)
    top = float(ref.ref64.abs().max())
    assert top > 0
    low = _lowered(case, op, family)

    def figure(pick):
        return max(float(np.abs(pick(entry).astype(np.float64) - ref.ref64[entry[1][:, 0], entry[1][:, 1], entry[1][:, 2]].numpy()).max()) for entry in low) / top

    oracle, chain = BC.max_error(ref.oracle32, ref), figure(lambda entry: entry[3])
    bar = BC.CANCEL_BAR_X * max(oracle, chain)
    intact = figure(lambda entry: entry[2][None])
    mutants = {drop: figure(lambda entry: entry[2][drop]) for drop in BC.MUTANTS}
    print(f"power {BC.call_id(case, op)} {family}: oracle {oracle:.2e} chain {chain:.2e} bar {bar:.2e} | intact {intact / bar:.3f} of it | "
          + "  ".join(f"-a{i}b{j} {mutants[(i, j)] / bar:.0f}x" for i, j in BC.MUTANTS))
    assert intact <= bar / 3, f"intact model {intact:.2e} vs a third of the bar {bar / 3:.2e}"
    for drop in BC.DESIGNATED[family]:
        assert mutants[drop] >= 3 * bar, f"mutant without a{drop[0]} b{drop[1]}: {mutants[drop]:.2e} vs 3 x the bar {3 * bar:.2e}"
