"""csrc/drs.hip on the device against the float64 statement of tests/drs_cases.py.

decide.  Bar: every P within the bound of drs_cases.bound -- the error model of two math libraries 2 ulp apart carried through the
definition on the REFERENCE's intermediate values -- the state within its bound, and, because test_drs_cases_cpu holds every uniform at
least 8 bounds away from its row's P, mask and counts EQUAL to the reference's with no exception.  The worst measured ratio
|P_dev - P_ref| / bound is printed per case; it has to stay below 1.
Sizes: b = 1, 2 (degenerate percentiles), 63 / 64 / 65 (a wave), 257 (one row past the block), 1000, 10 000 (40 rows per thread);
groups 32 / 3 / 2 (the prefix maximum over blocks).  q = None, 0 (first rank), 37.5 and 60 (interpolated: the radix select), 100 (the
max-reduce path, which must give the bits of the general path: checked against the same statement).

compact.  Bar: bit equality with src[selected][:room], every other row of dst untouched, the unclipped total exact.  Row lengths 1, 2, 3
(4-byte pieces, many rows per block), 784 (196 16-byte pieces: one row per block), 12 288 (3072 pieces: a row spans 12 blocks)."""
import functools

import numpy as np
import pytest
import torch

import drs_cases as DC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {"ratio": 0.0, "case": None}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def _case(b, groups, q, kind, call):
    c = DC.build(b, groups, q, kind, call)
    for v in (c["sig"], c["u"], c["dP"], c["dM"], *c["ref"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _run(rej, c, groups, q):
    mask, counts, P = rej.decide_device(_dev(c["sig"]), c["u"], q, DC.EPS, groups, want_p=True)
    return mask.cpu().numpy().astype(bool), counts.cpu().numpy(), P.cpu().numpy(), rej.last_bounds.cpu().numpy(), rej.D_tilde_M


@pytest.mark.parametrize("b,groups,q,kind", DC.all_cases(), ids=[DC.case_id(*c) for c in DC.all_cases()])
def test_decide_equals_the_statement(b, groups, q, kind):
    from cgs_amd.sampling import DeviceRejector
    first, second = _case(b, groups, q, kind, 0), _case(b, groups, q, kind, 1)
    assert first["margin_ok"] and second["margin_ok"]
    rej = DeviceRejector(DEV)
    rej.D_tilde_M = first["M0"]
    assert rej.D_tilde_M == first["M0"]
    runs = []
    for c in (first, second):                                            # the second call continues the first one's state
        mask, counts, P, bounds, M = _run(rej, c, groups, q)
        ref = c["ref"]
        ratio = float(np.max(np.abs(P - ref["P"]) / c["dP"]))
        print(f"{DC.case_id(b, groups, q, kind)}: worst |dP| / bound = {ratio:.3g}, |dM| = {abs(M - ref['M'][-1]):.3g} (bound {c['dM'][-1]:.3g})")
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, case=DC.case_id(b, groups, q, kind))
        assert np.all(np.abs(P - ref["P"]) <= c["dP"]), ratio
        assert np.array_equal(mask, c["u"] < P)
        assert np.array_equal(mask, ref["mask"])
        assert counts.dtype == np.int32 and np.array_equal(counts, ref["counts"])
        assert np.all(np.abs(bounds - ref["M"]) <= c["dM"]) and M == bounds[-1]
        runs.append((mask, counts, P, bounds, M))
    again = DeviceRejector(DEV)                                          # a rerun from the same start: bit-equal
    again.D_tilde_M = first["M0"]
    for c, (mask, counts, P, bounds, M) in zip((first, second), runs):
        m2, c2, P2, b2, M2 = _run(again, c, groups, q)
        assert np.array_equal(m2, mask) and np.array_equal(c2, counts) and np.array_equal(P2, P) and np.array_equal(b2, bounds) and M2 == M


def test_worst_ratio_over_the_cases_is_below_one():
    print(f"worst |dP| / bound over the decide cases run in this session: {WORST['ratio']:.3g} ({WORST['case']})")
    assert WORST["ratio"] < 1.0


def test_q100_takes_the_bits_of_the_general_path():
    """q = 100 skips the select; q just below 100 on a batch whose two top values are equal runs it and must give the same gamma."""
    from cgs_amd.sampling import DeviceRejector
    rs = np.random.RandomState(5)
    for b in (2, 65, 1000):
        sig = rs.uniform(0.05, 0.9, b).astype(np.float32)
        sig[rs.randint(b)] = sig.max()                                   # (at least) two rows share the top score
        sig[(int(np.argmax(sig)) + 1) % b] = sig.max()
        u = rs.rand(b)
        out = []
        for q in (100.0, 100.0 * (b - 1.5) / (b - 1)):                   # virtual index b - 1 and b - 1.5: ranks b - 2, b - 1
            rej = DeviceRejector(DEV)
            _, _, P = rej.decide_device(_dev(sig), u, q, DC.EPS, 1, want_p=True)
            out.append(P.cpu().numpy())
        assert np.array_equal(out[0], out[1]), b


def test_decide_draws_one_numpy_batch_per_group_and_reads_back_counts():
    from cgs_amd.sampling import DeviceRejector, Rejector
    b, groups = 64, 3
    sig = np.random.RandomState(9).uniform(0.01, 0.99, (b * groups, 1)).astype(np.float32)
    host = Rejector()
    np.random.seed(31)
    want = [host.sampling(np.arange(b), sig[g * b:(g + 1) * b], shift_percent=100.0) for g in range(groups)]
    tail = np.random.rand(2)
    rej = DeviceRejector(DEV)
    np.random.seed(31)
    mask, counts = rej.decide(_dev(sig), shift_percent=100.0, groups=groups)
    assert np.array_equal(np.random.rand(2), tail)
    assert isinstance(counts, np.ndarray) and [len(w) for w in want] == list(counts) and mask.device.type == "cuda"
    m = mask.cpu().numpy().astype(bool)
    for g in range(groups):
        assert np.array_equal(np.arange(b)[m[g * b:(g + 1) * b]], want[g])
    assert abs(rej.D_tilde_M - float(host.D_tilde_M)) <= 4 * np.spacing(abs(float(host.D_tilde_M)))


@pytest.mark.parametrize("n", [1, 64, 65, 257, 10000])
def test_set_score_max(n):
    from cgs_amd.sampling import DeviceRejector, Rejector
    rs = np.random.RandomState(n)
    for s in (rs.uniform(0.01, 0.99, n), rs.uniform(0.31, 0.64, n), np.r_[rs.uniform(0, 1, n - 1), 1.0], np.zeros(n)):
        s = s.astype(np.float32)
        host = Rejector()
        host.set_score_max(np.amax(s))
        rej = DeviceRejector(DEV)
        rej.set_score_max(_dev(s.reshape(-1, 1)))
        want = float(host.D_tilde_M)
        assert abs(rej.D_tilde_M - want) <= 5 * np.spacing(abs(want))   # two log1p 2 ulp apart each and a subtraction, or one log
        rej.set_score_max(np.amax(s))                                    # a host scalar takes the same route
        assert abs(rej.D_tilde_M - want) <= 5 * np.spacing(abs(want))


# ---------------------------------------------------------------------------------------------------------------- compact
ROWS = [1, 2, 3, 784, 1024, 1028, 12288]                             # 1024: 256 float4 pieces, a block; 1028: 257, the first row that spans two
NS = [1, 64, 65, 2048]
MASKS = ["none", "all", "alternating", "random", "take_all"]


@functools.lru_cache(maxsize=None)
def _src(n, row):
    """[n, row] fp32, every entry different from its neighbours' (a multiplicative hash of the flat index), made once per shape"""
    x = ((np.arange(n * row, dtype=np.uint64) * 2654435761 + 12345) % 16777213).astype(np.float32).reshape(n, row) - 8388606.0
    x.setflags(write=False)
    return x


def _mask(kind, n, rs):
    if kind == "none":
        return np.zeros(n, dtype=np.uint8)
    if kind == "all":
        return np.ones(n, dtype=np.uint8)
    if kind == "alternating":
        return (np.arange(n) % 2).astype(np.uint8)
    return (rs.rand(n) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", MASKS)
def test_compact_rows(kind, n, row):
    from cgs_amd import kernels as K
    rs = np.random.RandomState(n * 7 + row)
    src = _src(n, row)
    mask = _mask(kind, n, rs)
    groups = {1: 1, 64: 4, 65: 5, 2048: 32}[n]
    flags = None
    chosen = mask.astype(bool)
    if kind == "take_all":
        flags = (np.arange(groups) % 2 == 1).astype(np.uint8) if groups > 1 else np.ones(1, dtype=np.uint8)
        chosen = chosen | np.repeat(flags.astype(bool), n // groups)
    picked = src[chosen]
    total = picked.shape[0]
    src_d, mask_d = _dev(src), _dev(mask)
    flags_d = None if flags is None else _dev(flags)
    # (offset, capacity): everything fits | clipped in the middle of the batch | nothing fits | a pool that is already full
    for offset, capacity in ((3, 3 + n + 2), (2, 2 + max(total // 2, 1)), (5, 5), (7, 4)):
        dst = torch.full((capacity, row), float("nan"), dtype=torch.float32, device=DEV)
        tot = K.compact_rows(src_d, mask_d, dst, offset, take_all=flags_d)
        assert tot.dtype == torch.int32 and int(tot.cpu()[0]) == total
        got = dst.cpu().numpy()
        room = max(min(total, capacity - offset), 0)
        want = np.full((capacity, row), np.nan, dtype=np.float32)
        want[offset:offset + room] = picked[:room]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (offset, capacity)


def test_compact_rows_of_an_image_shaped_batch_through_the_rejector():
    """[n, H, W, C] rows, the mask of the latest decide(), host take_all flags: what reject_fill_fused queues per round."""
    from cgs_amd.sampling import DeviceRejector
    rs = np.random.RandomState(3)
    b, groups = 16, 4
    x = rs.randn(b * groups, 4, 4, 3).astype(np.float32)
    sig = rs.uniform(0.05, 0.95, (b * groups, 1)).astype(np.float32)
    rej = DeviceRejector(DEV)
    mask, counts = rej.decide(_dev(sig), rs.rand(b * groups), shift_percent=100.0, groups=groups)
    m = mask.cpu().numpy().astype(bool)
    pool = torch.full((40, 4, 4, 3), float("nan"), dtype=torch.float32, device=DEV)
    tot = rej.compact(_dev(x), pool, 1, take_all=[False, False, True, False])
    m[2 * b:3 * b] = True
    assert int(tot.cpu()[0]) == m.sum() == counts[0] + counts[1] + b + counts[3]
    k = min(int(m.sum()), 39)
    got = pool.cpu().numpy()
    assert np.array_equal(got[1:1 + k], x[m][:k]) and np.isnan(got[0]).all() and np.isnan(got[1 + k:]).all()


def test_wrappers_refuse_what_the_kernels_would_not_survive():
    from cgs_amd import kernels as K
    from cgs_amd.lib import CgsError
    x = torch.zeros((4, 2), dtype=torch.float32, device=DEV)
    m = torch.zeros(4, dtype=torch.uint8, device=DEV)
    with pytest.raises(CgsError):
        K.compact_rows(x, m[:3], torch.zeros((4, 2), device=DEV), 0)                      # a mask shorter than the batch
    with pytest.raises(CgsError):
        K.compact_rows(x, m, torch.zeros((4, 3), device=DEV), 0)                          # rows of another length
    with pytest.raises(CgsError):
        K.compact_rows(x, m, torch.zeros((4, 2), device=DEV), -1)
    with pytest.raises(CgsError):
        K.compact_rows(x, m, torch.zeros((4, 2), device=DEV), 0, take_all=torch.zeros(3, dtype=torch.uint8, device=DEV))
    st = torch.zeros(1, dtype=torch.float64, device=DEV)
    s = torch.full((6,), 0.5, dtype=torch.float32, device=DEV)
    with pytest.raises(CgsError):
        K.drs_decide(s, torch.zeros(5, dtype=torch.float64, device=DEV), st)             # one uniform short
    with pytest.raises(CgsError):
        K.drs_decide(s, torch.zeros(6, dtype=torch.float64, device=DEV), st, groups=4)
    with pytest.raises(CgsError):
        K.drs_decide(s, torch.zeros(6, dtype=torch.float64, device=DEV), st, shift_percent=101.0)
