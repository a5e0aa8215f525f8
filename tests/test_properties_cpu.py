"""Property tests (hypothesis) for the host-side accept/reject samplers and the update rule: invariants that hold for
any input, complementing the golden-vector tests."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from cgs_amd.sampling import IndependenceSampler, PolicyAdaptive, Rejector
from oracle import sampling_ref as S

sigm = st.lists(st.floats(min_value=1e-6, max_value=1 - 1e-6), min_size=1, max_size=200)


@settings(max_examples=60, deadline=None)
@given(sig=sigm, seed=st.integers(0, 2 ** 31 - 1), pct=st.sampled_from([None, 0.0, 60.0, 100.0]))
def test_rejector_mask_equals_oracle_and_is_monotone_in_state(sig, seed, pct):
    s = np.asarray(sig, dtype=np.float32).reshape(-1, 1)
    samples = np.arange(len(sig), dtype=np.float32).reshape(-1, 1)
    r, o = Rejector(), S.RejectorRef()
    for _ in range(2):                                   # two consecutive calls: the running bound persists
        np.random.seed(seed)
        good = r.sampling(samples, s, shift_percent=pct)
        np.random.seed(seed)
        mask, P = o.accept_mask(s, shift_percent=pct)
        assert np.array_equal(r.last_accept, mask)       # bit-exact with the pinned oracle
        assert np.array_equal(good[:, 0], samples[mask, 0])
        assert r.D_tilde_M == o.D_tilde_M and r.D_tilde_M >= 0.0          # bound never decreases (starts at logit(.5) = 0)
        assert np.all((P >= 0) & (P <= 1))
    if pct == 100.0:                                     # shift by the max => max P is exactly 1/2
        assert abs(np.max(P) - 0.5) < 1e-12


@settings(max_examples=60, deadline=None)
@given(sig=sigm, seed=st.integers(0, 2 ** 31 - 1), T=st.integers(0, 25), d0=st.floats(min_value=0.01, max_value=0.99))
def test_independence_sampler_matches_oracle_and_thinning(sig, seed, T, d0):
    s = np.asarray(sig, dtype=np.float64).reshape(-1, 1)
    samples = np.arange(len(sig), dtype=np.float32).reshape(-1, 1)
    mh, o = IndependenceSampler(T=T), S.IndependenceSamplerRef(T=T)
    mh.set_score_curr(d0); o.d_curr = d0
    np.random.seed(seed)
    got = mh.sampling(samples, s)
    np.random.seed(seed)
    want = o.accepted_indices(s)
    assert list(got[:, 0].astype(int)) == want if len(want) else got.shape[0] == 0
    assert len(want) <= len(sig) // (T + 1) + 1          # at most one sample per thinning period
    assert all(a <= b for a, b in zip(want, want[1:]))   # the chain only moves forward


@settings(max_examples=40, deadline=None)
@given(n=st.integers(1, 40), steps=st.integers(1, 6), rate=st.floats(min_value=1e-3, max_value=1.0),
       seed=st.integers(0, 10 ** 6), method=st.sampled_from(["sgd", "momentum", "ladam"]))
def test_policy_matches_oracle_state_machine(n, steps, rate, seed, method):
    rs = np.random.RandomState(seed)
    th = rs.randn(n, 2).astype(np.float32)
    p, o = PolicyAdaptive(rate, method), S.Policy(rate, method)
    ref = th.copy()
    for _ in range(steps):
        g, l = rs.randn(n, 2).astype(np.float32), rs.randn(n).astype(np.float32)
        p.apply_gradient(th, g, l)
        ref = o.step(ref, g, l).astype(np.float32)
        np.testing.assert_array_equal(th, ref)
    p.reset_moving_average()
    assert p.momentum is None and p.mean_square is None and p.loss is None


# ---- the weight-gradient planner (csrc/wgrad.hip, wgrad_geom) through its host-side query: no GPU needed ----------------------
def _wgrad_shapes():
    """The shapes tests/test_gpu_train_kernels.py places on the planner's edges, then a seeded sweep."""
    out = [(64, 64, 64, 3, 64, 5, 5, 2, 2), (8, 64, 64, 4, 32, 3, 3, 1, 1), (43, 16, 48, 4, 8, 3, 3, 1, 1), (33, 16, 16, 8, 16, 3, 3, 1, 1),
           (2, 32, 32, 8, 16, 3, 3, 1, 1), (3, 1, 683, 8, 16, 3, 3, 1, 1), (1, 3, 5, 8, 16, 3, 3, 1, 1), (64, 1, 1, 6272, 1024, 1, 1, 1, 1),
           (1, 1, 1, 1, 1, 1, 1, 1, 1), (128, 1, 1, 1, 1, 1, 1, 1, 1), (129, 1, 1, 1, 1, 1, 1, 1, 1)]
    rs = np.random.RandomState(2024)
    while len(out) < 4000:
        B = int(rs.choice([1, 2, 3, 5, 16, 33, 64, 130, 1024]))
        H, W = int(rs.randint(1, 70)), int(rs.randint(1, 70))
        cin, cout = int(rs.choice([1, 3, 4, 43, 64, 127, 128, 129, 130, 257, 512])), int(rs.choice([1, 3, 4, 64, 127, 128, 129, 130, 512]))
        kh, kw, sh, sw = int(rs.randint(1, 6)), int(rs.randint(1, 6)), int(rs.randint(1, 4)), int(rs.randint(1, 4))
        if B * H * W * max(cin, cout) < 2 ** 28:
            out.append((B, H, W, cin, cout, kh, kw, sh, sw))
    return out


def test_wgrad_plan_covers_every_pixel_once_and_matches_the_library():
    from cgs_amd import lib
    from wgrad_plan import SPLIT_CAP, WK, ceil_div, lib_splits, lib_ws_bytes, wgrad_plan
    l = lib.load()
    seen = set()
    for shape in _wgrad_shapes():
        B, H, W, cin, cout, kh, kw, sh, sw = shape
        p = wgrad_plan(*shape)
        nbytes = lib_ws_bytes(l, *shape)
        slab = 4 * kh * kw * cin * ceil_div(cout, 4) * 4
        assert nbytes > 0 and nbytes % slab == 0, shape                     # a positive whole number of slabs
        splits = nbytes // slab
        assert 1 <= splits <= SPLIT_CAP, (shape, splits)
        assert splits == lib_splits(l, *shape) == p.splits, (shape, splits, p)   # the restatement IS the library's plan
        if p.M <= 128:
            assert splits == 1, shape
        # the slabs tile the M pixels: none dropped, none counted twice, the last slab not empty
        assert p.m_per_split % WK == 0 and p.m_per_split > 0, (shape, p)
        assert p.splits * p.m_per_split >= p.M > (p.splits - 1) * p.m_per_split, (shape, p)
        seen.add((splits == SPLIT_CAP, splits == 1, p.M % p.m_per_split == 0))
    assert {s[0] for s in seen} == {True, False} and {s[1] for s in seen} == {True, False} and {s[2] for s in seen} == {True, False}


def test_wgrad_plan_refuses_non_positive_arguments():
    from cgs_amd import lib
    l = lib.load()
    good = [2, 8, 8, 4, 4, 3, 3, 2, 2]
    assert l.cgs_conv_wgrad_ws_bytes(*good) > 0
    for i in range(9):
        for bad in (0, -1):
            args = list(good)
            args[i] = bad
            assert l.cgs_conv_wgrad_ws_bytes(*args) == 0, args
