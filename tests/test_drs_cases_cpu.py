"""CPU-only checks of the rejection-sampling statement the GPU tests are held to (tests/drs_cases.py): it IS the product's host
Rejector and the oracle's, bit for bit; its percentile is numpy's; its grouped form is the per-batch form called in order; its cases
keep every uniform clear of its row's acceptance probability; and ``evaluate.reject_fill`` keeps the reference loops' counters."""
import os
import re

import numpy as np
import pytest

import drs_cases as DC
from conftest import ROOT, load_golden
from oracle import sampling_ref as S

NEW = ["cgs_drs_ws_bytes", "cgs_drs_decide", "cgs_drs_set_max", "cgs_compact_rows_ws_bytes", "cgs_compact_rows"]


# ---------------------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("kind", DC.KINDS)
def test_statement_equals_the_host_rejector_and_the_oracle_bit_for_bit(kind):
    from cgs_amd.sampling import Rejector
    for (b, groups) in DC.SHAPES:
        for q in DC.PERCENTS:
            for call in (0, 1):
                c = DC.build(b, groups, q, kind, call)
                host, orc = Rejector(), S.RejectorRef()
                host.D_tilde_M = orc.D_tilde_M = c["M0"]
                for g in range(groups):
                    rows = slice(g * b, (g + 1) * b)
                    P, n = host.acceptance_probability(c["sig"][rows].reshape(b, 1), DC.EPS, q)
                    assert n == b and np.array_equal(np.atleast_1d(P), c["ref"]["P"][rows]), (b, groups, q, call, g)
                    assert host.D_tilde_M == c["ref"]["M"][g]
                    state = np.random.RandomState(7)
                    m, Po = orc.accept_mask(c["sig"][rows].reshape(b, 1), DC.EPS, q, rng=state)
                    assert np.array_equal(np.atleast_1d(Po), c["ref"]["P"][rows]) and orc.D_tilde_M == c["ref"]["M"][g]
                    assert np.array_equal(m, np.random.RandomState(7).rand(b) < c["ref"]["P"][rows])
                assert np.array_equal(c["ref"]["counts"], c["ref"]["mask"].reshape(groups, b).sum(axis=1))


def test_statement_reproduces_the_committed_golden_masks():
    g = load_golden("g6_rejector.npz")
    for tag, q in (("p60", 60.0), ("p100", 100.0), ("none", None)):
        rs, M = np.random.RandomState(2019), 0.0
        for c in range(3):
            r = DC.decide_batch(g[f"{tag}_sig{c}"], rs.rand(257), M, DC.EPS, q)
            M = r["M"]
            assert np.array_equal(r["mask"], g[f"{tag}_mask{c}"]) and M == g[f"{tag}_M{c}"][0]


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, 1000])
def test_percentile_equals_live_numpy(n):
    rs = np.random.RandomState(n)
    F = rs.randn(n) * 5
    F[rs.randint(n, size=n // 3)] = F[0]                                 # ties
    for q in (0.0, 12.5, 37.5, 50.0, 60.0, 99.9, 100.0, 100.0 * (n - 1.5) / max(n - 1, 1) if n > 1 else 3.0):
        assert DC.percentile_linear(F, q)[0] == np.percentile(F, q), (n, q)


@pytest.mark.parametrize("b,groups", [(64, 32), (64, 3), (1000, 2), (5, 7)])
def test_grouped_form_equals_sequential_batches(b, groups):
    rs = np.random.RandomState(b + groups)
    sig = rs.uniform(0.001, 0.999, b * groups).astype(np.float32)
    sig[: b] *= 0.5                                                      # a bound that rises over the batches
    u = rs.rand(b * groups)
    for q in DC.PERCENTS:
        got = DC.decide(sig, u, -1.0, groups, DC.EPS, q)
        M = -1.0
        for g in range(groups):
            rows = slice(g * b, (g + 1) * b)
            one = DC.decide_batch(sig[rows], u[rows], M, DC.EPS, q)
            M = one["M"]
            assert M == got["M"][g] and np.array_equal(one["P"], got["P"][rows]) and np.array_equal(one["mask"], got["mask"][rows])
            assert int(one["mask"].sum()) == got["counts"][g]
        assert np.all(np.diff(got["M"]) >= 0)


def test_every_case_keeps_its_uniforms_clear_of_the_acceptance_probabilities():
    """The condition under which the GPU tests may demand mask equality with no exception: no row has |u - P| within 8 bounds."""
    worst = np.inf
    for case in DC.all_cases():
        for call in (0, 1):
            c = DC.build(*case, call=call)
            assert c["margin_ok"], (case, call)
            assert np.all(np.isfinite(c["dP"])) and np.all(c["dP"] > 0) and np.all(c["dP"] < 1e-5), (case, call)
            worst = min(worst, float(np.min(np.abs(c["u"] - c["ref"]["P"]) / c["dP"])))
    assert worst > DC.MARGIN
    assert len(DC.all_cases()) == 11 * 5 * 7


# ---------------------------------------------------------------------------------------------------------------- the fill loop
class _Scripted:
    """Scripted proposals (no device): batch i is rows [i * B, (i + 1) * B) of a fixed table; the score of a row is stored beside it."""

    def __init__(self, seed, B, width=3, lo=0.02, hi=0.98):
        self.rs, self.B, self.width, self.lo, self.hi = np.random.RandomState(seed), B, width, lo, hi
        self.made, self.scores = 0, {}

    def batch(self):
        x = (self.made * self.B + np.arange(self.B, dtype=np.float32))[:, None] + np.zeros(self.width, dtype=np.float32)
        s = self.rs.uniform(self.lo, self.hi, (self.B, 1)).astype(np.float32)
        self.scores[self.made] = s
        self.made += 1
        return x, s

    def propose(self):
        return self.batch()[0]

    def score(self, x):
        return self.scores[int(x[0, 0]) // self.B]

    def stream(self):
        while True:
            yield self.batch()


@pytest.mark.parametrize("eval_size,B,min_eff,hi", [(64, 16, 0.2, 0.98), (64, 16, 0.5, 0.98), (50, 16, None, 0.98), (40, 8, 0.2, 0.999999), (16, 16, 0.2, 0.5)])
def test_reject_fill_keeps_the_image_loops_counters(eval_size, B, min_eff, hi):
    """nsgan form: every batch counts as proposed; past eval_size / min_efficiency proposals whole batches are taken unseen."""
    from cgs_amd.evaluate import reject_fill
    from cgs_amd.sampling import Rejector
    rs = np.random.RandomState(3)
    base = (np.arange(eval_size, dtype=np.float32)[:, None] - 1000 + np.zeros(3, dtype=np.float32), rs.uniform(0.02, hi, (eval_size, 1)).astype(np.float32))
    real_max = np.float32(0.9)
    max_propose = eval_size / min_eff if min_eff else float("inf")
    a, r1 = _Scripted(5, B, hi=hi), Rejector()
    np.random.seed(11)
    r1.set_score_max(real_max)
    want, acc, prop = DC.fill_model(a.stream(), lambda x, s: r1.sampling(x, s, shift_percent=100.0), eval_size, base, max_propose)
    tail = np.random.rand(3)
    b, r2 = _Scripted(5, B, hi=hi), Rejector()
    np.random.seed(11)
    got, eff = reject_fill(b.propose, b.score, r2, eval_size, real_max, base=base, min_efficiency=min_eff)
    assert np.array_equal(np.random.rand(3), tail)
    assert got.shape == want.shape and np.array_equal(got, want) and eff == acc / prop and r2.D_tilde_M == r1.D_tilde_M
    assert a.made == b.made and prop == eval_size + a.made * B
    if min_eff == 0.5:
        assert prop > max_propose                                        # the cutoff was crossed: some batch was taken whole


@pytest.mark.parametrize("eval_size,hi", [(64, 0.98), (30, 0.9999999), (8, 0.6)])
def test_reject_fill_keeps_the_2d_loops_counters(eval_size, hi):
    """synthetic form: eval_size proposals per round, a round that yields nothing is not counted, no efficiency cutoff."""
    from cgs_amd.evaluate import reject_fill
    from cgs_amd.sampling import Rejector
    rs = np.random.RandomState(4)
    base = (rs.randn(eval_size, 2).astype(np.float32), rs.uniform(0.02, hi, (eval_size, 1)).astype(np.float32))
    a, r1 = _Scripted(6, eval_size, width=2, hi=hi), Rejector()
    np.random.seed(12)
    r1.set_score_max(np.float32(0.95))
    want, acc, prop = DC.fill_model(a.stream(), lambda x, s: r1.sampling(x, s, shift_percent=100.0), eval_size, base, productive_only=True)
    b, r2 = _Scripted(6, eval_size, width=2, hi=hi), Rejector()
    np.random.seed(12)
    got, eff = reject_fill(b.propose, b.score, r2, eval_size, np.float32(0.95), base=base, count_only_productive=True)
    assert np.array_equal(got, want) and eff == acc / prop and a.made == b.made


def test_reject_fill_stores_a_batch_even_when_nothing_was_accepted_before():
    """Where the image loop of the reference leaves uninitialised rows (its store is skipped while the count is zero), reject_fill stores."""
    from cgs_amd.evaluate import reject_fill

    class Script:
        def __init__(self):
            self.calls = 0

        def set_score_max(self, m):
            pass

        def sampling(self, x, s, epsilon=1e-8, shift_percent=60.0):
            self.calls += 1
            return x[:0] if self.calls == 1 else x[:3]

    base = (np.full((4, 2), -1.0, dtype=np.float32), np.full((4, 1), 0.5, dtype=np.float32))
    n = [0]

    def propose():
        n[0] += 1
        return np.full((4, 2), float(n[0]), dtype=np.float32)
    got, eff = reject_fill(propose, lambda x: np.full((4, 1), 0.5, dtype=np.float32), Script(), 4, 0.9, base=base)
    assert np.array_equal(got[:, 0], [1, 1, 1, 2]) and eff == 6 / 12


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_bindings_and_library_agree_on_the_new_entry_points():
    import ctypes
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    l = lib.load()
    for name in NEW:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert lib.SIGNATURES["cgs_drs_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert l.cgs_version() >= 114
    assert "drs.hip" in open(os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc", "Makefile")).read()
    assert lib.built_from() == lib.source_hash()                         # cgs_source_sha covers the new file
    for cite in ("sampling/rejector.py:16-34", "rejector.py:11-14", "nsgan/GAN.py:324-338"):
        assert cite in header


def test_workspace_queries_and_bad_arguments_launch_nothing():
    from cgs_amd import lib
    l = lib.load()
    assert int(l.cgs_drs_ws_bytes(64, 32)) == (1 + 32 + 64 * 32) * 8 and int(l.cgs_drs_ws_bytes(10000, 1)) == 10002 * 8
    for bad in ((0, 1), (1, 0), (-1, 1), (1, (1 << 20) + 1), (1 << 16, 1 << 15)):
        assert int(l.cgs_drs_ws_bytes(*bad)) == 0
        assert l.cgs_drs_decide(None, bad[0], bad[1], None, 1e-8, 60.0, None, None, None, None, None, None, 0, None) == lib.EINVAL
    for q, eps in ((100.5, 1e-8), (float("nan"), 1e-8), (60.0, 0.0), (60.0, -1.0)):
        assert l.cgs_drs_decide(None, 64, 1, None, eps, q, None, None, None, None, None, None, 0, None) == lib.EINVAL
    assert l.cgs_drs_decide(None, 64, 1, None, 1e-8, 60.0, None, None, None, None, None, None, 0, None) == lib.EINVAL      # null pointers
    assert l.cgs_drs_set_max(None, 0, None, None) == lib.EINVAL and l.cgs_drs_set_max(None, 5, None, None) == lib.EINVAL
    assert int(l.cgs_compact_rows_ws_bytes(2048)) == 2048 * 4 and int(l.cgs_compact_rows_ws_bytes(0)) == 0
    for n, row, groups, off, cap in ((-1, 2, 1, 0, 4), (4, 0, 1, 0, 4), (4, (1 << 22) + 1, 1, 0, 4), (5, 2, 2, 0, 4), (4, 2, 0, 0, 4), (4, 2, 1, -1, 4), (4, 2, 1, 0, -1)):
        assert l.cgs_compact_rows(None, n, row, None, None, groups, None, off, cap, None, None, 0, None) == lib.EINVAL
    assert l.cgs_compact_rows(None, 4, 2, None, None, 1, None, 0, 4, None, None, 0, None) == lib.EINVAL                      # null total
