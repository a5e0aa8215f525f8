"""CPU-only checks of the Metropolis-Hastings statement the GPU tests are held to (tests/mh_cases.py): it IS the product's host
``IndependenceSampler.walk``, called once per segment in order, on every case of the table -- rows, counts, final d and final cnt;
``fill_model`` keeps the counters of ``evaluate.collaborate`` under both rules; the new entry points are declared, bound and built;
and the device class refuses what the kernel does not compute before it touches a device."""
import os
import re

import numpy as np
import pytest

import mh_cases as MC
from conftest import ROOT

NEW = ["cgs_mh_ws_bytes", "cgs_mh_walk", "cgs_gather_rows"]


# ---------------------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("kind", MC.KINDS + ["special"])
def test_statement_equals_the_host_sampler_on_every_case(kind):
    names = MC.SPECIALS if kind == "special" else [c[0] for c in MC.TABLE if c[3] == kind]
    assert names
    for name in names:
        case = MC.build(name)
        for call, host in zip(case["calls"], MC.host_walk(case)):
            ref = call["ref"]
            assert np.array_equal(ref["rows"], host["rows"]) and np.array_equal(ref["counts"], host["counts"]), name
            assert ref["d"] == host["d"] and ref["cnt"] == host["cnt"] and ref["fill"] == host["fill"], name
            assert ref["span"][1] == len(ref["rows"]) == int(np.maximum(ref["counts"], 0).sum())


def test_the_table_covers_what_it_claims():
    T = MC.TABLE
    assert len(T) == 7 * 3 * 7 and len(set(MC.case_names())) == len(T) + len(MC.SPECIALS)
    for b in MC.BS:
        assert {c[4] for c in T if c[1] == b} == set(MC.TS) and {min(c[5], 4) for c in T if c[1] == b} == {0, 1, 3, 4}
    for kind in MC.KINDS:
        assert {c[4] for c in T if c[3] == kind} == set(MC.TS) and {min(c[5], 4) for c in T if c[3] == kind} == {0, 1, 3, 4}
    assert {c[7] for c in T} == set(range(len(MC.SEEDS)))
    for t in MC.TS:
        assert {c[6] for c in T if c[4] == t} == set(range(1, t + 3))                   # start counters 1 .. T + 2
    tiny = MC.build([c[0] for c in T if c[3] == "tiny" and c[1] == 1000][0])["calls"][0]["sig"]
    assert np.any((tiny > 0) & (tiny < np.finfo(np.float32).tiny))                       # fp32 denormal scores
    const = MC.build("constant-50000")["calls"][0]
    assert const["ref"]["d"] == float(np.float32(0.37)) and const["ref"]["counts"][0] == 2381      # every proposal moved: 50 000 serial steps
    dec = MC.build([c[0] for c in T if c[3] == "decreasing" and c[1] == 1000 and c[2] == 1][0])
    assert len(MC.segment_moves(dec["calls"][0]["sig"], dec["calls"][0]["u"], float(dec["seed"]))[0]) < 40      # windows passed over whole
    inside, at_end = MC.build("full-inside"), MC.build("full-at-segment-end")
    assert inside["calls"][0]["ref"]["counts"].tolist()[2:] == [-1, -1] and inside["calls"][0]["ref"]["fill"] > inside["capacity"]
    assert at_end["calls"][0]["ref"]["fill"] == at_end["capacity"] and at_end["calls"][0]["ref"]["counts"].tolist()[2:] == [-1, -1]
    assert set(MC.build("full-on-entry")["calls"][0]["ref"]["counts"].tolist()) == {-1}


def test_stretch_form_equals_the_per_proposal_loop():
    """The statement tests proposals a stretch at a time; spelled out one proposal at a time in numpy fp32 scalars it gives the same moves."""
    f32 = np.float32
    for name in ("b129-g3-", "b65-g1-", "b64-g32-"):
        for full in [c[0] for c in MC.TABLE if c[0].startswith(name)]:
            case = MC.build(full)
            call, d = case["calls"][0], float(case["seed"])
            b = case["b"]
            s, u = call["sig"][:b], call["u"][:b]
            pos = []
            for i in range(b):
                with np.errstate(all="ignore"):
                    odds = f32(f32(s[i] * f32(1.0 - d)) / f32(f32(d) * f32(f32(1.0) - s[i])))
                alpha = odds if odds < f32(1.0) else f32(1.0)
                if not (u[i] > float(alpha)):
                    pos.append(i)
                    d = float(s[i])
            got, d2 = MC.segment_moves(s, u, float(case["seed"]))
            assert got.tolist() == pos and d2 == d, full


# ---------------------------------------------------------------------------------------------------------------- the fill loop
class _Scripted:
    """Scripted proposals (no device): batch i is rows [i * B, (i + 1) * B) of a fixed table; the score of a row is stored beside it."""

    def __init__(self, seed, B, width=3):
        self.rs, self.B, self.width = np.random.RandomState(seed), B, width
        self.made, self.scores = 0, {}

    def batch(self):
        x = (self.made * self.B + np.arange(self.B, dtype=np.float32))[:, None] + np.zeros(self.width, dtype=np.float32)
        s = self.rs.uniform(0.02, 0.98, (self.B, 1)).astype(np.float32)
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


@pytest.mark.parametrize("eval_size,B,min_eff,T,productive", [(64, 16, 0.2, 5, False), (64, 16, 0.5, 5, False), (50, 16, None, 2, False), (40, 8, 0.2, 20, False),
                                                              (64, 64, None, 20, True), (30, 30, None, 40, True), (8, 8, None, 3, True)])
def test_fill_model_keeps_collaborates_counters(eval_size, B, min_eff, T, productive):
    """Both counter rules: the image loops count every batch and take whole batches past eval_size / min_efficiency proposals; the 2-D
    loops count only the batches that yielded something."""
    from cgs_amd.evaluate import collaborate
    from cgs_amd.sampling import IndependenceSampler
    rs = np.random.RandomState(3)
    base = (np.arange(eval_size, dtype=np.float32)[:, None] - 1000 + np.zeros(3, dtype=np.float32), rs.uniform(0.02, 0.98, (eval_size, 1)).astype(np.float32))
    max_propose = eval_size / min_eff if min_eff else float("inf")
    a, s1 = _Scripted(5, B), IndependenceSampler(T=T)
    np.random.seed(11)
    s1.set_score_curr(0.4)
    want, acc, prop = MC.fill_model(a.stream(), lambda sig: s1.walk(sig, np.random.uniform(0, 1, size=len(sig))), eval_size, base, max_propose, productive)
    tail = np.random.rand(3)
    b, s2 = _Scripted(5, B), IndependenceSampler(T=T)
    np.random.seed(11)
    got, eff = collaborate(b.propose, b.score, s2, eval_size, 0.4, base=base, min_efficiency=min_eff, count_only_productive=productive)
    assert np.array_equal(np.random.rand(3), tail)
    assert got.shape == want.shape and np.array_equal(got, want) and eff == acc / prop
    assert np.array_equal(np.ravel(s2.d_curr), np.ravel(s1.d_curr)) and s2.cnt_chain == s1.cnt_chain and a.made == b.made
    if not productive:
        assert prop == eval_size + a.made * B
    if min_eff == 0.5:
        assert prop > max_propose                                        # the cutoff was crossed: some batch was taken whole
    if T == 40:
        assert prop < eval_size + a.made * B                             # some round yielded nothing and was not counted


# ---------------------------------------------------------------------------------------------------------------- ABI and the class
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
    assert lib.SIGNATURES["cgs_mh_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert l.cgs_version() >= 115
    assert "mh.hip" in open(os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc", "Makefile")).read()
    assert lib.built_from() == lib.source_hash()                         # cgs_source_sha covers the new file
    for cite in ("sampling/idpsampler.py:4-53", "nsgan/GAN.py:369-375,420-426"):
        assert cite in header


def test_workspace_queries_and_bad_arguments_launch_nothing():
    from cgs_amd import lib
    l = lib.load()
    assert int(l.cgs_mh_ws_bytes(64, 32)) == 64 * 4 and int(l.cgs_mh_ws_bytes(10000, 1)) == 40000 and int(l.cgs_mh_ws_bytes(1, 1)) == 8
    walk = lambda b, groups, T=5, B=0, cap=10: l.cgs_mh_walk(None, b, groups, None, T, B, None, None, None, cap, None, None, None, None, 0, None)
    for bad in ((0, 1), (1, 0), (-1, 1), (1, (1 << 20) + 1), (1 << 16, 1 << 15)):
        assert int(l.cgs_mh_ws_bytes(*bad)) == 0
        assert walk(*bad) == lib.EINVAL
    assert walk(64, 1, T=-1) == lib.EINVAL and walk(64, 1, B=-1) == lib.EINVAL and walk(64, 1, cap=-1) == lib.EINVAL
    assert walk(64, 1) == lib.EINVAL                                     # null pointers
    assert b"mh_walk" in l.cgs_last_error()
    for n, row, listed, cap in ((-1, 2, 4, 4), (4, 0, 4, 4), (4, (1 << 22) + 1, 4, 4), (4, 2, -1, 4), (4, 2, 4, -1), (1 << 30, 1 << 11, 4, 4)):
        assert l.cgs_gather_rows(None, n, row, None, listed, None, None, cap, None) == lib.EINVAL
    assert l.cgs_gather_rows(None, 4, 2, None, 4, None, None, 4, None) == lib.EINVAL                                           # null span


def test_device_class_refuses_a_float64_seed_and_an_unstarted_chain():
    import torch
    from cgs_amd.sampling import DeviceIndependenceSampler
    s = DeviceIndependenceSampler(T=20)
    assert s.d_curr is None and s.thin_period == 20 and s.burn_in == 0
    for bad in (np.float64(0.5), np.mean(np.full((4, 1), 0.5, dtype=np.float32), dtype=np.float64), np.full(1, 0.5, dtype=np.float32), None, "0.5"):
        with pytest.raises(TypeError) as e:
            s.set_score_curr(bad)
        if isinstance(bad, np.float64):
            assert "double" in str(e.value)
    with pytest.raises(TypeError):
        s.set_score_curr(torch.zeros(1, dtype=torch.float64))            # a tensor seed is a 1-element fp32 DEVICE tensor
    with pytest.raises(ValueError, match="start"):
        s.walk_device(torch.zeros(4), np.zeros(4))                       # unstarted: refused before any device work
    assert s.d_curr is None
