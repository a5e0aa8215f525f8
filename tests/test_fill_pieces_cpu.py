"""The pieces the evaluation fill loops share (cgs_amd.evaluate: ``_FillCounter``, ``_draw_round``; csrc/rows.h: the gather's launch plan),
held on the CPU to what every leg's loop relies on: rounds drawn ahead and rewound leave the global numpy stream, and hand every batch the
uniforms, of the reference's one-batch-at-a-time loop -- bit for bit; the counter counts as ``tests/mh_cases.fill_model`` does."""
import os
import subprocess

import numpy as np
import pytest

import mh_cases as MC
from conftest import ROOT

B, ZDIM, EVAL = 16, 5, 80                                                # five batches fill the set; the cut-offs fall at batch 1 (0.9), 2 (0.76), 20 (0.2)


def _images(z):
    return np.tanh(z[:, :3]).astype(np.float32)


def _sigmoids(z):
    return (1.0 / (1.0 + np.exp(-z.sum(1, keepdims=True)))).astype(np.float32)


def _recording(leg, record):
    """The leg's host sampler, noting per batch the uniforms it drew and the rows it let through.  It draws as the reference does (the
    chain one scalar per proposal, idpsampler.py:50; the rejector one vector, rejector.py:33); the note is the leg's vector draw from the
    same stream position, which must leave the stream where the sampler's own draws leave it."""
    from cgs_amd.sampling import IndependenceSampler, Rejector

    def noted(vector_draw, sample):
        before = np.random.get_state()
        u = vector_draw()
        after_vector = np.random.get_state()
        np.random.set_state(before)
        acc = sample()
        _same_state(np.random.get_state(), after_vector)
        record.append((u, acc.shape[0]))
        return acc

    if leg == "chain":
        class Chain(IndependenceSampler):
            def sampling(self, samples, sigmoids, uniforms=None):
                return noted(lambda: np.random.uniform(0, 1, size=len(samples)), lambda: IndependenceSampler.sampling(self, samples, sigmoids))
        return Chain(T=2)

    class Rej(Rejector):
        def sampling(self, samples, sigmoids, epsilon=1e-8, shift_percent=60.0, ranking=None):
            return noted(lambda: np.random.rand(len(samples)), lambda: Rejector.sampling(self, samples, sigmoids, epsilon, shift_percent))
    return Rej()


def _same_state(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("min_eff", [None, 0.2, 0.76, 0.9])
@pytest.mark.parametrize("G", [1, 3, 4])
@pytest.mark.parametrize("leg", ["chain", "drs"])
def test_rounds_drawn_ahead_and_rewound_are_the_one_batch_loop(leg, G, min_eff):
    from cgs_amd import evaluate as E
    last, record = {}, []

    def propose():
        last["z"] = np.random.uniform(-1, 1, [B, ZDIM]).astype(np.float32)
        return _images(last["z"])

    score = lambda batch: _sigmoids(last["z"])
    sampler = _recording(leg, record)
    np.random.seed(23)
    with np.errstate(all="ignore"):
        if leg == "chain":
            want, eff = E.collaborate(propose, score, sampler, EVAL, 0.45, min_efficiency=min_eff)
        else:
            want, eff = E.reject_fill(propose, score, sampler, EVAL, 0.9, min_efficiency=min_eff)
    left = np.random.get_state()
    # the fused loops' form: rounds of G batches drawn `depth` ahead, counted a round at a time from the counts the loop above saw
    draw, blank = (E._UNIFORM, np.zeros(B)) if leg == "chain" else (E._RAND, None)
    np.random.seed(23)
    C = E._FillCounter(EVAL, min_eff)
    drawn, pending, seen, stop = 0, [], 0, None
    while stop is None:
        while len(pending) < 2:
            pending.append(E._draw_round(C, drawn, G, B, ZDIM, draw, blank))
            drawn += G
        z, us, flags, states = pending.pop(0)
        assert z.shape == (G * B, ZDIM) and z.dtype == np.float32 and len(us) == len(flags) == len(states) == G
        counts = []
        for j in range(G):
            i = seen + j
            assert flags[j] == (not C.through_ahead(i, B))
            if flags[j]:                                                 # past the budget: no draw, the leg's blank, the batch whole
                assert us[j] is blank
                counts.append(B)
            elif i < len(record):                                        # (a batch past the stopping one has no counterpart)
                assert us[j].dtype == np.float64 and np.array_equal(us[j], record[i][0])
                counts.append(record[i][1])
            else:
                counts.append(0)
        through_before = [C.cnt_propose + k * B < C.max_propose for k in range(G)]
        assert through_before == [not f for f in flags]                  # the rule known ahead is the rule the loop meets
        stop = C.add_round(counts, B)
        seen += G
    np.random.set_state(states[stop])
    _same_state(np.random.get_state(), left)
    assert C.efficiency == eff and C.cnt >= EVAL and want.shape[0] == EVAL
    n_through = sum(1 for i in range(seen - G + stop + 1) if C.through_ahead(i, B))
    assert n_through == len(record)                                      # the loop showed its sampler exactly the batches inside the budget


def _scripted(counts, b):
    for i, c in enumerate(counts):
        yield np.full((b, 1), float(i), dtype=np.float32), np.full(b, c)


@pytest.mark.parametrize("G", [1, 3, 4])
@pytest.mark.parametrize("name,min_eff,productive,first,counts", [
    ("cut-off inside a round", 0.2, False, 2, [0, 1, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0, 3, 0, 0, 0, 0, 1, 0, 0] + [5] * 12),
    ("cut-off at the start", 0.9, False, 0, [7] * 12),
    ("no cut-off, filled inside a round", None, False, 5, [3, 0, 9, 16, 2, 11, 0, 14, 16, 9, 4, 8]),
    ("productive only, rounds that yield nothing", None, True, 0, [0, 0, 0, 0, 9, 0, 0, 12, 0, 0, 0, 0, 0, 16, 0, 16, 0, 0, 14, 5, 0, 10]),
    ("productive only, a first pass that fills the set", None, True, EVAL, [1]),
])
def test_counter_rule_counts_as_the_fill_model(name, min_eff, productive, first, counts, G):
    from cgs_amd.evaluate import _FillCounter
    used = []

    def batches():
        for i, batch in enumerate(_scripted(counts, B)):
            used.append(i)
            yield batch
    base = (np.zeros((EVAL, 1), np.float32), np.full(EVAL, first))
    max_propose = EVAL / min_eff if min_eff else float("inf")
    _, accepted, proposed = MC.fill_model(batches(), lambda s: range(int(s[0])), EVAL, base, max_propose, productive)
    C = _FillCounter(EVAL, min_eff, productive)
    assert C.max_propose == max_propose
    C.start(first)
    stop, at = None, 0
    while not C.full:
        assert at < len(counts), "the script ran out"
        if productive:                                                   # (these loops take one batch per round and never draw ahead)
            assert C.through()
            stop = at if C.add(counts[at], B) else None
            at += 1
            continue
        rnd = []
        for k, c in enumerate(counts[at:at + G]):
            assert C.through_ahead(at + k, B) == (C.cnt_propose + k * B < C.max_propose)
            rnd.append(c if C.through_ahead(at + k, B) else B)
        j = C.add_round(rnd, B)
        stop = None if j is None else at + j
        at += G
    assert (C.cnt, C.cnt_propose) == (accepted, proposed)
    assert stop == (used[-1] if used else None)
    assert C.efficiency == accepted / proposed


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gather_launch_plan_under_the_host_sanitizers(tmp_path):
    """tests/abi/rows_plan_check.hip, a stand-alone program over csrc/rows.h's host side, built with the host's address and undefined-behaviour
    sanitizers and run on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a host-sanitizer run: meant for the GPU-less build container")
    exe = tmp_path / "rows_plan_check"
    r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=all", f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'collaborative-gan-sampling_amd', 'csrc')}",
                        os.path.join(ROOT, "tests", "abi", "rows_plan_check.hip"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "ROWS_PLAN_OK" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
