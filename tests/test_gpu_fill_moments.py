"""evaluate.collaborate_fused(..., moments=): the Frechet statistics of the accepted pool, accumulated on the device from the
scoring pass's features while the fill loop runs.  mnist, b = 16, G = 2, depth 2, K = 2, eval_size = 96, seeded.  ``proposer.result``
is wrapped to snapshot each round's device feature buffer, so the expected moments are numpy float64 over exactly the feature rows
of the returned samples; the bar is the derived bound of tests/test_gpu_pool_moments.py.

The cut-off branch (nsgan/GAN.py:410) needs no scores to be certain: the proposal counter starts at eval_size = 96, so with
min_efficiency = 0.9 the limit is 106.7 -- the first batch (counter 96) walks the chain, which emits at most 16 / 3 samples at thinning 2,
and every later batch (counter >= 112) is taken whole: at least 91 of the 96 rows come from the cut-off branch whatever D says."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N

ARCH, B, G, DEPTH, K, EVAL = "mnist", 16, 2, 2, 2, 96
U = 2.0 ** -53
_GAN = {}


def _gan():
    if "g" not in _GAN:
        from cgs_amd import ops
        from cgs_amd.model import GAN
        ops.reset_variables()
        _GAN["g"] = GAN(ARCH, batch_size=B, device=torch.device("cuda:0"), params=N.init_params(ARCH, 2019, True))
    return _GAN["g"]


def _fill(with_moments, min_efficiency=None):
    """One seeded fill -> (samples, efficiency, numpy RNG state after it, PoolMoments or None, [(features, rows) per sample order])."""
    from cgs_amd.evaluate import FusedProposer, collaborate_fused
    from cgs_amd.metrics import PoolMoments
    from cgs_amd.sampling import IndependenceSampler
    gc.collect()          # (dead proposers of earlier tests -- engines, streams, pinned buffers -- are finalised now, not at some allocation inside the fill)
    np.random.seed(77)
    prop = FusedProposer(_gan(), K, 0.1, batch=B, groups=G, depth=DEPTH, use_graph=False, features=with_moments)
    snaps = []
    if with_moments:
        inner = prop.result

        def result(k):
            r = inner(k)
            snaps.append((r[0].copy(), prop.feat_dev[k].cpu().numpy().copy()))
            return r
        prop.result = result
    pm = PoolMoments(prop.feat_width, prop.dev) if with_moments else None
    stats = {}
    out, eff = collaborate_fused(prop, IndependenceSampler(T=2), EVAL, 0.5, min_efficiency=min_efficiency, stats=stats, moments=pm)
    if with_moments:
        del prop.result   # (the wrapper refers to the proposer: without this the pair is a reference cycle that outlives the test)
    return out, eff, np.random.get_state(), pm, snaps, stats


def _rows_of(out, snaps):
    """The feature rows of the returned samples: every sample of ``out`` is a row of some round's images (found by exact match)."""
    feats = []
    imgs = np.concatenate([s[0] for s in snaps]).reshape(sum(len(s[0]) for s in snaps), -1)
    fall = np.concatenate([s[1] for s in snaps])
    flat = out.reshape(len(out), -1)
    for row in flat:
        hit = np.flatnonzero((imgs == row).all(1))
        assert hit.size >= 1
        feats.append(fall[hit[0]])
    return np.asarray(feats, dtype=np.float64)


@pytest.mark.parametrize("min_eff", [None, 0.9], ids=["chain", "cutoff"])
def test_moments_of_the_accepted_pool_and_an_undisturbed_fill(min_eff):
    out0, eff0, st0, _, _, stats0 = _fill(False, min_eff)
    out1, eff1, st1, pm, snaps, stats1 = _fill(True, min_eff)
    assert np.array_equal(out0, out1) and eff0 == eff1 and stats0["proposed"] == stats1["proposed"]
    assert st0[0] == st1[0] and np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:]
    if min_eff is not None:                                  # the too-inefficient branch was taken (module docstring): 1 chain batch + 6 whole ones
        assert EVAL + stats1["proposed"] > EVAL / min_eff and stats1["proposed"] <= 7 * B
    st = pm.state()
    assert st["n"] == pm.n == EVAL
    a = _rows_of(out1, snaps) - st["shift"]
    aa = np.abs(a)
    bound_s = 2.0 * (EVAL + 2) * U * aa.sum(0)
    bound_g = 2.0 * (EVAL + 2) * U * aa.T.dot(aa)
    rs = float((np.abs(st["sum"] - a.sum(0)) / np.maximum(bound_s, 1e-300)).max())
    rg = float((np.abs(st["gram"] - a.T.dot(a)) / np.maximum(bound_g, 1e-300)).max())
    print(f"\n[fill moments {min_eff}] rounds {stats1['rounds']}, proposed {stats1['proposed']}; worst |delta| / bound: sum {rs:.3g}, gram {rg:.3g}")
    assert rs <= 2.0 and rg <= 2.0
    assert np.array_equal(st["gram"], st["gram"].T)


def test_base_without_features_and_a_proposer_without_features_are_refused():
    from cgs_amd.evaluate import FusedProposer, collaborate_fused
    from cgs_amd.metrics import PoolMoments
    from cgs_amd.sampling import IndependenceSampler
    prop = FusedProposer(_gan(), K, 0.1, batch=B, groups=G, depth=DEPTH, use_graph=False, features=True)
    pm = PoolMoments(prop.feat_width, prop.dev)
    base = (np.zeros((B, 28, 28, 1), np.float32), np.full((B, 1), 0.5, np.float32))
    state = np.random.get_state()
    with pytest.raises(ValueError):
        collaborate_fused(prop, IndependenceSampler(T=2), EVAL, 0.5, base=base, moments=pm)
    plain = FusedProposer(_gan(), K, 0.1, batch=B, groups=G, depth=1, use_graph=False)
    with pytest.raises(ValueError):
        collaborate_fused(plain, IndependenceSampler(T=2), EVAL, 0.5, moments=pm)
    assert pm.n == 0 and np.array_equal(np.random.get_state()[1], state[1])          # refused before any draw or launch


def test_base_with_features_contributes_its_accepted_rows():
    from cgs_amd.evaluate import FusedProposer, collaborate_fused
    from cgs_amd.metrics import PoolMoments
    from cgs_amd.sampling import IndependenceSampler
    prop = FusedProposer(_gan(), K, 0.1, batch=B, groups=G, depth=DEPTH, use_graph=False, features=True)
    rs = np.random.RandomState(4)
    n0 = 400                                                                          # enough base proposals to fill the whole set
    base = (rs.uniform(-1, 1, (n0, 28, 28, 1)).astype(np.float32), rs.uniform(0.3, 0.7, (n0, 1)).astype(np.float32),
            rs.randn(n0, prop.feat_width).astype(np.float32))
    np.random.seed(5)
    want = IndependenceSampler(T=2)
    want.set_score_curr(0.5)
    rows = want.walk(base[1])[:EVAL]
    assert len(rows) == EVAL
    np.random.seed(5)
    pm = PoolMoments(prop.feat_width, prop.dev)
    out, _ = collaborate_fused(prop, IndependenceSampler(T=2), EVAL, 0.5, base=base, moments=pm)
    assert np.array_equal(out, base[0][rows])
    st = pm.state()
    a = base[2][rows].astype(np.float64) - st["shift"]
    assert st["n"] == EVAL and np.abs(st["gram"] - a.T.dot(a)).max() <= 4.0 * (EVAL + 2) * U * np.abs(a).T.dot(np.abs(a)).max()


def test_real_moments_takes_whole_batches_and_drops_the_padding():
    from cgs_amd.evaluate import FusedProposer
    from cgs_amd.metrics import PoolMoments, moments_mean_cov
    prop = FusedProposer(_gan(), K, 0.1, batch=B, groups=G, depth=1, use_graph=False, features=True)
    x = np.random.RandomState(8).uniform(-1, 1, (48, 28, 28, 1)).astype(np.float32)
    with pytest.raises(ValueError):
        prop.real_moments(x[:40], PoolMoments(prop.feat_width, prop.dev))             # two and a half batches
    with pytest.raises(ValueError):
        prop.score_real(x[:40])
    pm = prop.real_moments(x, PoolMoments(prop.feat_width, prop.dev))                 # one full round + one padded round
    assert pm.n == 48
    eng = prop.engines[0]
    feats = []
    for i in range(0, 48, B):                                                         # per-batch statistics: each batch on its own, padded with itself
        xb = torch.from_numpy(np.concatenate([x[i:i + B]] * G)).to(prop.dev)
        feats.append(eng.score_with_features(xb)[1][:B].cpu().double().numpy())
    feats = np.concatenate(feats)
    mean, cov = moments_mean_cov(pm.state())
    ref = np.cov(feats, rowvar=False)
    # (the reference rows come from other launches -- a batch at another position of the round -- so they agree with the accumulated
    # ones to fp32 forward accuracy, README's 1e-4 for one forward evaluation, not to the double arithmetic of the accumulation)
    assert np.abs(mean - feats.mean(0)).max() <= 1e-4 * np.abs(feats.mean(0)).max()
    assert np.abs(cov - ref).max() <= 1e-4 * np.abs(ref).max()
