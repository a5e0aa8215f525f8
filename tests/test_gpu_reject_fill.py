"""The DRS leg end to end: ``evaluate.reject_fill_fused`` on the MNIST net against ``evaluate.reject_fill`` with the host Rejector fed
the SAME device scores one batch at a time, and ``synthetic.evaluate_calibrated`` against the host Rejector / ``collaborate`` by hand.

mnist, b = 16, eval_size = 256, G = 1 and 4, depth 2, seeded.  ``proposer.launch`` is wrapped to snapshot each round's z, images and
scores, so the one-batch loop replays exactly the rows the fused loop decided on: equality of the pools is then bit equality, and the two
loops can only differ where a uniform falls within ~1e-15 of an acceptance probability.  The bound starts at logit(0.99), above every
score of the untrained D, so batches are thinned instead of reduced to their best row.  min_efficiency = 0.76 puts the cutoff at
336.8 proposals: the counter starts at 256 and moves by 16, so batches 0..5 meet the rejector and the cutoff falls inside round 2 of
G = 4 (two batches decided, two taken whole)."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N
from oracle import sampling_ref as S

DEV = torch.device("cuda:0")
ARCH, B, EVAL, REAL_MAX = "mnist", 16, 256, 0.99
_GAN = {}


def _gan():
    if "g" not in _GAN:
        from cgs_amd import ops
        from cgs_amd.model import GAN
        ops.reset_variables()
        _GAN["g"] = GAN(ARCH, batch_size=B, device=DEV, params=N.init_params(ARCH, 2019, True))
    return _GAN["g"]


def _base():
    if "base" not in _GAN:
        from cgs_amd.engine import RefineEngine
        one = RefineEngine(ARCH, _gan().build_variables(), EVAL, DEV, bn_groups=EVAL // B)
        z = torch.from_numpy(np.random.RandomState(8).uniform(-1, 1, (EVAL, 62)).astype(np.float32)).to(DEV)
        img = one.generate(z).clone()
        _GAN["base"] = (img, one.score(img).clone())
    return _GAN["base"]


def _fused(G, min_eff, features=False):
    from cgs_amd.evaluate import FusedProposer, reject_fill_fused
    from cgs_amd.metrics import CalibrationStats, PoolMoments
    from cgs_amd.sampling import DeviceRejector
    gc.collect()
    base = _base()
    prop = FusedProposer(_gan(), 1, 0.1, batch=B, groups=G, depth=2, use_graph=False, features=features)
    rounds, inner = [], prop.launch

    def launch(z, **kw):
        k = inner(z, **kw)
        prop.done[k].synchronize()
        rounds.append((np.array(z), prop.img_dev[k].cpu().numpy().copy(), prop.sig_dev[k].cpu().numpy().copy(),
                       prop.feat_dev[k].cpu().numpy().copy() if features else None))
        return k
    prop.launch = launch
    rej = DeviceRejector(DEV)
    kw, stats = {}, {}
    if features:
        from cgs_amd.engine import RefineEngine
        one = RefineEngine(ARCH, _gan().build_variables(), EVAL, DEV, bn_groups=EVAL // B)
        base = base + (one.score_with_features(base[0])[1].clone(),)
        kw = dict(moments=PoolMoments(prop.feat_width, DEV), calibration=CalibrationStats(DEV))
    np.random.seed(77)
    pool, eff = reject_fill_fused(prop, rej, EVAL, REAL_MAX, base=base, min_efficiency=min_eff, stats=stats, **kw)
    del prop.launch
    return dict(pool=pool, eff=eff, state=np.random.get_state(), rounds=rounds, M=rej.D_tilde_M, stats=stats, base=base, **kw)


def _one_batch_at_a_time(G, min_eff, rounds):
    from cgs_amd.evaluate import reject_fill
    from cgs_amd.sampling import Rejector
    base = _base()
    i = [0]

    def propose():
        z = np.random.uniform(-1, 1, [B, 62]).astype(np.float32)
        r, j = divmod(i[0], G)
        assert np.array_equal(z, rounds[r][0][j * B:(j + 1) * B])
        i[0] += 1
        return rounds[r][1][j * B:(j + 1) * B]

    def score(batch):
        r, j = divmod(i[0] - 1, G)
        return rounds[r][2][j * B:(j + 1) * B]
    rej = Rejector()
    np.random.seed(77)
    want, eff = reject_fill(propose, score, rej, EVAL, np.float32(REAL_MAX), base=(base[0].cpu().numpy(), base[1].cpu().numpy()), min_efficiency=min_eff)
    return want, eff, np.random.get_state(), float(rej.D_tilde_M), i[0]


@pytest.mark.parametrize("G,min_eff", [(1, None), (4, None), (4, 0.76), (4, 0.2)], ids=["G1", "G4", "G4-cutoff-mid-round", "G4-reference-cutoff"])
def test_fused_fill_equals_the_host_loop_on_the_same_scores(G, min_eff):
    got = _fused(G, min_eff)
    want, eff, state, M, batches = _one_batch_at_a_time(G, min_eff, got["rounds"])
    pool = got["pool"]
    assert isinstance(pool, torch.Tensor) and pool.device.type == "cuda" and tuple(pool.shape) == (EVAL, 28, 28, 1)      # it never visited the host
    assert np.array_equal(pool.cpu().numpy(), want.astype(np.float32))                       # the same rows in the same order
    assert got["eff"] == eff
    s = got["state"]
    assert s[0] == state[0] and np.array_equal(s[1], state[1]) and s[2:] == state[2:]         # the numpy stream, where the host loop leaves it
    assert abs(got["M"] - M) <= 4 * np.spacing(abs(M))
    assert got["stats"]["proposed"] == batches * B
    print(f"\n[reject_fill_fused G={G} min_eff={min_eff}] rounds {got['stats']['rounds']}, proposed {got['stats']['proposed']}, eff {eff:.4f}, "
          f"batches drawn ahead and dropped {got['stats']['discarded_batches']}")
    if min_eff == 0.76:
        assert EVAL + batches * B > EVAL / min_eff and batches > 6 and (6 % G) != 0        # cutoff crossed, inside a round


def test_fused_fill_feeds_moments_and_calibration_from_the_pool_and_moves_nothing():
    from cgs_amd import metrics as M
    plain, full = _fused(4, 0.76), _fused(4, 0.76, features=True)
    assert torch.equal(plain["pool"], full["pool"]) and plain["eff"] == full["eff"] and np.array_equal(plain["state"][1], full["state"][1])
    imgs = np.concatenate([full["base"][0].cpu().numpy()] + [r[1] for r in full["rounds"]]).reshape(-1, 784)
    sigs = np.concatenate([full["base"][1].cpu().numpy()] + [r[2] for r in full["rounds"]])
    feats = np.concatenate([full["base"][2].cpu().numpy()] + [r[3] for r in full["rounds"]])
    rows = [int(np.flatnonzero((imgs == row).all(1))[0]) for row in full["pool"].cpu().numpy().reshape(EVAL, -1)]
    st = full["moments"].state()
    assert st["n"] == EVAL
    mu, cov = M.moments_mean_cov(st)
    f = feats[rows].astype(np.float64)
    assert np.allclose(mu, f.mean(0), rtol=1e-9, atol=1e-12) and np.allclose(cov, np.cov(f, rowvar=False), rtol=1e-7, atol=1e-12)
    cal, want = full["calibration"].state(), M.calibration_state_of(sigs[rows], 0)
    assert cal["n"] == EVAL and np.array_equal(cal["count"], want["count"]) and np.allclose(cal["sum_p"], want["sum_p"], rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- the 2-D evaluation
def _setup_2d():
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.synthetic import DShaper, MLPDiscriminator
    Ws, bs = S.mlp_init(64, 6, seed=2019, scale=1.0)
    D = MLPDiscriminator.from_lists([w.numpy() for w in Ws], [b.numpy() for b in bs], "cuda:0")
    data = ToyDataset("Imbal-8Gaussians", 10.0, 0.9)
    sh = DShaper(D, lrd=1e-2)
    np.random.seed(2019)
    train_rs = np.random.RandomState(3)
    for _ in range(200):                                               # a D that tells the blurred modes from the sharp ones
        sh.step(data.next_batch(1000), (data.centeroids[train_rs.randint(8, size=1000)] + 0.8 * train_rs.randn(1000, 2)).astype(np.float32))
    return D, data


def test_evaluate_calibrated_equals_the_host_samplers_on_the_same_scores():
    from cgs_amd import metrics as M
    from cgs_amd.evaluate import collaborate
    from cgs_amd.sampling import IndependenceSampler, Rejector
    from cgs_amd.synthetic import evaluate_calibrated
    D, data = _setup_2d()
    n = 1000
    thres = data.std * 4
    sigmoid = lambda x: D.sigmoid_and_saliency(x, want_saliency=False)[0].cpu().numpy()

    def fresh():
        gen_rs = np.random.RandomState(5)
        generate = lambda: (data.centeroids[gen_rs.randint(8, size=n)] + 0.8 * gen_rs.randn(n, 2)).astype(np.float32)
        np.random.seed(11)
        return generate, generate(), data.next_batch(n)
    generate, eval_batch, target = fresh()
    out = evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, keep_pools=True)
    end = np.random.get_state()[1].copy()
    assert set(out) == {"standard", "rejection", "hastings", "pools"}
    assert out["pools"]["rejection"].device.type == "cuda"
    # by hand: the host Rejector in the loop of the 2-D driver, then collaborate, on the same generator stream and device scores
    generate, eval_batch2, target2 = fresh()
    assert np.array_equal(eval_batch2, eval_batch) and np.array_equal(target2, target)
    real_sig, eval_sig = sigmoid(target), sigmoid(eval_batch)
    rej = Rejector()
    rej.set_score_max(np.amax(real_sig))
    kept = [rej.sampling(eval_batch, eval_sig, shift_percent=100.0)]
    cnt, prop = kept[0].shape[0], n
    while cnt < n:
        extra = generate()
        acc = rej.sampling(extra, sigmoid(extra), shift_percent=100.0)
        if acc.shape[0] > 0:
            kept.append(acc)
            cnt += acc.shape[0]
            prop += n
    pool = np.concatenate(kept)[:n]
    assert np.array_equal(out["pools"]["rejection"].cpu().numpy(), pool)
    assert out["rejection"]["eff"] == cnt / prop
    samples, eff = collaborate(generate, sigmoid, IndependenceSampler(T=20), n, float(np.mean(real_sig)), base=(eval_batch, eval_sig),
                               count_only_productive=True)
    assert np.array_equal(out["pools"]["hastings"], samples) and out["hastings"]["eff"] == float(eff)
    assert np.array_equal(np.random.get_state()[1], end)
    for name, p in (("standard", eval_batch), ("rejection", pool), ("hastings", samples)):
        md, good = M.metrics_distance(p, data.centeroids, thres)
        want = {"mean_dist": float(md), "good": float(good), "kl": float(M.metrics_diversity(target, p, data.centeroids, thres)),
                "js": float(M.metrics_distribution(target, p, data.centeroids, thres))}
        assert {k: out[name][k] for k in want} == want, name
    print(f"\n[evaluate_calibrated] good: standard {out['standard']['good']:.3f}, rejection {out['rejection']['good']:.3f} (eff {out['rejection']['eff']:.3f}), "
          f"hastings {out['hastings']['good']:.3f} (eff {out['hastings']['eff']:.3f})")
    # maps= / diagnostics= add their entries and move nothing else
    generate, _, _ = fresh()
    full = evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, maps=dict(scale=8.0, nbins=20))
    assert np.array_equal(np.random.get_state()[1], end) and set(full) == {"standard", "rejection", "hastings", "maps"}
    for part in ("standard", "rejection", "hastings"):
        assert full[part] == out[part], part
    assert set(full["maps"]) == {"standard", "rejection", "hastings", "target", "landscape"} and full["maps"]["rejection"].shape == (20, 20)
    generate, _, _ = fresh()
    diag = evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, diagnostics=True)
    assert np.array_equal(np.random.get_state()[1], end) and set(diag) == {"standard", "rejection", "hastings", "calibration"}
    for part in ("rejection", "hastings"):
        assert diag[part]["eff"] == out[part]["eff"]
        for k in ("mean_dist", "good", "kl", "js"):
            assert abs(diag[part][k] - out[part][k]) <= 1e-6 * max(1.0, abs(out[part][k])), (part, k)
    assert set(diag["calibration"]) >= {"z_dawid", "brier", "ece", "mce"}
    with pytest.raises(ValueError):
        evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, maps=dict(nbins=10))
