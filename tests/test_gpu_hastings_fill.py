"""The Metropolis-Hastings legs end to end with the chain on the device: ``evaluate.hastings_fill_fused`` on the MNIST net against
``evaluate.collaborate`` with the host ``IndependenceSampler`` fed the SAME device scores one batch at a time, and the two 2-D
evaluations with a ``DeviceIndependenceSampler`` against themselves with the host sampler.

mnist, b = 16, eval_size = 256, G = 1 and 4, depth 2, T = 3, seeded: the set-up of test_gpu_reject_fill.  ``proposer.launch`` is wrapped
to snapshot each round's z, images and scores, so the one-batch loop replays exactly the rows the fused loop walked; the chain's
arithmetic is exact (tests/test_gpu_mh.py), so rows, order, efficiency, the chain's final state and the numpy stream are EQUAL.
min_efficiency = 0.76 puts the cutoff at 336.8 proposals: the counter starts at 256 and moves by 16, so batches 0..5 meet the chain and
the cutoff falls inside round 2 of G = 4 (two batches walked, two taken whole); 0.2 is the reference's (nsgan/GAN.py:18)."""
import gc
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N
from oracle import sampling_ref as S

DEV = torch.device("cuda:0")
ARCH, B, EVAL, T = "mnist", 16, 256, 3
REAL_MEAN = np.float32(0.52)                                           # np.mean of fp32 scores is an np.float32 (nsgan/GAN.py:401)
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
        sig, feat = one.score_with_features(img)
        _GAN["base"] = (img, sig.clone(), feat.clone())
    return _GAN["base"]


def _fused(G, min_eff, refine, features=False):
    from cgs_amd.evaluate import FusedProposer, hastings_fill_fused
    from cgs_amd.metrics import CalibrationStats, PoolMoments
    from cgs_amd.sampling import DeviceIndependenceSampler
    gc.collect()
    base = _base()
    prop = FusedProposer(_gan(), 1, 0.1, batch=B, groups=G, depth=2, use_graph=False, features=features)
    rounds, inner, refined = [], prop.launch, []

    def launch(z, **kw):
        k = inner(z, **kw)
        prop.done[k].synchronize()
        refined.append((kw.get("refine"), kw.get("to_host")))
        rounds.append((np.array(z), prop.img_dev[k].cpu().numpy().copy(), prop.sig_dev[k].cpu().numpy().copy(),
                       prop.feat_dev[k].cpu().numpy().copy() if features else None))
        return k
    prop.launch = launch
    mh = DeviceIndependenceSampler(T=T, device=DEV)
    kw, stats = {}, {}
    if features:
        kw = dict(moments=PoolMoments(prop.feat_width, DEV), calibration=CalibrationStats(DEV))
    np.random.seed(77)
    pool, eff = hastings_fill_fused(prop, mh, EVAL, REAL_MEAN, base=base if features else base[:2], refine=refine, min_efficiency=min_eff, stats=stats, **kw)
    del prop.launch
    assert set(refined) == {(refine, False)}                             # the leg asked for, and no copy of a round to the host
    return dict(pool=pool, eff=eff, state=np.random.get_state(), rounds=rounds, d=mh.d_curr, cnt=mh.cnt_chain, stats=stats, base=base, **kw)


def _one_batch_at_a_time(G, min_eff, rounds):
    from cgs_amd.evaluate import collaborate
    from cgs_amd.sampling import IndependenceSampler
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
    mh = IndependenceSampler(T=T)
    np.random.seed(77)
    want, eff = collaborate(propose, score, mh, EVAL, REAL_MEAN, base=(base[0].cpu().numpy(), base[1].cpu().numpy()), min_efficiency=min_eff)
    return want, eff, np.random.get_state(), float(np.ravel(mh.d_curr)[0]), mh.cnt_chain, i[0]


@pytest.mark.parametrize("refine", [True, False], ids=["collaborate", "hastings"])
@pytest.mark.parametrize("G,min_eff", [(1, None), (4, None), (4, 0.76), (4, 0.2)], ids=["G1", "G4", "G4-cutoff-mid-round", "G4-reference-cutoff"])
def test_fused_fill_equals_the_host_loop_on_the_same_scores(G, min_eff, refine):
    got = _fused(G, min_eff, refine)
    want, eff, state, d, cnt, batches = _one_batch_at_a_time(G, min_eff, got["rounds"])
    pool = got["pool"]
    assert isinstance(pool, torch.Tensor) and pool.device.type == "cuda" and tuple(pool.shape) == (EVAL, 28, 28, 1)      # it never visited the host
    assert np.array_equal(pool.cpu().numpy(), want.astype(np.float32))                       # the same rows in the same order
    assert got["eff"] == eff
    s = got["state"]
    assert s[0] == state[0] and np.array_equal(s[1], state[1]) and s[2:] == state[2:]         # the numpy stream, where the host loop leaves it
    assert got["d"] == d and got["cnt"] == cnt                                               # the chain, where the host loop leaves it
    assert got["stats"]["proposed"] == batches * B
    print(f"\n[hastings_fill_fused G={G} min_eff={min_eff} refine={refine}] rounds {got['stats']['rounds']}, proposed {got['stats']['proposed']}, "
          f"eff {eff:.4f}, batches drawn ahead and dropped {got['stats']['discarded_batches']}")
    if min_eff == 0.76:
        assert EVAL + batches * B > EVAL / min_eff and batches > 6 and (6 % G) != 0        # cutoff crossed, inside a round


def test_fused_fill_feeds_moments_and_calibration_from_the_pool_and_moves_nothing():
    from cgs_amd import metrics as M
    plain, full = _fused(4, 0.76, True), _fused(4, 0.76, True, features=True)
    assert torch.equal(plain["pool"], full["pool"]) and plain["eff"] == full["eff"] and np.array_equal(plain["state"][1], full["state"][1])
    assert plain["d"] == full["d"] and plain["cnt"] == full["cnt"]
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


# ---------------------------------------------------------------------------------------------------------------- the 2-D evaluations
def _setup_2d():
    if "2d" not in _GAN:
        from cgs_amd.datasets import ToyDataset
        from cgs_amd.synthetic import DShaper, MLPDiscriminator
        Ws, bs = S.mlp_init(64, 6, seed=2019, scale=1.0)
        D = MLPDiscriminator.from_lists([w.numpy() for w in Ws], [b.numpy() for b in bs], "cuda:0")
        data = ToyDataset("Imbal-8Gaussians", 10.0, 0.9)
        sh = DShaper(D, lrd=1e-2)
        np.random.seed(2019)
        train_rs = np.random.RandomState(3)
        for _ in range(200):                                           # a D that tells the blurred modes from the sharp ones
            sh.step(data.next_batch(1000), (data.centeroids[train_rs.randint(8, size=1000)] + 0.8 * train_rs.randn(1000, 2)).astype(np.float32))
        _GAN["2d"] = (D, data)
    return _GAN["2d"]


def _same_metrics(a, b, parts):
    for part in parts:
        assert a[part] == b[part], part                                  # mean_dist, good, kl, js and eff: the same pools, the same numbers


def test_evaluate_calibrated_with_a_device_sampler_equals_the_host_sampler():
    from cgs_amd.sampling import DeviceIndependenceSampler, IndependenceSampler
    from cgs_amd.synthetic import evaluate_calibrated
    D, data = _setup_2d()
    n = 1000
    outs = []
    for mh in (IndependenceSampler(T=20), DeviceIndependenceSampler(T=20, device=DEV)):
        gen_rs = np.random.RandomState(5)
        generate = lambda: (data.centeroids[gen_rs.randint(8, size=n)] + 0.8 * gen_rs.randn(n, 2)).astype(np.float32)
        np.random.seed(11)
        eval_batch, target = generate(), data.next_batch(n)
        out = evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, mh_sampler=mh, keep_pools=True, maps=dict(scale=8.0, nbins=20))
        outs.append((out, np.random.get_state()[1].copy(), float(np.ravel(mh.d_curr)[0]), mh.cnt_chain))
    (host, host_end, hd, hc), (dev, dev_end, dd, dc) = outs
    assert isinstance(host["pools"]["hastings"], np.ndarray)
    assert isinstance(dev["pools"]["hastings"], torch.Tensor) and dev["pools"]["hastings"].device.type == "cuda"
    assert np.array_equal(dev["pools"]["hastings"].cpu().numpy(), host["pools"]["hastings"])
    assert torch.equal(dev["pools"]["rejection"], host["pools"]["rejection"])
    _same_metrics(dev, host, ("standard", "rejection", "hastings"))
    assert np.array_equal(dev_end, host_end) and dd == hd and dc == hc
    assert np.array_equal(dev["maps"]["hastings"], host["maps"]["hastings"])
    print(f"\n[evaluate_calibrated, device chain] hastings good {dev['hastings']['good']:.3f}, eff {dev['hastings']['eff']:.3f}")
    gen_rs = np.random.RandomState(5)                                    # the device statistics take the device pool as it is
    np.random.seed(11)
    eval_batch, target = generate(), data.next_batch(n)
    diag = evaluate_calibrated(D, generate, eval_batch, target, data.centeroids, data.std, mh_sampler=DeviceIndependenceSampler(T=20, device=DEV), diagnostics=True)
    assert np.array_equal(np.random.get_state()[1], host_end) and diag["hastings"]["eff"] == host["hastings"]["eff"]
    for k in ("mean_dist", "good", "kl", "js"):
        assert abs(diag["hastings"][k] - host["hastings"][k]) <= 1e-6 * max(1.0, abs(host["hastings"][k])), k


def test_evaluate_collaborative_with_a_device_sampler_equals_the_host_sampler():
    from cgs_amd.sampling import DeviceIndependenceSampler, IndependenceSampler
    from cgs_amd.synthetic import Gan, Refiner, evaluate_collaborative
    D, data = _setup_2d()
    n = 1000
    outs = []
    for mh in (IndependenceSampler(T=20), DeviceIndependenceSampler(T=20, device=DEV)):
        ref = Refiner(types.SimpleNamespace(rollout_steps=5, rollout_rate=0.1, rollout_method="ladam"))
        ref.set_env(Gan(D), None, data)
        gen_rs = np.random.RandomState(5)
        generate = lambda: (data.centeroids[gen_rs.randint(8, size=n)] + 0.8 * gen_rs.randn(n, 2)).astype(np.float32)
        np.random.seed(11)
        eval_batch, target = generate(), data.next_batch(n)
        out = evaluate_collaborative(ref, D, generate, eval_batch, target, data.centeroids, data.std, mh_sampler=mh, keep_pools=True)
        outs.append((out, np.random.get_state()[1].copy(), float(np.ravel(mh.d_curr)[0]), mh.cnt_chain))
    (host, host_end, hd, hc), (dev, dev_end, dd, dc) = outs
    assert set(host) == set(dev) == {"standard", "refinement", "collaborate", "pools"}
    assert isinstance(host["pools"]["collaborate"], np.ndarray)
    assert isinstance(dev["pools"]["collaborate"], torch.Tensor) and dev["pools"]["collaborate"].device.type == "cuda"
    assert np.array_equal(dev["pools"]["collaborate"].cpu().numpy(), host["pools"]["collaborate"])
    assert np.array_equal(dev["pools"]["refinement"], host["pools"]["refinement"])
    _same_metrics(dev, host, ("standard", "refinement", "collaborate"))
    assert np.array_equal(dev_end, host_end) and dd == hd and dc == hc
    print(f"\n[evaluate_collaborative, device chain] collaborate good {dev['collaborate']['good']:.3f}, eff {dev['collaborate']['eff']:.3f}")
