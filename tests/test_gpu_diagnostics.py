"""csrc/diagnostics.hip on the device against the pure-numpy states of cgs_amd.metrics (calibration_state_of / mode_state_of), the
device classes against the goldens recorded from the reference, and the opt-in wiring into FusedProposer and evaluate_collaborative.

The bars are derived, not measured (the reasoning of section 18).  Counts, ``under`` and the maxima are integers or
selections: bit-equal.  Every sum adds n terms that carry at most one rounding each (y - p and 1 - p are exact for an fp32 p, up to the
denormal scores, where the second rounding is far below the bar), so for any order a sum that starts from s0 ends within
gamma_{n+1} <= (n + 2) u of (|s0| + sum |term|), u = 2^-53; numpy's own sum carries the same kind of error, hence 2 (n + 2) u.  The worst
observed ratio to that bound is printed per case.

Sizes: one element; 63 / 64 / 65 around the wave; 255 / 256 / 257 (still one block of 512); 4099 = 9 blocks with a short last chunk;
70001 = 137 blocks.  Bins 1, 20 (the reference's), 50 and 64 (the limit); modes 1, 8, 25 and 64 (the limit)."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N

U = 2.0 ** -53
SIZES = [1, 63, 64, 65, 255, 256, 257, 4099, 70001]
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _neighbours(edges):
    """The fp32 neighbours of every double edge (the largest fp32 below, the smallest at or above), 0, 1 and the smallest denormal --
    without the one negative value (below the first edge: the ``under`` case has its own test)."""
    out = [np.float32(0.0), np.float32(1.0), np.nextafter(np.float32(0), np.float32(1))]
    for e in edges:
        hi = np.float32(e)
        if float(hi) < e:
            hi = np.nextafter(hi, np.float32(np.inf))
        out += [np.nextafter(hi, np.float32(-np.inf)), hi]
    out = np.asarray(out, dtype=np.float32)
    return out[out >= 0]


@functools.lru_cache(maxsize=None)
def _cal_case(n, n_bins, label):
    """(scores, edges, the host twin's flat state, the flat sum of |term|s, start contents) -- computed once, read-only."""
    from cgs_amd import metrics as M
    rs = np.random.RandomState(100000 * label + 1000 * n_bins + n % 997)
    p = (1.0 / (1.0 + np.exp(-(rs.randn(n) * 1.5 + (1.0 if label else -1.0))))).astype(np.float32)
    edges = M.calibration_edges(n_bins)
    nb = _neighbours(edges)
    m = min(len(nb), max(1, n // 2))
    p[rs.choice(n, m, replace=False)] = rs.permutation(nb)[:m]
    st = M.calibration_state_of(p, label, n_bins)
    ref = M._cal_flat(st)
    p64 = p.astype(np.float64)
    y, S = float(label), n_bins + 1
    slot = np.digitize(p64, edges) - 1
    mag = np.zeros_like(ref)
    mag[S:2 * S] = np.bincount(slot, weights=np.abs(p64), minlength=S)
    mag[2 * S:3 * S] = ref[2 * S:3 * S]
    mag[3 * S + 1:3 * S + 4] = [np.abs(y - p64).sum(), np.abs(p64 * (1.0 - p64)).sum(), ((y - p64) ** 2).sum()]
    mag[3 * S + 6 + 3 * label] = np.abs(p64).sum()
    R = 3 * S + 11
    start = rs.randn(R) * 50.0
    counts = list(range(S)) + [3 * S, 3 * S + 4, 3 * S + 5, 3 * S + 8]
    start[counts] = rs.randint(0, 1000, len(counts))
    start[[3 * S + 7, 3 * S + 10]] = [0.5, 0.999]
    for v in (p, edges, ref, mag, start):
        v.setflags(write=False)
    return p, edges, ref, mag, start


def _cal_expect(n_bins, label, ref, start):
    S = n_bins + 1
    want = start + ref
    mx = 3 * S + 7 + 3 * label
    want[mx] = max(start[mx], ref[mx])
    o = 3 * S + 5 + 3 * (1 - label)
    want[o:o + 3] = start[o:o + 3]                                   # the other label's triple stays
    return want


def _cal_check(tag, got, want, mag, start, n, n_bins, label):
    S = n_bins + 1
    exact = list(range(S)) + [3 * S, 3 * S + 4, 3 * S + 5, 3 * S + 7, 3 * S + 8, 3 * S + 10] + list(range(3 * S + 5 + 3 * (1 - label), 3 * S + 8 + 3 * (1 - label)))
    assert np.array_equal(got[exact], want[exact]), (tag, got[exact], want[exact])
    sums = [j for j in range(3 * S + 11) if j not in exact]
    bound = 2.0 * (n + 2) * U * (np.abs(start[sums]) + mag[sums])
    ratio = float((np.abs(got[sums] - want[sums]) / np.maximum(bound, 1e-300)).max())
    print(f"\n[calibration {tag}] worst |delta| / bound over the sums: {ratio:.3g} (bar 1)")
    assert np.isfinite(got).all() and ratio <= 1.0, (tag, ratio)
    return ratio


@pytest.mark.parametrize("label", [0, 1])
@pytest.mark.parametrize("n_bins", [1, 20, 50, 64])
@pytest.mark.parametrize("n", SIZES)
def test_calibration_kernel_counts_bit_equal_sums_within_the_derived_bound_reruns_bit_equal(n, n_bins, label):
    from cgs_amd import kernels as K
    p, edges, ref, mag, start = _cal_case(n, n_bins, label)
    pd, ed = _dev(p), _dev(edges)
    for onto in ("zeros", "contents"):
        s0 = np.zeros_like(start) if onto == "zeros" else start
        st = _dev(s0)
        K.calibration_accumulate(pd if label else pd.view(n, 1), label, ed, st)
        _cal_check(f"n={n} bins={n_bins} y={label} {onto}", st.cpu().numpy(), _cal_expect(n_bins, label, ref, s0), mag, s0, n, n_bins, label)
        for ws in K._mom_ws.values():                                 # a NaN-filled workspace does not leak, and the rerun is bit-equal
            ws.fill_(float("nan"))
        st2 = _dev(s0)
        K.calibration_accumulate(pd, label, ed, st2)
        assert torch.equal(st, st2)


def test_three_chunked_calibration_updates_give_the_counts_and_the_sums_of_one():
    from cgs_amd import kernels as K
    n, n_bins, label = 70001, 20, 1
    p, edges, ref, mag, start = _cal_case(n, n_bins, label)
    ed, st = _dev(edges), _dev(start)
    for a, b in ((0, 5), (5, 40000), (40000, n)):
        K.calibration_accumulate(_dev(p[a:b]), label, ed, st)
    _cal_check("70001 in three updates", st.cpu().numpy(), _cal_expect(n_bins, label, ref, start), mag, start, n, n_bins, label)


def test_nan_and_large_scores_land_in_the_last_slot_and_negative_ones_in_under():
    from cgs_amd import kernels as K
    from cgs_amd import metrics as M
    p = np.array([0.25, np.nan, 1.5, -0.25, 0.75, -1e-30], dtype=np.float32)
    st = torch.zeros(3 * 21 + 11, dtype=torch.float64, device=DEV)
    K.calibration_accumulate(_dev(p), 1, _dev(M.calibration_edges(20)), st)
    got, want = M._cal_unflat(st.cpu().numpy(), 20), M.calibration_state_of(p, 1)
    assert np.array_equal(got["count"], want["count"]) and got["count"][20] == 2 and got["count"].sum() == 4
    assert got["under"] == want["under"] == 2 and got["n"] == want["n"] == 4 and got["label_n"][1] == 4
    assert got["label_max"][1] == want["label_max"][1] == 1.5
    assert np.array_equal(got["sum_p"][:20], want["sum_p"][:20]) and np.isnan(got["sum_p"][20]) and np.isnan(got["sum_sq"])
    with pytest.raises(ValueError):
        M.calibration_diagnostics(got)


def test_calibration_bad_arguments_raise_and_change_nothing():
    from cgs_amd import kernels as K
    from cgs_amd import lib as L
    from cgs_amd import metrics as M
    p = torch.full((300,), 0.5, dtype=torch.float32, device=DEV)
    e = _dev(M.calibration_edges(20))
    st = torch.zeros(3 * 21 + 11, dtype=torch.float64, device=DEV)
    bad = [lambda: K.calibration_accumulate(p.cpu(), 0, e, st), lambda: K.calibration_accumulate(p.double(), 0, e, st),
           lambda: K.calibration_accumulate(p[::2], 0, e, st), lambda: K.calibration_accumulate(p.view(150, 2), 0, e, st),
           lambda: K.calibration_accumulate(p, 2, e, st), lambda: K.calibration_accumulate(p, 0.5, e, st),
           lambda: K.calibration_accumulate(p, 0, e[:1], st), lambda: K.calibration_accumulate(p, 0, _dev(np.linspace(0, 1, 66)), torch.zeros(3 * 66 + 11, dtype=torch.float64, device=DEV)),
           lambda: K.calibration_accumulate(p, 0, e.float(), st), lambda: K.calibration_accumulate(p, 0, e.cpu(), st),
           lambda: K.calibration_accumulate(p, 0, e, st[:-1]), lambda: K.calibration_accumulate(p, 0, e, st.cpu())]
    for f in bad:
        with pytest.raises(L.CgsError):
            f()
    l = L.load()
    need = int(l.cgs_calibration_ws_bytes(300, 20))
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=DEV)
    args = (p.data_ptr(), 300, 0, e.data_ptr(), 20, st.data_ptr(), ws.data_ptr())
    assert l.cgs_calibration_accumulate(*args, need - 8, None) == L.EWORKSPACE
    assert l.cgs_calibration_accumulate(p.data_ptr(), 300, 0, e.data_ptr(), 20, st.data_ptr(), ws.data_ptr() + 4, need, None) == L.EINVAL
    torch.cuda.synchronize()
    assert not st.any() and not ws.any()                              # nothing was launched
    assert l.cgs_calibration_accumulate(*args, need, None) == L.OK
    torch.cuda.synchronize()
    assert st[9].item() == 300 and st[3 * 21].item() == 300              # (0.5 lies below the edge 0.500000005)


# ---------------------------------------------------------------------------------------------------------------- modes
@functools.lru_cache(maxsize=None)
def _mode_case(n, k):
    """Samples around k centroids (the first at the origin) plus constructed ties: thres = 5 s for a power of two s, (3 s, 4 s) and its
    mirror images lie EXACTLY thres from the origin (not a hit), their fp32 neighbours toward the origin are hits."""
    from cgs_amd import metrics as M
    rs = np.random.RandomState(1000 * k + n % 997)
    s = {1: 0.5, 8: 0.25, 25: 0.125, 64: 0.0625}[k]
    thres = 5.0 * s
    c = np.concatenate([np.zeros((1, 2)), rs.uniform(-20, 20, (k - 1, 2)) * thres])
    x = (c[rs.randint(k, size=n)] + rs.randn(n, 2) * thres / 2.0).astype(np.float32)
    a, b = np.float32(3 * s), np.float32(4 * s)
    an, bn = np.nextafter(a, np.float32(0)), np.nextafter(b, np.float32(0))
    ties = np.array([(a, b), (an, b), (a, bn), (b, a), (-a, b), (-an, -b), (b, -a), (-b, -an), (a, -b)], dtype=np.float32)
    m = min(len(ties), n)
    x[rs.choice(n, m, replace=False)] = ties[:m]
    st = M.mode_state_of(x, c, thres)
    if n >= len(ties):                                                # the construction does what it says, in the host twin already
        d0 = np.sqrt((ties.astype(np.float64) ** 2).sum(1))
        assert ((d0 == thres) == [1, 0, 0, 1, 1, 0, 1, 0, 1]).all() and (d0 <= thres).all()
    ref = np.concatenate([st["counts"].astype(np.float64), [st["n"], st["good"], st["sum_min"]]])
    start = np.concatenate([rs.randint(0, 1000, k + 2).astype(np.float64), [rs.randn() * 50.0]])
    for v in (x, c, ref, start):
        v.setflags(write=False)
    return x, c, thres, ref, start


def _mode_check(tag, got, ref, start, n, k):
    want = start + ref
    assert np.array_equal(got[:k + 2], want[:k + 2]), (tag, got[:k + 2], want[:k + 2])
    bound = 2.0 * (n + 2) * U * (abs(start[k + 2]) + ref[k + 2])
    ratio = abs(got[k + 2] - want[k + 2]) / bound
    print(f"\n[modes {tag}] |delta| / bound of the distance sum: {ratio:.3g} (bar 1)")
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("k", [1, 8, 25, 64])
@pytest.mark.parametrize("n", SIZES)
def test_mode_kernel_counts_bit_equal_distance_sum_within_the_bound_reruns_bit_equal(n, k):
    from cgs_amd import kernels as K
    x, c, thres, ref, start = _mode_case(n, k)
    xd, cd = _dev(x), _dev(c)
    for onto in ("zeros", "contents"):
        s0 = np.zeros_like(start) if onto == "zeros" else start
        st = _dev(s0)
        K.mode_stats_accumulate(xd, cd, thres, st)
        _mode_check(f"n={n} k={k} {onto}", st.cpu().numpy(), ref, s0, n, k)
        for ws in K._mom_ws.values():
            ws.fill_(float("nan"))
        st2 = _dev(s0)
        K.mode_stats_accumulate(xd, cd, thres, st2)
        assert torch.equal(st, st2)


def test_mode_bad_arguments_raise_and_change_nothing():
    from cgs_amd import kernels as K
    from cgs_amd import lib as L
    x = torch.ones((300, 2), dtype=torch.float32, device=DEV)
    c = torch.zeros((8, 2), dtype=torch.float64, device=DEV)
    st = torch.zeros(11, dtype=torch.float64, device=DEV)
    bad = [lambda: K.mode_stats_accumulate(x.cpu(), c, 1.0, st), lambda: K.mode_stats_accumulate(x.double(), c, 1.0, st),
           lambda: K.mode_stats_accumulate(torch.ones((2, 300), dtype=torch.float32, device=DEV).t(), c, 1.0, st),
           lambda: K.mode_stats_accumulate(x.view(200, 3), c, 1.0, st), lambda: K.mode_stats_accumulate(x, c[:0], 1.0, st[:3]),
           lambda: K.mode_stats_accumulate(x, torch.zeros((65, 2), dtype=torch.float64, device=DEV), 1.0, torch.zeros(68, dtype=torch.float64, device=DEV)),
           lambda: K.mode_stats_accumulate(x, c.float(), 1.0, st), lambda: K.mode_stats_accumulate(x, c.cpu(), 1.0, st),
           lambda: K.mode_stats_accumulate(x, c, 1.0, st[:-1]), lambda: K.mode_stats_accumulate(x, c, 1.0, st.float())]
    for f in bad:
        with pytest.raises(L.CgsError):
            f()
    l = L.load()
    need = int(l.cgs_mode_stats_ws_bytes(300, 8))
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=DEV)
    assert l.cgs_mode_stats_accumulate(x.data_ptr(), 300, c.data_ptr(), 8, 1.0, st.data_ptr(), ws.data_ptr(), need - 8, None) == L.EWORKSPACE
    torch.cuda.synchronize()
    assert not st.any() and not ws.any()


# ---------------------------------------------------------------------------------------------------------------- classes
def test_calibration_stats_in_batches_of_64_from_two_streams_gives_the_golden_diagnostics(golden_dir):
    """Golden c1 (1000 fake + 1500 real): the derived bound on each sum at these sizes is below 4e-9 and sum p (1 - p) > 400, so the
    quotients move by far less than the bar of 1e-7."""
    import os
    from cgs_amd.metrics import CalibrationStats
    g = np.load(os.path.join(golden_dir, "calibration_golden.npz"))
    cs = CalibrationStats(DEV)
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    i = 0
    for label, p in ((0, g["c1_fake"]), (1, g["c1_real"])):
        pd = _dev(p)
        torch.cuda.synchronize()
        for a in range(0, len(p), 64):
            with torch.cuda.stream(streams[i % 2]):
                cs.update(pd[a:a + 64], label)
            i += 1
    d = cs.diagnostics()
    st = cs.state()
    assert st["n"] == 2500 and list(st["label_n"]) == [1000, 1500] and st["sum_var"] > 400
    got = np.array([d["z_dawid"], d["brier"], d["ece"], d["mce"]])
    print("\n[CalibrationStats c1] |delta| to the golden:", np.abs(got - g["c1_diag"]))
    assert np.abs(got - g["c1_diag"]).max() <= 1e-7
    assert d["real_max"] == float(g["c1_real"].max()) and abs(d["real_mean"] - g["c1_real"].astype(np.float64).mean()) <= 1e-12
    with pytest.raises(ValueError):
        CalibrationStats("cpu")


@pytest.mark.parametrize("tag", ["g25", "imb8"])
def test_mode_stats_on_the_mode_golden_gives_the_reference_metrics(golden_dir, tag):
    import os
    from cgs_amd.metrics import ModeStats, mode_metrics, mode_state_of
    g = np.load(os.path.join(golden_dir, "mode_golden.npz"))
    c, thres = g[f"{tag}_centeroids"], float(g[f"{tag}_thres"][0])
    sm = ModeStats(c, thres, DEV).update(_dev(g[f"{tag}_model"][:300])).update(_dev(g[f"{tag}_model"][300:])).state()
    sr = ModeStats(c, thres, DEV).update(_dev(g[f"{tag}_real"])).state()
    host = mode_state_of(g[f"{tag}_model"], c, thres)
    assert np.array_equal(sm["counts"], host["counts"]) and (sm["n"], sm["good"]) == (1000, host["good"])
    m = mode_metrics(sm, sr)
    ref = np.concatenate([g[f"{tag}_ref_model_dist"], g[f"{tag}_ref_kl_js"]])
    assert np.abs(np.array([m["mean_dist"], m["good"], m["kl"], m["js"]]) - ref).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_fused_proposer_feeds_standard_and_real_scores_and_leaves_every_result_alone():
    """mnist, b = 8, G = 2, depth 2: one standard round (label 0) and 24 real images (label 1; the second round is half padding)."""
    import gc
    from cgs_amd import ops
    from cgs_amd.evaluate import FusedProposer, collaborate_fused
    from cgs_amd.metrics import CalibrationStats, calibration_diagnostics, calibration_merge, calibration_state_of
    from cgs_amd.model import GAN
    from cgs_amd.sampling import IndependenceSampler
    ops.reset_variables()
    gan = GAN("mnist", batch_size=8, device=DEV, params=N.init_params("mnist", 2019, True))
    rs = np.random.RandomState(5)
    z = rs.uniform(-1, 1, (16, 62)).astype(np.float32)
    real = rs.uniform(-1, 1, (24, 28, 28, 1)).astype(np.float32)
    runs = []
    for with_cal in (False, True):
        gc.collect()
        prop = FusedProposer(gan, 2, 0.1, batch=8, groups=2, depth=2, use_graph=False)
        cs = CalibrationStats(DEV) if with_cal else None
        kw = dict(calibration=cs) if with_cal else {}
        img, sig = prop.result(prop.launch(z, refine=False, **kw))
        img, sig = img.copy(), sig.copy()
        sreal = prop.score_real(real, **kw)
        np.random.seed(11)
        out, eff = collaborate_fused(prop, IndependenceSampler(T=2), 32, float(sreal.mean()))
        runs.append((img, sig, sreal, out, eff, np.random.get_state()[1].copy()))
        if with_cal:
            st = cs.state()
            assert st["n"] == 40 and list(st["label_n"]) == [16, 24] and st["under"] == 0
            host = calibration_diagnostics(calibration_merge(calibration_state_of(sig, 0), calibration_state_of(sreal, 1)))
            dev = cs.diagnostics()
            for key in ("z_dawid", "brier", "ece", "mce", "real_mean"):
                assert abs(dev[key] - host[key]) <= 1e-9, key
            assert dev["real_max"] == float(sreal.max())
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


def test_evaluate_collaborative_with_diagnostics_returns_the_same_metrics_and_the_calibration_of_its_scores():
    from cgs_amd.datasets import ToyDataset
    from cgs_amd.metrics import calibration_diagnostics, calibration_merge, calibration_state_of
    from cgs_amd.synthetic import Gan, MLPDiscriminator, Refiner, evaluate_collaborative
    D = MLPDiscriminator.init(2019, nhidden=64, nlayers=6, device=DEV)
    data = ToyDataset("25Gaussians", scale=1.0)
    n = 256
    outs = []
    for diag in (False, True):
        ref = Refiner(types.SimpleNamespace(rollout_steps=5, rollout_rate=0.05, rollout_method="ladam"))
        ref.set_env(Gan(D), None, data)
        rs = np.random.RandomState(2)
        np.random.seed(2019)
        gen = lambda: (data.next_batch(n) + 0.2 * rs.randn(n, 2)).astype(np.float32)
        eval_batch, target = gen(), data.next_batch(n).astype(np.float32)
        outs.append(evaluate_collaborative(ref, D, gen, eval_batch, target, data.centeroids, data.std, **(dict(diagnostics=True) if diag else {})))
    plain, full = outs
    assert set(plain) == {"standard", "refinement", "collaborate"} and set(full) == set(plain) | {"calibration"}
    for part in plain:
        for key, want in plain[part].items():
            got = full[part][key]
            if key == "mean_dist":
                assert abs(got - want) <= 2.0 * (n + 2) * U * want, (part, got, want)
            else:
                assert got == want, (part, key, got, want)             # the counts are identical, so are good, kl, js and eff
    sig = lambda x: D.sigmoid_and_saliency(x, want_saliency=False)[0].cpu().numpy()
    host = calibration_diagnostics(calibration_merge(calibration_state_of(sig(eval_batch), 0), calibration_state_of(sig(target), 1)))
    for key in ("z_dawid", "brier", "ece", "mce", "real_mean", "real_max"):
        assert abs(full["calibration"][key] - host[key]) <= 1e-9, key
    assert np.array_equal(full["calibration"]["weights"], host["weights"])
