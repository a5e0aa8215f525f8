"""csrc/knn.hip on the device against tests/knn_cases.py.  Bars: every D2 that comes out (minimum, D2(j, j),
radius) within (d + 3) 2^-53 relative of the EXACT rational D2 of the pair the restatement names; every discrete output (index, ball
count, metric) EQUAL to the restatement's -- tests/test_knn_cases_cpu.py proves every case's margin wide enough for that to be fair."""
import os

import numpy as np
import pytest
import torch

import knn_cases as KC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {"fraction": 0.0}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _fraction(tag, got, a_rows, b_rows):
    """Worst |got - exact D2| / (bound D2) over the rows; asserts it <= 1."""
    worst = max((KC.bound_fraction(g, a, b) for g, a, b in zip(got, a_rows, b_rows)), default=0.0)
    WORST["fraction"] = max(WORST["fraction"], worst)
    print(f"\n[knn {tag}] worst |delta| / bound = {worst:.3g} (bar 1; worst so far {WORST['fraction']:.3g})")
    assert worst <= 1.0, tag
    return worst


@pytest.mark.parametrize("name", [c[0] for c in KC.PAIR_CASES])
def test_nn_min_and_ball_count_equal_the_restatement(name):
    from cgs_amd import knn
    c = KC.pair_case(name)
    q, r = _dev(c["q"]), _dev(c["r"])
    want_d2, want_idx, _ = c["min"]
    d2, idx, own = knn.nn_min(q, r)
    assert own is None and d2.dtype == torch.float64 and idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    _fraction(f"nn_min {name}", d2.cpu().numpy(), c["q"], c["r"][want_idx])
    count = knn.ball_count(q, r, _dev(c["r2"]))
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), c["ball"])
    if "min_excl" in c:
        want_d2, want_idx, _ = c["min_excl"]
        d2, idx, own = knn.nn_min(q, r, exclude_self=True)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        if len(c["q"]) > 1:
            _fraction(f"nn_min excl {name}", d2.cpu().numpy(), c["q"], c["r"][want_idx])
        else:
            assert np.isinf(d2.cpu().numpy()).all() and (want_idx == -1).all()
        _fraction(f"nn_min self {name}", own.cpu().numpy(), c["q"], c["r"])
    first, again = knn.nn_min(q, r), knn.nn_min(q, r)                   # a rerun is bit-identical
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(count, knn.ball_count(q, r, _dev(c["r2"])))


@pytest.mark.parametrize("name", [c[0] for c in KC.RADII_CASES])
def test_knn_radii_are_within_the_bound_of_the_exact_kth_distance(name):
    from cgs_amd import knn
    c = KC.radii_case(name)
    x, other = _dev(c["x"]), (None if c["other"] is None else _dev(c["other"]))
    r2 = knn.knn_radii(x, c["k"], other)
    assert r2.dtype == torch.float64 and tuple(r2.shape) == (len(c["x"]),)
    got = r2.cpu().numpy()
    rows = slice(None) if len(got) <= 130 else np.arange(0, len(got), 16)                   # (the exact rationals of 125 rows of the 2000)
    refs = c["x"] if c["other"] is None else c["other"]
    _fraction(f"radii {name}", got[rows], c["x"][rows], refs[c["at"][rows]])
    assert np.all(np.abs(got - c["r2"]) <= 2 * KC.bound(c["d"]) * c["r2"])             # every row, against the float64 restatement (a bound each)
    assert torch.equal(r2, knn.knn_radii(x, c["k"], other))


def test_duplicated_rows_give_exact_zeros():
    from cgs_amd import knn
    base = KC.pool("gauss", 40, 33, 7)
    x = np.concatenate([base, base[:10], base[:10], base[:5]])            # rows 0..4: four copies, 5..9: three, 10..39: one
    xd = _dev(x)
    d2, idx, own = knn.nn_min(xd, xd, exclude_self=True)
    d2, idx, own = d2.cpu().numpy(), idx.cpu().numpy(), own.cpu().numpy()
    assert np.all(own == 0.0) and np.all(d2[:10] == 0.0) and np.all(d2[40:] == 0.0) and np.all(d2[10:40] > 0.0)
    want = KC.nn_min(x, x, exclude_self=True)
    assert np.array_equal(idx, want[1]) and list(idx[:3]) == [40, 41, 42] and list(idx[40:43]) == [0, 1, 2]     # the LOWEST index of the tie
    d2p, idxp, _ = knn.nn_min(xd, xd)                                     # itself included: row j's own index unless a copy stands before it
    assert np.all(d2p.cpu().numpy() == 0.0) and np.array_equal(idxp.cpu().numpy(), KC.nn_min(x, x)[1])
    for k in (1, 2, 3):
        r2 = knn.knn_radii(xd, k).cpu().numpy()
        copies = np.array([4] * 5 + [3] * 5 + [1] * 30 + ([4] * 5 + [3] * 5) * 2 + [4] * 5)
        assert np.all((r2 == 0.0) == (copies - 1 >= k)), k                # exactly 0 where the row has >= k OTHER copies
        assert np.array_equal(r2 == 0.0, KC.radii2(x, k)[0] == 0.0)


def test_d2_is_symmetric_in_bits():
    from cgs_amd import knn
    for d in (1, 2, 33, 70):
        x = KC.pool("gauss", 2, d, 100 + d)
        a, b = _dev(x[:1]), _dev(x[1:])
        ab, ba = knn.nn_min(a, b)[0], knn.nn_min(b, a)[0]
        assert torch.equal(ab, ba) and ab.item() > 0.0
        both = knn.nn_min(_dev(x), _dev(x), exclude_self=True)[0]
        assert both[0].item() == both[1].item() == ab.item()


def test_split_and_unsplit_plans_give_identical_bits():
    """The plan is a function of the shape, so the unsplit twin of the split case is the same 5 queries followed by 32763 padding queries
    far away (512 query tiles: one run), against the same references: the first 5 answers must be the same bits."""
    from cgs_amd import knn
    c = KC.pair_case(KC.SPLIT_PAIR)
    m, n = len(c["q"]), len(c["r"])
    padded = np.concatenate([c["q"], np.full((64 * 512 - m, 2), 1e3, dtype=np.float32)])
    assert knn.plan(m, n, 2)["splits"] > 1 and knn.plan(len(padded), n, 2)["splits"] == 1
    q, qp, r, r2 = _dev(c["q"]), _dev(padded), _dev(c["r"]), _dev(c["r2"])
    d2, idx, _ = knn.nn_min(q, r)
    d2p, idxp, _ = knn.nn_min(qp, r)
    assert torch.equal(d2, d2p[:m]) and torch.equal(idx, idxp[:m])
    assert torch.equal(knn.ball_count(q, r, r2), knn.ball_count(qp, r, r2)[:m])
    for k in (1, 3, 8):
        assert torch.equal(knn.knn_radii(q, k, r), knn.knn_radii(qp, k, r)[:m]), k
    assert int(knn.ball_count(qp, r, r2)[m:].sum()) == 0


def test_nn_distance_reproduces_the_references_plus_ten_identity():
    from cgs_amd import metrics as M
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(KC.__file__)), "golden", "g11_pairwise_distance.npz"))
    for tag in ("near", "far", "wide"):
        real, model, want = g[tag + "_real"], g[tag + "_model"], g[tag + "_out"]
        real32, model32 = real.astype(np.float32), model.astype(np.float32)
        host = M.pairwise_distance(real32, model32)                       # (the device takes the pools as fp32)
        if tag != "near":
            assert np.array_equal(host, want)                             # ... which these two are exactly
        dist, idx = M.nn_distance(_dev(real32), _dev(model32))
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        # a root halves the relative error and adds one rounding: either side is within bound / 2 + 2^-53 <= bound of the exact distance
        assert np.all(np.abs(dist - host) <= 2 * KC.bound(real.shape[1]) * host), tag
        D = np.sqrt(KC.sq_dist(real32, model32)) + 10.0 * np.identity(len(real))
        assert np.array_equal(idx, np.argmin(D, axis=0)), tag
        if tag == "far":                                                  # the self term wins: every other point is farther than 10
            assert np.all(dist == 10.0) and np.array_equal(idx, np.arange(len(real)))
    plain, pidx = M.nn_distance(_dev(g["far_real"].astype(np.float32)), _dev(g["far_model"].astype(np.float32)), exclude_self=False)
    assert np.all(plain.cpu().numpy() == 0.0) and np.array_equal(pidx.cpu().numpy(), np.arange(12))
    short, _ = M.nn_distance(_dev(g["near_real"].astype(np.float32)), _dev(g["near_model"][:5].astype(np.float32)))     # two lengths: no self term
    assert tuple(short.shape) == (5,)
    c = KC.radii_case("130_d33_k3")
    rho = M.knn_radii(_dev(c["x"]), 3).cpu().numpy()
    assert np.all(np.abs(rho - np.sqrt(c["r2"])) <= 2 * KC.bound(33) * np.sqrt(c["r2"]))


@pytest.mark.parametrize("name", [c[0] for c in KC.MANIFOLD_CASES])
def test_manifold_metrics_equal_the_restatement(name):
    from cgs_amd import metrics as M
    c = KC.manifold_case(name)
    got = M.manifold_metrics(_dev(c["real"]), _dev(c["fake"]), k=c["k"])
    print(f"\n[manifold {name}] {got}")
    assert got == c["want"] and got == M.manifold_metrics_host(c["real"], c["fake"], c["k"])
    assert got == M.manifold_metrics(c["real"], c["fake"], k=c["k"])      # host arrays are uploaded
    if name.startswith("collapsed"):                                      # every fake sits on one of the 8 real modes
        assert got["precision"] > 0.8 and got["recall"] < 0.2 and got["coverage"] < 0.2


def test_identical_pools_are_fully_precise_recalled_and_covered():
    from cgs_amd import metrics as M
    for kind, n, d, k in (("ring", 130, 2, 3), ("gauss", 65, 33, 8)):
        x = _dev(KC.pool(kind, n, d, 5))
        got = M.manifold_metrics(x, x.clone(), k=k)
        assert got["precision"] == got["recall"] == got["coverage"] == 1.0 and got["density"] >= 1.0
        assert got == KC.manifold(x.cpu().numpy(), x.cpu().numpy(), k)    # D2(j, i) == D2(i, j) in bits: the ties fall as on the host


def test_wrappers_refuse_what_the_library_would():
    from cgs_amd import knn
    from cgs_amd import lib as L
    from cgs_amd import metrics as M
    x = torch.ones((6, 3), dtype=torch.float32, device=DEV)
    r2 = torch.ones(6, dtype=torch.float64, device=DEV)
    bad = [lambda: knn.nn_min(x.cpu(), x), lambda: knn.nn_min(x, x.double()), lambda: knn.nn_min(x, x[:, :2].contiguous()),
           lambda: knn.nn_min(x, x[:5], exclude_self=True), lambda: knn.nn_min(x.t(), x), lambda: knn.nn_min(x[:0], x),
           lambda: knn.nn_min(torch.ones((2, 2049), dtype=torch.float32, device=DEV), torch.ones((2, 2049), dtype=torch.float32, device=DEV)),
           lambda: knn.knn_radii(x, 0), lambda: knn.knn_radii(x, 9), lambda: knn.knn_radii(x, 6), lambda: knn.knn_radii(x, 2.5),
           lambda: knn.knn_radii(x, 7, x), lambda: knn.knn_radii(x, 1, x, exclude_self=True),
           lambda: knn.ball_count(x, x, r2.float()), lambda: knn.ball_count(x, x, r2[:5]), lambda: knn.ball_count(x, x, r2.cpu())]
    for f in bad:
        with pytest.raises(L.CgsError):
            f()
    with pytest.raises(ValueError):
        M.manifold_metrics(x, torch.ones((6, 2), dtype=torch.float32, device=DEV))
    assert knn.knn_radii(x, 5).cpu().tolist() == [0.0] * 6 and knn.knn_radii(x, 6, x).cpu().tolist() == [0.0] * 6
    l = L.load()
    q = torch.zeros((5, 2), dtype=torch.float32, device=DEV)
    r = torch.zeros((3000, 2), dtype=torch.float32, device=DEV)
    out, idx = torch.empty(5, dtype=torch.float64, device=DEV), torch.empty(5, dtype=torch.int32, device=DEV)
    need = int(l.cgs_knn_ws_bytes(L.KNN_NN_MIN, 5, 3000, 2, 0))
    ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=DEV)
    call = lambda wsp, nbytes: l.cgs_nn_min(q.data_ptr(), 5, r.data_ptr(), 3000, 2, 0, out.data_ptr(), idx.data_ptr(), wsp, nbytes, None)
    assert call(ws.data_ptr(), need - 8) == L.EWORKSPACE and call(None, need) == L.EWORKSPACE and call(ws.data_ptr() + 4, need) == L.EINVAL
    assert call(ws.data_ptr(), need) == L.OK
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == [0] * 5 and out.cpu().tolist() == [0.0] * 5
