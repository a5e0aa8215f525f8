"""tests/knn_cases.py against brute-force loops, scipy's cdist and the reference's pairwise_distance (live where it is importable, and as
recorded in tests/golden/g11_pairwise_distance.npz); the margins that make equality of the discrete outputs a fair demand on the GPU;
the C ABI surface of csrc/knn.hip, its plan and its refusals.  No device."""
import ctypes
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest

import knn_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cgs_knn_plan", "cgs_knn_ws_bytes", "cgs_nn_min", "cgs_knn_radii", "cgs_ball_count"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "g11_pairwise_distance.npz")


def _loop_d2(a, b):
    s = 0.0
    for x, y in zip(a, b):
        df = float(x) - float(y)
        s += df * df
    return s


def test_restatement_equals_brute_force_loops():
    q, r = KC.pool("gauss", 7, 5, 1), KC.pool("gauss", 9, 5, 2)
    D2 = KC.sq_dist(q, r)
    loops = np.array([[_loop_d2(a, b) for b in r] for a in q])
    assert np.array_equal(D2, loops)
    best, idx, own = KC.nn_min(q, r)
    assert own is None
    for j in range(7):
        cand = sorted((loops[j, i], i) for i in range(9))
        assert (best[j], idx[j]) == cand[0]
        for k in (1, 3, 9):
            r2, at = KC.radii2(q, k, r)
            assert r2[j] == cand[k - 1][0] and loops[j, at[j]] == r2[j]
    x = np.concatenate([q, q[:3]])                                       # duplicated rows: ties, and zeros that are not the row itself
    L = np.array([[_loop_d2(a, b) for b in x] for a in x])
    best, idx, own = KC.nn_min(x, x, exclude_self=True)
    for j in range(10):
        cand = sorted((L[j, i], i) for i in range(10) if i != j)
        assert (best[j], idx[j]) == cand[0] and own[j] == 0.0
        for k in (1, 3, 9):
            assert KC.radii2(x, k)[0][j] == cand[k - 1][0]
    assert list(best[:3]) == [0.0] * 3 and list(idx[:3]) == [7, 8, 9] and list(idx[7:]) == [0, 1, 2]
    r2 = KC.radii2(r, 2)[0]
    assert list(KC.ball_count(q, r, r2)) == [sum(loops[j, i] <= r2[i] for i in range(9)) for j in range(7)]
    best, idx, own = KC.nn_min(q[:1], q[:1], exclude_self=True)          # no candidate
    assert np.isinf(best[0]) and idx[0] == -1 and own[0] == 0.0
    with pytest.raises(AssertionError):
        KC.radii2(q, 7)                                                  # 6 other rows


def test_manifold_restatement_equals_loops_over_the_definitions():
    real, fake, k = KC.pool("ring", 40, 2, 3), KC.pool("ring", 30, 2, 4), 3
    dist = lambda a, b: _loop_d2(a, b)
    rho = lambda pool_, i: sorted(dist(pool_[i], pool_[t]) for t in range(len(pool_)) if t != i)[k - 1]
    rr, rf = [rho(real, i) for i in range(40)], [rho(fake, j) for j in range(30)]
    count = [sum(dist(fake[j], real[i]) <= rr[i] for i in range(40)) for j in range(30)]
    want = {"precision": sum(c > 0 for c in count) / 30, "density": sum(count) / (k * 30),
            "recall": sum(any(dist(real[i], fake[j]) <= rf[j] for j in range(30)) for i in range(40)) / 40,
            "coverage": sum(min(dist(real[i], fake[j]) for j in range(30)) <= rr[i] for i in range(40)) / 40, "k": k, "n_real": 40, "n_fake": 30}
    assert KC.manifold(real, fake, k) == want
    from cgs_amd import metrics as M
    assert M.manifold_metrics_host(real, fake, k) == want
    same = KC.manifold(real, real, k)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0
    with pytest.raises(ValueError):
        M.manifold_metrics_host(real[:3], fake, 3)


def test_restatement_equals_scipys_cdist():
    cdist = pytest.importorskip("scipy.spatial.distance").cdist
    for name, *_ in KC.PAIR_CASES[:-1]:
        c = KC.pair_case(name)
        assert np.array_equal(np.sqrt(c["D2"]), cdist(c["q"], c["r"])), name


def _reference_pairwise_distance():
    """The reference's own function where its tree is importable (the build container only), else None."""
    path = "/root/reference/sampling/utils_sampling.py"
    if not os.path.exists(path):
        return None
    stubbed = []
    for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.gridspec", "sklearn", "sklearn.metrics"):
        if name not in sys.modules and importlib.util.find_spec(name.split(".")[0]) is None:
            sys.modules[name] = types.ModuleType(name)
            stubbed.append(name)
    if "sklearn.metrics" in stubbed:
        sys.modules["sklearn.metrics"].brier_score_loss = None
    try:
        spec = importlib.util.spec_from_file_location("_reference_utils_sampling", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.pairwise_distance
    finally:
        for name in stubbed:
            sys.modules.pop(name, None)


def test_pairwise_distance_equals_the_reference_bit_for_bit():
    from cgs_amd import metrics as M
    g = np.load(GOLDEN)
    live = _reference_pairwise_distance()
    for tag in ("near", "far", "wide"):
        real, model, want = g[tag + "_real"], g[tag + "_model"], g[tag + "_out"]
        for fn in (KC.pairwise_distance, M.pairwise_distance):
            assert np.array_equal(fn(real, model), want), (tag, fn.__module__)
        if live is not None:
            assert np.array_equal(live(real, model), want), tag
    assert np.all(g["far_out"] == 10.0)                                  # the self term wins: every other point is farther than 10
    assert np.all(g["near_out"] < 10.0)
    if live is not None:
        for name in ("130x130_ring", "64x64_d1", "2x2_d2"):
            c = KC.pair_case(name)
            assert np.array_equal(KC.pairwise_distance(c["r"], c["q"]), live(c["r"], c["q"])), name
    with pytest.raises(ValueError):
        M.pairwise_distance(g["near_real"], g["near_model"][:5])
    # exclude_self of nn_min gives the same: min(sqrt(min_{i != j} D2), sqrt(D2_jj) + 10)
    best, _, own = KC.nn_min(g["near_model"], g["near_real"], exclude_self=True)
    assert np.array_equal(np.minimum(np.sqrt(best), np.sqrt(own) + 10.0), g["near_out"])


def _margins():
    for name, *_ in KC.PAIR_CASES:
        c = KC.pair_case(name)
        yield "pair " + name, c["d"], c["margins"]
    for name, *_ in KC.RADII_CASES:
        c = KC.radii_case(name)
        yield "radii " + name, c["d"], c["margins"]
    for name, *_ in KC.MANIFOLD_CASES:
        c = KC.manifold_case(name)
        yield "manifold " + name, c["d"], c["margins"]


def test_every_gpu_cases_margin_exceeds_twice_the_bound_by_a_wide_factor():
    worst = None
    for tag, d, margins in _margins():
        for what, m in margins.items():
            ratio = m / (2.0 * KC.bound(d))
            assert ratio >= KC.WIDE, f"{tag} {what}: margin {m:.3g} is {ratio:.3g} x (2 bound)"
            if worst is None or ratio < worst[0]:
                worst = (ratio, tag, what, m)
    print(f"\n[knn margins] narrowest: {worst[1]} {worst[2]}: {worst[3]:.3g} = {worst[0]:.3g} x (2 bound); bar {KC.WIDE:g}")
    assert KC.bound(70) == 73 * 2.0 ** -53 and KC.bound(2048) < 2.3e-13


def test_case_lists_cover_the_edges_the_plan_has():
    sizes = {v for _, _, m, n, _ in KC.PAIR_CASES for v in (m, n)}
    assert {1, 2, 63, 64, 65, 130} <= sizes
    assert {1, 2, 31, 32, 33, 70} <= {d for *_, d in KC.PAIR_CASES}
    assert {1, 3, 8} == {k for _, _, _, _, k, _ in KC.RADII_CASES}
    assert any(k == (n - 1 if other is None else other) for _, _, n, _, k, other in KC.RADII_CASES)       # k = the number of candidates
    from cgs_amd import knn
    _, _, m, n, d = next(c for c in KC.PAIR_CASES if c[0] == KC.SPLIT_PAIR)
    assert knn.plan(m, n, d)["splits"] > 1
    for name in KC.SPLIT_RADII:
        _, _, n, d, _, other = next(c for c in KC.RADII_CASES if c[0] == name)
        assert knn.plan(n, n if other is None else other, d)["splits"] > 1, name
    assert all(knn.plan(m, n, d)["splits"] == 1 for name, _, m, n, d in KC.PAIR_CASES if name != KC.SPLIT_PAIR)


def test_abi_declares_types_and_exports_the_new_entry_points():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    l = lib.load()
    for name in NEW:
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert lib.SIGNATURES["cgs_knn_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert (lib.KNN_NN_MIN, lib.KNN_RADII, lib.KNN_BALL_COUNT) == tuple(int(re.search(r"#define CGS_KNN_" + n + r" (\d+)", header).group(1))
                                                                       for n in ("NN_MIN", "RADII", "BALL_COUNT"))
    assert "knn.hip" in open(os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc", "Makefile")).read()
    assert lib.built_from() == lib.source_hash()                         # the stamp covers knn.hip: source_hash() reads every csrc/*.hip
    assert os.path.exists(os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc", "knn.hip"))


def _shapes():
    for _, _, m, n, d in KC.PAIR_CASES:
        yield m, n, d
    for _, _, n, d, _, other in KC.RADII_CASES:
        yield n, (n if other is None else other), d
    yield from ((10000, 10000, 512), (50000, 50000, 512), (1, 1 << 30, 1), (1 << 30, 1, 2048), (300, 100000, 2))


def test_plan_covers_every_reference_tile_once_and_is_monotone():
    """csrc/knn.hip, knn_plan restated: 64 queries per block; the reference tiles are cut into as many runs as bring the grid to 512
    blocks, of at least 4 tiles each, at most 64 runs; every run but the last holds tiles_per_split tiles, none is empty."""
    from cgs_amd import knn, lib
    l = lib.load()
    for m, n, d in _shapes():
        p = knn.plan(m, n, d)
        qt, rt = -(-m // 64), -(-n // 64)
        want = max(1, min(-(-512 // qt), max(rt // 4, 1), 64))
        per = -(-rt // want)
        assert p == {"query_tiles": qt, "ref_tiles": rt, "tiles_per_split": per, "splits": -(-rt // per)}, (m, n, d)
        runs = [(s * p["tiles_per_split"], min((s + 1) * p["tiles_per_split"], rt)) for s in range(p["splits"])]
        assert runs[0][0] == 0 and runs[-1][1] == rt and all(a < b for a, b in runs) and all(runs[i][1] == runs[i + 1][0] for i in range(len(runs) - 1))
        for op, k, slots in ((lib.KNN_NN_MIN, 0, 3), (lib.KNN_RADII, 3, 3), (lib.KNN_RADII, 8, 8), (lib.KNN_BALL_COUNT, 0, 1)):
            need = p["splits"] * slots * m * 8 if p["splits"] > 1 else 0
            assert int(l.cgs_knn_ws_bytes(op, m, n, d, k)) == max(need, 8), (m, n, d, op)
    # more queries never mean more runs; more references never mean fewer tiles per run
    for n in (3000, 100000):
        splits = [knn.plan(m, n, 2)["splits"] for m in (1, 64, 65, 640, 6400, 64000)]
        assert splits == sorted(splits, reverse=True) and splits[0] > 1 and splits[-1] == 1
    for m in (5, 5000):
        per = [knn.plan(m, n, 2)["tiles_per_split"] for n in (1, 64, 65, 1000, 3000, 100000, 1 << 30)]
        assert per == sorted(per)


def test_refusals_come_before_any_pointer_is_read():
    from cgs_amd import knn, lib
    l = lib.load()
    err = lambda: l.cgs_last_error().decode()
    for m, n, d in ((0, 5, 2), (5, 0, 2), (5, 5, 0), (5, 5, 2049), (-1, 5, 2), ((1 << 30) + 1, 5, 2), (5, (1 << 30) + 1, 2)):
        assert knn.plan(m, n, d) is None
        for op in range(3):
            assert int(l.cgs_knn_ws_bytes(op, m, n, d, 1)) == 0
        assert l.cgs_nn_min(None, m, None, n, d, 0, None, None, None, 0, None) == lib.EINVAL and "nn_min: needs 1 <= d <= 2048" in err()
        assert l.cgs_ball_count(None, m, None, n, d, None, None, None, 0, None) == lib.EINVAL
        assert l.cgs_knn_radii(None, m, d, 1, 0, ctypes.c_void_p(8), n, None, None, 0, None) == lib.EINVAL
    assert int(l.cgs_knn_ws_bytes(3, 5, 5, 2, 1)) == 0 and int(l.cgs_knn_ws_bytes(-1, 5, 5, 2, 1)) == 0
    for k in (0, 9, -3):                                                                                  # k out of range
        assert int(l.cgs_knn_ws_bytes(lib.KNN_RADII, 50, 50, 2, k)) == 0
        assert l.cgs_knn_radii(None, 50, 2, k, 1, None, 0, None, None, 0, None) == lib.EINVAL and "outside 1..8" in err()
    assert l.cgs_knn_radii(None, 3, 2, 3, 1, None, 0, None, None, 0, None) == lib.EINVAL                    # 2 other rows, k = 3
    assert "2 candidates per row are fewer than k = 3" in err()
    assert l.cgs_knn_radii(None, 3, 2, 3, 0, ctypes.c_void_p(8), 2, None, None, 0, None) == lib.EINVAL and "fewer than k" in err()
    assert l.cgs_knn_radii(None, 3, 2, 1, 1, ctypes.c_void_p(8), 3, None, None, 0, None) == lib.EINVAL and "other == NULL" in err()
    assert l.cgs_nn_min(None, 5, None, 6, 2, 1, None, None, None, 0, None) == lib.EINVAL and "exclude_self needs n == m" in err()
    assert l.cgs_nn_min(None, 5, None, 5, 2, 2, None, None, None, 0, None) == lib.EINVAL
    assert l.cgs_nn_min(None, 5, None, 5, 2, 1, None, None, None, 0, None) == lib.EINVAL and "null" in err()   # a good shape: now the pointers
    assert l.cgs_ball_count(None, 5, None, 5, 2, None, None, None, 0, None) == lib.EINVAL and "null" in err()
    assert l.cgs_knn_radii(None, 5, 2, 4, 1, None, 0, None, None, 0, None) == lib.EINVAL and "null" in err()
