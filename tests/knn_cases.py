"""The nearest-neighbour queries and manifold metrics of two pools, stated once in float64 numpy straight from their definitions
(DESIGN.md section 33).  The kernels of csrc/knn.hip and the package's metrics.nn_distance / knn_radii / manifold_metrics are tested
against this file (tests/test_gpu_knn.py), and this file against brute-force loops, scipy and the reference (tests/test_knn_cases_cpu.py).

    D2(j, i)   sum_k (double(q_jk) - double(r_ik))^2, k ascending
    nn_min     per query the smallest D2 over the references and the lowest index that attains it; exclude_self leaves i == j out
    radii2     per row the k-th smallest D2 to the rows of the other pool, or to the OTHER rows of its own
    ball       per query #{i : D2(j, i) <= r2[i]}
    manifold   precision / recall / density / coverage, every comparison <= (on the squares)

The bound.  The kernel rounds q - r once (relative error u = 2^-53), then one fused multiply-add per coordinate rounds once more;
every term is non-negative, so the computed sum is sum_k t_k (1 + e)^2 prod (1 + e') with at most d + 2 factors per term:
|D2^ - D2| <= ((1 + u)^(d + 2) - 1) D2 <= (d + 3) u D2 for d <= 2048.  The float64 restatement below (product rounded, then d - 1 rounded
additions) obeys the same bound.  A discrete output (an index, a count, a metric) can therefore differ between two such evaluations only
where two compared values are closer than 2 bound(d) relatively: ``margins`` measures that gap per case, and the CPU test proves it wide.
"""
import functools
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
WIDE = 1e4            # every case's margin exceeds 2 bound(d) by at least this factor (tests/test_knn_cases_cpu.py)


def c_of(d):
    return d + 3


def bound(d):
    """Relative error bound of one D2 of width d against the exact value."""
    return c_of(d) * U


# ------------------------------------------------------------------------------------------------ inputs
def pool(kind, n, d, seed):
    """fp32 [n, d]: "gauss" = seeded standard normal; "ring" = the 8-Gaussians ring (radius 2, sigma 0.02; d must be 2);
    "mode0" = the ring's mode 0 alone."""
    rs = np.random.RandomState(seed)
    if kind == "gauss":
        return rs.randn(n, d).astype(np.float32)
    assert d == 2
    ang = 2.0 * np.pi * (rs.randint(8, size=n) if kind == "ring" else np.zeros(n, dtype=np.int64)) / 8.0
    centres = 2.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return (centres + 0.02 * rs.randn(n, 2)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
def sq_dist(q, r):
    """[m, n] float64: D2(j, i), the coordinates added in ascending order."""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    out = np.zeros((q.shape[0], r.shape[0]))
    for k in range(q.shape[1]):
        diff = q[:, k, None] - r[None, :, k]
        out += diff * diff
    return out


def _without_self(D2):
    D = np.array(D2)
    np.fill_diagonal(D, np.inf)
    return D


def nn_min(q, r, exclude_self=False):
    """-> (d2 [m], idx [m] (lowest index of the minimum; -1 and +inf without a candidate), self_d2 [m] or None)."""
    D2 = sq_dist(q, r)
    C = _without_self(D2) if exclude_self else D2
    idx = np.argmin(C, axis=1)
    best = C[np.arange(len(C)), idx]
    idx = np.where(np.isinf(best), -1, idx)
    return best, idx.astype(np.int32), (np.diagonal(D2).copy() if exclude_self else None)


def radii2(x, k, other=None):
    """-> (r2 [n]: the k-th smallest D2, at [n]: the index of a candidate that attains it)."""
    C = _without_self(sq_dist(x, x)) if other is None else sq_dist(x, other)
    assert 1 <= k <= C.shape[1] - (other is None)
    order = np.argsort(C, axis=1, kind="stable")[:, k - 1]
    return C[np.arange(len(C)), order], order


def ball_count(q, r, r2):
    return (sq_dist(q, r) <= np.asarray(r2)[None, :]).sum(axis=1).astype(np.int32)


def pairwise_distance(real, model):
    """The reference's sampling/utils_sampling.py:126-130 restated without scipy: min over the real axis of (distance + 10 I)."""
    dist = np.sqrt(sq_dist(real, model))
    return np.min(dist + 10.0 * np.identity(dist.shape[0]), axis=0)


def manifold(real, fake, k):
    r2_real, r2_fake = radii2(real, k)[0], radii2(fake, k)[0]
    cross = sq_dist(fake, real)                                          # [n_fake, n_real]
    count_fake = (cross <= r2_real[None, :]).sum(axis=1)
    count_real = (cross.T <= r2_fake[None, :]).sum(axis=1)
    covered = cross.min(axis=0) <= r2_real
    n_real, n_fake = len(real), len(fake)
    return {"precision": int((count_fake > 0).sum()) / n_fake, "recall": int((count_real > 0).sum()) / n_real,
            "density": int(count_fake.sum()) / (k * n_fake), "coverage": int(covered.sum()) / n_real, "k": k, "n_real": n_real, "n_fake": n_fake}


def exact_d2(a, b):
    """D2 of two fp32 rows as an exact rational."""
    return sum(((Fraction(float(x)) - Fraction(float(y))) ** 2 for x, y in zip(a, b)), Fraction(0))


def bound_fraction(got, a, b):
    """|got - D2(a, b)| / (bound(d) D2(a, b)) against the exact D2: <= 1 is within the bound (an exact 0 must be met exactly)."""
    ex = exact_d2(a, b)
    err = abs(Fraction(float(got)) - ex)
    if ex == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / (ex * Fraction(c_of(len(a))) * Fraction(1, 2 ** 53)))


# ------------------------------------------------------------------------------------------------ margins
def _rel_gap(lo, hi):
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(np.isinf(hi), np.inf, (hi - lo) / hi)
    return float(np.min(g)) if g.size else float("inf")


def margin_min(D2, exclude_self=False):
    """Smallest relative gap between a row's best and second-best candidate (inf where a row has fewer than two)."""
    C = np.sort(_without_self(D2) if exclude_self else np.asarray(D2), axis=1)
    return _rel_gap(C[:, 0], C[:, 1]) if C.shape[1] > 1 else float("inf")


def margin_kth(C, k):
    """Smallest relative gap between a row's k-th and (k + 1)-th candidate (C: candidates, excluded ones +inf)."""
    S = np.sort(C, axis=1)
    return _rel_gap(S[:, k - 1], S[:, k]) if S.shape[1] > k else float("inf")


def margin_ball(D2, r2):
    """Smallest |D2 - r2| / D2 over all ball tests."""
    D2 = np.asarray(D2)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.abs(D2 - np.asarray(r2)[None, :]) / D2
    return float(np.nanmin(g)) if g.size else float("inf")


# ------------------------------------------------------------------------------------------------ the cases
# (name, kind, m, n, d): m queries against n references.  m, n in {1, 2, 63, 64, 65, 130} and d in {1, 2, 31, 32, 33, 70} each occur;
# "split" is the shape the plan cuts (few queries against 3000 2-D references: 47 tiles, 10 runs of 5).
PAIR_CASES = [
    ("1x1_d1", "gauss", 1, 1, 1), ("2x1_d2", "gauss", 2, 1, 2), ("1x2_d31", "gauss", 1, 2, 31), ("63x64_d32", "gauss", 63, 64, 32),
    ("64x65_d33", "gauss", 64, 65, 33), ("65x63_d70", "gauss", 65, 63, 70), ("130x130_ring", "ring", 130, 130, 2),
    ("64x64_d1", "gauss", 64, 64, 1), ("130x2_d33", "gauss", 130, 2, 33), ("2x130_d32", "gauss", 2, 130, 32),
    ("65x130_d31", "gauss", 65, 130, 31), ("130x65_d70", "gauss", 130, 65, 70), ("2x2_d2", "gauss", 2, 2, 2),
    ("split_5x3000_ring", "ring", 5, 3000, 2),
]
SPLIT_PAIR = "split_5x3000_ring"
# (name, kind, n, d, k, n_other or None): k in {1, 3, 8}; "2_k1", "9_k8" and "130v8_k8" have k equal to the number of candidates;
# "split_self" (2000 rows against themselves: 32 x 32 tiles, 8 runs of 4) and "split_other" are cut by the plan.
RADII_CASES = [
    ("2_k1", "gauss", 2, 1, 1, None), ("63_ring_k3", "ring", 63, 2, 3, None), ("64_d31_k8", "gauss", 64, 31, 8, None),
    ("65_d32_k1", "gauss", 65, 32, 1, None), ("130_d33_k3", "gauss", 130, 33, 3, None), ("130_d70_k8", "gauss", 130, 70, 8, None),
    ("9_k8", "gauss", 9, 2, 8, None), ("1v2_k1", "gauss", 1, 2, 1, 2), ("65v130_d33_k8", "gauss", 65, 33, 8, 130),
    ("130v8_k8", "gauss", 130, 2, 8, 8), ("split_self", "ring", 2000, 2, 3, None), ("split_other", "ring", 5, 2, 3, 3000),
]
SPLIT_RADII = ("split_self", "split_other")
# (name, kind of the reals, kind of the fakes, n_real, n_fake, d, k)
MANIFOLD_CASES = [
    ("ring_130v65_k3", "ring", "ring", 130, 65, 2, 3), ("gauss_64v130_d33_k1", "gauss", "gauss", 64, 130, 33, 1),
    ("gauss_200v150_d70_k8", "gauss", "gauss", 200, 150, 70, 8), ("collapsed_400v300_k5", "ring", "mode0", 400, 300, 2, 5),
]


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """-> dict: q, r (fp32), r2 (float64 [n]: the ball radii handed to both sides), the restatement's answers and the margins."""
    _, kind, m, n, d = next(c for c in PAIR_CASES if c[0] == name)
    q, r = pool(kind, m, d, _seed(name)), pool(kind, n, d, _seed(name) + 1)
    D2 = sq_dist(q, r)
    r2 = radii2(r, min(3, n - 1))[0] if n >= 2 else np.full(n, float(d))
    out = {"q": q, "r": r, "d": d, "r2": r2, "D2": D2, "min": nn_min(q, r), "ball": ball_count(q, r, r2),
           "margins": {"min": margin_min(D2), "ball": margin_ball(D2, r2)}}
    if m == n:
        out["min_excl"] = nn_min(q, r, exclude_self=True)
        out["margins"]["min_excl"] = margin_min(D2, exclude_self=True)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def radii_case(name):
    _, kind, n, d, k, n_other = next(c for c in RADII_CASES if c[0] == name)
    x = pool(kind, n, d, _seed(name))
    other = None if n_other is None else pool(kind, n_other, d, _seed(name) + 1)
    C = _without_self(sq_dist(x, x)) if other is None else sq_dist(x, other)
    r2, at = radii2(x, k, other)
    for v in (x, other, r2, at):
        if v is not None:
            v.setflags(write=False)
    return {"x": x, "other": other, "d": d, "k": k, "r2": r2, "at": at, "margins": {"kth": margin_kth(C, k)}}


@functools.lru_cache(maxsize=None)
def manifold_case(name):
    _, kr, kf, n_real, n_fake, d, k = next(c for c in MANIFOLD_CASES if c[0] == name)
    real, fake = pool(kr, n_real, d, _seed(name)), pool(kf, n_fake, d, _seed(name) + 1)
    r2_real, r2_fake = radii2(real, k)[0], radii2(fake, k)[0]
    cross = sq_dist(fake, real)
    margins = {"ball_fake": margin_ball(cross, r2_real), "ball_real": margin_ball(cross.T, r2_fake),
               "kth_real": margin_kth(_without_self(sq_dist(real, real)), k), "kth_fake": margin_kth(_without_self(sq_dist(fake, fake)), k),
               "coverage": margin_ball(cross.min(axis=0)[None, :], r2_real)}
    real.setflags(write=False); fake.setflags(write=False)
    return {"real": real, "fake": fake, "d": d, "k": k, "want": manifold(real, fake, k), "margins": margins}
