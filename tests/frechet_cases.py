"""The Frechet distance from two moment states, three ways (csrc/frechet.hip):

STATEMENT   float64 numpy, the yardstick.  mean = shift + sum / n, cov = (gram - sum sum^T / n) / (n - ddof), symmetrised;
            R = S_r^{1/2} from eigh(S_r) with the eigenvalues clipped at 0, M = R S_f R symmetrised, Tr M^{1/2} = sum sqrt(max(eigvalsh(M), 0));
            fd = |dmu|^2 + Tr S_r + Tr S_f - 2 Tr M^{1/2}.  Tr M^{1/2} = Tr (S_r S_f)^{1/2}, and only symmetric positive semi-definite
            matrices are ever rooted.
TRANSCRIPT  the device algorithm in numpy float64, product for product: the coupled Newton-Schulz iteration with the stop rule below.
            The device differs from it only in the order of its sums.
CASES       pairs of seeded [n, d] fp32 clouds turned into states.  Class A: full rank (n >= 4 d); class B: rank-deficient.

The device algorithm (``transcript``).  For a symmetric positive semi-definite A:
    nrm = |A|_F;  nrm == 0 -> the root is the zero matrix, 0 iterations.  Y = A / nrm, Z = I, t_0 = Tr Y, delta_0 = inf.
    step k = 1 .. max_iters:  T = 1.5 I - 0.5 Z Y;  Y' = sym(Y T);  Z' = sym(T Z);  t_k = Tr Y';  delta_k = |t_k - t_{k-1}|
        t_k not finite                                   -> Y' discarded, stop, status 1
        delta_k <= TOL(d) t_k                            -> Y' kept, stop, status 0
        k >= 5, delta_k >= delta_{k-1}, delta_k < 1e-6 t_k -> Y' discarded (the last good iterate is kept), stop, status 1:
                                                            the trace no longer converges, what grows from here is rounding noise
                                                            in the null space of A, which Z amplifies by 1.5 per step
        otherwise                                        -> Y' kept; at k = max_iters stop, status 2
    A^{1/2} = sqrt(nrm) Y,  Tr A^{1/2} = sqrt(nrm) Tr Y.
TOL(d) = max(1e-15, d 2^-52): a trace adds d terms, each one rounded, so a difference of two traces below d ulps is not a signal.
The first root is R' = Y of S_r (R = sqrt(nrm_r) R'); the second one is taken of M' = sym(R' (S_f R')), M = nrm_r M'.

THE ORACLE: max over a class of |fd_transcript - fd_statement| / e_norm, e_norm = Tr S_r + Tr S_f + |dmu|^2, measured on this table
(tests/test_frechet_cases_cpu.py measures it again and asserts that it stays within 2x of the recorded pair -- another BLAS orders its
sums differently; the GPU test's bars are 4x the RECORDED numbers):
    ORACLE_A = 9.3e-16  (d2048; the others 0 .. 5.2e-16)      ORACLE_B = 1.25e-6  (same_63; same_130 7.7e-8, the others <= 1.4e-8)
For judging class B: on these cases scipy.linalg.sqrtm (metrics.frechet_from_moments, the host route) deviates from the statement by up
to SCIPY_B = 1.5e-8 (n100_d256), and the statement itself resolves eigenvalues of M only to about 1e-16 |M|, i.e. their roots to 1e-8
sqrt|M|: class B cannot be settled below about 1e-8 of e_norm by any of the three.  The two largest class-B deviations are the
identical pools: there M = S^2 has eigenvalues down to 1e-8 of the largest, Newton-Schulz grows such an eigenvalue by 1.5 per step,
and rule three ends the iteration while the smallest are still growing (status 1): the trace of the root is short by about 1e-6."""
import functools

import numpy as np

MAX_ITERS = 48
U52 = 2.0 ** -52
ORACLE_A = 9.3e-16
ORACLE_B = 1.25e-6
SCIPY_B = 1.5e-8


def tol(d):
    return max(1e-15, d * U52)


# ---------------------------------------------------------------------------------------------------------------- clouds and states
def cloud(seed, n, d, scale=1.0, offset=0.0):
    """[n, d] fp32: LeakyReLU features of a min(64, d)-dimensional latent plus noise of 1e-2 (covariance condition about 1e4)."""
    rs = np.random.RandomState(seed)
    k = min(64, d)
    h = rs.randn(n, k).dot(rs.randn(k, d) / np.sqrt(k))
    h = np.where(h > 0, h, 0.2 * h) + 1e-2 * rs.randn(n, d)
    return (h * scale + offset).astype(np.float32)


def state_of(x, shift=None):
    """The state PoolMoments would hold: shift = the fp32 column mean of the cloud unless given; sum / gram in float64."""
    x = np.asarray(x, dtype=np.float32)
    c = x.mean(0).astype(np.float32) if shift is None else np.asarray(shift, dtype=np.float32)
    a = x.astype(np.float64) - c.astype(np.float64)
    return dict(n=int(x.shape[0]), shift=c.astype(np.float64), sum=a.sum(0), gram=a.T.dot(a))


# name -> (class, builder of the two clouds, shifts or None)
def _pair(seed, n, d, scale_f=1.0, off_r=0.0, off_f=0.0, n_f=None):
    return lambda: (cloud(seed, n, d, 1.0, off_r), cloud(seed + 1, n_f or n, d, scale_f, off_f))


def _same(seed, n, d):
    def make():
        x = cloud(seed, n, d)
        return x, x.copy()
    return make


def _flat(seed, n, d, both):
    def make():
        row = cloud(seed, 1, d)
        flat = np.repeat(row, n, axis=0)
        return flat, (np.repeat(cloud(seed + 1, 1, d), n, axis=0) if both else cloud(seed + 1, n, d))
    return make


CASES = {
    "d1": ("A", _pair(11, 64, 1)),
    "d16": ("A", _pair(12, 64, 16)),
    "d63": ("A", _pair(13, 252, 63)),
    "d64": ("A", _pair(14, 256, 64)),
    "d65": ("A", _pair(15, 260, 65)),
    "d130": ("A", _pair(16, 520, 130)),
    "d200": ("A", _pair(17, 800, 200)),
    "d512": ("A", _pair(18, 4096, 512)),
    "d200_scaled": ("A", _pair(19, 800, 200, scale_f=1e3)),
    "d64_far": ("A", _pair(20, 256, 64, off_r=100.0, off_f=50.0)),
    "d2048": ("A", _pair(21, 8192, 2048)),
    "n40_d64": ("B", _pair(31, 40, 64)),
    "n100_d256": ("B", _pair(32, 100, 256)),
    "n3_d65": ("B", _pair(33, 3, 65)),
    "n2_d16": ("B", _pair(34, 2, 16)),
    "n64_d130_small": ("B", lambda: tuple(1e-3 * c for c in _pair(35, 64, 130)())),
    "same_63": ("B", _same(36, 63, 63)),
    "same_130": ("B", _same(37, 130, 130)),
    "both_flat": ("B", _flat(38, 20, 33, True)),
    "one_flat": ("B", _flat(39, 80, 33, False)),
}
CLASS_A = [k for k, v in CASES.items() if v[0] == "A"]
CLASS_B = [k for k, v in CASES.items() if v[0] == "B"]
SMALL = [k for k in CASES if k != "d2048"]


@functools.lru_cache(maxsize=None)
def states(name):
    """(state_r, state_f) of a case, built once; the arrays are read-only."""
    xr, xf = CASES[name][1]()
    out = (state_of(xr), state_of(xf))
    for st in out:
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------- shared head
def mean_terms(sr, sf, ddof=1):
    """(|dmu|^2, S_r, S_f) by the definitions of include/cgs_hip.h; the covariances symmetrised."""
    dmu = (sr["shift"] - sf["shift"]) + sr["sum"] / sr["n"] - sf["sum"] / sf["n"]

    def cov(st):
        c = (st["gram"] - np.outer(st["sum"], st["sum"]) / st["n"]) / (st["n"] - ddof)
        return 0.5 * (c + c.T)
    return float((dmu * dmu).sum()), cov(sr), cov(sf)


def _record(dmu2, tr_r, tr_f, tr_root, it0=0, it1=0, status=0):
    return dict(fd=dmu2 + tr_r + tr_f - 2.0 * tr_root, dmu2=dmu2, tr_r=tr_r, tr_f=tr_f, tr_root=tr_root, iters_r=it0, iters_m=it1,
                status=status, e_norm=tr_r + tr_f + dmu2)


# --------------------------------------------------------------------------------------------------------------------- statement
def statement(sr, sf, ddof=1):
    dmu2, S_r, S_f = mean_terms(sr, sf, ddof)
    w, V = np.linalg.eigh(S_r)
    R = (V * np.sqrt(np.maximum(w, 0.0))).dot(V.T)
    M = R.dot(S_f).dot(R)
    M = 0.5 * (M + M.T)
    tr_root = float(np.sqrt(np.maximum(np.linalg.eigvalsh(M), 0.0)).sum())
    return _record(dmu2, float(np.trace(S_r)), float(np.trace(S_f)), tr_root)


# -------------------------------------------------------------------------------------------------------------------- transcript
def newton_schulz_root(A, max_iters=MAX_ITERS):
    """-> (Y, nrm, Tr Y, iterations, status) with A^{1/2} = sqrt(nrm) Y; the rule in the module docstring."""
    d = A.shape[0]
    nrm = float(np.sqrt((A * A).sum()))
    if not nrm > 0.0:
        return np.zeros_like(A), 0.0, 0.0, 0, 0
    eye = np.eye(d)
    Y, Z = A / nrm, eye.copy()
    t_prev, d_prev = float(np.trace(Y)), np.inf
    for k in range(1, max_iters + 1):
        T = -0.5 * Z.dot(Y) + 1.5 * eye
        Yn, Zn = Y.dot(T), T.dot(Z)
        Yn, Zn = 0.5 * (Yn + Yn.T), 0.5 * (Zn + Zn.T)
        t = float(np.trace(Yn))
        dl = abs(t - t_prev)
        if not np.isfinite(t):
            return Y, nrm, t_prev, k, 1
        if dl <= tol(d) * t:
            return Yn, nrm, t, k, 0
        if k >= 5 and dl >= d_prev and dl < 1e-6 * t:
            return Y, nrm, t_prev, k, 1
        Y, Z, t_prev, d_prev = Yn, Zn, t, dl
    return Y, nrm, t_prev, max_iters, 2


def transcript(sr, sf, ddof=1, max_iters=MAX_ITERS):
    dmu2, S_r, S_f = mean_terms(sr, sf, ddof)
    Y, nrm_r, _, it0, st0 = newton_schulz_root(S_r, max_iters)
    M = Y.dot(S_f.dot(Y))
    M = 0.5 * (M + M.T)
    _, nrm_m, t, it1, st1 = newton_schulz_root(M, max_iters)
    tr_root = float(np.sqrt(nrm_r) * np.sqrt(nrm_m) * t)
    return _record(dmu2, float(np.trace(S_r)), float(np.trace(S_f)), tr_root, it0, it1, max(st0, st1))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(statement, transcript) of a case, computed once."""
    sr, sf = states(name)
    return statement(sr, sf), transcript(sr, sf)


def bar(name):
    """The GPU test's bar on |fd_dev - fd_statement| / e_norm."""
    d = states(name)[0]["shift"].shape[0]
    return max(4.0 * ORACLE_A, d * U52) if CASES[name][0] == "A" else 4.0 * ORACLE_B
