"""Discriminator rejection sampling, stated in float64 numpy: what csrc/drs.hip computes on the device, the cases the tests run it on,
and the bound on how far device and host may differ.

The definition is the reference's Rejector (sampling/rejector.py:16-34) called once per logical batch:

    d     = logit(clip(double(s), 1e-14, 1 - 1e-14))
    M_g   = max(M_{g-1}, max d over batch g)                 M_{-1}: the bound the call starts from
    F     = (d - M_g) - log(1 - exp((d - M_g) - eps))
    gamma = percentile(F over batch g, q), numpy's linear method; 0 for q = None
    P     = expit(F - gamma)           mask = u < P

``decide_batch`` is one such call, ``decide`` the grouped form (a prefix maximum over the batches, everything else per batch).

The error model.  Device and host run the same IEEE double operations in the same order; they differ through the exp / log / log1p of
two math libraries, each within 1 ulp of the truth, so 2 ulp apart.  Once an input differs, every later add / subtract / divide may
round differently too: half an ulp each side, one ulp apart.  ``bound`` carries these through the definition, on the REFERENCE's own
intermediate values (u(x) = the spacing of doubles at x):

    |dd|     <= 2 u(d)                                        (log(x / (1 - x)); the quotient is the same on both sides)
             or 2 u(log1p(t)) + 2 u(log1p(-t)) + u(d)         (scipy's form on [0.3, 0.65], t = 2 (x - 0.5))
    |dM_g|   <= max(|dM_{g-1}|, max |dd| over the batch)      (a maximum moves by no more than its inputs)
    |ddelta| <= |dd| + |dM| + u(delta)
    |de|     <= e expm1(|ddelta| + u(delta - eps)) + 2 u(e)   e = exp(delta - eps)
    |dw|     <= |de| + u(w)                                   w = 1 - e >= ~1e-8: the term that dominates, |de| / w
    |dF|     <= |ddelta| - log1p(-|dw| / w) + 2 u(log w) + u(F)
    |dgamma| <= max |dF| over the batch + 4 u(max(|lo|, |hi|, |hi - lo|))      (order statistics move by no more than the values)
    |dP|     <= (|dee| + u(1 + ee)) / ((1 + ee)(1 + ee - |dee| - u(1 + ee))) + u(P),   ee = exp(-(F - gamma)),
                |dee| <= ee expm1(|dF| + |dgamma| + u(F - gamma)) + 2 u(ee)

to first order P (1 - P)(|dF| + |dgamma|) + 2 u(P).  No factor is fitted to what the device gives."""
import numpy as np
from scipy.special import expit, logit

LO, HI = 1e-14, 1 - 1e-14
EPS = 1e-8


def percentile_linear(F, q):
    """np.percentile(F, q) for a 1-D F, spelled out: the linear method's virtual index, its two order statistics, numpy's two-sided lerp.
    -> (gamma, lo, hi)"""
    srt = np.sort(np.asarray(F, dtype=np.float64))
    n = srt.shape[0]
    v = (n - 1) * (q / 100.0)
    k = int(np.floor(v))
    if k >= n - 1:
        lo = hi = srt[n - 1]
        t = 0.0
    else:
        lo, hi, t = srt[k], srt[k + 1], v - k
    diff = hi - lo
    return (lo + diff * t if t < 0.5 else hi - diff * (1 - t)), lo, hi


def decide_batch(sig, u, M0, eps=EPS, q=60.0):
    """One Rejector.sampling call.  -> dict(d, M, F, gamma, lo, hi, P, mask)"""
    d = logit(np.clip(np.asarray(sig).astype(float).reshape(-1), LO, HI))
    M = np.maximum(M0, np.amax(d))
    delta = d - M
    F = delta - np.log(1 - np.exp(delta - eps))
    gamma, lo, hi = (0.0, 0.0, 0.0) if q is None else percentile_linear(F, q)
    P = expit(F - gamma) if q is not None else expit(F)
    return dict(d=d, M=float(M), F=F, gamma=gamma, lo=lo, hi=hi, P=P, mask=np.asarray(u) < P)


def decide(sig, u, M0, groups=1, eps=EPS, q=60.0):
    """The grouped form, vectorised over the batches.  -> dict(d, M [groups], F, gamma [groups], lo, hi, P, mask, counts [groups]),
    the per-row entries as [groups * b] arrays."""
    s = np.asarray(sig).astype(float).reshape(groups, -1)
    d = logit(np.clip(s, LO, HI))
    M = np.maximum.accumulate(np.concatenate([[M0], d.max(axis=1)]))[1:]
    delta = d - M[:, None]
    F = delta - np.log(1 - np.exp(delta - eps))
    if q is None:
        gamma = lo = hi = np.zeros(groups)
        P = expit(F)
    else:
        g3 = np.array([percentile_linear(F[g], q) for g in range(groups)])
        gamma, lo, hi = g3[:, 0], g3[:, 1], g3[:, 2]
        P = expit(F - gamma[:, None])
    mask = np.asarray(u).reshape(groups, -1) < P
    return dict(d=d.reshape(-1), M=M, F=F.reshape(-1), gamma=gamma, lo=lo, hi=hi, P=P.reshape(-1), mask=mask.reshape(-1),
                counts=mask.sum(axis=1).astype(np.int32))


def _u(x):
    return np.spacing(np.abs(x))


def bound(sig, ref, M0, groups=1, eps=EPS, q=60.0, dM0=0.0):
    """The error model of the module docstring on the reference values ``ref`` = decide(sig, ., M0, groups, eps, q).
    -> (|dP| bound per row, |dM| bound per batch); ``dM0``: the bound on the error of the starting state."""
    x = np.clip(np.asarray(sig).astype(float).reshape(groups, -1), LO, HI)
    d, F, P = (ref[k].reshape(groups, -1) for k in ("d", "F", "P"))
    t = 2 * (x - 0.5)
    inner = (x >= 0.3) & (x <= 0.65)
    with np.errstate(divide="ignore", invalid="ignore"):
        dd = np.where(inner, 2 * _u(np.log1p(np.where(inner, t, 0))) + 2 * _u(np.log1p(np.where(inner, -t, 0))) + _u(d), 2 * _u(d))
    dM = np.maximum.accumulate(np.concatenate([[dM0], dd.max(axis=1)]))[1:]
    M = np.asarray(ref["M"]).reshape(groups, 1)
    delta = d - M
    ddelta = dd + dM[:, None] + _u(delta)
    xx = delta - eps
    e = np.exp(xx)
    de = e * np.expm1(ddelta + _u(xx)) + 2 * _u(e)
    w = 1 - e
    dw = de + _u(w)
    dF = ddelta - np.log1p(-dw / w) + 2 * _u(np.log(w)) + _u(F)
    if q is None:
        gamma, dg = np.zeros((groups, 1)), np.zeros((groups, 1))
    else:
        lo, hi = np.asarray(ref["lo"]), np.asarray(ref["hi"])
        big = np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.abs(hi - lo))
        dg = (dF.max(axis=1) + 4 * _u(big)).reshape(groups, 1)
        gamma = np.asarray(ref["gamma"]).reshape(groups, 1)
    y = F - gamma
    ee = np.exp(-y)
    dee = ee * np.expm1(dF + dg + _u(y)) + 2 * _u(ee)
    den = 1 + ee
    dden = dee + _u(den)
    dP = dden / (den * (den - dden)) + _u(P)
    return dP.reshape(-1), dM


# ---------------------------------------------------------------------------------------------------------------- the cases
SHAPES = [(1, 1), (2, 1), (63, 1), (64, 1), (65, 1), (257, 1), (1000, 1), (10000, 1), (64, 32), (64, 3), (1000, 2)]      # (b, groups)
PERCENTS = [None, 0.0, 37.5, 60.0, 100.0]
KINDS = ["uniform", "clustered", "zero_one", "equal", "ties", "bound_above", "bound_below"]
MARGIN = 8.0          # no uniform lies within MARGIN * bound of its row's P: the device mask must then EQUAL the reference's


def case_id(b, groups, q, kind):
    return "%s-b%dx%d-q%s" % (kind, b, groups, "none" if q is None else "%g" % q)


def scores(kind, b, groups, q, seed):
    """-> (fp32 scores [groups * b], the bound the call starts from)"""
    rs = np.random.RandomState(seed)
    n = b * groups
    M0 = 0.0                                                        # Rejector's own start: logit(0.5)
    if kind == "uniform":
        s = rs.uniform(0.001, 0.999, n)
    elif kind == "clustered":
        s = 0.7 + rs.uniform(0, 1e-6, n)
    elif kind == "zero_one":
        s = rs.uniform(0.01, 0.99, n)
        s[rs.randint(n)] = 0.0
        s[rs.randint(n)] = 1.0
        if n > 2:
            s[rs.randint(n)] = 0.0
    elif kind == "equal":
        s = np.full(n, 0.8125)
    elif kind == "ties":                                            # the two ranks the percentile reads hold the same value
        s = rs.uniform(0.05, 0.95, (groups, b))
        s.sort(axis=1)
        k = min(int(np.floor((b - 1) * ((50.0 if q is None else q) / 100.0))), max(b - 2, 0))
        if b > 1:
            s[:, k + 1] = s[:, k]
        if b > 3:
            s[:, min(k + 2, b - 1)] = s[:, k]
        for g in range(groups):
            rs.shuffle(s[g])
        s = s.reshape(-1)
    elif kind == "bound_above":
        s, M0 = rs.uniform(0.05, 0.95, n), float(logit(0.999999))
    elif kind == "bound_below":
        s, M0 = rs.uniform(0.6, 0.95, n), -5.0
    else:
        raise ValueError(kind)
    return s.astype(np.float32), M0


def build(b, groups, q, kind, call=0):
    """Scores, starting bound and uniforms of a case (``call`` = 1: the second call, which continues the first one's state).  The
    uniforms come from the first of eight seeds that keeps every row MARGIN bounds away from its P.
    -> dict(sig, M0, u, ref, dP, dM, margin_ok)"""
    idx = (SHAPES.index((b, groups)) * len(PERCENTS) + PERCENTS.index(q)) * len(KINDS) + KINDS.index(kind)
    sig, M0 = scores(kind, b, groups, q, 1000 + 2 * idx + call)
    dM0 = 0.0
    if call == 1:
        first = build(b, groups, q, kind, 0)
        M0, dM0 = float(first["ref"]["M"][-1]), float(first["dM"][-1])
    n = b * groups
    for attempt in range(8):
        u = np.random.RandomState(50000 + 16 * idx + 8 * call + attempt).rand(n)
        ref = decide(sig, u, M0, groups, EPS, q)
        dP, dM = bound(sig, ref, M0, groups, EPS, q, dM0)
        ok = bool(np.all(np.abs(u - ref["P"]) > MARGIN * dP))
        if ok:
            break
    return dict(sig=sig, M0=M0, u=u, ref=ref, dP=dP, dM=dM, margin_ok=ok)


def all_cases():
    return [(b, g, q, kind) for (b, g) in SHAPES for q in PERCENTS for kind in KINDS]


# ---------------------------------------------------------------------------------------------------------------- the fill loops' counters
def fill_model(batches, sampling, eval_size, base, max_propose=float("inf"), productive_only=False):
    """The counter rules of the reference's two DRS fill loops (nsgan/GAN.py:312-343; synthetic/main.py:150-169 with
    ``productive_only``), restated independently of ``evaluate.reject_fill``: every kept row goes on a list that is cut to ``eval_size``
    at the end.  ``batches`` yields (samples, sigmoids); ``sampling`` is rejector.sampling.  A batch met at or past ``max_propose``
    proposals is kept whole without being shown to the rejector; with ``productive_only`` a batch that yields nothing does not count as
    proposed.  (Accepted rows are always kept: GAN.py:326 drops a batch's rows while nothing has been accepted yet, see reject_fill.)
    -> (samples [eval_size, ...], accepted, proposed)"""
    kept = [sampling(base[0], base[1])]
    accepted, proposed = kept[0].shape[0], eval_size
    while accepted < eval_size:
        samples, sigmoids = next(batches)
        rows = sampling(samples, sigmoids) if proposed < max_propose else samples
        kept.append(rows)
        accepted += rows.shape[0]
        if rows.shape[0] or not productive_only:
            proposed += samples.shape[0]
    return np.concatenate(kept)[:eval_size], accepted, proposed
