"""The Metropolis-Hastings independence chain, stated in numpy fp32: what csrc/mh.hip computes on the device, the cases the tests run
it on, and the counter rules of the two fill loops around it.  tests/test_mh_cases_cpu.py holds this statement to the product's host
``IndependenceSampler.walk`` on every case; tests/test_gpu_mh.py holds the kernel to this statement, with no tolerance.

Per logical batch ("segment") of b proposals, with fp32 scores s, one double u per proposal, the chain state d (a double) and cnt:
    per proposal i, in order, every operation a separately rounded fp32 one:
        odds  = (s_i * omd) / (df * (1.0f - s_i))        omd = float32(1.0 - d), df = float32(d)
        alpha = odds if odds < 1.0f else 1.0f            (Python's min(1.0, odds): a NaN gives 1.0)
        moved = not (u_i > float64(alpha));  if moved: d = s_i
    from the positions pos[0] < pos[1] < ... of the segment's moves: nothing is emitted unless there are more than B of them;
    first = pos[B]; the visits v = first .. b - 1 are active, a = v - first; emissions at a = a0, a0 + (T + 1), ..., a0 = max(0, T + 1 - cnt);
    the emitted row is the last move position <= v; cnt leaves as 1 + (active visits after the last emission), or cnt + (active visits)
    if nothing was emitted.
The proposals are tested a stretch at a time against the state they all see until one of them moves (a move changes the state only
for the proposals after it), which is the per-proposal loop with the arithmetic done on arrays."""
import functools

import numpy as np

f32 = np.float32
STRETCH = 256
KINDS = ["uniform", "quarters", "tiny", "near1", "constant", "increasing", "decreasing"]
BS = [1, 2, 63, 64, 65, 129, 1000]
GROUPS = [1, 3, 32]
TS = [0, 1, 5, 20]
SEEDS = [0.5, f32(0.3137), 0.0, 0.48372619384712345, 1.0, f32(0.5), 0.0621, f32(0.0), f32(0.9214), 0.77, f32(1e-3)]      # Python floats and np.float32


def moved_mask(s, u, d):
    """``moved`` of every proposal of ``s`` against the state ``d`` (a Python float: the double the chain holds)."""
    omd, df = f32(1.0 - d), f32(d)
    with np.errstate(all="ignore"):
        odds = (s * omd) / (df * (f32(1.0) - s))
    assert odds.dtype == np.float32
    alpha = np.where(odds < f32(1.0), odds, f32(1.0))
    return ~(u > alpha.astype(np.float64))


def segment_moves(s, u, d):
    """-> (positions of the moves of one segment, d afterwards)"""
    pos, i, b = [], 0, len(s)
    while i < b:
        hi = min(i + STRETCH, b)
        hit = np.flatnonzero(moved_mask(s[i:hi], u[i:hi], d))
        if hit.size == 0:
            i = hi
        else:
            p = i + int(hit[0])
            pos.append(p)
            d = float(s[p])
            i = p + 1
    return np.asarray(pos, dtype=np.int64), d


def segment_emissions(pos, b, cnt, T, B):
    """-> (emitted positions of one segment, cnt afterwards)"""
    if len(pos) <= B:
        return np.zeros(0, dtype=np.int64), cnt
    first = int(pos[B])
    active = b - first
    a0 = max(0, T + 1 - cnt)
    em = np.arange(a0, active, T + 1)
    held = pos[np.searchsorted(pos, first + em, side="right") - 1]
    cnt = 1 + (active - 1 - int(em[-1])) if len(em) else cnt + active
    return held, cnt


def walk(sig, u, groups, d, cnt, T, B, take_all=None, fill=0, capacity=None):
    """The statement of cgs_mh_walk.  sig: fp32 [groups * b]; u: float64 [groups * b]; d: the chain's score (a Python float or an
    np.float32); cnt: its counter.  -> dict(rows, counts, span, d, cnt, fill)"""
    sig = np.asarray(sig).reshape(-1)
    assert sig.dtype == np.float32
    d, cnt, fill = float(d), int(cnt), int(fill)
    n = len(sig)
    b = n // groups
    rows, counts, fill0 = [], [], fill
    for g in range(groups):
        if capacity is not None and fill >= capacity:
            counts.append(-1)
            continue
        if take_all is not None and take_all[g]:
            rows.extend(range(g * b, (g + 1) * b))
            counts.append(b)
            fill += b
            continue
        seg = slice(g * b, (g + 1) * b)
        pos, d = segment_moves(sig[seg], u[seg], d)
        held, cnt = segment_emissions(pos, b, cnt, T, B)
        rows.extend(int(g * b + p) for p in held)
        counts.append(len(held))
        fill += len(held)
    return dict(rows=np.asarray(rows, dtype=np.int32), counts=np.asarray(counts, dtype=np.int32), span=np.asarray([fill0, len(rows)], dtype=np.int64),
                d=d, cnt=cnt, fill=fill)


def scores(kind, n, rs, b=None):
    x = rs.uniform(0, 1, n).astype(f32)
    if kind == "uniform":
        return x
    if kind == "quarters":                                               # ties, exact 0 and 1
        return (np.round(x * 4) / 4).astype(f32)
    if kind == "tiny":                                                   # products s * (1 - d) down to fp32 denormals
        s = (x * f32(1e-6)).astype(f32)
        s[rs.randint(n, size=max(1, n // 16))] = f32(1e-40)
        s[rs.randint(n, size=max(1, n // 16))] = f32(3e-42)
        return s
    if kind == "near1":
        return (f32(1) - x * f32(1e-6)).astype(f32)
    if kind == "constant":                                               # every proposal moves once the chain is there
        return np.full(n, f32(0.37))
    if kind == "increasing":
        return np.sort(rs.uniform(0.01, 0.99, n)).astype(f32)
    if kind == "decreasing":                                             # almost nothing moves: whole windows are passed over
        return (f32(0.9) * np.exp2(-(np.arange(n) % (b or n)).astype(np.float64))).astype(f32)        # per segment
    raise KeyError(kind)


def table():
    """(name, b, groups, kind, T, B, cnt0, seed index): every b x groups x kind, with T, B, the start counter and the seed rotated so that
    every value of each meets every b, every groups and every kind."""
    out, k, seen = [], 0, {t: 0 for t in TS}
    for bi, b in enumerate(BS):
        for gi, groups in enumerate(GROUPS):
            for ki, kind in enumerate(KINDS):
                T = TS[(bi + gi + ki) % 4]
                B = [0, 1, 3, b + 5][(bi + 2 * gi + 3 * ki + k // 4) % 4]          # b + 5: more than the segment can move
                cnt0 = 1 + (seen[T] % (T + 2))                                     # 1 .. T + 2, each in turn
                seen[T] += 1
                out.append((f"b{b}-g{groups}-{kind}-T{T}-B{B}-c{cnt0}-s{k % len(SEEDS)}", b, groups, kind, T, B, cnt0, k % len(SEEDS)))
                k += 1
    return out


TABLE = table()
BY_NAME = {c[0]: c for c in TABLE}
SPECIALS = ["one-10000", "constant-50000", "take-first", "take-middle", "take-last", "take-all", "full-inside", "full-at-segment-end", "full-on-entry",
            "full-after-first-call"]


def case_names():
    return [c[0] for c in TABLE] + SPECIALS


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(b, groups, T, B, seed, cnt0, fill0, capacity, calls: [dict(sig, u, take_all, ref)]) -- two calls, the second continuing the
    chain of the first; ``ref`` is ``walk``'s result."""
    take = [None, None]
    fill0, capacity = 0, None
    if name in SPECIALS:
        rs = np.random.RandomState(1000 + SPECIALS.index(name))
        seed, cnt0, B = 0.48372619384712345, 3, 0
        if name == "one-10000":                                          # the 2-D evaluation's round
            b, groups, kind, T = 10000, 1, "uniform", 20
        elif name == "constant-50000":                                   # the longest serial path a call site reaches
            b, groups, kind, T = 50000, 1, "constant", 20
        elif name.startswith("take-"):
            b, groups, kind, T = 65, 3, "uniform", 1
            flags = {"first": [1, 0, 0], "middle": [0, 1, 0], "last": [0, 0, 1], "all": [1, 1, 1]}[name[5:]]
            take = [np.asarray(flags, dtype=np.uint8), np.asarray(flags[::-1], dtype=np.uint8)]
        else:
            b, groups, kind, T = 64, 4, "uniform", 1
    else:
        _, b, groups, kind, T, B, cnt0, si = BY_NAME[name]
        rs = np.random.RandomState(si * 7919 + b * 31 + groups)
        seed = SEEDS[si]
    n = b * groups
    sigs = [scores(kind, n, rs, b), scores(kind if kind != "constant" else "uniform", n, rs, b)]
    us = [rs.uniform(0, 1, n), rs.uniform(0, 1, n)]
    if name.startswith("full-"):
        free = walk(sigs[0], us[0], groups, seed, cnt0, T, B)["counts"]
        assert free[1] >= 2 and free[0] >= 1
        if name == "full-inside":                                        # reached inside segment 1: segments 2, 3 and the second call are not walked
            capacity = int(free[0]) + 1
        elif name == "full-at-segment-end":
            capacity = int(free[0] + free[1])
        elif name == "full-on-entry":
            fill0 = capacity = 40
        else:                                                            # the first call fills it with its last segment
            capacity = int(free.sum()) - 1
    calls, d, cnt, fill = [], seed, cnt0, fill0
    for sig, u, flags in zip(sigs, us, take):
        ref = walk(sig, u, groups, d, cnt, T, B, take_all=flags, fill=fill, capacity=capacity)
        for a in (sig, u, ref["rows"], ref["counts"], ref["span"]):
            a.setflags(write=False)
        calls.append(dict(sig=sig, u=u, take_all=flags, ref=ref))
        d, cnt, fill = ref["d"], ref["cnt"], ref["fill"]
    return dict(b=b, groups=groups, T=T, B=B, seed=seed, cnt0=cnt0, fill0=fill0, capacity=capacity, calls=calls)


def host_walk(case):
    """The product's host class on a case, one ``walk`` per segment in order, with the skip and take-all rules of the fill loops applied
    outside it -> per call dict(rows, counts, d, cnt, fill) in ``walk``'s form."""
    from cgs_amd.sampling import IndependenceSampler
    h = IndependenceSampler(T=case["T"], B=case["B"])
    h.set_score_curr(case["seed"])
    h.cnt_chain = case["cnt0"]
    b, groups, fill, out = case["b"], case["groups"], case["fill0"], []
    for call in case["calls"]:
        rows, counts = [], []
        for g in range(groups):
            if case["capacity"] is not None and fill >= case["capacity"]:
                counts.append(-1)
                continue
            if call["take_all"] is not None and call["take_all"][g]:
                got = list(range(b))
            else:
                with np.errstate(all="ignore"):
                    got = h.walk(call["sig"][g * b:(g + 1) * b].reshape(b, 1).copy(), call["u"][g * b:(g + 1) * b])
            rows.extend(g * b + r for r in got)
            counts.append(len(got))
            fill += len(got)
        out.append(dict(rows=np.asarray(rows, dtype=np.int32), counts=np.asarray(counts, dtype=np.int32),
                        d=float(np.asarray(h.d_curr).reshape(-1)[0]), cnt=int(h.cnt_chain), fill=fill))
    return out


def fill_model(batches, walk_rows, eval_size, base, max_propose=float("inf"), productive_only=False):
    """The counter rules of the reference's two Metropolis-Hastings fill loops (nsgan/GAN.py:348-376,398-426; synthetic/main.py:182-202,
    229-253 with ``productive_only``), restated independently of ``evaluate.collaborate``: every emitted row goes on a list that is cut to
    ``eval_size`` at the end.  ``batches`` yields (samples, sigmoids); ``walk_rows(sigmoids)`` -> the emitted row indices of one batch.  A
    batch met at or past ``max_propose`` proposals is kept whole without being shown to the chain; with ``productive_only`` a batch that
    yields nothing does not count as proposed.
    -> (samples [eval_size, ...], accepted, proposed)"""
    kept = [base[0][np.asarray(walk_rows(base[1]), dtype=np.int64)]]
    accepted, proposed = kept[0].shape[0], eval_size
    while accepted < eval_size:
        samples, sigmoids = next(batches)
        rows = samples[np.asarray(walk_rows(sigmoids), dtype=np.int64)] if proposed < max_propose else samples
        kept.append(rows)
        accepted += rows.shape[0]
        if rows.shape[0] or not productive_only:
            proposed += samples.shape[0]
    return np.concatenate(kept)[:eval_size], accepted, proposed
