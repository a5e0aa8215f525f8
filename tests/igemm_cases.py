"""The implicit-GEMM launch plans one by one: the planner of csrc/igemm.hip restated in plain Python integers, a float64 reference of
every form, seeded inputs and the case table two tests share (tests/test_igemm_cases_cpu.py checks the restatement against the library's
host-only queries, the table's coverage, the executed-FLOP count and the reference without a device; tests/test_gpu_igemm_plans.py holds
the launches to them).  Not a test module and not a conftest: the tests import it by name.  Exact-fp32 contraction only.

    geometry   conv_call_of (csrc/api.hip), cgs_geom_F / cgs_geom_T: the parity classes in their sorted order, vec, tap_parity, Np
    plan       igemm_plan (what cgs_igemm_launch applies and the host queries read; plan()'s "launch_cfg" is its grid step) in its own
               order: row policy, split-K (time model and slab test), tiles (with the second
               ask without tail_wide), tail split, half / tall (and its second row policy), bin packing, prio_t, uni, xcd_map, gx,
               cls_flip -> Plan: the exact kernel name, the reduce kernel that follows, the executed FLOP count, every plan feature
    brute_flops   the executed count again, by looping over every tile, row and tap
    reference64   oracle.ops_ref on float64 copies of the float32 inputs, the float64 epilogues of smallc_cases.py, and per form: the
               column sums / sums of squares (stats), the norm-backward column sums (nstats), refine_update1 in float64 (update), the
               sign bits of the pre-activation (signs)

The bar is the project's operator bar, unchanged: max|delta| <= 2e-5 max(1, sqrt(K / 1000)) max|ref| with K the longest class's
reduction length, times 1.5 under the forward tanh.  Its reference side (the float32 torch-CPU oracle against the float64 reference over
the table, normalised the same way) is ORACLE_WORST / ORACLE_OF_BAR below.
"""
import collections
import functools

import numpy as np
import torch

from oracle import ops_ref as R
from smallc_cases import (AUX_MARGIN, BWD_EPILOGUES, CONV_BWD_DATA, CONV_FWD, DECONV_BWD_DATA, DECONV_FWD, EPI_AFFINE_RELU, EPI_LRELU,
                          EPI_LRELU_BWD, EPI_NAMES, EPI_NONE, EPI_RELU_BWD_AFFINE, EPI_TANH, EPI_TANH_BWD, FAMILY_IGEMM, _off_zero, _randn,
                          bwd_epilogue64, ceil_div, fwd_epilogue64, layer_of, round_up, same_pad_before)

BK = 32
OP_NAMES = {CONV_FWD: "conv_fwd", CONV_BWD_DATA: "conv_bwd", DECONV_FWD: "deconv_fwd", DECONV_BWD_DATA: "deconv_bwd"}
FORMS = ("plain", "stats", "nstats", "update", "signs")
UPDATE_EPILOGUE, UPDATE_SPLITK, UPDATE_TAIL = 1, 2, 3

# The float32 oracle's worst max|delta| / max|ref| against the float64 reference over the table and its worst share of the bar
# (tests/test_igemm_cases_cpu.py prints every figure and asserts it against these): the reference side of the bar.
ORACLE_WORST, ORACLE_OF_BAR = 2.1e-6, 0.070      # 2.07e-6 = 0.069 of the bar at conv_fwd 2x20x18x32 -> 128, k 5, s 2 under the forward tanh

Cls = collections.namedtuple("Cls", "R C py px nty ntx dy0 dx0 K")
Geometry = collections.namedtuple("Geometry", "op dirT B Hin Win Cred Hout Wout N Np S So dstep nclasses tap_parity vec cls")


def geometry(op, B, H, W, Cin, Ho, Wo, Cout, k, s):
    """igemm_geometry(conv_call_of(...)) -- a linear layer is the 1x1 convolution over a 1x1 image (cgs_linear_fwd / _bwd_data)."""
    L = layer_of(op, H, W, Cin, Ho, Wo, Cout, k, s)
    if not L.dirT:
        c = Cls(L.Hs, L.Ws, 0, 0, L.kh, L.kw, -same_pad_before(L.Hb, L.kh, L.sh), -same_pad_before(L.Wb, L.kw, L.sw), L.kh * L.kw * L.Cb)
        vec = L.Cb % BK == 0 and c.nty <= 16 and c.ntx <= 16
        return Geometry(op, False, B, L.Hb, L.Wb, L.Cb, L.Hs, L.Ws, L.Cs, round_up(L.Cs, 64), L.sh, 1, 1, 1,
                        1 if L.sh == 2 and L.sw == 2 and L.Hs * L.Ws > 64 else 0, vec, (c,))
    assert L.sh <= 2 and L.sw <= 2
    pt, pl = same_pad_before(L.Hb, L.kh, L.sh), same_pad_before(L.Wb, L.kw, L.sw)
    cls = []
    for py in range(L.sh):
        for px in range(L.sw):
            Rr = (L.Hb - py + L.sh - 1) // L.sh if py < L.Hb else 0
            Cc = (L.Wb - px + L.sw - 1) // L.sw if px < L.Wb else 0
            ky0, kx0 = (py + pt) % L.sh, (px + pl) % L.sw
            nty = (L.kh - ky0 + L.sh - 1) // L.sh if ky0 < L.kh else 0
            ntx = (L.kw - kx0 + L.sw - 1) // L.sw if kx0 < L.kw else 0
            cls.append(Cls(Rr, Cc, py, px, nty, ntx, (py + pt - ky0) // L.sh, (px + pl - kx0) // L.sw, nty * ntx * L.Cs))
    vec = L.Cs % BK == 0 and all(c.nty <= 16 and c.ntx <= 16 for c in cls)
    cls.sort(key=lambda c: -c.K)          # heaviest class first (a stable insertion sort in the library; list.sort is stable too)
    return Geometry(op, True, B, L.Hs, L.Ws, L.Cs, L.Hb, L.Wb, L.Cb, round_up(L.Cb, 64), 1, L.sh, -1, L.sh * L.sw, 0, vec, tuple(cls))


def packed_floats(g):
    return sum(round_up(c.K, BK) * g.Np for c in g.cls)


def rows_of(g, c):
    return g.B * c.R * c.C


def valid_taps(g, c, pix):
    """Taps of base pixel ``pix`` of class c that fall inside the input image."""
    r, cc = divmod(pix, c.C)
    ny = sum(0 <= r * g.S + c.dy0 + ta * g.dstep < g.Hin for ta in range(c.nty))
    nx = sum(0 <= cc * g.S + c.dx0 + tb * g.dstep < g.Win for tb in range(c.ntx))
    return ny * nx


def pix_major(g):
    """igemm_pix_major."""
    maxRC = max(c.R * c.C for c in g.cls)
    return bool(g.vec) and g.B >= 128 and 1 < maxRC <= 256 and g.B * g.Hin * g.Win * g.Cred * 4 <= 384 << 20


def row_order(g):
    return 0 if not pix_major(g) else 2 if g.B % 128 == 0 else 1


def lpt_perm(g, c):
    """cgs_igemm_row_policy: base pixels by descending valid-tap count, stable."""
    return sorted(range(c.R * c.C), key=lambda pix: -valid_taps(g, c, pix))


def blocks(g, BN, BM=128):
    return sum(ceil_div(rows_of(g, c), BM) * (g.Np // BN) for c in g.cls)


def choose_splitk(g):
    BN = 128 if g.Np % 128 == 0 else 64
    nb = blocks(g, BN)
    live = [c for c in g.cls if c.R * c.C > 0]
    nk_min = min([ceil_div(c.K, BK) for c in live], default=1 << 30)
    if nb == 0 or nb >= 256 or nk_min < 8:
        return 1
    cap = min(nk_min // 4, 64)
    if cap < 2:
        return 1
    live = [c for c in g.cls if rows_of(g, c) > 0]
    nk_max = max(ceil_div(c.K, BK) for c in live)
    maxM = max(rows_of(g, c) for c in live)
    slice_mb = 0.0
    for c in live:
        slice_mb += float(rows_of(g, c)) * g.Np * 4e-6
    tile = (1.0 if BN == 128 else 0.5) * (0.5 if maxM <= 64 else 1.0)
    best, best_cost = 1, 1e30
    for s in range(2, cap + 1):
        cps = ceil_div(nk_max, s)
        if ceil_div(nk_max, cps) != s:
            continue
        load = (nb * s + 255) // 256
        cost = (1.41 if load == 1 else float(load)) * float(cps) * tile + 0.3 * slice_mb * float(s)
        if cost < best_cost:
            best_cost, best = cost, s
    return best


def splitk_bytes(g):
    s = choose_splitk(g)
    return s * sum(rows_of(g, c) for c in g.cls) * g.Np * 4 if s > 1 else 0


def round_rules(cus):
    return cus in (256, 0)


Tiles = collections.namedtuple("Tiles", "wide mid deep tall wide_for_tail deep_flipped")
Tail = collections.namedtuple("Tail", "start n s clip")
NO_TAIL = Tail(0, 0, 0, None)
State = collections.namedtuple("State", "g splitk pix_major lpt stat_part sign_out cus")


def blocks_per_cu(wide, deep):
    return (2 if wide else 3) if deep else (4 if wide else 5)


def choose_tail(st, wide, deep, tall, pad_ok=False):
    """igemm_choose_tail.  ``pad_ok``: without the refusal of padded ids (only to name the rows on which that refusal binds)."""
    g = st.g
    if not round_rules(st.cus):
        return NO_TAIL
    if not g.vec or st.splitk > 1 or st.stat_part or st.sign_out or g.N & 3 or tall:
        return NO_TAIL
    bn, tbk = 128 if wide else 64, 32 if deep else 16
    cl = g.cls[-1]
    Ml = rows_of(g, cl)
    if Ml <= 0:
        return NO_TAIL
    mtl = ceil_div(Ml, 128)
    Tl = mtl * (g.Np // bn)
    T = blocks(g, bn)
    Lslots = 256 * blocks_per_cu(wide, deep)
    nk = ceil_div(cl.K, tbk)
    if T < 256 or T > Lslots:
        return NO_TAIL
    r = T % 256
    if r == 0 or r > 176:
        return NO_TAIL
    S, clip = (256 + r // 2) // r, None
    if S > 16:
        S, clip = 16, "16"
    if S > nk // 4:
        S, clip = nk // 4, "nk/4"
    if S < 2:
        return NO_TAIL
    r = min(r, Tl)
    if any(rows_of(g, c) != Ml for c in g.cls):
        return NO_TAIL
    xcd = mtl % 8 == 0 or mtl >= 64
    ids = (round_up(mtl, 8) if xcd else mtl) * (g.Np // bn)
    if xcd and mtl % 8 and not pad_ok:
        return NO_TAIL
    return Tail(ids - r, r, S, clip)


def choose_tiles(st, tail_wide=True):
    g = st.g
    vec = bool(g.vec)
    maxRC = max(c.R * c.C for c in g.cls)
    wide, wide_for_tail = g.Np % 128 == 0, False
    if wide and st.lpt and maxRC <= 64:
        nb = sum((rows_of(g, c) // 128) * (g.Np // 128) for c in g.cls)
        if nb < 1024:
            wide = False
        if not wide and tail_wide and vec and st.splitk == 1 and not st.stat_part and not st.sign_out and g.N & 3 == 0 and g.nclasses == 1 and \
                512 <= nb <= 1024 and nb % 256 != 0 and nb % 256 <= 176 and choose_tail(st, True, False, False).s > 1:
            wide = wide_for_tail = True
    mid = 0
    if wide and vec and st.splitk == 1:
        wb = blocks(g, 128)
        if 256 <= wb < 512:
            wide, mid = False, 1
        elif wb < 256 and (st.stat_part or st.sign_out):
            wide, mid = False, 2
    deep, flipped = True, False
    if vec and st.splitk == 1 and not mid:
        bls = [ceil_div(rows_of(g, c), 128) * (g.Np // (128 if wide else 64)) for c in g.cls if rows_of(g, c) > 0]
        deep = min(bls, default=1 << 40) < 512
        if deep and not st.pix_major and g.nclasses > 1 and sum(bls) >= 1024:
            deep, flipped = False, True
    kmax = max(c.K for c in g.cls)
    tall = vec and not wide and not mid and not deep and st.splitk == 1 and g.Np == 64 and st.pix_major and g.B % 256 == 0 and kmax <= 512 and \
        blocks(g, 64, 256) >= 1536
    return Tiles(wide, mid, deep, tall, wide_for_tail and wide, flipped)


def tail_bytes(tl, wide):
    return tl.n * tl.s * 128 * (128 if wide else 64) * 4


def _state(g, splitk=1, stat_part=False, sign_out=False, cus=256, BM=128):
    pm = pix_major(g)
    return State(g, splitk, pm, pm and g.B % BM == 0, stat_part, sign_out, cus)


def slab_bytes(g, cus=256):
    """cgs_igemm_slab_bytes: what cgs_conv_ws_bytes_for adds behind the packed weights."""
    sk = splitk_bytes(g)
    if sk:
        return sk
    st = _state(g, cus=cus)
    t = choose_tiles(st)
    tl = choose_tail(st, t.wide, t.deep, t.tall)
    return tail_bytes(tl, t.wide) if tl.s > 1 else 0


def _tiles_and_tail(st, slab):
    """The launcher's two asks: tiles and tail, again without tail_wide when the slab has no room for the tail the wide tiles were for."""
    tiles = choose_tiles(st)
    tl = choose_tail(st, tiles.wide, tiles.deep, tiles.tall)
    fits = tl.s > 1 and slab >= tail_bytes(tl, tiles.wide)
    refused = False
    if tiles.wide_for_tail and not fits:
        refused = True
        tiles = choose_tiles(st, False)
        tl = choose_tail(st, tiles.wide, tiles.deep, tiles.tall)
        fits = tl.s > 1 and slab >= tail_bytes(tl, tiles.wide)
    return tiles, tl, fits, refused


def update_form(g, slab, cus=256):
    """cgs_igemm_update_form (epilogue none, no bias: what the *_bwd_data_update entry points pass)."""
    if not g.vec or g.N & 3:
        return 0
    need = splitk_bytes(g)
    if need and slab >= need:
        return UPDATE_SPLITK
    tiles, _, fits, _ = _tiles_and_tail(_state(g, cus=cus), slab)
    if tiles.tall:
        return 0
    return UPDATE_TAIL if fits else UPDATE_EPILOGUE


def signs_ok(g, epilogue):
    return g.N % 32 == 0 and epilogue in (EPI_AFFINE_RELU, EPI_LRELU) and choose_splitk(g) <= 1


def stat_rows(g):
    """cgs_conv_stat_layout at one group / cgs_conv_stat_partials: partial rows of the launch, 0 = not offered."""
    if g.N & 3 or len({c.R * c.C for c in g.cls}) != 1 or g.cls[0].R * g.cls[0].C <= 0:
        return 0
    return 2 * ceil_div(rows_of(g, g.cls[0]), 128) * g.nclasses


def count_flops(g, pm, BM):
    """cgs_igemm_count_flops."""
    macs = 0
    for c in g.cls:
        M, ntaps = rows_of(g, c), c.nty * c.ntx
        if not (g.vec and pm):
            macs += M * g.N * g.Cred * ntaps
            continue
        for m0 in range(0, M, BM):
            ml = min(m0 + BM - 1, M - 1)
            pf, pl = m0 // g.B, ml // g.B
            macs += (ml - m0 + 1) * g.N * g.Cred * (valid_taps(g, c, pf) if pf == pl else ntaps)
    return 2 * macs


def brute_flops(g, pm, BM):
    """The same count by brute force: every tile, every row's base pixel, every tap of a one-pixel tile tried against the image."""
    total = 0
    for c in g.cls:
        M, RC = rows_of(g, c), c.R * c.C
        for m0 in range(0, M, BM):
            m = np.arange(m0, min(m0 + BM, M))
            pix = m // g.B if pm else m % RC
            taps = 0
            one = g.vec and pm and bool((pix == pix[0]).all())
            r, cc = divmod(int(pix[0]), c.C)
            for ta in range(c.nty):
                for tb in range(c.ntx):
                    iy, ix = r * g.S + c.dy0 + ta * g.dstep, cc * g.S + c.dx0 + tb * g.dstep
                    taps += 1 if not one or (0 <= iy < g.Hin and 0 <= ix < g.Win) else 0
            total += len(m) * taps * g.N * g.Cred
    return 2 * total


Plan = collections.namedtuple(
    "Plan", "kernel twin BM BN TBK vec par row_order lpt perm perm_moved binpacked splitk nclasses empty_slices reduce half tall wide mid deep "
            "deep_flipped wide_for_tail tail_n tail_s tail_from tail_clip xcd_map padded_ids gx cls_flip uni prio_t flops ragged n_mod4 "
            "update refused tail_pad_refused")


def plan(g, slab, form="plain", epilogue=EPI_NONE, cus=256):
    """igemm_plan for a launch of geometry ``g`` with ``slab`` bytes of workspace behind its packed weights.
    ``form`` sets stat_part (stats, nstats), the norm-backward twin (nstats), sign_out (signs), up_mom (update) as the entry points do.
    ``refused``: the launcher returns an error instead (a form the call does not offer)."""
    assert form in FORMS
    stat_part, ns, sign_out, up = form in ("stats", "nstats"), form == "nstats", form == "signs", form == "update"
    refused = (stat_part and (g.N & 3 or epilogue != EPI_NONE or stat_rows(g) == 0)) or (sign_out and not signs_ok(g, epilogue))
    maxRC = max(c.R * c.C for c in g.cls)
    st = _state(g, stat_part=stat_part, sign_out=sign_out, cus=cus)
    need = 0 if sign_out else splitk_bytes(g)
    if need and slab >= need:
        st = st._replace(splitk=choose_splitk(g))
    tiles, tl, fits, narrow = _tiles_and_tail(st, slab)
    wide, deep, tall = tiles.wide, tiles.deep, tiles.tall
    BMp = 256 if tall else 128
    if tall:
        st = st._replace(lpt=st.pix_major and g.B % 256 == 0)
    perm = [lpt_perm(g, c) for c in g.cls] if st.lpt else None
    flops = count_flops(g, st.pix_major, BMp)
    pad_refused = tl.s <= 1 and choose_tail(st, wide, deep, tall, pad_ok=True).s > 1
    if not fits:
        tl = NO_TAIL
    vec = bool(g.vec)
    bn = 128 if wide else 64
    per_cu = blocks_per_cu(wide, deep) if vec else 2
    total_blocks = blocks(g, bn)
    one_round = round_rules(cus) and vec and st.splitk == 1 and not tall and 256 <= total_blocks <= 256 * per_cu
    prio = vec and not deep and st.splitk == 1 and st.pix_major and total_blocks >= 256
    nblk_n = g.Np // bn
    binpacked = bool(one_round and st.lpt and g.nclasses == 1 and g.B // 128 == 8 and 32 % nblk_n == 0)
    if binpacked:
        c = g.cls[0]
        RC, nbins = c.R * c.C, 32 // nblk_n
        cap = ceil_div(RC, nbins)
        load, items = [0] * nbins, [[] for _ in range(nbins)]
        for pix in perm[0]:
            best = -1
            for b in range(nbins):
                if len(items[b]) < ceil_div(RC - b, nbins) and len(items[b]) < cap and (best < 0 or load[b] < load[best]):
                    best = b
            items[best].append(pix)
            load[best] += valid_taps(g, c, pix)
        packed = list(perm[0])
        for b in range(nbins):
            for k, pix in enumerate(items[b]):
                packed[b + k * nbins] = pix
        perm[0] = packed
    uni = 0 if g.nclasses > 1 and wide and maxRC <= 64 else 1
    half = vec and wide and deep and st.splitk > 1 and not g.tap_parity and g.B * maxRC <= 64
    upd = 0
    if up:
        upd = UPDATE_SPLITK if st.splitk > 1 else UPDATE_TAIL if tl.s > 1 else UPDATE_EPILOGUE
        if not vec or tall or update_form(g, slab, cus) != upd:
            refused = True
    twin = 2 if up and st.splitk == 1 and not half and not tall and vec else 1 if ns else 0
    par = bool(g.tap_parity)
    if half:
        BM, BN, TBK, V, P = 64, 128, 32, True, False
    elif tall:
        BM, BN, TBK, V, P = 256, 64, 16, True, par
    elif vec:
        BM, BN, TBK, V, P = 128, bn, 32 if deep else 16, True, par
    else:
        BM, BN, TBK, V, P = 128, bn, 16, False, False
    name = "%s<%d, %d, 4, %s, %d, %s>" % (("igemm_kernel", "igemm_ns_kernel", "igemm_up_kernel")[twin], BM, BN, "true" if V else "false", TBK,
                                           "true" if P else "false")
    # launch_cfg
    maxM = max(rows_of(g, c) for c in g.cls)
    mtiles = ceil_div(maxM, BM)
    xcd = 1 if mtiles % 8 == 0 or mtiles >= 64 else 0
    gx = (round_up(mtiles, 8) if xcd else mtiles) * (g.Np // BN)
    if tl.s > 1:
        assert tl.start + tl.n == gx, "the tail planner and launch_cfg disagree on the grid"
        gx = tl.start + tl.n * tl.s
    sk = st.splitk
    total = gx * g.nclasses * sk
    flip = 0
    if round_rules(cus) and g.nclasses > 1 and not st.pix_major and 256 < total <= 512 and gx > 0 and 256 % gx == 0 and tl.s <= 1:
        per_round = 256 // gx
        if sk > 1 and per_round % g.nclasses == 0:
            flip = g.nclasses
        elif sk == 1 and per_round < g.nclasses and g.nclasses % per_round == 0:
            flip = per_round
    reduce = "none"
    if tl.s > 1:
        reduce = "tail_reduce_kernel<%s>" % ("true" if up else "false")
    if sk > 1:
        reduce = "splitk_reduce_stats_kernel" if stat_part else "splitk_reduce_kernel<%s>" % ("true" if up else "false")
    empty = False
    if sk > 1:
        for c in g.cls:          # (the kernel slices every class by its own K tiles: cps = ceil(nk / splitk), igemm_body)
            nk = ceil_div(c.K, TBK)
            cps = ceil_div(nk, sk)
            empty = empty or (rows_of(g, c) > 0 and (sk - 1) * cps >= nk)
    ragged = any(rows_of(g, c) % BM for c in g.cls)
    moved = bool(perm) and any(p != list(range(len(p))) for p in perm)
    return Plan(name, twin, BM, BN, TBK, V, P, 0 if not st.pix_major else 2 if st.lpt else 1, st.lpt, perm, moved, binpacked, sk, g.nclasses,
                empty, reduce, bool(half), bool(tall), wide, tiles.mid, deep, tiles.deep_flipped,
                "taken" if tiles.wide_for_tail else "refused" if narrow else None, tl.n, tl.s, tl.start, tl.clip if tl.s > 1 else None, xcd,
                bool(xcd and mtiles % 8), gx, flip, uni, (85, 170, 0) if prio else (0, 0, 0), flops, ragged, g.N % 4, upd, bool(refused), pad_refused)


# ---- a call, as the tables and the tests name it -------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "op B H W Cin Cout k s form epilogue slab why")


def out_hw(case):
    """(Ho, Wo) of the call: a conv's strided side; a deconv's output is 2H x 2W, or 2H-1 x 2W-1 where ``why`` asks for the odd size."""
    if case.op in (CONV_FWD, CONV_BWD_DATA):
        return ceil_div(case.H, case.s), ceil_div(case.W, case.s)
    odd = 1 if "2H-1" in case.why else 0
    return case.s * case.H - odd * (case.s - 1), case.s * case.W - odd * (case.s - 1)


def case_geometry(case):
    Ho, Wo = out_hw(case)
    return geometry(case.op, case.B, case.H, case.W, case.Cin, Ho, Wo, case.Cout, case.k, case.s)


def query_geometry(case):
    """The geometry cgs_conv_ws_bytes_for sizes the slab for: a deconv's output bounded by stride x input."""
    return geometry(case.op, case.B, case.H, case.W, case.Cin, case.H * case.s, case.W * case.s, case.Cout, case.k, case.s)


def ws_bytes(lib, case):
    """The workspace the row names: "full" = what kernels._WsCache hands the call, "none" = the fp32 packed weights alone, no slab."""
    c = case
    if c.slab == "full":
        return max(int(lib.cgs_conv_ws_bytes_for(c.op, c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.s, c.s)), 16)
    return none_ws_bytes(c)


def none_ws_bytes(case):
    """The fp32 packed weights and not a byte more (cgs_conv_ws_bytes sizes some geometries at 6 bytes per weight for the split-bf16 form:
    that would leave a slab behind the fp32 image)."""
    return max(4 * packed_floats(case_geometry(case)), 16)


def case_plan(lib, case, cus=256):
    g = case_geometry(case)
    return plan(g, ws_bytes(lib, case) - 4 * packed_floats(g), case.form, case.epilogue, cus)


def case_id(case):
    return "%s-%dx%dx%dx%d-%d-k%ds%d-%s-%s-%s" % (OP_NAMES[case.op], case.B, case.H, case.W, case.Cin, case.Cout, case.k, case.s, case.form,
                                                   EPI_NAMES[case.epilogue], case.slab) + ("-odd" if "2H-1" in case.why else "")


def macs(case):
    g = case_geometry(case)
    return sum(rows_of(g, c) * c.K for c in g.cls) * g.N


def kmax(case):
    return max(c.K for c in case_geometry(case).cls)


def bar(case):
    return (1.5 if case.epilogue == EPI_TANH else 1.0) * 2e-5 * max(1.0, (kmax(case) / 1000.0) ** 0.5)


MAC_BUDGET = 2.25e9       # "about 2 GMAC" per float64 reference

F, BD, TF, TB = CONV_FWD, CONV_BWD_DATA, DECONV_FWD, DECONV_BWD_DATA


def _c(op, B, H, W, Cin, Cout, k, s, form="plain", epilogue=EPI_NONE, slab="full", why=""):
    return Case(op, B, H, W, Cin, Cout, k, s, form, epilogue, slab, why)


# (op, B, H, W, Cin, Cout, k, s, form, epilogue, slab, what the row is there for).  H, W, Cin, Cout are the entry point's: the input side of the
# forward ops, the side the gradient is taken w.r.t. for the backward-data ops; a linear layer is k = 1, s = 1 over a 1x1 image.
CASES = [
    # ---- generic K (non-VEC) ----
    _c(F, 3, 5, 7, 3, 20, 3, 1, epilogue=EPI_LRELU, why="non-VEC 128x64: Cred = 3, K = 27, N off the 64 grid, ragged image-major tile"),
    _c(F, 2, 6, 5, 20, 128, 3, 2, epilogue=EPI_TANH, why="non-VEC 128x128: Cred % 32 != 0 with K % 16 != 0, tanh"),
    _c(TF, 3, 5, 4, 20, 24, 1, 2, why="non-VEC transposed 1x1 stride 2: three classes with zero taps"),
    _c(TF, 2, 3, 4, 24, 40, 5, 2, epilogue=EPI_AFFINE_RELU, why="non-VEC transposed 2H-1: classes of unequal RxC, 9/6/6/4 taps, affine_relu"),
    _c(F, 1, 1, 1, 100, 70, 1, 1, why="linear, B = 1, 1x1 spatial, non-VEC"),
    # ---- VEC, image-major, small ----
    _c(F, 1, 1, 1, 64, 64, 1, 1, why="linear, B = 1, VEC 128x64 32-deep"),
    _c(F, 3, 9, 7, 32, 128, 3, 1, epilogue=EPI_AFFINE_RELU, why="VEC 128x128 32-deep natural order, ragged image-major tile, affine_relu"),
    _c(F, 2, 20, 18, 32, 64, 3, 2, epilogue=EPI_LRELU, why="VEC 128x64 32-deep parity tap order (stride 2, 90 base pixels)"),
    _c(F, 2, 20, 18, 32, 128, 5, 2, epilogue=EPI_TANH, why="VEC 128x128 32-deep parity tap order, 5x5"),
    _c(TF, 2, 5, 6, 32, 64, 5, 2, epilogue=EPI_TANH, why="VEC transposed 2H-1: four classes of unequal RxC, uni = 1"),
    _c(TF, 2, 4, 4, 32, 128, 4, 2, epilogue=EPI_LRELU, why="VEC transposed four equal classes, wide, grid <= 8x8: uni = 0"),
    _c(TF, 2, 3, 3, 32, 32, 3, 2, "signs", EPI_LRELU, why="signs form on a tiny grid: mid by the sign rule does not apply at Np = 64"),
    _c(TF, 1, 2, 2, 32, 128, 3, 2, "signs", EPI_AFFINE_RELU, why="signs form, Np = 128: mid by the statistics / sign-mask rule"),
    _c(BD, 2, 9, 7, 64, 32, 3, 1, epilogue=EPI_RELU_BWD_AFFINE, why="conv backward-data stride 1 (one class), relu' affine"),
    _c(BD, 2, 10, 6, 32, 64, 4, 2, epilogue=EPI_LRELU_BWD, why="conv backward-data stride 2: four classes, lrelu'"),
    _c(TB, 2, 5, 7, 64, 32, 4, 2, epilogue=EPI_TANH_BWD, why="deconv backward-data (forward direction over dy), tanh'"),
    # ---- split-K ----
    _c(F, 64, 1, 1, 1024, 128, 1, 1, epilogue=EPI_LRELU, why="linear split-K, 64 rows: half (64-row tile), lrelu through the reduce"),
    _c(BD, 64, 1, 1, 512, 1024, 1, 1, why="linear backward split-K, half"),
    _c(F, 4, 4, 4, 256, 70, 3, 1, epilogue=EPI_TANH, why="split-K one class, N % 4 != 0, tanh through the reduce"),
    _c(F, 4, 4, 4, 256, 64, 3, 1, epilogue=EPI_AFFINE_RELU, why="split-K one class, affine_relu through the reduce"),
    _c(F, 4, 4, 4, 256, 64, 3, 1, epilogue=EPI_AFFINE_RELU, slab="none", why="the same without a slab: not split"),
    _c(TF, 2, 4, 4, 128, 64, 5, 2, why="split-K four classes of 9/6/6/4 taps, every class sliced by its own K tiles"),
    _c(BD, 2, 8, 8, 64, 128, 5, 2, epilogue=EPI_RELU_BWD_AFFINE, why="split-K four classes, relu' affine through the reduce"),
    _c(BD, 2, 8, 8, 64, 128, 5, 2, epilogue=EPI_LRELU_BWD, why="split-K four classes, lrelu' through the reduce"),
    _c(TB, 4, 4, 4, 64, 256, 3, 2, epilogue=EPI_TANH_BWD, why="split-K, tanh' through the reduce"),
    _c(F, 4, 8, 8, 256, 64, 3, 2, "stats", why="split-K with statistics: splitk_reduce_stats_kernel"),
    _c(F, 4, 8, 8, 256, 64, 3, 2, "stats", slab="none", why="statistics without a slab: the one-pass epilogue"),
    _c(BD, 4, 8, 8, 64, 256, 3, 2, "nstats", why="norm-backward sums through splitk_reduce_stats_kernel (igemm_ns_kernel launched)"),
    _c(BD, 4, 8, 8, 64, 256, 3, 2, "nstats", slab="none", why="norm-backward sums from the one-pass epilogue of igemm_ns_kernel"),
    _c(BD, 4, 8, 8, 64, 256, 3, 2, "update", why="fused update through splitk_reduce_kernel<true>"),
    _c(BD, 4, 8, 8, 64, 256, 3, 2, "update", slab="none", why="fused update in the epilogue of igemm_up_kernel"),
    _c(BD, 1, 1, 1, 256, 512, 5, 2, why="split-K, image-major, whole K slices per round: cls_flip = nclasses"),
    # ---- many-block grids: row orders, 16-deep tiles, the round rules ----
    _c(BD, 128, 2, 2, 32, 32, 2, 1, why="row order 2 (whole-tile pixel-major), a heaviest-first permutation that is not the identity"),
    _c(F, 130, 8, 8, 32, 32, 3, 1, epilogue=EPI_LRELU, why="row order 1 (ragged pixel-major), xcd_map on with mtiles % 8 != 0: padded ids"),
    _c(F, 130, 2, 2, 32, 32, 3, 1, why="row order 1, ragged last m-tile, xcd_map off"),
    _c(F, 1024, 7, 7, 32, 32, 3, 1, epilogue=EPI_TANH, why="one round of whole-tile pixel-major blocks at B = 1024: the bin-packed permutation"),
    _c(F, 256, 16, 16, 32, 32, 3, 1, why="pixel-major 16-deep launch of >= 256 blocks: prio_t"),
    _c(BD, 8, 32, 32, 512, 32, 1, 2, why="256..511 blocks of 128x128: mid by the block-slot rule"),
    _c(BD, 64, 32, 32, 32, 32, 3, 2, why="image-major, four classes over two rounds: cls_flip = per_round < nclasses"),
    _c(TF, 32, 32, 32, 32, 32, 3, 2, epilogue=EPI_LRELU, why="four classes that together fill 1024 slots: deep flipped, 128x64 16-deep"),
    _c(BD, 32, 32, 32, 512, 32, 1, 2, why="128x128 16-deep natural order"),
    _c(F, 64, 32, 32, 32, 512, 1, 2, epilogue=EPI_LRELU, why="128x128 16-deep parity tap order"),
    _c(F, 256, 32, 32, 32, 32, 3, 2, epilogue=EPI_TANH, why="128x64 16-deep parity tap order"),
    _c(BD, 2048, 14, 14, 32, 32, 3, 2, why="tall 256x64 tiles, natural order, second row policy at 256"),
    _c(TB, 2048, 14, 14, 32, 32, 1, 2, why="tall 256x64 tiles, parity tap order"),
    # ---- the update twin, tile by tile ----
    _c(BD, 1, 1, 1, 128, 32, 1, 1, "update", why="igemm_up_kernel 128x128 32-deep (linear backward)"),
    _c(TB, 1, 9, 9, 128, 32, 1, 2, "update", why="igemm_up_kernel 128x128 32-deep parity"),
    _c(BD, 3, 5, 5, 32, 32, 3, 1, "update", slab="none", why="igemm_up_kernel 128x64 32-deep, image-major (with a slab the call is split 2 ways)"),
    _c(TB, 1, 9, 9, 32, 32, 1, 2, "update", why="igemm_up_kernel 128x64 32-deep parity"),
    _c(BD, 32, 32, 32, 512, 32, 1, 2, "update", why="igemm_up_kernel 128x128 16-deep"),
    _c(TB, 16, 32, 32, 512, 32, 1, 2, "update", why="igemm_up_kernel 128x128 16-deep parity"),
    _c(BD, 64, 32, 32, 32, 32, 1, 1, "update", why="igemm_up_kernel 128x64 16-deep"),
    _c(TB, 64, 32, 32, 32, 32, 1, 2, "update", why="igemm_up_kernel 128x64 16-deep parity"),
    # ---- the norm-backward twin, tile by tile ----
    _c(BD, 8, 3, 3, 128, 64, 2, 1, "nstats", why="igemm_ns_kernel 128x128 32-deep"),
    _c(TB, 1, 9, 9, 128, 64, 2, 2, "nstats", why="igemm_ns_kernel 128x128 32-deep parity"),
    _c(TB, 1, 9, 9, 32, 32, 3, 2, "nstats", why="igemm_ns_kernel 128x64 32-deep parity"),
    _c(BD, 64, 32, 32, 32, 32, 1, 1, "nstats", why="igemm_ns_kernel 128x64 16-deep"),
    _c(TB, 64, 32, 32, 32, 32, 1, 2, "nstats", why="igemm_ns_kernel 128x64 16-deep parity"),
    _c(BD, 32, 32, 32, 512, 32, 1, 2, "nstats", why="igemm_ns_kernel 128x128 16-deep"),
    _c(BD, 2048, 14, 14, 32, 32, 1, 2, "nstats", why="igemm_ns_kernel tall"),
    _c(BD, 32, 32, 32, 256, 32, 1, 2, "nstats", why="igemm_ns_kernel 128x128 32-deep, not split: its one-pass norm-backward epilogue"),
    _c(TB, 1, 9, 9, 32, 32, 3, 2, "nstats", slab="none", why="igemm_ns_kernel 128x64 32-deep parity, not split: its one-pass epilogue"),
    _c(F, 32800, 1, 1, 256, 32, 1, 1, why="257 tiles, one past a whole round, per-XCD decode: the tail split refused for its padded ids"),
    _c(BD, 3, 5, 5, 20, 24, 3, 1, "nstats", why="igemm_ns_kernel non-VEC 128x64"),
    _c(BD, 3, 5, 5, 128, 20, 3, 1, "nstats", why="igemm_ns_kernel non-VEC 128x128"),
    _c(TB, 16, 32, 32, 512, 32, 1, 2, "nstats", why="igemm_ns_kernel 128x128 16-deep parity"),
    _c(BD, 1, 1, 1, 128, 64, 2, 1, "nstats", why="igemm_ns_kernel on the 64-row tile of a split launch"),
    _c(TB, 2048, 14, 14, 32, 32, 1, 2, "nstats", why="igemm_ns_kernel tall, parity"),
    # ---- tail split ----
    _c(F, 4096, 3, 3, 64, 32, 2, 1, epilogue=EPI_AFFINE_RELU, why="tail: bn 64, one class, xcd_map on, S clipped by nk/4, affine_relu through tail_reduce_kernel"),
    _c(BD, 4096, 3, 3, 32, 64, 2, 1, epilogue=EPI_LRELU_BWD, why="tail: an aux epilogue through tail_reduce_kernel"),
    _c(BD, 4096, 3, 3, 32, 64, 2, 1, "update", why="tail: the update through tail_reduce_kernel<true>"),
    _c(BD, 4096, 3, 3, 32, 64, 2, 1, "update", slab="none", why="the same without a slab: the epilogue of igemm_up_kernel"),
    _c(TF, 1024, 3, 3, 64, 32, 4, 2, epilogue=EPI_TANH, why="tail: four equal classes"),
    _c(BD, 130, 8, 8, 512, 64, 4, 2, epilogue=EPI_RELU_BWD_AFFINE, why="tail: xcd_map off"),
    _c(F, 2048, 3, 3, 32, 512, 2, 1, epilogue=EPI_LRELU, why="tail: wide_for_tail taken, bn 128"),
    _c(F, 2048, 3, 3, 32, 512, 2, 1, epilogue=EPI_LRELU, slab="none", why="wide_for_tail refused for lack of slab: the narrow plan"),
    _c(F, 33700, 1, 1, 2048, 32, 1, 1, why="tail: eight tiles past a whole round, S clipped by 16 (linear, 264 tiles, the last ragged)"),
    _c(BD, 130, 4, 4, 32, 512, 5, 2, why="split-K four classes of 9/6/6/4 taps at ragged pixel-major rows: empty slices"),
]


# ---- inputs (seeded float32) and the float64 reference --------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "x w bias a b aux theta m mean invstd gamma beta seed")
RATE, ALPHA, LEAK = 0.1, 0.9, 0.2


def shapes(case):
    """-> (input, weight, output) shapes of the call."""
    c = case
    Ho, Wo = out_hw(c)
    if c.op == CONV_FWD:
        return (c.B, c.H, c.W, c.Cin), (c.k, c.k, c.Cin, c.Cout), (c.B, Ho, Wo, c.Cout)
    if c.op == DECONV_FWD:
        return (c.B, c.H, c.W, c.Cin), (c.k, c.k, c.Cout, c.Cin), (c.B, Ho, Wo, c.Cout)
    if c.op == CONV_BWD_DATA:
        return (c.B, Ho, Wo, c.Cout), (c.k, c.k, c.Cin, c.Cout), (c.B, c.H, c.W, c.Cin)
    return (c.B, Ho, Wo, c.Cout), (c.k, c.k, c.Cout, c.Cin), (c.B, c.H, c.W, c.Cin)


def linear64(case, x, w):
    """The call's contraction in float64, no bias, no epilogue."""
    c = case
    xs, ws, os_ = shapes(c)
    zero = torch.zeros(os_[3], dtype=x.dtype)
    if c.op == CONV_FWD:
        return R.conv2d(x, w, zero, c.s, c.s)
    if c.op == DECONV_FWD:
        return R.deconv2d(x, w, zero, os_, c.s, c.s)
    if c.op == CONV_BWD_DATA:          # the transposed convolution of dy with the conv's weights viewed as [k, k, N = Cin, Cs = Cout]
        return R.deconv2d(x, w, zero, os_, c.s, c.s)
    return R.conv2d(x, w, zero, c.s, c.s)       # deconv backward-data: the strided conv of dy with [k, k, Cout, Cin] read as HWIO


def _draw(case, seed):
    c = case
    xs, ws, os_ = shapes(c)
    N = os_[3]
    fwd = c.op in (CONV_FWD, DECONV_FWD)
    aux = None
    if c.epilogue == EPI_TANH_BWD:
        aux = torch.tanh(_randn(os_, seed + 7))
    elif c.epilogue >= EPI_RELU_BWD_AFFINE:
        aux = _off_zero(_randn(os_, seed + 6))
    mean, invstd, gamma, beta = _randn((N,), seed + 10, 0.1), _randn((N,), seed + 11).abs() + 0.5, _randn((N,), seed + 12).abs() + 0.5, \
        _randn((N,), seed + 13, 0.3)
    if c.form == "nstats":      # the norm's input x: elements whose pre-activation scale * x + shift is near zero are moved out to +-4 AUX_MARGIN
        aux = _randn(os_, seed + 6).double()
        sc = gamma.double() * invstd.double()
        sh = beta.double() - mean.double() * sc
        u = aux * sc + sh
        aux = torch.where(u.abs() < 2 * AUX_MARGIN, (torch.where(u < 0, -4 * AUX_MARGIN, 4 * AUX_MARGIN) - sh) / sc, aux).float()
    return Inputs(_randn(xs, seed), _randn(ws, seed + 1, 0.7 / max(kmax(c), 1) ** 0.5), _randn((N,), seed + 2, 0.2) if fwd else None,
                  _randn((N,), seed + 3).abs() + 0.5, _randn((N,), seed + 4, 0.3), aux,
                  _randn(os_, seed + 8, RATE) if c.form == "update" else None, _randn(os_, seed + 9, 0.1) if c.form == "update" else None,
                  mean, invstd, gamma, beta, seed)


def sign_deciding(case, inp, lin):
    """The float64 values whose sign the call's result hangs on (None: none): the aux tensor of relu' / lrelu', the pre-activation of the
    signs form, the norm's pre-activation scale * x + shift of the nstats form."""
    if case.form == "signs":
        v = lin + inp.bias.double()
        return inp.a.double() * v + inp.b.double() if case.epilogue == EPI_AFFINE_RELU else v
    if case.form == "nstats":
        sc = inp.gamma.double() * inp.invstd.double()
        return inp.aux.double() * sc + (inp.beta.double() - inp.mean.double() * sc)
    if case.epilogue in (EPI_RELU_BWD_AFFINE, EPI_LRELU_BWD):
        return inp.aux.double()
    return None


@functools.lru_cache(maxsize=4)
def inputs_and_reference(case):
    """-> (Inputs, lin): seeded inputs and the float64 contraction.  Seeds are rejected and redrawn until no sign-deciding value lies
    within AUX_MARGIN of zero."""
    c = case
    seed0 = 15485863 + 7919 * c.B + 131 * c.H + 17 * c.W + 5 * c.Cin + 3 * c.Cout + c.k + 2 * c.s + 31 * c.op
    for attempt in range(64):
        inp = _draw(c, seed0 + 1000 * attempt)
        with torch.no_grad():
            lin = linear64(c, inp.x.double(), inp.w.double())
            v = sign_deciding(c, inp, lin)
        if v is None or float(v.abs().min()) >= AUX_MARGIN:
            return inp, lin
    raise AssertionError(f"{case_id(c)}: no seed keeps the sign-deciding values {AUX_MARGIN} off zero")


def expected64(case, inp, lin):
    """The float64 result of the call: a dict of what the form leaves."""
    c = case
    fwd = c.op in (CONV_FWD, DECONV_FWD)
    if c.form == "update":
        g = lin
        m = RATE * g + ALPHA * inp.m.double()        # refine_update1, not the first step: m <- alpha m + rate g, theta <- theta - m
        return {"theta": inp.theta.double() - m, "m": m}
    if c.form == "signs":
        pre = sign_deciding(c, inp, lin)
        return {"out": fwd_epilogue64(lin, inp.bias, c.epilogue, inp.a, inp.b), "signs": pre > 0}
    if fwd:
        out = fwd_epilogue64(lin, inp.bias, c.epilogue, inp.a, inp.b)
    else:
        out = bwd_epilogue64(lin, c.epilogue, a=inp.a, aux=inp.aux)
    res = {"out": out}
    flat = out.reshape(-1, out.shape[-1])
    if c.form == "stats":
        res["sum"], res["sumsq"] = flat.sum(0), (flat * flat).sum(0)
    if c.form == "nstats":
        sc = inp.gamma.double() * inp.invstd.double()
        x = inp.aux.double().reshape(flat.shape)
        u = x * sc + (inp.beta.double() - inp.mean.double() * sc)
        d = flat * torch.where(u > 0, torch.ones_like(u), torch.full_like(u, LEAK))
        res["sum"], res["sumsq"] = d.sum(0), (d * (x - inp.mean.double()) * inp.invstd.double()).sum(0)
    return res


def oracle32(case, inp):
    """The float32 torch-CPU oracle of the call's stored tensor (the reference side of the bar)."""
    c = case
    with torch.no_grad():
        lin = linear64(c, inp.x, inp.w)
        if c.form == "update":
            return inp.theta - (RATE * lin + ALPHA * inp.m)
        if c.op in (CONV_FWD, DECONV_FWD):
            return fwd_epilogue64(lin, None, c.epilogue, inp.a, inp.b) if inp.bias is None else _fwd32(lin + inp.bias, c.epilogue, inp.a, inp.b)
        return _bwd32(lin, c.epilogue, inp.a, inp.aux)


def _fwd32(v, e, a, b):
    return torch.maximum(v, 0.2 * v) if e == EPI_LRELU else torch.tanh(v) if e == EPI_TANH else torch.relu(a * v + b) if e == EPI_AFFINE_RELU else v


def _bwd32(lin, e, a, aux):
    if e == EPI_RELU_BWD_AFFINE:
        return torch.where(aux > 0, lin * a, torch.zeros_like(lin))
    if e == EPI_LRELU_BWD:
        return torch.where(aux > 0, lin, 0.2 * lin)
    return lin * (1.0 - aux * aux) if e == EPI_TANH_BWD else lin
