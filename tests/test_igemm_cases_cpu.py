"""tests/igemm_cases.py without a device: the restated planner against the library's host-only queries (on the table and on a sweep of a few
thousand geometries around it), the table's coverage of the plan features, the executed-FLOP count by brute force, the size budget of
the float64 references, and the float32 oracle's own distance from the float64 reference (the reference side of the bar).  Without a
device the library's round rules are on, so the restatement is compared at cus = 256.  Run with -s for the figures and the coverage list.

cgs_conv_igemm_plan returns the library's whole plan of a call without launching it; on every table row and on every sweep call, in every
form its entry points offer and at the sweep's three workspaces, it is compared with plan() field by field: the kernel name, the reduce
kernel, the tail, xcd_map, cls_flip, uni, gx, the split-K factor, prio_t, the row order, the executed FLOPs, every class's permutation
(bin packing included) and whether the launcher would refuse the form."""
import ctypes
import random

import pytest
import torch

import igemm_cases as IC
from igemm_cases import BD, F, TB, TF


@pytest.fixture(scope="module")
def lib():
    from cgs_amd import lib as L
    return L.load()


def whole_batch(g):
    return 0x7fffffff // (4 * max(g.Hin * g.Win * g.Cred, g.Hout * g.Wout * g.N)) >= g.B


def lib_family(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s, epilogue, nbytes):
    return int(lib.cgs_conv_family(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, epilogue, nbytes))


def check_call(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s):
    """Every host-only query of the library about one call against the restatement.  -> the number of comparisons made."""
    g = IC.geometry(op, B, H, W, Cin, Ho, Wo, Cout, k, s)
    packed_ws = int(lib.cgs_conv_ws_bytes(op, k, k, s, s, Cin, Cout))
    full = int(lib.cgs_conv_ws_bytes_for(op, B, H, W, Cin, Cout, k, k, s, s))
    # the slab: split-K slabs S x sum M_i x Np x 4, or the tail's n x s x 128 x bn x 4
    gq = IC.geometry(op, B, H, W, Cin, H * s, W * s, Cout, k, s)
    assert full - packed_ws == IC.slab_bytes(gq), ("slab bytes", op, B, H, W, Cin, Cout, k, s, full - packed_ws, IC.slab_bytes(gq))
    n = 1
    full = max(full, 16)
    if lib_family(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s, IC.EPI_NONE, full) != IC.FAMILY_IGEMM:
        return n
    packed4 = 4 * IC.packed_floats(g)
    assert packed4 <= packed_ws or op in (BD, TF)
    if op in (BD, TB):            # the fused update: at the full workspace, at the packed weights alone, and four bytes short of the slab in use
        need = IC.splitk_bytes(g)
        if not need:
            st = IC._state(g)
            tiles, tl, _, _ = IC._tiles_and_tail(st, 1 << 60)
            need = IC.tail_bytes(tl, tiles.wide) if tl.s > 1 else 0
        for nbytes in {full, packed4, packed4 + need - 4 if need else packed4}:
            if nbytes < packed4 or nbytes <= 0 or lib_family(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s, IC.EPI_NONE, nbytes) != IC.FAMILY_IGEMM:
                continue
            order = ctypes.c_int(-1)
            got = int(lib.cgs_conv_update_form(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, nbytes, ctypes.addressof(order)))
            want = IC.update_form(g, nbytes - packed4) if whole_batch(g) else 0
            assert got == want, ("update form", op, B, H, W, Cin, Ho, Wo, Cout, k, s, nbytes - packed4, got, want)
            assert not whole_batch(g) or order.value == IC.row_order(g), ("row order", op, B, H, W, Cin, Cout, k, s)
            n += 1
    if op in (F, TF):
        for e in (IC.EPI_LRELU, IC.EPI_AFFINE_RELU, IC.EPI_TANH):
            if lib_family(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s, e, full) != IC.FAMILY_IGEMM:
                continue
            got = int(lib.cgs_conv_signs_ok(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, e, full))
            assert got == int(IC.signs_ok(g, e) and whole_batch(g)), ("signs_ok", op, B, H, W, Cin, Cout, k, s, e)
            n += 1
    if op == F:
        got = int(lib.cgs_conv_stat_partials(B, H, W, Cin, Cout, k, k, s, s, full))
        assert got == (IC.stat_rows(g) if whole_batch(g) else 0), ("stat_partials", B, H, W, Cin, Cout, k, s)
        n += 1
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    got = int(lib.cgs_conv_stat_layout(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, B, full, ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c)))
    want = IC.stat_rows(g) if whole_batch(g) else 0
    assert got == want and (not want or (a.value, b.value, c.value) == (want, 1, 0)), ("stat_layout", op, B, H, W, Cin, Cout, k, s, got, want)
    return n + 1


FORM_CODES = {"plain": 0, "stats": 1, "nstats": 2, "signs": 3, "update": 4}          # CGS_FORM_* of include/cgs_hip.h
# the forms the entry points of an op offer, each with the epilogue they pass (the signs entry point: the forward's own relu / lrelu)
OP_FORMS = {F: (("plain", IC.EPI_NONE), ("stats", IC.EPI_NONE)), TF: (("plain", IC.EPI_NONE), ("stats", IC.EPI_NONE), ("signs", IC.EPI_LRELU)),
            BD: (("plain", IC.EPI_NONE), ("nstats", IC.EPI_NONE), ("update", IC.EPI_NONE)),
            TB: (("plain", IC.EPI_NONE), ("nstats", IC.EPI_NONE), ("update", IC.EPI_NONE))}


def sweep_workspaces(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s):
    """The workspaces the sweep asks about: full, the packed weights alone, four bytes short of the slab the plain call would use."""
    g = IC.geometry(op, B, H, W, Cin, Ho, Wo, Cout, k, s)
    full = max(int(lib.cgs_conv_ws_bytes_for(op, B, H, W, Cin, Cout, k, k, s, s)), 16)
    packed4 = 4 * IC.packed_floats(g)
    need = IC.splitk_bytes(g)
    if not need:
        tiles, tl, _, _ = IC._tiles_and_tail(IC._state(g), 1 << 60)
        need = IC.tail_bytes(tl, tiles.wide) if tl.s > 1 else 0
    return sorted({full, packed4, packed4 + need - 4 if need else packed4})


def check_plan(call, form, epilogue, nbytes):
    """cgs_conv_igemm_plan, the whole plan before the launch, field by field against the restated planner.  -> comparisons made."""
    from cgs_amd import lib as L
    op, B, H, W, Cin, Ho, Wo, Cout, k, s = call
    got = L.conv_igemm_plan(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, epilogue, FORM_CODES[form], nbytes)
    g = IC.geometry(op, B, H, W, Cin, Ho, Wo, Cout, k, s)
    packed4 = 4 * IC.packed_floats(g)
    what = (call, form, epilogue, nbytes)
    if nbytes < packed4 or nbytes <= 0 or not whole_batch(g) or lib_family(L.load(), op, B, H, W, Cin, Ho, Wo, Cout, k, s, epilogue, nbytes) != IC.FAMILY_IGEMM:
        assert got is None, what
        return 1
    p = IC.plan(g, nbytes - packed4, form, epilogue)
    assert (got is None) == p.refused, ("refused", what, got, p.refused)
    if got is None:
        return 1
    want = {"kernel": p.kernel, "reduce": p.reduce, "tail": (p.tail_n, p.tail_s if p.tail_s > 1 else 0),
            "plan": (p.xcd_map, p.cls_flip, p.uni, p.gx, p.splitk), "prio_t": tuple(p.prio_t), "row_order": p.row_order, "flops": float(p.flops),
            "perm": None if p.perm is None else [list(q) for q in p.perm] + [[]] * (4 - len(p.perm))}
    assert p.flops < 2 ** 53
    for field in want:
        assert got[field] == want[field], (field, what, got[field], want[field])
    return len(want) + 1


def call_of(case):
    Ho, Wo = IC.out_hw(case)
    if case.op in (F, BD):
        Ho = Wo = 0
    return (case.op, case.B, case.H, case.W, case.Cin, Ho, Wo, case.Cout, case.k, case.s)


def test_restatement_equals_the_library_on_the_table(lib):
    n = 0
    for case in IC.CASES:
        op, B, H, W, Cin, Ho, Wo, Cout, k, s = call_of(case)
        assert lib_family(lib, op, B, H, W, Cin, Ho, Wo, Cout, k, s, case.epilogue, IC.ws_bytes(lib, case)) == IC.FAMILY_IGEMM, IC.case_id(case)
        n += check_call(lib, *call_of(case))
        p = IC.case_plan(lib, case)
        assert not p.refused, (IC.case_id(case), "the entry point would refuse this form")
        # the whole plan, before any launch: at the row's own workspace (where the query must answer) and at the sweep's three
        from cgs_amd import lib as L
        assert L.conv_igemm_plan(op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, case.epilogue, FORM_CODES[case.form], IC.ws_bytes(lib, case)) is not None
        for nbytes in sorted({IC.ws_bytes(lib, case), *sweep_workspaces(lib, *call_of(case))}):
            n += check_plan(call_of(case), case.form, case.epilogue, nbytes)
    print(f"\nrestatement == library on {len(IC.CASES)} table rows, {n} comparisons")


def test_restatement_equals_the_library_on_a_sweep(lib):
    """B 1..4096, grids 1x1..32x32, channels on and off the 32 and 64 grids, k 1..5, s 1..2, odd transposed sizes 2H-1: a condition that is
    restated wrongly but does not bind on the table shows here."""
    rng = random.Random(20261021)
    Bs = [1, 2, 3, 4, 7, 8, 16, 32, 64, 100, 128, 130, 192, 256, 384, 512, 1000, 1024, 2048, 4096]
    Cs = [3, 20, 32, 64, 70, 96, 128, 160, 256, 512, 1024]
    calls = set()
    for case in IC.CASES:            # around the table: the same call at neighbouring batch sizes and grids
        for dB in (-1, 0, 1):
            for dH in (-1, 0, 1):
                c = case._replace(B=max(1, case.B + dB), H=max(1, case.H + dH))
                calls.add(call_of(c))
    while len(calls) < 4000:
        op, B, k, s = rng.choice((F, BD, TF, TB)), rng.choice(Bs), rng.randint(1, 5), rng.randint(1, 2)
        H, W = rng.randint(1, 32), rng.randint(1, 32)
        if rng.random() < 0.5:
            W = H
        Cin, Cout = rng.choice(Cs), rng.choice(Cs)
        if B * H * W * max(Cin, Cout) * 4 * (s * s if op in (TF, TB) else 1) > 0x7fffffff:
            continue
        Ho = Wo = 0
        if op in (TF, TB):
            odd = s == 2 and rng.random() < 0.3
            Ho, Wo = s * H - odd, s * W - odd
        calls.add((op, B, H, W, Cin, Ho, Wo, Cout, k, s))
    n = sum(check_call(lib, *c) for c in sorted(calls))
    # the whole plan of every call, in every form its op's entry points offer, at the three workspaces (a call that does not take the
    # implicit-GEMM family there must be answered with "no plan")
    planned = 0
    for c in sorted(calls):
        made = [check_plan(c, form, epilogue, nbytes) for nbytes in sweep_workspaces(lib, *c) for form, epilogue in OP_FORMS[c[0]]]
        n += sum(made)
        planned += max(made) > 1             # (a "no plan" answer is one comparison, a plan nine)
    assert planned > len(calls) // 2
    print(f"\nrestatement == library on a sweep of {len(calls)} calls ({planned} with a plan to compare), {n} comparisons")


def features(case, p):
    """The plan features a table row reaches, by name."""
    g = IC.case_geometry(case)
    f = {p.kernel, "row order %d" % p.row_order, "uni %d" % p.uni, "xcd_map %d" % p.xcd_map}
    f.add("split-K" if p.splitk > 1 else "no split-K")
    if p.lpt and p.perm_moved:
        f.add("a permutation that is not the identity")
    if p.binpacked:
        f.add("bin-packed permutation")
    if p.splitk > 1:
        f |= {"split-K %s" % ("one class" if p.nclasses == 1 else "four classes"), "reduce " + p.reduce,
              "split-K reduce epilogue " + IC.EPI_NAMES[case.epilogue]}
        if p.empty_slices:
            f.add("split-K class with empty slices")
        if p.n_mod4:
            f.add("split-K N % 4 != 0")
        if p.half:
            f.add("half")
    if p.tail_s > 1:
        f |= {"tail bn %d" % p.BN, "tail xcd_map %d" % p.xcd_map, "tail %s" % ("one class" if p.nclasses == 1 else "four equal classes"),
              "reduce " + p.reduce}
        if case.epilogue >= IC.EPI_RELU_BWD_AFFINE:
            f.add("tail aux epilogue")
        if case.epilogue == IC.EPI_AFFINE_RELU:
            f.add("tail affine epilogue")
        if p.tail_clip:
            f.add("tail S clipped by " + p.tail_clip)
    if p.wide_for_tail:
        f.add("wide_for_tail " + p.wide_for_tail)
    if p.padded_ids:
        f.add("padded ids")
    if p.tail_pad_refused:
        f.add("tail refused for padded ids")
    if case.form in ("stats", "nstats") and p.splitk == 1:
        f.add("one-pass " + p.kernel)
    f.add("cls_flip 0" if not p.cls_flip else "cls_flip nclasses (split-K)" if p.splitk > 1 else "cls_flip per_round < nclasses")
    if p.mid:
        f.add("mid rule %d" % p.mid)
    if p.deep_flipped:
        f.add("deep flipped by tot_blocks >= 1024")
    if p.prio_t[0]:
        f.add("prio_t")
    if p.tall:
        f.add("tall")
    if not p.vec:
        if g.Cred % 32 and any(c.K % 16 for c in g.cls):
            f.add("non-VEC Cred % 32 != 0 with K % 16 != 0")
        if any(c.K == 0 for c in g.cls):
            f.add("non-VEC class with zero taps")
    if g.N % 64:
        f.add("N off the 64 grid")
    if len({(c.R, c.C) for c in g.cls}) > 1:
        f.add("classes of unequal RxC")
    if g.Hout * g.Wout == 1:
        f.add("1x1 spatial")
    if g.B == 1:
        f.add("B = 1")
    if p.ragged:
        f.add("ragged last m-tile, row order %d" % p.row_order)
    return f


VEC8 = ["%s<128, %d, 4, true, %d, %s>" % ("%s", bn, tbk, par) for bn in (128, 64) for tbk in (32, 16) for par in ("false", "true")]
REQUIRED = [n % "igemm_kernel" for n in VEC8] + [n % "igemm_up_kernel" for n in VEC8] + [
    "igemm_kernel<64, 128, 4, true, 32, false>", "igemm_kernel<256, 64, 4, true, 16, false>", "igemm_kernel<256, 64, 4, true, 16, true>",
    "igemm_kernel<128, 128, 4, false, 16, false>", "igemm_kernel<128, 64, 4, false, 16, false>",
    "row order 0", "row order 1", "row order 2", "bin-packed permutation", "a permutation that is not the identity",
    "split-K one class", "split-K four classes", "split-K class with empty slices", "reduce splitk_reduce_kernel<false>",
    "reduce splitk_reduce_kernel<true>", "reduce splitk_reduce_stats_kernel", "split-K N % 4 != 0", "half",
] + ["split-K reduce epilogue " + IC.EPI_NAMES[e] for e in range(7)] + [
    "tail bn 128", "tail bn 64", "tail xcd_map 1", "tail xcd_map 0", "tail one class", "tail four equal classes", "tail aux epilogue",
    "tail affine epilogue", "reduce tail_reduce_kernel<true>", "reduce tail_reduce_kernel<false>", "wide_for_tail taken", "wide_for_tail refused",
    "tail S clipped by nk/4", "tail S clipped by 16", "padded ids", "cls_flip 0", "cls_flip nclasses (split-K)", "cls_flip per_round < nclasses",
    "uni 0", "uni 1", "mid rule 1", "mid rule 2", "deep flipped by tot_blocks >= 1024", "prio_t", "tall",
    "non-VEC Cred % 32 != 0 with K % 16 != 0", "N off the 64 grid", "non-VEC class with zero taps", "classes of unequal RxC", "1x1 spatial", "B = 1",
    "ragged last m-tile, row order 0", "ragged last m-tile, row order 1", "tail refused for padded ids",
]
# every igemm_ns_kernel the nstats entry points can reach: the twin of each of the 13 tiles
REQUIRED += [n % "igemm_ns_kernel" for n in VEC8] + [n.replace("igemm_kernel", "igemm_ns_kernel") for n in REQUIRED if n.startswith("igemm_kernel<") and
                                                      n not in [v % "igemm_kernel" for v in VEC8]]
# ... and, not split over K, the epilogues that tell the twins apart (a split block leaves raw slabs and returns before any epilogue): the
# one-pass statistics of igemm_kernel and the norm-backward sums of every 32-deep igemm_ns_kernel that can launch unsplit.  (The 64 x 128
# tile launches split only; igemm_ns_kernel<128, 128, 4, true, 32, true> has one class, so unsplit it has either < 256 wide blocks -- the
# statistics rule then narrows it to 128 x 64 -- or >= 512, which is 16-deep.)
REQUIRED += ["one-pass igemm_kernel<128, 64, 4, true, 32, false>", "one-pass igemm_ns_kernel<128, 128, 4, true, 32, false>",
             "one-pass igemm_ns_kernel<128, 64, 4, true, 32, false>", "one-pass igemm_ns_kernel<128, 64, 4, true, 32, true>"]


def test_the_table_reaches_every_plan_feature(lib):
    reached = {}
    for case in IC.CASES:
        for f in features(case, IC.case_plan(lib, case)):
            reached.setdefault(f, []).append(IC.case_id(case))
    print()
    for f in sorted(reached):
        print(f"{f:60s} {len(reached[f]):3d} rows, first {reached[f][0]}")
    ns = sorted(f for f in reached if f.startswith("igemm_ns_kernel"))
    print("igemm_ns_kernel instantiations reached:", ns)
    missing = [f for f in REQUIRED if f not in reached]
    assert not missing, missing
    assert len(ns) == 13, ns


def test_rows_without_a_slab_plan_differently_from_their_twins(lib):
    """A "none" row is there for the plan a call takes when the workspace holds the packed weights only: it has no slab at all, and its
    plan is not the plan of the same call at the full workspace."""
    n = 0
    for case in IC.CASES:
        if case.slab != "none":
            continue
        g = IC.case_geometry(case)
        assert IC.ws_bytes(lib, case) - 4 * IC.packed_floats(g) == 0 or IC.packed_floats(g) < 4
        p, twin = IC.case_plan(lib, case), IC.case_plan(lib, case._replace(slab="full"))
        assert (p.kernel, p.reduce, p.splitk, p.tail_s) != (twin.kernel, twin.reduce, twin.splitk, twin.tail_s), IC.case_id(case)
        assert p.splitk == 1 and p.tail_s <= 1, IC.case_id(case)
        n += 1
    assert n >= 6


def test_every_row_is_there_for_a_reason_and_inside_the_budget(lib):
    assert len({IC.case_id(c) for c in IC.CASES}) == len(IC.CASES)
    for case in IC.CASES:
        assert case.why and case.slab in ("full", "none") and case.form in IC.FORMS
        assert IC.macs(case) <= IC.MAC_BUDGET, (IC.case_id(case), IC.macs(case))


def test_executed_flops_by_brute_force(lib):
    for case in IC.CASES:
        g, p = IC.case_geometry(case), IC.case_plan(lib, case)
        assert p.flops == IC.brute_flops(g, p.row_order > 0, p.BM if p.tall else 128) and p.flops < 2 ** 53, IC.case_id(case)


def test_oracle_side_of_the_bar():
    """The float32 torch-CPU oracle against the float64 reference, normalised as the GPU test normalises; and no sign-deciding value
    within AUX_MARGIN of zero."""
    worst, worst_of_bar, at = 0.0, 0.0, None
    print()
    for case in IC.CASES:
        inp, lin = IC.inputs_and_reference(case)
        v = IC.sign_deciding(case, inp, lin)
        assert v is None or float(v.abs().min()) >= IC.AUX_MARGIN, IC.case_id(case)
        want = IC.expected64(case, inp, lin)
        ref = want["theta"] if case.form == "update" else want["out"]
        got = IC.oracle32(case, inp)
        fig = float((got.double() - ref).abs().max() / ref.abs().max())
        print(f"oracle {IC.case_id(case)}: max|delta|/max|ref| = {fig:.3e} = {fig / IC.bar(case):.3f} of the bar")
        if fig / IC.bar(case) > worst_of_bar:
            worst_of_bar, at = fig / IC.bar(case), IC.case_id(case)
        worst = max(worst, fig)
    print(f"worst {worst:.3e}, {worst_of_bar:.3f} of the bar at {at}")
    assert worst <= IC.ORACLE_WORST and worst_of_bar <= IC.ORACLE_OF_BAR < 1.0
