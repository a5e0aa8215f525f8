#!/usr/bin/env python3
"""Answers of the six host-only planning queries of libcgs_hip.so (cgs_conv_ws_bytes, cgs_conv_ws_bytes_for, cgs_conv_family,
cgs_conv_stat_partials, cgs_conv_stat_layout, cgs_conv_signs_ok) over a fixed seeded case list, in each of the three contraction
modes -- the equivalence check for a change to the dispatcher (csrc/api.hip) that must not move a planning answer:

    CGS_LIB=<old build>/libcgs_hip.so python tools/plan_sweep.py dump old.txt
    CGS_LIB=<new build>/libcgs_hip.so python tools/plan_sweep.py dump new.txt
    python tools/plan_sweep.py diff old.txt new.txt          # exit status 1 and the first differing cases if they differ

No GPU is needed: with no device visible the planners take their "round rules apply" branch, which is what they do on an MI355X.
The case list: (a) every conv / deconv / linear layer of every architecture of nets.py at the batch sizes of the README, for the four
ops and every epilogue code, with workspaces of 0, cgs_conv_ws_bytes, cgs_conv_ws_bytes_for bytes and one byte less than each;
(b) a seeded random part (--random N geometries, six queries each): kernel 1-7, stride 1-3, odd and even sizes, channel counts on and
off the multiples of 4 / 16 / 32 / 64, statistics groups that do and do not divide B, deconv output sizes consistent and inconsistent
with 'SAME'; (c) non-positive and out-of-range arguments.  Every int product the library forms stays below 2^31.
`dump` prints the coverage of the list (families met per mode, share of non-zero answers per query) and fails if it is too thin."""
import argparse
import ctypes as C
import importlib.util
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "collaborative-gan-sampling_amd")
MODES = ("f32", "bx6", "bx6_all")
FAMILIES = ("IGEMM", "QUAD", "SMALLN_T", "SMALLN_F", "PATCH", "TAPS", "DOT", "IGEMM_BX6")
CONV_FWD, CONV_BWD_DATA, DECONV_FWD, DECONV_BWD_DATA = range(4)
OPS = (CONV_FWD, CONV_BWD_DATA, DECONV_FWD, DECONV_BWD_DATA)
EPILOGUES = range(7)
BATCHES = (8, 64, 256, 1024, 2048)         # the README's batch sizes and their fused multiples (8 x 256, 32 x 64, 2 x 1024)


def load_lib():
    lib = C.CDLL(os.environ.get("CGS_LIB") or os.path.join(PKG, "libcgs_hip.so"))
    i, z, p = C.c_int, C.c_size_t, C.POINTER(C.c_int)
    for name, res, args in (("cgs_conv_ws_bytes", z, [i] * 7), ("cgs_conv_ws_bytes_for", z, [i] * 10), ("cgs_conv_family", i, [i] * 13 + [z]),
                            ("cgs_conv_stat_partials", i, [i] * 9 + [z]), ("cgs_conv_stat_layout", i, [i] * 13 + [z, p, p, p]),
                            ("cgs_conv_signs_ok", i, [i] * 13 + [z]), ("cgs_set_contraction", i, [i])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def same(size, stride):
    return -(-size // stride)


def arch_layers():
    """(H, W, Cin, Ho, Wo, Cout, k, s, is_deconv) of every conv / deconv / linear layer of every architecture (a linear layer is a
    1x1 convolution over a 1x1 image)."""
    spec = importlib.util.spec_from_file_location("cgs_nets", os.path.join(PKG, "nets.py"))
    nets = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nets)
    out = []

    def walk(layers, shape, A):
        for L in layers:
            if L[0] == "linear":
                n = 1
                for d in shape:
                    n *= d
                out.append((1, 1, n, 1, 1, L[2], 1, 1, False))
                shape = (L[2],)
            elif L[0] == "reshape":
                shape = tuple(L[1])
            elif L[0] == "flatten":
                n = 1
                for d in shape:
                    n *= d
                shape = (n,)
            elif L[0] == "conv":
                k, s = nets.layer_ks(L, A["k"], A["stride"])
                ho, wo = same(shape[0], s), same(shape[1], s)
                out.append((shape[0], shape[1], shape[2], ho, wo, L[2], k, s, False))
                shape = (ho, wo, L[2])
            elif L[0] == "deconv":
                k, s = nets.layer_ks(L, A["k"], A["stride"])
                out.append((shape[0], shape[1], shape[2], L[2][0], L[2][1], L[2][2], k, s, True))
                shape = tuple(L[2])
            elif L[0] == "res":
                walk(L[1], shape, A)
        return shape

    for name in sorted(nets.ARCHS):
        A = nets.ARCHS[name]
        img = walk(A["g_tail"], walk(A["g_head"], nets.g_input_shape(A), A), A)
        walk(A["d"], img, A)
    return sorted(set(out))


def cases(n_random, seed=2019):
    """Yield (op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, group_images, ws_kind, in_range); H, W, Cin describe the op's
    input (for the backward-data ops: the tensor the gradient is taken w.r.t.), as at the entry points.  ws_kind: 0 = no workspace,
    1 / 2 = cgs_conv_ws_bytes / cgs_conv_ws_bytes_for bytes, 3 / 4 = one byte less than those."""
    for (H, W, Cin, Ho, Wo, Cout, k, s, deconv) in arch_layers():                                    # (a)
        for B in BATCHES:
            if B * max(H * W * Cin, Ho * Wo * Cout) >= 1 << 31:
                continue
            for op in ((DECONV_FWD, DECONV_BWD_DATA) if deconv else (CONV_FWD, CONV_BWD_DATA)):
                for epi in EPILOGUES:
                    for ws_kind in range(5):
                        for group in sorted({B, max(B // 8, 1)}):
                            yield (op, B, H, W, Cin, Ho, Wo, Cout, k, k, s, s, epi, group, ws_kind, True)
    rnd = random.Random(seed)                                                                       # (b)
    chans = [1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 32, 48, 64, 96, 100, 128, 192, 256, 320, 384, 512]
    for _ in range(n_random):
        op = rnd.choice(OPS)
        kh = rnd.randint(1, 7)
        kw = kh if rnd.random() < 0.7 else rnd.randint(1, 7)
        sh = rnd.choice((1, 2, 2, 2, 3)) if op in (CONV_FWD, DECONV_BWD_DATA) else rnd.choice((1, 2, 2, 2, 2, 2, 2, 3))
        sw = sh if rnd.random() < 0.85 else rnd.randint(1, 3)
        H = rnd.choice((1, 2, 3, 4, 5, 7, 8, 9, 14, 16, 17, 28, 32, 33, 64))
        W = H if rnd.random() < 0.7 else rnd.choice((1, 2, 3, 4, 5, 7, 8, 9, 14, 16, 17, 28, 32, 33, 64))
        Cin, Cout = rnd.choice(chans), rnd.choice(chans)
        if rnd.random() < 0.5:                      # (the MFMA families want both channel counts on the multiples of 32 / 64)
            Cin, Cout = rnd.choice((32, 64, 128, 256, 512)), rnd.choice((64, 128, 256, 512))
        B = rnd.choice((1, 2, 3, 8, 16, 24, 64, 100, 128, 256, 384, 512, 1024, 2048, 4096))
        if op in (CONV_FWD, CONV_BWD_DATA):
            Ho, Wo = same(H, sh), same(W, sw)
        else:                                        # deconv: the output a 'SAME' conv of that stride maps back to H x W -- or not
            Ho, Wo = H * sh - rnd.randrange(sh), W * sw - rnd.randrange(sw)
            if rnd.random() < 0.15:
                Ho, Wo = Ho + rnd.choice((-sh, 1, sh, 2 * sh)), Wo + rnd.choice((-1, 0, sw))
                Ho, Wo = max(Ho, 1), max(Wo, 1)
        if max(H * W * Cin, Ho * Wo * Cout, H * sh * W * sw * Cout) >= 1 << 29:
            continue
        divisors = [g for g in (1, 2, 4, 8, 16, 32, 64, 128, 256) if B % g == 0]
        group = B if rnd.random() < 0.4 else rnd.choice(divisors) if rnd.random() < 0.8 else rnd.choice((3, 5, 7, 48, 96))
        epi = rnd.choice((0, 0, 1, 1, 1, 2, 2, 3, 4, 5, 5, 6))
        yield (op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epi, group, rnd.choice((0, 1, 2, 2, 2, 2, 3, 4)), True)
    base = (CONV_FWD, 64, 16, 16, 64, 8, 8, 128, 4, 4, 2, 2, 1, 64, 2)                              # (c)
    for pos in range(14):
        for bad in (0, -1, -7) + ((4, 7, 99) if pos in (0, 12) else (1 << 12,) if pos in (8, 9) else (3, 5) if pos in (10, 11, 13) else ()):
            for op in OPS:
                c = list(base)
                c[0] = op
                if op >= DECONV_FWD:
                    c[2], c[3], c[4], c[5], c[6], c[7] = 8, 8, 128, 16, 16, 64
                c[pos] = bad
                for ws_kind in (0, 2):
                    yield tuple(c[:14]) + (ws_kind, False)


def answers(lib, case):
    op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epi, group, ws_kind, _ = case
    packed = lib.cgs_conv_ws_bytes(op, kh, kw, sh, sw, Cin, Cout)
    full = lib.cgs_conv_ws_bytes_for(op, B, H, W, Cin, Cout, kh, kw, sh, sw)
    ws = (0, packed, full, max(packed - 1, 0), max(full - 1, 0))[ws_kind]
    r, n, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    fam = lib.cgs_conv_family(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epi, ws)
    part = lib.cgs_conv_stat_partials(B, H, W, Cin, Cout, kh, kw, sh, sw, ws)
    rows = lib.cgs_conv_stat_layout(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, group, ws, C.byref(r), C.byref(n), C.byref(s))
    signs = lib.cgs_conv_signs_ok(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epi, ws)
    return (packed, full, fam, part, rows, r.value, n.value, s.value, signs)


def dump(path, n_random):
    lib = load_lib()
    met = {m: set() for m in MODES}
    nonzero, in_range, total = [0, 0, 0, 0], 0, 0
    with open(path, "w") as f:
        for mode, name in enumerate(MODES):
            assert lib.cgs_set_contraction(mode) == 0
            for case in cases(n_random):
                a = answers(lib, case)
                f.write(f"{name} {' '.join(map(str, case[:15]))} -> {' '.join(map(str, a))}\n")
                total += 6
                if a[2] >= 0:
                    met[name].add(a[2])
                if case[15]:
                    in_range += 1
                    for j, v in enumerate((a[3], a[4], a[8], a[1] - a[0])):
                        nonzero[j] += v != 0
    print(f"{total} answers ({total // 18} cases x 6 queries x 3 contraction modes) -> {path}")
    ok = True
    for name in MODES:
        want = set(range(8)) - ({7} if name == "f32" else set())
        print(f"  {name}: families met: {', '.join(FAMILIES[i] for i in sorted(met[name]))}")
        ok = ok and met[name] == want
    for j, q in enumerate(("stat_partials", "stat_layout", "signs_ok", "ws_bytes_for slab part")):
        print(f"  {q}: non-zero in {100.0 * nonzero[j] / in_range:.1f} % of the {in_range} in-range cases (all modes)")
        ok = ok and nonzero[j] * 10 >= in_range
    if not ok:
        sys.exit("the case list is too thin: a reachable family is missing or a query answers non-zero in under a tenth of the in-range cases")


def diff(a, b):
    n = bad = 0
    with open(a) as fa, open(b) as fb:
        for la, lb in zip(fa, fb):
            n += 1
            if la != lb:
                bad += 1
                if bad <= 20:
                    print(f"- {la}+ {lb}", end="")
        if fa.readline() or fb.readline():
            sys.exit("the files hold different case lists")
    print(f"{n} lines (one per case and contraction mode) compared, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--random", type=int, default=60000, help="random geometries (each asked of the six queries in three modes)")
    x = sub.add_parser("diff")
    x.add_argument("a")
    x.add_argument("b")
    args = ap.parse_args()
    dump(args.out, args.random) if args.cmd == "dump" else diff(args.a, args.b)
