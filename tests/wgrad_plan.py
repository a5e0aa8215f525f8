"""The weight-gradient launch plan (csrc/wgrad.hip, ``wgrad_geom``) restated in plain Python integers, shared by the CPU planner
properties (test_properties_cpu.py) and the device tests (test_gpu_train_kernels.py).  Not a test module and not a conftest: the
tests import it by name.  The restatement is checked against the library through ``cgs_conv_wgrad_ws_bytes`` wherever it is used."""
import collections

WT = 128        # tile rows (kh*kw*Cin) and columns (Cout) of one block
WK = 32         # pixels per reduction step
SPLIT_CAP = 256

Plan = collections.namedtuple("Plan", "M Kc Csp Ho Wo pt pl tiles splits m_per_split")


def ceil_div(a, b):
    return -(-a // b)


def same_pad_before(size, k, s):
    """TF 'SAME': the smaller half of the total padding goes in front."""
    tot = max((ceil_div(size, s) - 1) * s + k - size, 0)
    return tot // 2


def wgrad_plan(B, H, W, Cin, Cout, kh, kw, sh, sw):
    Ho, Wo = ceil_div(H, sh), ceil_div(W, sw)
    M = B * Ho * Wo
    Kc = kh * kw * Cin
    tiles = ceil_div(Kc, WT) * ceil_div(Cout, WT)
    splits = ceil_div(1024, tiles)                       # two rounds of blocks over 512 slots
    splits = min(splits, ceil_div(M, 4 * WK), SPLIT_CAP)  # at least four steps per block, at most 256 slabs
    splits = max(splits, 1)
    mps = ceil_div(ceil_div(M, splits), WK) * WK         # whole 32-pixel steps
    return Plan(M, Kc, ceil_div(Cout, 4) * 4, Ho, Wo, same_pad_before(H, kh, sh), same_pad_before(W, kw, sw), tiles,
                ceil_div(M, mps), mps)


def lib_ws_bytes(lib, B, H, W, Cin, Cout, kh, kw, sh, sw):
    return int(lib.cgs_conv_wgrad_ws_bytes(B, H, W, Cin, Cout, kh, kw, sh, sw))


def lib_splits(lib, B, H, W, Cin, Cout, kh, kw, sh, sw):
    """The library's own split count: its workspace is ``splits`` slabs of ``Kc * round_up(Cout, 4)`` floats."""
    nbytes = lib_ws_bytes(lib, B, H, W, Cin, Cout, kh, kw, sh, sw)
    slab = 4 * kh * kw * Cin * ceil_div(Cout, 4) * 4
    assert nbytes > 0 and nbytes % slab == 0, (nbytes, slab)
    return nbytes // slab
