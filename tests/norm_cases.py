"""Float64 definitions, seeded inputs and the case tables of the norm (+ lrelu) kernels (csrc/bn.hip), shared by the CPU checks
(test_norm_cases_cpu.py) and the device tests (test_gpu_norm_paths.py).  Not a test module and not a conftest: the tests import it
by name.  Everything here runs on the CPU; nothing imports the library.

The definitions (x is [groups, M, C] float32, statistics are per (group, channel)):
  forward    mean, biased var, invstd = 1/sqrt(var + eps), y = lrelu(gamma * (x - mean) * invstd + beta)
  backward   u = gamma * (x - mean) * invstd + beta, d = dy * (u > 0 ? 1 : leak), xhat = (x - mean) * invstd,
             dx = gamma * invstd * (d - m1 - xhat * m2), m1 = mean(d), m2 = mean(d * xhat); mean / invstd are the float32
             tensors the kernel is handed
  from partial rows   the statistics are BY DEFINITION those of the rows the layout assigns to the group, added in float64:
             forward mean = sum(a) / M, var = max(0, sum(b) / M - mean^2); backward m1 = sum(a) / M, m2 = sum(b) / M.
             They need not be the statistics of x, so a test may hand in rows that are not sums of x: that pins the addressing.
"""
import collections
import functools

import torch

EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # the kernels take eps as a float: the reference uses that very value
KINK = 1e-4      # no backward input has |u| below this: a float32 u of O(1) operands is off by ~1e-6, so kernel and reference agree on u > 0
CONST = 0.5      # value of the constant channel: its float32 sums are exact, var == 0, invstd == 1/sqrt(eps), y == lrelu(beta)
BETA_MIN = 1e-3  # |beta| of every channel (the constant channel's u IS beta; so is every channel's at M = 1)


def lrelu(u, leak):
    return torch.where(u > 0, u, leak * u)


# ----------------------------------------------------------------------------- float64 definitions
def stats_from_x(x):
    """x [groups, M, C] -> float64 (mean, var, invstd), each [groups, C]."""
    xd = x.double()
    mean = xd.mean(1)
    var = ((xd - mean[:, None]) ** 2).mean(1)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def ref_fwd(x, gamma, beta, mean, invstd, leak):
    g, b = gamma.double(), beta.double()
    return lrelu(g * (x.double() - mean.double()[:, None]) * invstd.double()[:, None] + b, leak)


def ref_u(x, gamma, beta, mean, invstd):
    return gamma.double() * (x.double() - mean.double()[:, None]) * invstd.double()[:, None] + beta.double()


def ref_bwd(dy, x, gamma, beta, mean, invstd, leak, m1=None, m2=None):
    """dx in float64; m1 / m2 [groups, C] given (from partial rows) or, by default, the means over the group's rows."""
    mu, inv = mean.double()[:, None], invstd.double()[:, None]
    u = ref_u(x, gamma, beta, mean, invstd)
    d = torch.where(u > 0, dy.double(), float(leak) * dy.double())
    xhat = (x.double() - mu) * inv
    m1 = d.mean(1) if m1 is None else m1.double()
    m2 = (d * xhat).mean(1) if m2 is None else m2.double()
    return gamma.double() * inv * (d - m1[:, None] - xhat * m2[:, None])


# ----------------------------------------------------------------------------- inputs from x
Inputs = collections.namedtuple("Inputs", "x dy gamma beta mean invstd const_c")


def kink_count(inp):
    """Elements whose u lies within KINK of lrelu's kink, with the float32 mean / invstd of ``inp``."""
    return int((ref_u(inp.x, inp.gamma, inp.beta, inp.mean, inp.invstd).abs() < KINK).sum())


@functools.lru_cache(maxsize=4)
def _build(groups, M, C, seed):
    g = torch.Generator().manual_seed(1000 * seed + 7)
    x = (torch.randn((groups, M, C), generator=g) * 1.5 + 0.3).float()
    dy = torch.randn((groups, M, C), generator=g).float()
    gamma = (torch.randn(C, generator=g) * 0.1 + 1.0).float()
    beta = (torch.randn(C, generator=g) * 0.1).float()
    beta = torch.where(beta < 0, -1.0, 1.0) * beta.abs().clamp_min(BETA_MIN)
    const_c = (5 * seed + 3) % C
    x[:, :, const_c] = CONST
    for _ in range(50):
        mean, var, invstd = stats_from_x(x)
        mean32, invstd32 = mean.float(), invstd.float()
        u = ref_u(x, gamma, beta, mean32, invstd32)
        bad = u.abs() < KINK
        if not bad.any():
            break
        away = torch.where(u < 0, -1.0, 1.0) * torch.sign(gamma.double())          # the direction in x that grows |u|
        x = torch.where(bad, x.double() + away * 0.01 * torch.sqrt(var)[:, None], x.double()).float()
    inp = Inputs(x, dy, gamma, beta, mean32, invstd32, const_c)
    n = kink_count(inp)
    assert n == 0, f"{n} elements within {KINK} of the kink after the repair ({groups} x {M} x {C})"       # a condition, not a measurement
    assert bool((x[:, :, const_c] == CONST).all())
    return inp


def build_inputs(groups, M_group, C, leak=0.2, seed=0):
    """Seeded inputs of one case: x ~ N(0.3, 1.5^2) with one channel constant at CONST, dy ~ N(0, 1), gamma ~ 1 +- 0.1,
    beta ~ +-0.1 (|beta| >= BETA_MIN), and mean / invstd = the float64 statistics of x rounded to float32 (what the backward kernels
    are handed).  x is repaired until no element has |u| < KINK; the builder asserts that.  The kink does not move with ``leak``:
    one set of inputs serves every leak of a shape."""
    del leak
    return _build(int(groups), int(M_group), int(C), int(seed))


# ----------------------------------------------------------------------------- synthetic partial rows
Partials = collections.namedtuple("Partials", "part layout owner groups M")      # layout = (rows_total, rows_per_seg, nseg, seg_stride)


def owned_rows(groups, rows_per_seg, nseg, seg_stride):
    """[groups][nseg * rows_per_seg] row indices: group g owns, in every segment sg, the rows sg * seg_stride + g * rows_per_seg + i."""
    return [[sg * seg_stride + g * rows_per_seg + i for sg in range(nseg) for i in range(rows_per_seg)] for g in range(groups)]


def build_partials(groups, rows_per_seg, nseg, seg_stride, C, M_group=136, seed=0):
    """A [rows_total, 2, C] float32 buffer of partial rows.  Every row a group owns holds distinct random values, every row no
    group owns is NaN.  Per (group, channel) the a-rows add up to M * mu with 0.1 <= |mu| <= 1 and the b-rows to M * (mu^2 + v) with
    0.5 <= v <= 2.5: read as forward sums var = v >= 0.1 * E[x^2]; all terms of a sum share one sign, so the float64 sum of the
    float32 rows has no cancellation of its own."""
    if nseg == 1 and seg_stride == 0:
        seg_stride = groups * rows_per_seg
    assert seg_stride >= groups * rows_per_seg
    rows_total = nseg * seg_stride
    g = torch.Generator().manual_seed(1000 * seed + 13)
    n = nseg * rows_per_seg
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)
    mu = (0.1 + 0.9 * rnd(groups, 1, C)) * torch.where(rnd(groups, 1, C) < 0.5, -1.0, 1.0)
    e2 = mu * mu + 0.5 + 2.0 * rnd(groups, 1, C)
    wa, wb = 0.5 + rnd(groups, n, C), 0.5 + rnd(groups, n, C)
    a = M_group * mu * wa / wa.sum(1, keepdim=True)
    b = M_group * e2 * wb / wb.sum(1, keepdim=True)
    part = torch.full((rows_total, 2, C), float("nan"), dtype=torch.float32)
    owner = torch.full((rows_total,), -1, dtype=torch.int64)
    for gi, rows in enumerate(owned_rows(groups, rows_per_seg, nseg, seg_stride)):
        idx = torch.tensor(rows)
        assert bool((owner[idx] == -1).all())
        owner[idx] = gi
        part[idx, 0] = a[gi].float()
        part[idx, 1] = b[gi].float()
    return Partials(part, (rows_total, rows_per_seg, nseg, seg_stride), owner, groups, M_group)


def partial_sums(p):
    """float64 (sum(a) / M, sum(b) / M), each [groups, C], over the rows the layout assigns to each group."""
    _, rows_per_seg, nseg, seg_stride = p.layout
    rows = owned_rows(p.groups, rows_per_seg, nseg, seg_stride)
    a = torch.stack([p.part[torch.tensor(r), 0].double().sum(0) for r in rows]) / p.M
    b = torch.stack([p.part[torch.tensor(r), 1].double().sum(0) for r in rows]) / p.M
    return a, b


def stats_from_partials(p):
    """float64 (mean, invstd) of the forward from partial rows."""
    m, e2 = partial_sums(p)
    var = (e2 - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + EPS)


# ----------------------------------------------------------------------------- the case tables of test_gpu_norm_paths.py
# From x.  (kind, groups, M_group, C, path, leaks): kind "bn" = cgs_bn_train_lrelu_* (groups == 1), "in" = cgs_instnorm_lrelu_* (groups = B).
LK = (0.2, 1.0)
LK0 = (0.2, 1.0, 0.0)      # one case per path also runs relu
RELOAD_M = 43691           # smallest M with 3 * M * 16 > 8192 * 256 float4; M * 16 = 699056 is no multiple of 8192 * 256
FROM_X = (
    [("bn", 1, M, C, "norm_small", LK0 if (M, C) == (17, 40) else LK) for M in (1, 16, 17, 128) for C in (4, 40, 64, 68)] + [
        ("in", 3, 128, 40, "norm_small", LK),
        ("bn", 1, 129, 4, "norm_passes", LK),
        ("bn", 1, 129, 40, "norm_passes", LK0),         # C/4 = 10 threads a row: tpr = 8, a ragged second sweep
        ("bn", 1, 200, 1028, "norm_passes", LK),        # tpr = 256, second sweep of one float4
        ("bn", 1, 8193, 8, "norm_passes", LK),          # just past 16 * CGS_BN_MAX_BLOCKS rows: rows_per_block 17
        # generic apply branch across groups: n4 = 3 * 130 * 10 = 3900, ceil(n4 / 256) = 16 blocks, 16 % 5 != 0 so (stride * 4) % 40 != 0
        ("in", 3, 130, 40, "norm_passes", LK),
        ("in", 2049, 129, 4, "norm_passes", LK),        # B > 2048: in_geom's one stage-1 block per sample
        # fixed-channel apply branch re-loading its parameters: 8192 blocks, the threads 0..15 cross from group 0 into group 2
        ("in", 3, RELOAD_M, 64, "norm_passes", (0.2,)),
    ])
BWD_FROM_X = FROM_X        # every from-x case runs forward and backward

# From partials.  (groups, rows_per_seg, nseg, seg_stride, M_group, C, path, leaks); seg_stride 0 = rows packed (one segment).
MB2_ROWS = (2 << 20) // (8 * 4)       # rows of a [M, 8] tensor of exactly 2 MB
FROM_PARTIALS = [
    (1, 1, 1, 0, 136, 8, "norm_fa", LK),
    (1, 16, 1, 0, 136, 72, "norm_fa", LK0),
    (3, 2, 4, 7, 136, 8, "norm_fa", LK),                # a NaN gap row behind the three groups of every segment
    (3, 2, 4, 7, 136, 72, "norm_fa", LK),
    (1, 4, 1, 0, MB2_ROWS, 8, "norm_fa", LK),           # the size limit: exactly 2 MB ...
    (1, 4, 1, 0, MB2_ROWS + 1, 8, "norm_finalize", LK),  # ... and one row more
    (1025, 2, 1, 0, 40, 8, "norm_fa", LK),              # groups * ceil(C / 64) > 1024: one chunk of rows per group
    (1, 17, 1, 0, 136, 8, "norm_finalize", LK),
    (1, 1023, 1, 0, 136, 72, "norm_finalize", LK0),
    (3, 5, 4, 20, 136, 8, "norm_finalize", LK),         # 20 partial rows a group; NaN gap rows 15..19 of every segment
    (3, 5, 4, 20, 136, 72, "norm_finalize", LK),
    (1, 1024, 1, 0, 136, 8, "norm_sliced", LK),
    (1, 1025, 1, 0, 136, 72, "norm_sliced", LK0),
    (1, 1030, 1, 0, 136, 8, "norm_sliced", LK),
    (2, 1024, 1, 0, 136, 8, "norm_finalize", LK),       # 1024 rows, two groups: not sliced
    (1, 1024, 2, 1027, 136, 8, "norm_finalize", LK),    # 1024 rows a segment, two segments: not sliced
]
