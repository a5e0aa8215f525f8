"""The G step of the 2-D generator at 65..256 hidden units, host side: the two C ABI entries (csrc/mlp2d_wide_gstep.hip), their refusals
and the workspace size; the float64 restatement's BN backward at 256 x 6 against a hand-written numpy one.

It also holds what the GPU tests (test_gpu_synthetic_wide_gstep.py) share: the inputs of a case, the error measures, the float32-CPU
figures the bars are derived from, and the ReLU-kink condition on a case's inputs."""
import os
import re

import numpy as np
import pytest
import torch

import test_synthetic_train_cpu as R
from test_gpu_synthetic_train import perturbed_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cgs_mlp2d_wide_g_step_ws_bytes", "cgs_mlp2d_wide_g_step")


# ---- shared with the GPU tests ----------------------------------------------------------------------------------------------------
def case_inputs(seed, nh, nl, B, shift=0.0):
    """-> (P host arrays, z [B,2] float32, grad_plugin [B,2] float32 = 1e-3 randn) of a gradient case.  ``shift``: every beta becomes
    +shift at the even units and -shift at the odd ones, so that a unit is on for every sample or off for every sample"""
    P = perturbed_params(seed, nh, nl)
    if shift:
        for k in P:
            if k.endswith("/beta"):
                P[k] = (shift * (1 - 2 * (np.arange(nh) % 2))).astype(np.float32)
    rs = np.random.RandomState(seed + 7)
    return P, rs.randn(B, 2).astype(np.float32), (1e-3 * rs.randn(B, 2)).astype(np.float32)


def bn_outputs(P, z):
    """y = gamma xhat + beta of every BN layer of a training-mode forward (what the ReLU decides on), in the dtype of P; nothing moves"""
    n = R.nlayers_of(P, "generator/g_fc")
    h, ys = z, []
    for i in range(n - 1):
        a = h @ P[f"generator/g_fc{i + 1}/kernel"] + P[f"generator/g_fc{i + 1}/bias"]
        bn = R.bn_name(i)
        y = (a - a.mean(0)) / torch.sqrt(a.var(0, unbiased=False) + R.EPS) * P[f"{bn}/gamma"] + P[f"{bn}/beta"]
        ys.append(y)
        h = torch.relu(y)
    return ys


def kink_margin(P, z):
    """-> (min |y| of the float64 forward, m = 4 max |y_float32 - y_float64|): an entry with |y| < m can take the other ReLU branch in
    float32 arithmetic, and one flip moves a gradient by far more than rounding does"""
    y64 = bn_outputs(R.to_torch(P, torch.float64), torch.as_tensor(z, dtype=torch.float64))
    y32 = bn_outputs(R.to_torch(P, torch.float32), torch.as_tensor(z, dtype=torch.float32))
    m = 4 * max((a.double() - b).abs().max().item() for a, b in zip(y32, y64))
    return min(b.abs().min().item() for b in y64), m


def find_seed(nh, nl, B, shift=0.0, tries=2000):
    """the first seed whose float64 forward has no BN output closer to 0 than m"""
    for seed in range(tries):
        P, z, _ = case_inputs(seed, nh, nl, B, shift)
        lo, m = kink_margin(P, z)
        if lo >= m:
            return seed
    return None


def g_step_ref(P, z, gp, dtype, lr=0.0):
    """R.g_step on copies in `dtype` -> ({name: gradient}, {name: tensor after})"""
    Q = R.to_torch(P, dtype)
    g = R.g_step(Q, torch.as_tensor(z, dtype=dtype), torch.as_tensor(gp, dtype=dtype), lr)
    return g, Q


def grad_errs(got, ref, nl):
    """-> (worst kernel / last-bias error: max |dg| / max |g_ref| per tensor; worst BN-fed bias: max |gb| / max |dW of its layer|, the
    bias gradient being zero in exact arithmetic).  got / ref: {name: tensor}"""
    ek = eb = 0.0
    for i in range(nl):
        kw, kb = f"generator/g_fc{i + 1}/kernel", f"generator/g_fc{i + 1}/bias"
        rw = ref[kw].double()
        ek = max(ek, ((got[kw].double() - rw).abs().max() / rw.abs().max()).item())
        if i < nl - 1:
            eb = max(eb, (got[kb].double().abs().max() / rw.abs().max()).item())
        else:
            rb = ref[kb].double()
            ek = max(ek, ((got[kb].double() - rb).abs().max() / rb.abs().max()).item())
    return ek, eb


# (nh, nl, B, shift) -> (seed, float32-CPU worst kernel error, float32-CPU worst BN-fed bias), measured by grad_errs on the float32 run of
# the restatement against its float64 run on the case's own inputs; the seed is the first one that kink_margin accepts.
#
# Depths.  The margin m grows with the depth (1e-5 after one BN layer at B = 8200, 4e-5 after five), so the wanted shapes (256, 6, 257),
# (256, 6, 1000), (96, 3, 8200) and (256, 3, 8200) find no kink-free seed in 2000 tries; neither do (256, 3, 1000) nor (256, 2, 8200),
# where 2.1 million BN outputs stand against a margin of 3e-5.  Their number of layers is reduced until a seed is found, never their B:
# (256, 4, 257), (256, 2, 1000), (96, 2, 8200); 256 units at B = 8200 have no kink-free seed at any depth.
# The full depths, and with them the MFMA layers at T = 64, run as the shift = 8 cases instead: beta = +-8 turns every unit on for the
# whole batch or off for the whole batch, which is kink-free by construction (asserted like the others).  Their nets are worse
# conditioned (every layer's input carries a common offset of 8 that the next BN removes again), so their float32-CPU figures, and with
# them their bars, are larger.
GRAD_CASES = {
    (65, 2, 33, 0.0): (0, 6.5e-07, 5.7e-07),        # no hidden -> hidden layer
    (96, 3, 37, 0.0): (0, 1.0e-06, 3.5e-07),
    (129, 4, 65, 0.0): (1, 1.4e-06, 6.6e-07),       # two row groups plus one row
    (200, 6, 97, 0.0): (30, 2.9e-06, 1.7e-06),
    (256, 4, 257, 0.0): (992, 3.0e-06, 6.4e-07),    # two chunks plus one sample
    (256, 2, 1000, 0.0): (33, 1.1e-06, 3.0e-07),
    (96, 2, 8200, 0.0): (1, 4.7e-07, 3.6e-07),      # T = 64
    (256, 6, 257, 8.0): (0, 9.4e-04, 2.6e-05),
    (256, 6, 1000, 8.0): (0, 2.4e-03, 4.6e-06),
    (96, 3, 8200, 8.0): (0, 4.8e-05, 2.2e-06),      # T = 64
    (256, 6, 8200, 8.0): (0, 2.7e-04, 1.0e-05),     # T = 64
}


EMBED_SEED = 1690            # case_inputs(EMBED_SEED, 64, 6, 1000): the first seed that kink_margin accepts for the 64 x 6 net

CARRIED = (129, 4, 65)      # five carried G steps: two row groups plus one row, two MFMA layers
CARRIED_SEED = 14           # the first seed that carried_kink_free accepts


def carried_batches(seed):
    rs = np.random.RandomState(seed + 1000)
    return [(rs.randn(CARRIED[2], 2).astype(np.float32), (1e-1 * rs.randn(CARRIED[2], 2)).astype(np.float32)) for _ in range(5)]


def carried_kink_free(seed):
    """the kink condition at every one of the five steps, each on the variables its float64 and float32 trajectories have reached"""
    P = perturbed_params(seed, CARRIED[0], CARRIED[1])
    Q64, Q32 = R.to_torch(P, torch.float64), R.to_torch(P, torch.float32)
    for z, gp in carried_batches(seed):
        z64, z32 = torch.as_tensor(z, dtype=torch.float64), torch.as_tensor(z)
        y64, y32 = bn_outputs(Q64, z64), bn_outputs(Q32, z32)
        m = 4 * max((a.double() - b).abs().max().item() for a, b in zip(y32, y64))
        if min(b.abs().min().item() for b in y64) < m:
            return False
        R.g_step(Q64, z64, torch.as_tensor(gp, dtype=torch.float64), 5e-3)
        R.g_step(Q32, z32, torch.as_tensor(gp), 5e-3)
    return True


def embed(P, wide):
    """the narrow net of P in the first units of a `wide`-unit net: the others take zero weights in and out, zero bias, gamma 1, beta 0"""
    from cgs_amd.synthetic import WideMLPGenerator
    nl = R.nlayers_of(P, "generator/g_fc")
    E = WideMLPGenerator.init_params(0, wide, nl)
    for k, v in P.items():
        e = np.zeros_like(E[k]) if k.endswith("/kernel") or k.endswith("/bias") else E[k]
        e[tuple(slice(0, n) for n in v.shape)] = v
        E[k] = e
    return E


# ---- tests --------------------------------------------------------------------------------------------------------------------------
def _step(l, nl, nh, B=1000, ws=None, ws_bytes=0, fn="cgs_mlp2d_wide_g_step"):
    return getattr(l, fn)(None, None, None, None, None, None, nl, nh, None, None, B, 1e-5, 5e-3, None, None, None, ws, ws_bytes, None)


def test_new_symbols_are_declared_and_typed():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        nargs = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
    l = lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert lib.SIGNATURES["cgs_mlp2d_wide_g_step"] == lib.SIGNATURES["cgs_mlp2d_g_step"]


@pytest.mark.parametrize("nl,nh", [(6, 64), (6, 257), (7, 256), (1, 256)])
def test_wide_g_step_refuses_other_widths_and_depths(nl, nh):
    from cgs_amd import lib
    l = lib.load()
    assert _step(l, nl, nh) == lib.EINVAL
    msg = l.cgs_last_error()
    assert msg.startswith(b"mlp2d_wide_g_step") and b"need 2..6, 65..256" in msg
    assert int(l.cgs_mlp2d_wide_g_step_ws_bytes(1000, nl, nh)) == 0


@pytest.mark.parametrize("nl,nh", [(6, 256), (2, 65), (6, 128)])
def test_wide_g_step_accepts_65_to_256_units(nl, nh):
    """Past the shape check the next refusal is the null weight array: still CGS_EINVAL, another message."""
    from cgs_amd import lib
    l = lib.load()
    assert _step(l, nl, nh) == lib.EINVAL and b"mlp2d_wide_g_step: null weight array" in l.cgs_last_error()


def test_narrow_g_step_still_stops_at_64_units():
    from cgs_amd import lib
    l = lib.load()
    assert _step(l, 6, 256, fn="cgs_mlp2d_g_step") == lib.EINVAL
    msg = l.cgs_last_error()
    assert msg.startswith(b"mlp2d_g_step") and b"nlayers" in msg


def _ladder(fn, narrow, step):
    """-> [(what, call arguments, return code, message)] of every refusal of a generator entry point, in the order the entry point checks.
    The pointer arrays are host arrays of non-null dummy addresses: every rung returns before anything is dereferenced on the device."""
    import ctypes as C
    from cgs_amd import lib
    who = fn[4:].encode()
    nl, nh, B = (6, 64, 1000) if narrow else (6, 256, 1000)
    buf = (C.c_float * 4)()
    addr = C.addressof(buf)
    full = lambda n: (C.c_void_p * 6)(*([addr] * n + [None] * (6 - n)))
    W, BN = full(nl), full(nl - 1)
    l = lib.load()
    if narrow:
        need = lambda b: int(l.cgs_mlp2d_gen_ws_bytes(b, nl, 1 if step else 0))
    else:
        need = lambda b: int(getattr(l, "cgs_mlp2d_wide_g_step_ws_bytes" if step else "cgs_mlp2d_wide_gen_ws_bytes")(b, nl, nh))

    def args(w=W, b=W, gamma=BN, beta=BN, mm=BN, mv=BN, nl_=nl, nh_=nh, z=addr, out=addr, B_=B, train=1, eps=1e-5, ws=addr, ws_bytes=None):
        ws_bytes = need(B_) if ws_bytes is None else ws_bytes
        if step:        # w b gamma beta mm mv nl nh z grad_plugin B eps lr gw gb x ws ws_bytes stream
            return (w, b, gamma, beta, mm, mv, nl_, nh_, z, out, B_, eps, 5e-3, None, None, None, ws, ws_bytes, None)
        return (w, b, gamma, beta, mm, mv, nl_, nh_, z, out, B_, train, eps, None, ws, ws_bytes, None)

    lo, hi = (1, 64) if narrow else (65, 256)
    shape = lambda a, h: b"%s: nlayers=%d nhidden=%d (need 2..6, %d..%d)" % (who, a, h, lo, hi)
    badarg = lambda b_, t: b"%s: bad argument (B=%d, training=%d)" % (who, b_, t)
    E, EW = lib.EINVAL, lib.EWORKSPACE
    rungs = [
        ("one layer", args(nl_=1), E, shape(1, nh)),
        ("seven layers", args(nl_=7), E, shape(7, nh)),
        ("too wide", args(nh_=hi + 1), E, shape(nl, hi + 1)),
        ("too narrow", args(nh_=lo - 1), E, shape(nl, lo - 1)),
        ("shape before anything else", args(nl_=7, w=None, out=None, gamma=None, B_=0, eps=0.0, ws=None), E, shape(7, nh)),
        ("null w array", args(w=None), E, who + b": null weight array"),
        ("null b array", args(b=None), E, who + b": null weight array"),
        ("a null weight", args(w=full(nl - 1)), E, who + b": null weight"),
        ("a null bias", args(b=full(nl - 1)), E, who + b": null weight"),
        ("weights before the output", args(w=full(nl - 1), out=None, gamma=None), E, who + b": null weight"),
        ("null output / grad_plugin", args(out=None), E, who + (b": null grad_plugin" if step else b": null output")),
        ("output before batch norm", args(out=None, gamma=None, B_=0), E, who + (b": null grad_plugin" if step else b": null output")),
    ]
    for k in ("gamma", "beta", "mm", "mv"):
        rungs.append(("null %s array" % k, args(**{k: None}), E, who + b": null batch-norm array"))
    rungs.append(("arrays before variables", args(gamma=full(nl - 2), beta=None), E, who + b": null batch-norm array"))
    for k in ("gamma", "beta", "mm", "mv"):
        rungs.append(("a null %s" % k, args(**{k: full(nl - 2)}), E, who + b": null batch-norm variable"))
    rungs.append(("batch norm before the batch", args(mv=full(nl - 2), B_=0, ws=None), E, who + b": null batch-norm variable"))
    rungs += [
        ("null z", args(z=None), E, badarg(B, 1)),
        ("B = 1 in training", args(B_=1), E, badarg(1, 1)),
        ("B = 0", args(B_=0), E, badarg(0, 1)),
        ("B < 0", args(B_=-5), E, badarg(-5, 1)),
        ("eps = 0", args(eps=0.0), E, badarg(B, 1)),
        ("eps < 0", args(eps=-1e-5), E, badarg(B, 1)),
        ("eps nan", args(eps=float("nan")), E, badarg(B, 1)),
        ("the batch before the workspace", args(B_=1, ws=None, ws_bytes=0), E, badarg(1, 1)),
    ]
    if not step:
        rungs += [("B = 0 at inference", args(B_=0, train=0), E, badarg(0, 0)),
                  ("eps = 0 at inference", args(train=0, eps=0.0), E, badarg(B, 0)),
                  ("any non-zero is_training is training", args(B_=1, train=7), E, badarg(1, 1))]
    if not narrow:
        rungs.append(("B = 2^24 + 1", args(B_=(1 << 24) + 1, ws_bytes=1 << 40), E, badarg((1 << 24) + 1, 1)))
        if not step:
            rungs.append(("B = 2^24 + 1 at inference", args(B_=(1 << 24) + 1, train=0, ws_bytes=1 << 40), E, badarg((1 << 24) + 1, 0)))
    n = need(B)
    assert n > 4
    wsmsg = lambda have: b"%s: workspace %d < %d bytes" % (who, have, n)
    rungs += [
        ("short workspace", args(ws_bytes=n - 4), EW, wsmsg(n - 4)),
        ("no workspace bytes", args(ws_bytes=0), EW, wsmsg(0)),
        ("null workspace", args(ws=None), EW, wsmsg(n)),
    ]
    if not step:
        rungs.append(("short workspace at inference", args(train=0, ws_bytes=n - 4), EW, wsmsg(n - 4)))
    return l, rungs


@pytest.mark.parametrize("fn,narrow,step", [("cgs_mlp2d_gen_fwd", True, False), ("cgs_mlp2d_g_step", True, True),
                                            ("cgs_mlp2d_wide_gen_fwd", False, False), ("cgs_mlp2d_wide_g_step", False, True)])
def test_generator_entry_points_refuse_in_one_order_with_one_text(fn, narrow, step):
    """The whole refusal ladder of the four generator entry points -- shape, weight arrays, weights, output or grad_plugin, batch-norm
    arrays, batch-norm variables, batch and eps, workspace -- rung by rung: the return code and the full text of cgs_last_error().
    Every rung returns before the first device call."""
    l, rungs = _ladder(fn, narrow, step)
    for what, a, rc, msg in rungs:
        assert getattr(l, fn)(*a) == rc, (fn, what)
        assert l.cgs_last_error() == msg, (fn, what)


def test_wide_g_step_workspace_size():
    from cgs_amd import lib
    l = lib.load()
    ws = lambda B, nl, nh: int(l.cgs_mlp2d_wide_g_step_ws_bytes(B, nl, nh))
    fwd = lambda B, nl, nh: int(l.cgs_mlp2d_wide_gen_ws_bytes(B, nl, nh))
    assert ws(0, 6, 256) == 0 and ws(-1, 6, 256) == 0 and ws((1 << 24) + 1, 6, 256) == 0 and ws(1 << 24, 6, 256) > 0
    for nl, nh in ((6, 256), (3, 96), (2, 65), (6, 200)):
        nhp = -(-nh // 32) * 32
        prev = 0
        # mlpw_chunk steps at every multiple of 2048 samples: both sides of the first steps, and a large batch
        for B in (2, 31, 32, 33, 1000, 2047, 2048, 2049, 4096, 4097, 8200, 10000, 100000):
            n = ws(B, nl, nh)
            assert n >= fwd(B, nl, nh) + (nl - 1) * B * nhp * 4 and n % 4 == 0
            assert n >= prev, (nl, nh, B)
            prev = n


def _numpy_g_step(P, z, gp):
    """the G step's gradients in plain float64 numpy: forward, then dxhat = gamma [gamma xhat + beta > 0] dh and
    da = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) layer by layer"""
    nl = R.nlayers_of(P, "generator/g_fc")
    W = [np.asarray(P[f"generator/g_fc{i + 1}/kernel"], np.float64) for i in range(nl)]
    b = [np.asarray(P[f"generator/g_fc{i + 1}/bias"], np.float64) for i in range(nl)]
    gam = [np.asarray(P[f"{R.bn_name(i)}/gamma"], np.float64) for i in range(nl - 1)]
    bet = [np.asarray(P[f"{R.bn_name(i)}/beta"], np.float64) for i in range(nl - 1)]
    h, hs, xh, rs = z.astype(np.float64), [], [], []
    for i in range(nl - 1):
        hs.append(h)
        a = h @ W[i] + b[i]
        r = 1.0 / np.sqrt(a.var(0) + R.EPS)
        x = (a - a.mean(0)) * r
        xh.append(x); rs.append(r)
        h = np.maximum(gam[i] * x + bet[i], 0.0)
    hs.append(h)
    g = {}
    d = gp.astype(np.float64)
    for i in range(nl - 1, -1, -1):
        g[f"generator/g_fc{i + 1}/kernel"] = hs[i].T @ d
        g[f"generator/g_fc{i + 1}/bias"] = d.sum(0)
        if i == 0:
            break
        dh = d @ W[i].T
        dx = np.where(gam[i - 1] * xh[i - 1] + bet[i - 1] > 0, dh * gam[i - 1], 0.0)
        d = rs[i - 1] * (dx - dx.mean(0) - xh[i - 1] * (dx * xh[i - 1]).mean(0))
    return g


def test_restatement_bn_backward_at_256_x_6_matches_numpy():
    P, z, gp = case_inputs(3, 256, 6, 300)
    ref, _ = g_step_ref(P, z, gp, torch.float64)
    want = _numpy_g_step(P, z, gp)
    for k, v in want.items():
        scale = max(np.abs(want[k.replace("/bias", "/kernel")]).max(), 1e-300)
        assert np.abs(ref[k].numpy() - v).max() / scale < 1e-10, k
