"""The refusal ladders of the discriminator-side 2-D entry points (csrc/mlp2d.hip, csrc/mlp2d_wide_train.hip), rung by rung: the return
code and the full text of cgs_last_error(), and the three workspace-size queries.  The generator's ladders are walked in
test_synthetic_wide_gstep_cpu.py.  Every rung returns before the first device call: the pointers are host addresses of a dummy buffer."""
import ctypes as C

import pytest

NL, B = 6, 1000
SHAPES = ((1, 2), (512, 6), (4097, 3))      # (B, nlayers) of the size queries


def _env():
    from cgs_amd import lib
    buf = (C.c_float * 4)()
    addr = C.addressof(buf)
    full = lambda n: (C.c_void_p * 6)(*([addr] * n + [None] * (6 - n)))
    return lib, lib.load(), buf, addr, full


def _train_bytes(Bt, nl):
    return (Bt * (nl - 1) * 64 * 2 + Bt * 2) * 4


def _wide_train_bytes(Bt, nl, nh):
    nhp = -(-nh // 32) * 32
    return (2 * (nl - 1) * Bt * nhp + 2 * Bt + 16 * ((nl - 2) * nhp * nhp + (nl + 2) * nhp + 4)) * 4


def _gen_bytes(Bn, nl, bwd):
    H = nl - 1
    return (H * Bn * 64 * (2 if bwd else 1) + H * 256 * 128 + H * 128) * 4


def _net_rungs(who, args, full, lo, hi, nh, extra_shapes=()):
    """shape, then the weight arrays, then every weight: the rungs every entry point starts with"""
    from cgs_amd import lib
    E = lib.EINVAL
    shape = lambda a, h: b"%s: nlayers=%d nhidden=%d (need 2..6, %d..%d)" % (who, a, h, lo, hi)
    rungs = [
        ("one layer", args(nl=1), E, shape(1, nh)),
        ("seven layers", args(nl=7), E, shape(7, nh)),
        ("no units", args(nh=0), E, shape(NL, 0)),
        ("257 units", args(nh=257), E, shape(NL, 257)),
    ]
    rungs += [("%d units" % h, args(nh=h), E, shape(NL, h)) for h in extra_shapes]
    rungs += [
        ("shape before the weights", args(nl=7, w=None), E, shape(7, nh)),
        ("null w array", args(w=None), E, who + b": null weight array"),
        ("null b array", args(b=None), E, who + b": null weight array"),
        ("a null weight", args(w=full(NL - 1)), E, who + b": null weight"),
        ("a null bias", args(b=full(NL - 1)), E, who + b": null weight"),
    ]
    return rungs


def _walk(l, fn, rungs):
    for what, a, rc, msg in rungs:
        assert getattr(l, fn)(*a) == rc, (fn, what)
        assert l.cgs_last_error() == msg, (fn, what)


@pytest.mark.parametrize("nh", [64, 256])
def test_sigmoid_saliency_refuses_rung_by_rung(nh):
    lib, l, buf, addr, full = _env()
    W = full(NL)
    who = b"mlp2d_sigmoid_saliency"

    def args(w=W, b=W, nl=NL, nh=nh, x=addr, sig=addr, sal=addr, B_=B):
        return (w, b, nl, nh, x, sig, sal, B_, 1.0 / B, None)

    bad = who + b": bad argument"
    rungs = _net_rungs(who, args, full, 1, 256, nh) + [
        ("weights before the batch", args(w=full(NL - 1), B_=0, x=None), lib.EINVAL, who + b": null weight"),
        ("B = 0", args(B_=0), lib.EINVAL, bad),
        ("B < 0", args(B_=-3), lib.EINVAL, bad),
        ("null x", args(x=None), lib.EINVAL, bad),
        ("null sigmoid", args(sig=None), lib.EINVAL, bad),
    ]
    _walk(l, "cgs_mlp2d_sigmoid_saliency", rungs)


@pytest.mark.parametrize("nh", [64, 256])
@pytest.mark.parametrize("dev", [False, True])
def test_refine2d_refuses_rung_by_rung(nh, dev):
    lib, l, buf, addr, full = _env()
    W = full(NL)
    who = b"refine2d"
    fn = "cgs_refine2d_devbase" if dev else "cgs_refine2d"

    def args(w=W, b=W, nl=NL, nh=nh, x=addr, base=addr, steps=10, method=2, bx=addr, bs=addr, traj=None, B_=B):
        return (w, b, nl, nh, x, base if dev else 0.5, 1.0 / B, steps, 0.1, method, bx, bs, traj, B_, None)

    bad = who + b": bad argument"
    E = lib.EINVAL
    rungs = []
    if dev:
        rungs += [("null baseline", args(base=None), E, b"refine2d_devbase: null baseline pointer"),
                  ("the baseline before the shape", args(base=None, nl=7, w=None), E, b"refine2d_devbase: null baseline pointer")]
    rungs += _net_rungs(who, args, full, 1, 256, nh) + [
        ("weights before the batch", args(w=full(NL - 1), B_=0, method=3), E, who + b": null weight"),
        ("B = 0", args(B_=0), E, bad),
        ("B < 0", args(B_=-3), E, bad),
        ("steps = -1", args(steps=-1), E, bad),
        ("method = -1", args(method=-1), E, bad),
        ("method = 3", args(method=3), E, bad),
        ("null x", args(x=None), E, bad),
        ("null best_x", args(bx=None), E, bad),
        ("null best_step", args(bs=None), E, bad),
    ]
    _walk(l, fn, rungs)


@pytest.mark.parametrize("wide", [False, True])
def test_d_step_refuses_rung_by_rung(wide):
    lib, l, buf, addr, full = _env()
    W = full(NL)
    nh0 = 256 if wide else 64
    fn = "cgs_mlp2d_wide_d_step" if wide else "cgs_mlp2d_d_step"
    who = fn[4:].encode()
    need = lambda bt: _wide_train_bytes(bt, NL, nh0) if wide else _train_bytes(bt, NL)

    def args(w=W, b=W, nl=NL, nh=nh0, real=addr, Br=B, fake=addr, Bf=B, ws=addr, ws_bytes=None):
        ws_bytes = need(Br + Bf) if ws_bytes is None else ws_bytes
        return (w, b, nl, nh, real, Br, fake, Bf, 1e-3, None, None, None, ws, ws_bytes, None)

    bad = who + b": bad argument"
    E, EW = lib.EINVAL, lib.EWORKSPACE
    lo, hi = (65, 256) if wide else (1, 64)
    rungs = _net_rungs(who, args, full, lo, hi, nh0, extra_shapes=(64,) if wide else (65,)) + [
        ("weights before the batch", args(w=full(NL - 1), Br=0, ws=None), E, who + b": null weight"),
        ("B_real = 0", args(Br=0), E, bad),
        ("B_real < 0", args(Br=-1), E, bad),
        ("B_fake = 0", args(Bf=0), E, bad),
        ("B_fake < 0", args(Bf=-1), E, bad),
        ("null real", args(real=None), E, bad),
        ("null fake", args(fake=None), E, bad),
        ("the batch before the workspace", args(Bf=0, ws=None, ws_bytes=0), E, bad),
    ]
    if wide:
        rungs += [("B_real + B_fake = 2^24 + 1", args(Br=1 << 24, Bf=1, ws_bytes=1 << 44), E, bad),
                  ("... the other way round", args(Br=1, Bf=1 << 24, ws_bytes=1 << 44), E, bad)]
    n = need(2 * B)
    wsmsg = lambda have: b"%s: workspace %d < %d bytes" % (who, have, n)
    rungs += [
        ("workspace one byte short", args(ws_bytes=n - 1), EW, wsmsg(n - 1)),
        ("no workspace bytes", args(ws_bytes=0), EW, wsmsg(0)),
        ("null workspace", args(ws=None), EW, wsmsg(n)),
    ]
    _walk(l, fn, rungs)
    assert int(l.cgs_mlp2d_wide_train_ws_bytes(2 * B, NL, nh0) if wide else l.cgs_mlp2d_train_ws_bytes(2 * B, NL)) == n


def test_train_ws_bytes():
    _, l, *_ = _env()
    q = lambda b, nl: int(l.cgs_mlp2d_train_ws_bytes(b, nl))
    for b, nl in ((0, 6), (-1, 6), (512, 1), (512, 7)):
        assert q(b, nl) == 0, (b, nl)
    for b, nl in SHAPES:
        assert q(b, nl) == _train_bytes(b, nl), (b, nl)


def test_wide_train_ws_bytes():
    _, l, *_ = _env()
    q = lambda b, nl, nh: int(l.cgs_mlp2d_wide_train_ws_bytes(b, nl, nh))
    for b, nl, nh in ((0, 6, 256), (-1, 6, 256), (512, 1, 256), (512, 7, 256), (512, 6, 64), (512, 6, 0), (512, 6, 257)):
        assert q(b, nl, nh) == 0, (b, nl, nh)
    for nh in (65, 96, 200, 256):
        for b, nl in SHAPES:
            assert q(b, nl, nh) == _wide_train_bytes(b, nl, nh), (b, nl, nh)


def test_gen_ws_bytes():
    _, l, *_ = _env()
    q = lambda b, nl, bwd: int(l.cgs_mlp2d_gen_ws_bytes(b, nl, bwd))
    for b, nl in ((0, 6), (-1, 6), (512, 1), (512, 7)):
        assert q(b, nl, 0) == 0 and q(b, nl, 1) == 0, (b, nl)
    for b, nl in SHAPES:
        for bwd in (0, 1):
            assert q(b, nl, bwd) == _gen_bytes(b, nl, bwd), (b, nl, bwd)
