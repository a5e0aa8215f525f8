"""The refinement loop's momentum step inside the backward-data launch that produces its gradient (include/cgs_hip.h,
cgs_*_bwd_data_update; csrc/igemm.hip: igemm_up_kernel and the update forms of the two reduce kernels), and the norm-backward sums at
a size the engine used to keep on the separate pass.

The fused entry point and the two-launch form (plain backward-data, then cgs_refine_update) share ONE element formula (refine_update1,
csrc/cgs_internal.h) and the gradient element is the same fp32 value in a register as in memory: feature and momentum are held to
``torch.equal``, not to a tolerance.  Both paths of a case get the SAME workspace size, so they take the same tile plan; a workspace of
only the packed weights (no room for split-K slabs) is how a small shape is made to reach the one-pass epilogue."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATE, ALPHA = 0.1, 0.9


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Call:
    """One backward-data call on raw pointers with a workspace of a chosen size: ``op`` "deconv" (forward direction: a strided conv of
    dy) or "conv" (transposed direction); B, H (square feature grid), Cin (the feature's channels), Cout (channels of dy), k, stride."""

    def __init__(self, op, B, H, Cin, Cout, k, s, slabs):
        from cgs_amd import lib
        self.lib = lib
        self.deconv = op == "deconv"
        self.op = lib.DECONV_BWD_DATA if self.deconv else lib.CONV_BWD_DATA
        Ho = H * s if self.deconv else -(-H // s)
        self.dims = (B, H, H, Cin, Ho, Ho, Cout, k, k, s, s)
        d = dev()
        self.dy = rnd((B, Ho, Ho, Cout), 3).to(d)
        self.w = (rnd((k, k, Cout, Cin), 2, 0.05) if self.deconv else rnd((k, k, Cin, Cout), 2, 0.05)).to(d)
        self.shape = (B, H, H, Cin)
        packed = lib.conv_ws_bytes(self.op, k, k, s, s, Cin, Cout)
        full = max(lib.conv_ws_bytes_for(self.op, B, H, H, Cin, Cout, k, k, s, s), 16)
        self.ws_bytes = full if slabs else packed
        if not slabs and self.form()[0] != 0:
            # cgs_conv_ws_bytes also covers the wider packed layouts of other kernel families: the smallest workspace the query accepts is
            # the exact-fp32 packed image alone -- no room for partial slabs behind it (a host-side bisection: the query launches nothing)
            lo, hi = 0, packed // 16
            while hi - lo > 1:
                mid = (lo + hi) // 2
                self.ws_bytes = mid * 16
                lo, hi = (lo, mid) if self.form()[0] != 0 else (mid, hi)
            self.ws_bytes = hi * 16
        self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=d)

    def form(self):
        order = C.c_int(0)
        f = int(self.lib.load().cgs_conv_update_form(self.op, *self.dims, self.ws_bytes, C.addressof(order)))
        return f, order.value

    def family(self):
        return int(self.lib.load().cgs_conv_family(self.op, *self.dims, self.lib.EPI_NONE, self.ws_bytes))

    def _geom(self):
        B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw = self.dims
        return (B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw) if self.deconv else (B, H, W, Cin, Cout, kh, kw, sh, sw)

    def plain(self, dx):
        name = "cgs_deconv2d_nhwc_bwd_data" if self.deconv else "cgs_conv2d_nhwc_bwd_data"
        self.lib.call(name, self.dy.data_ptr(), self.w.data_ptr(), dx.data_ptr(), *self._geom(), self.lib.EPI_NONE, None, None,
                      self.ws.data_ptr(), self.ws_bytes, 0, _stream())
        return self.lib.last_kernel()

    def fused_rc(self, theta, m, first):
        name = "cgs_deconv2d_nhwc_bwd_data_update" if self.deconv else "cgs_conv2d_nhwc_bwd_data_update"
        return int(getattr(self.lib.load(), name)(self.dy.data_ptr(), self.w.data_ptr(), theta.data_ptr(), m.data_ptr(), *self._geom(),
                                                   RATE, ALPHA, 1 if first else 0, self.ws.data_ptr(), self.ws_bytes, 0, _stream()))


EPILOGUE, SPLITK, TAIL = 1, 2, 3

# (id, op, B, H, Cin, Cout, k, stride, workspace with slab room, form to pin, row order to pin, PAR to pin or None)
CASES = [
    ("a-full-tile-pixel-major", "deconv", 128, 4, 256, 128, 5, 2, False, EPILOGUE, 2, False),
    ("b-ragged-M%128=64", "deconv", 3, 8, 256, 128, 5, 2, False, EPILOGUE, 0, False),      # M = 3 x 64: the last tile's second wave lies past M
    ("c-image-major", "deconv", 5, 8, 128, 64, 5, 2, False, EPILOGUE, 0, False),
    ("d-split-k", "deconv", 4, 4, 256, 128, 5, 2, True, SPLITK, 0, None),                  # 1 x 2 tiles, K = 3200
    ("e-tail-split", "deconv", 640, 8, 128, 64, 5, 2, True, TAIL, 2, None),
    ("f-transposed", "conv", 5, 8, 64, 128, 5, 2, False, EPILOGUE, 0, False),              # conv backward-data: four parity classes
    ("f-forward-parity-taps", "deconv", 2, 16, 64, 32, 3, 2, False, EPILOGUE, 0, True),    # stride 2 onto more than 64 pixels: the PAR kernels
    ("f-stride-1", "conv", 3, 8, 64, 96, 3, 1, False, EPILOGUE, 0, False),                 # ... ragged too (M = 192)
    ("g-64-channels", "deconv", 128, 4, 64, 64, 5, 2, False, EPILOGUE, 2, False),
    ("g-128-channels", "deconv", 130, 4, 128, 64, 5, 2, False, EPILOGUE, 1, False),        # pixel-major, tiles that straddle two pixels
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_update_is_the_two_launch_form_bit_for_bit(case):
    """Both paths from identical feature / momentum inputs, a first step (the momentum buffer starts as NaN: it must not be read into the
    result) and a second one; the case must take the form it pins (fail, not skip -- except the tail split, should no small shape plan one)."""
    from cgs_amd import lib
    cid, op, B, H, Cin, Cout, k, s, slabs, want_form, want_order, want_par = case
    c = _Call(op, B, H, Cin, Cout, k, s, slabs)
    assert c.family() == lib.FAMILY_IGEMM
    form, order = c.form()
    if want_form == TAIL and form != TAIL:
        pytest.skip(f"no tail split planned for this shape (form {form})")
    assert (form, order) == (want_form, want_order), f"{cid}: planned form {form}, row order {order}"
    d = dev()
    theta0 = rnd(c.shape, 7).to(d)
    th_f, th_s = theta0.clone(), theta0.clone()
    m_f, m_s = torch.full(c.shape, float("nan"), device=d), torch.full(c.shape, float("nan"), device=d)
    g = torch.empty(c.shape, device=d)
    for step in range(2):
        first = step == 0
        assert c.fused_rc(th_f, m_f, first) == 0, lib.load().cgs_last_error().decode()
        kname = lib.last_kernel()
        if form == SPLITK:
            assert kname.startswith("igemm_kernel<")                  # raw slabs from the plain kernel; the reduce pass updates
        else:
            assert kname.startswith("igemm_up_kernel<"), kname
            if want_par is not None:
                assert kname.endswith(", true>" if want_par else ", false>"), kname
        if form == TAIL:
            assert lib.load().cgs_last_tail_tiles() > 0 and lib.load().cgs_last_tail_split() > 1
        pname = c.plain(g)
        assert pname.split("<")[1] == kname.split("<")[1]             # the same tile plan
        lib.call("cgs_refine_update", th_s.data_ptr(), m_s.data_ptr(), g.data_ptr(), RATE, ALPHA, 1 if first else 0, 0, 0.0, 0.0, g.numel(),
                 _stream())
        assert torch.isfinite(m_f).all() and torch.isfinite(th_f).all()
        assert torch.equal(m_f, m_s), f"{cid} step {step}: momentum differs"
        assert torch.equal(th_f, th_s), f"{cid} step {step}: feature differs"
    assert not torch.equal(th_f, theta0)


@pytest.mark.parametrize("why,op,B,H,Cin,Cout,k,s", [
    ("Cin % 4 != 0", "deconv", 4, 8, 6, 64, 3, 2),
    ("a reduction that is not whole 32-channel chunks", "deconv", 3, 8, 128, 3, 3, 2),
])
def test_not_offered_is_honest(why, op, B, H, Cin, Cout, k, s):
    """Where the query says no, the entry point returns its error code and leaves feature and momentum untouched."""
    from cgs_amd import lib
    c = _Call(op, B, H, Cin, Cout, k, s, True)
    assert c.form()[0] == 0
    d = dev()
    theta0, m0 = rnd(c.shape, 7).to(d), rnd(c.shape, 8).to(d)
    theta, m = theta0.clone(), m0.clone()
    rc = c.fused_rc(theta, m, False)
    torch.cuda.synchronize()
    assert rc == lib.EINVAL and "cgs_conv_update_form" in lib.load().cgs_last_error().decode()
    assert torch.equal(theta, theta0) and torch.equal(m, m0)
    from cgs_amd import kernels as K
    assert K.conv_update_form(c.op, *c.dims) is None
    with pytest.raises(lib.CgsError):
        K.deconv2d_bwd_data(c.dy, c.w, (H, H), s, s, update=K.FusedUpdate(theta, m, RATE, ALPHA, False))
    assert torch.equal(theta, theta0) and torch.equal(m, m0)


def test_no_twin_in_the_split_bf16_mode():
    from cgs_amd import kernels as K, lib
    with K.contraction("bx6_all"):
        assert K.conv_update_form(lib.DECONV_BWD_DATA, 128, 4, 4, 256, 8, 8, 128, 5, 5, 2, 2) is None
    assert K.conv_update_form(lib.DECONV_BWD_DATA, 128, 4, 4, 256, 8, 8, 128, 5, 5, 2, 2) is not None


_PARAMS = {}


def _setup(arch, B):
    from oracle import nets_ref as N
    from cgs_amd.nets import ARCHS, g_input_shape, to_device
    if arch not in _PARAMS:
        _PARAMS[arch] = N.init_params(arch, 2019, True)
    d = dev()
    z = torch.from_numpy(np.random.RandomState(6).uniform(-1, 1, (B,) + g_input_shape(ARCHS[arch])).astype(np.float32)).to(d)
    return to_device(_PARAMS[arch], d), z


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("arch", ["dcgan64", "dcgan32"])
def test_engine_fused_and_separate_updates_agree_bit_for_bit(arch, use_graph):
    """Refined features, images, best-step indices and scores of the engine with the update in the backward-data launch against the same
    engine held to the separate kernel (``fused_update = False``); deterministic and probabilistic mode, momentum and sgd.  With a clip set
    both engines take the separate kernel: the pair still agrees, and no update-carrying launch is recorded for either."""
    from cgs_amd import kernels as K
    from cgs_amd.engine import RefineEngine
    B, steps = 16, 3
    P, z = _setup(arch, B)
    fused = RefineEngine(arch, P, B, dev(), use_graph=use_graph)
    sep = RefineEngine(arch, P, B, dev(), use_graph=use_graph)
    assert fused.update_form is not None and fused.fused_update
    sep.fused_update = False
    idx = np.random.RandomState(3).randint(steps + 1, size=B)
    for kw in (dict(), dict(method="sgd"), dict(mode="probabilistic", indices=idx), dict(vmin=-0.5, vmax=0.5)):
        for _ in range(2 if use_graph else 1):                       # (graph: the capture call, then a replay)
            got = [t.clone() for t in fused.refine_from_z(z, steps, 0.1, **kw)]
            want = [t.clone() for t in sep.refine_from_z(z, steps, 0.1, **kw)]
            for a, b in zip(got, want):
                assert torch.isfinite(a).all() and torch.equal(a, b), kw
    if not use_graph:
        # the records name what ran: the fused program has no refine_update, the clip program has one per step and no update launch
        for kw, n_sep in ((dict(), 0), (dict(vmin=-0.5, vmax=0.5), steps)):
            K.PROFILE = {}
            try:
                fused.refine_from_z(z, steps, 0.1, **kw)
                torch.cuda.synchronize()
                rec = K.PROFILE
            finally:
                K.PROFILE = None
            assert len(rec.get("refine_update", [0, []])[1]) == n_sep
            assert ("igemm_up_kernel" in " ".join(rec)) == (n_sep == 0 and fused.update_form[0] != "splitk")


@pytest.mark.parametrize("B", [96, 104])
def test_norm_backward_sums_at_the_former_48_mb_limit(B):
    """test_backward_data_leaves_the_norm_backward_sums's check of the norm's input gradient at the size where the engine's limit stood: a
    32 x 32 x 128 norm input at batch 96 is 50.3 MB (48 MiB to the byte, the old limit itself), at batch 104 54.5 MB -- past it.  From the
    partials == the separate-pass kernels to 1e-5 (that test's bar)."""
    from cgs_amd import kernels as K, lib
    H, Cn, Cabove, k, s_, leak = 32, 128, 256, 5, 2, 0.2
    d = dev()
    x = rnd((B, H, H, Cn), 1).to(d)
    assert x.numel() * 4 >= 48 * 2 ** 20
    gamma, beta = (rnd((Cn,), 4, 0.2) + 1).to(d), rnd((Cn,), 5, 0.1).to(d)
    _, mean, invstd = K.instnorm_lrelu_fwd(x.view(1, -1, Cn), gamma, beta, leak)
    Ho = H // s_
    w = rnd((k, k, Cn, Cabove), 2, 0.05).to(d)
    g = rnd((B, Ho, Ho, Cabove), 3).to(d)
    lay = K.conv_stat_layout(lib.CONV_BWD_DATA, B, H, H, Cn, 0, 0, Cabove, k, k, s_, s_, B)
    assert lay is not None
    part = torch.full((lay[0], 2, Cn), float("nan"), device=d)
    ns = K.NormBwdStats(x, mean, invstd, gamma, beta, leak, B, part, lay)
    dy = K.conv2d_bwd_data(g, w, (H, H), s_, s_, nstat=ns)
    assert lib.last_kernel().startswith("igemm_ns_kernel")
    assert torch.isfinite(part).all()
    want = K.instnorm_lrelu_bwd_data(dy.view(1, -1, Cn).clone(), x.view(1, -1, Cn), gamma, beta, mean, invstd, leak)
    got = K.norm_lrelu_bwd_from_partials(dy, x, ns, 1, out=dy)
    err = (got.reshape(-1) - want.reshape(-1)).abs().max().item()
    ref = want.abs().max().item() + 1e-30
    print(f"\n[nstats B={B}] max|delta| = {err:.3e}, max|ref| = {ref:.3e} (bar 1e-5 of max|ref|)")
    assert err <= 1e-5 * ref


def test_the_engine_links_the_big_norms_too():
    """No size gate is left in the engine: at a batch whose norm inputs pass 48 MB every batch norm of D that sits under a conv has its
    backward sums linked (the library's own "not available" is the only limit)."""
    from cgs_amd.engine import RefineEngine, _BnTrainLrelu
    B = 512                                                           # D's first norm input: 512 x 16 x 16 x 128 floats = 67 MB
    P, _ = _setup("dcgan64", 1)
    eng = RefineEngine("dcgan64", P, B, dev())
    norms = [st for st in eng.d.stages if isinstance(st, _BnTrainLrelu)]
    assert norms and max(st.out.numel() * 4 for st in norms) > 48 * 2 ** 20
    big = [st for st in norms if st.out.numel() * 4 > 48 * 2 ** 20]
    assert all(st.bstat is not None for st in big)
