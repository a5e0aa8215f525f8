"""The implicit-GEMM launch plans one by one (csrc/igemm.hip: igemm_plan, cgs_igemm_launch, the three reduce kernels and the _ns / _up
twins): one test per row of tests/igemm_cases.py's table.  Each row runs its call through cgs_amd.kernels at the workspace the row names
("full": what the workspace cache hands the call; "none": the fp32 packed weights alone, no slab) and asserts, in this order,

    the query    what cgs_conv_igemm_plan said about the call and workspace before the launch (kernel, tail, plan note, executed FLOPs)
                 is what the launch noted
    the plan     cgs_last_kernel() is the predicted instantiation, exactly; cgs_last_tail_tiles() / cgs_last_tail_split(),
                 cgs_last_igemm_plan() (xcd_map, cls_flip, uni, gx, split-K factor) and cgs_last_executed_flops() equal the restated
                 planner's answer -- so a plan change that sends the row elsewhere fails here by name instead of testing another plan
    the result   against float64 at the project's operator bar, unchanged: max|delta| <= 2e-5 max(1, sqrt(K / 1000)) max|ref| with K the
                 longest class's reduction length, x 1.5 under the forward tanh
    the form     statistics: the partial rows summed in float64 against the reference's column sums at the same bar, rows past the launch's own never written; update: theta and m against the float64 update at the bar and
                 bit-equal to the unfused pair (backward-data, then cgs_refine_update); signs: every bit
    a second run bit-identical in everything it leaves

On a device that does not report 256 compute units the round rules are off: the prediction is made for that count, and only the rows
whose prediction changes with it (their named feature is a round rule) skip.

The float32 torch-CPU oracle's own worst against the same reference: igemm_cases.ORACLE_WORST / ORACLE_OF_BAR.
The device's measured worst over the table (MI355X, 126 figures on 78 rows; every figure is printed before it is asserted, run with -s):
    2.32e-6 of max|ref| = 0.081 of the bar   at conv_fwd-33700x1x1x2048-32-k1s1-plain-none-full (264 tiles, tail split 8 x 16, K = 2048)
    9.98e-7               0.049              at conv_bwd-4x8x8x64-256-k3s2-nstats-none-none (the one-pass norm-backward epilogue)
    1.37e-6               0.046              at conv_fwd-256x32x32x32-32-k3s2-plain-tanh-full
    update rows (theta drawn at the scale of rate x g): at most 0.033 of the bar on theta and m
Every name, tail, plan-note and FLOP assertion holds, every second run is bit-identical, no defect was found; the module takes 9 s.
"""
import pytest
import torch

import igemm_cases as IC
from igemm_cases import BD, F, TB, TF
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu


def hold(got, want, tol, what):
    err = float((got.detach().cpu().double() - want).abs().max())
    ref = float(want.abs().max())
    print(f"device {what}: max|delta|/max|ref| = {err / ref:.3e} = {err / ref / tol:.3f} of the bar {tol:.2e}")
    assert tuple(got.shape) == tuple(want.shape)
    assert err <= tol * ref, f"{what}: max|delta| = {err:.3e} vs {tol:.2e} x max|ref| = {tol * ref:.3e}"


def unpack_signs(words, P, N):
    """uint32 word[(c / 32) * P + p], bit 8 * (c % 4) + (c % 32) / 4 -> bool [P, N]."""
    w = words.cpu().view(N // 32, P).to(torch.int64) & 0xffffffff
    c = torch.arange(N)
    bit = 8 * (c % 4) + (c % 32) // 4
    return ((w[c // 32, :] >> bit[:, None]) & 1).bool().t()


@pytest.mark.parametrize("case", IC.CASES, ids=IC.case_id)
def test_launch_plan(case, monkeypatch):
    from cgs_amd import kernels as K, lib as L
    d = dev()
    lib = L.load()
    c = case
    cus = torch.cuda.get_device_properties(d).multi_processor_count
    pred = IC.case_plan(lib, c, cus)
    if cus != 256 and pred != IC.case_plan(lib, c, 256):
        pytest.skip(f"the row is there for a round rule, and the device reports {cus} compute units")
    assert not pred.refused
    monkeypatch.setattr(K, "WS", K._WsCache())
    if c.slab == "none":
        monkeypatch.setattr(L, "conv_ws_bytes_for", lambda *call: IC.none_ws_bytes(c))        # the fp32 packed weights, not a byte of slab
    inp, lin = IC.inputs_and_reference(c)
    want = IC.expected64(c, inp, lin)
    g = IC.case_geometry(c)
    Ho, Wo = IC.out_hw(c)
    x, w = inp.x.to(d), inp.w.to(d)
    bias = None if inp.bias is None else inp.bias.to(d)
    a, b = inp.a.to(d), inp.b.to(d)
    aux = None if inp.aux is None else inp.aux.to(d)
    P, N = g.B * g.Hout * g.Wout, g.N
    rows = IC.stat_rows(g)
    fwd_a = a if c.epilogue == IC.EPI_AFFINE_RELU else None
    fwd_b = b if c.epilogue == IC.EPI_AFFINE_RELU else None
    bwd = K.conv2d_bwd_data if c.op == BD else K.deconv2d_bwd_data

    def run():
        """-> everything the call leaves, as a dict of device tensors."""
        left = {}
        if c.form in ("stats", "nstats"):
            left["part"] = torch.full((rows + 2, 2, N), float("nan"), device=d)
        if c.form == "plain" and c.op == F:
            left["out"] = K.conv2d_fwd(x, w, bias, c.s, c.s, c.epilogue, fwd_a, fwd_b)
        elif c.form == "plain" and c.op == TF:
            left["out"] = K.deconv2d_fwd(x, w, bias, (Ho, Wo), c.s, c.s, c.epilogue, fwd_a, fwd_b)
        elif c.form == "plain":
            left["out"] = bwd(x, w, (c.H, c.W), c.s, c.s, epilogue=c.epilogue, ep_a=a if c.epilogue == IC.EPI_RELU_BWD_AFFINE else None, ep_aux=aux)
        elif c.form == "stats" and c.op == F:
            left["out"] = K.conv2d_fwd_stats(x, w, bias, left["part"], c.s, c.s)
        elif c.form == "stats":
            left["out"] = K.deconv2d_fwd(x, w, bias, (Ho, Wo), c.s, c.s, part=left["part"])
        elif c.form == "signs":
            left["signs"] = torch.zeros(P * N // 32, dtype=torch.int32, device=d)
            left["out"] = K.deconv2d_fwd(x, w, bias, (Ho, Wo), c.s, c.s, c.epilogue, fwd_a, fwd_b, signs=left["signs"])
        elif c.form == "nstats":
            layout = K.conv_stat_layout(c.op, c.B, c.H, c.W, c.Cin, Ho if c.op == TB else 0, Wo if c.op == TB else 0, c.Cout, c.k, c.k, c.s, c.s, c.B)
            assert layout is not None and layout[0] == rows
            ns = K.NormBwdStats(aux, inp.mean.to(d).view(1, N), inp.invstd.to(d).view(1, N), inp.gamma.to(d), inp.beta.to(d), IC.LEAK, c.B,
                                left["part"], layout)
            left["out"] = bwd(x, w, (c.H, c.W), c.s, c.s, nstat=ns)
        else:
            assert c.form == "update"
            left["theta"], left["m"] = inp.theta.to(d), inp.m.to(d)
            bwd(x, w, (c.H, c.W), c.s, c.s, update=K.FusedUpdate(left["theta"], left["m"], IC.RATE, IC.ALPHA, False))
        left["plan"] = (L.last_kernel(), int(lib.cgs_last_tail_tiles()), int(lib.cgs_last_tail_split()), L.last_igemm_plan(),
                        float(lib.cgs_last_executed_flops()))
        return left

    # what the library says about this call and workspace BEFORE the launch (cgs_conv_igemm_plan, host only) ...
    said = L.conv_igemm_plan(c.op, c.B, c.H, c.W, c.Cin, Ho if c.op in (TF, TB) else 0, Wo if c.op in (TF, TB) else 0, c.Cout, c.k, c.k, c.s, c.s,
                             c.epilogue, {"plain": L.FORM_PLAIN, "stats": L.FORM_STATS, "nstats": L.FORM_NSTATS, "signs": L.FORM_SIGNS,
                                          "update": L.FORM_UPDATE}[c.form], IC.ws_bytes(lib, c))
    assert said is not None
    got = run()
    name, tiles, split, (xcd, flip, uni, gx, sk), flops = got["plan"]
    what = IC.case_id(c)
    # ... is what the launch noted
    assert (said["kernel"], *said["tail"], said["plan"], said["flops"]) == got["plan"], (said, got["plan"])
    print(f"\n{what}: {name} tail {tiles} x {split}, xcd_map {xcd} cls_flip {flip} uni {uni} gx {gx} split-K {sk}, {flops:.0f} flops, then {pred.reduce}")
    assert name == pred.kernel, (name, pred.kernel)
    assert (tiles, split) == (pred.tail_n, pred.tail_s if pred.tail_s > 1 else 0), (tiles, split, pred.tail_n, pred.tail_s)
    assert (xcd, flip, uni, gx, sk) == (pred.xcd_map, pred.cls_flip, pred.uni, pred.gx, pred.splitk), ((xcd, flip, uni, gx, sk), pred)
    assert flops == float(pred.flops) and pred.flops < 2 ** 53, (flops, pred.flops)
    tol = IC.bar(c)
    if c.form == "update":
        hold(got["theta"], want["theta"], tol, what + " theta")
        hold(got["m"], want["m"], tol, what + " m")
        theta, m = inp.theta.to(d), inp.m.to(d)
        K.refine_update(theta, m, bwd(x, w, (c.H, c.W), c.s, c.s), IC.RATE, IC.ALPHA, False)
        assert torch.equal(theta, got["theta"]) and torch.equal(m, got["m"]), what + ": the fused update differs from the unfused pair"
    else:
        hold(got["out"], want["out"], tol, what)
    if c.form in ("stats", "nstats"):
        part = got["part"]
        assert torch.isfinite(part[:rows]).all() and torch.isnan(part[rows:]).all(), what + ": partial rows"
        sums = part[:rows].double().sum(0).cpu()
        hold(sums[0], want["sum"], tol, what + " column sums")
        hold(sums[1], want["sumsq"], tol, what + " second column sums")
    if c.form == "signs":
        bits = unpack_signs(got["signs"], P, N)
        assert torch.equal(bits, want["signs"].reshape(P, N)), what + f": {int((bits != want['signs'].reshape(P, N)).sum())} sign bits differ"
    again = run()
    assert again["plan"] == got["plan"]
    for key in got:
        if key != "plan":
            assert torch.equal(again[key].view(torch.int32), got[key].view(torch.int32)), what + f": the second run's {key} differs"
