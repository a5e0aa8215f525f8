"""csrc/frechet.hip on the MI355X: the float64 product against numpy float64 at its derived bound, the distance against the float64
statement of tests/frechet_cases.py at bars fixed from the CPU oracle recorded there, and metrics.frechet_device end to end.

Product: every entry within 2 gamma_{d+1} (|alpha| sum_k |a_ik b_kj| + |diag|) of numpy, gamma_m = m u / (1 - m u), u = 2^-53 -- the bound of
a length-d double inner product in any order plus the one rounding of the alpha / diag step (same factor 2: the
reference carries an error of the same kind).
Distance: |fd_dev - fd_statement| / e_norm <= max(4 ORACLE_A, d 2^-52) on class A, 4 ORACLE_B on class B (frechet_cases.bar): the device
runs the transcription's arithmetic in another summation order, 4 is the project's margin of GPU over CPU oracle.
Worst measured ratios to the bars: product 0.11 (d = 17); distance class A 0.113 (d16), class B 0.251 (same_63);
the device stays within 1.5e-15 (A) / 9e-14 (B) of e_norm of the transcription, with its iteration counts except on n64_d130_small (23, not 25)."""
import ctypes

import numpy as np
import pytest
import torch

import frechet_cases as FC

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MM_SIZES = [1, 15, 16, 17, 63, 64, 65, 130, 512]


def _dev():
    return torch.device("cuda:0")


def _gamma(m):
    return m * U / (1.0 - m * U)


@pytest.mark.parametrize("d", MM_SIZES)
def test_f64_matmul_meets_the_derived_bound_reads_nothing_past_d_and_reruns_bit_equal(d):
    """General non-symmetric operands with entries of both signs and four decades of magnitude.  The operands are the leading d x d
    doubles of NaN-filled buffers with NaN behind them: a read past row or column d - 1 that reached a product would poison an entry."""
    from cgs_amd import kernels as K
    rs = np.random.RandomState(100 + d)
    a = rs.randn(d, d) * 10.0 ** rs.uniform(-2, 2, (d, d))
    b = rs.randn(d, d) * 10.0 ** rs.uniform(-2, 2, (d, d))
    alpha, diag = -0.37, 2.5
    ref = alpha * a.dot(b) + diag * np.eye(d)
    bound = 2.0 * _gamma(d + 1) * (abs(alpha) * np.abs(a).dot(np.abs(b)) + abs(diag) * np.eye(d))

    def padded(m):
        buf = torch.full((d * d + 4096,), float("nan"), dtype=torch.float64, device=_dev())
        buf[:d * d] = torch.from_numpy(m).to(_dev()).reshape(-1)
        return buf, buf[:d * d].view(d, d)
    abuf, ad = padded(a)
    bbuf, bd = padded(b)
    obuf = torch.full((d * d + 4096,), -7.0, dtype=torch.float64, device=_dev())
    out = K.f64_matmul(ad, bd, out=obuf[:d * d].view(d, d), alpha=alpha, diag=diag)
    h = out.cpu().numpy()
    assert np.isfinite(h).all()
    ratio = float((np.abs(h - ref) / np.maximum(bound, 1e-300)).max())
    print(f"\n[f64_matmul d={d}] worst |delta| / bound: {ratio:.3g} (bar 1, the factor 2 is in the bound)")
    assert ratio <= 1.0
    assert bool((obuf[d * d:] == -7.0).all())                       # nothing written behind the result
    out2 = K.f64_matmul(ad, bd, alpha=alpha, diag=diag)
    assert torch.equal(out, out2)
    plain = K.f64_matmul(ad, bd)                                     # the defaults: alpha = 1, diag = 0
    assert float((np.abs(plain.cpu().numpy() - a.dot(b)) / np.maximum(2.0 * _gamma(d + 1) * np.abs(a).dot(np.abs(b)), 1e-300)).max()) <= 1.0
    with pytest.raises(Exception):
        K.f64_matmul(ad, bd, out=ad)
    with pytest.raises(Exception):
        K.f64_matmul(ad.float(), bd)


def _upload(st):
    dev = _dev()
    return (torch.from_numpy(np.array(st["sum"])).to(dev), torch.from_numpy(np.array(st["gram"])).to(dev),
            torch.from_numpy(np.array(st["shift"]).astype(np.float32)).to(dev), int(st["n"]))


def _run_raw(name, fill):
    """The entry point on a workspace of exactly cgs_frechet_ws_bytes(d) with a canary tail, prefilled with ``fill``."""
    from cgs_amd import lib as L
    sr, sf = FC.states(name)
    d = sr["shift"].shape[0]
    need = int(L.load().cgs_frechet_ws_bytes(d))
    assert need % 8 == 0 and need > 0
    tail = 1024
    ws = torch.full((need // 8 + tail,), fill, dtype=torch.float64, device=_dev())
    ws[need // 8:] = 12345.0
    out = torch.full((8 + 8,), -1.0, dtype=torch.float64, device=_dev())
    s_r, g_r, c_r, n_r = _upload(sr)
    s_f, g_f, c_f, n_f = _upload(sf)
    L.call("cgs_frechet_from_moments", s_r.data_ptr(), g_r.data_ptr(), c_r.data_ptr(), n_r, s_f.data_ptr(), g_f.data_ptr(), c_f.data_ptr(), n_f,
           d, 1, FC.MAX_ITERS, out.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((ws[need // 8:] == 12345.0).all()), "the workspace was written past cgs_frechet_ws_bytes(d)"
    assert bool((out[8:] == -1.0).all())
    return out[:8].cpu().numpy()


@pytest.mark.parametrize("name", list(FC.CASES))
def test_distance_meets_the_bar_of_its_class_is_finite_and_reruns_bit_equal(name):
    ref, tr = FC.reference(name)
    cls = FC.CASES[name][0]
    h = _run_raw(name, 0.0)
    assert np.isfinite(h).all(), h
    err = abs(h[0] - ref["fd"]) / ref["e_norm"]
    vs_tr = abs(h[0] - tr["fd"]) / ref["e_norm"]
    print(f"\n[frechet {name} ({cls})] fd {h[0]:.12g} (statement {ref['fd']:.12g}); error {err:.3g} of e_norm = {err / FC.bar(name):.3g} of the bar "
          f"{FC.bar(name):.3g}; against the transcription {vs_tr:.3g}; iterations {int(h[5])} / {int(h[6])} (transcription {tr['iters_r']} / "
          f"{tr['iters_m']}), status {int(h[7])} ({tr['status']})")
    assert err <= FC.bar(name)
    if cls == "A":
        assert int(h[7]) == 0
    assert int(h[7]) in (0, 1, 2)
    assert abs(int(h[5]) - tr["iters_r"]) <= 2 and abs(int(h[6]) - tr["iters_m"]) <= 2
    for i, key in ((1, "dmu2"), (2, "tr_r"), (3, "tr_f")):           # plain sums of d terms
        assert abs(h[i] - ref[key]) <= 4.0 * _gamma(len(FC.states(name)[0]["shift"]) + 4) * max(ref["e_norm"], 1e-300), key
    assert abs(h[4] - ref["tr_root"]) / ref["e_norm"] <= FC.bar(name)
    h2 = _run_raw(name, float("nan"))                                # a NaN-filled workspace does not leak; the rerun is bit-equal
    assert np.array_equal(h, h2)


def test_end_to_end_pools_in_three_batches_and_a_state_through_from_state():
    """d = 130, n = 1000 per pool, three unequal batches each through PoolMoments.update: frechet_device against frechet_distance on the
    same features at the class-A bar; the same through host states and from_state: the same bits."""
    from cgs_amd.metrics import PoolMoments, frechet_device, frechet_distance
    d, n = 130, 1000
    xr, xf = FC.cloud(71, n, d, 1.0, 3.0), FC.cloud(72, n, d, 1.3, 2.5)
    pools = []
    for x in (xr, xf):
        pm = PoolMoments(d, _dev())
        for a, b in ((0, 300), (300, 333), (333, n)):
            pm.update(torch.from_numpy(x[a:b].copy()).to(_dev()))
        pools.append(pm)
    rec = frechet_device(*pools, details=True)
    fd = frechet_device(*pools)
    assert isinstance(fd, float) and fd == rec["fd"] and rec["status"] == 0
    host = frechet_distance(xr, xf)
    e_norm = rec["tr_r"] + rec["tr_f"] + rec["dmu2"]
    err = abs(fd - host) / e_norm
    bar = max(4.0 * FC.ORACLE_A, d * FC.U52)
    print(f"\n[frechet_device end to end] fd {fd:.12g}, host {host:.12g}: {err:.3g} of e_norm (bar {bar:.3g}); iterations {rec['iters_r']} / {rec['iters_m']}")
    assert err <= bar
    states = [pm.state() for pm in pools]
    again = frechet_device(PoolMoments.from_state(states[0], _dev()), states[1], details=True)      # one uploaded here, one inside
    assert again == rec
    with pytest.raises(ValueError):
        frechet_device(pools[0], PoolMoments(d + 1, _dev()).update(torch.zeros((4, d + 1), device=_dev())))
    with pytest.raises(ValueError):
        frechet_device(pools[0], PoolMoments(d, _dev()).update(torch.zeros((1, d), device=_dev())))     # n - ddof = 0
