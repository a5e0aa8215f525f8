"""The device Frechet distance without a device: the statement against today's host route, the numpy transcription of the device
algorithm over the whole case table (finite; its error against the statement per class is THE ORACLE recorded in frechet_cases.py), the
C ABI surface and every refusal of csrc/frechet.hip, and PoolMoments.from_state's refusal."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import frechet_cases as FC
from conftest import ROOT

NEW = ["cgs_f64_matmul", "cgs_frechet_ws_bytes", "cgs_frechet_from_moments"]


def _rel(a, ref):
    return abs(a["fd"] - ref["fd"]) / ref["e_norm"]


def test_statement_agrees_with_the_host_route_on_full_rank_pools():
    """Class A (d = 2048 left to the transcription test: sqrtm alone is a minute there): |statement - frechet_from_moments| / e_norm.
    Measured 0 .. 2.2e-15 (d65); the bar is 64 ulps, both are backward-stable decompositions of matrices of condition 1e4."""
    from cgs_amd.metrics import frechet_from_moments, moments_mean_cov
    worst = 0.0
    for name in FC.CLASS_A:
        if name == "d2048":
            continue
        sr, sf = FC.states(name)
        ref = FC.reference(name)[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host = frechet_from_moments(*moments_mean_cov(sr), *moments_mean_cov(sf))
        dev = abs(host - ref["fd"]) / ref["e_norm"]
        print(f"\n[frechet statement vs host route] {name}: {dev:.3g}")
        worst = max(worst, dev)
    assert worst <= 64 * FC.U52, worst


def test_transcription_is_finite_on_the_whole_table_and_its_error_is_the_recorded_oracle():
    worst = {"A": 0.0, "B": 0.0}
    for name, (cls, _) in FC.CASES.items():
        ref, tr = FC.reference(name)
        assert all(np.isfinite(v) for v in tr.values()), (name, tr)
        assert all(np.isfinite(v) for v in ref.values()), (name, ref)
        e = _rel(tr, ref)
        print(f"\n[frechet transcription] {name} ({cls}): error {e:.3g} of e_norm, iterations {tr['iters_r']} / {tr['iters_m']}, status {tr['status']}")
        worst[cls] = max(worst[cls], e)
        if cls == "A":
            assert tr["status"] == 0, name
        assert 0 <= tr["iters_r"] <= FC.MAX_ITERS and 0 <= tr["iters_m"] <= FC.MAX_ITERS
    print(f"\n[frechet oracle] measured A {worst['A']:.3g} (recorded {FC.ORACLE_A}), B {worst['B']:.3g} (recorded {FC.ORACLE_B})")
    assert worst["A"] <= 2.0 * FC.ORACLE_A and worst["B"] <= 2.0 * FC.ORACLE_B, worst


def test_degenerate_pools_have_their_closed_forms():
    """Both covariances zero: fd = |dmu|^2 exactly, no iteration.  One zero: fd = |dmu|^2 + Tr S_f.  Identical pools: 0 within the bar."""
    _, tr = FC.reference("both_flat")
    assert tr["tr_r"] == 0.0 and tr["tr_f"] == 0.0 and tr["tr_root"] == 0.0 and tr["fd"] == tr["dmu2"] and tr["iters_r"] == tr["iters_m"] == 0
    _, tr = FC.reference("one_flat")
    assert tr["tr_r"] == 0.0 and tr["tr_root"] == 0.0 and tr["fd"] == tr["dmu2"] + tr["tr_f"]
    for name in ("same_63", "same_130"):
        ref, tr = FC.reference(name)
        assert abs(tr["fd"]) <= FC.bar(name) * ref["e_norm"]


def test_header_bindings_and_library_agree_on_the_new_entry_points():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    l = lib.load()
    for name in NEW:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert len(lib.SIGNATURES["cgs_frechet_from_moments"][1]) == 15
    assert l.cgs_version() >= 116


def test_workspace_query():
    from cgs_amd import lib
    l = lib.load()
    for d in (1, 17, 512, 2048):
        assert int(l.cgs_frechet_ws_bytes(d)) == 8 * (32 + d + 6 * d * d)          # control block, row sums, six matrices
    for d in (0, -1, 2049):
        assert int(l.cgs_frechet_ws_bytes(d)) == 0


def test_every_refusal_comes_before_any_launch():
    """No device here: a call that got as far as a launch would not return these codes."""
    from cgs_amd import lib
    l = lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                   # a non-null, 8-byte aligned stand-in; never dereferenced on a refusal
    odd = ctypes.c_void_p(p.value + 4)

    def fr(d=16, n_r=10, n_f=10, ddof=1, iters=48, sum_r=p, gram_r=p, sum_f=p, gram_f=p, out=p, ws=p, ws_bytes=1 << 40):
        return l.cgs_frechet_from_moments(sum_r, gram_r, None, n_r, sum_f, gram_f, None, n_f, d, ddof, iters, out, ws, ws_bytes, None)

    for d in (0, -3, 2049):
        assert fr(d=d) == lib.EINVAL
        assert l.cgs_f64_matmul(p, p, odd, d, 1.0, 0.0, None) == lib.EINVAL
    assert fr(n_r=1) == lib.EINVAL and fr(n_f=1) == lib.EINVAL and fr(n_r=0, ddof=0) == lib.EINVAL and fr(n_f=5, ddof=5) == lib.EINVAL
    for k in ("sum_r", "gram_r", "sum_f", "gram_f", "out"):
        assert fr(**{k: None}) == lib.EINVAL, k
    assert fr(iters=0) == lib.EINVAL and fr(iters=65) == lib.EINVAL
    assert fr(ws=odd) == lib.EINVAL
    need = int(l.cgs_frechet_ws_bytes(16))
    assert fr(ws_bytes=need - 1) == lib.EWORKSPACE and fr(ws=None) == lib.EWORKSPACE
    assert b"workspace" in l.cgs_last_error()
    q = ctypes.c_void_p(p.value + 8)
    assert l.cgs_f64_matmul(None, p, q, 4, 1.0, 0.0, None) == lib.EINVAL
    assert l.cgs_f64_matmul(p, None, q, 4, 1.0, 0.0, None) == lib.EINVAL
    assert l.cgs_f64_matmul(p, q, None, 4, 1.0, 0.0, None) == lib.EINVAL
    assert l.cgs_f64_matmul(p, q, p, 4, 1.0, 0.0, None) == lib.EINVAL and l.cgs_f64_matmul(p, q, q, 4, 1.0, 0.0, None) == lib.EINVAL      # c aliases


def test_from_state_refuses_a_host_device_like_the_constructor_and_leaves_the_state_alone():
    from cgs_amd.metrics import PoolMoments, frechet_device
    assert callable(frechet_device)
    sr, _ = FC.states("d16")
    before = {k: np.array(v) for k, v in sr.items()}
    with pytest.raises(ValueError, match="GPU"):
        PoolMoments(16, "cpu")
    with pytest.raises(ValueError, match="GPU"):
        PoolMoments.from_state(sr, "cpu")
    for k, v in before.items():
        assert np.array_equal(np.asarray(sr[k]), v)
