"""Tensor-level wrappers over the nearest-neighbour entry points of the C ABI (csrc/knn.hip; include/cgs_hip.h),
in the launch / scratch / check pattern of kernels.py, whose pieces they use.  They live beside kernels.py, not in it: what kernels.py
hands to the C ABI is pinned call by call by tests/golden/abi_trace.json, and these calls are pinned by tests/test_gpu_knn.py instead.

Every op evaluates D2(j, i) = sum_k (double(q_jk) - double(r_ik))^2 in double on the device and never stores the matrix."""
import ctypes
import operator

import torch

from . import lib as L
from .kernels import _chk, _ptr, _state_call

MAX_D, MAX_K = 2048, 8


def plan(m, n, d):
    """The launch plan of an m-query, n-reference, d-wide call (cgs_knn_plan; host only): {"query_tiles", "ref_tiles", "tiles_per_split",
    "splits"}, or None where the library refuses the shape."""
    out = (ctypes.c_int * 4)()
    if not L.load().cgs_knn_plan(int(m), int(n), int(d), out):
        return None
    return dict(zip(("query_tiles", "ref_tiles", "tiles_per_split", "splits"), (int(v) for v in out)))


def _pool(t, who, name, d=None, device=None):
    _chk(t, f"{who}: {name}")
    if t.dim() != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= MAX_D or (d is not None and t.shape[1] != d) or \
            (device is not None and t.device != device):
        raise L.CgsError(f"{who}: {name} must be [rows >= 1, {d if d is not None else f'1 <= d <= {MAX_D}'}] on {device or 'the GPU'}, "
                         f"got {tuple(t.shape)} on {t.device}")
    return t


def nn_min(qry, ref, exclude_self=False):
    """For each row j of ``qry`` ([m, d] device fp32) the smallest D2(j, i) over the rows of ``ref`` ([n, d]) and the lowest index that
    attains it.  ``exclude_self`` (needs n == m) leaves i == j out and returns D2(j, j) too.
    -> (d2 float64 [m], idx int32 [m], self_d2 float64 [m] or None), on the device; no candidate: d2 = +inf, idx = -1."""
    _pool(qry, "nn_min", "qry")
    m, d = qry.shape
    _pool(ref, "nn_min", "ref", d, qry.device)
    n = ref.shape[0]
    excl = 1 if exclude_self else 0
    if excl and n != m:
        raise L.CgsError(f"nn_min: exclude_self needs pools of one length, got {m} and {n}")
    out = torch.empty((1 + excl, m), dtype=torch.float64, device=qry.device)
    idx = torch.empty(m, dtype=torch.int32, device=qry.device)
    _state_call(qry.device, ("cgs_knn_ws_bytes", L.KNN_NN_MIN, m, n, d, 0), f"nn_min: unsupported shape (m={m}, n={n}, d={d})",
                "cgs_nn_min", _ptr(qry), m, _ptr(ref), n, d, excl, _ptr(out), _ptr(idx))
    return out[0], idx, (out[1] if excl else None)


def knn_radii(x, k, other=None, exclude_self=None):
    """For each row of ``x`` ([n, d] device fp32) the k-th smallest D2 to the rows of ``other`` ([n_other, d]), or, without ``other``, to
    the other rows of ``x`` (``exclude_self`` defaults to True there and must stay False with ``other``).  1 <= k <= 8; fewer than k
    candidates is an error.  -> float64 [n] on the device (SQUARED radii)."""
    _pool(x, "knn_radii", "x")
    n, d = x.shape
    try:
        k = operator.index(k)
    except TypeError:
        raise L.CgsError("knn_radii: k must be an integer") from None
    if not 1 <= k <= MAX_K:
        raise L.CgsError(f"knn_radii: k = {k} outside 1..{MAX_K}")
    if other is not None:
        _pool(other, "knn_radii", "other", d, x.device)
    excl = int(other is None) if exclude_self is None else int(bool(exclude_self))
    if excl and other is not None:
        raise L.CgsError("knn_radii: exclude_self is for a pool against itself (other=None)")
    n_ref = n if other is None else other.shape[0]
    if n_ref - excl < k:
        raise L.CgsError(f"knn_radii: {n_ref - excl} candidates per row are fewer than k = {k}")
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    _state_call(x.device, ("cgs_knn_ws_bytes", L.KNN_RADII, n, n_ref, d, k), f"knn_radii: unsupported shape (n={n}, n_other={n_ref}, d={d}, k={k})",
                "cgs_knn_radii", _ptr(x), n, d, k, excl, _ptr(other), 0 if other is None else n_ref, _ptr(out))
    return out


def ball_count(qry, ref, ref_r2):
    """For each row j of ``qry`` ([m, d] device fp32) the number of rows i of ``ref`` ([n, d]) with D2(j, i) <= ref_r2[i] (float64 [n] on
    the device).  -> int32 [m] on the device."""
    _pool(qry, "ball_count", "qry")
    m, d = qry.shape
    _pool(ref, "ball_count", "ref", d, qry.device)
    n = ref.shape[0]
    if not (isinstance(ref_r2, torch.Tensor) and ref_r2.is_cuda and ref_r2.dtype == torch.float64 and ref_r2.is_contiguous()
            and tuple(ref_r2.shape) == (n,) and ref_r2.device == qry.device):
        raise L.CgsError(f"ball_count: ref_r2 must be a contiguous float64 [{n}] tensor on {qry.device}")
    out = torch.empty(m, dtype=torch.int32, device=qry.device)
    _state_call(qry.device, ("cgs_knn_ws_bytes", L.KNN_BALL_COUNT, m, n, d, 0), f"ball_count: unsupported shape (m={m}, n={n}, d={d})",
                "cgs_ball_count", _ptr(qry), m, _ptr(ref), n, d, _ptr(ref_r2), _ptr(out))
    return out
