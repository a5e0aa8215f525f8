"""Tensor-level wrappers over the C ABI (include/cgs_hip.h): torch CUDA(ROCm) tensors in, tensors out.

PyTorch is plumbing only here -- device memory (``torch.empty``), the current HIP stream, and
nothing else: every FLOP below runs in libcgs_hip.so.  Activations are NHWC fp32 contiguous; weight
layouts are the reference's (nsgan/ops.py:39,51,76).  Packed-weight workspaces are cached per
(weight storage, version, op): frozen weights are packed once.
"""
import ctypes
import math
import operator
import weakref

import numpy as np
import torch

from . import lib as L

LEAK = 0.2      # nsgan/ops.py:69
BN_EPS = 1e-5   # nsgan/ops.py:23


def _chk(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise L.CgsError(f"{name}: expected a contiguous fp32 tensor on the GPU, got "
                         f"{type(t).__name__} {getattr(t, 'dtype', None)} {getattr(t, 'device', None)}")
    return t


def _typed(t, who, name, dtype, shape, device=None):
    """The one typed-tensor check: a contiguous ``dtype`` tensor of exactly ``shape`` on the GPU (on ``device`` when given)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)
            and (device is None or t.device == device)):
        raise L.CgsError(f"{who}: {name} must be a contiguous {dtype} {tuple(shape)} tensor on {device or 'the GPU'}, got "
                         f"{type(t).__name__} {getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))} {getattr(t, 'device', None)}")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(out, like_or_shape, device=None, dtype=torch.float32):
    """``out`` if given, else a fresh tensor like a tensor / of a shape (on ``device``)."""
    if out is not None:
        return out
    if isinstance(like_or_shape, torch.Tensor):
        return torch.empty_like(like_or_shape)
    return torch.empty(like_or_shape, dtype=dtype, device=device)


def _stats(stats, shape, device):
    """The (mean, invstd) pair of a norm: the caller's, or fresh fp32 tensors of ``shape``."""
    if stats is not None:
        return stats
    return torch.empty(shape, dtype=torch.float32, device=device), torch.empty(shape, dtype=torch.float32, device=device)


# ---- optional per-kernel timing (bench.py): {name: [flops, [(ev_start, ev_end), ...], executed_flops, algorithmic_bytes]} or None.
# Events are recorded on the stream the kernel is launched on (torch's current stream).  Conv-family records are keyed by the
# kernel instantiation the dispatcher launched (cgs_last_kernel); the HBM-bound multi-kernel ops (batch norm passes, the
# momentum update) by their entry point.
PROFILE = None


PROFILE_BY_LAYER = False      # key the records by kernel + layer shape instead of kernel only


def _launch(prof, name, *args):
    """``L.call(name, *args)``; with ``PROFILE`` set, timed under the record ``prof()`` = (flops, algorithmic bytes, op, tag) describes:
    keyed by ``op``, or (op None) by the kernel the dispatcher launched, plus the layer ``tag`` under ``PROFILE_BY_LAYER``.  ``prof`` is
    a callable so that an unprofiled call formats no tag and sums no bytes."""
    if PROFILE is None:
        return L.call(name, *args)
    flops, nbytes, op, tag = prof()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.call(name, *args)
    e1.record()
    executed = flops
    if op is None:
        op = L.load().cgs_last_kernel().decode()                           # the instantiation the dispatcher actually launched
        executed = float(L.load().cgs_last_executed_flops()) or flops      # minus the skipped zero-padding taps
    rec = PROFILE.setdefault(op + " " + tag if PROFILE_BY_LAYER and tag else op, [0.0, [], 0.0, 0.0])
    rec[0] += flops
    rec[1].append((e0, e1))
    rec[2] += executed
    rec[3] += nbytes


def _nb(*tensors):
    """Algorithmic HBM bytes of a launch: every operand tensor once."""
    return 4.0 * sum(t.numel() for t in tensors if t is not None)


def same_out(size, stride):
    """nsgan/ops.py:28-29."""
    return int(math.ceil(float(size) / float(stride)))


# ---- contraction arithmetic of the implicit-GEMM layers (include/cgs_hip.h, cgs_set_contraction): "f32" = exact fp32 MFMA (default),
# "bx6" = opt-in split-bf16 MFMA for the big layers, "bx6_all" = the same for every eligible call (test coverage).  The library keeps
# the mode per host thread; this module mirrors the mode of the thread that drives it (one host thread per process here).
CONTRACTION = "f32"     # the mode this module last put in force (informational; the thread's real state is asked of the library)


def set_contraction(mode):
    """Switch the CALLING THREAD's contraction mode; returns the previous one.  The library keeps the mode per host thread
    (a second host thread starts in "f32" whatever another thread set), so the compare is against the thread's own state."""
    global CONTRACTION
    prev = L.get_contraction()
    if mode != prev:
        L.set_contraction(mode)
    CONTRACTION = mode
    return prev


class contraction:
    """``with contraction("bx6"): ...`` -- the mode for the block, the previous mode restored after it (generic ops.* calls,
    DShaper steps and other engines of the thread do not inherit an engine's opt-in)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = set_contraction(self.mode)
        return self

    def __exit__(self, *exc):
        set_contraction(self.prev)
        return False


class _WsCache:
    """Packed-weight workspaces, keyed by the weight tensor (identity + version), the op, the call geometry, the HIP
    stream AND the kernel family the library will run (``cgs_conv_family``): every family keeps its own packed layout,
    and which one serves a call depends on the fused epilogue too, so the family is part of the key -- a workspace is
    only ever reported as pre-packed to the family that packed it."""

    def __init__(self):
        self._d = {}
        self._family = {}
        self.epoch = 0        # bumped by invalidate(): engines compare it with the epoch their packed copies / folded affines belong to
        self.clears = 0       # bumped by clear()
        self.record = None    # a list: every weight tensor asked for is appended as a weak reference (the generic path's hipGraph capture
                              # learns which weights its recorded program reads, sampling/collaborator.py::_GenericGraph)

    def plan(self, op, B, H, W, cin, ho, wo, cout, kh, kw, sh, sw, epilogue):
        """(kernel family, workspace bytes) of a call; asked of the library once per distinct call signature."""
        # (the family depends on the calling thread's contraction mode: asked of the library itself, so a caller that switched it
        # through lib.set_contraction / the C ABI directly is keyed correctly too)
        key = (op, B, H, W, cin, ho, wo, cout, kh, kw, sh, sw, epilogue, int(L.load().cgs_get_contraction()))
        hit = self._family.get(key)
        if hit is None:
            nbytes = max(L.conv_ws_bytes_for(op, B, H, W, cin, cout, kh, kw, sh, sw), 16)
            f = int(L.load().cgs_conv_family(op, B, H, W, cin, ho, wo, cout, kh, kw, sh, sw, epilogue, nbytes))
            if f < 0:
                raise L.CgsError(f"cgs_conv_family failed ({f}): {L.load().cgs_last_error().decode()}")
            hit = self._family[key] = (f, nbytes)
        return hit

    def get(self, w, op, kh, kw, sh, sw, cin, cout, bhw=(0, 0, 0), epilogue=0, out_hw=(0, 0), ptrs=()):
        """``bhw`` = (B, H, W) of the call: sizes the optional split-K slab area behind the packed weights.
        ``ptrs``: every device pointer of the call; if one is not 16-byte aligned the library may pick another family than
        the planned one, so such calls get a scratch workspace and always re-pack."""
        fam, nbytes = self.plan(op, bhw[0], bhw[1], bhw[2], cin, out_hw[0], out_hw[1], cout, kh, kw, sh, sw, epilogue)
        if self.record is not None:
            self.record.append(weakref.ref(w))
        aligned = not any(p is not None and (p & 15) for p in ptrs)
        if not aligned:
            fam = -1
        # one packed copy per HIP stream: the pack kernel is ordered only with later work of the stream that ran it
        key = (w.data_ptr(), op, kh, kw, sh, sw, cin, cout, w.device.index, bhw, fam, torch.cuda.current_stream(w.device).cuda_stream)
        hit = self._d.get(key)
        if hit is not None and hit[0]() is w:
            if hit[1] == w._version and aligned:
                return hit[2], 1
            self._d[key] = (hit[0], w._version, hit[2])      # stale: re-pack into the SAME buffer (hipGraphs keep its address)
            return hit[2], 0
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        if len(self._d) > 512:
            # only entries whose weight tensor is gone: a captured hipGraph holds the raw address of its workspaces
            # (ws_prepacked = 1), so an entry of a live weight is never dropped behind an engine's back
            for k in [k for k, v in self._d.items() if v[0]() is None]:
                del self._d[k]
        self._d[key] = (weakref.ref(w), w._version, ws)
        return ws, 0

    def invalidate(self):
        """Weights were updated in place by a kernel torch does not see (the Adam step, a checkpoint restore): every packed
        copy is stale.  Eager calls re-pack on their next use; every RefineEngine notices the new epoch at its next call and
        re-folds its inference-bn affines and re-packs the workspaces its captured hipGraphs read (engine._resync)."""
        for key, (ref, _, ws) in list(self._d.items()):
            self._d[key] = (ref, -1, ws)
        self.epoch += 1

    def clear(self):
        self._d.clear()
        self.clears += 1      # (the buffers a captured generic-path hipGraph points into are gone: it compares this counter)


WS = _WsCache()


class _Scratch:
    """Scratch buffers of one kind, one per (caller's key, device, HIP stream): a kernel's scratch is ordered only with the work of the
    stream it ran on.  A buffer holds ``max(nbytes, floor) // itemsize + pad`` elements.  Asked with a byte count it grows: a larger
    request replaces the buffer.  Asked with a callable (a size query, made only when the key has no buffer yet) it never does: the
    norm kernels leave sums there that ``*_param_grads`` reads in a later call, and captured hipGraphs hold the address."""

    def __init__(self, dtype=torch.float32, pad=0, floor=0):
        self._d = {}
        self.dtype, self.itemsize, self.pad, self.floor = dtype, torch.empty(0, dtype=dtype).element_size(), pad, floor

    def get(self, nbytes, device, key=()):
        key = (*key, device.index, torch.cuda.current_stream(device).cuda_stream)
        ws = self._d.get(key)
        if callable(nbytes):
            if ws is not None:
                return ws
            nbytes = nbytes()
        elif ws is not None and ws.numel() * self.itemsize >= nbytes:
            return ws
        ws = self._d[key] = torch.empty(max(nbytes, self.floor) // self.itemsize + self.pad, dtype=self.dtype, device=device)
        return ws

    def values(self):
        return self._d.values()


_bn_ws, _in_ws = _Scratch(), _Scratch(pad=4)                         # keyed (C,) and (B, HW, C): fixed once made
_wgrad_ws, _mom_ws = _Scratch(pad=4, floor=16), _Scratch(torch.float64, pad=1, floor=8)      # one per stream, grow-only


def _bn_workspace(M, C, device):
    return _bn_ws.get(lambda: L.bn_ws_bytes(M, C), device, (C,))


def _in_workspace(B, HW, C, device):
    return _in_ws.get(lambda: int(L.load().cgs_instnorm_ws_bytes(B, HW, C)), device, (B, HW, C))


# ----------------------------------------------------------------------------- conv family
# op -> (tag of the profile record, its arrow, is the (Ho, Wo) pair part of the entry points' geometry, {form: entry point})
_CONV = {
    L.CONV_FWD: ("conv_fwd", "->", False, {"plain": "cgs_conv2d_nhwc_fwd", "stats": "cgs_conv2d_nhwc_fwd_stats"}),
    L.CONV_BWD_DATA: ("conv_bwd", "<-", False, {"plain": "cgs_conv2d_nhwc_bwd_data", "nstats": "cgs_conv2d_nhwc_bwd_data_nstats",
                                                "update": "cgs_conv2d_nhwc_bwd_data_update"}),
    L.DECONV_FWD: ("deconv_fwd", "->", True, {"plain": "cgs_deconv2d_nhwc_fwd", "stats": "cgs_deconv2d_nhwc_fwd_stats",
                                              "signs": "cgs_deconv2d_nhwc_fwd_signs"}),
    L.DECONV_BWD_DATA: ("deconv_bwd", "<-", True, {"plain": "cgs_deconv2d_nhwc_bwd_data", "nstats": "cgs_deconv2d_nhwc_bwd_data_nstats",
                                                   "signs": "cgs_deconv2d_nhwc_bwd_data_signs", "update": "cgs_deconv2d_nhwc_bwd_data_update"}),
}


def _conv_call(op, form, bufs, w, geom, mid, ptrs, traffic, epilogue=L.EPI_NONE, part=None):
    """One launch of the conv family, the Python side of ``conv_entry`` (csrc/api.hip): every entry point takes its tensors ``bufs``,
    the geometry (``geom`` = (B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw); the conv ops' entry points and workspace plan go without
    Ho, Wo), the form's own arguments ``mid``, the packed-weight workspace, the partial-row buffer ``part`` of a statistics form, the
    stream.  ``ptrs``: the device pointers ``WS.get`` checks for alignment; ``traffic()``: the algorithmic bytes of the record."""
    B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw = geom
    what, arrow, with_out_hw, entries = _CONV[op]
    ws, pre = WS.get(w, op, kh, kw, sh, sw, Cin, Cout, (B, H, W), epilogue, (Ho, Wo) if with_out_hw else (0, 0), ptrs=ptrs)
    mh, mw = (H, W) if with_out_hw else (Ho, Wo)                      # the grid the contraction runs over: the strided side
    _launch(lambda: (2.0 * B * mh * mw * Cin * Cout * kh * kw, traffic(), None, f"{what} {H}x{W} {Cin}{arrow}{Cout}"),
            entries[form], *bufs, *(geom if with_out_hw else (B, H, W, Cin, Cout, kh, kw, sh, sw)), *mid, _ptr(ws), ws.numel() * 4, pre,
            *(() if part is None else (_ptr(part), part.numel() * 4)), _stream())


def _conv_fwd(op, x, w, bias, y, geom, epilogue, ep_a, ep_b, signs=None, part=None, part_ptr=()):
    """The forward forms: plain / signs (fused epilogue, the mask behind it) and stats (no epilogue: the partial rows behind the workspace)."""
    mid = () if part is not None else (epilogue, _ptr(ep_a), _ptr(ep_b)) + (() if signs is None else (signs.data_ptr(),))
    _conv_call(op, "stats" if part is not None else "plain" if signs is None else "signs", (_ptr(x), _ptr(w), _ptr(bias), _ptr(y)), w, geom, mid,
               (_ptr(x), _ptr(bias), _ptr(y)) + (part_ptr or (_ptr(ep_a), _ptr(ep_b))), lambda: _nb(x, w, y), epilogue, part)
    return y


def _conv_bwd_data(op, who, dy, w, geom, out, epilogue, ep_a, ep_aux, ep_signs, nstat, update):
    """The backward-data forms: plain / signs (fused epilogue), nstats (the norm-backward sums too), update (the momentum step instead
    of the result; returns None)."""
    B, H, W, Cin = geom[:4]
    if update is not None:
        if epilogue != L.EPI_NONE or nstat is not None or ep_signs is not None or tuple(update.theta.shape) != (B, H, W, Cin) \
                or update.m.shape != update.theta.shape:
            raise L.CgsError(f"{who}: the fused update comes with no epilogue, on theta and m of the gradient's shape")
        # dy and w once, theta read and written, m written (and read from the second step on); the gradient itself never goes to memory
        _conv_call(op, "update", (_ptr(dy), _ptr(w), _ptr(update.theta), _ptr(update.m)), w, geom, update.args(),
                   (_ptr(dy), _ptr(update.theta), _ptr(update.m)),
                   lambda: _nb(dy, w, update.theta, update.theta, update.m) + (0.0 if update.first else _nb(update.m)))
        return None
    if nstat is not None and (epilogue != L.EPI_NONE or ep_signs is not None):
        raise L.CgsError(f"{who}: norm-backward statistics come with no epilogue")
    dx = _out(out, (B, H, W, Cin), dy.device)
    if nstat is not None:
        form, mid = "nstats", nstat.args()
    elif ep_signs is not None:
        form, mid = "signs", (epilogue, _ptr(ep_a), ep_signs.data_ptr())
    else:
        form, mid = "plain", (epilogue, _ptr(ep_a), _ptr(ep_aux))
    _conv_call(op, form, (_ptr(dy), _ptr(w), _ptr(dx)), w, geom, mid, (_ptr(dy), _ptr(dx), _ptr(ep_a), _ptr(ep_aux)),
               lambda: _nb(dy, w, dx, ep_aux if ep_signs is None else ep_signs, nstat.x if nstat is not None else None), epilogue,
               nstat.part if nstat is not None else None)
    return dx


def conv2d_fwd(x, w, bias, sh=2, sw=2, epilogue=L.EPI_NONE, ep_a=None, ep_b=None, out=None):
    """tf.nn.conv2d 'SAME' + bias (+ fused epilogue).  nsgan/ops.py:41-44."""
    _chk(x, "x"); _chk(w, "w")
    B, H, W, Cin = x.shape
    kh, kw, Cin2, Cout = w.shape
    if Cin2 != Cin:
        raise L.CgsError(f"conv2d: weight Cin {Cin2} != input channels {Cin}")
    y = _out(out, (B, same_out(H, sh), same_out(W, sw), Cout), x.device)
    return _conv_fwd(L.CONV_FWD, x, w, bias, y, (B, H, W, Cin, y.shape[1], y.shape[2], Cout, kh, kw, sh, sw), epilogue, ep_a, ep_b)


def conv_stat_partials(x_shape, w_shape, sh=2, sw=2):
    """Partial rows G that ``conv2d_fwd_stats`` writes for this call (0: the fused statistics are not available for it)."""
    B, H, W, Cin = x_shape
    kh, kw, _, Cout = w_shape
    _, nbytes = WS.plan(L.CONV_FWD, B, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw, L.EPI_NONE)
    return int(L.load().cgs_conv_stat_partials(B, H, W, Cin, Cout, kh, kw, sh, sw, nbytes))


def conv_stat_layout(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, group_images):
    """Where the partial rows of every group of ``group_images`` consecutive images lie in the buffer ``conv2d_fwd_stats`` /
    ``deconv2d_fwd(part=...)`` fill: (rows_total, rows_per_seg, nseg, seg_stride), or None when the fused statistics are not
    available for the call (include/cgs_hip.h, cgs_conv_stat_layout)."""
    _, nbytes = WS.plan(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, L.EPI_NONE)
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rows = int(L.load().cgs_conv_stat_layout(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, int(group_images), nbytes,
                                             ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c)))
    return (rows, a.value, b.value, c.value) if rows > 0 else None


def groupnorm_lrelu_fwd_from_partials(x, part, layout, groups, scale, offset, leak=1.0, eps=BN_EPS, out=None, stats=None):
    """Norm over ``groups`` groups of consecutive rows of x ([groups * M_group, C] flattened; instance norm: one group per sample)
    whose statistics the producing convolution left in ``part`` (``layout`` = conv_stat_layout(...) of that call)."""
    _chk(x, "x"); _chk(part, "part")
    C_ = x.shape[-1]
    Mg = x.numel() // (groups * C_)
    y = _out(out, x)
    mean, invstd = _stats(stats, (groups, C_), x.device)
    ws = _in_workspace(groups, Mg, C_, x.device)
    _launch(lambda: (0.0, _nb(x, y), "groupnorm_lrelu_fwd_from_partials", ""),
            "cgs_groupnorm_lrelu_fwd_from_partials", _ptr(x), _ptr(part), groups, layout[1], layout[2], layout[3], _ptr(scale), _ptr(offset),
            eps, leak, _ptr(y), _ptr(mean), _ptr(invstd), Mg, C_, _ptr(ws), ws.numel() * 4, _stream())
    return y, mean, invstd


def conv2d_fwd_stats(x, w, bias, part, sh=2, sw=2, out=None):
    """conv2d_fwd (no epilogue) that also leaves the per-block column sums / sums of squares of its output in ``part``
    [G, 2, Cout] for the batch norm that follows (``bn_train_lrelu_fwd_from_partials``)."""
    _chk(x, "x"); _chk(w, "w"); _chk(part, "part")
    B, H, W, Cin = x.shape
    kh, kw, Cin2, Cout = w.shape
    if Cin2 != Cin:
        raise L.CgsError(f"conv2d: weight Cin {Cin2} != input channels {Cin}")
    y = _out(out, (B, same_out(H, sh), same_out(W, sw), Cout), x.device)
    return _conv_fwd(L.CONV_FWD, x, w, bias, y, (B, H, W, Cin, y.shape[1], y.shape[2], Cout, kh, kw, sh, sw), L.EPI_NONE, None, None,
                     part=part, part_ptr=(_ptr(part),))


def bn_train_lrelu_fwd_from_partials(x, part, gamma, beta, leak=LEAK, eps=BN_EPS, out=None, stats=None):
    """bn_train_lrelu_fwd whose statistics pass is replaced by the partial sums of the producing conv."""
    _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    y = _out(out, x)
    mean, invstd = _stats(stats, C, x.device)
    ws = _bn_workspace(M, C, x.device)
    _launch(lambda: (0.0, _nb(x, y), "bn_train_lrelu_fwd_from_partials", ""),                          # read x, write y
            "cgs_bn_train_lrelu_fwd_from_partials", _ptr(x), _ptr(part), part.shape[0], _ptr(gamma), _ptr(beta), eps, leak, _ptr(y),
            _ptr(mean), _ptr(invstd), M, C, _ptr(ws), ws.numel() * 4, _stream())
    return y, mean, invstd


class NormBwdStats:
    """What a backward-data call needs to ALSO leave the two column sums of the norm (+ lrelu) whose output gradient it produces
    (include/cgs_hip.h, cgs_*_bwd_data_nstats): the norm's input ``x`` (same shape as the call's result), its saved ``mean`` / ``invstd``
    ([groups, C]), ``gamma`` / ``beta``, the lrelu ``leak``, the images per statistics group, and the partial-row buffer ``part``
    ([rows, 2, C]) with its ``layout`` = conv_stat_layout(<the *_BWD_DATA op>, ...).  ``norm_lrelu_bwd_from_partials`` consumes it."""
    __slots__ = ("x", "mean", "invstd", "gamma", "beta", "leak", "group_images", "part", "layout")

    def __init__(self, x, mean, invstd, gamma, beta, leak, group_images, part, layout):
        self.x, self.mean, self.invstd, self.gamma, self.beta = x, mean, invstd, gamma, beta
        self.leak, self.group_images, self.part, self.layout = float(leak), int(group_images), part, layout

    def args(self):
        return (_ptr(self.x), _ptr(self.mean), _ptr(self.invstd), _ptr(self.gamma), _ptr(self.beta), self.leak, self.group_images)


class FusedUpdate:
    """What a backward-data call needs to apply the refinement loop's momentum / sgd step INSTEAD of storing its result (include/cgs_hip.h,
    cgs_*_bwd_data_update): the result is the gradient w.r.t. ``theta``; ``theta`` and the momentum buffer ``m`` (its shape) are updated in
    place exactly as ``refine_update`` without a clip would.  Only where ``conv_update_form`` offers it for the call."""
    __slots__ = ("theta", "m", "rate", "alpha", "first")

    def __init__(self, theta, m, rate, alpha, first):
        self.theta, self.m, self.rate, self.alpha, self.first = _chk(theta, "theta"), _chk(m, "m"), float(rate), float(alpha), bool(first)

    def args(self):
        return (self.rate, self.alpha, 1 if self.first else 0)


UPDATE_FORMS = {0: None, 1: "epilogue", 2: "splitk", 3: "tail"}


def conv_update_form(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw):
    """Where the backward-data call ``op`` (CONV_BWD_DATA / DECONV_BWD_DATA; arguments as the entry point's) would apply a ``FusedUpdate``:
    ("epilogue" | "splitk" | "tail", row order 0 / 1 / 2 of the launch), or None when the library does not offer it for the call
    (include/cgs_hip.h, cgs_conv_update_form).  Answers for the workspace ``WS`` hands that call."""
    _, nbytes = WS.plan(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, L.EPI_NONE)
    order = ctypes.c_int(0)
    form = int(L.load().cgs_conv_update_form(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, nbytes, ctypes.addressof(order)))
    return (UPDATE_FORMS[form], order.value) if form > 0 else None


def conv2d_bwd_data(dy, w, in_hw, sh=2, sw=2, out=None, epilogue=L.EPI_NONE, ep_a=None, ep_aux=None, nstat=None, update=None):
    """Input gradient of conv2d_fwd (Conv2DBackpropInput; sampling/collaborator.py:31).
    ``epilogue`` = one of the *_BWD modes folds the activation gradient of the layer below in.
    ``nstat`` (a NormBwdStats; no epilogue): the result is the gradient at the output of a norm -- leave that norm's backward sums too.
    ``update`` (a FusedUpdate; no epilogue, no nstat): the gradient is not stored, the momentum step is applied instead; returns None."""
    _chk(dy, "dy"); _chk(w, "w")
    kh, kw, Cin, Cout = w.shape
    B, Ho, Wo, _ = dy.shape
    H, W = in_hw
    return _conv_bwd_data(L.CONV_BWD_DATA, "conv2d_bwd_data", dy, w, (B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw), out, epilogue, ep_a, ep_aux,
                          None, nstat, update)


def conv_signs_ok(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue):
    """Can this call leave (forward, relu / lrelu epilogue) or take (backward-data, relu' / lrelu' epilogue) a sign mask
    instead of the fp32 aux tensor?  (include/cgs_hip.h, "sign masks")"""
    _, nbytes = WS.plan(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue)
    return bool(L.load().cgs_conv_signs_ok(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, nbytes))


def deconv2d_fwd(x, w, bias, out_hw, sh=2, sw=2, epilogue=L.EPI_NONE, ep_a=None, ep_b=None, out=None, signs=None, part=None):
    """tf.nn.conv2d_transpose (default 'SAME') + bias (+ fused epilogue).  nsgan/ops.py:55,61-62.
    ``signs``: int32 [B*Ho*Wo*Cout/32] that receives the sign mask of the output (only where ``conv_signs_ok``).
    ``part``: [rows, 2, Cout] that receives the statistics partials of the output (no epilogue; rows = conv_stat_layout(...)[0])."""
    _chk(x, "x"); _chk(w, "w")
    B, H, W, Cin = x.shape
    kh, kw, Cout, Cin2 = w.shape
    if Cin2 != Cin:
        raise L.CgsError(f"deconv2d: weight Cin {Cin2} != input channels {Cin}")
    Ho, Wo = out_hw
    if part is not None and (epilogue != L.EPI_NONE or signs is not None):
        raise L.CgsError("deconv2d_fwd: the statistics partials are those of the plain output (no epilogue, no sign mask)")
    y = _out(out, (B, Ho, Wo, Cout), x.device)
    return _conv_fwd(L.DECONV_FWD, x, w, bias, y, (B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw), epilogue, ep_a, ep_b, signs, part)


def deconv2d_bwd_data(dy, w, in_hw, sh=2, sw=2, out=None, epilogue=L.EPI_NONE, ep_a=None, ep_aux=None, ep_signs=None, nstat=None, update=None):
    """Input gradient of deconv2d_fwd: a strided 'SAME' conv of dy with the deconv weights.
    ``ep_signs``: the sign mask of the saved activation instead of ``ep_aux`` (relu' / lrelu' epilogues, where ``conv_signs_ok``).
    ``nstat``, ``update``: as in conv2d_bwd_data."""
    _chk(dy, "dy"); _chk(w, "w")
    kh, kw, Cout, Cin = w.shape
    B, Ho, Wo, _ = dy.shape
    H, W = in_hw
    return _conv_bwd_data(L.DECONV_BWD_DATA, "deconv2d_bwd_data", dy, w, (B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw), out, epilogue, ep_a,
                          ep_aux, ep_signs, nstat, update)


def linear_fwd(x, w, bias, epilogue=L.EPI_NONE, out=None):
    """tf.matmul(x, Matrix) + bias.  nsgan/ops.py:81-83."""
    _chk(x, "x"); _chk(w, "w")
    B, K = x.shape
    K2, N = w.shape
    if K2 != K:
        raise L.CgsError(f"linear: Matrix rows {K2} != input features {K}")
    y = _out(out, (B, N), x.device)
    ws, pre = (None, 0) if N == 1 else WS.get(w, L.CONV_FWD, 1, 1, 1, 1, K, N, (B, 1, 1), epilogue, ptrs=(_ptr(x), _ptr(bias), _ptr(y)))
    _launch(lambda: (2.0 * B * K * N, _nb(x, w, y), "linear_out1_fwd" if N == 1 else None, "" if N == 1 else f"linear_fwd {K}->{N}"),
            "cgs_linear_fwd", _ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, K, N, epilogue, _ptr(ws), 0 if ws is None else ws.numel() * 4, pre, _stream())
    return y


def linear_bwd_data(dy, w, out=None):
    _chk(dy, "dy"); _chk(w, "w")
    B, N = dy.shape
    K = w.shape[0]
    dx = _out(out, (B, K), dy.device)
    ws, pre = (None, 0) if N == 1 else WS.get(w, L.CONV_BWD_DATA, 1, 1, 1, 1, K, N, (B, 1, 1), ptrs=(_ptr(dy), _ptr(dx)))
    _launch(lambda: (2.0 * B * K * N, _nb(dy, w, dx), "linear_out1_bwd" if N == 1 else None, "" if N == 1 else f"linear_bwd {K}<-{N}"),
            "cgs_linear_bwd_data", _ptr(dy), _ptr(w), _ptr(dx), B, K, N, _ptr(ws), 0 if ws is None else ws.numel() * 4, pre, _stream())
    return dx


# ----------------------------------------------------------------------------- batch norm / activations
def bn_train_lrelu_fwd(x, gamma, beta, leak=LEAK, eps=BN_EPS, out=None, stats=None):
    """Batch-statistics bn (+ lrelu; leak=1 -> plain bn).  Returns (y, mean, invstd).  nsgan/ops.py:19-26.
    ``stats`` = optional preallocated (mean, invstd)."""
    _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    y = _out(out, x)
    mean, invstd = _stats(stats, C, x.device)
    ws = _bn_workspace(M, C, x.device)
    _launch(lambda: (0.0, _nb(x, x, y), "bn_train_lrelu_fwd", ""),     # statistics pass + apply pass
            "cgs_bn_train_lrelu_fwd", _ptr(x), _ptr(gamma), _ptr(beta), eps, leak, _ptr(y), _ptr(mean), _ptr(invstd),
            M, C, _ptr(ws), ws.numel() * 4, _stream())
    return y, mean, invstd


def bn_train_lrelu_bwd_data(dy, x, gamma, beta, mean, invstd, leak=LEAK, out=None):
    _chk(dy, "dy"); _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    dx = _out(out, x)
    ws = _bn_workspace(M, C, x.device)
    _launch(lambda: (0.0, _nb(dy, x, dy, x, dx), "bn_train_lrelu_bwd_data", ""),     # sums pass (dy, x) + apply pass (dy, x -> dx)
            "cgs_bn_train_lrelu_bwd_data", _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), leak,
            _ptr(dx), M, C, _ptr(ws), ws.numel() * 4, _stream())
    return dx


# synchronised batch statistics: the reductions stop at per-channel sums (double) that the caller all-reduces over the ranks
def bn_sync_fwd_sums(x, sums):
    """sums[2, C] (float64, device) <- (sum x, sum x^2) over the local rows."""
    _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    ws = _bn_workspace(M, C, x.device)
    L.call("cgs_bn_sync_fwd_sums", _ptr(x), sums.data_ptr(), M, C, _ptr(ws), ws.numel() * 4, _stream())
    return sums


def bn_sync_fwd_apply(x, gamma, beta, sums, m_total, leak=LEAK, eps=BN_EPS, out=None, stats=None):
    _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    y = _out(out, x)
    mean, invstd = _stats(stats, C, x.device)
    ws = _bn_workspace(M, C, x.device)
    L.call("cgs_bn_sync_fwd_apply", _ptr(x), _ptr(gamma), _ptr(beta), eps, leak, sums.data_ptr(), int(m_total), _ptr(y),
           _ptr(mean), _ptr(invstd), M, C, _ptr(ws), ws.numel() * 4, _stream())
    return y, mean, invstd


def bn_sync_bwd_sums(dy, x, gamma, beta, mean, invstd, sums, leak=LEAK):
    _chk(dy, "dy"); _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    ws = _bn_workspace(M, C, x.device)
    L.call("cgs_bn_sync_bwd_sums", _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), leak,
           sums.data_ptr(), M, C, _ptr(ws), ws.numel() * 4, _stream())
    return sums


def bn_sync_bwd_apply(dy, x, gamma, beta, mean, invstd, sums, m_total, leak=LEAK, out=None):
    _chk(dy, "dy"); _chk(x, "x")
    C = x.shape[-1]
    M = x.numel() // C
    dx = _out(out, x)
    ws = _bn_workspace(M, C, x.device)
    L.call("cgs_bn_sync_bwd_apply", _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), leak,
           sums.data_ptr(), int(m_total), _ptr(dx), M, C, _ptr(ws), ws.numel() * 4, _stream())
    return dx


def instnorm_lrelu_fwd(x, scale, offset, leak=1.0, eps=BN_EPS, out=None, stats=None):
    """Instance norm over the H*W pixels of every (sample, channel) (+ lrelu; leak 0 = relu, 1 = none).
    x: [B,H,W,C].  Returns (y, mean[B,C], invstd[B,C])."""
    _chk(x, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    y = _out(out, x)
    mean, invstd = _stats(stats, (B, C), x.device)
    ws = _in_workspace(B, HW, C, x.device)
    _launch(lambda: (0.0, _nb(x, x, y), "instnorm_lrelu_fwd", ""),
            "cgs_instnorm_lrelu_fwd", _ptr(x), _ptr(scale), _ptr(offset), eps, leak, _ptr(y), _ptr(mean), _ptr(invstd), B, HW, C,
            _ptr(ws), ws.numel() * 4, _stream())
    return y, mean, invstd


def instnorm_lrelu_bwd_data(dy, x, scale, offset, mean, invstd, leak=1.0, out=None):
    _chk(dy, "dy"); _chk(x, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    dx = _out(out, x)
    ws = _in_workspace(B, HW, C, x.device)
    _launch(lambda: (0.0, _nb(dy, x, dy, x, dx), "instnorm_lrelu_bwd_data", ""),
            "cgs_instnorm_lrelu_bwd_data", _ptr(dy), _ptr(x), _ptr(scale), _ptr(offset), _ptr(mean), _ptr(invstd), leak, _ptr(dx),
            B, HW, C, _ptr(ws), ws.numel() * 4, _stream())
    return dx


def norm_lrelu_bwd_from_partials(dy, x, nstat, groups, out=None):
    """Backward-data of batch / instance norm (+ lrelu) from the column sums the producing backward-data call left in ``nstat.part``
    (cgs_norm_lrelu_bwd_from_partials): finalize + one pass over dy and x.  dy / x: [groups * M_group, ..., C] (groups = 1: batch norm)."""
    _chk(dy, "dy"); _chk(x, "x")
    C_ = x.shape[-1]
    Mg = x.numel() // (groups * C_)
    dx = _out(out, x)
    ws = _in_workspace(groups, Mg, C_, x.device) if groups > 1 else _bn_workspace(Mg, C_, x.device)
    lay = nstat.layout
    _launch(lambda: (0.0, _nb(dy, x, dx), "norm_lrelu_bwd_from_partials", ""),
            "cgs_norm_lrelu_bwd_from_partials", _ptr(dy), _ptr(x), _ptr(nstat.part), groups, lay[1], lay[2], lay[3], _ptr(nstat.gamma), _ptr(nstat.beta),
            _ptr(nstat.mean), _ptr(nstat.invstd), nstat.leak, _ptr(dx), Mg, C_, _ptr(ws), ws.numel() * 4, _stream())
    return dx


def add(a, b, out=None):
    _chk(a, "a"); _chk(b, "b")
    o = _out(out, a)
    L.call("cgs_add", _ptr(a), _ptr(b), _ptr(o), a.numel(), _stream())
    return o


def bn_fold(gamma, beta, moving_mean, moving_var, eps=BN_EPS, out=None):
    """Inference-mode bn as a per-channel affine (a, b).  nsgan/GAN.py:87,94.  ``out`` = (a, b) to refresh in place."""
    C = gamma.numel()
    a, b = _stats(out, C, gamma.device)
    L.call("cgs_bn_fold", _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var), eps, _ptr(a), _ptr(b), C, _stream())
    return a, b


def affine_relu_fwd(x, a, b, out=None):
    _chk(x, "x")
    C = x.shape[-1]
    y = _out(out, x)
    L.call("cgs_affine_relu_fwd", _ptr(x), _ptr(a), _ptr(b), _ptr(y), x.numel() // C, C, _stream())
    return y


def affine_relu_bwd(dy, y, a, out=None):
    _chk(dy, "dy"); _chk(y, "y")
    C = y.shape[-1]
    dx = _out(out, y)
    L.call("cgs_affine_relu_bwd", _ptr(dy), _ptr(y), _ptr(a), _ptr(dx), y.numel() // C, C, _stream())
    return dx


def affine_fwd(x, a, b, out=None):
    _chk(x, "x")
    C = x.shape[-1]
    y = _out(out, x)
    L.call("cgs_affine_fwd", _ptr(x), _ptr(a), _ptr(b), _ptr(y), x.numel() // C, C, _stream())
    return y


def affine_bwd(dy, a, out=None):
    _chk(dy, "dy")
    C = dy.shape[-1]
    dx = _out(out, dy)
    L.call("cgs_affine_bwd", _ptr(dy), _ptr(a), _ptr(dx), dy.numel() // C, C, _stream())
    return dx


def lrelu_fwd(x, leak=LEAK, out=None):
    _chk(x, "x")
    y = _out(out, x)
    L.call("cgs_lrelu_fwd", _ptr(x), leak, _ptr(y), x.numel(), _stream())
    return y


def lrelu_bwd(dy, y, leak=LEAK, out=None):
    _chk(dy, "dy"); _chk(y, "y")
    dx = _out(out, y)
    L.call("cgs_lrelu_bwd", _ptr(dy), _ptr(y), leak, _ptr(dx), y.numel(), _stream())
    return dx


def tanh_fwd(x, out=None):
    _chk(x, "x")
    y = _out(out, x)
    L.call("cgs_tanh_fwd", _ptr(x), _ptr(y), x.numel(), _stream())
    return y


def tanh_bwd(dy, y, out=None):
    _chk(dy, "dy"); _chk(y, "y")
    dx = _out(out, y)
    L.call("cgs_tanh_bwd", _ptr(dy), _ptr(y), _ptr(dx), y.numel(), _stream())
    return dx


# ----------------------------------------------------------------------------- refinement-loop scalars
def bce_ones_grad_rowmean(logits, dlogits=None, logit_mean=None):
    """d softplus(-l)/dl = sigmoid(l) - 1 and the per-sample mean logit (collaborator.py:31-37)."""
    _chk(logits, "logits")
    B = logits.shape[0]
    P = logits.numel() // B
    dl = _out(dlogits, logits)
    lm = _out(logit_mean, B, logits.device)
    L.call("cgs_bce_ones_grad_rowmean", _ptr(logits), _ptr(dl), _ptr(lm), B, P, _stream())
    return dl, lm


def bce_ones_fwd(logits, out=None):
    """softplus(-logits): sigmoid_cross_entropy_with_logits(labels=1), unreduced (nsgan/GAN.py:176-177)."""
    _chk(logits, "logits")
    o = _out(out, logits)
    L.call("cgs_bce_ones_fwd", _ptr(logits), _ptr(o), logits.numel(), _stream())
    return o


def bce_ones_bwd(dloss, logits, out=None):
    """dloss * (sigmoid(logits) - 1)."""
    _chk(dloss, "dloss"); _chk(logits, "logits")
    o = _out(out, logits)
    L.call("cgs_bce_ones_bwd", _ptr(dloss), _ptr(logits), _ptr(o), logits.numel(), _stream())
    return o


def sigmoid_rowmean(logits, out=None):
    """Per-sample discriminator score: the mean over a sample's logits of sigmoid(logit), [B, 1]   (fake_sigmoids, nsgan/GAN.py:154-155)."""
    _chk(logits, "logits")
    B = logits.shape[0]
    o = _out(out, (B, 1), logits.device)
    L.call("cgs_sigmoid_rowmean", _ptr(logits), _ptr(o), B, logits.numel() // B, _stream())
    return o


def clip(x, vmin, vmax, out=None):
    """tf.clip_by_value (sampling/collaborator.py:69-70)."""
    _chk(x, "x")
    o = _out(out, x)
    L.call("cgs_clip", _ptr(x), float(vmin), float(vmax), _ptr(o), x.numel(), _stream())
    return o


def refine_update(theta, m, g, rate, alpha, first, vmin=None, vmax=None):
    """In-place momentum / sgd step on theta (+ optional clip).  policy.py:27-37, collaborator.py:66-70."""
    use_clip = 1 if (vmin and vmax) else 0          # the reference's truthiness test (quirk Q5)
    _launch(lambda: (0.0, _nb(theta, theta, m, g) + (0.0 if first else _nb(m)), "refine_update", ""),
            "cgs_refine_update", _ptr(theta), _ptr(m), _ptr(g), rate, alpha, 1 if first else 0, use_clip,
            float(vmin or 0.0), float(vmax or 0.0), theta.numel(), _stream())


def refine_select(theta, logit, forced, step_index, best_theta, best_logit, best_step):
    """Row-wise best-sample select.  collaborator.py:76-83."""
    B = theta.shape[0]
    L.call("cgs_refine_select", _ptr(theta), _ptr(logit), _ptr(forced), step_index, _ptr(best_theta), _ptr(best_logit),
           _ptr(best_step), B, theta.numel() // B, _stream())


def refine_select2(rows, best_rows, theta, best_theta, logit, forced, step_index, best_logit, best_step, tickets=None):
    """refine_select_rows(rows) + refine_select(theta) with the two row copies in one launch; with ``tickets`` (int32 [B], zero: the call leaves
    it zero) the scalars too -- otherwise they follow in a second launch."""
    B = theta.shape[0]
    if tickets is not None and (tickets.dtype != torch.int32 or tickets.numel() < B or not tickets.is_contiguous() or tickets.device != theta.device):
        raise L.CgsError("refine_select2: tickets must be a contiguous int32 device tensor of at least B elements")
    L.call("cgs_refine_select2", _ptr(rows), _ptr(best_rows), rows.numel() // B, _ptr(theta), _ptr(best_theta), theta.numel() // B, _ptr(logit),
           _ptr(forced), step_index, _ptr(best_logit), _ptr(best_step), _ptr(tickets), B, _stream())


def linear_out1_bce(x, w, bias, logits, dlogits, logit_mean):
    """The one-logit head of D + the loss seed (linear_fwd(N = 1) then bce_ones_grad_rowmean) in one launch."""
    _chk(x, "x"); _chk(w, "w")
    B, K = x.shape
    _launch(lambda: (2.0 * B * K, _nb(x, w, logits), "linear_out1_fwd", ""),
            "cgs_linear_out1_bce", _ptr(x), _ptr(w), _ptr(bias), _ptr(logits), _ptr(dlogits), _ptr(logit_mean), B, K, _stream())
    return logits


def _loss_kind(kind, allowed):
    code = L.LOSSES.get(kind) if isinstance(kind, str) else kind
    if code not in [L.LOSSES[k] for k in allowed]:
        raise L.CgsError(f"loss {kind!r}: expected one of {allowed}")
    return code


class LadamState:
    """The ladam rule's per-sample state on the device (include/cgs_hip.h, cgs_ladam_seed): ``s_real`` [1] the mean score of real data the
    per-sample loss is measured against, ``loss_avg`` [B] its running average, ``gain`` [B] the step's per-sample factor.  ``s_real`` is read
    by the launch, so a captured program replays with whatever ``set_real`` wrote last."""

    def __init__(self, B, device):
        self.s_real = torch.zeros(1, dtype=torch.float32, device=device)
        self.loss_avg = torch.empty(B, dtype=torch.float32, device=device)
        self.gain = torch.empty(B, dtype=torch.float32, device=device)

    def set_real(self, value):
        """A float, or a device scalar (copied in stream order: no host synchronisation either way)."""
        if isinstance(value, torch.Tensor):
            self.s_real.copy_(value.reshape(1))
        else:
            self.s_real.fill_(float(value))

    def arg(self, first):
        return ctypes.byref(L.LadamSeed(_ptr(self.s_real), _ptr(self.loss_avg), _ptr(self.gain), 1 if first else 0))


def refine_loss_seed(logits, kind, dlogits=None, logit_mean=None, ladam=None, first=False):
    """d loss / d logit of the unreduced refinement loss ``kind`` ("bce": softplus(-l), "lsq": (l - 1)^2, "linear": -l) and the per-sample
    mean logit, which is that of ``bce_ones_grad_rowmean`` bit for bit.  ``ladam``: a ``LadamState`` this launch advances by one step."""
    _chk(logits, "logits")
    B = logits.shape[0]
    dl = _out(dlogits, logits)
    lm = _out(logit_mean, B, logits.device)
    L.call("cgs_refine_loss_seed", _ptr(logits), _loss_kind(kind, ("bce", "lsq", "linear")), _ptr(dl), _ptr(lm), B, logits.numel() // B,
           None if ladam is None else ladam.arg(first), _stream())
    return dl, lm


def linear_out1_seed(x, w, bias, logits, dlogits, logit_mean, kind, ladam=None, first=False):
    """``linear_out1_bce`` for any refinement loss: linear_fwd(N = 1) then ``refine_loss_seed`` in one launch."""
    _chk(x, "x"); _chk(w, "w")
    B, K = x.shape
    _launch(lambda: (2.0 * B * K, _nb(x, w, logits), "linear_out1_fwd", ""),
            "cgs_linear_out1_seed", _ptr(x), _ptr(w), _ptr(bias), _ptr(logits), _ptr(dlogits), _ptr(logit_mean), B, K,
            _loss_kind(kind, ("bce", "lsq", "linear")), None if ladam is None else ladam.arg(first), _stream())
    return logits


def ladam_gain(loss, loss_avg, gain, first):
    """The ladam rule's running loss and per-sample gain from a per-sample ``loss`` [B] on the device (policy.py:48-51,56)."""
    for t, name in ((loss, "loss"), (loss_avg, "loss_avg"), (gain, "gain")):
        _chk(t, name)
    B = loss.numel()
    if loss_avg.numel() != B or gain.numel() != B:
        raise L.CgsError("ladam_gain: loss, loss_avg and gain must have one size")
    L.call("cgs_ladam_gain", _ptr(loss), _ptr(loss_avg), _ptr(gain), 1 if first else 0, B, _stream())
    return gain


def refine_update_ladam(theta, m, v, g, gain, rate, first, vmin=None, vmax=None):
    """In-place ladam step on the map ``theta`` [B, ...] (+ optional clip) with the per-sample ``gain`` a seed launch left.  policy.py:39-59."""
    for t, name in ((theta, "theta"), (m, "m"), (v, "v"), (g, "g"), (gain, "gain")):
        _chk(t, name)
    B = theta.shape[0]
    if m.numel() != theta.numel() or v.numel() != theta.numel() or g.numel() != theta.numel() or gain.numel() < B:
        raise L.CgsError("refine_update_ladam: theta, m, v and g must have one size, gain at least B elements")
    use_clip = 1 if (vmin and vmax) else 0          # the reference's truthiness test (quirk Q5)
    _launch(lambda: (0.0, _nb(theta, theta, m, v, g) + (0.0 if first else _nb(m, v)), "refine_update_ladam", ""),
            "cgs_refine_update_ladam", _ptr(theta), _ptr(m), _ptr(v), _ptr(g), _ptr(gain), float(rate), 1 if first else 0, use_clip,
            float(vmin or 0.0), float(vmax or 0.0), B, theta.numel() // B, _stream())


def refine_select_rows(src, logit, forced, step_index, dst, best_logit):
    """Copy the rows of ``src`` whose sample is selected at this step into ``dst`` (predicate of refine_select;
    call before it, which updates best_logit)."""
    B = src.shape[0]
    L.call("cgs_refine_select_rows", _ptr(src), _ptr(logit), _ptr(forced), step_index, _ptr(dst), _ptr(best_logit),
           B, src.numel() // B, _stream())


# ----------------------------------------------------------------------------- D shaping step (weight gradients, Adam)
def conv2d_bwd_weight(x, dy, kh, kw, sh=2, sw=2, out=None, accumulate=False):
    """dw[kh,kw,Cin,Cout] (+)= weight gradient of conv2d_fwd (Conv2DBackpropFilter)."""
    _chk(x, "x"); _chk(dy, "dy")
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    dw = _out(out, (kh, kw, Cin, Cout), x.device)
    ws = _wgrad_ws.get(int(L.load().cgs_conv_wgrad_ws_bytes(B, H, W, Cin, Cout, kh, kw, sh, sw)), x.device)
    # (the weight-gradient GEMM multiplies the zero-padding taps too: issued = nominal flops; the slab reduce rides in the same record)
    _launch(lambda: (2.0 * B * dy.shape[1] * dy.shape[2] * Cout * kh * kw * Cin, _nb(x, dy, dw), "wgrad_kernel", ""),
            "cgs_conv2d_nhwc_bwd_weight", _ptr(x), _ptr(dy), _ptr(dw), B, H, W, Cin, Cout, kh, kw, sh, sw,
            1 if accumulate else 0, _ptr(ws), ws.numel() * 4, _stream())
    return dw


def conv_wgrad_cout1_ok(x_shape, kh, kw, sh, sw):
    """Does the one-output-channel weight gradient (conv2d_bwd_weight_cout1) take this call?  (the library's own answer: its workspace query)"""
    B, H, W, Cin = x_shape
    return int(L.load().cgs_conv_wgrad_cout1_ws_bytes(B, H, W, Cin, kh, kw, sh, sw)) > 0


def conv2d_bwd_weight_cout1(x, dy, kh, kw, sh=2, sw=2, out=None, accumulate=False):
    """dw[kh,kw,Cin,1] (+)= weight gradient of conv2d_fwd to ONE output channel over a deep reduction (Cin % 4 == 0,
    kh * kw * Cin >= 1024, sh == sw: the PatchGAN logit head); dy: [B,Ho,Wo,1].  Any other shape is an error: conv2d_bwd_weight serves it."""
    _chk(x, "x"); _chk(dy, "dy")
    B, H, W, Cin = x.shape
    if dy.shape[3] != 1:
        raise L.CgsError(f"conv2d_bwd_weight_cout1: dy has {dy.shape[3]} channels")
    dw = _out(out, (kh, kw, Cin, 1), x.device)
    ws = _wgrad_ws.get(int(L.load().cgs_conv_wgrad_cout1_ws_bytes(B, H, W, Cin, kh, kw, sh, sw)), x.device)
    _launch(lambda: (2.0 * B * dy.shape[1] * dy.shape[2] * kh * kw * Cin, _nb(x, dy, dw), "wgrad_cout1_kernel", ""),
            "cgs_conv2d_nhwc_bwd_weight_cout1", _ptr(x), _ptr(dy), _ptr(dw), B, H, W, Cin, kh, kw, sh, sw,
            1 if accumulate else 0, _ptr(ws), ws.numel() * 4, _stream())
    return dw


def deconv2d_bwd_weight(x, dy, kh, kw, sh=2, sw=2, out=None, accumulate=False):
    """dw[kh,kw,Cout,Cin] (+)= weight gradient of deconv2d_fwd(x, w) contracted with dy[B,Ho,Wo,Cout] (the generator's update)."""
    _chk(x, "x"); _chk(dy, "dy")
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    dw = _out(out, (kh, kw, Cout, Cin), x.device)
    ws = _wgrad_ws.get(int(L.load().cgs_deconv_wgrad_ws_bytes(B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw)), x.device)
    _launch(lambda: (2.0 * B * H * W * Cin * kh * kw * Cout, _nb(x, dy, dw), "wgrad_kernel", ""),
            "cgs_deconv2d_nhwc_bwd_weight", _ptr(x), _ptr(dy), _ptr(dw), B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw,
            1 if accumulate else 0, _ptr(ws), ws.numel() * 4, _stream())
    return dw


def linear_bwd_weight(x, dy, out=None, accumulate=False):
    """dw[in,out] (+)= x^T dy."""
    _chk(x, "x"); _chk(dy, "dy")
    B, K = x.shape
    N = dy.shape[1]
    dw = _out(out, (K, N), x.device)
    ws = _wgrad_ws.get(int(L.load().cgs_conv_wgrad_ws_bytes(B, 1, 1, K, N, 1, 1, 1, 1)), x.device)
    _launch(lambda: (2.0 * B * K * N, _nb(x, dy, dw), "wgrad_kernel", ""),
            "cgs_linear_bwd_weight", _ptr(x), _ptr(dy), _ptr(dw), B, K, N, 1 if accumulate else 0, _ptr(ws), ws.numel() * 4, _stream())
    return dw


def bias_grad(dy, out=None, accumulate=False):
    """db[C] (+)= sum of dy over every axis but the last."""
    _chk(dy, "dy")
    C = dy.shape[-1]
    M = dy.numel() // C
    db = _out(out, C, dy.device)
    if C % 4 != 0:                                   # the single-logit head: a B-element sum
        s = dy.reshape(M, C).sum(0)
        db.copy_(db + s if accumulate else s)
        return db
    ws = _bn_workspace(M, C, dy.device)
    L.call("cgs_bias_grad", _ptr(dy), _ptr(db), M, C, 1 if accumulate else 0, _ptr(ws), ws.numel() * 4, _stream())
    return db


def bn_train_param_grads(x, dgamma, dbeta, accumulate=False):
    """(dgamma, dbeta) (+)= from the statistics the bn_train_lrelu_bwd_data call JUST made on ``x`` left in its workspace."""
    C = x.shape[-1]
    M = x.numel() // C
    ws = _bn_workspace(M, C, x.device)
    L.call("cgs_bn_train_param_grads", _ptr(ws), M, C, _ptr(dgamma), _ptr(dbeta), 1 if accumulate else 0, _stream())


def instnorm_param_grads(x, dscale, doffset, accumulate=False):
    """(dscale, doffset) (+)= from the per-sample sums the instnorm_lrelu_bwd_data call JUST made on ``x`` (same stream, so the same
    workspace) left in its workspace; x: the norm's input [B,H,W,C]."""
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    ws = _in_workspace(B, HW, C, x.device)
    L.call("cgs_instnorm_param_grads", _ptr(ws), B, HW, C, _ptr(dscale), _ptr(doffset), 1 if accumulate else 0, _stream())


def bce_logits_grad(logits, target, scale, dlogits=None, loss=None):
    """dlogits = scale*(sigmoid(l) - target); loss[0] = scale * sum BCE(l, target)."""
    _chk(logits, "logits")
    dl = _out(dlogits, logits)
    L.call("cgs_bce_logits_grad", _ptr(logits), float(target), float(scale), _ptr(dl), _ptr(loss), logits.numel(), _stream())
    return dl


def gan_logits_grad(logits, kind, target, scale, dlogits=None, loss=None):
    """``bce_logits_grad`` for the GAN training loss ``kind``: "bce"; "lsq" (l - target)^2; "hinge" relu(1 - l) on real (target 1),
    relu(1 + l) on fake (target 0); "linear" -l (the generator's side of hinge).  dlogits = scale * d loss, loss[0] = scale * sum loss."""
    _chk(logits, "logits")
    dl = _out(dlogits, logits)
    L.call("cgs_gan_logits_grad", _ptr(logits), _loss_kind(kind, ("bce", "lsq", "linear", "hinge")), float(target), float(scale), _ptr(dl), _ptr(loss),
           logits.numel(), _stream())
    return dl


def gan_loss(logits, kind, target, dloss=None, out=None):
    """The loss ``kind`` of ``gan_logits_grad`` per logit, unreduced ("lsq", "hinge", "linear"); with ``dloss`` its input gradient
    dloss * d loss / d logit."""
    _chk(logits, "logits")
    if dloss is not None:
        _chk(dloss, "dloss")
    o = _out(out, logits)
    L.call("cgs_gan_loss", _ptr(logits), _loss_kind(kind, ("lsq", "linear", "hinge")), float(target), _ptr(dloss), _ptr(o), logits.numel(), _stream())
    return o


def adam_step(w, g, m, v, lr_t, beta1, beta2, eps):
    L.call("cgs_adam_step", _ptr(w), _ptr(g), _ptr(m), _ptr(v), float(lr_t), float(beta1), float(beta2), float(eps), w.numel(), _stream())


# ----------------------------------------------------------------------------- one Adam launch per optimizer, lr_t in device memory
ADAM_CHUNK = 2048       # elements per block of cgs_adam_multi (8 per thread): a 6.4 M-element weight is 3136 blocks, a bias one


def adam_chunk_plan(sizes, chunk=ADAM_CHUNK):
    """The block -> (slot, begin, count) map of ``cgs_adam_multi`` for slots of ``sizes`` elements: chunks of at most ``chunk`` elements,
    in slot order, none crossing a slot, every element in exactly one; a slot of 0 elements gets none.  len(result) is the grid size."""
    if chunk <= 0:
        raise ValueError(f"adam_chunk_plan: chunk={chunk}")
    plan = []
    for slot, n in enumerate(sizes):
        if n < 0:
            raise ValueError(f"adam_chunk_plan: slot {slot} has {n} elements")
        for begin in range(0, n, chunk):
            plan.append((slot, begin, min(chunk, n - begin)))
    return plan


class AdamTable:
    """The (w, g, m, v) slots of one optimizer as ``cgs_adam_multi`` reads them: the slot table, the chunk plan and the ``lr_t`` scalar, all in
    device memory and built once.  Holds the tensors, so the raw addresses in the table stay valid as long as the table lives."""

    def __init__(self, slots):
        self.slots = [tuple(s) for s in slots]
        if not self.slots:
            raise L.CgsError("AdamTable: no slots")
        dev = self.slots[0][0].device
        for i, (w, g, m, v) in enumerate(self.slots):
            for t, what in ((w, "w"), (g, "g"), (m, "m"), (v, "v")):
                _chk(t, f"AdamTable slot {i} {what}")
                if t.device != dev or t.numel() != w.numel():
                    raise L.CgsError(f"AdamTable slot {i}: {what} has {t.numel()} elements on {t.device}, w {w.numel()} on {dev}")
        table = np.zeros(len(self.slots), dtype=np.dtype([("w", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<u8")]))
        for i, (w, g, m, v) in enumerate(self.slots):
            table[i] = (w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel())
        chunks = adam_chunk_plan([s[0].numel() for s in self.slots])
        plan = np.zeros(len(chunks), dtype=np.dtype([("slot", "<i4"), ("count", "<u4"), ("begin", "<u8")]))
        for i, c in enumerate(chunks):
            plan[i] = (c[0], c[2], c[1])
        self.n_chunks = len(chunks)
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        self.plan = torch.from_numpy(plan.view(np.uint8).copy()).to(dev) if chunks else None
        self.lr_t = torch.zeros(1, dtype=torch.float32, device=dev)

    def step(self, lr_t, b1, b2, eps):
        """One Adam step of every slot.  ``lr_t`` reaches the device scalar by a stream-ordered fill (the value rides as that kernel's
        argument: nothing on the host has to outlive the call); the update launch itself has the same arguments every time.
        ``lr_t=None``: the update alone, at whatever the device scalar holds -- what a captured program records, its owner filling
        ``self.lr_t`` before every replay."""
        if lr_t is not None:
            self.lr_t.fill_(float(lr_t))
        L.call("cgs_adam_multi", _ptr(self.table), len(self.slots), _ptr(self.plan), self.n_chunks, _ptr(self.lr_t),
               float(b1), float(b2), float(eps), _stream())


def bn_moving_update(mean, invstd, moving_mean, moving_var, decay, eps=BN_EPS):
    """ops.bn's moving averages of one norm from its saved batch statistics, in place, in one launch."""
    _chk(mean, "mean"); _chk(invstd, "invstd"); _chk(moving_mean, "moving_mean"); _chk(moving_var, "moving_var")
    C = mean.numel()
    if invstd.numel() != C or moving_mean.numel() != C or moving_var.numel() != C:
        raise L.CgsError(f"bn_moving_update: {C} / {invstd.numel()} / {moving_mean.numel()} / {moving_var.numel()} channels")
    L.call("cgs_bn_moving_update", _ptr(mean), _ptr(invstd), _ptr(moving_mean), _ptr(moving_var), C, float(decay), float(eps), _stream())


# ----------------------------------------------------------------------------- pool statistics (csrc/moments.hip)
def _state_call(device, query, refusal, name, *args):
    """A launch that works in the stream's float64 scratch: under ``device``, ask ``query`` = (a ``*_ws_bytes`` entry, its arguments)
    for the size -- 0: the library does not serve the call, ``refusal`` says so; no query: the smallest area -- take the scratch and
    call ``name(*args, scratch, its bytes, stream)``."""
    with torch.cuda.device(device):
        need = int(getattr(L.load(), query[0])(*query[1:])) if query else 8
        if need == 0:
            raise L.CgsError(refusal)
        ws = _mom_ws.get(need, device)
        L.call(name, *args, _ptr(ws), ws.numel() * 8, _stream())


def pool_moments(x, sum, gram, shift=None, rows=None):
    """sum[d] += sum_i a_i, gram[d,d] += sum_i a_i a_i^T with a_i = double(x[r_i]) - double(shift), in double on the device.
    x: [n, d] contiguous fp32 on the GPU; sum / gram: float64 on the same device, updated in place; shift: [d] fp32 or None (= 0);
    rows: None (every row of x) or a HOST integer array of row indices into x (checked here: the kernel trusts them), any order, repeats
    allowed, empty = a no-op."""
    _chk(x, "x")
    if x.dim() != 2:
        raise L.CgsError(f"pool_moments: x must be [n, d], got {tuple(x.shape)}")
    n, d = x.shape
    _typed(sum, "pool_moments", "sum", torch.float64, (d,), x.device)
    _typed(gram, "pool_moments", "gram", torch.float64, (d, d), x.device)
    if shift is not None:
        _chk(shift, "shift")
        if tuple(shift.shape) != (d,) or shift.device != x.device:
            raise L.CgsError(f"pool_moments: shift must be [{d}] on {x.device}")
    m, rows_dev = n, None
    if rows is not None:
        r = np.asarray(rows)
        if r.ndim != 1 or (r.size and r.dtype.kind not in "iu"):
            raise L.CgsError("pool_moments: rows must be a 1-D host array of integers")
        m = int(r.size)
        if m == 0:
            return
        if int(r.min()) < 0 or int(r.max()) >= n:
            raise L.CgsError(f"pool_moments: row index outside [0, {n})")
        rows_dev = torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32)).to(x.device)
    if m == 0:
        return
    _state_call(x.device, ("cgs_pool_moments_ws_bytes", m, d), f"pool_moments: unsupported shape (m={m}, d={d}): 1 <= d <= 2048",
                "cgs_pool_moments_accumulate", _ptr(x), n, d, _ptr(rows_dev), m, _ptr(shift), _ptr(sum), _ptr(gram))


def spatial_mean(x, out=None):
    """[B, ..., C] -> [B, C]: the mean over every axis between the first and the last (a conv discriminator's feature map per sample)."""
    _chk(x, "x")
    B, C = x.shape[0], x.shape[-1]
    o = _out(out, (B, C), x.device)
    L.call("cgs_spatial_mean", _ptr(x), _ptr(o), B, x.numel() // (B * C), C, _stream())
    return o


# ----------------------------------------------------------------------------- the Frechet distance from two states (csrc/frechet.hip)
def f64_matmul(a, b, out=None, alpha=1.0, diag=0.0):
    """out = alpha * a @ b + diag * I for square float64 matrices on the GPU (d <= 2048), in double on the float64 MFMA; ``out`` must not
    be ``a`` or ``b``."""
    if not (isinstance(a, torch.Tensor) and a.dim() == 2 and a.shape[0] == a.shape[1]):
        raise L.CgsError("f64_matmul: a must be a square matrix")
    d = a.shape[0]
    _typed(a, "f64_matmul", "a", torch.float64, (d, d))
    _typed(b, "f64_matmul", "b", torch.float64, (d, d), a.device)
    o = _out(out, (d, d), a.device, torch.float64)
    _typed(o, "f64_matmul", "out", torch.float64, (d, d), a.device)
    with torch.cuda.device(a.device):
        L.call("cgs_f64_matmul", _ptr(a), _ptr(b), _ptr(o), d, float(alpha), float(diag), _stream())
    return o


def frechet_from_moments(sum_r, gram_r, shift_r, n_r, sum_f, gram_f, shift_f, n_f, ddof=1, max_iters=48, out=None):
    """The Frechet distance of two pools from the device tensors of their states (``metrics.PoolMoments``: sum [d] / gram [d, d]
    float64, shift [d] fp32 or None, n rows), queued on the current stream.  Returns ``out``, 8 device doubles: fd, |dmu|^2, Tr S_r,
    Tr S_f, Tr (S_r^1/2 S_f S_r^1/2)^1/2, the two roots' iteration counts, status (include/cgs_hip.h).  Nothing is read back here."""
    if not (isinstance(sum_r, torch.Tensor) and sum_r.dim() == 1):
        raise L.CgsError("frechet_from_moments: sum_r must be a [d] tensor")
    d, dev = sum_r.shape[0], sum_r.device
    for t, name, shape in ((sum_r, "sum_r", (d,)), (gram_r, "gram_r", (d, d)), (sum_f, "sum_f", (d,)), (gram_f, "gram_f", (d, d))):
        _typed(t, "frechet_from_moments", name, torch.float64, shape, dev)
    for t, name in ((shift_r, "shift_r"), (shift_f, "shift_f")):
        if t is not None:
            _chk(t, name)
            if tuple(t.shape) != (d,) or t.device != dev:
                raise L.CgsError(f"frechet_from_moments: {name} must be [{d}] on {dev}")
    o = _out(out, 8, dev, torch.float64)
    _typed(o, "frechet_from_moments", "out", torch.float64, (8,), dev)
    _state_call(dev, ("cgs_frechet_ws_bytes", d), f"frechet_from_moments: unsupported width d={d}: 1 <= d <= 2048",
                "cgs_frechet_from_moments", _ptr(sum_r), _ptr(gram_r), _ptr(shift_r), int(n_r), _ptr(sum_f), _ptr(gram_f), _ptr(shift_f), int(n_f),
                d, int(ddof), int(max_iters), _ptr(o))
    return o


# ----------------------------------------------------------------------------- calibration / mode statistics (csrc/diagnostics.hip)
CAL_MAX_BINS, MODE_MAX_K = 64, 64


def calibration_accumulate(p, label, edges, state):
    """Add the calibration statistics of the scores ``p`` (device fp32 [n] or [n, 1]), all of label ``label`` (0 fake, 1 real), to
    ``state``: float64 [3 (n_bins + 1) + 11] on the same device, layout in include/cgs_hip.h.  ``edges``: float64 [n_bins + 1] on the
    device (np.linspace(0., 1. + 1e-8, n_bins + 1)), 1 <= n_bins <= 64.  The host twin is metrics.calibration_state_of."""
    _chk(p, "p")
    if not (p.dim() == 1 or (p.dim() == 2 and p.shape[1] == 1)):
        raise L.CgsError(f"calibration_accumulate: p must be [n] or [n, 1], got {tuple(p.shape)}")
    try:
        label = operator.index(label)
    except TypeError:
        label = None
    if label not in (0, 1):
        raise L.CgsError("calibration_accumulate: label must be the integer 0 (fake) or 1 (real)")
    if not (isinstance(edges, torch.Tensor) and edges.dim() == 1):
        raise L.CgsError("calibration_accumulate: edges must be a 1-D float64 device tensor")
    n_bins = edges.shape[0] - 1
    if not 1 <= n_bins <= CAL_MAX_BINS:
        raise L.CgsError(f"calibration_accumulate: n_bins = {n_bins} outside 1..{CAL_MAX_BINS}")
    _typed(edges, "calibration_accumulate", "edges", torch.float64, (n_bins + 1,), p.device)
    _typed(state, "calibration_accumulate", "state", torch.float64, (3 * (n_bins + 1) + 11,), p.device)
    n = p.shape[0]
    if n == 0:
        return
    _state_call(p.device, ("cgs_calibration_ws_bytes", n, n_bins), f"calibration_accumulate: unsupported size (n={n}, n_bins={n_bins})",
                "cgs_calibration_accumulate", _ptr(p), n, label, _ptr(edges), n_bins, _ptr(state))


def mode_stats_accumulate(x, centeroids, thres, state):
    """Add the mode statistics of the 2-D samples ``x`` (device fp32 [n, 2]) to ``state``: float64 [k + 3] on the same device (per-mode
    hit counts | n | good | sum of the distance to the nearest mode).  ``centeroids``: float64 [k, 2] on the device, 1 <= k <= 64;
    ``thres``: a host float.  The host twin is metrics.mode_state_of."""
    _chk(x, "x")
    if x.dim() != 2 or x.shape[1] != 2:
        raise L.CgsError(f"mode_stats_accumulate: x must be [n, 2], got {tuple(x.shape)}")
    if not (isinstance(centeroids, torch.Tensor) and centeroids.dim() == 2 and centeroids.shape[1] == 2):
        raise L.CgsError("mode_stats_accumulate: centeroids must be a float64 [k, 2] device tensor")
    k = centeroids.shape[0]
    if not 1 <= k <= MODE_MAX_K:
        raise L.CgsError(f"mode_stats_accumulate: k = {k} outside 1..{MODE_MAX_K}")
    _typed(centeroids, "mode_stats_accumulate", "centeroids", torch.float64, (k, 2), x.device)
    _typed(state, "mode_stats_accumulate", "state", torch.float64, (k + 3,), x.device)
    n = x.shape[0]
    if n == 0:
        return
    _state_call(x.device, ("cgs_mode_stats_ws_bytes", n, k), f"mode_stats_accumulate: unsupported size (n={n}, k={k})",
                "cgs_mode_stats_accumulate", _ptr(x), n, _ptr(centeroids), k, float(thres), _ptr(state))


# ----------------------------------------------------------------------------- density map of a 2-D pool (csrc/kde2d.hip)
KDE_MAX_CELLS = 1 << 20


def kde2d_accumulate(x, axis_x, axis_y, whiten, state):
    """Add the un-normalised Gaussian kernel sums of the 2-D samples ``x`` (device fp32 [n, 2]) on the grid ``axis_x`` x ``axis_y`` (device
    fp32 [gx], [gy]) to ``state``: float64 [gx * gy + 1] on the same device (row-major [gx][gy] sums | n).  ``whiten``: float64 [3] on the
    device, w00, w10, w11 of the inverse Cholesky factor of the kernel covariance (metrics.kde_whiten).  The host twin is
    metrics.density_state_of."""
    _chk(x, "x")
    if x.dim() != 2 or x.shape[1] != 2:
        raise L.CgsError(f"kde2d_accumulate: x must be [n, 2], got {tuple(x.shape)}")
    for t, name in ((axis_x, "axis_x"), (axis_y, "axis_y")):
        _chk(t, name)
        if t.dim() != 1 or t.device != x.device:
            raise L.CgsError(f"kde2d_accumulate: {name} must be a 1-D fp32 tensor on {x.device}")
    gx, gy = axis_x.shape[0], axis_y.shape[0]
    if gx < 1 or gy < 1 or gx * gy > KDE_MAX_CELLS:
        raise L.CgsError(f"kde2d_accumulate: grid {gx} x {gy} outside 1 <= gx, gy, gx * gy <= 2^20")
    _typed(whiten, "kde2d_accumulate", "whiten", torch.float64, (3,), x.device)
    _typed(state, "kde2d_accumulate", "state", torch.float64, (gx * gy + 1,), x.device)
    n = x.shape[0]
    if n == 0:
        return
    _state_call(x.device, ("cgs_kde2d_ws_bytes", n, gx, gy), f"kde2d_accumulate: unsupported size (n={n}, grid {gx} x {gy})",
                "cgs_kde2d_accumulate", _ptr(x), n, _ptr(axis_x), gx, _ptr(axis_y), gy, _ptr(whiten), _ptr(state))


# ----------------------------------------------------------------------------- rejection sampling (csrc/drs.hip)
def drs_set_max(sig, state):
    """state[0] = logit(clip(max sig, 1e-14, 1 - 1e-14)): ``Rejector.set_score_max(np.amax(sig))`` on device scores (fp32, any shape, at
    least one).  ``state``: float64 [1] on the same device."""
    _chk(sig, "sig")
    _typed(state, "drs_set_max", "state", torch.float64, (1,), sig.device)
    if sig.numel() < 1:
        raise L.CgsError("drs_set_max: no score")
    with torch.cuda.device(sig.device):
        L.call("cgs_drs_set_max", _ptr(sig), sig.numel(), _ptr(state), _stream())


def drs_decide(sig, uniforms, state, groups=1, shift_percent=60.0, epsilon=1e-8, want_p=False, want_bounds=False):
    """The accept decision of ``Rejector.sampling`` for ``groups`` logical batches of device scores ``sig`` (fp32 [n] or [n, 1], n a whole
    number of groups), as if it had been called once per batch in order (include/cgs_hip.h).  ``uniforms``: float64 [n] on the device;
    ``state``: float64 [1], the running bound, advanced in place; ``shift_percent``: 0..100 or None.
    -> (mask uint8 [n], counts int32 [groups], P float64 [n] or None, bounds float64 [groups] or None), all on the device."""
    _chk(sig, "sig")
    if not (sig.dim() == 1 or (sig.dim() == 2 and sig.shape[1] == 1)):
        raise L.CgsError(f"drs_decide: sig must be [n] or [n, 1], got {tuple(sig.shape)}")
    n, dev = sig.shape[0], sig.device
    try:
        groups = operator.index(groups)
    except TypeError:
        groups = 0
    if groups < 1 or n < 1 or n % groups:
        raise L.CgsError(f"drs_decide: {n} scores are not {groups} whole batches")
    q = -1.0 if shift_percent is None else float(shift_percent)
    if shift_percent is not None and not 0.0 <= q <= 100.0:
        raise L.CgsError(f"drs_decide: shift_percent = {shift_percent} outside [0, 100]")
    if not float(epsilon) > 0.0:
        raise L.CgsError(f"drs_decide: epsilon = {epsilon} must be positive")
    _typed(uniforms, "drs_decide", "uniforms", torch.float64, (n,), dev)
    _typed(state, "drs_decide", "state", torch.float64, (1,), dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.empty(groups, dtype=torch.int32, device=dev)
    P = torch.empty(n, dtype=torch.float64, device=dev) if want_p else None
    bounds = torch.empty(groups, dtype=torch.float64, device=dev) if want_bounds else None
    b = n // groups
    _state_call(dev, ("cgs_drs_ws_bytes", b, groups), f"drs_decide: unsupported size (b={b}, groups={groups})",
                "cgs_drs_decide", _ptr(sig), b, groups, _ptr(uniforms), float(epsilon), q, _ptr(state), _ptr(bounds), _ptr(P), _ptr(mask), _ptr(counts))
    return mask, counts, P, bounds


def compact_rows(src, mask, dst, offset, take_all=None, total=None):
    """Copy the rows of ``src`` (device fp32 [n, ...]) whose ``mask`` byte (device uint8 [n]) is set -- or every row of a group flagged in
    ``take_all`` (device uint8 [groups], n a whole number of groups) -- in ascending order to ``dst[offset], dst[offset + 1], ...``
    (device fp32 [capacity, ...] of the same row shape); rows past the end of ``dst`` are dropped.
    -> ``total``: int32 [1] on the device, the unclipped number of selected rows."""
    _chk(src, "src")
    _chk(dst, "dst")
    if src.dim() < 1 or dst.dim() != src.dim() or tuple(dst.shape[1:]) != tuple(src.shape[1:]) or dst.device != src.device:
        raise L.CgsError(f"compact_rows: dst {tuple(dst.shape)} must hold rows of src {tuple(src.shape)} on {src.device}")
    n, dev = src.shape[0], src.device
    row = src.numel() // n if n else max(dst.numel() // max(dst.shape[0], 1), 1)
    if n and row < 1:
        raise L.CgsError("compact_rows: empty rows")
    _typed(mask, "compact_rows", "mask", torch.uint8, (n,), dev)
    groups = 1
    if take_all is not None:
        if not (isinstance(take_all, torch.Tensor) and take_all.dim() == 1 and take_all.shape[0] >= 1):
            raise L.CgsError("compact_rows: take_all must be a 1-D uint8 device tensor, one flag per group")
        groups = take_all.shape[0]
        _typed(take_all, "compact_rows", "take_all", torch.uint8, (groups,), dev)
        if n % groups:
            raise L.CgsError(f"compact_rows: {n} rows are not {groups} whole groups")
    offset = operator.index(offset)
    if offset < 0:
        raise L.CgsError(f"compact_rows: offset = {offset} is negative")
    if total is None:
        total = torch.empty(1, dtype=torch.int32, device=dev)
    else:
        _typed(total, "compact_rows", "total", torch.int32, (1,), dev)
    _state_call(dev, ("cgs_compact_rows_ws_bytes", n) if n else None, f"compact_rows: unsupported size (n={n})",
                "cgs_compact_rows", _ptr(src), n, row, _ptr(mask), _ptr(take_all), groups, _ptr(dst), offset, dst.shape[0], _ptr(total))
    return total


# ----------------------------------------------------------------------------- Metropolis-Hastings independence chain (csrc/mh.hip)
MH_NO_CAPACITY = 1 << 62


def mh_walk(sig, uniforms, state, T, B=0, groups=1, take_all=None, fill=None, capacity=None):
    """``IndependenceSampler.walk`` for ``groups`` logical batches of device scores ``sig`` (fp32 [n] or [n, 1], n a whole number of
    groups), as if it had been called once per batch in order (include/cgs_hip.h).  ``uniforms``: float64 [n] on the device; ``state``:
    float64 [2], d and cnt, advanced in place; ``take_all``: None or uint8 [groups] on the device, the batches listed whole instead of
    walked; ``fill``: int64 [1] on the device, the unclipped number of rows the pool has received, advanced in place, with ``capacity``
    the pool's rows: a batch that starts with fill >= capacity is not walked (count -1).  Without both it is a plain walk.
    -> (rows int32 [n]: indices into sig's rows in emission order, counts int32 [groups], span int64 [2]: fill at entry and the number
    of rows listed), all on the device."""
    _chk(sig, "sig")
    if not (sig.dim() == 1 or (sig.dim() == 2 and sig.shape[1] == 1)):
        raise L.CgsError(f"mh_walk: sig must be [n] or [n, 1], got {tuple(sig.shape)}")
    n, dev = sig.shape[0], sig.device
    try:
        groups, T, B = operator.index(groups), operator.index(T), operator.index(B)
    except TypeError:
        raise L.CgsError("mh_walk: groups, T and B must be integers") from None
    if groups < 1 or n < 1 or n % groups:
        raise L.CgsError(f"mh_walk: {n} scores are not {groups} whole batches")
    if T < 0 or B < 0 or T >= 1 << 31 or B >= 1 << 31:
        raise L.CgsError(f"mh_walk: T = {T} and B = {B} must be in [0, 2^31)")
    _typed(uniforms, "mh_walk", "uniforms", torch.float64, (n,), dev)
    _typed(state, "mh_walk", "state", torch.float64, (2,), dev)
    if take_all is not None:
        _typed(take_all, "mh_walk", "take_all", torch.uint8, (groups,), dev)
    if (fill is None) != (capacity is None):
        raise L.CgsError("mh_walk: fill and capacity come together")
    if fill is None:
        fill, capacity = torch.zeros(1, dtype=torch.int64, device=dev), MH_NO_CAPACITY
    else:
        _typed(fill, "mh_walk", "fill", torch.int64, (1,), dev)
        capacity = operator.index(capacity)
        if capacity < 0:
            raise L.CgsError(f"mh_walk: capacity = {capacity} is negative")
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(groups, dtype=torch.int32, device=dev)
    span = torch.empty(2, dtype=torch.int64, device=dev)
    b = n // groups
    _state_call(dev, ("cgs_mh_ws_bytes", b, groups), f"mh_walk: unsupported size (b={b}, groups={groups})",
                "cgs_mh_walk", _ptr(sig), b, groups, _ptr(uniforms), T, B, _ptr(take_all), _ptr(state), _ptr(fill), capacity, _ptr(rows), _ptr(counts),
                _ptr(span))
    return rows, counts, span


def gather_rows(src, rows, span, dst):
    """``dst[span[0] + k] = src[rows[k]]`` for k < span[1]: ``src`` device fp32 [n, ...], ``rows`` device int32 [m] (a row may repeat; an
    index outside [0, n) copies nothing), ``span`` device int64 [2], ``dst`` device fp32 [capacity, ...] of the same row shape; rows past
    the end of ``dst`` are dropped.  ``rows`` and ``span`` are what ``mh_walk`` returns."""
    _chk(src, "src")
    _chk(dst, "dst")
    if src.dim() < 1 or dst.dim() != src.dim() or tuple(dst.shape[1:]) != tuple(src.shape[1:]) or dst.device != src.device:
        raise L.CgsError(f"gather_rows: dst {tuple(dst.shape)} must hold rows of src {tuple(src.shape)} on {src.device}")
    n, dev = src.shape[0], src.device
    if not (isinstance(rows, torch.Tensor) and rows.dim() == 1):
        raise L.CgsError("gather_rows: rows must be a 1-D int32 device tensor")
    _typed(rows, "gather_rows", "rows", torch.int32, (rows.shape[0],), dev)
    _typed(span, "gather_rows", "span", torch.int64, (2,), dev)
    if n == 0 or rows.shape[0] == 0 or dst.shape[0] == 0:
        return
    row = src.numel() // n
    if row < 1:
        raise L.CgsError("gather_rows: empty rows")
    with torch.cuda.device(dev):
        L.call("cgs_gather_rows", _ptr(src), n, row, _ptr(rows), rows.shape[0], _ptr(span), _ptr(dst), dst.shape[0], _stream())
