"""DeviceIndependenceSampler: the Metropolis-Hastings independence chain whose walk and row gather run on the GPU (csrc/mh.hip).

The arithmetic is ``IndependenceSampler.walk``'s (reference sampling/idpsampler.py:4-53) for fp32 scores and a started chain, operation
by operation; the scores stay where the discriminator left them, the emitted rows go straight into a device pool, and the host sees
one count per logical batch.  The uniforms are drawn on the host from the global numpy stream, ``np.random.uniform(0, 1, size=b)`` per
walked batch in batch order, so the stream ends where the reference's per-proposal draws would leave it.  The chain state (the score
of the current state and the thinning counter) lives on the device and is carried from call to call.  Not served, and refused before
any launch: an ``np.float64`` seed or float64 scores (numpy then computes the acceptance ratio in double) and an unstarted chain (it
takes its first proposal without a draw).  The host ``IndependenceSampler`` stays what it is."""
import numpy as np
import torch

from .. import kernels as K


class DeviceIndependenceSampler(object):
    def __init__(self, T=5, B=0, device="cuda:0"):
        self.thin_period = int(T)
        self.burn_in = int(B)
        self.dev = torch.device(device)
        self._dev_state = None                                                  # d, cnt: two doubles on the device, made at first use
        self._started = False

    @property
    def _state(self):
        if self._dev_state is None:
            self._dev_state = torch.tensor([0.0, 1.0], dtype=torch.float64, device=self.dev)      # cnt = 1: idpsampler.py:9
        return self._dev_state

    # ------------------------------------------------------------------------------------------------------------------ the state
    def set_score_curr(self, d_curr):
        """Start (or restart) the chain from a state with score ``d_curr``: a Python float, an ``np.float32`` or a 1-element fp32
        device tensor.  The device keeps it as a double, which holds either exactly."""
        if isinstance(d_curr, torch.Tensor):
            if not (d_curr.is_cuda and d_curr.dtype == torch.float32 and d_curr.numel() == 1):
                raise TypeError("set_score_curr: a tensor seed must be a 1-element fp32 device tensor")
            self._state[0:1].copy_(d_curr.reshape(1).to(self.dev))
        elif isinstance(d_curr, np.float32) or type(d_curr) in (float, int):
            self._state[0:1].fill_(float(d_curr))
        elif d_curr is None:
            raise TypeError("set_score_curr: an unstarted chain (None) is not served on the device: it takes its first proposal without "
                            "a draw; use the host IndependenceSampler")
        else:
            raise TypeError(f"set_score_curr: {type(d_curr).__name__} seed: with an np.float64 (or array) state numpy promotes the acceptance "
                            "ratio to double, which the device chain does not compute; pass float(x), np.float32(x), or use the host "
                            "IndependenceSampler")
        self._started = True

    @property
    def d_curr(self):
        """The score of the chain's current state as a host float (a synchronising read of one double); None before the start."""
        return float(self._state[0].item()) if self._started else None

    @property
    def cnt_chain(self):
        """Visits since the last emitted sample (a synchronising read of one double)."""
        return int(self._state[1].item())

    @cnt_chain.setter
    def cnt_chain(self, value):
        self._state[1:2].fill_(float(int(value)))

    # ------------------------------------------------------------------------------------------------------------------- the walk
    def _flags(self, take_all, groups, want_host):
        """-> (take_all as a device uint8 tensor or None, the flags as host booleans if ``want_host``)"""
        if take_all is None:
            return None, [False] * groups
        if isinstance(take_all, torch.Tensor):
            dev = take_all.to(self.dev, torch.uint8).contiguous()
            host = take_all.cpu().numpy().astype(bool).reshape(-1) if want_host else None      # (a synchronising read: only to draw uniforms)
        else:
            host = np.asarray(take_all, dtype=bool).reshape(-1)
            dev = torch.from_numpy(np.ascontiguousarray(host.astype(np.uint8))).to(self.dev)
        if dev.dim() != 1 or dev.shape[0] != groups:
            raise ValueError(f"{dev.numel()} take_all flags for {groups} batches")
        return dev, None if host is None else [bool(f) for f in host]

    def walk_device(self, sig_dev, uniforms=None, groups=1, take_all=None, fill=None, capacity=None):
        """``groups`` logical batches of device scores (fp32 [n] or [n, 1]) through the chain, as ``IndependenceSampler.walk`` called
        once per batch, in order, would take them.  ``uniforms``: None (``np.random.uniform(0, 1, size=b)`` per walked batch, in batch
        order), n host doubles, or a float64 [n] device tensor; ``take_all``: per batch, list its rows whole instead of walking it (host booleans or a device uint8
        tensor); ``fill`` (device int64 [1]) / ``capacity``: the pool's unclipped fill count, advanced in place, and its size -- a batch
        that starts with the pool full is not walked (count -1) and leaves the chain untouched.
        -> (rows int32 [n], counts int32 [groups], span int64 [2]) on the device, queued on the current stream."""
        if not self._started:
            raise ValueError("the device chain needs a start (set_score_curr): an unstarted chain takes its first proposal without a draw")
        if not isinstance(sig_dev, torch.Tensor) or sig_dev.dtype != torch.float32:
            raise TypeError("walk_device: the scores must be an fp32 device tensor (float64 scores promote the acceptance ratio to double: "
                            "use the host IndependenceSampler)")
        n = sig_dev.shape[0]
        if groups < 1 or n % groups:
            raise ValueError(f"{n} scores are not {groups} whole batches")
        b = n // groups
        flags_dev, flags = self._flags(take_all, groups, uniforms is None)
        if isinstance(uniforms, torch.Tensor):
            return K.mh_walk(sig_dev, uniforms, self._state, self.thin_period, self.burn_in, groups, flags_dev, fill, capacity)
        if uniforms is None:
            u = np.zeros(n, dtype=np.float64)
            for g in range(groups):
                if not flags[g]:
                    u[g * b:(g + 1) * b] = np.random.uniform(0, 1, size=b)          # idpsampler.py:50, one per proposal
        else:
            u = np.array(uniforms, dtype=np.float64).reshape(-1)                    # (a copy: the caller's array may be read-only)
            if u.shape[0] != n:
                raise ValueError(f"{u.shape[0]} uniforms for {n} scores")
        return K.mh_walk(sig_dev, torch.from_numpy(u).to(self.dev), self._state, self.thin_period, self.burn_in, groups, flags_dev, fill, capacity)

    def walk(self, sig_dev, uniforms=None, groups=1, take_all=None, fill=None, capacity=None):
        """``walk_device`` with the result read back -> (rows: the emitted row indices as a host int32 array, counts: host int32 [groups])."""
        rows, counts, span = self.walk_device(sig_dev, uniforms, groups, take_all, fill, capacity)
        listed = int(span.cpu()[1])
        return rows.cpu().numpy()[:listed], counts.cpu().numpy()

    def gather(self, src_dev, pool_dev, span, rows):
        """``pool_dev[span[0] + k] = src_dev[rows[k]]`` for the ``rows`` and ``span`` of a walk; rows past the pool's end are dropped."""
        K.gather_rows(src_dev, rows, span, pool_dev)
