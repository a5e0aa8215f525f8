"""DeviceRejector: Discriminator Rejection Sampling whose accept decision and compaction run on the GPU (csrc/drs.hip).

The arithmetic is ``Rejector``'s (reference sampling/rejector.py:7-38) in its operation order; the scores stay where the discriminator
left them, the accepted rows go straight into a device pool, and the host sees one count per logical batch.  The uniforms are drawn on
the host from the global numpy stream, ``np.random.rand(b)`` per batch in batch order, so the stream ends where the reference's
per-batch ``sampling`` calls would leave it.  The host ``Rejector`` stays what it is."""
import numpy as np
import torch

from .. import kernels as K


class DeviceRejector(object):
    def __init__(self, device="cuda:0"):
        self.dev = torch.device(device)
        self._state = torch.zeros(1, dtype=torch.float64, device=self.dev)      # running max logit; 0.0 = logit(0.5) (rejector.py:9)
        self.last_accept = None                                                 # device mask of the latest decide()
        self.last_bounds = None                                                 # device D_tilde_M after each batch of the latest decide()

    @property
    def D_tilde_M(self):
        """The running bound as a host float (a synchronising read of one double)."""
        return float(self._state.item())

    @D_tilde_M.setter
    def D_tilde_M(self, value):
        self._state.fill_(float(value))

    def set_score_max(self, real_scores):
        """``Rejector.set_score_max(np.amax(real_scores))``: a device fp32 tensor of scores is reduced on the device; a host array or
        scalar is uploaded first (scores are fp32 wherever the discriminator leaves them)."""
        if not isinstance(real_scores, torch.Tensor):
            real_scores = torch.from_numpy(np.ascontiguousarray(np.asarray(real_scores, dtype=np.float32).reshape(-1)))
        K.drs_set_max(real_scores.to(self.dev, torch.float32).contiguous(), self._state)

    def _uniforms(self, n, groups, uniforms):
        if uniforms is None:
            b = n // groups
            uniforms = np.concatenate([np.random.rand(b) for _ in range(groups)])   # rejector.py:33, once per batch
        u = np.array(uniforms, dtype=np.float64).reshape(-1)                        # (a copy: the caller's array may be read-only)
        if u.shape[0] != n:
            raise ValueError(f"{u.shape[0]} uniforms for {n} scores")
        return torch.from_numpy(u).to(self.dev)

    def decide_device(self, sig_dev, uniforms=None, shift_percent=60.0, epsilon=1e-8, groups=1, want_p=False):
        """``decide`` without the read-back: -> (mask uint8 [n], counts int32 [groups], P float64 [n] or None), all on the device,
        queued on the current stream."""
        n = sig_dev.shape[0]
        if groups < 1 or n % groups:
            raise ValueError(f"{n} scores are not {groups} whole batches")
        u = self._uniforms(n, groups, uniforms)
        mask, counts, P, bounds = K.drs_decide(sig_dev, u, self._state, groups, shift_percent, epsilon, want_p=want_p, want_bounds=True)
        self.last_accept, self.last_bounds = mask, bounds
        return mask, counts, P

    def decide(self, sig_dev, uniforms=None, shift_percent=60.0, epsilon=1e-8, groups=1):
        """Accept or reject ``groups`` logical batches of device scores (fp32 [n] or [n, 1]) as ``Rejector.sampling`` called once per
        batch, in order, would.  ``uniforms``: None (np.random.rand(b) per batch, in batch order) or n host doubles.
        -> (mask: uint8 [n] on the device, counts: int32 host array [groups], the accepted rows per batch)."""
        mask, counts, _ = self.decide_device(sig_dev, uniforms, shift_percent, epsilon, groups)
        return mask, counts.cpu().numpy()

    def rewind_to(self, group):
        """Put the bound back to what it was after batch ``group`` of the latest decide(): the fill loops decide a round of batches at
        once and may find that the reference's loop would have stopped inside it."""
        self._state.copy_(self.last_bounds[group:group + 1])

    def compact(self, src_dev, pool_dev, offset, take_all=None, mask=None):
        """Copy the rows of ``src_dev`` the latest decide() accepted (or ``mask``'s) -- every row of a batch flagged in ``take_all`` (host
        booleans or a device uint8 tensor, one per batch) -- to ``pool_dev[offset:]`` in order; rows past the pool's end are dropped.
        -> a device int32 [1]: the unclipped number of selected rows."""
        mask = self.last_accept if mask is None else mask
        if take_all is not None and not isinstance(take_all, torch.Tensor):
            take_all = torch.from_numpy(np.ascontiguousarray(np.asarray(take_all, dtype=bool).astype(np.uint8))).to(self.dev)
        return K.compact_rows(src_dev, mask, pool_dev, offset, take_all=take_all)
