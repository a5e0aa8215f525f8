"""Sample-quality metrics used right after the refinement path.

2-D mode metrics: the reference's sampling/utils_sampling.py:132-184 (mean distance to the nearest mode, rate of
"good" samples within ``thres`` of a mode, KL of the per-mode frequencies, JS of the frequencies including the
"no mode" bin), as reported in the reference's figures (README.md:26-28).
Image metric: the Frechet distance between two feature clouds (the formula behind the reference's tfgan
``mnist_frechet_distance``, nsgan/utils_mnist.py:85-116); the feature extractor is pluggable because the
reference's classifier graph is a missing binary blob.
"""
import numpy as np
from scipy import linalg, stats


def _mode_distances(samples, centeroids):
    samples, centeroids = np.asarray(samples), np.asarray(centeroids)
    return np.linalg.norm(samples[:, None, :] - centeroids[None, :, :], axis=2)          # [n, k]


def metrics_distance(samples, centeroids, thres):
    """(mean distance to the nearest mode, fraction of samples closer than ``thres`` to a mode).  utils_sampling.py:132-145."""
    dist_min = _mode_distances(samples, centeroids).min(axis=1)
    return float(np.mean(dist_min)), float((dist_min < thres).sum() / dist_min.size)


def freq_category(samples, centeroids, thres):
    """(per-mode frequencies among samples that hit a mode, frequencies incl. a last "no mode" bin).  :147-161."""
    hits = _mode_distances(samples, centeroids) < thres
    counts = hits.sum(axis=0)
    total, n = counts.sum(), hits.shape[0]
    freqs_valid = counts / total if total > 0 else np.ones(len(counts)) / len(counts)
    return freqs_valid, np.append(counts, n - total) / n


def kl_div(predictions, targets):
    """:169-177 (targets clipped away from 0/1; scipy entropy renormalises both)."""
    return float(stats.entropy(predictions, np.clip(targets, 1e-12, 1 - 1e-12)))


def metrics_diversity(real_batch, model_batch, centeroids, thres):
    """KL(model mode frequencies || real mode frequencies).  :163-167."""
    return kl_div(freq_category(model_batch, centeroids, thres)[0], freq_category(real_batch, centeroids, thres)[0])


def metrics_distribution(real_batch, model_batch, centeroids, thres):
    """JS divergence of the frequencies including the "no mode" bin.  :179-184."""
    fr, fm = freq_category(real_batch, centeroids, thres)[1], freq_category(model_batch, centeroids, thres)[1]
    avg = 0.5 * (fr + fm)
    return 0.5 * kl_div(fr, avg) + 0.5 * kl_div(fm, avg)


def frechet_distance(feat_real, feat_fake):
    """|mu_r - mu_f|^2 + Tr(S_r + S_f - 2 (S_r S_f)^{1/2}) between two [n, d] feature clouds."""
    fr, ff = np.asarray(feat_real, dtype=np.float64), np.asarray(feat_fake, dtype=np.float64)
    mu_r, mu_f = fr.mean(0), ff.mean(0)
    s_r, s_f = np.cov(fr, rowvar=False), np.cov(ff, rowvar=False)
    return frechet_from_moments(mu_r, s_r, mu_f, s_f)


def frechet_from_moments(mu_r, s_r, mu_f, s_f):
    """The same distance from the two means and covariances (the tail of ``frechet_distance``, operation for operation)."""
    covmean, _ = linalg.sqrtm(s_r.dot(s_f), disp=False)
    covmean = covmean.real if np.iscomplexobj(covmean) else covmean
    return float(((mu_r - mu_f) ** 2).sum() + np.trace(s_r) + np.trace(s_f) - 2.0 * np.trace(covmean))


# ------------------------------------------------------------------------------------------------------------------------------
# Streaming form: a pool's Frechet statistics are n, s = sum(x - c) and G = sum (x - c)(x - c)^T about a fixed shift c -- d + d^2
# numbers however large the pool.  A STATE is the dict {"n": int, "shift": [d], "sum": [d], "gram": [d, d]} of float64 host arrays;
# the functions below are pure numpy on states.  ``PoolMoments`` keeps sum / gram in double on the device and adds to them batch by
# batch (csrc/moments.hip) as the fill loop accepts samples; ``all_reduce_moments`` adds the states of the ranks.
def _state(n, shift, s, g):
    return dict(n=int(n), shift=np.asarray(shift, dtype=np.float64), sum=np.asarray(s, dtype=np.float64), gram=np.asarray(g, dtype=np.float64))


def moments_of(x, shift=None):
    """The state of a whole [n, d] cloud in float64 numpy (tests, small pools); shift defaults to 0."""
    x = np.asarray(x, dtype=np.float64)
    c = np.zeros(x.shape[1]) if shift is None else np.asarray(shift, dtype=np.float64)
    a = x - c
    return _state(x.shape[0], c, a.sum(0), a.T.dot(a))


def moments_rebase(state, new_shift):
    """The same pool about another shift: delta = shift - new_shift, s' = s + n delta, G' = G + s delta^T + delta s^T + n delta delta^T."""
    n, s, g = state["n"], state["sum"], state["gram"]
    new_shift = np.asarray(new_shift, dtype=np.float64)
    delta = state["shift"] - new_shift
    return _state(n, new_shift, s + n * delta, g + np.outer(s, delta) + np.outer(delta, s) + n * np.outer(delta, delta))


def moments_merge(a, b):
    """The union of two pools about the shift of ``a`` (``b`` is rebased onto it)."""
    b = moments_rebase(b, a["shift"])
    return _state(a["n"] + b["n"], a["shift"], a["sum"] + b["sum"], a["gram"] + b["gram"])


def moments_mean_cov(state, ddof=1):
    """(mean, covariance) of the pool: mean = shift + s / n, cov = (G - s s^T / n) / (n - ddof)  (ddof = 1 as in np.cov)."""
    n, s = state["n"], state["sum"]
    return state["shift"] + s / n, (state["gram"] - np.outer(s, s) / n) / (n - ddof)


class PoolMoments:
    """n, sum(x - shift), sum (x - shift)(x - shift)^T of every feature row handed to ``update``, the last two as float64 DEVICE
    tensors.  ``shift=None``: the first update fixes the shift to that batch's fp32 column mean (computed on the device), which keeps
    G - s s^T / n free of cancellation for features far from 0.  Updates may come from different HIP streams (the slots of a
    ``FusedProposer``): each one waits for the one before it."""

    def __init__(self, d, device, shift=None):
        import torch
        self.torch = torch
        self.d, self.device = int(d), torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PoolMoments accumulates on a GPU device (the host form is moments_of / moments_merge)")
        self.n = 0
        self.shift = None if shift is None else torch.as_tensor(np.asarray(shift, dtype=np.float32)).reshape(self.d).contiguous().to(self.device)
        self.sum = torch.zeros(self.d, dtype=torch.float64, device=self.device)
        self.gram = torch.zeros((self.d, self.d), dtype=torch.float64, device=self.device)
        self._last = None                      # event behind the latest update

    def update(self, feat, rows=None):
        """Add the rows of ``feat`` (device fp32 [n, d]; ``rows``: host integer array, default all) to the pool."""
        from . import kernels as K
        torch = self.torch
        if feat.dim() != 2 or feat.shape[1] != self.d:
            raise ValueError(f"PoolMoments.update: features {tuple(feat.shape)} are not [n, {self.d}]")
        m = feat.shape[0] if rows is None else int(np.asarray(rows).size)
        if m == 0:
            return self
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            if self._last is not None:
                st.wait_event(self._last)
            if self.shift is None:
                sel = feat if rows is None else feat[torch.as_tensor(np.asarray(rows, dtype=np.int64), device=self.device)]
                self.shift = K.spatial_mean(sel.contiguous().view(1, sel.shape[0], self.d)).view(self.d)
            K.pool_moments(feat, self.sum, self.gram, shift=self.shift, rows=rows)
            self._last = torch.cuda.Event()
            self._last.record(st)
        self.n += m
        return self

    def state(self):
        """{"n", "shift", "sum", "gram"} as float64 host arrays (waits for the updates queued so far)."""
        if self._last is not None:
            self._last.synchronize()
        shift = np.zeros(self.d) if self.shift is None else self.shift.cpu().numpy().astype(np.float64)
        return _state(self.n, shift, self.sum.cpu().numpy(), self.gram.cpu().numpy())

    def mean_cov(self, ddof=1):
        return moments_mean_cov(self.state(), ddof)


def all_reduce_moments(moments, group=None):
    """The state of the union of every rank's pool: rank 0's shift is broadcast, each rank rebases onto it, and ONE all-reduce adds
    [n | sum | gram] in double (1 + d + d^2 numbers per rank instead of the pool).  ``moments``: a state or a ``PoolMoments``.
    "nccl" (RCCL) broadcasts and reduces device tensors; any other backend is staged through the host like ``dist.gather_pool``.
    Without a process group it is the identity."""
    import torch
    import torch.distributed as dist
    dev = moments.device if isinstance(moments, PoolMoments) else None
    st = moments.state() if isinstance(moments, PoolMoments) else moments
    if not (dist.is_available() and dist.is_initialized()):
        return st
    d = st["shift"].shape[0]
    on_dev = dist.get_backend(group) == "nccl"
    if on_dev and dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    root = dist.get_global_rank(group, 0) if group is not None else 0
    shift = torch.from_numpy(st["shift"].copy())
    shift = shift.to(dev) if on_dev else shift
    dist.broadcast(shift, src=root, group=group)
    st = moments_rebase(st, shift.cpu().numpy())
    flat = torch.from_numpy(np.concatenate([[float(st["n"])], st["sum"], st["gram"].reshape(-1)]))
    flat = flat.to(dev) if on_dev else flat
    dist.all_reduce(flat, group=group)
    h = flat.cpu().numpy()
    return _state(int(round(h[0])), st["shift"], h[1:1 + d], h[1 + d:].reshape(d, d))
