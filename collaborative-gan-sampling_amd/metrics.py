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


def _freqs_from_counts(counts, n):
    """Per-mode hit counts of ``n`` samples -> (frequencies among the hits, frequencies incl. a last "no mode" bin): the tail of
    ``freq_category``, shared with ``mode_metrics``."""
    total = counts.sum()
    freqs_valid = counts / total if total > 0 else np.ones(len(counts)) / len(counts)
    return freqs_valid, np.append(counts, n - total) / n


def freq_category(samples, centeroids, thres):
    """(per-mode frequencies among samples that hit a mode, frequencies incl. a last "no mode" bin).  :147-161."""
    hits = _mode_distances(samples, centeroids) < thres
    return _freqs_from_counts(hits.sum(axis=0), hits.shape[0])


def kl_div(predictions, targets):
    """:169-177 (targets clipped away from 0/1; scipy entropy renormalises both)."""
    return float(stats.entropy(predictions, np.clip(targets, 1e-12, 1 - 1e-12)))


def _js_from_freqs(fr, fm):
    avg = 0.5 * (fr + fm)
    return 0.5 * kl_div(fr, avg) + 0.5 * kl_div(fm, avg)


def metrics_diversity(real_batch, model_batch, centeroids, thres):
    """KL(model mode frequencies || real mode frequencies).  :163-167."""
    return kl_div(freq_category(model_batch, centeroids, thres)[0], freq_category(real_batch, centeroids, thres)[0])


def metrics_distribution(real_batch, model_batch, centeroids, thres):
    """JS divergence of the frequencies including the "no mode" bin.  :179-184."""
    return _js_from_freqs(freq_category(real_batch, centeroids, thres)[1], freq_category(model_batch, centeroids, thres)[1])


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

    @classmethod
    def from_state(cls, state, device):
        """A pool on ``device`` that holds a host state (e.g. the result of ``all_reduce_moments``): sum / gram uploaded as they are.
        The shift is kept as fp32 (a PoolMoments shift always is one); a state whose shift is not representable is rebased first."""
        import torch
        shift = np.asarray(state["shift"], dtype=np.float64)
        shift32 = shift.astype(np.float32)
        if not np.array_equal(shift32.astype(np.float64), shift):
            state = moments_rebase(state, shift32.astype(np.float64))
        pm = cls(shift.shape[0], device, shift=shift32)          # raises on a non-GPU device
        pm.n = int(state["n"])
        pm.sum = torch.from_numpy(np.ascontiguousarray(state["sum"], dtype=np.float64).reshape(pm.d)).to(pm.device)
        pm.gram = torch.from_numpy(np.ascontiguousarray(state["gram"], dtype=np.float64).reshape(pm.d, pm.d)).to(pm.device)
        return pm


def frechet_device(real, fake, ddof=1, max_iters=48, details=False):
    """The Frechet distance of two pools computed on the device from their states (csrc/frechet.hip): both
    covariances, the two matrix square roots (Newton-Schulz in double on the float64 MFMA) and the traces stay there; the one
    read-back is the 64-byte record.  ``real`` / ``fake``: ``PoolMoments`` (their queued updates are waited for through their events) or
    host states, which are uploaded to the other one's device (cuda:current if both are states).  Returns the distance, or with
    ``details`` the record {fd, dmu2, tr_r, tr_f, tr_root, iters_r, iters_m, status}; status 0 = tolerance met, 1 = stalled and the
    last good iterate kept (rank-deficient covariances end here), 2 = iteration cap."""
    import torch
    from . import kernels as K
    dev = next((m.device for m in (real, fake) if isinstance(m, PoolMoments)), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    real, fake = (m if isinstance(m, PoolMoments) else PoolMoments.from_state(m, dev) for m in (real, fake))
    if real.d != fake.d or real.device != fake.device:
        raise ValueError(f"frechet_device: pools of width {real.d} on {real.device} and {fake.d} on {fake.device}")
    if min(real.n, fake.n) - ddof <= 0:
        raise ValueError(f"frechet_device: needs more than ddof = {ddof} rows per pool (n = {real.n}, {fake.n})")
    with torch.cuda.device(real.device):
        st = torch.cuda.current_stream(real.device)
        for m in (real, fake):
            if m._last is not None:
                st.wait_event(m._last)
        out = K.frechet_from_moments(real.sum, real.gram, real.shift, real.n, fake.sum, fake.gram, fake.shift, fake.n, ddof=ddof,
                                     max_iters=max_iters)
        h = out.cpu().numpy()                                     # the one read-back: 8 doubles
    if not details:
        return float(h[0])
    return dict(fd=float(h[0]), dmu2=float(h[1]), tr_r=float(h[2]), tr_f=float(h[3]), tr_root=float(h[4]), iters_r=int(h[5]), iters_m=int(h[6]),
                status=int(h[7]))


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


# ------------------------------------------------------------------------------------------------------------------------------
# Calibration of D's scores and the 2-D mode statistics in the same streaming form: a STATE is a small dict of
# host arrays that ADDS across batches, slots and ranks; the functions below are pure numpy on states, ``CalibrationStats`` /
# ``ModeStats`` keep the state in double on the device (csrc/diagnostics.hip) and ``all_reduce_calibration`` / ``all_reduce_modes``
# add the ranks' states.
#
# Calibration (the reference's calibration_diagnostic, utils_sampling.py:186-299).  edges = np.linspace(0., 1. + 1e-8, n_bins + 1); a
# score p (fp32, widened to double exactly) of label y falls into slot np.digitize(p, edges) - 1 of n_bins + 1 slots -- the last one
# catches p >= edges[-1] and NaN, as np.bincount(..., minlength=len(bins)) does; p < edges[0] (the reference's bincount raises) is
# counted in ``under`` and nowhere else.
def calibration_edges(n_bins=20):
    return np.linspace(0., 1. + 1e-8, n_bins + 1)


def _cal_state(n_bins, count, sum_p, sum_y, n, sum_ymp, sum_var, sum_sq, under, label_n, label_sum, label_max):
    i64, f64 = (lambda a: np.asarray(a, dtype=np.int64)), (lambda a: np.asarray(a, dtype=np.float64))
    return dict(n_bins=int(n_bins), count=i64(count), sum_p=f64(sum_p), sum_y=f64(sum_y), n=int(n), sum_ymp=float(sum_ymp),
                sum_var=float(sum_var), sum_sq=float(sum_sq), under=int(under), label_n=i64(label_n), label_sum=f64(label_sum),
                label_max=f64(label_max))


def calibration_state_of(p, label, n_bins=20):
    """The state of the scores ``p`` (any shape; fp32 values, possibly in a float64 holder), all of label ``label`` (0 fake, 1 real), in
    float64 numpy.  {"n_bins", "count" [S], "sum_p" [S], "sum_y" [S], "n", "sum_ymp" = sum (y - p), "sum_var" = sum p (1 - p), "sum_sq" =
    sum (y - p)^2, "under", "label_n" [2], "label_sum" [2], "label_max" [2]} with S = n_bins + 1."""
    if label not in (0, 1):
        raise ValueError(f"label must be 0 or 1, got {label!r}")
    if not 1 <= n_bins <= 64:
        raise ValueError(f"n_bins = {n_bins} outside 1..64")
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    S = n_bins + 1
    slot = np.digitize(p, calibration_edges(n_bins)) - 1
    under = int((slot < 0).sum())
    p, slot = p[slot >= 0], slot[slot >= 0]
    y = float(label)
    count = np.bincount(slot, minlength=S)
    ln, ls, lm = np.zeros(2, np.int64), np.zeros(2), np.zeros(2)
    ln[label], ls[label] = p.size, p.sum()
    lm[label] = np.fmax.reduce(p, initial=0.0)                        # (a NaN never wins; every counted score is >= edges[0] = 0)
    return _cal_state(n_bins, count, np.bincount(slot, weights=p, minlength=S), y * count, p.size, (y - p).sum(), (p * (1.0 - p)).sum(),
                      ((y - p) ** 2).sum(), under, ln, ls, lm)


def calibration_merge(a, b):
    """The state of the union of two score sets."""
    if a["n_bins"] != b["n_bins"]:
        raise ValueError(f"calibration_merge: {a['n_bins']} and {b['n_bins']} bins do not add")
    add = {k: a[k] + b[k] for k in ("count", "sum_p", "sum_y", "n", "sum_ymp", "sum_var", "sum_sq", "under", "label_n", "label_sum")}
    return _cal_state(a["n_bins"], label_max=np.fmax(a["label_max"], b["label_max"]), **add)


def calibration_diagnostics(state):
    """{"z_dawid", "brier", "ece", "mce"} (calibration_diagnostic's four, utils_sampling.py:290-299), the bins behind them ("accuracy",
    "confidence", "weights" over the non-empty slots: calibration_bins, :219-282) and the real scores' "real_mean" / "real_max" (what
    mh_sampler.set_score_curr and rejector.set_score_max are seeded with).  Equals the reference on float64 holders of the fp32 scores
    (the image path, nsgan/GAN.py:287-301); on fp32 arrays (the 2-D call site, synthetic/main.py:115-123) the reference computes z_dawid and
    brier in fp32, so there the match is to fp32 rounding only."""
    if state["under"] > 0:
        raise ValueError(f"{state['under']} scores lie below the first bin edge (the reference's np.bincount raises on them)")
    nz = state["count"] != 0
    count = state["count"][nz]
    accuracy, confidence, weights = state["sum_y"][nz] / count, state["sum_p"][nz] / count, count / state["n"]
    gap = np.absolute(accuracy - confidence)
    real_n = int(state["label_n"][1])
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.float64(state["sum_ymp"]) / np.sqrt(np.float64(state["sum_var"]))
        brier = np.float64(state["sum_sq"]) / state["n"]
    return dict(z_dawid=float(z), brier=float(brier), ece=float(np.sum(gap * weights)), mce=float(np.max(gap)) if gap.size else float("nan"),
                accuracy=accuracy, confidence=confidence, weights=weights,
                real_mean=float(state["label_sum"][1] / real_n) if real_n else float("nan"), real_max=float(state["label_max"][1]))


def _cal_flat(st):
    """A state in the device layout of include/cgs_hip.h: 3 S + 11 doubles."""
    lab = np.stack([st["label_n"].astype(np.float64), st["label_sum"], st["label_max"]], axis=1).reshape(-1)
    return np.concatenate([st["count"].astype(np.float64), st["sum_p"], st["sum_y"],
                           [float(st["n"]), st["sum_ymp"], st["sum_var"], st["sum_sq"], float(st["under"])], lab])


def _cal_unflat(h, n_bins):
    S = n_bins + 1
    g, lab = h[3 * S:3 * S + 5], h[3 * S + 5:].reshape(2, 3)
    return _cal_state(n_bins, np.rint(h[:S]), h[S:2 * S], h[2 * S:3 * S], round(g[0]), g[1], g[2], g[3], round(g[4]), np.rint(lab[:, 0]),
                      lab[:, 1], lab[:, 2])


# 2-D modes (utils_sampling.py:132-161): per sample and mode dist = sqrt(dx dx + dy dy) in double, products and sum rounded separately.
def _mode_state(counts, n, good, sum_min):
    return dict(counts=np.asarray(counts, dtype=np.int64), n=int(n), good=int(good), sum_min=float(sum_min))


def mode_state_of(samples, centeroids, thres):
    """The state of a [n, 2] sample pool in float64 numpy: {"counts" [k]: samples closer than ``thres`` to mode j (a sample may hit
    several), "n", "good": samples whose nearest mode is closer than ``thres``, "sum_min": sum of the distance to the nearest mode}."""
    dist = _mode_distances(np.asarray(samples, dtype=np.float64), np.asarray(centeroids, dtype=np.float64))
    if dist.shape[0] == 0:
        return _mode_state(np.zeros(dist.shape[1], np.int64), 0, 0, 0.0)
    dist_min = dist.min(axis=1)
    return _mode_state((dist < thres).sum(axis=0), dist.shape[0], (dist_min < thres).sum(), dist_min.sum())


def mode_merge(a, b):
    if a["counts"].shape != b["counts"].shape:
        raise ValueError("mode_merge: the states count different numbers of modes")
    return _mode_state(a["counts"] + b["counts"], a["n"] + b["n"], a["good"] + b["good"], a["sum_min"] + b["sum_min"])


def mode_metrics(model_state, real_state):
    """{"mean_dist", "good", "kl", "js"} of a model pool against a real pool from their states: metrics_distance, metrics_diversity and
    metrics_distribution without the pools."""
    fm, fr = _freqs_from_counts(model_state["counts"], model_state["n"]), _freqs_from_counts(real_state["counts"], real_state["n"])
    return dict(mean_dist=float(model_state["sum_min"] / model_state["n"]), good=float(model_state["good"] / model_state["n"]),
                kl=kl_div(fm[0], fr[0]), js=_js_from_freqs(fr[1], fm[1]))


class _DeviceStats:
    """A float64 state vector on the device that ``_accumulate`` adds to.  Updates may come from different HIP streams (the slots of a
    ``FusedProposer``): each one waits for the one before it, as in ``PoolMoments``."""

    def _init(self, device, size, who):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{who} accumulates on a GPU device (the host form is the *_state_of / *_merge functions)")
        self.vec = torch.zeros(size, dtype=torch.float64, device=self.device)
        self._last = None                      # event behind the latest update

    def _chained(self, launch):
        torch = self.torch
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            if self._last is not None:
                st.wait_event(self._last)
            launch()
            self._last = torch.cuda.Event()
            self._last.record(st)
        return self

    def _host(self):
        if self._last is not None:
            self._last.synchronize()
        return self.vec.cpu().numpy()


class CalibrationStats(_DeviceStats):
    """The calibration state of every score handed to ``update``, as ONE float64 device tensor (layout: include/cgs_hip.h)."""

    def __init__(self, device, n_bins=20):
        if not 1 <= n_bins <= 64:
            raise ValueError(f"n_bins = {n_bins} outside 1..64")
        self.n_bins = int(n_bins)
        self._init(device, 3 * (self.n_bins + 1) + 11, "CalibrationStats")
        self.edges = self.torch.from_numpy(calibration_edges(self.n_bins)).to(self.device)

    def update(self, p, label):
        """Add the scores ``p`` (device fp32 [n] or [n, 1]), all of label ``label`` (0 fake, 1 real)."""
        from . import kernels as K
        return self._chained(lambda: K.calibration_accumulate(p, label, self.edges, self.vec))

    def state(self):
        """The state as host arrays (waits for the updates queued so far)."""
        return _cal_unflat(self._host(), self.n_bins)

    def diagnostics(self):
        return calibration_diagnostics(self.state())


class ModeStats(_DeviceStats):
    """The mode state of every 2-D sample handed to ``update``: k + 3 doubles on the device."""

    def __init__(self, centeroids, thres, device):
        c = np.ascontiguousarray(centeroids, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != 2 or not 1 <= c.shape[0] <= 64:
            raise ValueError(f"centeroids {c.shape} are not [k, 2] with 1 <= k <= 64")
        self.k, self.thres = c.shape[0], float(thres)
        self._init(device, self.k + 3, "ModeStats")
        self.centeroids = self.torch.from_numpy(c).to(self.device)

    def update(self, x):
        """Add the samples ``x`` (device fp32 [n, 2])."""
        from . import kernels as K
        return self._chained(lambda: K.mode_stats_accumulate(x, self.centeroids, self.thres, self.vec))

    def state(self):
        h = self._host()
        return _mode_state(np.rint(h[:self.k]), round(h[self.k]), round(h[self.k + 1]), h[self.k + 2])


def _all_reduce_flat(stats, flat_of, max_index, group):
    """SUM all-reduce of a flat state (device tensor under "nccl", else staged through the host); the entries ``max_index`` travel in a
    second, MAX all-reduce.  Returns the reduced flat host array, or None without a process group."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    on_dev = dist.get_backend(group) == "nccl"
    if isinstance(stats, _DeviceStats):
        stats._host()                                                   # (every queued update is behind us)
        flat = stats.vec.clone() if on_dev else stats.vec.cpu()
    else:
        flat = torch.from_numpy(flat_of(stats))
        flat = flat.to(torch.device("cuda", torch.cuda.current_device())) if on_dev else flat
    mx = flat[max_index].clone() if max_index else None
    dist.all_reduce(flat, group=group)
    if mx is not None:
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        flat[max_index] = mx
    return flat.cpu().numpy()


def all_reduce_calibration(stats, group=None):
    """The calibration state of every rank's scores together: ONE SUM all-reduce of the 3 S + 11 doubles and one MAX all-reduce of the two
    maxima.  ``stats``: a state or a ``CalibrationStats``.  Without a process group it is the identity."""
    st = stats.state() if isinstance(stats, CalibrationStats) else stats
    S = st["n_bins"] + 1
    h = _all_reduce_flat(stats, _cal_flat, [3 * S + 7, 3 * S + 10], group)
    return st if h is None else _cal_unflat(h, st["n_bins"])


def all_reduce_modes(stats, group=None):
    """The mode state of every rank's pool together: ONE SUM all-reduce of k + 3 doubles.  ``stats``: a state or a ``ModeStats``."""
    st = stats.state() if isinstance(stats, ModeStats) else stats
    k = st["counts"].shape[0]
    h = _all_reduce_flat(stats, lambda s: np.concatenate([s["counts"].astype(np.float64), [float(s["n"]), float(s["good"]), s["sum_min"]]]), [], group)
    return st if h is None else _mode_state(np.rint(h[:k]), round(h[k]), round(h[k + 1]), h[k + 2])


# ------------------------------------------------------------------------------------------------------------------------------
# The density map of a 2-D pool in the same streaming form: the arithmetic of the reference's draw_kde
# (utils_sampling.py:97-112) without the drawing.  Grid: each axis is np.linspace(-scale, scale, nbins) rounded to fp32, the map is defined
# at those coordinates widened exactly, index [i, j] = the point (x_i, y_j) as np.mgrid lays it out.  Bandwidth: C = f^2 cov(samples,
# ddof=1), f = bw_scale n^(-1/6) (Scott's factor for d = 2, halved by set_bandwidth(k.factor / 2.)); C = L L^T, W = L^-1 lower triangular.
# density(g) = sum_k exp(-1/2 |W (g - x_k)|^2) / (n 2 pi sqrt(det C)).  A STATE is {"sums" [gx, gy]: the un-normalised kernel sums, "n",
# "whiten" [3]: w00, w10, w11}; with the bandwidth fixed it ADDS across batches, slots and ranks.
def kde_axes(scale, nbins=100):
    """One axis of the reference's grid (np.mgrid[-scale:scale:nbins*1j]) as the fp32 coordinates the map is defined at."""
    return np.linspace(-scale, scale, nbins).astype(np.float32)


def kde_whiten(cov, n, bw_scale=0.5):
    """(whiten, norm) of a pool of ``n`` samples with covariance ``cov`` ([2, 2], ddof = 1): whiten = [w00, w10, w11] of W = L^-1 with
    L L^T = (bw_scale n^(-1/6))^2 cov, norm = n 2 pi sqrt(det C).  ValueError for n < 2 and for a covariance that is not positive definite
    to working precision (a collinear pool): scipy's gaussian_kde raises there too."""
    cov = np.asarray(cov, dtype=np.float64)
    if cov.shape != (2, 2):
        raise ValueError(f"kde_whiten: covariance {cov.shape} is not [2, 2]")
    if n < 2:
        raise ValueError(f"kde_whiten: a bandwidth needs at least 2 samples, got {n}")
    c = (bw_scale * float(n) ** (-1.0 / 6.0)) ** 2 * cov
    try:
        l = np.linalg.cholesky(c)
    except np.linalg.LinAlgError:
        l = None
    # (rounding can leave a collinear pool a pivot of ~1e-16 c11 instead of 0: below 64 eps of c11 the factor carries no digit)
    if l is None or not np.isfinite(l).all() or l[1, 1] ** 2 <= 64.0 * np.finfo(np.float64).eps * c[1, 1]:
        raise ValueError("kde_whiten: the pool's covariance is not positive definite (fewer than 2 distinct samples, or a collinear pool)")
    whiten = np.array([1.0 / l[0, 0], -l[1, 0] / (l[0, 0] * l[1, 1]), 1.0 / l[1, 1]])
    return whiten, float(n * 2.0 * np.pi * l[0, 0] * l[1, 1])


def _density_state(sums, n, whiten):
    return dict(sums=np.asarray(sums, dtype=np.float64), n=int(n), whiten=np.asarray(whiten, dtype=np.float64).reshape(3))


def density_state_of(samples, axis_x, axis_y, whiten, chunk=512):
    """The state of a [n, 2] pool on the grid ``axis_x`` x ``axis_y`` in float64 numpy: sums[i, j] = sum_k exp(-1/2 |W (g_ij - x_k)|^2),
    difference first, then whitened (``chunk`` samples at a time: n gx gy terms)."""
    x = np.asarray(samples, dtype=np.float64).reshape(-1, 2)
    ax, ay = np.asarray(axis_x, dtype=np.float64).reshape(-1), np.asarray(axis_y, dtype=np.float64).reshape(-1)
    w00, w10, w11 = np.asarray(whiten, dtype=np.float64).reshape(3)
    sums = np.zeros((ax.size, ay.size))
    for a in range(0, x.shape[0], chunk):
        dx = ax[None, :, None] - x[a:a + chunk, 0][:, None, None]           # [m, gx, 1]
        dy = ay[None, None, :] - x[a:a + chunk, 1][:, None, None]           # [m, 1, gy]
        u, v = w00 * dx, w10 * dx + w11 * dy
        sums += np.exp(-0.5 * (u * u + v * v)).sum(axis=0)
    return _density_state(sums, x.shape[0], [w00, w10, w11])


def density_merge(a, b):
    """The state of the union of two pools under ONE bandwidth."""
    if a["sums"].shape != b["sums"].shape or not np.array_equal(a["whiten"], b["whiten"]):
        raise ValueError("density_merge: the states are of different grids or bandwidths and do not add")
    return _density_state(a["sums"] + b["sums"], a["n"] + b["n"], a["whiten"])


def density_values(state, norm=None):
    """The [gx, gy] float64 map: sums / (n 2 pi sqrt(det C)) with the state's own n and sqrt(det C) = 1 / (w00 w11) of its bandwidth;
    ``norm`` (``kde_whiten``'s, for the pool the bandwidth came from) replaces that divisor."""
    if norm is None:
        norm = state["n"] * 2.0 * np.pi / (state["whiten"][0] * state["whiten"][2])
    return state["sums"] / norm


class DensityMap(_DeviceStats):
    """The density state of every 2-D sample handed to ``update`` on a fixed grid under a FIXED bandwidth (which is what makes it additive):
    gx gy + 1 doubles on the device (csrc/kde2d.hip)."""

    def __init__(self, axis_x, axis_y, whiten, device):
        ax, ay = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (axis_x, axis_y))
        w = np.ascontiguousarray(whiten, dtype=np.float64).reshape(-1)
        if ax.size < 1 or ay.size < 1 or ax.size * ay.size > 1 << 20:
            raise ValueError(f"grid {ax.size} x {ay.size} outside 1 <= gx, gy, gx * gy <= 2^20")
        if w.shape != (3,):
            raise ValueError("whiten must hold the three numbers w00, w10, w11 (kde_whiten)")
        self.gx, self.gy, self.whiten_host = ax.size, ay.size, w
        self._init(device, self.gx * self.gy + 1, "DensityMap")
        self.axis_x, self.axis_y = self.torch.from_numpy(ax).to(self.device), self.torch.from_numpy(ay).to(self.device)
        self.whiten = self.torch.from_numpy(w).to(self.device)

    def update(self, x):
        """Add the samples ``x`` (device fp32 [n, 2])."""
        from . import kernels as K
        return self._chained(lambda: K.kde2d_accumulate(x, self.axis_x, self.axis_y, self.whiten, self.vec))

    def state(self):
        h = self._host()
        return _density_state(h[:-1].reshape(self.gx, self.gy), round(h[-1]), self.whiten_host)

    def values(self, norm=None):
        return density_values(self.state(), norm)


def all_reduce_density(stats, group=None):
    """The density state of every rank's pool together (same grid, same bandwidth on every rank): ONE SUM all-reduce of gx gy + 1 doubles.
    ``stats``: a state or a ``DensityMap``."""
    st = stats.state() if isinstance(stats, DensityMap) else stats
    h = _all_reduce_flat(stats, lambda s: np.concatenate([s["sums"].reshape(-1), [float(s["n"])]]), [], group)
    return st if h is None else _density_state(h[:-1].reshape(st["sums"].shape), round(h[-1]), st["whiten"])


def kde_grid(samples, scale, nbins=100, bw_scale=0.5, device=None):
    """The map ``draw_kde(samples, scale, fname)`` colours, computed on the device in two passes: the pool's covariance from a
    ``PoolMoments`` (five doubles to the host), ``kde_whiten``, one ``DensityMap.update``.  ``samples``: [n, 2], a host array or a device
    tensor (taken as fp32).  Returns (zi [nbins, nbins] float64, (vmin, vmax)) with the colour limits draw_kde hands to pcolormesh:
    (min, max(0.2 max, min))."""
    import torch
    if isinstance(samples, torch.Tensor):
        dev = samples.device if device is None else torch.device(device)
        x = samples.to(dev, torch.float32).contiguous()
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        x = torch.from_numpy(np.array(samples, dtype=np.float32, order="C")).to(dev)
    if x.dim() != 2 or x.shape[1] != 2:
        raise ValueError(f"kde_grid: samples {tuple(x.shape)} are not [n, 2]")
    n = x.shape[0]
    if n < 2:
        raise ValueError(f"kde_grid: a bandwidth needs at least 2 samples, got {n}")
    _, cov = PoolMoments(2, dev).update(x).mean_cov(ddof=1)
    whiten, norm = kde_whiten(cov, n, bw_scale)
    axis = kde_axes(scale, nbins)
    zi = DensityMap(axis, axis, whiten, dev).update(x).values(norm)
    lo, hi = float(zi.min()), float(zi.max())
    return zi, (lo, max(hi * 0.2, lo))


# ----------------------------------------------------------------------------- nearest-neighbour metrics (csrc/knn.hip)
def _sq_distances(a, b):
    """[len(a), len(b)] float64 squared distances in the difference form, the coordinates added in ascending order: the sum scipy's
    ``cdist`` takes the root of."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"pools {a.shape} and {b.shape} are not [n, d] and [m, d]")
    out = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        diff = a[:, k, None] - b[None, :, k]
        out += diff * diff
    return out


def pairwise_distance(real_batch, model_batch):
    """The reference's ``pairwise_distance`` (sampling/utils_sampling.py:126-130) on host arrays, without scipy: per model sample the
    distance to the nearest real sample, the real sample of the SAME index standing 10 farther away than it is (``cdist + 10 I``, minimum
    over the real axis).  Like the reference it needs pools of one length."""
    dist = np.sqrt(_sq_distances(real_batch, model_batch))
    if dist.shape[0] != dist.shape[1]:
        raise ValueError(f"pairwise_distance: the 10 I term needs pools of one length, got {dist.shape[0]} and {dist.shape[1]}")
    return np.min(dist + 10.0 * np.identity(dist.shape[0]), axis=0)


def _device_pool(x, who, device=None):
    import torch
    if isinstance(x, torch.Tensor):
        if not x.is_cuda and device is None:
            raise ValueError(f"{who}: a host tensor needs device=")
        x = x.to(x.device if device is None else device, torch.float32).contiguous()
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        x = torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(dev)
    if x.dim() != 2:
        raise ValueError(f"{who}: a pool is [n, d], got {tuple(x.shape)}")
    return x


def nn_distance(real, model, exclude_self=None):
    """``pairwise_distance`` on device pools (fp32 [n, d]; host arrays are uploaded) through ``cgs_nn_min``: per MODEL sample j the distance
    to the nearest real sample and that sample's index, as device tensors (float64 [m], int32 [m]).  ``exclude_self``: True = the
    reference's rule, the real sample of index j counts as 10 farther away than it is (needs pools of one length; the index is j where
    that term still wins); False = the plain nearest neighbour; None = True for pools of one length, else False.  The root of the
    minimum is the minimum of the roots (sqrt is monotone and correctly rounded), so with True the result equals
    ``pairwise_distance`` wherever the kernel's D2 equals the host's."""
    import torch
    from . import knn
    model = _device_pool(model, "nn_distance")
    real = _device_pool(real, "nn_distance", model.device)
    if exclude_self is None:
        exclude_self = real.shape[0] == model.shape[0]
    d2, idx, self_d2 = knn.nn_min(model, real, exclude_self=exclude_self)
    dist = torch.sqrt(d2)
    if not exclude_self:
        return dist, idx
    own = torch.sqrt(self_d2) + 10.0
    j = torch.arange(model.shape[0], dtype=torch.int32, device=model.device)
    wins = (own < dist) | ((own == dist) & (j < idx))
    return torch.where(wins, own, dist), torch.where(wins, j, idx)


def knn_radii(x, k):
    """The distance from every row of the device pool ``x`` (fp32 [n, d]) to its k-th nearest OTHER row (1 <= k <= 8, k < n): float64 [n]
    on the device.  (``cgs_amd.knn.knn_radii`` returns the squares and takes a second pool.)"""
    import torch
    from . import knn
    return torch.sqrt(knn.knn_radii(_device_pool(x, "knn_radii"), k))


def _manifold_result(hits_fake, balls_fake, hits_real, covered, k, n_real, n_fake):
    return {"precision": hits_fake / n_fake, "recall": hits_real / n_real, "density": balls_fake / (k * n_fake), "coverage": covered / n_real,
            "k": int(k), "n_real": int(n_real), "n_fake": int(n_fake)}


def manifold_metrics(real_feat, fake_feat, k=5):
    """The k-nearest-neighbour manifold metrics of two device pools of features (fp32 [n_real, d] and [n_fake, d]; host arrays are
    uploaded): precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020), every comparison ``<=``, with
    rho_k(x) the distance from x to its k-th nearest other row of its own pool:
        count_j   = #{i : |f_j - r_i| <= rho_k(r_i)}            precision = mean_j [count_j > 0]       density = sum_j count_j / (k n_fake)
        recall    = the precision formula with the pools exchanged (radii within the fakes)
        coverage  = mean_i [min_j |r_i - f_j| <= rho_k(r_i)]
    Two ``knn_radii``, two ``ball_count`` and one ``nn_min`` launch (csrc/knn.hip; the comparisons are made on the squares), four integer
    sums in torch on the device, ONE readback of four integers.  Returns {"precision", "recall", "density", "coverage", "k", "n_real",
    "n_fake"}.  NOT additive across ranks: a k-th neighbour needs the whole pool, so ranks first assemble it (``dist.gather_pool``) and
    one of them calls this; there is no collective of its own."""
    import torch
    from . import knn
    real = _device_pool(real_feat, "manifold_metrics")
    fake = _device_pool(fake_feat, "manifold_metrics", real.device)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"manifold_metrics: features of width {real.shape[1]} and {fake.shape[1]}")
    r2_real, r2_fake = knn.knn_radii(real, k), knn.knn_radii(fake, k)
    count_fake = knn.ball_count(fake, real, r2_real)
    count_real = knn.ball_count(real, fake, r2_fake)
    near_d2, _, _ = knn.nn_min(real, fake)
    sums = torch.stack([(count_fake > 0).sum(), count_fake.sum(dtype=torch.int64), (count_real > 0).sum(), (near_d2 <= r2_real).sum()]).cpu()
    hits_fake, balls_fake, hits_real, covered = (int(v) for v in sums)
    return _manifold_result(hits_fake, balls_fake, hits_real, covered, k, real.shape[0], fake.shape[0])


def manifold_metrics_host(real_feat, fake_feat, k=5):
    """``manifold_metrics`` in float64 numpy on host arrays: the same definitions on the full distance matrices."""
    real, fake = np.asarray(real_feat, dtype=np.float64), np.asarray(fake_feat, dtype=np.float64)

    def radii2(x):
        if not 1 <= k < len(x):
            raise ValueError(f"manifold_metrics_host: k = {k} needs 1 <= k < {len(x)} rows")
        d2 = _sq_distances(x, x)
        np.fill_diagonal(d2, np.inf)
        return np.partition(d2, k - 1, axis=1)[:, k - 1]
    r2_real, r2_fake = radii2(real), radii2(fake)
    cross = _sq_distances(fake, real)                                       # [n_fake, n_real]
    count_fake = (cross <= r2_real[None, :]).sum(axis=1)
    count_real = (cross.T <= r2_fake[None, :]).sum(axis=1)
    covered = cross.min(axis=0) <= r2_real
    return _manifold_result(int((count_fake > 0).sum()), int(count_fake.sum()), int((count_real > 0).sum()), int(covered.sum()), k,
                            len(real), len(fake))
