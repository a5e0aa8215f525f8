"""The 2-D (synthetic/) side of the reference on the GPU: BASELINE config 1.

* ``MLPDiscriminator``  -- the ReLU MLP D of synthetic/GAN.py:28-37 with the three tensors refiner_cpu fetches
  (``fake_samples`` / ``fake_sigmoid`` / ``fake_saliency``, synthetic/GAN.py:105-111) evaluated by one HIP kernel.
* ``Session`` / ``gan`` -- a ``sess.run(fetches, feed_dict)`` adaptor so the reference-shaped host loop
  ``sampling.refiner_cpu.Refiner`` drives the GPU discriminator unchanged (K+2 launches per batch).
* ``Refiner``           -- same class surface as ``refiner_cpu.Refiner`` (``Refiner(args)``, ``set_env``,
  ``manipulate_sample``), but the whole K-step loop -- D forward, saliency, ladam / momentum / sgd update, best-loss
  tracking, trajectory -- is ONE kernel launch (up to 64 hidden units: one wave per sample, weights in LDS; 65..256 units, the
  25-Gaussians D: a tile of samples per workgroup on the fp32 MFMA, weights streamed from L2).
* ``DShaper`` / ``WideDShaper`` -- the D update of the calibrate / shape modes (synthetic/main.py:361-370), in place on the
  discriminator's tensors: up to 64 units and 65..256 units; ``d_shaper`` picks the class by width.  ``shape_step`` takes either.
* ``MLPGenerator`` / ``GStep`` -- the batch-normalised MLP G of synthetic/GAN.py:39-49 (training- and inference-mode forward)
  and its update g_optim (GAN.py:83-101) on the device, up to 64 hidden units.
* ``WideMLPGenerator``  -- the same forward, both modes, at 65..256 units (the 25-Gaussians G: 256 x 6); ``mlp_generator`` picks the class
  by width.
* ``WideGStep``         -- ``GStep`` for a ``WideMLPGenerator`` (cgs_mlp2d_wide_g_step); ``g_stepper`` picks the class by width.
* ``GanTrainer``        -- the iteration loop of synthetic/main.py:350-395 (train | calibrate | shape | test) on the 64-unit pieces.
* ``WideGanTrainer``    -- the same loop for a D and a G of any supported width: calibrate, shape and test always, train while G is narrow.
* ``Gan2DTrainer``      -- the same loop, all four modes, for any supported widths of G and D (``g_stepper`` and ``d_shaper``).

Variable names follow tf.layers.dense: ``discriminator/d_fc<i>/kernel`` ([din, dout]) and ``.../bias``; G's are
``generator/g_fc<i>/kernel|bias`` and ``generator/BatchNorm[_k]/gamma|beta|moving_mean|moving_variance``.
"""
import ctypes as C

import numpy as np
import torch

from . import checkpoint as CK
from . import lib as L
from .datasets import NoiseDataset
from .kernels import _Scratch

_METHODS = {"sgd": 0, "momentum": 1, "ladam": 2}


def glorot_uniform(rs, din, dout):
    """tf.layers.dense's default kernel initializer (glorot_uniform: U(-l, l), l = sqrt(6 / (din + dout))) from a numpy RandomState."""
    lim = np.sqrt(6.0 / (din + dout))
    return rs.uniform(-lim, lim, size=(din, dout)).astype(np.float32)


def _dense_init(prefix, dims, seed):
    """{prefix<i>/kernel: glorot-uniform, prefix<i>/bias: zeros} for the dense chain ``dims`` (tf.layers.dense defaults)."""
    rs = np.random.RandomState(seed)
    P = {}
    for i in range(len(dims) - 1):
        P[f"{prefix}{i + 1}/kernel"] = glorot_uniform(rs, dims[i], dims[i + 1])
        P[f"{prefix}{i + 1}/bias"] = np.zeros(dims[i + 1], np.float32)
    return P


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _upload(x, dev):
    """A host batch -> float32 device tensor without a host synchronisation (pinned staging, asynchronous copy); device tensors pass."""
    if isinstance(x, torch.Tensor) and x.device == dev:
        return x.float().contiguous()
    t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)) if not isinstance(x, torch.Tensor) else x.float().contiguous()
    return t.pin_memory().to(dev, non_blocking=True)


class MLPDiscriminator:
    def __init__(self, params, device="cuda:0"):
        """``params``: {"discriminator/d_fc1/kernel": [2,nh], "discriminator/d_fc1/bias": [nh], ...}."""
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise L.CgsError("MLPDiscriminator needs a GPU device (the host loop with a caller-supplied sess is sampling.refiner_cpu)")
        L.load()
        n = 1
        while f"discriminator/d_fc{n + 1}/kernel" in params:
            n += 1
        self.nlayers = n
        self.w = [torch.as_tensor(np.asarray(params[f"discriminator/d_fc{i + 1}/kernel"]), dtype=torch.float32).contiguous().to(self.dev) for i in range(n)]
        self.b = [torch.as_tensor(np.asarray(params[f"discriminator/d_fc{i + 1}/bias"]), dtype=torch.float32).contiguous().to(self.dev) for i in range(n)]
        self.nhidden = int(self.w[0].shape[1])
        if self.w[0].shape[0] != 2 or self.w[-1].shape[1] != 1 or self.nhidden > 256 or not 2 <= n <= 6:
            # up to 64 units every layer's weights (and their transposes) are LDS-resident: 6 layers = 133 KB of the CU's 160 KB; from 65 to
            # 256 the sample-tile kernels keep only a tile's activations in LDS (T = 64 at 256 units: 143 KB) and stream the weights from L2
            raise L.CgsError(f"MLPDiscriminator: unsupported shape (2 -> {self.nhidden} x {n - 1} -> 1; need nhidden <= 256, 2..6 layers)")
        self._wp = (C.c_void_p * n)(*[t.data_ptr() for t in self.w])
        self._bp = (C.c_void_p * n)(*[t.data_ptr() for t in self.b])

    @classmethod
    def from_lists(cls, Ws, bs, device="cuda:0"):
        P = {}
        for i, (w, b) in enumerate(zip(Ws, bs)):
            P[f"discriminator/d_fc{i + 1}/kernel"], P[f"discriminator/d_fc{i + 1}/bias"] = np.asarray(w), np.asarray(b)
        return cls(P, device)

    @staticmethod
    def init_params(seed, nhidden=64, nlayers=6):
        """Seeded tf.layers.dense defaults (glorot-uniform kernels, zero biases) for 2 -> nhidden x (nlayers-1) -> 1, as host arrays."""
        return _dense_init("discriminator/d_fc", [2] + [nhidden] * (nlayers - 1) + [1], seed)

    @classmethod
    def init(cls, seed, nhidden=64, nlayers=6, device="cuda:0"):
        return cls(cls.init_params(seed, nhidden, nlayers), device)

    def params(self):
        """{TF variable name: device tensor} -- the D half of a synthetic/main.py checkpoint (``checkpoint.save`` writes it)."""
        P = {}
        for i in range(self.nlayers):
            P[f"discriminator/d_fc{i + 1}/kernel"], P[f"discriminator/d_fc{i + 1}/bias"] = self.w[i], self.b[i]
        return P

    def _x(self, x):
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.dev) if not isinstance(x, torch.Tensor) else x.float().contiguous().to(self.dev)

    def sigmoid_and_saliency(self, x, want_saliency=True):
        """-> (sigmoid [B,1], saliency [B,2] or None) as device tensors; saliency carries the 1/B factor (quirk Q8)."""
        xd = self._x(x)
        B = xd.shape[0]
        sig = torch.empty(B, dtype=torch.float32, device=self.dev)
        sal = torch.empty((B, 2), dtype=torch.float32, device=self.dev) if want_saliency else None
        L.call("cgs_mlp2d_sigmoid_saliency", self._wp, self._bp, self.nlayers, self.nhidden, xd.data_ptr(), sig.data_ptr(),
               None if sal is None else sal.data_ptr(), B, 1.0 / B, torch.cuda.current_stream(self.dev).cuda_stream)
        return sig.view(B, 1), sal

    def refine(self, fake_batch, real_sigmoid_mean, steps, rate, method="ladam", want_traj=False):
        """The fused K-step loop.  -> (best_x [B,2], best_step [B], traj [B,K+1,2] or None) device tensors."""
        if method not in _METHODS:
            raise NotImplementedError(method)
        xd = self._x(fake_batch)
        B = xd.shape[0]
        best = torch.empty((B, 2), dtype=torch.float32, device=self.dev)
        step = torch.empty(B, dtype=torch.float32, device=self.dev)
        traj = torch.empty((B, steps + 1, 2), dtype=torch.float32, device=self.dev) if want_traj else None
        tail = (1.0 / B, int(steps), float(rate), _METHODS[method], best.data_ptr(), step.data_ptr(),
                None if traj is None else traj.data_ptr(), B, torch.cuda.current_stream(self.dev).cuda_stream)
        if isinstance(real_sigmoid_mean, torch.Tensor):            # a device scalar: no host round trip, batches queue back to back
            base = real_sigmoid_mean.to(self.dev, torch.float32).reshape(1)
            L.call("cgs_refine2d_devbase", self._wp, self._bp, self.nlayers, self.nhidden, xd.data_ptr(), base.data_ptr(), *tail)
        else:
            L.call("cgs_refine2d", self._wp, self._bp, self.nlayers, self.nhidden, xd.data_ptr(), float(real_sigmoid_mean), *tail)
        return best, step, traj


class Gan:
    """The three graph handles refiner_cpu reads off the reference's GAN object (synthetic/GAN.py:105-111)."""
    fake_samples, fake_sigmoid, fake_saliency = "fake_samples", "fake_sigmoid", "fake_saliency"

    def __init__(self, discriminator):
        self.D = discriminator


class Session:
    """``sess.run([gan.fake_sigmoid, gan.fake_saliency], feed_dict={gan.fake_samples: x})`` on the GPU discriminator."""

    def __init__(self, gan):
        self.gan, self.n_runs = gan, 0

    def run(self, fetches, feed_dict):
        single = not isinstance(fetches, (list, tuple))
        names = [fetches] if single else list(fetches)
        sig, sal = self.gan.D.sigmoid_and_saliency(feed_dict[Gan.fake_samples], want_saliency=Gan.fake_saliency in names)
        self.n_runs += 1
        out = [{Gan.fake_sigmoid: sig, Gan.fake_saliency: sal}[n].cpu().numpy() for n in names]
        return out[0] if single else out


class Refiner:
    """refiner_cpu.Refiner's surface (sampling/refiner_cpu.py:8-81) with the loop fused on the device."""

    def __init__(self, args):
        self.forward_steps, self.step_size, self.method = args.rollout_steps, args.rollout_rate, args.rollout_method
        if self.method not in _METHODS:
            raise NotImplementedError(self.method)

    def set_env(self, gan, sess, data):
        self.gan, self.sess, self.data = gan, sess, data

    def manipulate_sample(self, fake_batch, mode='deterministic'):
        if mode not in ('deterministic', 'probabilistic'):
            raise NotImplementedError
        D = self.gan.D
        real = self.data.next_batch(fake_batch.shape[0])                        # consumes the global RNG like :22
        real_sig, _ = D.sigmoid_and_saliency(real, want_saliency=False)
        baseline = np.mean(real_sig.cpu().numpy())                              # np.mean(real_sigmoid), :28
        best, step, traj = D.refine(fake_batch, baseline, self.forward_steps, self.step_size, self.method,
                                    want_traj=(mode == 'probabilistic'))
        self.optimal_step = step.cpu().numpy()
        if mode == 'probabilistic':                                             # per-call draw, float64 out (:72-76)
            n = len(fake_batch)
            pick = np.random.randint(self.forward_steps + 1, size=n)
            return traj.cpu().numpy().astype(np.float64)[np.arange(n), pick, :]
        return best.cpu().numpy().astype(fake_batch.dtype, copy=False)


def _need_narrow(discriminator, who):
    """DShaper, GanTrainer and the generator are 64-unit kernels; scoring, refining and WideDShaper's D step run up to 256 units."""
    if discriminator.nhidden > 64:
        raise L.CgsError(f"{who}: discriminator has {discriminator.nhidden} hidden units, the limit here is 64: the D step and the "
                         "generator are still 64-unit kernels (sigmoid_and_saliency / refine / Refiner serve up to 256)")


class DShaper:
    """The D update of the 2-D shaping loop (synthetic/main.py:366-370): one ``tf.train.GradientDescentOptimizer(lrd)`` step on
    d_loss = mean BCE(D(real), 1) + mean BCE(D(refined), 0) (synthetic/GAN.py:69-74,98-99), run on the device IN PLACE on the
    ``MLPDiscriminator``'s own weight tensors (two per-sample forward/backward launches + one gradient/update launch).
    The refiner reads the same tensors, so the next ``manipulate_sample`` sees the shaped D."""

    _entry = "cgs_mlp2d_d_step"

    def __init__(self, discriminator, lrd=1e-2):                      # synthetic/main.py:39 (--lrd 1e-2)
        _need_narrow(discriminator, "DShaper")
        self._setup(discriminator, lrd)

    def _setup(self, discriminator, lrd):
        self.D, self.lrd = discriminator, float(lrd)
        self.loss = torch.zeros(2, dtype=torch.float32, device=discriminator.dev)
        self.gw = [torch.zeros_like(t) for t in discriminator.w]
        self.gb = [torch.zeros_like(t) for t in discriminator.b]
        n = discriminator.nlayers
        self._gwp = (C.c_void_p * n)(*[t.data_ptr() for t in self.gw])
        self._gbp = (C.c_void_p * n)(*[t.data_ptr() for t in self.gb])
        self._ws = _Scratch(pad=4)

    def _run(self, real, refined, lr):
        D = self.D
        xr, xf = D._x(real), D._x(refined)
        ws = self._ws.get(self._ws_bytes(xr.shape[0] + xf.shape[0]), D.dev)
        L.call(self._entry, D._wp, D._bp, D.nlayers, D.nhidden, xr.data_ptr(), xr.shape[0], xf.data_ptr(), xf.shape[0],
               float(lr), self._gwp, self._gbp, self.loss.data_ptr(), ws.data_ptr(), ws.numel() * 4,
               torch.cuda.current_stream(D.dev).cuda_stream)
        return self.loss

    def _ws_bytes(self, B_total):
        return int(L.load().cgs_mlp2d_train_ws_bytes(B_total, self.D.nlayers))

    def loss_and_grads(self, real, refined):
        """((d_loss_real, d_loss_fake) device tensor, [dW...], [db...]) without touching the weights."""
        return self._run(real, refined, 0.0), self.gw, self.gb

    def step(self, real, refined):
        """One SGD step of D; returns (d_loss_real, d_loss_fake) as evaluated BEFORE the update (device tensor)."""
        return self._run(real, refined, self.lrd)


class WideDShaper(DShaper):
    """``DShaper`` for a D of 65..256 hidden units (the 25-Gaussians runs: 256 x 6), same surface, same in-place update: a sample tile
    per workgroup keeps every layer's activation and pre-activation gradient, the hidden -> hidden weight gradients are MFMA products
    over sample chunks of a size fixed by the batch alone, added in chunk order (csrc/mlp2d_wide_train.hip; deterministic)."""

    _entry = "cgs_mlp2d_wide_d_step"

    def __init__(self, discriminator, lrd=1e-2):
        if discriminator.nhidden <= 64:
            raise L.CgsError(f"WideDShaper: discriminator has {discriminator.nhidden} hidden units; up to 64 units the D step is DShaper "
                             "(d_shaper() picks the class by width)")
        self._setup(discriminator, lrd)

    def _ws_bytes(self, B_total):
        return int(L.load().cgs_mlp2d_wide_train_ws_bytes(B_total, self.D.nlayers, self.D.nhidden))


def d_shaper(discriminator, lrd=1e-2):
    """The D update for this discriminator's width: ``DShaper`` up to 64 hidden units, ``WideDShaper`` above."""
    return (DShaper if discriminator.nhidden <= 64 else WideDShaper)(discriminator, lrd)


def shape_step(refiner, shaper, noise_sample, real_batch):
    """One iteration of synthetic/main.py:366-370:
    ``refined = refiner.manipulate_sample(noise_sample, 'probabilistic'); sess.run(d_optim, {inputs: real, generates: refined})``."""
    refined = refiner.manipulate_sample(noise_sample, 'probabilistic')
    return shaper.step(real_batch, refined), refined


def proposer(refiner, generate, discriminator):
    """propose() / score() closures for ``evaluate.collaborate`` on the 2-D path (synthetic/main.py:240-243):
    ``generate()`` -> a generator batch (``sess.run(gan.generates, {z: noise.next_batch(n)})`` in the reference -- G is outside
    the hot path, so the caller supplies it); propose = the device refiner on it; score = the device D's sigmoid."""
    def propose():
        return refiner.manipulate_sample(generate())

    def score(batch):
        return discriminator.sigmoid_and_saliency(batch, want_saliency=False)[0].cpu().numpy()      # float32 [n, 1] like sess.run(gan.fake_sigmoid) (synthetic/main.py:232)

    return propose, score


def landscape_grid(scale, ngrids=21):
    """The [ngrids^2, 2] float64 grid the reference scores for its critic landscape (synthetic/main.py:318-329): row i * ngrids + j is
    (-scale + i * step, -scale + j * step), step = 2 scale / (ngrids - 1), each in the reference's order of operations."""
    step = 2 * scale / (ngrids - 1)
    axis = -scale + np.arange(ngrids) * step
    grid = np.zeros((ngrids * ngrids, 2))
    grid[:, 0], grid[:, 1] = np.repeat(axis, ngrids), np.tile(axis, ngrids)
    return grid


def _device_chain_fill(mh, discriminator, propose, eval_size, real_sigmoid_mean, base, base_sig):
    """The fill loop of synthetic/main.py:182-202 / 229-253 with the chain on the device (``mh``: a sampling.DeviceIndependenceSampler):
    scores stay where D left them, every round is ONE segment of ``eval_size`` proposals, the pool is a device tensor; per round the host
    reads one count and hands it to the productive-only counter rule (:196-202, :245-251: ``cnt_propose += eval_size`` for a round that
    yielded rows, and for no other).  ``propose()`` -> the round's proposals (host array or device tensor); the round's uniforms are drawn
    after it, where the reference's ``sampling`` call stands.
    -> (pool: device fp32 [eval_size, 2], efficiency)"""
    from .evaluate import _FillCounter
    dev = discriminator.dev
    pool = torch.empty((eval_size, 2), dtype=torch.float32, device=dev)
    fill = torch.zeros(1, dtype=torch.int64, device=dev)
    mh.set_score_curr(real_sigmoid_mean)                                               # :183,230

    def one_round(x, sig):
        rows, counts, span = mh.walk_device(sig, None, 1, None, fill, eval_size)
        mh.gather(x, pool, span, rows)
        return int(counts.cpu()[0])                                                    # the round's only read-back
    C = _FillCounter(eval_size, productive_only=True)
    C.start(one_round(_upload(base, dev), base_sig))
    while not C.full:
        x = _upload(propose(), dev)
        C.add(one_round(x, discriminator.sigmoid_and_saliency(x, want_saliency=False)[0]), eval_size)
    return pool, C.efficiency


def _check_maps(maps):
    if maps is not None and ("scale" not in maps or set(maps) - {"scale", "nbins", "grid_scale", "ngrids"}):
        raise ValueError(f"maps: needs 'scale', takes 'nbins', 'grid_scale', 'ngrids'; got {sorted(maps)}")


def _check_manifold(manifold):
    if manifold is not None and (set(manifold) != {"k"} or not 1 <= int(manifold["k"]) <= 8):
        raise ValueError(f"manifold: takes 'k' in 1..8 alone; got {manifold}")


def _add_manifold(out, manifold, pools, target_batch, dev):
    """Each row of ``out`` named in ``pools`` ((name, pool) pairs) gains precision / recall / density / coverage of its pool against
    ``target_batch``, the 2-D points as features (``metrics.manifold_metrics``: csrc/knn.hip)."""
    from . import metrics as Mx
    target = _upload(target_batch, dev)
    for name, pool in pools:
        got = Mx.manifold_metrics(target, _upload(pool, dev), k=int(manifold["k"]))
        out[name].update({key: got[key] for key in ("precision", "recall", "density", "coverage")})


def _quality_of(diagnostics, target_batch, centeroids, thres, dev):
    """-> quality(samples): the reference's four 2-D metrics of a pool against ``target_batch`` (utils_sampling.py:132-184) -- on the host
    as the reference computes them, or, with ``diagnostics``, from ``metrics.ModeStats`` on the device."""
    from . import metrics as Mx
    if diagnostics:
        real_modes = Mx.ModeStats(centeroids, thres, dev).update(_upload(target_batch, dev)).state()

    def quality(samples):
        if diagnostics:
            return Mx.mode_metrics(Mx.ModeStats(centeroids, thres, dev).update(_upload(samples, dev)).state(), real_modes)
        if isinstance(samples, torch.Tensor):
            samples = samples.cpu().numpy()
        mean_dist, good = Mx.metrics_distance(samples, centeroids, thres)
        return {"mean_dist": float(mean_dist), "good": float(good),
                "kl": float(Mx.metrics_diversity(target_batch, samples, centeroids, thres)),
                "js": float(Mx.metrics_distribution(target_batch, samples, centeroids, thres))}
    return quality


def _batch_generator(generate, n):
    """``generate`` as a callable: an ``MLPGenerator`` becomes training-mode G on fresh noise, n per batch (main.py:158-159,239-240)."""
    if not isinstance(generate, MLPGenerator):
        return generate
    noise = NoiseDataset()
    return lambda: generate.generate(noise.next_batch(n)).cpu().numpy()


def _maps_of(maps, pools, discriminator):
    """The density maps of ``pools`` ((name, pool) pairs) and D's landscape, as ``maps`` asks for them (``evaluate_collaborative``)."""
    from . import metrics as Mx
    scale, nbins = maps["scale"], maps.get("nbins", 100)
    out = {name: Mx.kde_grid(pool, scale, nbins, device=discriminator.dev)[0] for name, pool in pools}
    grid = landscape_grid(maps.get("grid_scale", scale), maps.get("ngrids", 21))
    out["landscape"] = (grid, discriminator.sigmoid_and_saliency(grid, want_saliency=False)[0].cpu().numpy())
    return out


def evaluate_collaborative(refiner, discriminator, generate, eval_batch, target_batch, centeroids, std, mh_sampler=None, diagnostics=False,
                           maps=None, keep_pools=False, manifold=None):
    """The "shape"-mode evaluation of synthetic/main.py:215-263 on the device refiner: refine the evaluation batch, report its
    quality, then D-score -> MH fill (thinning T = 20, chain seeded with mean(real_sigmoid)) until ``len(eval_batch)`` samples
    are accepted (proposal counter advancing only for productive batches, :251) and report the collaborative sample's
    quality.  Returns {"refinement": {...}, "collaborate": {..., "eff": accepted / proposed}} with the reference's four 2-D
    metrics (utils_sampling.py:132-184; ``thres`` = 4 std as in main.py:221).  ``generate``: a callable returning a generator batch,
    or an ``MLPGenerator`` (then each proposal batch is G in training mode on ``NoiseDataset().next_batch(len(eval_batch))``).
    ``diagnostics=True``: D's scores of ``eval_batch`` (label 0) and ``target_batch`` (label 1) go into a ``metrics.CalibrationStats``
    as in synthetic/main.py:115-123 and the result gains "calibration" (``metrics.calibration_diagnostics``: the row's z_dawid brier ece
    mce, computed in double where the reference's fp32 arrays give fp32 sums); the pools' quality then comes from ``metrics.ModeStats``
    on the device, the pools taken as fp32.  Draws, samples and ``eff`` are those of ``diagnostics=False``.
    ``maps=dict(scale=region, nbins=100, grid_scale=..., ngrids=21)``: what the reference's ``--eval_type full`` draws, without the
    drawing.  The result gains "maps": the [nbins, nbins] float64 density maps (``metrics.kde_grid``, draw_kde of main.py:142,222,256,337)
    of the pools under "standard", "refinement", "collaborate" and "target", and "landscape": (grid, sigmoid), D's score on
    ``landscape_grid(grid_scale, ngrids)`` (main.py:115,130,318-333; ``grid_scale`` defaults to ``scale``).  The maps draw nothing from the
    numpy stream and are made after everything else: every other entry is that of ``maps=None``.
    ``mh_sampler``: a ``sampling.DeviceIndependenceSampler`` runs the collaborate leg's chain on the device (csrc/mh.hip): the refined
    proposals' scores stay where D left them, the pool is a device tensor handed to ``ModeStats`` and ``kde_grid`` as it is, one count
    per round comes back; samples, ``eff`` and the numpy stream are those of the host sampler.  ``keep_pools=True`` adds "pools": the
    refinement pool and the collaborate pool (a device tensor on the device route).
    ``manifold=dict(k=...)``: the rows "standard", "refinement" and "collaborate" each gain "precision", "recall", "density" and
    "coverage" of their pool against ``target_batch`` (``metrics.manifold_metrics``, the 2-D points as features, 1 <= k <= 8).  Like the
    maps they draw nothing and are computed after everything else: the draws and every other entry are those of ``manifold=None``.
    """
    from . import metrics as Mx
    from .evaluate import collaborate
    from .sampling import DeviceIndependenceSampler, IndependenceSampler
    _check_maps(maps)                                                                  # before any draw
    _check_manifold(manifold)
    quality = _quality_of(diagnostics, target_batch, centeroids, std * 4, discriminator.dev)
    generate = _batch_generator(generate, len(eval_batch))
    _, score = proposer(refiner, generate, discriminator)
    real_sigmoid = score(target_batch)                                                 # main.py:116
    out = {"standard": quality(eval_batch)}
    if diagnostics:                                                                    # :116-117,123: straight from D's device output
        cal = Mx.CalibrationStats(discriminator.dev)
        cal.update(discriminator.sigmoid_and_saliency(eval_batch, want_saliency=False)[0], 0)
        cal.update(discriminator.sigmoid_and_saliency(target_batch, want_saliency=False)[0], 1)
        out["calibration"] = cal.diagnostics()
    refined = refiner.manipulate_sample(eval_batch)                                    # :217
    out["refinement"] = quality(refined)
    mh = mh_sampler if mh_sampler is not None else IndependenceSampler(T=20)           # main.py:80
    propose = lambda: refiner.manipulate_sample(generate())                            # :239-241 (eval_size proposals per round)
    if isinstance(mh, DeviceIndependenceSampler):
        refined_dev = _upload(refined, discriminator.dev)
        samples, eff = _device_chain_fill(mh, discriminator, propose, len(eval_batch), float(np.mean(real_sigmoid)), refined_dev,
                                          discriminator.sigmoid_and_saliency(refined_dev, want_saliency=False)[0])
    else:
        samples, eff = collaborate(propose, score, mh, len(eval_batch), float(np.mean(real_sigmoid)),
                                   base=(refined, score(refined)), count_only_productive=True)  # :229-253
    out["collaborate"] = dict(quality(samples), eff=float(eff))
    if keep_pools:
        out["pools"] = {"refinement": refined, "collaborate": samples}
    if maps is not None:
        out["maps"] = _maps_of(maps, (("standard", eval_batch), ("refinement", refined), ("collaborate", samples), ("target", target_batch)),
                               discriminator)
    if manifold is not None:
        _add_manifold(out, manifold, (("standard", eval_batch), ("refinement", refined), ("collaborate", samples)), target_batch, discriminator.dev)
    return out


def evaluate_calibrated(discriminator, generate, eval_batch, target_batch, centeroids, std, rejector=None, mh_sampler=None, diagnostics=False,
                        maps=None, keep_pools=False, manifold=None):
    """The "calibrate"-mode evaluation of synthetic/main.py:137-214: the standard pool's quality, then the two samplers a calibrated D
    is for.  Rejection (:149-181): a ``sampling.DeviceRejector`` with its bound seeded by max(real_sigmoid) and shift_percent = 100
    decides the evaluation batch and then fresh generator batches of ``len(eval_batch)`` until that many samples are accepted (the
    proposal counter advancing only for productive batches, :163-169); scores, decisions, compaction and the pool stay on the device,
    one count per batch comes back.  Hastings (:182-214): ``evaluate.collaborate`` on UNREFINED proposals with the sampler of
    main.py:77-81 (``IndependenceSampler(T=20)``), chain seeded with mean(real_sigmoid), the evaluation batch as base.
    Returns {"standard": {...}, "rejection": {..., "eff"}, "hastings": {..., "eff"}} with the reference's four 2-D metrics
    (``thres`` = 4 std).  ``generate`` / ``diagnostics`` / ``maps`` as in ``evaluate_collaborative`` (the maps' pools: "standard",
    "rejection", "hastings", "target"); ``keep_pools=True`` adds "pools": the rejection pool (a device tensor) and the hastings pool.
    The numpy stream is consumed as the reference consumes it: per rejection batch one uniform per proposal, then the chain's.
    ``mh_sampler``: a ``sampling.DeviceIndependenceSampler`` runs the hastings leg's chain on the device (csrc/mh.hip) on the scores D
    left there; the hastings pool is then a device tensor too, handed to ``ModeStats`` and ``kde_grid`` as it is; samples, ``eff`` and the
    numpy stream are those of the host sampler.  ``manifold=dict(k=...)`` as in ``evaluate_collaborative``: the rows "standard", "rejection"
    and "hastings" gain the four numbers of their pool against ``target_batch``, after everything else."""
    from . import metrics as Mx
    from .evaluate import _FillCounter, collaborate
    from .sampling import DeviceIndependenceSampler, DeviceRejector, IndependenceSampler
    dev = discriminator.dev
    eval_size = len(eval_batch)
    _check_maps(maps)                                                                  # before any draw
    _check_manifold(manifold)
    quality = _quality_of(diagnostics, target_batch, centeroids, std * 4, dev)
    generate = _batch_generator(generate, eval_size)
    sigmoid = lambda x: discriminator.sigmoid_and_saliency(x, want_saliency=False)[0]
    eval_dev = _upload(eval_batch, dev)
    real_sig, eval_sig = sigmoid(target_batch), sigmoid(eval_dev)                      # main.py:116-117
    out = {"standard": quality(eval_batch)}
    if diagnostics:                                                                    # :123
        cal = Mx.CalibrationStats(dev)
        cal.update(eval_sig, 0)
        cal.update(real_sig, 1)
        out["calibration"] = cal.diagnostics()
    # rejection, :149-169
    rej = rejector if rejector is not None else DeviceRejector(dev)
    pool = torch.empty((eval_size, 2), dtype=torch.float32, device=dev)
    rej.set_score_max(real_sig)                                                        # :152
    _, counts = rej.decide(eval_sig, shift_percent=100.0)                              # :153
    rej.compact(eval_dev, pool, 0)
    C = _FillCounter(eval_size, productive_only=True)                                  # :163-169
    C.start(int(counts[0]))
    while not C.full:
        extra = _upload(generate(), dev)                                               # :158-159
        _, counts = rej.decide(sigmoid(extra), shift_percent=100.0)                    # :160-161
        rej.compact(extra, pool, C.cnt)
        C.add(int(counts[0]), eval_size)                                               # :169 (its own constant, whatever the batch holds)
    out["rejection"] = dict(quality(pool), eff=float(C.efficiency))
    # hastings, :182-202
    mh = mh_sampler if mh_sampler is not None else IndependenceSampler(T=20)           # main.py:80
    score = lambda batch: sigmoid(batch).cpu().numpy()
    real_host = real_sig.cpu().numpy()
    if isinstance(mh, DeviceIndependenceSampler):
        samples, eff = _device_chain_fill(mh, discriminator, generate, eval_size, float(np.mean(real_host)), eval_dev, eval_sig)
    else:
        samples, eff = collaborate(generate, score, mh, eval_size, float(np.mean(real_host)), base=(eval_batch, eval_sig.cpu().numpy()),
                                   count_only_productive=True)
    out["hastings"] = dict(quality(samples), eff=float(eff))
    if keep_pools:
        out["pools"] = {"rejection": pool, "hastings": samples}
    if maps is not None:
        out["maps"] = _maps_of(maps, (("standard", eval_batch), ("rejection", pool.cpu().numpy()), ("hastings", samples), ("target", target_batch)),
                               discriminator)
    if manifold is not None:
        _add_manifold(out, manifold, (("standard", eval_dev), ("rejection", pool), ("hastings", samples)), target_batch, dev)
    return out


def _bn_name(k):
    """tf.contrib.layers.batch_norm's default scopes in creation order: BatchNorm, BatchNorm_1, ..."""
    return "generator/BatchNorm" if k == 0 else f"generator/BatchNorm_{k}"


class MLPGenerator:
    """The 2-D generator of synthetic/GAN.py:39-49 on the device: 2 -> nhidden x (nlayers-1) -> 2, every hidden dense layer followed by
    tf.contrib.layers.batch_norm(decay=0.9, epsilon=1e-5, scale=True, updates_collections=None) and a ReLU.  The variables are device
    tensors under their TF names; ``generate`` in training mode moves the BN moving averages in place, as every ``sess.run`` of
    ``gan.generates`` does in the reference."""
    # GAN.py:43,47 pass epsilon=1e-5, but rank-2 inputs take TF 1.x's fused path, whose nn_impl.fused_batch_norm raises any epsilon below
    # cuDNN's minimum to 1.001e-5: the value the reference computes with
    EPS = 1.001e-5
    _entry = "cgs_mlp2d_gen_fwd"

    def __init__(self, params, device="cuda:0"):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise L.CgsError("MLPGenerator needs a GPU device")
        L.load()
        n = 1
        while f"generator/g_fc{n + 1}/kernel" in params:
            n += 1
        self.nlayers = n
        f32 = lambda name: torch.as_tensor(np.asarray(params[name]), dtype=torch.float32).contiguous().to(self.dev)
        self.w = [f32(f"generator/g_fc{i + 1}/kernel") for i in range(n)]
        self.b = [f32(f"generator/g_fc{i + 1}/bias") for i in range(n)]
        self.nhidden = int(self.w[0].shape[1])
        self._check_shape()
        self.gamma, self.beta, self.moving_mean, self.moving_variance = ([f32(f"{_bn_name(k)}/{v}") for k in range(n - 1)]
                                                                         for v in ("gamma", "beta", "moving_mean", "moving_variance"))
        ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self._wp, self._bp = ptrs(self.w), ptrs(self.b)
        self._gp, self._betap = ptrs(self.gamma), ptrs(self.beta)
        self._mmp, self._mvp = ptrs(self.moving_mean), ptrs(self.moving_variance)
        self._ws = _Scratch(pad=4)

    def _shape_ok(self):
        return self.w[0].shape[0] == 2 and self.w[-1].shape[1] == 2 and 2 <= self.nlayers <= 6

    def _check_shape(self):
        if self.nhidden > 64 or not self._shape_ok():
            raise L.CgsError(f"MLPGenerator: unsupported shape (2 -> {self.nhidden} x {self.nlayers - 1} -> 2; need nhidden <= 64, 2..6 layers)")

    @staticmethod
    def init_params(seed, nhidden=64, nlayers=6):
        """Seeded TF defaults as host arrays: glorot-uniform kernels and zero biases (tf.layers.dense), gamma 1, beta 0, moving mean 0,
        moving variance 1 (tf.contrib.layers.batch_norm)."""
        P = _dense_init("generator/g_fc", [2] + [nhidden] * (nlayers - 1) + [2], seed)
        for k in range(nlayers - 1):
            one, zero = np.ones(nhidden, np.float32), np.zeros(nhidden, np.float32)
            P.update({f"{_bn_name(k)}/gamma": one, f"{_bn_name(k)}/beta": zero.copy(),
                      f"{_bn_name(k)}/moving_mean": zero.copy(), f"{_bn_name(k)}/moving_variance": one.copy()})
        return P

    @classmethod
    def init(cls, seed, nhidden=64, nlayers=6, device="cuda:0"):
        return cls(cls.init_params(seed, nhidden, nlayers), device)

    @classmethod
    def from_params(cls, params, device="cuda:0"):
        """From a ``{name: array}`` map such as ``checkpoint.load`` returns; other (e.g. discriminator/...) names are ignored."""
        return cls(params, device)

    def params(self):
        """{TF variable name: device tensor} -- the G half of a synthetic/main.py checkpoint."""
        P = {}
        for i in range(self.nlayers):
            P[f"generator/g_fc{i + 1}/kernel"], P[f"generator/g_fc{i + 1}/bias"] = self.w[i], self.b[i]
        for k in range(self.nlayers - 1):
            for v, ts in (("gamma", self.gamma), ("beta", self.beta), ("moving_mean", self.moving_mean), ("moving_variance", self.moving_variance)):
                P[f"{_bn_name(k)}/{v}"] = ts[k]
        return P

    def _workspace(self, B, with_backward):
        return self._ws.get(self._ws_bytes(B, with_backward), self.dev)

    def _ws_bytes(self, B, with_backward):
        return int(L.load().cgs_mlp2d_gen_ws_bytes(B, self.nlayers, int(with_backward)))

    def generate(self, z, is_training=True, batch_stats=False):
        """G(z) as a device [B,2] tensor.  Training mode (``gan.generates``): batch statistics, moving averages updated in place;
        inference mode (``gan.fake_samples``, GAN.py:105): the moving statistics.  ``batch_stats=True`` (training mode) also returns
        the [nlayers-1, 2, nhidden] (mean, biased variance) of every BN layer."""
        zd = _upload(z, self.dev)
        B = zd.shape[0]
        x = torch.empty((B, 2), dtype=torch.float32, device=self.dev)
        st = torch.empty((self.nlayers - 1, 2, self.nhidden), dtype=torch.float32, device=self.dev) if batch_stats else None
        ws = self._workspace(B, False)
        L.call(self._entry, self._wp, self._bp, self._gp, self._betap, self._mmp, self._mvp, self.nlayers, self.nhidden,
               zd.data_ptr(), x.data_ptr(), B, int(bool(is_training)), self.EPS, None if st is None else st.data_ptr(),
               ws.data_ptr(), ws.numel() * 4, _stream(self.dev))
        return (x, st) if batch_stats else x


class WideMLPGenerator(MLPGenerator):
    """``MLPGenerator`` for 65..256 hidden units (the 25-Gaussians runs: 256 x 6), same surface: the forward in both modes on sample tiles,
    the hidden -> hidden layers on the fp32 MFMA with the weights streamed from L2, the batch statistics combined from fixed 32-row groups
    in row order (csrc/mlp2d_wide_gen.hip; deterministic).  ``GStep`` does not take it: the G update at this width is ``WideGStep``."""

    _entry = "cgs_mlp2d_wide_gen_fwd"

    def _check_shape(self):
        if self.nhidden <= 64:
            raise L.CgsError(f"WideMLPGenerator: generator has {self.nhidden} hidden units; up to 64 units the generator is MLPGenerator "
                             "(mlp_generator() picks the class by width)")
        if self.nhidden > 256 or not self._shape_ok():
            raise L.CgsError(f"WideMLPGenerator: unsupported shape (2 -> {self.nhidden} x {self.nlayers - 1} -> 2; need 65 <= nhidden <= 256, 2..6 layers)")

    @staticmethod
    def init_params(seed, nhidden=256, nlayers=6):
        return MLPGenerator.init_params(seed, nhidden, nlayers)

    @classmethod
    def init(cls, seed, nhidden=256, nlayers=6, device="cuda:0"):
        return cls(cls.init_params(seed, nhidden, nlayers), device)

    def _ws_bytes(self, B, with_backward):
        if with_backward:
            raise L.CgsError("WideMLPGenerator: the G step at 65..256 hidden units is not built (the forward keeps what it will need)")
        return int(L.load().cgs_mlp2d_wide_gen_ws_bytes(B, self.nlayers, self.nhidden))


def mlp_generator(params, device="cuda:0"):
    """The generator for this checkpoint's width: ``MLPGenerator`` up to 64 hidden units, ``WideMLPGenerator`` above."""
    nh = int(np.asarray(params["generator/g_fc1/kernel"]).shape[1])
    return (MLPGenerator if nh <= 64 else WideMLPGenerator)(params, device)


class GStep:
    """The generator update g_optim (synthetic/GAN.py:83-101, run at synthetic/main.py:379-380): gradients of ``generates`` w.r.t.
    g_vars (the g_fc kernels and biases only -- the BN gamma / beta do not carry 'g_' in their names) against a caller-supplied
    grad_plugin [B,2], then GradientDescentOptimizer(lrg) IN PLACE on the ``MLPGenerator``'s tensors.  Its training-mode forward moves
    the BN moving averages once more, like the reference's g_optim run."""

    _entry = "cgs_mlp2d_g_step"

    def __init__(self, generator, lrg=5e-3):                          # synthetic/main.py:38 (--lrg 5e-3)
        self.G, self.lrg = generator, float(lrg)
        self.gw = [torch.zeros_like(t) for t in generator.w]
        self.gb = [torch.zeros_like(t) for t in generator.b]
        n = generator.nlayers
        self._gwp = (C.c_void_p * n)(*[t.data_ptr() for t in self.gw])
        self._gbp = (C.c_void_p * n)(*[t.data_ptr() for t in self.gb])

    def _workspace(self, B):
        return self.G._workspace(B, True)

    def _run(self, z, grad_plugin, lr, want_x=False):
        G = self.G
        zd, gd = _upload(z, G.dev), _upload(grad_plugin, G.dev)
        B = zd.shape[0]
        if tuple(gd.shape) != (B, 2):
            raise L.CgsError(f"{type(self).__name__}: grad_plugin shape {tuple(gd.shape)} != ({B}, 2)")
        ws = self._workspace(B)
        x = torch.empty((B, 2), dtype=torch.float32, device=G.dev) if want_x else None
        L.call(self._entry, G._wp, G._bp, G._gp, G._betap, G._mmp, G._mvp, G.nlayers, G.nhidden, zd.data_ptr(), gd.data_ptr(), B,
               G.EPS, float(lr), self._gwp, self._gbp, None if x is None else x.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream(G.dev))
        return x

    def grads(self, z, grad_plugin):
        """([dW...], [db...]) device tensors; the weights stay as they are (the moving averages still move: the forward runs)."""
        self._run(z, grad_plugin, 0.0)
        return self.gw, self.gb

    def step(self, z, grad_plugin, want_x=False):
        """One SGD step of G; ``want_x``: also return G(z) [B,2] of the step's own forward (before the update)."""
        return self._run(z, grad_plugin, self.lrg, want_x)


class WideGStep(GStep):
    """``GStep`` for a ``WideMLPGenerator`` (65..256 hidden units; the 25-Gaussians runs: 256 x 6), same surface, same in-place update:
    the wide forward, then one launch per BN layer back down the net on the same sample tiles, the batch sums of the BN backward from
    fixed 32-row groups in row order, the hidden -> hidden weight gradients as MFMA products over sample chunks of a size fixed by the
    batch alone, added in chunk order (csrc/mlp2d_wide_gstep.hip; deterministic).  The step keeps its own workspace, whose first bytes
    are the forward's; the generator's stays the forward-only one."""

    _entry = "cgs_mlp2d_wide_g_step"

    def __init__(self, generator, lrg=5e-3):
        if not isinstance(generator, WideMLPGenerator):
            raise L.CgsError(f"WideGStep: generator has {generator.nhidden} hidden units; up to 64 units the G step is GStep "
                             "(g_stepper() picks the class by width)")
        super().__init__(generator, lrg)
        self._ws = _Scratch(pad=4)

    def _workspace(self, B):
        G = self.G
        return self._ws.get(int(L.load().cgs_mlp2d_wide_g_step_ws_bytes(B, G.nlayers, G.nhidden)), G.dev)


def g_stepper(generator, lrg=5e-3):
    """The G update for this generator's width: ``GStep`` up to 64 hidden units, ``WideGStep`` above."""
    return (WideGStep if isinstance(generator, WideMLPGenerator) else GStep)(generator, lrg)


class GanTrainer:
    """The iteration loop of synthetic/main.py:350-395 with d_steps = g_steps = 1, on the device, in the reference's order and with its
    host RNG draws (``data`` / ``noise`` consume the global numpy stream exactly as ToyDataset / NoiseDataset do there):

    * train:     real, z -> D step on (real, G(z))                        then  z' -> D saliency of G(z') -> G step on (z', saliency)
    * calibrate: real, z -> D step on (real, G(z))
    * shape:     real, z -> D step on (real, probabilistic refinement of G(z))   (``refiner``: a ``synthetic.Refiner``)
    * test:      real, z drawn, nothing trained

    G runs in training mode wherever the reference runs ``gan.generates``: once in the D step and twice (same z) in the G step, so the
    BN moving averages move three times per train iteration.  Nothing inside an iteration waits for the device; the last D losses stay in
    the device tensor ``d_loss`` (d_loss_real, d_loss_fake)."""

    MODES = ("train", "calibrate", "shape", "test")

    def __init__(self, G, D, data, noise=None, batch_size=1000, lrd=1e-2, lrg=5e-3, refiner=None):
        _need_narrow(D, "GanTrainer")
        self.G, self.D, self.data = G, D, data
        self.noise = noise if noise is not None else NoiseDataset()
        self.batch_size = int(batch_size)
        self.dshaper, self.gstep = DShaper(D, lrd), GStep(G, lrg)
        self.d_loss = self.dshaper.loss
        self.refiner = refiner
        self.eval_noise = self.eval_batch = self.target_batch = None

    def prepare_eval(self, eval_size=10000):
        """main.py:297-300: eval noise, its training-mode G batch, then the target batch (same draws, same order)."""
        self.eval_noise = self.noise.next_batch(eval_size)
        self.eval_batch = self.G.generate(self.eval_noise)
        self.target_batch = self.data.next_batch(eval_size)
        return self.eval_batch, self.target_batch

    def _refine(self, fake):
        """refiner.manipulate_sample(fake, 'probabilistic') (sampling/refiner_cpu.py:19-76) with the baseline and the trajectory kept on
        the device: the same draws (real batch, then the per-sample step pick), no host round trip."""
        r, D, dev = self.refiner, self.D, self.D.dev
        n = fake.shape[0]
        real = _upload(r.data.next_batch(n), dev)
        real_sig, _ = D.sigmoid_and_saliency(real, want_saliency=False)
        _, _, traj = D.refine(fake, real_sig.mean(), r.forward_steps, r.step_size, r.method, want_traj=True)
        pick = torch.from_numpy(np.random.randint(r.forward_steps + 1, size=n)).pin_memory().to(dev, non_blocking=True)
        return traj[torch.arange(n, device=dev), pick]

    def iteration(self, mode="train"):
        if mode not in self.MODES:
            raise NotImplementedError(mode)
        B = self.batch_size
        real = _upload(self.data.next_batch(B), self.D.dev)              # main.py:356-357
        z = self.noise.next_batch(B)
        if mode in ("train", "calibrate"):
            self.dshaper.step(real, self.G.generate(z))
        elif mode == "shape":
            if self.refiner is None:
                raise ValueError("shape mode needs a refiner")
            self.dshaper.step(real, self._refine(self.G.generate(z)))
        if mode == "train":                                              # main.py:376-380
            z = _upload(self.noise.next_batch(B), self.G.dev)
            _, grad_default = self.D.sigmoid_and_saliency(self.G.generate(z))      # grad_default = d g_loss / d generates (1/B inside)
            self.gstep.step(z, grad_default)
        return self.d_loss

    def run(self, niters, mode="train", save_every=0, save_prefix=None, eval_every=1000, on_eval=None):
        """``niters`` iterations i = 0 .. niters-1.  Like main.py:384-395: at i % eval_every == 0 a train run regenerates the eval batch
        (training-mode G on the eval noise, after ``prepare_eval``) and ``on_eval(i, self)`` is called; with ``save_every`` the {G, D}
        checkpoint ``<save_prefix>-<i>.safetensors`` is written at every i % save_every == 0, i > 0 (so the iteration-1000 checkpoint
        is the state after iterations 0 .. 1000).  Returns the paths written.

        A bit-equal host RNG stream and bit-equal moving statistics (against a reference run with its evaluation) need ``prepare_eval()``
        BEFORE ``run()``: main.py draws the eval noise and the target batch before its loop (:297-300), and every eval-batch regeneration
        is one more training-mode G call.  Without it the loop draws only the iterations' own batches."""
        written = []
        for i in range(niters):
            self.iteration(mode)
            if i % eval_every == 0:
                if mode == "train" and self.eval_noise is not None:
                    self.eval_batch = self.G.generate(self.eval_noise)
                if on_eval is not None:
                    on_eval(i, self)
            if save_every and i % save_every == 0 and i > 0:
                path = f"{save_prefix}-{i}.safetensors"
                self.save(path)
                written.append(path)
        return written

    def save(self, path):
        CK.save(path, {**self.G.params(), **self.D.params()})

    @staticmethod
    def load(path, device="cuda:0"):
        """-> (MLPGenerator, MLPDiscriminator) from a {G, D} checkpoint (ours, or a converted synthetic/main.py one)."""
        P = CK.load(path)
        return MLPGenerator.from_params(P, device), MLPDiscriminator(P, device)


class WideGanTrainer(GanTrainer):
    """``GanTrainer`` for a discriminator of any supported width (``d_shaper``) and either generator class.  calibrate, shape and test run
    whatever the widths (the reference's 25-Gaussians command lines: 256 x 6 for both nets, from a checkpoint); train needs the G update and
    so a generator of at most 64 units, with the narrow ``GStep`` and the saliency of whichever D there is."""

    def __init__(self, G, D, data, noise=None, batch_size=1000, lrd=1e-2, lrg=5e-3, refiner=None):
        self.G, self.D, self.data = G, D, data
        self.noise = noise if noise is not None else NoiseDataset()
        self.batch_size = int(batch_size)
        self.dshaper = d_shaper(D, lrd)
        self.gstep = None if isinstance(G, WideMLPGenerator) else GStep(G, lrg)
        self.d_loss = self.dshaper.loss
        self.refiner = refiner
        self.eval_noise = self.eval_batch = self.target_batch = None

    def iteration(self, mode="train"):
        if mode == "train" and self.gstep is None:                       # before any draw: the host RNG stream stays where it was
            raise L.CgsError(f"WideGanTrainer: train mode needs the G step, which is not built for a generator of {self.G.nhidden} hidden "
                             "units (65..256: forward only); calibrate, shape and test run")
        return super().iteration(mode)

    @staticmethod
    def load(path, device="cuda:0"):
        """-> (MLPGenerator or WideMLPGenerator, MLPDiscriminator) from a {G, D} checkpoint, each class by its width."""
        P = CK.load(path)
        return mlp_generator(P, device), MLPDiscriminator(P, device)


class Gan2DTrainer(WideGanTrainer):
    """The loop for any supported widths of G and D in all four modes (``g_stepper``, ``d_shaper``): at the reference's 25-Gaussians
    widths (256 x 6 for both nets) ``train`` runs generate -> wide D step -> generate -> saliency -> wide G step, with the reference's
    host RNG draws in its order and the moving averages moving three times per iteration.  ``WideGanTrainer`` keeps its refusal of train
    with a wide G; this class is the one that trains there."""

    def __init__(self, G, D, data, noise=None, batch_size=1000, lrd=1e-2, lrg=5e-3, refiner=None):
        super().__init__(G, D, data, noise, batch_size, lrd, lrg, refiner)
        self.gstep = g_stepper(G, lrg)
