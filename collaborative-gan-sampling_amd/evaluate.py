"""Collaborative sampling = refine, then accept/reject: the step right after the hot path
(nsgan/GAN.py:398-426 "collaborate", synthetic/main.py:232-253).

``collaborate`` is the fill loop both reference drivers run: proposals come from the refiner, their discriminator
scores drive the MH independence chain (``IndependenceSampler``, thinning T=20), and accepted samples fill an
evaluation set of ``eval_size``.  The proposals here come from the device engine (one refine call per batch, images
and sigmoids read back once per batch); the chain is host code exactly like the reference's.
"""
import numpy as np

MIN_EFFICIENCY = 0.2     # nsgan/GAN.py:18


class _FillCounter:
    """The counter rule of the reference's fill loops, stated once (nsgan/GAN.py:311-346,348-376,398-426; synthetic/main.py:149-169,
    182-202,229-253).  ``cnt`` rows accepted, ``cnt_propose`` proposals made: the first pass's ``eval_size`` proposals are the counter's
    start (``start``).  While ``cnt_propose < max_propose`` a batch goes through the sampler; past that budget (GAN.py:283,323,357,410)
    it is taken whole.  ``productive_only`` (main.py:163-169,196-202,245-251): a batch that yields nothing is not counted as proposed."""

    def __init__(self, eval_size, min_efficiency=None, productive_only=False):
        self.eval_size, self.productive_only = eval_size, productive_only
        self.cnt, self.cnt_propose = 0, eval_size
        self.max_propose = eval_size / min_efficiency if min_efficiency else float("inf")

    def start(self, n):
        """The first pass (``base``) yielded n rows."""
        self.cnt = n

    def through(self):
        """Does the batch at hand go through the sampler (True), or is it taken whole?"""
        return self.cnt_propose < self.max_propose

    def through_ahead(self, i, b):
        """``through()`` for the i-th batch of b proposals after the first pass, known before any batch is counted: every batch moves
        the proposal counter by b (GAN.py:339,375,426; not so with ``productive_only``, whose loops do not draw ahead)."""
        return self.eval_size + i * b < self.max_propose

    def add(self, n, proposed):
        """A batch of ``proposed`` proposals yielded n rows (taken whole: n = proposed) -> is the pool full?"""
        self.cnt += n
        if n > 0 or not self.productive_only:
            self.cnt_propose += proposed
        return self.cnt >= self.eval_size

    def add_round(self, counts, b):
        """``add`` for a round's batches of b in order, up to the one that fills the pool -> its index, None if the round does not."""
        for j, n in enumerate(counts):
            if self.add(int(n), b):
                return j
        return None

    @property
    def full(self):
        return self.cnt >= self.eval_size

    @property
    def efficiency(self):
        return self.cnt / self.cnt_propose


def _host_fill(name, seed, accepted, propose, score, eval_size, base, min_efficiency, count_only_productive, max_rounds):
    """The one-batch-at-a-time fill loop both host legs run.  ``seed()`` seeds the sampler; ``accepted(batch, sigmoids)`` -> the rows of
    the batch it lets through."""
    C = _FillCounter(eval_size, min_efficiency, count_only_productive)
    out = None
    seed()
    if base is not None:
        acc = accepted(base[0], base[1])
        if acc.shape[0] > 0:
            out = np.empty((eval_size,) + acc.shape[1:], dtype=acc.dtype)
            k = min(acc.shape[0], eval_size)
            out[:k] = acc[:k]
        C.start(acc.shape[0])
    rounds = 0
    while not C.full:
        rounds += 1
        if rounds > max_rounds:
            raise RuntimeError("%s: no sample accepted in %d rounds" % (name, max_rounds))
        batch = propose()
        B = batch.shape[0]
        if out is None:
            out = np.empty((eval_size,) + batch.shape[1:], dtype=np.float32)
        acc = accepted(batch, score(batch)) if C.through() else batch               # (else: too inefficient, take the batch as is)
        n = acc.shape[0]
        if n > 0:
            k = min(n, eval_size - C.cnt)
            out[C.cnt:C.cnt + k] = acc[:k]
        C.add(n, B)
    return out, C.efficiency


def collaborate(propose, score, mh_sampler, eval_size, real_sigmoid_mean, base=None, min_efficiency=None,
                count_only_productive=False, max_rounds=100000):
    """Fill ``eval_size`` accepted samples.

    propose()            -> refined batch as ndarray [B, ...]           (g_refine_detem / manipulate_sample)
    score(batch)         -> discriminator sigmoids [B, 1]               (fake_sigmoids)
    base                 -> optional (samples, sigmoids) for the first MH pass (nsgan uses the *standard* samples
                            there, nsgan/GAN.py:402, quirk Q10; synthetic uses the refined evaluation batch)
    min_efficiency       -> nsgan/GAN.py:283,410: once the proposals exceed eval_size over min_efficiency, stop rejecting
                            and take whole batches
    count_only_productive-> synthetic/main.py:251: the proposal counter only advances for batches that yielded samples
    Returns (samples [eval_size, ...], efficiency = accepted / proposed)."""
    return _host_fill("collaborate", lambda: mh_sampler.set_score_curr(real_sigmoid_mean), mh_sampler.sampling,    # nsgan/GAN.py:401
                      propose, score, eval_size, base, min_efficiency, count_only_productive, max_rounds)


def engine_proposer(engine, steps, rate, rng=None, **refine_kw):
    """propose() / score() closures over a ``RefineEngine``: z ~ U(-1,1) (nsgan/GAN.py:408), refine on device,
    read the images back; score = sigmoid(D(images)) with D on batch statistics (nsgan/GAN.py:154-155)."""
    import torch
    rng = rng or np.random
    zdim = engine.A["z_dim"]

    def propose():
        z = torch.from_numpy(rng.uniform(-1, 1, [engine.B, zdim]).astype(np.float32)).to(engine.dev)
        return engine.refine_from_z(z, steps, rate, **refine_kw)[0].cpu().numpy()

    def score(batch):
        x = torch.from_numpy(np.ascontiguousarray(batch, dtype=np.float32)).to(engine.dev)
        return engine.score(x).cpu().numpy()                 # float32 [B, 1]: what sess.run(fake_sigmoids) hands the chain (nsgan/GAN.py:409)

    return propose, score


# ------------------------------------------------------------------------------------------------------------------------------
# The same fill loop with G logical batches per device round (SURVEY.md 8f-1 on the fast path).
#
# nsgan/GAN.py:398-426 runs one batch_size-64 batch per iteration (nsgan/main.py:32): sess.run(g_refine_detem), sess.run(fake_sigmoids),
# the host chain.  At 64 samples every launch is latency-bound.  Here a ROUND is G such iterations: their z batches are drawn in the
# reference's order, refined in ONE engine call (``bn_groups`` = G: D's batch statistics per logical batch, nsgan/GAN.py:175), scored on
# the device the same way, and copied to pinned host memory once; the host chain walks round r while the device refines round r + 1.
# The global numpy stream is consumed exactly as the reference's loop consumes it -- per iteration the z draw, then one uniform per
# proposal for the chain (drawn ahead, handed to ``IndependenceSampler.walk``) -- and is rewound at the end to where the reference's
# loop would have left it, so the accepted set, the efficiency and every later np.random draw are those of the one-batch-at-a-time loop.
class FusedProposer:
    """G logical batches of ``batch`` samples per round on a ``model.GAN``'s engines; ``depth`` rounds in flight (one engine + HIP
    stream + pinned result buffers each)."""

    def __init__(self, gan, steps, rate, batch=None, groups=32, depth=2, method="momentum", mode="deterministic", contraction="f32",
                 use_graph=True, indices=None, features=False):
        import torch
        from .engine import RefineEngine
        self.torch = torch
        self.b, self.G = int(batch or gan.batch_size), int(groups)
        self.steps, self.rate, self.method, self.mode = steps, rate, method, mode
        self.dev = gan.device
        A = gan.A
        self.zdim = A["z_dim"]
        n = self.b * self.G
        P = gan.build_variables()
        # (own engines rather than gan.engine()'s cached one: every round in flight needs its own activation buffers)
        self.engines = [RefineEngine(A, P, n, self.dev, use_graph=use_graph, bn_groups=self.G, contraction=contraction) for _ in range(depth)]
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(depth)]
        img = (n,) + tuple(A["img"])
        self.z_host = [torch.empty((n, self.zdim), dtype=torch.float32).pin_memory() for _ in range(depth)]
        self.z_dev = [torch.empty((n, self.zdim), dtype=torch.float32, device=self.dev) for _ in range(depth)]
        self.img_host = [torch.empty(img, dtype=torch.float32).pin_memory() for _ in range(depth)]
        self.sig_host = [torch.empty((n, 1), dtype=torch.float32).pin_memory() for _ in range(depth)]
        self.sig_dev = [torch.empty((n, 1), dtype=torch.float32, device=self.dev) for _ in range(depth)]
        self.done = [torch.cuda.Event() for _ in range(depth)]
        # features=True: every launch also keeps D's features of the round (engine.score_with_features) in a per-slot DEVICE buffer;
        # nothing more is copied to the host -- ``accumulate`` adds chosen rows of it to a metrics.PoolMoments on the slot's stream
        self.feat_dev = None
        if features:
            self.feat_width = self.engines[0].feature_width()
            self.feat_dev = [torch.empty((n, self.feat_width), dtype=torch.float32, device=self.dev) for _ in range(depth)]
        self.depth, self.launched = depth, 0
        self.img_dev = [None] * depth              # the engine's own image buffer of the slot's latest round (valid until the slot is launched again)
        self.indices = None
        if mode == "probabilistic":      # the reference bakes ONE draw of size batch_size into the graph, for every batch (collaborator.py:54-56)
            one = np.asarray(indices) if indices is not None else np.random.randint(steps + 1, size=self.b)
            self.indices = np.tile(one, self.G)

    def launch(self, z, refine=True, calibration=None, to_host=True):
        """Queue one round on the next slot: z [G*b, z_dim] (host array) -> images + sigmoids in the slot's pinned buffers.
        ``refine=False``: the standard samples instead (fake_images / fake_sigmoids, nsgan/GAN.py:153-155).  Returns the slot.
        ``calibration`` (a metrics.CalibrationStats, optional): the round's sigmoids are added to it with label 0 on the slot's stream,
        from the device buffer the scoring pass wrote -- with ``refine=False`` the ``sigmoid_standard`` half of nsgan/GAN.py:287-301;
        nothing more is copied to the host.  ``to_host=False``: neither images nor sigmoids are copied to the pinned buffers (``result`` then
        only waits); the round is read on the device, from ``img_dev[slot]`` / ``sig_dev[slot]`` (``reject_fill_fused``)."""
        torch = self.torch
        k = self.launched % self.depth
        self.launched += 1
        self.z_host[k].numpy()[...] = z
        e, st = self.engines[k], self.streams[k]
        with torch.cuda.stream(st):
            self.z_dev[k].copy_(self.z_host[k], non_blocking=True)
            if refine:
                kw = dict(mode="probabilistic", indices=self.indices) if self.mode == "probabilistic" else {}
                img = e.refine_from_z(self.z_dev[k], self.steps, self.rate, method=self.method, **kw)[0]
            else:
                img = e.generate(self.z_dev[k])
            self.img_dev[k] = img
            if to_host:
                self.img_host[k].copy_(img, non_blocking=True)    # (before score(): D's forward re-uses no G buffer, but keep the order plain)
            if self.feat_dev is not None:
                e.score_with_features(img, out=self.sig_dev[k], feat_out=self.feat_dev[k])
            else:
                e.score(img, out=self.sig_dev[k])
            if to_host:
                self.sig_host[k].copy_(self.sig_dev[k], non_blocking=True)
            self.done[k].record(st)
            if calibration is not None:                           # (behind ``done``: result(k) does not wait for it)
                calibration.update(self.sig_dev[k], 0)
        return k

    def result(self, k):
        """Wait for slot k -> (images [G*b, ...], sigmoids [G*b, 1]) float32 host arrays (views of the pinned buffers: valid until
        the slot is launched again)."""
        self.done[k].synchronize()
        return self.img_host[k].numpy(), self.sig_host[k].numpy()

    def accumulate(self, k, rows, moments):
        """Queue ``moments.update`` of rows ``rows`` (host integers into the slot's G*b samples) of slot k's features on the slot's
        stream.  Valid from ``result(k)`` until the slot is launched again."""
        if self.feat_dev is None:
            raise ValueError("FusedProposer(features=True) keeps the features accumulate() reads")
        with self.torch.cuda.stream(self.streams[k]):
            moments.update(self.feat_dev[k], rows)

    def _real_rounds(self, x, each):
        """A real evaluation set in rounds of ``G`` whole batches: ``each(i, m, round)`` on slot 0's stream with the round starting at
        x[i] as a device tensor, of which the first m rows are x's -- a last partial round is padded with repeats of whole batches."""
        torch = self.torch
        n = self.b * self.G
        N = x.shape[0]
        if N % self.b:
            raise ValueError(f"{N} real samples are not whole batches of {self.b}")
        for i in range(0, N, n):
            xb = np.asarray(x[i:i + n], dtype=np.float32)
            m = xb.shape[0]
            if m < n:
                xb = np.concatenate([xb] + [xb[:self.b]] * ((n - m) // self.b))
            with torch.cuda.stream(self.streams[0]):
                each(i, m, torch.from_numpy(np.ascontiguousarray(xb)).to(self.dev))

    def real_moments(self, x, moments):
        """Add D's features of a real evaluation set to ``moments``, ``batch`` samples per set of batch statistics like ``score_real``
        (same padding of a last partial round; the padding batches are left out).  Returns ``moments``."""
        e, n = self.engines[0], self.b * self.G
        self._real_rounds(x, lambda i, m, xd: moments.update(e.score_with_features(xd)[1], None if m == n else np.arange(m)))
        return moments

    def score_real(self, x, chunk=None, calibration=None):
        """np.mean-able sigmoids of a real evaluation set, scored ``batch`` samples at a time like nsgan/GAN.py:388-390
        (``G`` batches per launch; x.shape[0] must be a multiple of ``batch``; a last partial round is padded with repeats
        of whole batches, whose scores are dropped).  ``calibration`` (a metrics.CalibrationStats, optional): the same scores, padding
        left out, are added to it with label 1 on the device (``sigmoid_real`` of nsgan/GAN.py:287-289)."""
        e = self.engines[0]
        out = np.empty((x.shape[0], 1), dtype=np.float32)

        def each(i, m, xd):
            s = e.score(xd)
            if calibration is not None:
                calibration.update(s[:m], 1)
            out[i:i + m] = s.cpu().numpy()[:m]
        self._real_rounds(x, each)
        return out


_UNIFORM = lambda b: np.random.uniform(0, 1, size=b)                    # idpsampler.py:50, one per proposal
_RAND = lambda b: np.random.rand(b)                                     # rejector.py:33, one per proposal


def _draw_round(counter, drawn, G, b, zdim, draw, blank=None):
    """One round of G logical batches of b from the global numpy stream, consumed per batch as the reference's loop consumes it
    (nsgan/GAN.py:321-323,355-357,408-410): the z draw; then, if the batch will go through the sampler -- known ahead from ``drawn``, the
    batches drawn before this round (``counter.through_ahead``) -- the leg's per-proposal ``draw(b)``, else ``blank`` and no draw; then a
    snapshot of the stream, where the one-batch-at-a-time loop stands after this batch.
    -> (z [G * b, zdim] fp32, the uniforms per batch, the take-whole flag per batch, the stream state after each batch)"""
    zs, us, flags, states = [], [], [], []
    for i in range(drawn, drawn + G):
        zs.append(np.random.uniform(-1, 1, [b, zdim]).astype(np.float32))
        through = counter.through_ahead(i, b)
        us.append(draw(b) if through else blank)
        flags.append(not through)
        states.append(np.random.get_state())
    return np.concatenate(zs), us, flags, states


class _FusedFill:
    """What the fused loops share around their per-round work: the argument checks, the counter, the rounds drawn ahead and in flight, the
    tail; and, for the loops whose pool stays on the device (``pools=True``), the pool with D's features (``moments``) and scores
    (``calibration``) of its rows beside it, and the event that orders a round's device work behind the round before, whichever stream
    that ran on.  ``name``: the public function, for its messages; ``draw`` / ``blank``: ``_draw_round``'s."""

    def __init__(self, name, proposer, eval_size, base, min_efficiency, max_rounds, moments, draw, blank=None, base_form="samples", pools=False,
                 calibration=None):
        if moments is not None:
            if proposer.feat_dev is None:
                raise ValueError(f"{name}(moments=...) needs FusedProposer(features=True)")
            if base is not None and len(base) != 3:
                raise ValueError(f"{name}(moments=...): base must carry features too, as ({base_form}, sigmoids, features)")
        self.name, self.proposer, self.max_rounds, self.draw, self.blank = name, proposer, max_rounds, draw, blank
        self.moments, self.calibration = moments, calibration
        self.counter = _FillCounter(eval_size, min_efficiency)
        self.drawn = self.rounds = 0                   # logical batches drawn so far; rounds taken
        self.pending = []                              # rounds in flight: whatever ``launch`` returned, the slot first
        self.final_state = self.pool = self.chain = None
        self.t_wait = self.t_chain = 0.0
        if pools:
            import torch
            self.torch = torch
            new = lambda *row: torch.empty((eval_size,) + row, dtype=torch.float32, device=proposer.dev)
            self.pool = new(*proposer.engines[0].A["img"])
            self.feat_pool = new(proposer.feat_width) if moments is not None else None
            self.sig_pool = new(1) if calibration is not None else None

    def next_round(self, launch):
        """The head of the loop: keep ``depth`` rounds in flight -- ``launch(z, uniforms, flags, states)`` queues one just drawn and
        returns what the loop will want of it, the slot first -- and hand out the oldest."""
        self.rounds += 1
        if self.rounds > self.max_rounds:
            raise RuntimeError("%s: no sample accepted in %d rounds" % (self.name, self.max_rounds))
        P = self.proposer
        while len(self.pending) < P.depth:
            drawn = _draw_round(self.counter, self.drawn, P.G, P.b, P.zdim, self.draw, self.blank)
            self.drawn += P.G
            self.pending.append(launch(*drawn))
        return self.pending.pop(0)

    def count_round(self, counts, states):
        """Count a round's batches -> the one that fills the pool (the stream will be rewound to where the reference's loop stands after
        it), or None."""
        j = self.counter.add_round(counts, self.proposer.b)
        if j is not None:
            self.final_state = states[j]
        return j

    def on_device(self, x):
        torch = self.torch
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return t.to(self.proposer.dev, torch.float32).contiguous()

    def base_sources(self, base):
        """-> (samples, sigmoids, features or None) of ``base`` on the device"""
        return self.on_device(base[0]), self.on_device(base[1]), self.on_device(base[2]) if self.moments is not None else None

    def slot_sources(self, slot):
        P = self.proposer
        return P.img_dev[slot], P.sig_dev[slot], P.feat_dev[slot] if self.moments is not None else None

    def into_pools(self, imgs, sigs, feats):
        """-> the (source, pool) pairs a round's rows are copied along"""
        return [(src, pool) for src, pool in ((imgs, self.pool), (feats, self.feat_pool), (sigs, self.sig_pool)) if pool is not None]

    def chain_behind(self, stream):
        self.chain = self.torch.cuda.Event()
        self.chain.record(stream)

    def finish(self, stats, **seconds):
        """The tail -> the efficiency."""
        C, P = self.counter, self.proposer
        for entry in self.pending:                     # rounds drawn ahead that the reference's loop never reaches: drained, discarded
            P.result(entry[0])
        if self.final_state is not None:
            np.random.set_state(self.final_state)      # the global stream where the one-batch-at-a-time loop leaves it
        if self.pool is not None:
            self.torch.cuda.current_stream(P.dev).wait_event(self.chain)
            if self.moments is not None:
                self.moments.update(self.feat_pool)
            if self.calibration is not None:
                self.calibration.update(self.sig_pool, 0)
        if stats is not None:
            proposed = C.cnt_propose - C.eval_size
            stats.update(rounds=self.rounds, proposed=proposed, discarded_batches=self.drawn - proposed // P.b, **seconds)
        return C.efficiency


def collaborate_fused(proposer, mh_sampler, eval_size, real_sigmoid_mean, base=None, min_efficiency=None, max_rounds=100000, stats=None,
                      moments=None):
    """``collaborate`` (count_only_productive=False: the nsgan form, nsgan/GAN.py:398-426) over a ``FusedProposer``.
    ``stats`` (dict, optional) receives rounds / proposals / host-chain seconds / device-wait seconds.
    Returns (samples [eval_size, ...], efficiency) -- bit-identical to ``collaborate`` fed by one-batch-at-a-time proposals of the
    same engine arithmetic, global numpy stream included.
    ``moments`` (a metrics.PoolMoments, optional; needs ``FusedProposer(features=True)``): D's features of exactly the rows copied
    into the result are added to it on the device, one update per round; ``base`` must then be (images, sigmoids, features).  The
    samples, the efficiency and every draw are those of the run without it."""
    import time
    F = _FusedFill("collaborate_fused", proposer, eval_size, base, min_efficiency, max_rounds, moments, _UNIFORM, base_form="images")
    b, G, C = proposer.b, proposer.G, F.counter
    out = None
    mh_sampler.set_score_curr(real_sigmoid_mean)                                   # nsgan/GAN.py:401
    if base is not None:
        if moments is None:
            acc = mh_sampler.sampling(base[0], base[1])
        else:                                                                       # (sampling() spelled out: the accepted ROWS are needed)
            base_rows = mh_sampler.walk(base[1])
            acc = np.asarray([base[0][i] for i in base_rows], dtype=np.float32)
        if acc.shape[0] > 0:
            out = np.empty((eval_size,) + acc.shape[1:], dtype=acc.dtype)
            k = min(acc.shape[0], eval_size)
            out[:k] = acc[:k]
            if moments is not None:
                import torch
                f = base[2] if isinstance(base[2], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(base[2], dtype=np.float32))
                moments.update(f.to(proposer.dev), np.asarray(base_rows[:k], dtype=np.int64))
        C.start(acc.shape[0])
    while not C.full:
        slot, us, flags, states = F.next_round(lambda z, *drawn: (proposer.launch(z), *drawn))
        t0 = time.perf_counter()
        imgs, sigs = proposer.result(slot)
        t1 = time.perf_counter()
        F.t_wait += t1 - t0
        if out is None:
            out = np.empty((eval_size,) + imgs.shape[1:], dtype=np.float32)
        taken = []                                     # rows of this round's slot copied into ``out`` (moments)
        for j in range(G):                             # the host chain, a round behind the device (one counter call per batch: it is timed)
            batch, cnt = imgs[j * b:(j + 1) * b], C.cnt
            if not flags[j]:
                # (a private copy of the batch's scores: the chain keeps a VIEW of the score it moved to -- idpsampler.py:52 -- and the
                # pinned buffer behind ``sigs`` is overwritten when its slot is launched again)
                rows = mh_sampler.walk(sigs[j * b:(j + 1) * b].copy(), us[j])
                n = len(rows)
                if n > 0:
                    k = min(n, eval_size - cnt)
                    out[cnt:cnt + k] = batch[rows[:k]]
                    if moments is not None:
                        taken.extend(j * b + r for r in rows[:k])
            else:                                                                   # too inefficient: take the batch as is
                n, k = b, min(b, eval_size - cnt)
                out[cnt:cnt + k] = batch[:k]
                if moments is not None:
                    taken.extend(range(j * b, j * b + k))
            if C.add(n, b):
                F.final_state = states[j]
                break
        if taken:                                      # (the slot is launched again at the top of the loop at the earliest)
            proposer.accumulate(slot, np.asarray(taken, dtype=np.int64), moments)
        F.t_chain += time.perf_counter() - t1
    return out, F.finish(stats, host_chain_s=F.t_chain, device_wait_s=F.t_wait)


# ------------------------------------------------------------------------------------------------------------------------------
# The DRS leg of the evaluation (nsgan/GAN.py:311-346, synthetic/main.py:149-169): the same fill loop with the Rejector in the chain's place.
def reject_fill(propose, score, rejector, eval_size, real_sigmoid_max, base=None, min_efficiency=None, count_only_productive=False,
                shift_percent=100.0, epsilon=1e-8, max_rounds=100000):
    """Fill ``eval_size`` samples by discriminator rejection sampling: the counterpart of ``collaborate``.

    propose()            -> a batch of standard samples as ndarray [B, ...]      (fake_images / gan.generates)
    score(batch)         -> discriminator sigmoids [B, 1]                        (fake_sigmoids)
    rejector             -> a ``sampling.Rejector``; its bound is seeded with ``real_sigmoid_max`` (np.amax(sigmoid_real), GAN.py:314)
    base                 -> optional (samples, sigmoids) for the first pass (the standard evaluation set, GAN.py:315, main.py:153)
    min_efficiency       -> GAN.py:283,323: once the proposals exceed eval_size over min_efficiency, stop rejecting and take whole batches
    count_only_productive-> main.py:163-169: the proposal counter only advances for batches that yielded samples
    shift_percent        -> 100.0 at every call site of the reference
    One deliberate difference: GAN.py:326 stores a batch's accepted rows only when something had been accepted before, which leaves
    rows of np.empty garbage in the evaluation set while the counter moves on.  The rows are stored always here: uninitialised memory
    defines no parity.
    Returns (samples [eval_size, ...], efficiency = accepted / proposed)."""
    return _host_fill("reject_fill", lambda: rejector.set_score_max(real_sigmoid_max),
                      lambda batch, sigmoids: rejector.sampling(batch, sigmoids, epsilon=epsilon, shift_percent=shift_percent),
                      propose, score, eval_size, base, min_efficiency, count_only_productive, max_rounds)


def reject_fill_fused(proposer, rejector, eval_size, real_sigmoid_max, base=None, min_efficiency=None, shift_percent=100.0, epsilon=1e-8,
                      max_rounds=100000, stats=None, moments=None, calibration=None):
    """``reject_fill`` (count_only_productive=False: the nsgan form, nsgan/GAN.py:311-346) over a ``FusedProposer`` and a
    ``sampling.DeviceRejector``: G logical batches of standard samples per round (``launch(..., refine=False)``), the accept decision
    and the compaction queued on the slot's stream behind the round, the pool on the device from start to end.  Per round the host
    receives the G accept counts and nothing else; no image, accepted or rejected, is copied to it.
    ``real_sigmoid_max``: a device tensor of the real scores (reduced on the device) or a host scalar / array.
    ``base``: (samples, sigmoids) of the standard evaluation set, device tensors or host arrays, decided as ONE batch (GAN.py:315);
    with ``moments`` it must be (samples, sigmoids, features).
    ``moments`` (a metrics.PoolMoments; needs ``FusedProposer(features=True)``) / ``calibration`` (a metrics.CalibrationStats): D's
    features / scores of exactly the rows of the returned pool are compacted beside it and added once, from the device, at the end
    (the scores with label 0).
    Returns (pool: device fp32 tensor [eval_size, ...], efficiency) -- the rows, their order, the efficiency, ``rejector.D_tilde_M``
    and the global numpy stream afterwards are those of ``reject_fill`` with a host ``Rejector`` fed the same scores one batch at a time."""
    import time
    F = _FusedFill("reject_fill_fused", proposer, eval_size, base, min_efficiency, max_rounds, moments, _RAND, pools=True, calibration=calibration)
    torch, b, G, dev, C = F.torch, proposer.b, proposer.G, proposer.dev, F.counter

    def compact_all(imgs, sigs, feats, offset, take_all=None):
        for src, pool in F.into_pools(imgs, sigs, feats):
            rejector.compact(src, pool, offset, take_all)

    rejector.set_score_max(real_sigmoid_max)                                           # nsgan/GAN.py:314
    if base is not None:
        imgs, sigs, feats = F.base_sources(base)
        _, counts, _ = rejector.decide_device(sigs, None, shift_percent, epsilon, groups=1)     # :315, the whole set as one batch
        compact_all(imgs, sigs, feats, 0)
        C.start(int(counts.cpu()[0]))
    F.chain_behind(torch.cuda.current_stream(dev))                                     # (the rounds run on the slots' streams)
    while not C.full:
        slot, us, flags, states = F.next_round(lambda z, *drawn: (proposer.launch(z, refine=False, to_host=False), *drawn))
        G1 = G - sum(flags)                            # the batches that go through the rejector come first: the counter only grows
        imgs, sigs, feats = F.slot_sources(slot)
        st = proposer.streams[slot]
        t0 = time.perf_counter()
        with torch.cuda.stream(st):                    # (behind the slot's ``done``: the same stream)
            st.wait_event(F.chain)                     # the decide + compact before this one, whichever stream it ran on
            mask = torch.zeros(b * G, dtype=torch.uint8, device=dev) if G1 < G else None
            if G1 > 0:
                m, counts, _ = rejector.decide_device(sigs[:G1 * b], np.concatenate(us[:G1]), shift_percent, epsilon, groups=G1)
                if mask is None:
                    mask = m
                else:
                    mask[:G1 * b].copy_(m)
            rejector.last_accept = mask
            compact_all(imgs, sigs, feats, min(C.cnt, eval_size), flags if G1 < G else None)
            accepted = counts.cpu().numpy() if G1 > 0 else np.zeros(0, dtype=np.int32)          # the round's only read-back
        F.t_wait += time.perf_counter() - t0
        j = F.count_round(list(accepted) + [b] * (G - G1), states)
        if j is not None and j < G1 - 1:               # the reference's loop stops here: later batches never reach its rejector
            with torch.cuda.stream(st):
                rejector.rewind_to(j)
        F.chain_behind(st)
    return F.pool, F.finish(stats, device_wait_s=F.t_wait)


# ------------------------------------------------------------------------------------------------------------------------------
# The Metropolis-Hastings legs with the chain on the device (nsgan/GAN.py:348-376 hastings, :398-426 collaborate).
def hastings_fill_fused(proposer, sampler, eval_size, real_sigmoid_mean, base=None, refine=True, min_efficiency=None, max_rounds=100000,
                        stats=None, moments=None, calibration=None):
    """``collaborate`` (count_only_productive=False: the nsgan form) over a ``FusedProposer`` and a ``sampling.DeviceIndependenceSampler``:
    G logical batches per round (``launch(..., refine=refine, to_host=False)``: ``refine=True`` is the collaborate leg, GAN.py:398-426,
    ``refine=False`` the hastings leg on standard samples, :348-376), the chain's walk and the gather of the emitted rows queued on the
    slot's stream behind the round, the pool on the device from start to end.  The chain state is shared by the slots' streams, so the
    walks are ordered by events in round order; a round queued ahead of the one that fills the pool finds the pool full and leaves the
    chain untouched, as the reference's loop, which never reaches it, would.  Per round the host receives the G counts and nothing else.
    z and the uniforms are drawn on the host in the reference's order, exactly as ``collaborate_fused`` draws them.
    ``real_sigmoid_mean``: a Python float, an ``np.float32`` or a 1-element fp32 device tensor (``sampler.set_score_curr``).
    ``base``: (samples, sigmoids) for the first pass, device tensors or host arrays, walked as ONE batch (GAN.py:351,402); with
    ``moments`` it must be (samples, sigmoids, features).
    ``moments`` (a metrics.PoolMoments; needs ``FusedProposer(features=True)``) / ``calibration`` (a metrics.CalibrationStats): D's
    features / scores of exactly the rows of the returned pool are gathered beside it and added once, from the device, at the end (the
    scores with label 0).
    Returns (pool: device fp32 tensor [eval_size, ...], efficiency) -- the rows, their order, the efficiency, the sampler's final
    ``d_curr`` and ``cnt_chain`` and the global numpy stream afterwards are those of ``collaborate`` with a host ``IndependenceSampler``
    fed the same scores one batch at a time."""
    import time
    F = _FusedFill("hastings_fill_fused", proposer, eval_size, base, min_efficiency, max_rounds, moments, _UNIFORM, blank=np.zeros(proposer.b),
                   pools=True, calibration=calibration)
    torch, G, dev, C = F.torch, proposer.G, proposer.dev, F.counter
    fill = torch.zeros(1, dtype=torch.int64, device=dev)               # rows the pool has received, unclipped; the walks advance it

    def walk_and_gather(imgs, sigs, feats, uniforms, groups, take_all):
        rows, counts, span = sampler.walk_device(sigs, uniforms, groups, take_all, fill, eval_size)
        for src, pool in F.into_pools(imgs, sigs, feats):
            sampler.gather(src, pool, span, rows)
        return counts

    sampler.set_score_curr(real_sigmoid_mean)                                          # nsgan/GAN.py:350,401
    if base is not None:
        imgs, sigs, feats = F.base_sources(base)
        if tuple(imgs.shape[1:]) != tuple(F.pool.shape[1:]):
            raise ValueError(f"hastings_fill_fused: base samples {tuple(imgs.shape)} are not rows of the proposer's {tuple(F.pool.shape[1:])}")
        C.start(int(walk_and_gather(imgs, sigs, feats, None, 1, None).cpu()[0]))       # :351,402
    F.chain_behind(torch.cuda.current_stream(dev))                                     # (the rounds run on the slots' streams)

    def launch_round(z, us, flags, states):            # the walk is queued with the round: ``pending`` holds its device counts
        st =proposer.streams[proposer.launched % proposer.depth]
        with torch.cuda.stream(st):                    # (uploaded while the slot's stream is idle: a copy from pageable memory waits for the stream)
            u_dev = torch.from_numpy(np.concatenate(us)).to(dev)
            flags_dev = torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(dev) if any(flags) else None
        slot = proposer.launch(z, refine=refine, to_host=False)
        with torch.cuda.stream(st):                    # (behind the slot's ``done``: the same stream)
            st.wait_event(F.chain)                     # the walk before this one, whichever stream it ran on: the chain state is shared
            counts = walk_and_gather(*F.slot_sources(slot), u_dev, G, flags_dev)
            F.chain_behind(st)
        return slot, counts, states

    while not C.full:
        slot, counts, states = F.next_round(launch_round)
        t0 = time.perf_counter()
        with torch.cuda.stream(proposer.streams[slot]):
            emitted = counts.cpu().numpy()                                             # the round's only read-back
        t1 = time.perf_counter()
        F.t_wait += t1 - t0
        F.count_round(emitted, states)                 # (never -1 here: the pool was not full when this batch was reached)
        F.t_chain += time.perf_counter() - t1
    return F.pool, F.finish(stats, host_chain_s=F.t_chain, device_wait_s=F.t_wait)


# ------------------------------------------------------------------------------------------------------------------------------
# The reference's log rows. ``diag``: a dict with z_dawid / brier / ece / mce (metrics.calibration_diagnostics).
def row_nsgan(ckpt, it, cs, fd, eff, diag):
    """One line of GAN.write (nsgan/GAN.py:493-497): ckpt iter CS FD eff z_dawid brier ece mce."""
    return "%d    %d    %.4f    %.4f    %.4f    %.4f    %.4f    %.4f    %.4f\r\n" % (
        ckpt, it, cs, fd, eff, diag["z_dawid"], diag["brier"], diag["ece"], diag["mce"])


def row_synthetic(ckpt, it, quality, eff, diag):
    """One line of save_metrics (synthetic/main.py:106-110): ckpt iter mean_dist good kl js eff z_dawid brier ece mce.  ``quality``: a
    dict with mean_dist / good / kl / js (metrics.mode_metrics, synthetic.evaluate_collaborative)."""
    return "%d    %d    %.4f    %.4f    %.4f    %.4f    %.4f    %.4f    %.4f    %.4f    %.4f\r\n" % (
        ckpt, it, quality["mean_dist"], quality["good"], quality["kl"], quality["js"], eff, diag["z_dawid"], diag["brier"], diag["ece"], diag["mce"])
