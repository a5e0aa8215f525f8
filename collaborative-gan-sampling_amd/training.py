"""Training the image GAN on the device: the generator's update and the train loop (nsgan/GAN.py:132-146, 211-223).

``shaping.DShaper`` is the D update of that loop; ``GStepper`` is its counterpart for G: ONE Adam step on
``g_loss = mean BCE(D(G(z)), 1)`` with G **and** D in training mode (batch statistics; ``generator(z, is_training=True)`` at :120, D bound at
:121), the optimizer at ``learning_rate*5`` (:145) over the ``g_`` variables only.  Forward, backward-data, the weight / bias / gamma / beta
gradients (wgrad.hip: ``cgs_deconv2d_nhwc_bwd_weight`` for the transposed convolutions) and the Adam update run on the same stage tapes and in
place on the same parameter tensors the ``RefineEngine`` and the ``DShaper`` read.  ``GanTrainer`` strings the two steps into the
reference's iteration, so the package can produce the checkpoint it then shapes and refines.
"""
import gc
import math

import torch

from . import checkpoint
from . import kernels as K
from . import lib as L
from .engine import Tape, _BnTrainLrelu, _Conv, _Deconv, _Linear, _View, link_backward_fusion
from .nets import ARCHS, g_input_shape
from .shaping import DShaper

BN_DECAY = 0.9      # nsgan/ops.py:21


class GStepper:
    def __init__(self, arch, params, batch_size, device="cuda:0", learning_rate=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, loss="bce"):
        """``loss``: G's training loss, the mean over every logit of "bce" (softplus(-l), nsgan/GAN.py:130-131), "lsq" ((l - 1)^2) or
        "linear" (-l, the generator's side of a hinge discriminator)."""
        if loss not in ("bce", "lsq", "linear"):
            raise L.CgsError(f"GStepper: loss {loss!r}: expected 'bce', 'lsq' or 'linear'")
        self.loss = loss
        self.A = ARCHS[arch] if isinstance(arch, str) else arch
        self.dev = torch.device(device)
        self.B = int(batch_size)
        self.lr, self.b1, self.b2, self.eps, self.t = learning_rate * 5, beta1, beta2, eps, 0       # nsgan/GAN.py:145
        A = self.A
        with torch.cuda.device(self.dev):
            self.g = Tape(A["g_head"] + A["g_tail"], g_input_shape(A), params, "generator", self.B, A["k"], A["stride"], True, self.dev)
            self.d = Tape(A["d"], A["img"], params, "discriminator", self.B, A["k"], A["stride"], True, self.dev)     # data gradients only
            link_backward_fusion(self.g.stages + self.d.stages)              # across the G / D seam too (the tanh under D's first conv)
            f32 = dict(dtype=torch.float32, device=self.dev)
            self.dlogits = torch.empty((self.B,) + tuple(self.d.out_shape), **f32)
            self.loss_buf = torch.zeros(1, **f32)
            self.x_in = [None] * len(self.g.stages)
            name_of = {id(v): k for k, v in params.items()}
            # trainable tensors (the g_vars of nsgan/GAN.py:139) with gradient and Adam slots; the moving statistics of G's norms
            self.slots, self.names, self.moving = [], [], []        # (param, grad, m, v) | TF names | (stage, moving_mean, moving_variance)
            for st in self.g.stages:
                if isinstance(st, (_Linear, _Deconv)):
                    attrs = ("w", "b")
                elif isinstance(st, _BnTrainLrelu):
                    attrs = ("gamma", "beta")
                    scope = name_of[id(st.gamma)].rsplit("/", 1)[0]
                    self.moving.append((st, params[scope + "/moving_mean"], params[scope + "/moving_variance"]))
                elif isinstance(st, _View):
                    attrs = ()
                else:
                    raise NotImplementedError(f"GStepper: no parameter gradients for a {type(st).__name__} stage")
                for n in attrs:
                    p = getattr(st, n)
                    g = torch.zeros_like(p)
                    setattr(st, "g_" + n, g)
                    self.slots.append((p, g, torch.zeros_like(p), torch.zeros_like(p)))
                    self.names.append(name_of[id(p)])
        self.table = None       # a kernels.AdamTable over ``slots`` while a GanTrainer records the step into a hipGraph

    # -- G in training mode ------------------------------------------------------------------------------
    def forward(self, z):
        """``generator(z, is_training=True)`` (nsgan/GAN.py:120): batch statistics, and the moving averages of every norm move once, as in
        ``ops.bn``.  Returns the tape's own output buffer (valid until the next forward)."""
        with torch.cuda.device(self.dev):
            x = z.contiguous()
            for i, st in enumerate(self.g.stages):
                self.x_in[i] = x
                x = st.fwd(x)
            if self.table is not None:                         # being recorded: one launch per norm
                for st, mm, mv in self.moving:
                    K.bn_moving_update(st.mean, st.invstd, mm, mv, BN_DECAY, K.BN_EPS)
                return x
            with torch.no_grad():
                for st, mm, mv in self.moving:
                    var = st.invstd.pow(-2).sub_(K.BN_EPS)     # the (biased) batch variance behind invstd = 1 / sqrt(var + eps)
                    torch._foreach_mul_([mm, mv], BN_DECAY)
                    torch._foreach_add_([mm, mv], [st.mean, var], alpha=1.0 - BN_DECAY)
            return x

    # -- the way back through G, with parameter gradients --------------------------------------------------
    def _backward(self, dy):
        stages = self.g.stages
        for idx in range(len(stages) - 1, -1, -1):
            st = stages[idx]
            first = idx == 0
            if isinstance(st, _View):
                dy = st.bwd(dy)
            elif isinstance(st, _BnTrainLrelu):
                dy = st.bwd(dy)                                            # dx in place; statistics stay in the bn workspace
                K.bn_train_param_grads(st.x, st.g_gamma, st.g_beta)
            elif isinstance(st, _Linear):
                if st.epi == L.EPI_LRELU and not st.pre_folded:
                    dy = K.lrelu_bwd(dy, st.out, out=dy)
                K.linear_bwd_weight(st.x_in, dy, out=st.g_w)
                K.bias_grad(dy, out=st.g_b)
                if not first:
                    dy = K.linear_bwd_data(dy, st.w, out=st.dx)
            elif isinstance(st, _Deconv):
                if st.epi == L.EPI_TANH and not st.pre_folded:
                    dy = K.tanh_bwd(dy, st.out, out=dy)
                kh, kw = st.w.shape[0], st.w.shape[1]
                K.deconv2d_bwd_weight(self.x_in[idx], dy, kh, kw, st.s, st.s, out=st.g_w)
                K.bias_grad(dy, out=st.g_b)
                if not first:
                    e, a, aux = st.bwd_epi
                    dy = K.deconv2d_bwd_data(dy, st.w, st.in_hw, st.s, st.s, out=st.dx, epilogue=e, ep_a=a, ep_aux=aux)
            else:
                raise NotImplementedError(type(st).__name__)

    def loss_and_grads(self, z):
        """g_loss (device scalar tensor) and the gradients of every G variable (left in the ``g_*`` buffers).  D's variables are read only."""
        with torch.cuda.device(self.dev):
            logits = self.d.forward(self.forward(z))
            if self.loss == "bce":
                K.bce_logits_grad(logits, 1.0, 1.0 / logits.numel(), self.dlogits, self.loss_buf)
            else:
                K.gan_logits_grad(logits, self.loss, 1.0, 1.0 / logits.numel(), self.dlogits, self.loss_buf)
            self._backward(self.d.backward(self.dlogits))
            return self.loss_buf[0].clone()

    def step(self, z):
        """One Adam step of G (nsgan/GAN.py:223).  Returns g_loss before the update."""
        loss = self.loss_and_grads(z)
        if self.table is not None:          # being recorded: one launch at the lr_t its owner writes into device memory; ``t`` is the owner's
            with torch.cuda.device(self.dev):
                self.table.step(None, self.b1, self.b2, self.eps)
            K.WS.invalidate()
            return loss
        self.t += 1
        lr_t = self.lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)      # tf.train.AdamOptimizer
        with torch.cuda.device(self.dev):
            for p, g, m, v in self.slots:
                K.adam_step(p, g, m, v, lr_t, self.b1, self.b2, self.eps)
        K.WS.invalidate()                   # packed copies of the old weights are stale (re-packed on next use)
        return loss

    def grads(self):
        return dict(zip(self.names, (g for _, g, _, _ in self.slots)))


class GanTrainer:
    """The reference's train loop body (nsgan/GAN.py:219-223) on one parameter store: a D step on (real, G(z)), then a G step on the same z.

    ``use_graph=True``: the whole iteration is captured once as a hipGraph and replayed.  The first call runs eagerly on the trainer's own
    side stream (a train step has side effects, so the warm-up is a real iteration; it also brings the stream-keyed workspaces to their final
    size), the second captures and replays, later ones replay.  ``path`` names what the last call ran, ``graph_fallback`` why a capture was
    refused (the trainer then goes on with eager launches)."""

    def __init__(self, arch, params, batch_size, device="cuda:0", learning_rate=2e-4, beta1=0.5, engine=None, use_graph=False, loss="bce"):
        """``loss``: "bce" (the reference's), "lsq" (least squares on both sides) or "hinge" (D's hinge with the linear loss -l for G)."""
        if loss not in ("bce", "lsq", "hinge"):
            raise L.CgsError(f"GanTrainer: loss {loss!r}: expected 'bce', 'lsq' or 'hinge'")
        self.arch, self.P, self.loss = arch, params, loss
        self.dshaper = DShaper(arch, params, batch_size, device, learning_rate=learning_rate, beta1=beta1, loss=loss)
        self.gstepper = GStepper(arch, params, batch_size, device, learning_rate=learning_rate, beta1=beta1,
                                 loss="linear" if loss == "hinge" else loss)
        self.engine = engine                # an optional RefineEngine on the same parameter tensors: kept coherent after every iteration
        self.use_graph = bool(use_graph)
        self.path, self.graph_fallback = "eager", None
        self._graph = self._gstream = self._out = self._tables = None
        self._warm = False
        if self.use_graph:
            gs = self.gstepper
            f32 = dict(dtype=torch.float32, device=gs.dev)
            self._real = torch.empty((gs.B,) + tuple(gs.A["img"]), **f32)
            self._z = torch.empty((gs.B,) + tuple(g_input_shape(gs.A)), **f32)

    def _program(self, real, z):
        fake = self.gstepper.forward(z)
        d_loss = self.dshaper.step(real, fake)
        g_loss = self.gstepper.step(z)
        return d_loss, g_loss

    def iteration(self, real, z):
        """-> (d_loss, g_loss), both before their update.  G runs in training mode in both steps: its moving averages move twice."""
        if self.use_graph and self.graph_fallback is None and K.PROFILE is None:
            out = self._graph_iteration(real, z)
        else:
            self.path = "eager"
            out = self._program(real, z)
        if self.engine is not None:
            self.engine.refresh_weights()
        return out

    # -- the captured form ---------------------------------------------------------------------------------
    def _capture(self):
        """Record ``_program`` on the static inputs.  Weights change at every replay, so the program must CONTAIN the pack kernels: every
        packed copy is marked stale first, and the first use of each weight (and again after D's Adam) re-packs into the buffer the warm-up made."""
        steppers = (self.dshaper, self.gstepper)
        if self._tables is None:
            self._tables = [K.AdamTable(st.slots) for st in steppers]
        torch.cuda.synchronize(self.gstepper.dev)
        gc_was_on = gc.isenabled()
        gc.disable()                        # (a finalizer that reaches HIP inside a capture aborts the process: engine.py, refine)
        for st, tb in zip(steppers, self._tables):
            st.table = tb
        try:
            K.WS.invalidate()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self._gstream, capture_error_mode="thread_local"):
                out = self._program(self._real, self._z)
        except L.CgsError:
            raise
        except Exception as ex:             # noqa: BLE001 (HIP / the allocator / another thread's HIP call refused the capture)
            raise L.GraphCaptureError(f"{type(ex).__name__}: {str(ex)[:300]}") from ex
        finally:
            for st in steppers:
                st.table = None
            K.WS.invalidate()               # the host cache's versions describe a program that was recorded, not run
            if gc_was_on:
                gc.enable()
        self._graph, self._out = g, out

    def _graph_iteration(self, real, z):
        gs = self.gstepper
        for t, buf, what in ((real, self._real, "real"), (z, self._z, "z")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(buf.shape):
                raise L.CgsError(f"GanTrainer.iteration: {what} is {tuple(getattr(t, 'shape', ()))}, the trainer was built for {tuple(buf.shape)}")
        with torch.cuda.device(gs.dev):
            if self._gstream is None:
                self._gstream = torch.cuda.Stream(gs.dev)
            cur = torch.cuda.current_stream(gs.dev)
            self._gstream.wait_stream(cur)
            with torch.cuda.stream(self._gstream):
                self._real.copy_(real)
                self._z.copy_(z)
                if self._warm and self._graph is None:
                    try:
                        self._capture()
                    except L.GraphCaptureError as ex:
                        self.graph_fallback = str(ex)
                if not self._warm or self._graph is None:
                    self.path, self._warm = "eager", True
                    out = self._program(self._real, self._z)
                else:
                    for st, tb in zip((self.dshaper, gs), self._tables):
                        st.t += 1
                        tb.lr_t.fill_(st.lr * math.sqrt(1.0 - st.b2 ** st.t) / (1.0 - st.b1 ** st.t))      # tf.train.AdamOptimizer
                    self._graph.replay()
                    K.WS.invalidate()       # the replay re-packed and then updated the weights behind the host cache's back
                    self.path, out = "graph", self._out
            cur.wait_stream(self._gstream)
            return out[0].clone(), out[1].clone()        # fresh tensors on the caller's stream: later iterations leave them alone

    def save(self, path):
        """The TF key space of ``checkpoint.py`` (variables only: Adam's slots are not part of it, as ``clean_tf_names`` drops them)."""
        checkpoint.save(path, self.P)

    def load(self, path):
        """Restore INTO the live tensors, so the steppers and an attached engine keep pointing at them.  A checkpoint carries no optimizer
        state: both steppers start again from zero moments and ``t = 0``, as a fresh trainer on the loaded variables would."""
        new = checkpoint.load(path)
        checkpoint.check_against_arch(new, self.arch)
        with torch.no_grad():
            for k, v in self.P.items():
                v.copy_(torch.from_numpy(new[k]))
            for stepper in (self.dshaper, self.gstepper):
                stepper.t = 0
                for _, _, m, v in stepper.slots:
                    m.zero_(); v.zero_()
        K.WS.invalidate()
        if self.engine is not None:
            self.engine.refresh_weights()
