"""The 64-unit 2-D discriminator kernels of csrc/mlp2d.hip (mlp_saliency_kernel, refine2d_kernel, mlp_train_fwdbwd_kernel /
mlp_train_grad_kernel), stated once in float64 numpy, and the case tables their tests share (tests/test_mlp2d_cases_cpu.py checks the
definitions and derives the bars without a device; tests/test_gpu_mlp2d_narrow.py holds the kernels to them).  No test in this file.

    ref64          forward, ReLU masks and backward of the float32 weights; which rows sit on a ReLU kink
    teacher_forced the refiner's recurrence with every gradient taken at the DEVICE's own recorded point: an error does not pass
                   through D again, so the comparison is one step deep, K times, and a chaotic K-step loop can be held to ~1e-5
    d_step64       d_loss_real, d_loss_fake (means) and every dW, db of their sum, by the explicit backward

Bars.  The reference side of every measured bar is the float32 torch-CPU oracle (oracle.sampling_ref) against these float64
definitions over the very tables below; the bar is 4x that (the margin tests/test_gpu_synthetic_wide.py gives a float32 implementation
that adds in another order).  tests/test_mlp2d_cases_cpu.py prints the oracle's numbers and asserts them inside the bars; the device's
stand in the docstring of tests/test_gpu_mlp2d_narrow.py.

    quantity                                          oracle's worst   bar
    |d sigmoid|                                       1.9e-6           2e-5   (SIGMOID_BAR: the project's device-score bar)
    max|d saliency| / max|saliency|, kept rows        ORACLE_SALIENCY  4x
    one refiner step, |d x| absolute, kept rows       ORACLE_STEP      4x
    D step: |d loss| / |loss|                         ORACLE_DLOSS     min(4x, 2e-5)  (2e-5, 2e-4: the bars of
    D step: max|d grad| / max|grad|, per tensor       ORACLE_DGRAD     min(4x, 2e-4)   test_mlp_d_step_gradients_and_sgd_vs_autograd)
"""
import functools

import numpy as np

from oracle import sampling_ref as S

F32 = np.float32
NEAR = 1e-6             # a pre-activation within NEAR * max|z| (max over its layer and batch) of zero: a rounding may take the other branch
KINK_CAP = 0.05         # at most this share of a case's rows may be dropped for that

SIGMOID_BAR = 2e-5
ORACLE_SALIENCY = 2.39e-6     # worst at (64, 6, 4097) scale 2 (so is |d sigmoid|)
ORACLE_STEP = 5.6e-6          # worst at (33, 4, 1000, 10, ladam, 0.1) scale 2
ORACLE_DLOSS = 2.2e-6         # worst at (5, 33, 1, 64): one real row
ORACLE_DGRAD = 3.1e-6         # the same case
SALIENCY_BAR = 4 * ORACLE_SALIENCY
STEP_BAR = 4 * ORACLE_STEP
DLOSS_BAR = min(4 * ORACLE_DLOSS, 2e-5)
DGRAD_BAR = min(4 * ORACLE_DGRAD, 2e-4)
DEVICE_SIGMOID = 1.8e-6       # the device's measured worst |d sigmoid| over SALIENCY (1.751e-6 at (64, 6, 4097) scale 2): the refiner's pick of
                              # the best step is a minimum of the true losses up to twice this

# (nh, nl, B), each at weight scales 1.0 and 2.0.  256 blocks x 16 waves take 4096 samples a turn.
SALIENCY = [(64, 6, 1), (64, 6, 4097), (64, 2, 17), (63, 3, 333), (33, 4, 1000), (7, 5, 15), (1, 2, 64), (16, 6, 8200)]
SCALES = [1.0, 2.0]

# (nh, nl, B, K, method, rate, scale)
REFINE = [(64, 6, 1000, 10, "ladam", 0.1, 1.0), (64, 6, 4097, 5, "ladam", 0.05, 2.0), (64, 2, 17, 5, "sgd", 20.0, 2.0),
          (63, 3, 333, 5, "momentum", 60.0, 2.0), (33, 4, 1000, 10, "ladam", 0.1, 2.0), (7, 5, 15, 5, "ladam", 0.05, 2.0),
          (16, 6, 8200, 3, "ladam", 0.05, 2.0), (64, 6, 333, 5, "sgd", 200.0, 1.0), (64, 6, 333, 5, "momentum", 60.0, 1.0)]

# (nl, nh, B_real, B_fake)
DSTEP = [(6, 64, 4100, 4097), (2, 1, 5, 3), (3, 63, 77, 130), (4, 7, 64, 1), (5, 33, 1, 64), (6, 64, 1000, 1000)]


def case_id(c):
    return "-".join(str(v) for v in c)


def net(nh, nl, seed, scale):
    """S.mlp_init as float32 numpy arrays ([din, dout] kernels, [dout] biases)."""
    Ws, bs = S.mlp_init(nh, nl, seed=seed, scale=scale)
    return [w.numpy() for w in Ws], [b.numpy() for b in bs]


def _forward64(Ws, bs, x):
    W = [w.astype(np.float64) for w in Ws]
    b = [v.astype(np.float64) for v in bs]
    h = np.asarray(x, np.float64)
    hs, zs, near = [h], [], np.zeros(len(h), bool)
    for i in range(len(W) - 1):
        z = h @ W[i] + b[i]
        near |= (np.abs(z) < NEAR * np.abs(z).max()).any(axis=1)
        zs.append(z)
        h = np.maximum(z, 0.0)
        hs.append(h)
    return W, hs, zs, (h @ W[-1] + b[-1])[:, 0], near


def ref64(Ws, bs, x, inv_batch=None):
    """float64 forward, ReLU masks and backward of the float32 weights -> (sigmoid [B], saliency [B,2] = inv_batch (sigmoid - 1) d logit / dx
    (inv_batch: 1 / B unless given), near [B]); near[b]: some pre-activation of row b lies within 1e-6 max|z| (max over its layer) of
    zero -- a rounding may take the other ReLU branch there, which changes one gradient path discretely whatever computes it
    (DESIGN.md section 4)."""
    W, hs, zs, logit, near = _forward64(Ws, bs, x)
    g = np.broadcast_to(W[-1][:, 0], hs[-1].shape).copy()
    for i in range(len(W) - 2, -1, -1):
        g = (g * (zs[i] > 0)) @ W[i].T
    sig = 1.0 / (1.0 + np.exp(-logit))
    sal = (sig - 1.0)[:, None] * g
    return sig, (sal / len(sal) if inv_batch is None else sal * inv_batch), near


def teacher_forced(Ws, bs, traj, base, rate, method):
    """refine2d_kernel's recurrence (sampling/refiner_cpu.py:19-81, policy.py:26-61) in float64 with the gradients evaluated at the recorded
    points traj[:, i] ([B, K+1, 2] float32): -> (pred [B, K+1, 2] with pred[:, i+1] = traj[:, i] - update_i and pred[:, 0] = traj[:, 0],
    loss64 [B, K+1] = base - sigmoid at all K+1 recorded points, near [B] OR-ed over them).  The optimizer state (momentum: m; ladam: m, v
    and the running loss) is accumulated from those same points.  base, rate and 1 / B enter as the float32 values the kernel is handed,
    0.9f, 0.1f and 1e-8f as their float32 values."""
    traj = np.asarray(traj)
    B, K = traj.shape[0], traj.shape[1] - 1
    base, rate, inv = float(F32(base)), float(F32(rate)), float(F32(1.0 / B))
    c09, c01, eps = float(F32(0.9)), float(F32(0.1)), float(F32(1e-8))
    pred = np.empty((B, K + 1, 2))
    pred[:, 0] = traj[:, 0]
    loss64, near = np.empty((B, K + 1)), np.zeros(B, bool)
    m = v = ll = None
    for i in range(K + 1):
        sig, g, nr = ref64(Ws, bs, traj[:, i], inv)
        loss64[:, i] = base - sig
        near |= nr
        if i == K:
            break
        loss = loss64[:, i]
        if method == "sgd":
            upd = rate * g
        elif method == "momentum":
            m = rate * g if i == 0 else c09 * m + rate * g
            upd = m
        elif method == "ladam":
            if i == 0:
                m, v, ll = g, g * g, loss
            else:
                m, v, ll = c09 * m + c01 * g, 0.5 * v + 0.5 * (g * g), 0.5 * ll + 0.5 * loss
            upd = rate * m / (np.sqrt(v) + eps) * (np.maximum(ll + 0.5, 0.0) ** 2)[:, None]
        else:
            raise NotImplementedError(method)
        pred[:, i + 1] = traj[:, i].astype(np.float64) - upd
    return pred, loss64, near


def d_step64(Ws, bs, real, fake):
    """-> (d_loss_real, d_loss_fake, [dW...], [db...], near_real [B_real], near_fake [B_fake]): mean BCE(D(real), 1), mean BCE(D(fake), 0)
    (synthetic/GAN.py:60-74) and the gradient of their sum in every D variable, float64, by the explicit backward."""
    n = len(Ws)
    dW, db = [np.zeros(w.shape) for w in Ws], [np.zeros(b.shape) for b in bs]
    losses, nears = [], []
    for x, t in ((real, 1.0), (fake, 0.0)):
        W, hs, zs, logit, near = _forward64(Ws, bs, x)
        losses.append(float(np.mean(np.maximum(logit, 0.0) - logit * t + np.log1p(np.exp(-np.abs(logit))))))
        nears.append(near)
        d = ((1.0 / (1.0 + np.exp(-logit)) - t) / len(logit))[:, None]          # d loss / d logit
        for i in range(n - 1, -1, -1):
            dW[i] += hs[i].T @ d
            db[i] += d.sum(axis=0)
            if i:
                d = (d @ W[i].T) * (zs[i - 1] > 0)
    return losses[0], losses[1], dW, db, nears[0], nears[1]


# ---- the cases' inputs (seeded; computed once per process and shared, never written to) -----------------------------------------
@functools.lru_cache(maxsize=None)
def saliency_case(nh, nl, B, scale):
    """-> (Ws, bs, x [B,2] float32, (sigmoid, saliency, near) of ref64)."""
    Ws, bs = net(nh, nl, 7 + nh + nl, scale)
    x = (3.0 * np.random.RandomState(1000 + B + nh).randn(B, 2)).astype(F32)
    return Ws, bs, x, ref64(Ws, bs, x)


@functools.lru_cache(maxsize=None)
def refine_case(nh, nl, B, K, method, rate, scale):
    """-> (Ws, bs, x [B,2] float32, base): base = the float32 oracle's mean sigmoid of a real batch of 512 (refiner_cpu.py:23,28)."""
    import torch
    Ws, bs = net(nh, nl, 2019 + nh + nl, scale)
    rs = np.random.RandomState(B + nh + K)
    x = (3.0 * rs.randn(B, 2)).astype(F32)
    real = S.toy_next_batch("Imbal-8Gaussians", 10.0, 0.9, 512, rs).astype(F32)
    sig, _ = S.mlp_sigmoid_and_saliency([torch.from_numpy(w) for w in Ws], [torch.from_numpy(b) for b in bs], real)
    return Ws, bs, x, float(F32(np.mean(sig)))


@functools.lru_cache(maxsize=None)
def dstep_case(nl, nh, Br, Bf):
    """-> (Ws, bs, real [Br,2], fake [Bf,2], dropped): the first Br / Bf rows that are not near a kink, of seeded candidate batches a little
    larger than asked for, so that the batch sizes (and with them the number of turns of the sample loop) are exactly the table's;
    dropped = the share of candidates looked at that sat near a kink."""
    Ws, bs = net(nh, nl, 3 + nh + nl, 2.0)
    rs = np.random.RandomState(5 + Br + Bf)
    out, looked, drop = [], 0, 0
    for B, real in ((Br, True), (Bf, False)):
        N = max(64, B + B // 10 + 8)
        cand = (S.toy_next_batch("Imbal-8Gaussians", 10.0, 0.9, N, rs)[rs.permutation(N)] if real else 3.0 * rs.randn(N, 2)).astype(F32)
        near = ref64(Ws, bs, cand)[2]
        idx = np.flatnonzero(~near)[:B]
        assert len(idx) == B
        out.append(np.ascontiguousarray(cand[idx]))
        looked += idx[-1] + 1
        drop += int(near[:idx[-1] + 1].sum())
    return Ws, bs, out[0], out[1], drop / looked


def refine_f32(Ws, bs, x, base, K, rate, method):
    """refine2d_kernel's loop restated in float32 numpy, operation by operation, on the float32 torch-CPU oracle D
    (S.mlp_sigmoid_and_saliency): the stand-in for the device.  -> (traj [B, K+1, 2], best [B, 2], best_step [B]), all float32."""
    import torch
    Wt, bt = [torch.from_numpy(w) for w in Ws], [torch.from_numpy(b) for b in bs]

    def d_fn(p):
        sig, g = S.mlp_sigmoid_and_saliency(Wt, bt, p)
        return sig[:, 0].astype(F32), g.astype(F32)
    base, rate = F32(base), F32(rate)
    c09, c01, half, eps = F32(0.9), F32(0.1), F32(0.5), F32(1e-8)
    x = np.array(x, dtype=F32)
    B = len(x)
    traj = np.empty((B, K + 1, 2), F32)
    traj[:, 0] = x
    sig, g = d_fn(x)
    loss = base - sig
    best, bl, bstep = x.copy(), loss.copy(), np.zeros(B, F32)
    m = v = ll = None
    for i in range(K):
        if method == "sgd":
            x = x - rate * g
        elif method == "momentum":
            a = rate * g
            m = a if i == 0 else c09 * m + a
            x = x - m
        else:
            if i == 0:
                m, v, ll = g, g * g, loss
            else:
                m, v, ll = c09 * m + c01 * g, half * v + half * (g * g), half * ll + half * loss
            c = np.maximum(ll + half, F32(0.0))
            x = x - rate * m / (np.sqrt(v) + eps) * (c * c)[:, None]
        assert x.dtype == F32
        sig, g = d_fn(x)
        loss = base - sig
        upd = (bl - loss) > 0
        bl[upd], best[upd], bstep[upd] = loss[upd], x[upd], i + 1
        traj[:, i + 1] = x
    return traj, best, bstep
