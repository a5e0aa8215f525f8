"""float64 definitions of the refinement losses, the GAN training losses and the ladam step, shared by the loss tests (CPU: checked
against float64 torch autograd and oracle.sampling_ref.Policy; GPU: what the kernels are compared with).  No test in this file."""
import numpy as np

U = 2.0 ** -24           # unit roundoff of fp32
B1, B2, B3, EPS = 0.9, 0.5, 0.5, 1e-8
C1, C2 = np.float64(np.float32(1.0 - B1)), np.float64(np.float32(1.0 - B2))      # the rule's (1 - beta) factors as the fp32 the kernel is handed
REFINE_KINDS = ("bce", "lsq", "linear")
D_KINDS = ("bce", "lsq", "hinge")
KINK_MARGIN = 1e-4


def make_logits(shape, seed):
    """Seeded N(0, 6) logits with +40 and -40 planted, every one at least KINK_MARGIN away from the hinge kinks at +-1 (fp32)."""
    rs = np.random.RandomState(seed)
    l = rs.normal(0.0, 6.0, int(np.prod(shape)))
    if l.size >= 2:
        l[0], l[-1] = 40.0, -40.0
    for k in (-1.0, 1.0):
        near = np.abs(l - k) < 10 * KINK_MARGIN
        l[near] = k + 10 * KINK_MARGIN
    l = l.astype(np.float32).reshape(shape)
    assert min(np.abs(l.astype(np.float64) - 1.0).min(), np.abs(l.astype(np.float64) + 1.0).min()) >= KINK_MARGIN
    return l


# ---- the refiner's loss per logit, unreduced, and d(sum loss)/d logit (collaborator.py:30-31) ----------------------------------
def refine_loss(kind, l):
    l = np.asarray(l, dtype=np.float64)
    return {"bce": lambda: np.logaddexp(0.0, -l), "lsq": lambda: (l - 1.0) ** 2, "linear": lambda: -l}[kind]()


def refine_dlogits(kind, l):
    l = np.asarray(l, dtype=np.float64)
    return {"bce": lambda: -1.0 / (1.0 + np.exp(l)), "lsq": lambda: 2.0 * (l - 1.0), "linear": lambda: -np.ones_like(l)}[kind]()


def sigmoid(l):
    l = np.asarray(l, dtype=np.float64)
    return np.where(l >= 0, 1.0 / (1.0 + np.exp(-np.abs(l))), np.exp(-np.abs(l)) / (1.0 + np.exp(-np.abs(l))))


# ---- D's (and G's) training losses per logit; target 1 = real, 0 = fake ---------------------------------------------------------
def d_loss(kind, l, target):
    l = np.asarray(l, dtype=np.float64)
    if kind == "bce":
        return np.maximum(l, 0.0) - l * target + np.log1p(np.exp(-np.abs(l)))
    if kind == "lsq":
        return (l - target) ** 2
    if kind == "hinge":
        return np.maximum(1.0 - l, 0.0) if target == 1.0 else np.maximum(1.0 + l, 0.0)
    if kind == "linear":
        return -l
    raise ValueError(kind)


def d_dlogits(kind, l, target):
    l = np.asarray(l, dtype=np.float64)
    if kind == "bce":
        return sigmoid(l) - target
    if kind == "lsq":
        return 2.0 * (l - target)
    if kind == "hinge":
        return np.where(l < 1.0, -1.0, 0.0) if target == 1.0 else np.where(l > -1.0, 1.0, 0.0)
    if kind == "linear":
        return -np.ones_like(l)
    raise ValueError(kind)


# ---- the ladam rule on an activation map (policy.py:39-59) ----------------------------------------------------------------------
def ladam_state(loss, loss_avg, first):
    """(running loss, per-sample gain) after one step (policy.py:48-51,56)."""
    loss = np.asarray(loss, dtype=np.float64)
    avg = loss if first else B3 * np.asarray(loss_avg, dtype=np.float64) + (1.0 - B3) * loss
    return avg, np.clip(avg + 0.5, 0.0, 1e4) ** 2


def ladam_step(theta, m, v, g, gain, rate, first, vmin=None, vmax=None, c1=C1, c2=C2):
    """(theta, m, v) after one step, float64; ``gain`` per sample [B].  c1 / c2: the (1 - beta) factors (default: as the kernel gets them)."""
    theta, g = np.asarray(theta, dtype=np.float64), np.asarray(g, dtype=np.float64)
    B = theta.shape[0]
    if first:
        m, v = g.copy(), g * g
    else:
        m = B1 * np.asarray(m, dtype=np.float64) + c1 * g
        v = B2 * np.asarray(v, dtype=np.float64) + c2 * (g * g)
    step = (rate * m / (np.sqrt(v) + EPS)) * np.asarray(gain, dtype=np.float64).reshape((B,) + (1,) * (theta.ndim - 1))
    out = theta - step
    if vmin and vmax:
        out = np.clip(out, vmin, vmax)
    return out, m, v


def ladam_bound(theta, m, v, g, gain, rate, first):
    """|fp32 theta' - float64 theta'| of one step from the SAME fp32 inputs, per element, from the operation count of the formula
    (DESIGN.md section 21).  Roundings, each at most U relative: m = 0.9f*m + c1*g is two products and a sum, and 0.9f is itself rounded,
    so |dm| <= 3U (0.9|m| + c1|g|) (0 on the first step: m = g); v = 0.5 v + 0.5 g^2 rounds g^2 and the sum, sqrt once more on half of
    that, + 1e-8f twice (constant, sum): the denominator is off by at most 4U; rate (its fp32 value), rate*m, the quotient, * gain: 4U;
    the final subtraction U |theta'|.  Sum of the first-order terms, times 2 for the second-order ones."""
    theta, g = np.asarray(theta, dtype=np.float64), np.asarray(g, dtype=np.float64)
    new, m2, v2 = ladam_step(theta, m, v, g, gain, rate, first)
    B = theta.shape[0]
    scale = rate * np.asarray(gain, dtype=np.float64).reshape((B,) + (1,) * (theta.ndim - 1)) / (np.sqrt(v2) + EPS)
    dm = 0.0 if first else 3.0 * U * (B1 * np.abs(np.asarray(m, dtype=np.float64)) + C1 * np.abs(g))
    return 2.0 * (U * np.abs(new) + 8.0 * U * np.abs(new - theta) + scale * dm)
