"""The fused refiner on the least-squares and linear losses and on the ladam rule, and the D / G steps on the least-squares and hinge
losses.  The reference for a loss closure is the generic path on the same device, which differentiates any
closure; for ladam a loop written here from the engine's own evaluation and the float64 step of tests/loss_cases.py.
Seeds: parameters N.init_params(arch, 2019), inputs RandomState(0)."""
import numpy as np
import pytest
import torch

import loss_cases as LC
from oracle import nets_ref as N

pytestmark = pytest.mark.gpu

CASES = [("mnist", 4), ("cyclegan_tiny", 2)]          # the one-logit head | patch logits
KSTEPS, RATE = 3, 0.1


def dev():
    return torch.device("cuda:0")


def relerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def setup(arch, B):
    from cgs_amd import ops
    from cgs_amd.model import GAN
    d = dev()
    ops.reset_variables()
    gan = GAN(arch, batch_size=B, device=d, params=N.init_params(arch, 2019, True))
    rs = np.random.RandomState(0)
    if arch == "mnist":
        inp = rs.uniform(-1, 1, (B, 62)).astype(np.float32)
    else:
        inp = rs.uniform(-1, 1, (B,) + tuple(N.ARCHS[arch]["img"])).astype(np.float32)
    f0 = gan.input_to_feature(torch.from_numpy(inp).to(d)).detach().clone()
    return gan, f0


def closure(kind):
    from cgs_amd import ops
    return {"bce": lambda l: ops.sigmoid_cross_entropy_with_logits(labels=ops.ones_like(l), logits=l),
            "lsq": lambda l: ops.least_squares_loss(l, 1.0), "linear": lambda l: ops.hinge_loss(l)}[kind]


@pytest.mark.parametrize("kind", ("lsq", "linear"))
@pytest.mark.parametrize("arch,B", CASES)
def test_loss_closures_take_the_engine_and_agree_with_the_generic_path(arch, B, kind):
    from functools import partial
    from cgs_amd import ops
    from cgs_amd.sampling.collaborator import Refiner
    gan, f0 = setup(arch, B)
    D = partial(gan.discriminator, is_training=True, reuse=True)
    fn = closure(kind)
    re_, rg = Refiner(KSTEPS, RATE), Refiner(KSTEPS, RATE)
    re_.set_env(D, gan.feature_to_data, fn)
    rg.set_env(D, gan.feature_to_data, fn)
    rg.force_generic = True
    rg.use_graph = False
    # one evaluation
    lm_g, grad_g = rg.compute_forward_logits_and_grad(f0)
    lm_e, grad_e = gan.engine(B).compute_forward_logits_and_grad(f0, loss=kind)
    e1, e2 = relerr(lm_e.cpu(), lm_g.cpu()), relerr(grad_e.cpu(), grad_g.cpu())
    print(f"{arch} {kind}: one evaluation: logit {e1:.2e}, gradient {e2:.2e}")
    assert e1 < 1e-4 and e2 < 1e-4
    # K steps
    with pytest.warns(RuntimeWarning) if "refiner.force_generic is set" not in Refiner._WARNED else _nullcontext():
        img_g = rg.build_refiner(f0, None, "deterministic")
    img_e = re_.build_refiner(f0, None, "deterministic")
    assert re_.path == "engine" and re_.why_generic is None and re_.loss_kind == kind
    assert rg.path == "generic" and gan.build_refiner(KSTEPS, RATE, loss=kind)._engine_owner() is gan
    for name in ("optimal_logit", "optimal_feature", "default_logit"):
        e = relerr(getattr(re_, name).cpu(), getattr(rg, name).cpu())
        print(f"{arch} {kind}: {name} {e:.2e}")
        assert e < 2e-3, name
    assert relerr(img_e.cpu(), img_g.cpu()) < 5e-2
    # the selected step: equal, except where the two paths' best logits tie to 1e-6 relative -- at most one sample of the batch
    se, sg = re_.optimal_step.cpu().numpy(), rg.optimal_step.cpu().numpy()
    le, lg = re_.optimal_logit.cpu().numpy().astype(np.float64), rg.optimal_logit.cpu().numpy().astype(np.float64)
    differ = np.nonzero(se != sg)[0]
    assert len(differ) <= 1 and all(abs(le[i] - lg[i]) < 1e-6 * abs(lg[i]) for i in differ), (se, sg)
    ops.reset_variables()


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def test_probe_verdicts_and_the_ladam_attribute():
    from functools import partial
    from cgs_amd import ops
    from cgs_amd.model import GAN
    from cgs_amd.sampling.collaborator import Refiner
    gan, _ = setup("mnist", 4)
    d = dev()
    assert Refiner._loss_kind(GAN.loss_refine, d) == "bce"
    for kind in LC.REFINE_KINDS:
        assert Refiner._loss_kind(closure(kind), d) == kind
    assert Refiner._loss_kind(lambda l: (l - 1.0) ** 2, d) == "lsq" and Refiner._loss_kind(lambda l: -l, d) == "linear"
    assert Refiner._loss_kind(lambda l: 0.5 * (l - 1.0) ** 2, d) is None and Refiner._loss_kind(lambda l: l ** 2, d) is None
    assert Refiner._loss_kind(lambda l: torch.relu(1.0 - l), d) is None and Refiner._loss_kind(lambda l: (-l).mean(), d) is None
    D = partial(gan.discriminator, is_training=True, reuse=True)
    r = Refiner(2, 0.1, "ladam")
    r.set_env(D, gan.feature_to_data, closure("bce"))
    assert r.real_sigmoid_mean is None and r._engine_owner() is None and "real_sigmoid_mean" in r.why_generic
    r.real_sigmoid_mean = 0.6
    assert r._engine_owner() is gan
    with pytest.raises(ValueError):
        gan.build_refiner(2, 0.1, loss="hinge")
    ops.reset_variables()


@pytest.mark.parametrize("arch,B", CASES)
def test_eager_and_captured_programs_are_bit_equal_and_replay_a_new_real_score(arch, B):
    from cgs_amd import ops
    gan, f0 = setup(arch, B)
    eager, graph = gan.engine(B, use_graph=False), gan.engine(B, use_graph=True)
    assert eager._ladam is None and eager.mean_square is None                   # the ladam state is allocated at first use only
    for kind, method, s_real in (("lsq", "momentum", None), ("linear", "sgd", None), ("lsq", "ladam", 0.6), ("bce", "ladam", 0.6)):
        a = [t.clone() for t in eager.refine(f0, KSTEPS, RATE, method=method, loss=kind, real_sigmoid_mean=s_real)]
        b = [t.clone() for t in graph.refine(f0, KSTEPS, RATE, method=method, loss=kind, real_sigmoid_mean=s_real)]
        assert all(torch.equal(u, v) for u, v in zip(a, b)), (kind, method)
    n_graphs = len(graph._graphs)
    assert n_graphs == 4
    for s_real in (0.3, torch.tensor(0.45, device=dev())):                      # another value: the same graph, the eager result for it
        a = [t.clone() for t in eager.refine(f0, KSTEPS, RATE, method="ladam", loss="lsq", real_sigmoid_mean=s_real)]
        b = [t.clone() for t in graph.refine(f0, KSTEPS, RATE, method="ladam", loss="lsq", real_sigmoid_mean=s_real)]
        assert len(graph._graphs) == n_graphs
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    c = [t.clone() for t in eager.refine(f0, KSTEPS, RATE, method="ladam", loss="lsq", real_sigmoid_mean=0.6)]
    assert not torch.equal(c[4], a[4])                                          # (the real score does steer the steps)
    ops.reset_variables()


@pytest.mark.parametrize("arch,B", CASES)
def test_defaults_are_the_cross_entropy_program(arch, B):
    from cgs_amd import ops
    gan, f0 = setup(arch, B)
    for use_graph in (False, True):
        eng = gan.engine(B, use_graph=use_graph)
        a = [t.clone() for t in eng.refine(f0, KSTEPS, RATE)]
        b = [t.clone() for t in eng.refine(f0, KSTEPS, RATE, loss="bce")]
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        if use_graph:
            assert len(eng._graphs) == 1
    lm, g = (t.clone() for t in eng.compute_forward_logits_and_grad(f0))
    lm2, g2 = eng.compute_forward_logits_and_grad(f0, loss="bce")
    assert torch.equal(lm, lm2) and torch.equal(g, g2)
    ops.reset_variables()


@pytest.mark.parametrize("arch,B", CASES)
def test_ladam_program_against_a_loop_of_its_pieces(arch, B):
    """engine.refine(method="ladam") at K = 3 against: the engine's own evaluation and score per step, the float64 ladam step of
    loss_cases in between, the strict-> selection of collaborator.py:76."""
    from cgs_amd import ops
    gan, f0 = setup(arch, B)
    eng = gan.engine(B, use_graph=False)
    d = dev()
    s_real = 0.6
    theta = f0.cpu().numpy().astype(np.float64)
    m = v = avg = None
    logits = []
    for i in range(KSTEPS + 1):
        th32 = torch.from_numpy(theta.astype(np.float32)).to(d)
        lm, grad = eng.compute_forward_logits_and_grad(th32)
        logits.append(lm.cpu().numpy().astype(np.float64))
        if i == KSTEPS:
            break
        grad = grad.cpu().numpy().astype(np.float64)
        sig = eng.score(eng.feature_to_data(th32)).cpu().numpy().astype(np.float64).reshape(B)
        avg, gain = LC.ladam_state(float(np.float32(s_real)) - sig, avg, i == 0)
        theta, m, v = LC.ladam_step(theta, m, v, grad, gain, float(np.float32(RATE)), i == 0)
    logits = np.stack(logits)
    best = logits[0].copy()
    for i in range(1, KSTEPS + 1):
        best = np.where(logits[i] > best, logits[i], best)
    img, dl, ol, os_, of = eng.refine(f0, KSTEPS, RATE, method="ladam", real_sigmoid_mean=s_real)
    e0, e1 = relerr(dl.cpu(), logits[0]), relerr(ol.cpu(), best)
    print(f"{arch} ladam K={KSTEPS}: default_logit {e0:.2e}, optimal_logit {e1:.2e} of max|ref|; steps taken {os_.cpu().numpy()}")
    assert e0 < 1e-6 and e1 < 2e-3
    assert not torch.equal(of, f0) or float(os_.max()) == 1.0
    ops.reset_variables()


@pytest.mark.parametrize("kind", ("lsq", "hinge"))
def test_d_step_matches_float64_autograd(kind):
    """DShaper(loss=...) on mnist at batch 4: d_loss and every variable's gradient against float64 autograd of the branch the device
    evaluated -- the helper and the bars of tests/test_gpu_shaping.py (1e-5 on the loss, 2e-5 of max|ref| on a gradient)."""
    from test_gpu_shaping import _oracle_d_with_lrelu_sides, close, rnd
    from cgs_amd import lib as L
    from cgs_amd.engine import _BnTrainLrelu, _Conv, _Linear
    from cgs_amd.nets import to_device
    from cgs_amd.shaping import DShaper
    arch, B = "mnist", 4
    P = N.init_params(arch, 2019, True)
    real = rnd((B,) + tuple(N.ARCHS[arch]["img"]), 1).clamp(-1, 1)
    fake = torch.tanh(rnd((B,) + tuple(N.ARCHS[arch]["img"]), 2))
    d = dev()
    Pd = to_device(P, d)
    sh = DShaper(arch, Pd, B, d, learning_rate=1e-3, loss=kind)

    def lrelu_sides(x):
        sh.tape.forward(x.to(d))
        return [(st.out > 0).cpu() for st in sh.tape.stages
                if (isinstance(st, (_Conv, _Linear)) and st.epi == L.EPI_LRELU) or (isinstance(st, _BnTrainLrelu) and st.leak != 1.0)]
    sides_r, sides_f = lrelu_sides(real), lrelu_sides(fake)
    Pg = {k: (v.clone().double().requires_grad_(True) if k.startswith("discriminator/") and "moving" not in k else v.double()) for k, v in P.items()}
    lr = _oracle_d_with_lrelu_sides(arch, Pg, real.double(), sides_r)
    lf = _oracle_d_with_lrelu_sides(arch, Pg, fake.double(), sides_f)
    assert min(float((lr.abs() - 1).abs().min()), float((lf.abs() - 1).abs().min())) >= LC.KINK_MARGIN      # no logit on a hinge kink
    if kind == "lsq":
        loss = ((lr - 1.0) ** 2).mean() + (lf ** 2).mean()
    else:
        loss = torch.relu(1.0 - lr).mean() + torch.relu(1.0 + lf).mean()
    loss.backward()
    got_loss = sh.loss_and_grads(real.to(d), fake.to(d))
    print(f"D step {kind}: d_loss {got_loss.item():.6f} vs {loss.item():.6f}")
    assert abs(got_loss.item() - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    names = [k for k in Pg if Pg[k].requires_grad]
    checked = 0
    for st in sh.tape.stages:
        for attr in ("w", "b", "gamma", "beta"):
            if hasattr(st, "g_" + attr):
                name = [k for k in names if Pd[k] is getattr(st, attr)][0]
                g_ref, got = Pg[name].grad, getattr(st, "g_" + attr).cpu().double()
                if float(g_ref.abs().max()) < 1e-6:
                    assert float(got.abs().max()) < 1e-4
                else:
                    close(got, g_ref, 2e-5)
                checked += 1
    assert checked == len(names)


def test_lsq_trainer_iterations_are_bit_equal():
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B = "mnist", 4
    d = dev()
    rs = np.random.RandomState(0)
    real = torch.from_numpy(rs.uniform(-1, 1, (B,) + tuple(N.ARCHS[arch]["img"])).astype(np.float32)).to(d)
    z = torch.from_numpy(rs.uniform(-1, 1, (B, 62)).astype(np.float32)).to(d)
    outs = []
    for _ in range(2):
        P = to_device(N.init_params(arch, 2019, True), d)
        tr = GanTrainer(arch, P, B, d, loss="lsq")
        dl, gl = tr.iteration(real, z)
        outs.append((float(dl), float(gl), {k: v.clone() for k, v in P.items()}))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and outs[0][0] > 0
    assert all(torch.equal(outs[0][2][k], outs[1][2][k]) for k in outs[0][2])
    Pb = to_device(N.init_params(arch, 2019, True), d)
    db, gb = GanTrainer(arch, Pb, B, d).iteration(real, z)
    assert float(db) != outs[0][0]                                             # (not the cross-entropy step under another name)
