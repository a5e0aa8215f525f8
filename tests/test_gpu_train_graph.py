"""The train iteration of the image GAN replayed as a captured hipGraph (``training.GanTrainer(use_graph=True)``) and the two kernels that make
it capturable: ``cgs_adam_multi`` (one Adam launch per optimizer, ``lr_t`` in device memory) and ``cgs_bn_moving_update``.

The yardstick of the captured form is the eager form of the same process: losses, variables and Adam moments bit for bit (both forms run the
same kernels on the same bits; the multi-tensor Adam shares its per-element function with ``adam_kernel``), the generator's moving statistics
within 1e-6 of max|ref| (one kernel against six torch launches; they feed no training-mode forward).  Figures measured on one MI355X run:
adam_multi bit-equal to adam_step and against float64 w <= 1.9e-7 / m <= 6.0e-8 / v <= 1.5e-7 (bars 9.2e-7 / 2.4e-7 / 6.8e-7);
bn_moving_update <= 1.2e-7 (bar 1e-6); graph against eager: losses, variables and moments bit-equal, the moving statistics <= 2.2e-7 (bar 1e-6)."""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N
from test_gpu_train_kernels import BETA1, BETA2, EPS, adam_grad, check_adam_state, lr_at

SENTINEL = 777.25
MOVING_TOL = 1e-6       # one ops.bn update of the device's batch statistics (<= 1.1e-7 measured there)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def uniform(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).float()


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


# ================================================================================================ cgs_adam_multi
PAD = 37        # sentinel elements in front of, between and behind the tensors (odd: the slices are only 4-byte aligned)


def carve(sizes, fill):
    """One buffer holding a slice per size with PAD sentinels on both sides of each; -> (buffer, slices, mask of the sentinel elements)."""
    total = PAD + sum(n + PAD for n in sizes)
    buf = torch.full((total,), SENTINEL, device=dev())
    guard = torch.ones(total, dtype=torch.bool, device=dev())
    views, at = [], PAD
    for i, n in enumerate(sizes):
        v = buf[at:at + n]
        v.copy_(fill(i, n))
        guard[at:at + n] = False
        views.append(v)
        at += n + PAD
    return buf, views, guard


def run_adam_table(sizes):
    from cgs_amd import kernels as K
    d = dev()
    wb, w, guard = carve(sizes, lambda i, n: rnd((n,), 80 + i, 0.05).to(d))
    gb, g, _ = carve(sizes, lambda i, n: torch.zeros(n, device=d))
    mb, m, _ = carve(sizes, lambda i, n: torch.zeros(n, device=d))
    vb, v, _ = carve(sizes, lambda i, n: torch.zeros(n, device=d))
    table = K.AdamTable(list(zip(w, g, m, v)))
    built = (table.table.data_ptr(), table.plan.data_ptr(), table.lr_t.data_ptr(), table.table.clone(), table.plan.clone())
    assert table.n_chunks == sum((n + K.ADAM_CHUNK - 1) // K.ADAM_CHUNK for n in sizes)
    # the per-tensor kernel on copies
    w1, m1, v1 = [t.clone() for t in w], [t.clone() for t in m], [t.clone() for t in v]
    for t in range(1, 4):
        lr_t = lr_at(1e-3, t) * (1.0 + 0.37 * t)                 # a different, unrelated value each step
        grads = [adam_grad(n + 8, 10 * t + i)[1:n + 1] for i, n in enumerate(sizes)]      # ([0] is an exact zero: n = 1 would not move)
        for gi, new in zip(g, grads):
            gi.copy_(new)
        before = [(a.cpu(), b.cpu(), c.cpu()) for a, b, c in zip(w, m, v)]
        table.step(lr_t, BETA1, BETA2, EPS)
        for i, n in enumerate(sizes):
            if n:
                K.adam_step(w1[i], g[i], m1[i], v1[i], lr_t, BETA1, BETA2, EPS)
        for i, n in enumerate(sizes):
            assert torch.equal(w[i], w1[i]) and torch.equal(m[i], m1[i]) and torch.equal(v[i], v1[i]), (t, i, n)
            if n:
                check_adam_state((w[i], m[i], v[i]), before[i], grads[i], lr_t, f"adam_multi n={n} t={t}")
                assert not torch.equal(w[i].cpu(), before[i][0])
        for buf in (wb, mb, vb, gb):
            assert bool((buf[guard] == SENTINEL).all()), t           # bit-unchanged around every slice
        assert float(table.lr_t.cpu()[0]) == float(torch.tensor(lr_t, dtype=torch.float32))
    # nothing of the table was rebuilt: only the device scalar was rewritten between the steps
    assert built[:3] == (table.table.data_ptr(), table.plan.data_ptr(), table.lr_t.data_ptr())
    assert torch.equal(built[3], table.table) and torch.equal(built[4], table.plan)


def test_adam_multi_is_adam_step_bit_for_bit_on_every_slot_of_one_table():
    run_adam_table([1, 3, 255, 256, 257, 1025, 65537, 0])


def test_adam_multi_with_a_single_slot():
    run_adam_table([5000])


def test_adam_multi_refuses_an_empty_or_missing_table_and_accepts_empty_slots():
    from cgs_amd import kernels as K, lib
    l = lib.load()
    d = dev()
    stream = torch.cuda.current_stream().cuda_stream
    lr = torch.zeros(1, device=d)
    some = torch.zeros(64, dtype=torch.uint8, device=d)
    assert l.cgs_adam_multi(some.data_ptr(), 0, some.data_ptr(), 0, lr.data_ptr(), BETA1, BETA2, EPS, stream) == lib.EINVAL
    assert "adam_multi" in l.cgs_last_error().decode()
    assert l.cgs_adam_multi(None, 1, some.data_ptr(), 1, lr.data_ptr(), BETA1, BETA2, EPS, stream) == lib.EINVAL
    assert l.cgs_adam_multi(some.data_ptr(), 1, some.data_ptr(), 1, None, BETA1, BETA2, EPS, stream) == lib.EINVAL
    assert l.cgs_adam_multi(some.data_ptr(), 1, None, 1, lr.data_ptr(), BETA1, BETA2, EPS, stream) == lib.EINVAL
    with pytest.raises(lib.CgsError):
        K.AdamTable([])
    with pytest.raises(lib.CgsError):
        K.AdamTable([(torch.zeros(4, device=d), torch.zeros(3, device=d), torch.zeros(4, device=d), torch.zeros(4, device=d))])
    empty = K.AdamTable([tuple(torch.zeros(0, device=d) for _ in range(4))])          # only empty slots: legal, no launch
    assert empty.n_chunks == 0
    empty.step(1e-3, BETA1, BETA2, EPS)
    torch.cuda.synchronize()


# ================================================================================================ cgs_bn_moving_update
@pytest.mark.parametrize("C", [1, 3, 64, 130])
def test_bn_moving_update_twice_against_the_float64_formula(C):
    from cgs_amd import kernels as K
    d = dev()
    buf_m = torch.full((C + 2 * PAD,), SENTINEL, device=d)
    buf_v = torch.full((C + 2 * PAD,), SENTINEL, device=d)
    mm, mv = buf_m[PAD:PAD + C], buf_v[PAD:PAD + C]
    mm.copy_(rnd((C,), 20, 0.5))
    mv.copy_(rnd((C,), 21).abs() + 0.1)
    ref_m, ref_v = mm.cpu().double(), mv.cpu().double()
    for k in range(2):
        mean = rnd((C,), 22 + k).to(d)
        var = rnd((C,), 24 + k).abs() * 10.0 ** uniform((C,), 26 + k).mul(2)          # 1e-2 .. 1e+2 times |N(0, 1)|
        invstd = (1.0 / torch.sqrt(var + 1e-5)).to(d)
        K.bn_moving_update(mean, invstd, mm, mv, 0.9, 1e-5)
        ref_m = 0.9 * ref_m + (1.0 - 0.9) * mean.cpu().double()                        # from the device's own float32 mean / invstd
        ref_v = 0.9 * ref_v + (1.0 - 0.9) * (invstd.cpu().double().pow(-2) - 1e-5)
        e_m, e_v = rel(mm, ref_m), rel(mv, ref_v)
        print(f"bn_moving_update C={C} update {k + 1}: mean {e_m:.2e} var {e_v:.2e} (bar {MOVING_TOL:.0e})")
        assert e_m <= MOVING_TOL and e_v <= MOVING_TOL
    for buf in (buf_m, buf_v):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + C:] == SENTINEL).all())


def test_bn_moving_update_refuses_bad_arguments():
    from cgs_amd import kernels as K, lib
    d = dev()
    a = torch.ones(4, device=d)
    with pytest.raises(lib.CgsError):
        K.bn_moving_update(a, a, a.clone(), torch.ones(5, device=d), 0.9)
    with pytest.raises(lib.CgsError):
        K.bn_moving_update(a, a, a.clone(), a.clone(), 1.5)
    assert lib.load().cgs_bn_moving_update(None, a.data_ptr(), a.data_ptr(), a.data_ptr(), 4, 0.9, 1e-5, 0) == lib.EINVAL


# ================================================================================================ graph against eager
ITERS = 4


def inputs(arch, B, i, base=0):
    A = N.ARCHS[arch]
    return torch.tanh(rnd((B,) + tuple(A["img"]), 1300 + base + i)).to(dev()), uniform((B, A["z_dim"]), 1400 + base + i).to(dev())


def snapshot(tr):
    return dict(P={k: v.clone() for k, v in tr.P.items()},
                mv=[(m.clone(), v.clone()) for st in (tr.dshaper, tr.gstepper) for _, _, m, v in st.slots],
                t=(tr.dshaper.t, tr.gstepper.t))


@functools.lru_cache(maxsize=None)
def eager_reference(arch, B):
    """ITERS eager iterations from the seeded checkpoint, computed once per net: (initial host parameters, per iteration (d_loss, g_loss,
    snapshot)).  The snapshots stay on the device and are never written to."""
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    P = N.init_params(arch, 2019, True)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev())
    steps = []
    for i in range(ITERS):
        d_loss, g_loss = tr.iteration(*inputs(arch, B, i))
        assert tr.path == "eager"
        steps.append((d_loss.clone(), g_loss.clone(), snapshot(tr)))
    return P, steps


def assert_same_state(tr, want, what):
    """Variables, Adam moments and step counts bit-equal; the generator's moving statistics within MOVING_TOL of max|ref|."""
    got = snapshot(tr)
    assert got["t"] == want["t"], (what, got["t"], want["t"])
    worst = 0.0
    for k, v in want["P"].items():
        if k.startswith("generator/") and "moving_" in k:
            e = rel(got["P"][k], v)
            worst = max(worst, e)
            assert e <= MOVING_TOL, (what, k, e)
        else:
            assert torch.equal(got["P"][k], v), (what, k)
    for i, ((m, v), (m0, v0)) in enumerate(zip(got["mv"], want["mv"])):
        assert torch.equal(m, m0) and torch.equal(v, v0), (what, "Adam slot", i)
    return worst


@pytest.mark.parametrize("arch,B", [("mnist", 16), ("dcgan32", 8)])
def test_graph_iterations_equal_eager_iterations_bit_for_bit(arch, B):
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    P, steps = eager_reference(arch, B)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev(), use_graph=True)
    assert tr.path == "eager" and tr.graph_fallback is None
    for i, (d_ref, g_ref, want) in enumerate(steps):
        d_loss, g_loss = tr.iteration(*inputs(arch, B, i))
        assert tr.path == ("eager" if i == 0 else "graph") and tr.graph_fallback is None, (i, tr.path, tr.graph_fallback)
        assert torch.equal(d_loss, d_ref) and torch.equal(g_loss, g_ref), (i, float(d_loss), float(d_ref), float(g_loss), float(g_ref))
        assert math.isfinite(float(d_loss)) and math.isfinite(float(g_loss))
        worst = assert_same_state(tr, want, f"{arch} iteration {i + 1}")
        print(f"{arch} B={B} iteration {i + 1} ({tr.path}): losses, variables, m, v bit-equal; moving statistics {worst:.2e} (bar {MOVING_TOL:.0e})")
    moved = next(k for k in P if k.startswith("generator/") and "moving_" not in k)
    assert not torch.equal(steps[0][2]["P"][moved], steps[-1][2]["P"][moved])


def test_capture_records_the_pack_kernels_even_when_the_packed_copies_are_fresh():
    """Between the warm-up and the capture, forwards on the trainer's own stream leave fresh packed copies of G's and D's weights there.  The
    program must still contain the pack kernels (every replay changes the weights): without them the first G forward of iteration 3 reads the
    weights of iteration 2."""
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B = "mnist", 16
    P, steps = eager_reference(arch, B)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev(), use_graph=True)
    tr.iteration(*inputs(arch, B, 0))
    real, z = inputs(arch, B, 0)
    torch.cuda.synchronize()
    with torch.cuda.stream(tr._gstream):                 # tape forwards only: no variable, moment or moving statistic is written
        tr.dshaper.tape.forward(tr.gstepper.g.forward(z))
    torch.cuda.synchronize()
    for i in range(1, ITERS):
        d_loss, g_loss = tr.iteration(*inputs(arch, B, i))
        assert tr.path == "graph"
        assert torch.equal(d_loss, steps[i][0]) and torch.equal(g_loss, steps[i][1]), i
        assert_same_state(tr, steps[i][2], f"iteration {i + 1}")


def test_returned_losses_and_the_callers_inputs_are_not_aliased_by_the_graph():
    """Losses of iteration k survive iteration k + 1 (they are not the graph's static outputs), and overwriting ``real`` / ``z`` after a call
    changes nothing: the program reads its own static copies."""
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B = "mnist", 16
    P, steps = eager_reference(arch, B)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev(), use_graph=True)
    kept = []
    for i in range(ITERS):
        real, z = inputs(arch, B, i)
        out = tr.iteration(real, z)
        real.fill_(float("nan"))
        z.fill_(float("nan"))
        kept.append((out, float(out[0]), float(out[1])))
        for (d_loss, g_loss), d0, g0 in kept:
            assert float(d_loss) == d0 and float(g_loss) == g0
    assert len({t.data_ptr() for out, _, _ in kept for t in out}) == 2 * ITERS
    assert tr.path == "graph"
    for (out, _, _), (d_ref, g_ref, _) in zip(kept, steps):
        assert torch.equal(out[0], d_ref) and torch.equal(out[1], g_ref)
    assert_same_state(tr, steps[-1][2], "after overwritten inputs")


def test_load_under_a_live_graph_resets_the_optimizer_and_keeps_the_graph(tmp_path):
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B = "mnist", 16
    P, steps = eager_reference(arch, B)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev(), use_graph=True)
    path = os.path.join(str(tmp_path), "start.npz")
    tr.save(path)
    for i in range(3):
        tr.iteration(*inputs(arch, B, i, base=50))
    graph = tr._graph
    assert tr.path == "graph" and graph is not None and tr.gstepper.t == 3
    tr.load(path)
    assert tr.gstepper.t == 0 and tr.dshaper.t == 0
    for i in range(2):          # the file holds the fixture's start: two more iterations are the fresh eager trainer's first two
        d_loss, g_loss = tr.iteration(*inputs(arch, B, i))
        assert tr.path == "graph" and tr._graph is graph
        assert torch.equal(d_loss, steps[i][0]) and torch.equal(g_loss, steps[i][1])
        assert_same_state(tr, steps[i][2], f"iteration {i + 1} after load")


def test_engine_refreshed_after_a_replayed_iteration_equals_a_fresh_one(tmp_path):
    from cgs_amd import checkpoint
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B, K = "mnist", 16, 3
    P, _ = eager_reference(arch, B)
    Pd = to_device(P, dev())
    eng = RefineEngine(arch, Pd, B, dev())
    zd = uniform((B, 62), 5).to(dev())
    tr = GanTrainer(arch, Pd, B, dev(), engine=eng, use_graph=True)
    tr.iteration(*inputs(arch, B, 0))
    warm = [t.clone() for t in eng.refine_from_z(zd, K, 0.1)]
    tr.iteration(*inputs(arch, B, 1))
    assert tr.path == "graph"
    after = [t.clone() for t in eng.refine_from_z(zd, K, 0.1)]
    path = os.path.join(str(tmp_path), "gan.npz")
    tr.save(path)
    fresh = [t.clone() for t in RefineEngine(arch, to_device(checkpoint.load(path), dev()), B, dev()).refine_from_z(zd, K, 0.1)]
    assert not torch.equal(after[0], warm[0])
    for a, b in zip(after, fresh):
        assert torch.equal(a, b)


def test_a_wrong_input_shape_raises_and_leaves_the_state_untouched():
    from cgs_amd import lib
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B = "mnist", 16
    P, steps = eager_reference(arch, B)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev(), use_graph=True)
    real, z = inputs(arch, B, 0)
    for when in range(3):                    # before the warm-up, before the capture, under a live graph
        before = snapshot(tr)
        for bad in ((real[:B - 1], z), (real, z[:, :61]), (real.reshape(B, 28 * 28), z), (real, z[:B - 1])):
            with pytest.raises(lib.CgsError):
                tr.iteration(*bad)
        after = snapshot(tr)
        assert after["t"] == before["t"] == (when, when)
        assert all(torch.equal(after["P"][k], v) for k, v in before["P"].items())
        assert all(torch.equal(a, c) and torch.equal(b, e) for (a, b), (c, e) in zip(after["mv"], before["mv"]))
        tr.iteration(*inputs(arch, B, when))
        assert_same_state(tr, steps[when][2], f"iteration {when + 1} after refused calls")
    assert tr.path == "graph"


def test_profiling_runs_eagerly_and_a_refused_capture_falls_back(monkeypatch):
    from cgs_amd import kernels as K
    from cgs_amd.nets import to_device
    from cgs_amd.training import GanTrainer
    arch, B = "mnist", 16
    P, steps = eager_reference(arch, B)
    tr = GanTrainer(arch, to_device(P, dev()), B, dev(), use_graph=True)
    monkeypatch.setattr(K, "PROFILE", {})
    tr.iteration(*inputs(arch, B, 0))
    tr.iteration(*inputs(arch, B, 1))
    assert tr.path == "eager" and tr._graph is None and tr.graph_fallback is None
    monkeypatch.setattr(K, "PROFILE", None)
    assert_same_state(tr, steps[1][2], "two profiled iterations")

    class Refuses:                           # the capture context refusing, as HIP or the allocator might
        def __init__(self, *a, **k):
            raise RuntimeError("capture refused (simulated)")
    tr.iteration(*inputs(arch, B, 2))        # the warm-up of the graph path
    monkeypatch.setattr(torch.cuda, "graph", Refuses)
    tr.iteration(*inputs(arch, B, 3))
    assert tr.path == "eager" and "capture refused (simulated)" in tr.graph_fallback
    assert_same_state(tr, steps[3][2], "after a refused capture")
