"""Synchronised batch statistics: one logical batch split over ranks must reproduce the unsplit batch.

(a) kernel level, one process: the sums of two half batches added = the all-reduce; each half applied with the global
    sums equals the whole-batch bn forward / backward-data.
(b) engine level, two processes sharing the one GPU of the test box, the 2*C sums all-reduced over a gloo group (RCCL
    needs one device per rank): each rank refines half of a batch with sync_bn; the halves together equal the
    single-process whole-batch refinement."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


@pytest.mark.parametrize("M,C,leak", [(4096, 128, 0.2), (64, 1024, 0.2), (1000, 64, 1.0)])
def test_split_sums_equal_whole_batch(M, C, leak):
    from cgs_amd import kernels as K
    d = dev()
    x, dy = (rnd((M, C), 1) * 1.7 + 0.3).to(d), rnd((M, C), 2).to(d)
    gamma, beta = (rnd((C,), 3).abs() + 0.5).to(d), rnd((C,), 4, 0.3).to(d)
    y, mean, invstd = K.bn_train_lrelu_fwd(x, gamma, beta, leak)
    dx = K.bn_train_lrelu_bwd_data(dy.clone(), x, gamma, beta, mean, invstd, leak)
    h = M // 2 if M % 2 == 0 else M // 3          # uneven split too
    parts = [(x[:h].contiguous(), dy[:h].contiguous()), (x[h:].contiguous(), dy[h:].contiguous())]
    sums = [K.bn_sync_fwd_sums(px, torch.empty((2, C), dtype=torch.float64, device=d)) for px, _ in parts]
    tot = sums[0] + sums[1]
    ys, stats = [], []
    for px, _ in parts:
        yy, m, iv = K.bn_sync_fwd_apply(px, gamma, beta, tot, M, leak)
        ys.append(yy); stats.append((m, iv))
    assert torch.allclose(stats[0][0], mean, rtol=0, atol=1e-6) and torch.allclose(stats[0][1], invstd, rtol=1e-6, atol=0)
    assert torch.equal(stats[0][0], stats[1][0]) and torch.equal(stats[0][1], stats[1][1])
    assert torch.allclose(torch.cat(ys), y, rtol=1e-5, atol=1e-5)
    bs = [K.bn_sync_bwd_sums(pdy, px, gamma, beta, m, iv, torch.empty((2, C), dtype=torch.float64, device=d), leak)
          for (px, pdy), (m, iv) in zip(parts, stats)]
    btot = bs[0] + bs[1]
    dxs = [K.bn_sync_bwd_apply(pdy.clone(), px, gamma, beta, m, iv, btot, M, leak) for (px, pdy), (m, iv) in zip(parts, stats)]
    got = torch.cat(dxs)
    assert (got - dx).abs().max().item() <= 2e-5 * dx.abs().max().item()


@pytest.mark.parametrize("M,C", [(129, 4), (129, 40)])
def test_one_rank_equals_the_unsynchronised_norm(M, C):
    """One rank: the second halves finish the statistics from ONE slice of sums (bn_finalize_slices_kernel /
    bn_finalize2_slices_kernel with nslices = 1) and must give what bn_train_lrelu_fwd / _bwd_data give, within the bars above.
    129 rows: the smallest M past the one-launch small path; C = 40: one tail channel group."""
    from cgs_amd import kernels as K
    d, leak = dev(), 0.2
    x, dy = (rnd((M, C), 1) * 1.7 + 0.3).to(d), rnd((M, C), 2).to(d)
    gamma, beta = (rnd((C,), 3).abs() + 0.5).to(d), rnd((C,), 4, 0.3).to(d)
    y, mean, invstd = K.bn_train_lrelu_fwd(x, gamma, beta, leak)
    dx = K.bn_train_lrelu_bwd_data(dy.clone(), x, gamma, beta, mean, invstd, leak)

    def run():
        sums = K.bn_sync_fwd_sums(x, torch.empty((2, C), dtype=torch.float64, device=d))
        ys, m, iv = K.bn_sync_fwd_apply(x, gamma, beta, sums, M, leak)
        bsums = K.bn_sync_bwd_sums(dy, x, gamma, beta, m, iv, torch.empty((2, C), dtype=torch.float64, device=d), leak)
        return ys, m, iv, K.bn_sync_bwd_apply(dy.clone(), x, gamma, beta, m, iv, bsums, M, leak)

    ys, m, iv, dxs = run()
    assert torch.allclose(m, mean, rtol=0, atol=1e-6) and torch.allclose(iv, invstd, rtol=1e-6, atol=0)
    assert torch.allclose(ys, y, rtol=1e-5, atol=1e-5)
    assert (dxs - dx).abs().max().item() <= 2e-5 * dx.abs().max().item()
    assert all(torch.equal(a, b) for a, b in zip((ys, m, iv, dxs), run()))          # bit-equal over two runs


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, arch, B, K, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device, ARCHS
    from oracle import nets_ref as N
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = torch.device("cuda:0")
    P = to_device(N.init_params(arch, 2019, True), d)
    z = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (B, ARCHS[arch]["z_dim"])).astype(np.float32)).to(d)
    h = B // world
    eng = RefineEngine(arch, P, h, d, sync_bn=True)
    img, dl, ol, st, of = [t.cpu() for t in eng.refine_from_z(z[rank * h:(rank + 1) * h], K, 0.1)]
    torch.save(dict(img=img, dl=dl, ol=ol, st=st, of=of), f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("arch,B,K", [("mnist", 16, 3), ("dcgan32", 8, 2)])
def test_two_ranks_reproduce_the_whole_batch(arch, B, K, tmp_path):
    import torch.multiprocessing as mp
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device, ARCHS
    from oracle import nets_ref as N
    out = str(tmp_path / "shard")
    mp.spawn(_worker, args=(2, _free_port(), arch, B, K, out), nprocs=2, join=True)
    d = dev()
    P = to_device(N.init_params(arch, 2019, True), d)
    z = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (B, ARCHS[arch]["z_dim"])).astype(np.float32)).to(d)
    img, dl, ol, st, of = [t.cpu() for t in RefineEngine(arch, P, B, d).refine_from_z(z, K, 0.1)]
    sh = [torch.load(f"{out}.{r}") for r in range(2)]
    cat = lambda k: torch.cat([s[k] for s in sh])
    assert torch.allclose(cat("dl"), dl, rtol=1e-4, atol=1e-5)          # D(G(theta0)) with whole-batch statistics
    assert torch.allclose(cat("ol"), ol, rtol=2e-3, atol=2e-4)
    assert torch.allclose(cat("of"), of, rtol=0, atol=2e-3 * of.abs().max().item())
    assert torch.allclose(cat("img"), img, rtol=0, atol=5e-3)
    same = (cat("st") == st)
    assert same.float().mean().item() >= 0.85                            # ties in the strict '>' may flip a step index
    # and it is NOT what two independent half batches give (the statistics really are shared)
    eng_h = RefineEngine(arch, P, B // 2, d)
    dl_indep = torch.cat([eng_h.refine_from_z(z[i * (B // 2):(i + 1) * (B // 2)], K, 0.1)[1].cpu().clone() for i in range(2)])
    assert (dl_indep - dl).abs().max().item() > 10 * (cat("dl") - dl).abs().max().item()
