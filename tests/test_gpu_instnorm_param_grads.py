"""``cgs_instnorm_param_grads`` (csrc/wgrad_dot.hip): an instance norm's scale / offset gradients from the per-sample sums its backward-data
call leaves in its workspace, against the float64 formula on the branch the device evaluated (the sign of the stage's OUTPUT decides each
LeakyReLU, as in test_gpu_shaping.py).  Bar: 2e-5 of max|ref|, the project's bar for parameter gradients against float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops_ref as R

# (B, H, W, C): HW = 64 one launch | odd HW | HW = 129: the first size on the three-launch path | several partial rows per sample |
# many samples | B = 1
SHAPES = [(3, 8, 8, 16), (5, 7, 9, 32), (2, 3, 43, 8), (2, 32, 32, 64), (64, 4, 4, 128), (1, 12, 12, 8)]
LEAKS = [0.2, 0.0, 1.0]
BAR = 2e-5


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs().max().item()
    ref = want.abs().max().item() + 1e-30
    print(f"{what}: max|delta|={err:.3e} max|ref|={ref:.3e} ratio={err / ref:.3e} bar={BAR:.1e}")
    assert torch.isfinite(got).all() and err <= BAR * ref, f"{what}: max|delta|={err:.3e} vs max|ref|={ref:.3e}"


class Case:
    """Inputs on the device, the forward done, and the float64 reference of the branch that forward took."""

    def __init__(self, shape, leak):
        from cgs_amd import kernels as K
        B, H, W, C = shape
        d = dev()
        self.leak = leak
        self.x = (rnd(shape, 1) * 1.5 + 0.3).to(d)
        self.scale, self.offset = (1.0 + 0.2 * rnd((C,), 2)).to(d), (0.1 * rnd((C,), 3)).to(d)
        self.dy = rnd(shape, 4).to(d)
        self.y, self.mean, self.invstd = K.instnorm_lrelu_fwd(self.x, self.scale, self.offset, leak)
        x64 = self.x.cpu().double()
        mean = x64.mean(dim=(1, 2), keepdim=True)
        xhat = (x64 - mean) / torch.sqrt(((x64 - mean) ** 2).mean(dim=(1, 2), keepdim=True) + R.BN_EPS)
        dd = self.dy.cpu().double()
        dd = dd * torch.where(self.y.cpu() > 0, torch.ones_like(dd), torch.full_like(dd, leak))
        self.want_scale, self.want_offset = (dd * xhat).sum(dim=(0, 1, 2)), dd.sum(dim=(0, 1, 2))

    def run(self, dscale, doffset, accumulate=False):
        from cgs_amd import kernels as K
        K.instnorm_lrelu_bwd_data(self.dy, self.x, self.scale, self.offset, self.mean, self.invstd, self.leak)
        K.instnorm_param_grads(self.x, dscale, doffset, accumulate)
        return dscale, doffset


@pytest.mark.parametrize("leak", LEAKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_param_grads_match_float64(shape, leak):
    c = Case(shape, leak)
    C = shape[3]
    nan = lambda: torch.full((C,), float("nan"), device=dev())
    gs, go = c.run(nan(), nan())                                   # NaN-filled outputs are overwritten
    close(gs, c.want_scale, f"dscale {shape} leak={leak}")
    close(go, c.want_offset, f"doffset {shape} leak={leak}")
    gs2, go2 = c.run(nan(), nan())                                 # a rerun is bit-identical
    assert torch.equal(gs, gs2) and torch.equal(go, go2)
    old_s, old_o = rnd((C,), 8, 30.0), rnd((C,), 9, 30.0)          # accumulation onto unrelated contents
    as_, ao = c.run(old_s.to(dev()), old_o.to(dev()), accumulate=True)
    close(as_, old_s.double() + c.want_scale, f"accumulated dscale {shape} leak={leak}")
    close(ao, old_o.double() + c.want_offset, f"accumulated doffset {shape} leak={leak}")
    assert not torch.equal(as_.cpu(), old_s)
