"""csrc/kde2d.hip on the device against the float64 state of cgs_amd.metrics.density_state_of.

Bar: every cell of the UN-normalised map within 1e-4 of max|ref| (the project's bar for one forward evaluation), n exact, no cell left out.
Where it comes from: per (cell, sample) pair the kernel rounds the coordinate difference once, W (pre-scaled, rounded to fp32 once per block)
and five more fp32 operations before v_exp_f32 (1 ulp): the exponent q (in log2 units) carries a relative error of a few 2^-24, the term
2^-q a relative error of ~ q ln2 4 2^-24 <= 2e-5 at q = 100 -- and a term that far down is 2^-100 of a near one.  An fp32 run adds at most
128 terms (<= 128 2^-24 = 7.6e-6 relative to the run's sum, all terms positive), everything after that is double.  The worst measured ratio
|delta| / max|ref| is printed per case.

Sizes.  The slicing depends on (n, cells) alone (kde_plan, restated in test_kde_cases_cpu.plan): on a grid of one tile a slice is 64 samples
up to n = 32768 (n = 1, 63, 64, 65: one slice; 127: one slice of 128 less one; 128: two slices; 129: 128 + 1; 193: 128 + 65, one run and a
second, partial one), on 100 x 100 n = 4099 is 33 slices of 128 with 3 samples in the last, n = 10000 is 40 slices of 256 = two staged runs
each.  Grids: 1 x 1, 1 x 7, 3 x 5 (a thread's four cells partly past the grid), 1025 x 1 and 1 x 1025 (one cell past the 1024-cell tile in
each direction), 100 x 100 (the reference's: ten tiles, the last one partial)."""
import functools

import numpy as np
import pytest
import torch

import kde_cases as KC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 1e-4
SMALL_N = [1, 63, 64, 65, 127, 128, 129, 193]
CASES = ([(n, g) for g in ((1, 1), (1, 7), (3, 5)) for n in SMALL_N + [4099]]
         + [(n, g) for g in ((1025, 1), (1, 1025)) for n in (1, 65, 193, 4099)]
         + [(n, (100, 100)) for n in (64, 4099, 10000)])


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _samples():
    x = (np.random.RandomState(7).randn(10000, 2) * 1.2).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _whiten(rho=0.6):
    from cgs_amd.metrics import kde_whiten
    w, _ = kde_whiten(np.array([[1.0, rho * np.sqrt(1.5)], [rho * np.sqrt(1.5), 1.5]]), 64)       # f = 0.25: kernel widths ~ 0.25 .. 0.3
    w.setflags(write=False)
    return w


def _axis(g, near):
    """g > 1: np.linspace(-3, 3, g) in fp32; one point: 0.1 beside the first sample's coordinate (so the map has a cell of order 1)."""
    return np.linspace(-3.0, 3.0, g).astype(np.float32) if g > 1 else np.array([near + 0.1], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _case(n, grid):
    """(samples, axes, the host twin's flat [sums | n], start contents) -- computed once, read-only."""
    from cgs_amd import metrics as M
    x = _samples()[:n]
    ax, ay = _axis(grid[0], x[0, 0]), _axis(grid[1], x[0, 1])
    st = M.density_state_of(x, ax, ay, _whiten())
    ref = np.concatenate([st["sums"].reshape(-1), [float(st["n"])]])
    rs = np.random.RandomState(n + 7 * grid[0] + grid[1])
    start = np.concatenate([np.abs(rs.randn(ref.size - 1)) * ref[:-1].max(), [float(rs.randint(0, 1000))]])
    for v in (ax, ay, ref, start):
        v.setflags(write=False)
    return x, ax, ay, ref, start


def _check(tag, got, ref, start):
    """got against start + ref: the added part within BAR of max|ref|, every cell, n exact."""
    assert np.isfinite(got).all(), tag
    assert got[-1] == start[-1] + ref[-1], (tag, got[-1])
    top = np.abs(ref[:-1]).max()
    assert top > 1e-30, (tag, top)                                      # the case has something to measure
    err = np.abs(got[:-1] - (start[:-1] + ref[:-1]))
    slack = 4.0 * 2.0 ** -53 * np.abs(start[:-1])                        # (the one double addition onto the contents)
    ratio = float((np.maximum(err - slack, 0.0) / top).max())
    print(f"\n[kde2d {tag}] worst |delta| / max|ref| = {ratio:.3g} (bar {BAR:g})")
    assert ratio <= BAR, (tag, ratio)
    return ratio


@pytest.mark.parametrize("n,grid", CASES)
def test_kernel_every_cell_within_the_bar_n_exact_reruns_bit_equal(n, grid):
    from cgs_amd import kernels as K
    x, ax, ay, ref, start = _case(n, grid)
    xd, axd, ayd, wd = _dev(x), _dev(ax), _dev(ay), _dev(_whiten())
    for onto in ("zeros", "contents"):
        s0 = np.zeros_like(start) if onto == "zeros" else start
        st = _dev(s0)
        K.kde2d_accumulate(xd, axd, ayd, wd, st)
        _check(f"n={n} grid={grid[0]}x{grid[1]} {onto}", st.cpu().numpy(), ref, s0)
        for ws in K._mom_ws.values():                                   # a NaN-filled workspace does not leak, and the rerun is bit-equal
            ws.fill_(float("nan"))
        st2 = _dev(s0)
        K.kde2d_accumulate(xd, axd, ayd, wd, st2)
        assert torch.equal(st, st2)


def test_an_update_in_three_batches_gives_the_map_of_one():
    from cgs_amd import kernels as K
    n, grid = 4099, (100, 100)
    x, ax, ay, ref, start = _case(n, grid)
    axd, ayd, wd, st = _dev(ax), _dev(ay), _dev(_whiten()), _dev(start)
    for a, b in ((0, 5), (5, 2000), (2000, n)):
        K.kde2d_accumulate(_dev(x[a:b]), axd, ayd, wd, st)
    K.kde2d_accumulate(_dev(x[:0]), axd, ayd, wd, st)                    # no sample: nothing moves
    _check("4099 in three updates", st.cpu().numpy(), ref, start)


def test_a_sample_on_a_grid_point_adds_exactly_one_to_that_cell():
    from cgs_amd import kernels as K
    from cgs_amd import metrics as M
    ax, ay = M.kde_axes(4.0, 9), M.kde_axes(2.5, 12)
    x = np.array([[ax[3], ay[5]], [ax[8], ay[0]]], dtype=np.float32)
    for k in range(2):                                                   # ONE sample on a point: exactly 1.0 there, whatever the bandwidth
        st = torch.zeros(9 * 12 + 1, dtype=torch.float64, device=DEV)
        K.kde2d_accumulate(_dev(x[k:k + 1]), _dev(ax), _dev(ay), _dev(_whiten()), st)
        got = st.cpu().numpy()
        assert got[[3 * 12 + 5, 8 * 12 + 0][k]] == 1.0 and got[-1] == 1.0
        ref = M.density_state_of(x[k:k + 1], ax, ay, _whiten())["sums"]
        _check(f"sample {k} on a grid point", got, np.concatenate([ref.reshape(-1), [1.0]]), np.zeros(9 * 12 + 1))
    w = _whiten() * 1e3                                                  # both samples under W x 1e3: every other cell is exactly 0
    assert np.array_equal(np.nonzero(M.density_state_of(x, ax, ay, w)["sums"]), [[3, 8], [5, 0]])
    st = torch.zeros(9 * 12 + 1, dtype=torch.float64, device=DEV)
    K.kde2d_accumulate(_dev(x), _dev(ax), _dev(ay), _dev(w), st)
    want = np.zeros((9, 12))
    want[3, 5] = want[8, 0] = 1.0
    assert np.array_equal(st.cpu().numpy(), np.concatenate([want.reshape(-1), [2.0]]))


def test_a_pool_far_from_the_grid_leaves_exact_zeros_and_no_nan():
    from cgs_amd import kernels as K
    from cgs_amd import metrics as M
    ax = M.kde_axes(4.0, 37)
    x = _samples()[:1000] + np.float32(1000.0)
    for w in (_whiten(), _whiten() * 1e3):
        assert not M.density_state_of(x[:50], ax, ax, w)["sums"].any()  # the float64 definition is exactly 0 there too
        st = torch.zeros(37 * 37 + 1, dtype=torch.float64, device=DEV)
        K.kde2d_accumulate(_dev(x), _dev(ax), _dev(ax), _dev(w), st)
        got = st.cpu().numpy()
        assert np.isfinite(got).all() and not got[:-1].any() and got[-1] == 1000.0


def test_a_strongly_correlated_bandwidth_uses_the_off_diagonal_term():
    from cgs_amd import kernels as K
    from cgs_amd import metrics as M
    x = KC.pool("corr", 2000)
    ax = M.kde_axes(4.0, 40)
    whiten, norm = M.kde_whiten(np.cov(x.astype(np.float64), rowvar=False), len(x))
    assert abs(whiten[1]) > 2.0 * whiten[0]                               # rho = 0.95: w10 = -rho / sqrt(1 - rho^2) w00-ish
    ref = M.density_state_of(x, ax, ax, whiten)
    st = torch.zeros(40 * 40 + 1, dtype=torch.float64, device=DEV)
    K.kde2d_accumulate(_dev(x), _dev(ax), _dev(ax), _dev(whiten), st)
    _check("rho = 0.95", st.cpu().numpy(), np.concatenate([ref["sums"].reshape(-1), [2000.0]]), np.zeros(40 * 40 + 1))
    wrong = M.density_state_of(x, ax, ax, [whiten[0], 0.0, whiten[2]])["sums"]                     # the bar tells the two apart
    assert np.abs(wrong - ref["sums"]).max() > 100 * BAR * ref["sums"].max()
    want = KC.density(x, ax, ax)
    assert np.abs(st.cpu().numpy()[:-1].reshape(40, 40) / norm - want).max() <= BAR * want.max()


def test_bad_arguments_raise_and_change_nothing():
    from cgs_amd import kernels as K
    from cgs_amd import lib as L
    x = torch.ones((300, 2), dtype=torch.float32, device=DEV)
    ax, ay = torch.zeros(5, dtype=torch.float32, device=DEV), torch.zeros(4, dtype=torch.float32, device=DEV)
    w = torch.ones(3, dtype=torch.float64, device=DEV)
    st = torch.zeros(21, dtype=torch.float64, device=DEV)
    big = torch.zeros(1025, dtype=torch.float32, device=DEV)
    bad = [lambda: K.kde2d_accumulate(x.cpu(), ax, ay, w, st), lambda: K.kde2d_accumulate(x.double(), ax, ay, w, st),
           lambda: K.kde2d_accumulate(torch.ones((2, 300), dtype=torch.float32, device=DEV).t(), ax, ay, w, st),
           lambda: K.kde2d_accumulate(x.view(200, 3), ax, ay, w, st), lambda: K.kde2d_accumulate(x, ax.double(), ay, w, st),
           lambda: K.kde2d_accumulate(x, ax.cpu(), ay, w, st), lambda: K.kde2d_accumulate(x, ax.view(5, 1), ay, w, st),
           lambda: K.kde2d_accumulate(x, ax[:0], ay, w, st[:1]), lambda: K.kde2d_accumulate(x, big, torch.zeros(1024, dtype=torch.float32, device=DEV), w, st),
           lambda: K.kde2d_accumulate(x, ax, ay, w.float(), st), lambda: K.kde2d_accumulate(x, ax, ay, w.cpu(), st),
           lambda: K.kde2d_accumulate(x, ax, ay, w[:2], st), lambda: K.kde2d_accumulate(x, ax, ay, w, st[:-1]),
           lambda: K.kde2d_accumulate(x, ax, ay, w, st.float()), lambda: K.kde2d_accumulate(x, ay, ax, w, st[:-1])]
    for f in bad:
        with pytest.raises(L.CgsError):
            f()
    l = L.load()
    need = int(l.cgs_kde2d_ws_bytes(300, 5, 4))
    assert need == 3 * 20 * 8                                            # three slices: 128, 128 and 44 samples
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=DEV)
    args = lambda n, gx, gy, wsp, nbytes: l.cgs_kde2d_accumulate(x.data_ptr(), n, ax.data_ptr(), gx, ay.data_ptr(), gy, w.data_ptr(), st.data_ptr(), wsp, nbytes, None)
    assert args(300, 0, 4, ws.data_ptr(), need) == L.EINVAL
    assert args(300, 5, 0, ws.data_ptr(), need) == L.EINVAL
    assert args(300, 1025, 1024, ws.data_ptr(), need) == L.EINVAL
    assert args(-1, 5, 4, ws.data_ptr(), need) == L.EINVAL
    assert args(300, 5, 4, ws.data_ptr(), need - 8) == L.EWORKSPACE
    assert args(300, 5, 4, None, need) == L.EWORKSPACE
    assert args(300, 5, 4, ws.data_ptr() + 4, need) == L.EINVAL          # a misaligned workspace
    torch.cuda.synchronize()
    assert not st.any() and not ws.any()                                  # nothing was launched
    assert args(300, 5, 4, ws.data_ptr(), need) == L.OK
    torch.cuda.synchronize()
    assert st[-1].item() == 300 and (st[:-1] > 0).all()
