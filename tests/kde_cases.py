"""The density map of a 2-D pool, stated once in float64 numpy: the arithmetic of the reference's draw_kde
(sampling/utils_sampling.py:97-112) without the drawing.  The package's metrics.kde_* / density_* functions and the kernel of
csrc/kde2d.hip are tested against this file, and this file against live scipy (tests/test_kde_cases_cpu.py).

    grid       each axis np.linspace(-scale, scale, nbins) in float64; ``axes32`` rounds it to fp32, the coordinates the device map is
               defined at (widened exactly).  map[i, j] is the point (x_i, y_j), as np.mgrid lays it out.
    bandwidth  f = bw_scale n^(-1/6)  (Scott's factor for d = 2, halved by set_bandwidth(k.factor / 2.));  C = f^2 cov(samples, ddof=1),
               C = L L^T, W = L^-1 = [[w00, 0], [w10, w11]].  n < 2 or a C that is not positive definite: ValueError.
    value      density(g) = sum_k exp(-1/2 |W (g - x_k)|^2) / (n 2 pi sqrt(det C))
"""
import functools

import numpy as np


def axes64(scale, nbins=100):
    return np.linspace(-scale, scale, nbins)


def axes32(scale, nbins=100):
    return axes64(scale, nbins).astype(np.float32)


def bandwidth(samples, bw_scale=0.5):
    """(W [2, 2] lower triangular, sqrt(det C)) of the pool."""
    x = np.asarray(samples, dtype=np.float64)
    n = x.shape[0]
    if n < 2:
        raise ValueError("a bandwidth needs at least 2 samples")
    f = bw_scale * n ** (-1.0 / 6.0)
    c = f * f * np.cov(x, rowvar=False, ddof=1)
    try:
        l = np.linalg.cholesky(c)
    except np.linalg.LinAlgError:
        raise ValueError("the pool's covariance is not positive definite")
    return np.linalg.inv(l), float(l[0, 0] * l[1, 1])


def kernel_sums(samples, axis_x, axis_y, W, chunk=512):
    """sums[i, j] = sum_k exp(-1/2 |W (g_ij - x_k)|^2) in float64: the difference first, then the whitening."""
    x = np.asarray(samples, dtype=np.float64)
    ax, ay = np.asarray(axis_x, dtype=np.float64), np.asarray(axis_y, dtype=np.float64)
    out = np.zeros((ax.size, ay.size))
    for a in range(0, x.shape[0], chunk):
        d = np.stack(np.broadcast_arrays(ax[None, :, None] - x[a:a + chunk, 0, None, None], ay[None, None, :] - x[a:a + chunk, 1, None, None]), axis=-1)
        w = d @ W.T                                                          # [m, gx, gy, 2]: W (g - x)
        out += np.exp(-0.5 * (w * w).sum(axis=-1)).sum(axis=0)
    return out


def density(samples, axis_x, axis_y, bw_scale=0.5):
    """The [gx, gy] float64 map of the pool on the grid axis_x x axis_y."""
    W, sqrt_det = bandwidth(samples, bw_scale)
    n = np.asarray(samples).shape[0]
    return kernel_sums(samples, axis_x, axis_y, W) / (n * 2.0 * np.pi * sqrt_det)


def colour_limits(zi):
    """(vmin, vmax) as draw_kde hands them to pcolormesh (utils_sampling.py:111-112)."""
    return float(np.min(zi)), float(max(np.max(zi) * 0.2, np.min(zi)))


def landscape_loop(grid_region, ngrids=21):
    """synthetic/main.py:318-329, the loop as the reference writes it."""
    grid_batch = np.zeros((ngrids * ngrids, 2))
    step = 2 * grid_region / (ngrids - 1)
    for i in range(ngrids):
        for j in range(ngrids):
            grid_batch[i * ngrids + j, 0] = -grid_region + i * step
            grid_batch[i * ngrids + j, 1] = -grid_region + j * step
    return grid_batch


@functools.lru_cache(maxsize=None)
def pool(kind, n=10000, seed=0):
    """Seeded fp32 pools, read-only: "iso" (isotropic), "corr" (correlation 0.95), "modes9" (nine tight modes on a 3 x 3 lattice),
    "modes25" (the 25-Gaussians lattice at scale 1)."""
    rs = np.random.RandomState(1000 + seed)
    z = rs.randn(n, 2)
    if kind == "iso":
        x = 1.2 * z + np.array([0.3, -0.2])
    elif kind == "corr":
        x = z @ np.linalg.cholesky(np.array([[1.0, 0.95], [0.95, 1.0]])).T * 1.5
    elif kind == "modes9":
        side = np.array([-2.0, 0.0, 2.0])
        c = np.array([(a, b) for a in side for b in side])
        x = c[rs.randint(9, size=n)] + 0.05 * z
    elif kind == "modes25":
        side = np.linspace(-2.0, 2.0, 5)
        c = np.array([(a, b) for a in side for b in side])
        x = c[rs.randint(25, size=n)] + 0.05 * z
    else:
        raise KeyError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x
