// The Frechet distance between two pools from their moment states (metrics.PoolMoments), on the device and in double throughout:
//
//   fd = |dmu|^2 + Tr S_r + Tr S_f - 2 Tr (S_r^{1/2} S_f S_r^{1/2})^{1/2}
//
// The two matrix square roots are coupled Newton-Schulz iterations (three d x d products per step) on the float64 matrix instruction
// v_mfma_f64_16x16x4_f64; DESIGN.md section 25 states the algorithm and its stop rule, tests/frechet_cases.py restates it in numpy.
//
// 1. f64_matmul_kernel<Q>: C = alpha A B + diag I for row-major d x d doubles, B general.  A block of 256 threads owns a tile of
//    TM x TM results, TM = 32 Q; its four waves (2 x 2) own Q x Q accumulators of 16 x 16 each.  Q = 1 below d = 1024 (d = 512: 256
//    blocks, one per CU, where 64 x 64 tiles would leave three quarters of the CUs idle), Q = 2 from there on (operand reuse 2; 256
//    blocks at 1024, 1024 at 2048).  No K split: a result is one chain of MFMA accumulations in ascending k, there is nothing to fold and
//    no workspace.  The K loop walks 32 at a time through LDS; the next tile is loaded to registers under the current tile's MFMAs.
//    Loads are predicated: rows, columns and k past d contribute exact zeros and nothing outside the three matrices is touched.
//    f64 operand map (moments.hip; NOT the f32 map): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result
//    col = l & 15, row = (l >> 4) + 4 * reg.  LDS: the A tile is [row][k] with rows 34 doubles apart -- the 32 lanes a ds_read_b64
//    serves per cycle are 16 rows x 2 k, double index 34 row + k = 2 row + k (mod 32): 32 different bank pairs; the B tile is [k][col]
//    with rows TM + 16 doubles apart (= 16 mod 32: two k rows of 16 consecutive doubles, 32 banks apart, as in moments.hip).  Both tiles
//    are written 32 (A) or TM (B) consecutive doubles at a time.
//    blockIdx.z runs up to two independent products in one launch, and a device flag (`skip`) turns the launch into an early exit.
// 2. The iteration's small kernels: covariance from a state, row sums of squares (the Frobenius norm, two levels in a fixed order),
//    the decision kernel (one block: trace in a fixed order, then the stop rule), and the symmetrising commit through a 32 x 32 LDS
//    transpose.  No atomics anywhere: a rerun is bit-equal.  Every launch of a root's iteration is queued up front; once the decision
//    kernel has set the root's `done` flag the remaining ones return at once.
#include "cgs_internal.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define FR_MAX_D 2048
#define FR_MAX_ITERS 64
#define FR_KT 32                 // k per LDS tile
#define FR_A_ROW 34              // doubles between two rows of the A tile (see above)
#define FR_WIDE_D 1024           // from this d on: 64 x 64 tiles
#define FR_CTL_DOUBLES 32        // the control block in front of the workspace
#define FR_MATS 6                // Y, Z, T, Y', Z', S_f

struct FmmParams {
    const double *a0, *b0, *a1, *b1;
    double *c0, *c1;
    const int* skip;             // device flag or null: non-zero -> the launch does nothing
    int d;
    double alpha, diag;
};

template <int Q>
__global__ __launch_bounds__(256) void f64_matmul_kernel(FmmParams p) {
    constexpr int TM = 32 * Q, B_ROW = TM + 16, U = TM / 8, B_KS = 256 / TM;
    __shared__ double As[TM][FR_A_ROW];
    __shared__ double Bs[FR_KT][B_ROW];
    if (p.skip && *p.skip) return;                                   // (block-uniform)
    const double* __restrict__ A = blockIdx.z ? p.a1 : p.a0;
    const double* __restrict__ B = blockIdx.z ? p.b1 : p.b0;
    double* __restrict__ C = blockIdx.z ? p.c1 : p.c0;
    const int d = p.d, t = threadIdx.x;
    const int row0 = blockIdx.y * TM, col0 = blockIdx.x * TM;
    const int ak = t & 31, ar = t >> 5;                              // A loader: k ak of rows ar, ar + 8, ...
    const int bc = t % TM, bk = t / TM;                              // B loader: column bc of k rows bk, bk + B_KS, ...
    const bool okc = col0 + bc < d;

    double va[U], vb[U];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = row0 + ar + 8 * u, ka = k0 + ak, kb = k0 + bk + B_KS * u;
            va[u] = (r < d && ka < d) ? A[(size_t)r * d + ka] : 0.0;
            vb[u] = (okc && kb < d) ? B[(size_t)kb * d + col0 + bc] : 0.0;
        }
    };

    const int lane = t & 63, wv = t >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int lr = lane >> 4, lc = lane & 15;
    f64x4 acc[Q][Q];
#pragma unroll
    for (int a = 0; a < Q; ++a)
#pragma unroll
        for (int b = 0; b < Q; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    fetch(0);
    for (int k0 = 0; k0 < d; k0 += FR_KT) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            As[ar + 8 * u][ak] = va[u];
            Bs[bk + B_KS * u][bc] = vb[u];
        }
        __syncthreads();
        if (k0 + FR_KT < d) fetch(k0 + FR_KT);                       // (block-uniform) in flight under the products below
#pragma unroll
        for (int kk = 0; kk < FR_KT / 4; ++kk) {
            double av[Q], bv[Q];
#pragma unroll
            for (int a = 0; a < Q; ++a) av[a] = As[16 * (Q * wr + a) + lc][4 * kk + lr];
#pragma unroll
            for (int b = 0; b < Q; ++b) bv[b] = Bs[4 * kk + lr][16 * (Q * wc + b) + lc];
#pragma unroll
            for (int a = 0; a < Q; ++a)
#pragma unroll
                for (int b = 0; b < Q; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

#pragma unroll
    for (int a = 0; a < Q; ++a)
#pragma unroll
        for (int b = 0; b < Q; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {                            // f64 result map: row = (lane >> 4) + 4 * reg, col = lane & 15
                const int r = row0 + 16 * (Q * wr + a) + lr + 4 * e, c = col0 + 16 * (Q * wc + b) + lc;
                if (r < d && c < d) C[(size_t)r * d + c] = p.alpha * acc[a][b][e] + (r == c ? p.diag : 0.0);
            }
}

static int fmm_launch(const FmmParams& p, int count, hipStream_t s) {
    if (p.d >= FR_WIDE_D) {
        const int T = cgs_ceil_div(p.d, 64);
        hipLaunchKernelGGL(f64_matmul_kernel<2>, dim3(T, T, count), dim3(256), 0, s, p);
    } else {
        const int T = cgs_ceil_div(p.d, 32);
        hipLaunchKernelGGL(f64_matmul_kernel<1>, dim3(T, T, count), dim3(256), 0, s, p);
    }
    CGS_CHECK_LAUNCH("f64_matmul");
    return CGS_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the iteration
#pragma clang fp contract(off)   // the scalar kernels below round every operation separately, as the numpy restatement does

struct FrCtl {                   // per root r (0: of S_r, 1: of M'), written by one thread of one-block kernels only
    double nrm[2];               // |A|_F
    double t_prev[2], d_prev[2]; // the last kept trace and the last |difference of traces|
    double t_keep[2];            // Tr of the iterate that is kept
    double dmu2, tr_r, tr_f;
    int done[2], commit[2], iters[2], status[2];
};
static_assert(sizeof(FrCtl) <= FR_CTL_DOUBLES * sizeof(double), "control block");

// the sum of one value per thread of a 256-thread block, in a fixed tree order; every thread gets it
__device__ __forceinline__ double fr_block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// grid (d, 2): row blockIdx.x of cov = (gram - sum sum^T / n) / (n - ddof), symmetrised, of pool blockIdx.y
__global__ __launch_bounds__(256) void fr_cov_kernel(const double* __restrict__ sum_r, const double* __restrict__ gram_r, double n_r, double* __restrict__ out_r,
                                                     const double* __restrict__ sum_f, const double* __restrict__ gram_f, double n_f, double* __restrict__ out_f,
                                                     int d, double ddof) {
    const double* __restrict__ s = blockIdx.y ? sum_f : sum_r;
    const double* __restrict__ g = blockIdx.y ? gram_f : gram_r;
    double* __restrict__ out = blockIdx.y ? out_f : out_r;
    const double n = blockIdx.y ? n_f : n_r;
    const int i = blockIdx.x;
    const double si = s[i];
    for (int j = threadIdx.x; j < d; j += 256) {
        const double sj = s[j];
        const double cij = (g[(size_t)i * d + j] - si * sj / n) / (n - ddof);
        const double cji = (g[(size_t)j * d + i] - sj * si / n) / (n - ddof);
        out[(size_t)i * d + j] = 0.5 * (cij + cji);
    }
}

// grid (d): rowsq[i] = sum_j a[i][j]^2, ascending j per thread, then the tree
__global__ __launch_bounds__(256) void fr_rowsq_kernel(const double* __restrict__ a, double* __restrict__ rowsq, int d) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    double v = 0.0;
    for (int j = threadIdx.x; j < d; j += 256) {
        const double x = a[(size_t)i * d + j];
        v += x * x;
    }
    v = fr_block_sum(v, sh);
    if (threadIdx.x == 0) rowsq[i] = v;
}

// one block: the start of root r on the unscaled matrix a.  Root 0 also leaves |dmu|^2 and the two covariance traces.
__global__ __launch_bounds__(256) void fr_begin_kernel(FrCtl* __restrict__ ctl, int r, const double* __restrict__ a, const double* __restrict__ rowsq, int d,
                                                       const double* __restrict__ s_f, const double* __restrict__ sum_r, const float* __restrict__ shift_r,
                                                       double n_r, const double* __restrict__ sum_f, const float* __restrict__ shift_f, double n_f) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double v = 0.0;
    for (int i = t; i < d; i += 256) v += rowsq[i];
    const double nrm = sqrt(fr_block_sum(v, sh));
    const bool zero = !(nrm > 0.0);
    v = 0.0;
    if (!zero)
        for (int i = t; i < d; i += 256) v += a[(size_t)i * d + i] / nrm;
    const double t0 = fr_block_sum(v, sh);
    if (r == 0) {
        double tr = 0.0, tf = 0.0, m2 = 0.0;
        for (int i = t; i < d; i += 256) {
            tr += a[(size_t)i * d + i];
            tf += s_f[(size_t)i * d + i];
            const double cr = shift_r ? (double)shift_r[i] : 0.0, cf = shift_f ? (double)shift_f[i] : 0.0;
            const double dm = (cr - cf) + sum_r[i] / n_r - sum_f[i] / n_f;
            m2 += dm * dm;
        }
        tr = fr_block_sum(tr, sh);
        tf = fr_block_sum(tf, sh);
        m2 = fr_block_sum(m2, sh);
        if (t == 0) { ctl->tr_r = tr; ctl->tr_f = tf; ctl->dmu2 = m2; }
    }
    if (t == 0) {
        ctl->nrm[r] = zero ? 0.0 : nrm;
        ctl->t_prev[r] = t0;
        ctl->d_prev[r] = __builtin_inf();
        ctl->t_keep[r] = t0;
        ctl->done[r] = zero ? 1 : 0;                                  // an exactly zero matrix: its root is zero, no iteration
        ctl->commit[r] = 0;
        ctl->iters[r] = 0;
        ctl->status[r] = 0;
    }
}

// y = y / nrm (zero for a zero matrix), z = I
__global__ __launch_bounds__(256) void fr_scale_kernel(const FrCtl* __restrict__ ctl, int r, double* __restrict__ y, double* __restrict__ z, int d) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)d * d) return;
    const double nrm = ctl->nrm[r];
    y[e] = nrm > 0.0 ? y[e] / nrm : 0.0;
    z[e] = (e / d == e % d) ? 1.0 : 0.0;
}

// one block: the stop rule of step k on the candidate yn (tests/frechet_cases.py, newton_schulz_root)
__global__ __launch_bounds__(256) void fr_decide_kernel(FrCtl* __restrict__ ctl, int r, const double* __restrict__ yn, int d, int k, int max_iters, double tol) {
    __shared__ double sh[256];
    if (ctl->done[r]) {                                              // (block-uniform)
        if (threadIdx.x == 0) ctl->commit[r] = 0;
        return;
    }
    double v = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) v += yn[(size_t)i * d + i];
    const double tr = fr_block_sum(v, sh);
    if (threadIdx.x != 0) return;
    const double dl = fabs(tr - ctl->t_prev[r]);
    if (!isfinite(tr)) {
        ctl->done[r] = 1; ctl->commit[r] = 0; ctl->status[r] = 1; ctl->iters[r] = k;
    } else if (dl <= tol * tr) {
        ctl->done[r] = 1; ctl->commit[r] = 1; ctl->status[r] = 0; ctl->iters[r] = k; ctl->t_keep[r] = tr;
    } else if (k >= 5 && dl >= ctl->d_prev[r] && dl < 1e-6 * tr) {
        ctl->done[r] = 1; ctl->commit[r] = 0; ctl->status[r] = 1; ctl->iters[r] = k;
    } else {
        ctl->commit[r] = 1; ctl->t_prev[r] = tr; ctl->d_prev[r] = dl; ctl->t_keep[r] = tr;
        if (k == max_iters) { ctl->done[r] = 1; ctl->status[r] = 2; ctl->iters[r] = k; }
    }
}

// grid (ceil(d / 32), ceil(d / 32), count): dst = (src + src^T) / 2 tile by tile; gate (device flag or null): zero -> nothing is written
__global__ __launch_bounds__(256) void fr_sym_kernel(const int* __restrict__ gate, const double* __restrict__ s0, double* __restrict__ d0,
                                                     const double* __restrict__ s1, double* __restrict__ d1, int d) {
    __shared__ double sa[32][33], sb[32][33];
    if (gate && !*gate) return;                                      // (block-uniform)
    const double* __restrict__ src = blockIdx.z ? s1 : s0;
    double* __restrict__ dst = blockIdx.z ? d1 : d0;
    const int c = threadIdx.x & 31, rq = threadIdx.x >> 5;
    const int I = blockIdx.y * 32, J = blockIdx.x * 32;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = rq + 8 * u;
        sa[r][c] = (I + r < d && J + c < d) ? src[(size_t)(I + r) * d + J + c] : 0.0;
        sb[r][c] = (J + r < d && I + c < d) ? src[(size_t)(J + r) * d + I + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = rq + 8 * u;
        if (I + r < d && J + c < d) dst[(size_t)(I + r) * d + J + c] = 0.5 * (sa[r][c] + sb[c][r]);
    }
}

__global__ void fr_finish_kernel(const FrCtl* __restrict__ ctl, double* __restrict__ out) {
    const double tr_root = sqrt(ctl->nrm[0]) * sqrt(ctl->nrm[1]) * ctl->t_keep[1];
    out[0] = ctl->dmu2 + ctl->tr_r + ctl->tr_f - 2.0 * tr_root;
    out[1] = ctl->dmu2;
    out[2] = ctl->tr_r;
    out[3] = ctl->tr_f;
    out[4] = tr_root;
    out[5] = (double)ctl->iters[0];
    out[6] = (double)ctl->iters[1];
    out[7] = (double)(ctl->status[0] > ctl->status[1] ? ctl->status[0] : ctl->status[1]);
}

static size_t fr_ws_doubles(int d) { return (size_t)FR_CTL_DOUBLES + (size_t)d + (size_t)FR_MATS * d * d; }

#define FR_LAUNCH(...)                          \
    do {                                        \
        hipLaunchKernelGGL(__VA_ARGS__);        \
        CGS_CHECK_LAUNCH("frechet_from_moments"); \
    } while (0)

// the queued launches of root r: Y holds the unscaled matrix and rowsq its row sums of squares
static int fr_root(FrCtl* ctl, int r, double* Y, double* Z, double* T, double* Yn, double* Zn, const double* rowsq, const double* S_f, const double* sum_r,
                   const float* shift_r, double n_r, const double* sum_f, const float* shift_f, double n_f, int d, int max_iters, hipStream_t s) {
    const int T32 = cgs_ceil_div(d, 32);
    const double tol = d * 0x1p-52 > 1e-15 ? d * 0x1p-52 : 1e-15;
    FR_LAUNCH(fr_begin_kernel, dim3(1), dim3(256), 0, s, ctl, r, Y, rowsq, d, S_f, sum_r, shift_r, n_r, sum_f, shift_f, n_f);
    FR_LAUNCH(fr_scale_kernel, dim3((unsigned)(((size_t)d * d + 255) / 256)), dim3(256), 0, s, ctl, r, Y, Z, d);
    FmmParams p;
    p.skip = &ctl->done[r]; p.d = d;
    for (int k = 1; k <= max_iters; ++k) {
        p.a0 = Z; p.b0 = Y; p.c0 = T; p.a1 = p.b1 = nullptr; p.c1 = nullptr; p.alpha = -0.5; p.diag = 1.5;       // T = 1.5 I - 0.5 Z Y
        int rc = fmm_launch(p, 1, s);
        if (rc != CGS_OK) return rc;
        p.a0 = Y; p.b0 = T; p.c0 = Yn; p.a1 = T; p.b1 = Z; p.c1 = Zn; p.alpha = 1.0; p.diag = 0.0;               // Y' = Y T, Z' = T Z
        rc = fmm_launch(p, 2, s);
        if (rc != CGS_OK) return rc;
        FR_LAUNCH(fr_decide_kernel, dim3(1), dim3(256), 0, s, ctl, r, Yn, d, k, max_iters, tol);
        FR_LAUNCH(fr_sym_kernel, dim3(T32, T32, 2), dim3(256), 0, s, &ctl->commit[r], Yn, Y, Zn, Z, d);
    }
    return CGS_OK;
}

extern "C" {

int cgs_f64_matmul(const double* a, const double* b, double* c, int d, double alpha, double diag, void* stream) {
    if (d < 1 || d > FR_MAX_D) return cgs_set_error(CGS_EINVAL, "f64_matmul: needs 1 <= d <= %d (d=%d)", FR_MAX_D, d);
    if (!a || !b || !c || c == a || c == b) return cgs_set_error(CGS_EINVAL, "f64_matmul: null a / b / c, or c aliases an operand");
    FmmParams p;
    p.a0 = a; p.b0 = b; p.c0 = c; p.a1 = p.b1 = nullptr; p.c1 = nullptr; p.skip = nullptr; p.d = d; p.alpha = alpha; p.diag = diag;
    return fmm_launch(p, 1, (hipStream_t)stream);
}

size_t cgs_frechet_ws_bytes(int d) {
    if (d < 1 || d > FR_MAX_D) return 0;
    return fr_ws_doubles(d) * sizeof(double);
}

int cgs_frechet_from_moments(const double* sum_r, const double* gram_r, const float* shift_r, long long n_r, const double* sum_f, const double* gram_f,
                             const float* shift_f, long long n_f, int d, int ddof, int max_iters, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (d < 1 || d > FR_MAX_D) return cgs_set_error(CGS_EINVAL, "frechet_from_moments: needs 1 <= d <= %d (d=%d)", FR_MAX_D, d);
    if (max_iters < 1 || max_iters > FR_MAX_ITERS)
        return cgs_set_error(CGS_EINVAL, "frechet_from_moments: needs 1 <= max_iters <= %d (max_iters=%d)", FR_MAX_ITERS, max_iters);
    if (n_r - ddof <= 0 || n_f - ddof <= 0 || n_r <= 0 || n_f <= 0)
        return cgs_set_error(CGS_EINVAL, "frechet_from_moments: needs n > 0 and n - ddof > 0 (n_r=%lld n_f=%lld ddof=%d)", n_r, n_f, ddof);
    if (!sum_r || !gram_r || !sum_f || !gram_f || !out) return cgs_set_error(CGS_EINVAL, "frechet_from_moments: null sum / gram / out");
    const size_t need = fr_ws_doubles(d) * sizeof(double);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "frechet_from_moments: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 7) return cgs_set_error(CGS_EINVAL, "frechet_from_moments: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t dd = (size_t)d * d;
    FrCtl* ctl = (FrCtl*)ws;
    double* rowsq = (double*)ws + FR_CTL_DOUBLES;
    double *Y = rowsq + d, *Z = Y + dd, *T = Z + dd, *Yn = T + dd, *Zn = Yn + dd, *S_f = Zn + dd;
    const double nr = (double)n_r, nf = (double)n_f;
    const int T32 = cgs_ceil_div(d, 32);

    FR_LAUNCH(fr_cov_kernel, dim3(d, 2), dim3(256), 0, s, sum_r, gram_r, nr, Y, sum_f, gram_f, nf, S_f, d, (double)ddof);
    FR_LAUNCH(fr_rowsq_kernel, dim3(d), dim3(256), 0, s, Y, rowsq, d);
    int rc = fr_root(ctl, 0, Y, Z, T, Yn, Zn, rowsq, S_f, sum_r, shift_r, nr, sum_f, shift_f, nf, d, max_iters, s);
    if (rc != CGS_OK) return rc;
    FmmParams p;                                                      // M' = sym(R' (S_f R')), R' = Y
    p.skip = nullptr; p.d = d; p.alpha = 1.0; p.diag = 0.0; p.a1 = p.b1 = nullptr; p.c1 = nullptr;
    p.a0 = S_f; p.b0 = Y; p.c0 = T;
    if ((rc = fmm_launch(p, 1, s)) != CGS_OK) return rc;
    p.a0 = Y; p.b0 = T; p.c0 = Yn;
    if ((rc = fmm_launch(p, 1, s)) != CGS_OK) return rc;
    FR_LAUNCH(fr_sym_kernel, dim3(T32, T32, 1), dim3(256), 0, s, (const int*)nullptr, Yn, Y, (const double*)nullptr, (double*)nullptr, d);
    FR_LAUNCH(fr_rowsq_kernel, dim3(d), dim3(256), 0, s, Y, rowsq, d);
    rc = fr_root(ctl, 1, Y, Z, T, Yn, Zn, rowsq, S_f, sum_r, shift_r, nr, sum_f, shift_f, nf, d, max_iters, s);
    if (rc != CGS_OK) return rc;
    FR_LAUNCH(fr_finish_kernel, dim3(1), dim3(1), 0, s, ctl, out);
    return CGS_OK;
}

}  // extern "C"
