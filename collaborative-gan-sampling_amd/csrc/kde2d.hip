// The density map of a 2-D sample pool on a grid, additive, in double on the device (metrics.DensityMap): the
// arithmetic behind the reference's draw_kde (sampling/utils_sampling.py:97-112) without the drawing.
//
//   state[i * gy + j] += sum_k exp(-1/2 |W (g_ij - x_k)|^2)        g_ij = (axis_x[i], axis_y[j]),  W = [[w00, 0], [w10, w11]]
//   state[gx * gy]    += n
//
// un-normalised: whoever reads the state divides by n 2 pi sqrt(det C), C = (W^T W)^-1.  n * gx * gy Gaussian evaluations, the form:
// 1. kde2d_partial_kernel, grid (cell tiles, sample slices), 256 threads.  A thread owns KDE_CELLS = 4 cells (cell tile + t + 256 k: the
//    final stores are coalesced) with their fp32 coordinates in registers and one fp32 accumulator each -- four independent chains
//    through v_exp_f32.  The block walks its slice of the samples in runs of KDE_RUN = 128, staged through LDS (double-buffered: one
//    barrier per run); every lane reads the SAME sample, an LDS broadcast.  Per (cell, sample): subtract first, then whiten,
//        dx = gx - x0, dy = gy - x1;  u = w00 dx, v = w10 dx + w11 dy;  acc += exp2(-(u u + v v))
//    with W scaled by sqrt(1/2 log2 e) once per block, in double, before it is rounded to fp32: the exponent needs no further multiply.
//    (Whitening sample and grid point separately and subtracting after would round twice at whitened magnitudes of 40..400.)  An fp32
//    accumulator lives for ONE run; it is then added into the cell's double accumulator.  The block leaves one double per cell in
//    ws[slice][cell].
// 2. kde2d_fold_kernel: per cell the slices are added in ascending order and then onto state[cell]; one thread adds n.
// No floating-point atomics, so two calls with the same inputs from the same state end bit-equal.  v_exp_f32 of an argument below -126
// gives 0 (it flushes denormal results), of -inf gives 0; a NaN can only come from a non-finite sample, axis or W (or from
// w10 dx + w11 dy overflowing in both terms, |W d| ~ 1e38).
#include "cgs_internal.h"

#define KDE_THREADS 256
#define KDE_CELLS 4                              // cells per thread
#define KDE_TILE (KDE_THREADS * KDE_CELLS)       // cells per block
#define KDE_RUN 128                              // samples per staged run = the life of an fp32 accumulator (2 floats per sample: one per thread)
#define KDE_MIN_SLICE 64                         // a slice is a whole number of these (but for the last): a 64-sample batch is one slice
#define KDE_TARGET_BLOCKS 512                    // tiles x slices aimed at: two blocks per CU
#define KDE_MAX_CELLS (1L << 20)
#define KDE_MAX_N 0x40000000L
#define KDE_EXP_SCALE 0.84932180028801904        // sqrt(1/2 log2 e) = 1 / sqrt(2 ln 2)

struct KdePlan {
    int cells, tiles, slice, slices;
};

// The slicing depends on (n, gx gy) alone.
static bool kde_plan(KdePlan& p, long n, long gx, long gy) {
    if (gx < 1 || gy < 1 || gx > KDE_MAX_CELLS || gy > KDE_MAX_CELLS || gx * gy > KDE_MAX_CELLS || n < 0 || n > KDE_MAX_N) return false;
    p.cells = (int)(gx * gy);
    p.tiles = (p.cells + KDE_TILE - 1) / KDE_TILE;
    if (n == 0) { p.slice = KDE_MIN_SLICE; p.slices = 0; return true; }
    long want = (KDE_TARGET_BLOCKS + p.tiles - 1) / p.tiles;
    const long by_n = n / KDE_MIN_SLICE > 1 ? n / KDE_MIN_SLICE : 1;
    if (want > by_n) want = by_n;
    const long per = (n + want - 1) / want;
    const long slice = (per + KDE_MIN_SLICE - 1) / KDE_MIN_SLICE * KDE_MIN_SLICE;
    p.slice = (int)slice;
    p.slices = (int)((n + slice - 1) / slice);
    return true;
}

__global__ __launch_bounds__(KDE_THREADS) void kde2d_partial_kernel(const float* __restrict__ x, int n, const float* __restrict__ axis_x,
                                                                    const float* __restrict__ axis_y, int gy, int cells,
                                                                    const double* __restrict__ whiten, int slice, double* __restrict__ ws) {
    __shared__ __align__(8) float sm[2][2 * KDE_RUN];
    const int t = threadIdx.x;
    const float w00 = (float)(whiten[0] * KDE_EXP_SCALE), w10 = (float)(whiten[1] * KDE_EXP_SCALE), w11 = (float)(whiten[2] * KDE_EXP_SCALE);
    float cx[KDE_CELLS], cy[KDE_CELLS];
    double sum[KDE_CELLS];
    const int c0 = blockIdx.x * KDE_TILE + t;
#pragma unroll
    for (int k = 0; k < KDE_CELLS; ++k) {
        const int c = c0 + k * KDE_THREADS;
        const int i = c < cells ? c / gy : 0, j = c < cells ? c - i * gy : 0;      // (a cell past the grid computes on cell 0 and stores nothing)
        cx[k] = axis_x[i];
        cy[k] = axis_y[j];
        sum[k] = 0.0;
    }
    const long s0 = (long)blockIdx.y * slice;
    const long s1 = s0 + slice < n ? s0 + slice : n;
    const int runs = (int)((s1 - s0 + KDE_RUN - 1) / KDE_RUN);
    {
        const long f = 2 * s0 + t;
        sm[0][t] = f < 2 * s1 ? x[f] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < runs; ++r) {
        const long base = s0 + (long)r * KDE_RUN;
        if (r + 1 < runs) {                                                        // the other buffer: last read before the barrier that ended run r - 1
            const long f = 2 * (base + KDE_RUN) + t;
            sm[(r + 1) & 1][t] = f < 2 * s1 ? x[f] : 0.f;
        }
        const int cnt = s1 - base < KDE_RUN ? (int)(s1 - base) : KDE_RUN;
        const float2* sp = reinterpret_cast<const float2*>(sm[r & 1]);
        float acc[KDE_CELLS];
#pragma unroll
        for (int k = 0; k < KDE_CELLS; ++k) acc[k] = 0.f;
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float2 s = sp[j];
#pragma unroll
            for (int k = 0; k < KDE_CELLS; ++k) {
                const float dx = cx[k] - s.x, dy = cy[k] - s.y;
                const float u = w00 * dx, v = fmaf(w10, dx, w11 * dy);
                acc[k] += __builtin_amdgcn_exp2f(-fmaf(u, u, v * v));
            }
        }
#pragma unroll
        for (int k = 0; k < KDE_CELLS; ++k) sum[k] += (double)acc[k];
        __syncthreads();
    }
    double* row = ws + (size_t)blockIdx.y * cells;
#pragma unroll
    for (int k = 0; k < KDE_CELLS; ++k) {
        const int c = c0 + k * KDE_THREADS;
        if (c < cells) row[c] = sum[k];
    }
}

// state[c] += ws[0][c] + ws[1][c] + ..., ascending; state[cells] += n
__global__ __launch_bounds__(KDE_THREADS) void kde2d_fold_kernel(const double* __restrict__ ws, int slices, int cells, int n, double* __restrict__ state) {
    const int c = blockIdx.x * KDE_THREADS + threadIdx.x;
    if (c < cells) {
        double v = ws[c];
        for (int s = 1; s < slices; ++s) v += ws[(size_t)s * cells + c];
        state[c] += v;
    }
    if (c == 0) state[cells] += (double)n;
}

extern "C" {

size_t cgs_kde2d_ws_bytes(int n, int gx, int gy) {
    KdePlan p;
    if (!kde_plan(p, n, gx, gy)) return 0;
    return (size_t)p.slices * p.cells * sizeof(double);
}

int cgs_kde2d_accumulate(const float* x, int n, const float* axis_x, int gx, const float* axis_y, int gy, const double* whiten, double* state,
                         void* ws, size_t ws_bytes, void* stream) {
    KdePlan p;
    if (!kde_plan(p, n, gx, gy))
        return cgs_set_error(CGS_EINVAL, "kde2d_accumulate: needs 1 <= gx, gy, gx * gy <= 2^20, 0 <= n <= 2^30 (n=%d gx=%d gy=%d)", n, gx, gy);
    if (n == 0) return CGS_OK;
    if (!x || !axis_x || !axis_y || !whiten || !state) return cgs_set_error(CGS_EINVAL, "kde2d_accumulate: null x / axis_x / axis_y / whiten / state");
    const size_t need = (size_t)p.slices * p.cells * sizeof(double);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "kde2d_accumulate: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 7) return cgs_set_error(CGS_EINVAL, "kde2d_accumulate: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kde2d_partial_kernel, dim3(p.tiles, p.slices), dim3(KDE_THREADS), 0, s, x, n, axis_x, axis_y, gy, p.cells, whiten, p.slice,
                       (double*)ws);
    CGS_CHECK_LAUNCH("kde2d_accumulate");
    hipLaunchKernelGGL(kde2d_fold_kernel, dim3(cgs_ceil_div(p.cells, KDE_THREADS)), dim3(KDE_THREADS), 0, s, (const double*)ws, p.slices, p.cells, n, state);
    CGS_CHECK_LAUNCH("kde2d_accumulate");
    return CGS_OK;
}

}  // extern "C"
