// Additive pool statistics behind the log rows' diagnostic columns, in double on the device (metrics.CalibrationStats / ModeStats):
//
//   calibration (sampling/utils_sampling.py:186-299 of the reference): per slot of np.digitize(double(p), edges) - 1 the count, sum p and
//   sum y; n, sum (y - p), sum p (1 - p), sum (y - p)^2, the scores below the first edge; per label n_y, sum p, max p.
//   2-D modes (utils_sampling.py:132-161): per mode the samples closer than thres, n, the samples whose NEAREST mode is closer than
//   thres, sum of the distance to the nearest mode.
//
// Both are reductions over 10^3 .. 10^6 elements: launch- and latency-bound.  The form is the same for both:
// 1. *_partial_kernel, one WAVE per block, a grid over contiguous chunks of the input (diag_plan: 512 elements per block, longer chunks
//    past 1024 blocks).  A lane walks elements lane, lane + 64, ... of its chunk in ascending order and keeps its own double sums --
//    the per-slot sums in its own column of an LDS table [rows][64], so no two lanes ever add to the same word.  The 64 columns of
//    every row are then folded by a halving tree (32, 16, ... 1), an order fixed by the lane index alone.  Counts are integers:
//    calibration counts its slots with LDS integer atomics, the mode kernel with one ballot per mode (lane j keeps mode j's count).
//    The block leaves ONE row in the state's layout in the workspace.
// 2. diag_fold_kernel, one block: entry j of the rows is added in ascending block order and then to state[j] (the two maxima: max).
// No floating-point atomics anywhere, so a rerun from the same start is bit-equal.  Every summed term is a double expression of
// exactly converted fp32 inputs; floating-point contraction is OFF in this file: a fused dx * dx + dy * dy differs in the last bit from
// numpy's two products and one sum, and with it a `dist < thres` decision.
#include "cgs_internal.h"

#pragma clang fp contract(off)

#define DIAG_LANES 64
#define DIAG_PER_BLOCK 512       // elements per block aimed at (8 per lane)
#define DIAG_MAX_BLOCKS 1024
#define DIAG_MAX_N 0x40000000L
#define CAL_MAX_BINS 64
#define MODE_MAX_K 64
#define CAL_EXTRA 5              // table rows past the slots: sum (y - p), sum p (1 - p), sum (y - p)^2, sum p, max p

struct DiagPlan {
    int chunk, blocks;
};

static bool diag_plan(DiagPlan& p, long n) {
    if (n < 0 || n > DIAG_MAX_N) return false;
    if (n == 0) { p.chunk = DIAG_LANES; p.blocks = 0; return true; }
    long blocks = (n + DIAG_PER_BLOCK - 1) / DIAG_PER_BLOCK;
    if (blocks > DIAG_MAX_BLOCKS) blocks = DIAG_MAX_BLOCKS;
    const long per = (n + blocks - 1) / blocks;
    const long chunk = (per + DIAG_LANES - 1) / DIAG_LANES * DIAG_LANES;
    p.chunk = (int)chunk;
    p.blocks = (int)((n + chunk - 1) / chunk);
    return true;
}

// rows [0, rows) of tab[.][64]: column 0 ends as the fold of the 64 columns by halving; row `max_row` folds with max instead of +
__device__ __forceinline__ void diag_fold_columns(double* tab, int rows, int max_row, int lane) {
    for (int stride = DIAG_LANES / 2; stride >= 1; stride >>= 1) {
        __syncthreads();
        for (int idx = lane; idx < rows * stride; idx += DIAG_LANES) {
            const int r = idx / stride, c = idx - r * stride;
            const double a = tab[r * DIAG_LANES + c], b = tab[r * DIAG_LANES + c + stride];
            tab[r * DIAG_LANES + c] = r == max_row ? (b > a ? b : a) : a + b;
        }
    }
    __syncthreads();
}

// state / row layout, S = n_bins + 1 slots:  [0, S) count | [S, 2S) sum p | [2S, 3S) sum y | 3S: n, sum (y - p), sum p (1 - p), sum (y - p)^2,
// under | 3S + 5 + 3 y: n_y, sum p, max p of label y
__global__ __launch_bounds__(DIAG_LANES) void calibration_partial_kernel(const float* __restrict__ p, int n, int label, const double* __restrict__ edges,
                                                                         int n_bins, int chunk, double* __restrict__ rows) {
    __shared__ double tab[(CAL_MAX_BINS + 1 + CAL_EXTRA) * DIAG_LANES];
    __shared__ double edge[CAL_MAX_BINS + 1];
    __shared__ unsigned cnt[CAL_MAX_BINS + 2];                      // the slots, then `under`
    const int lane = threadIdx.x;
    const int S = n_bins + 1, T = S + CAL_EXTRA;
    for (int r = 0; r < T; ++r) tab[r * DIAG_LANES + lane] = 0.0;   // (a lane's own column: no barrier needed before it adds to it)
    for (int j = lane; j < S; j += DIAG_LANES) edge[j] = edges[j];
    for (int j = lane; j < S + 1; j += DIAG_LANES) cnt[j] = 0u;
    __syncthreads();
    const int c0 = blockIdx.x * chunk;
    const int c1 = c0 + chunk < n ? c0 + chunk : n;
    const double y = (double)label;
    double s_ymp = 0.0, s_var = 0.0, s_sq = 0.0, s_p = 0.0, mx = 0.0;
    for (int i = c0 + lane; i < c1; i += DIAG_LANES) {
        const double v = (double)p[i];
        int lo = 0, hi = S;                                         // edges <= v, compared in double (np.digitize, right = False)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (edge[mid] <= v) lo = mid + 1; else hi = mid;
        }
        const int slot = v != v ? n_bins : lo - 1;                  // NaN sorts past every edge
        if (slot < 0) { atomicAdd(&cnt[S], 1u); continue; }         // below the first edge: counted, nothing else
        atomicAdd(&cnt[slot], 1u);
        tab[slot * DIAG_LANES + lane] += v;
        const double d = y - v, q = 1.0 - v;
        s_ymp += d;
        s_var += v * q;
        s_sq += d * d;
        s_p += v;
        mx = v > mx ? v : mx;                                       // (a NaN never wins)
    }
    tab[(S + 0) * DIAG_LANES + lane] = s_ymp;
    tab[(S + 1) * DIAG_LANES + lane] = s_var;
    tab[(S + 2) * DIAG_LANES + lane] = s_sq;
    tab[(S + 3) * DIAG_LANES + lane] = s_p;
    tab[(S + 4) * DIAG_LANES + lane] = mx;
    diag_fold_columns(tab, T, S + 4, lane);
    double* row = rows + (size_t)blockIdx.x * (3 * S + 11);
    unsigned total = 0;
    for (int j = 0; j < S; ++j) total += cnt[j];
    for (int j = lane; j < S; j += DIAG_LANES) {
        row[j] = (double)cnt[j];
        row[S + j] = tab[j * DIAG_LANES];
        row[2 * S + j] = y * (double)cnt[j];
    }
    if (lane == 0) {
        double* g = row + 3 * S;
        g[0] = (double)total;
        g[1] = tab[(S + 0) * DIAG_LANES];
        g[2] = tab[(S + 1) * DIAG_LANES];
        g[3] = tab[(S + 2) * DIAG_LANES];
        g[4] = (double)cnt[S];
        for (int l = 0; l < 2; ++l) {                               // the other label's triple: zeros the fold never reads
            const bool mine = l == label;
            g[5 + 3 * l] = mine ? (double)total : 0.0;
            g[6 + 3 * l] = mine ? tab[(S + 3) * DIAG_LANES] : 0.0;
            g[7 + 3 * l] = mine ? tab[(S + 4) * DIAG_LANES] : 0.0;
        }
    }
}

// state / row layout:  [0, k) count per mode | k: n, good, sum of min_j dist_j
__global__ __launch_bounds__(DIAG_LANES) void mode_partial_kernel(const float* __restrict__ x, int n, const double* __restrict__ cent, int k, double thres,
                                                                  int chunk, double* __restrict__ rows) {
    __shared__ double tab[DIAG_LANES];
    __shared__ double c[2 * MODE_MAX_K];
    const int lane = threadIdx.x;
    for (int j = lane; j < 2 * k; j += DIAG_LANES) c[j] = cent[j];
    __syncthreads();
    const int c0 = blockIdx.x * chunk;
    const int c1 = c0 + chunk < n ? c0 + chunk : n;
    unsigned mine = 0, good = 0;                                    // lane j: hits of mode j; every lane: the same count of good samples
    double s_min = 0.0;
    for (int base = c0; base < c1; base += DIAG_LANES) {            // (wave-uniform trip count: the ballots below see every lane)
        const int i = base + lane;
        const bool in = i < c1;
        const double x0 = in ? (double)x[2 * (size_t)i] : 0.0, x1 = in ? (double)x[2 * (size_t)i + 1] : 0.0;
        double m = 0.0;
        for (int j = 0; j < k; ++j) {
            const double dx = x0 - c[2 * j], dy = x1 - c[2 * j + 1];
            const double xx = dx * dx, yy = dy * dy;
            const double dist = sqrt(xx + yy);
            const unsigned long long hit = __ballot(in && dist < thres);
            if (lane == j) mine += (unsigned)__popcll(hit);
            if (j == 0 || dist < m || dist != dist) m = dist;       // np.min: a NaN stays
        }
        good += (unsigned)__popcll(__ballot(in && m < thres));
        if (in) s_min += m;
    }
    tab[lane] = s_min;
    diag_fold_columns(tab, 1, -1, lane);
    double* row = rows + (size_t)blockIdx.x * (k + 3);
    if (lane < k) row[lane] = (double)mine;
    if (lane == 0) {
        row[k] = (double)(c1 - c0);
        row[k + 1] = (double)good;
        row[k + 2] = tab[0];
    }
}

// state[j] (+)= rows[0][j] + rows[1][j] + ..., ascending; entries max_a / max_b take the max, entries in [skip0, skip1) are left alone
__global__ __launch_bounds__(256) void diag_fold_kernel(const double* __restrict__ rows, int blocks, int R, double* __restrict__ state, int max_a, int max_b,
                                                        int skip0, int skip1) {
    for (int j = threadIdx.x; j < R; j += 256) {
        if (j >= skip0 && j < skip1) continue;
        const bool is_max = j == max_a || j == max_b;
        double v = rows[j];
        for (int b = 1; b < blocks; ++b) {
            const double w = rows[(size_t)b * R + j];
            v = is_max ? (w > v ? w : v) : v + w;
        }
        const double s = state[j];
        state[j] = is_max ? (v > s ? v : s) : s + v;
    }
}

extern "C" {

size_t cgs_calibration_ws_bytes(int n, int n_bins) {
    DiagPlan p;
    if (n_bins < 1 || n_bins > CAL_MAX_BINS || !diag_plan(p, n)) return 0;
    return (size_t)p.blocks * (3 * (n_bins + 1) + 11) * sizeof(double);
}

int cgs_calibration_accumulate(const float* p, int n, int label, const double* edges, int n_bins, double* state, void* ws, size_t ws_bytes,
                               void* stream) {
    DiagPlan pl;
    if (n_bins < 1 || n_bins > CAL_MAX_BINS || (label != 0 && label != 1) || !diag_plan(pl, n))
        return cgs_set_error(CGS_EINVAL, "calibration_accumulate: needs 1 <= n_bins <= %d, label 0 or 1, 0 <= n <= 2^30 (n=%d n_bins=%d label=%d)",
                             CAL_MAX_BINS, n, n_bins, label);
    if (n == 0) return CGS_OK;
    if (!p || !edges || !state) return cgs_set_error(CGS_EINVAL, "calibration_accumulate: null p / edges / state");
    const int S = n_bins + 1, R = 3 * S + 11;
    const size_t need = (size_t)pl.blocks * R * sizeof(double);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "calibration_accumulate: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 7) return cgs_set_error(CGS_EINVAL, "calibration_accumulate: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(calibration_partial_kernel, dim3(pl.blocks), dim3(DIAG_LANES), 0, s, p, n, label, edges, n_bins, pl.chunk, (double*)ws);
    CGS_CHECK_LAUNCH("calibration_accumulate");
    const int other = 3 * S + 5 + 3 * (1 - label);                  // the other label's triple keeps its contents
    hipLaunchKernelGGL(diag_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, pl.blocks, R, state, 3 * S + 7 + 3 * label, -1, other, other + 3);
    CGS_CHECK_LAUNCH("calibration_accumulate");
    return CGS_OK;
}

size_t cgs_mode_stats_ws_bytes(int n, int k) {
    DiagPlan p;
    if (k < 1 || k > MODE_MAX_K || !diag_plan(p, n)) return 0;
    return (size_t)p.blocks * (k + 3) * sizeof(double);
}

int cgs_mode_stats_accumulate(const float* x, int n, const double* centeroids, int k, double thres, double* state, void* ws, size_t ws_bytes,
                              void* stream) {
    DiagPlan pl;
    if (k < 1 || k > MODE_MAX_K || !diag_plan(pl, n))
        return cgs_set_error(CGS_EINVAL, "mode_stats_accumulate: needs 1 <= k <= %d, 0 <= n <= 2^30 (n=%d k=%d)", MODE_MAX_K, n, k);
    if (n == 0) return CGS_OK;
    if (!x || !centeroids || !state) return cgs_set_error(CGS_EINVAL, "mode_stats_accumulate: null x / centeroids / state");
    const int R = k + 3;
    const size_t need = (size_t)pl.blocks * R * sizeof(double);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "mode_stats_accumulate: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 7) return cgs_set_error(CGS_EINVAL, "mode_stats_accumulate: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mode_partial_kernel, dim3(pl.blocks), dim3(DIAG_LANES), 0, s, x, n, centeroids, k, thres, pl.chunk, (double*)ws);
    CGS_CHECK_LAUNCH("mode_stats_accumulate");
    hipLaunchKernelGGL(diag_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, pl.blocks, R, state, -1, -1, -1, -1);
    CGS_CHECK_LAUNCH("mode_stats_accumulate");
    return CGS_OK;
}

}  // extern "C"
