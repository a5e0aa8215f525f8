// Discriminator rejection sampling on the device (sampling.DeviceRejector): the accept decision of the reference's
// Rejector (sampling/rejector.py:16-34) per logical batch, and the stable compaction of the accepted rows into a pool.
//
//   decide, per group g of b scores, as if rejector.sampling had been called once per batch, in order:
//     d     = logit(clip(double(s), 1e-14, 1 - 1e-14))                   logit as scipy.special computes it: log(x / (1 - x)) outside
//                                                                        [0.3, 0.65], log1p(t) - log1p(-t), t = 2 (x - 0.5), inside
//     M_g   = max(M_{g-1}, max_i d_i)                                    M_{-1} = the state; the state leaves as M_{groups-1}
//     F     = (d - M_g) - log(1 - exp((d - M_g) - eps))                  1 - exp(x), NOT -expm1(x): parity with the reference
//     gamma = percentile(F over the group, q)                            numpy's linear method: v = (b - 1) (q / 100), the order
//                                                                        statistics lo = F_(floor v), hi = F_(floor v + 1), t = v - floor v,
//                                                                        lo + (hi - lo) t for t < 0.5, hi - (hi - lo)(1 - t) otherwise
//     P     = 1 / (1 + exp(-(F - gamma)))      mask = u < P      counts[g] = sum mask
//
// Two launches.  1. drs_logit_kernel, one block per group: d of every row into the workspace, the group's max d beside it; block 0 copies
// the state in, so that launch 2 may overwrite it.  2. drs_decide_kernel, one block per group: M_g from the copied state and the group
// maxima 0..g (a maximum: exact in any order), F in place of d, then an EXACT selection of the two order statistics: a radix select over
// the 64-bit patterns of F, sign-fixed so they order as unsigned, 8 bits per pass, 256 bins in LDS counted with integer atomics (a count
// does not depend on the order of its additions) and scanned in lane order; F_(k+1) is F_(k) if more than k + 1 values are <= it, else
// the minimum of the values above it.  v >= b - 1 (q = 100, every reference call site; b = 1) skips the select: both statistics are the
// block's max F, put through the same interpolation arithmetic, so the bits are those of the general path.  A thread only ever re-reads
// the workspace entries it wrote itself.  No floating-point atomics, no floating-point sum at all: a rerun is bit-equal.  Floating-point
// contraction is OFF in this file: the reference rounds every product and sum separately.  A NaN score is not supported (numpy would
// propagate it to the whole batch).
//
//   compact: the rows i with mask[i] != 0 -- or every row of a group whose take_all flag is set, the reference's "too inefficient, take
//   the whole batch" branch (nsgan/GAN.py:332-338) -- go to dst[offset + k] in ascending order of i, k = 0, 1, ...; rows with
//   offset + k >= capacity are dropped; the unclipped number of selected rows is left in *total.
//
// Two launches.  1. compact_scan_kernel, one block: a thread counts a contiguous run of rows, the 256 counts are scanned in thread
// order, the thread writes the indices of its selected rows to list[] from its offset on.  2. rows_gather_kernel (rows.h, which also holds the launch
// plan and the pool limits) with CompactedRows: dst row k <- src row list[k].
#include "rows.h"

#pragma clang fp contract(off)

#define DRS_THREADS ROWS_THREADS
#define DRS_LO 1e-14
#define DRS_HI (1 - 1e-14)

// scipy.special.logit of an already clipped score
__device__ __forceinline__ double drs_logit(double x) {
    if (x < 0.3 || x > 0.65) return log(x / (1.0 - x));
    const double s = 2.0 * (x - 0.5);
    return log1p(s) - log1p(-s);
}
__device__ __forceinline__ double drs_clip(double s) { return s < DRS_LO ? DRS_LO : (s > DRS_HI ? DRS_HI : s); }

// order-preserving map of a double's bit pattern onto unsigned integers
__device__ __forceinline__ unsigned long long drs_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double drs_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// max (IS_MAX) or min of one double per thread, left in every thread; tab: DRS_THREADS doubles of LDS
template <bool IS_MAX>
__device__ __forceinline__ double drs_block_extreme(double v, double* tab, int t) {
    __syncthreads();                                                // (tab may still be read from the call before)
    tab[t] = v;
    for (int stride = DRS_THREADS / 2; stride >= 1; stride >>= 1) {
        __syncthreads();
        if (t < stride) {
            const double a = tab[t], b = tab[t + stride];
            tab[t] = IS_MAX ? (b > a ? b : a) : (b < a ? b : a);
        }
    }
    __syncthreads();
    return tab[0];
}

// inclusive scan of one unsigned per thread in thread order; wsum: DRS_THREADS / 64 words of LDS
__device__ __forceinline__ unsigned drs_block_scan(unsigned v, unsigned* wsum, int t) {
    const int lane = t & 63, wave = t >> 6;
    unsigned s = v;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(s, off, 64);
        if (lane >= off) s += o;
    }
    __syncthreads();                                                // (wsum may still be read from the call before)
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    for (int w = 0; w < wave; ++w) s += wsum[w];
    return s;
}

// ws: [0] the state as the call found it | [1, 1 + groups) max d per group | [1 + groups, 1 + groups + n) d, then F, per row
__global__ __launch_bounds__(DRS_THREADS) void drs_logit_kernel(const float* __restrict__ sig, int b, int groups, const double* __restrict__ state,
                                                                double* __restrict__ ws) {
    __shared__ double tab[DRS_THREADS];
    const int t = threadIdx.x, g = blockIdx.x;
    const float* s = sig + (size_t)g * b;
    double* d = ws + 1 + groups + (size_t)g * b;
    double mx = -INFINITY;
    for (int i = t; i < b; i += DRS_THREADS) {
        const double v = drs_logit(drs_clip((double)s[i]));
        d[i] = v;
        mx = v > mx ? v : mx;
    }
    mx = drs_block_extreme<true>(mx, tab, t);
    if (t == 0) {
        ws[1 + g] = mx;
        if (g == 0) ws[0] = state[0];
    }
}

__global__ __launch_bounds__(DRS_THREADS) void drs_decide_kernel(int b, int groups, const double* __restrict__ u, double eps, int has_q, int k_lo,
                                                                 double frac, double* __restrict__ ws, double* __restrict__ state,
                                                                 double* __restrict__ bounds, double* __restrict__ P, unsigned char* __restrict__ mask,
                                                                 int* __restrict__ counts) {
    __shared__ double tab[DRS_THREADS];
    __shared__ unsigned hist[DRS_THREADS];
    __shared__ unsigned wsum[DRS_THREADS / 64];
    __shared__ unsigned sel[2];
    __shared__ unsigned acc;
    const int t = threadIdx.x, g = blockIdx.x;
    double* F = ws + 1 + groups + (size_t)g * b;
    // M_g
    double M = t == 0 ? ws[0] : -INFINITY;
    for (int j = t; j <= g; j += DRS_THREADS) {
        const double v = ws[1 + j];
        M = v > M ? v : M;
    }
    M = drs_block_extreme<true>(M, tab, t);
    if (t == 0) {
        if (bounds) bounds[g] = M;
        if (g == groups - 1) state[0] = M;
    }
    // F in place of d
    double top = -INFINITY;
    for (int i = t; i < b; i += DRS_THREADS) {
        const double delta = F[i] - M;
        const double f = delta - log(1.0 - exp(delta - eps));
        F[i] = f;
        top = f > top ? f : top;
    }
    double gamma = 0.0;
    if (has_q) {
        double lo, hi;
        if (k_lo >= b - 1) {
            lo = hi = drs_block_extreme<true>(top, tab, t);
        } else {
            unsigned long long prefix = 0;
            unsigned k = (unsigned)k_lo;                            // rank among the rows that share `prefix`
            for (int shift = 56; shift >= 0; shift -= 8) {
                hist[t] = 0u;
                __syncthreads();
                const unsigned long long high = shift == 56 ? 0ull : (~0ull << (shift + 8));
                for (int i = t; i < b; i += DRS_THREADS) {
                    const unsigned long long key = drs_key(F[i]);
                    if ((key & high) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                const unsigned mine = hist[t];
                const unsigned incl = drs_block_scan(mine, wsum, t);
                if (mine > 0u && incl - mine <= k && k < incl) {    // exactly one bin holds rank k
                    sel[0] = (unsigned)t;
                    sel[1] = incl - mine;
                }
                __syncthreads();
                prefix |= (unsigned long long)sel[0] << shift;
                k -= sel[1];
                __syncthreads();
            }
            lo = drs_unkey(prefix);
            // F_(k_lo + 1): lo again if more than k_lo + 1 rows are <= lo, else the smallest row above it
            if (t == 0) acc = 0u;
            __syncthreads();
            unsigned le = 0u;
            double above = INFINITY;
            for (int i = t; i < b; i += DRS_THREADS) {
                const double f = F[i];
                if (drs_key(f) <= prefix) ++le;
                else above = f < above ? f : above;
            }
            atomicAdd(&acc, le);
            above = drs_block_extreme<false>(above, tab, t);       // (its barriers also order the atomics before the read below)
            hi = acc >= (unsigned)k_lo + 2u ? lo : above;
            __syncthreads();
        }
        const double diff = hi - lo;
        gamma = frac < 0.5 ? lo + diff * frac : hi - diff * (1.0 - frac);
    }
    if (t == 0) acc = 0u;
    __syncthreads();
    unsigned hits = 0u;
    for (int i = t; i < b; i += DRS_THREADS) {
        const size_t r = (size_t)g * b + i;
        const double p = 1.0 / (1.0 + exp(-(F[i] - gamma)));
        const bool take = u[r] < p;
        if (P) P[r] = p;
        mask[r] = take ? 1 : 0;
        hits += take ? 1u : 0u;
    }
    atomicAdd(&acc, hits);
    __syncthreads();
    if (t == 0) counts[g] = (int)acc;
}

// state = logit(clip(max s)) (rejector.py:11-14 on np.amax of the real scores)
__global__ __launch_bounds__(DRS_THREADS) void drs_set_max_kernel(const float* __restrict__ sig, int n, double* __restrict__ state) {
    __shared__ double tab[DRS_THREADS];
    const int t = threadIdx.x;
    double mx = -INFINITY;
    for (int i = t; i < n; i += DRS_THREADS) {
        const double v = (double)sig[i];
        mx = v > mx ? v : mx;
    }
    mx = drs_block_extreme<true>(mx, tab, t);
    if (t == 0) state[0] = drs_logit(drs_clip(mx));
}

__global__ __launch_bounds__(DRS_THREADS) void compact_scan_kernel(const unsigned char* __restrict__ mask, const unsigned char* __restrict__ take_all,
                                                                   int n, int b, int* __restrict__ list, int* __restrict__ total) {
    __shared__ unsigned wsum[DRS_THREADS / 64];
    const int t = threadIdx.x;
    const int chunk = (n + DRS_THREADS - 1) / DRS_THREADS;
    const long i0 = (long)t * chunk;
    const int c0 = i0 < n ? (int)i0 : n;
    const int c1 = i0 + chunk < n ? (int)(i0 + chunk) : n;
    unsigned cnt = 0u;
    for (int i = c0; i < c1; ++i) cnt += ((take_all && take_all[i / b]) || mask[i]) ? 1u : 0u;
    const unsigned incl = drs_block_scan(cnt, wsum, t);
    unsigned k = incl - cnt;
    for (int i = c0; i < c1; ++i)
        if ((take_all && take_all[i / b]) || mask[i]) list[k++] = i;
    if (t == DRS_THREADS - 1) total[0] = (int)incl;
}

// the compaction's rows for rows_gather_kernel: the first min(total, room) entries of the scan's list, to dst (the offset is in the pointer)
struct CompactedRows {
    const int* list;
    const int* total;
    long room;
    __device__ bool span(long long& at, long long& cnt) const {
        at = 0;
        cnt = total[0] < room ? total[0] : room;
        return true;
    }
    __device__ bool row(long long k, long long& r) const {
        r = list[k];
        return true;
    }
};

extern "C" {

size_t cgs_drs_ws_bytes(int b, int groups) {
    if (!rows_batches_ok(b, groups)) return 0;
    return (size_t)(1 + (long)groups + (long)b * groups) * sizeof(double);
}

int cgs_drs_decide(const float* sig, int b, int groups, const double* uniforms, double epsilon, double shift_percent, double* state, double* bounds,
                   double* P, unsigned char* mask, int* counts, void* ws, size_t ws_bytes, void* stream) {
    if (!rows_batches_ok(b, groups) || !(shift_percent <= 100.0) || !(epsilon > 0.0))
        return cgs_set_error(CGS_EINVAL, "drs_decide: needs 1 <= b, 1 <= groups <= 2^20, b * groups <= 2^30, shift_percent <= 100 (negative: none), epsilon > 0 "
                             "(b=%d groups=%d shift_percent=%g epsilon=%g)", b, groups, shift_percent, epsilon);
    if (!sig || !uniforms || !state || !mask || !counts) return cgs_set_error(CGS_EINVAL, "drs_decide: null sig / uniforms / state / mask / counts");
    const size_t need = cgs_drs_ws_bytes(b, groups);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "drs_decide: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 7) return cgs_set_error(CGS_EINVAL, "drs_decide: the workspace must be 8-byte aligned");
    const int has_q = shift_percent >= 0.0;
    int k_lo = 0;
    double frac = 0.0;
    if (has_q) {                                                    // numpy: virtual index (b - 1) * (q / 100), both rounded
        const double v = (double)(b - 1) * (shift_percent / 100.0);
        const double fl = floor(v);
        if (fl >= (double)(b - 1)) k_lo = b - 1;                    // both order statistics are the last one
        else { k_lo = (int)fl; frac = v - fl; }
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(drs_logit_kernel, dim3(groups), dim3(DRS_THREADS), 0, s, sig, b, groups, (const double*)state, (double*)ws);
    CGS_CHECK_LAUNCH("drs_decide");
    hipLaunchKernelGGL(drs_decide_kernel, dim3(groups), dim3(DRS_THREADS), 0, s, b, groups, uniforms, epsilon, has_q, k_lo, frac, (double*)ws, state, bounds,
                       P, mask, counts);
    CGS_CHECK_LAUNCH("drs_decide");
    return CGS_OK;
}

int cgs_drs_set_max(const float* sig, int n, double* state, void* stream) {
    if (n < 1 || n > ROWS_MAX_N) return cgs_set_error(CGS_EINVAL, "drs_set_max: needs 1 <= n <= 2^30 (n=%d)", n);
    if (!sig || !state) return cgs_set_error(CGS_EINVAL, "drs_set_max: null sig / state");
    hipLaunchKernelGGL(drs_set_max_kernel, dim3(1), dim3(DRS_THREADS), 0, (hipStream_t)stream, sig, n, state);
    CGS_CHECK_LAUNCH("drs_set_max");
    return CGS_OK;
}

size_t cgs_compact_rows_ws_bytes(int n) {
    if (n < 1 || n > ROWS_MAX_N) return 0;
    return (size_t)n * sizeof(int);
}

int cgs_compact_rows(const float* src, int n, int row, const unsigned char* mask, const unsigned char* take_all, int groups, float* dst, long long offset,
                     long long capacity, int* total, void* ws, size_t ws_bytes, void* stream) {
    if (!rows_source_ok(n, row) || offset < 0 || capacity < 0 || groups < 1 || (n > 0 && n % groups != 0))
        return cgs_set_error(CGS_EINVAL, "compact_rows: needs 0 <= n <= 2^30 in whole groups, 1 <= row <= 2^22, n * row <= 2^40, offset >= 0, capacity >= 0 "
                             "(n=%d row=%d groups=%d offset=%lld capacity=%lld)", n, row, groups, offset, capacity);
    if (!total) return cgs_set_error(CGS_EINVAL, "compact_rows: null total");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(total, 0, sizeof(int), s) != hipSuccess) return cgs_set_error(CGS_ELAUNCH, "compact_rows: memset of total failed");
        return CGS_OK;
    }
    if (!src || !mask || !dst) return cgs_set_error(CGS_EINVAL, "compact_rows: null src / mask / dst");
    const size_t need = (size_t)n * sizeof(int);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "compact_rows: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 3) return cgs_set_error(CGS_EINVAL, "compact_rows: the workspace must be 4-byte aligned");
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(DRS_THREADS), 0, s, mask, take_all, n, n / groups, (int*)ws, total);
    CGS_CHECK_LAUNCH("compact_rows");
    const long room = capacity > offset ? (long)(capacity - offset) : 0;
    const long most = room < n ? room : n;                          // rows the gather can have to write
    if (most == 0) return CGS_OK;
    rows_gather_launch(src, dst + (size_t)offset * row, row, most, CompactedRows{(const int*)ws, total, room}, s);
    CGS_CHECK_LAUNCH("compact_rows");
    return CGS_OK;
}

}  // extern "C"
