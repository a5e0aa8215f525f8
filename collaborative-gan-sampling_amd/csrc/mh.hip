// The Metropolis-Hastings independence chain on the device (sampling.DeviceIndependenceSampler): what the
// reference's IndependenceSampler (sampling/idpsampler.py:4-53) emits per logical batch ("segment") of b proposals, and the gather of the
// emitted rows -- a row may repeat, so the stable compaction of drs.hip does not serve -- into a pool.
//
//   walk, per segment, as if IndependenceSampler.walk had been called once per batch, in order; d (a double) and cnt are carried on:
//     per proposal i, in order, every operation a separately rounded fp32 one:
//       odds  = (s_i * omd) / (df * (1.0f - s_i))        omd = (float)(1.0 - d), df = (float)d
//       alpha = odds < 1.0f ? odds : 1.0f                (Python's min(1.0, odds): a NaN gives 1.0)
//       moved = !(u_i > (double)alpha);  if moved: d = s_i
//     from the positions pos[0] < pos[1] < ... of the segment's moves: nothing is emitted unless there are more than B of them;
//     first = pos[B]; the visits v = first .. b - 1 are active, a = v - first; emissions at a = a0, a0 + (T + 1), ..., a0 = max(0, T + 1 - cnt);
//     the emitted row is the last move position <= v; cnt leaves as 1 + (active visits after the last emission), or cnt + (active visits)
//     if nothing was emitted.
//
// One launch of one block; the segments are taken in order.  Phase 1: wave 0 owns the chain.  It loads a window of 64 proposals, evaluates
// `moved` for every lane against the current d -- the definition itself, no monotonicity shortcut -- ballots, jumps to the first set lane
// above the last move, and repeats inside the window until no lane moves; then the next window.  moves + windows steps instead of b.  The
// moves of a window leave as one bit mask, from which the lanes write their positions to the workspace.  Phase 2, the whole block:
// emission k stands at visit first + a0 + k (T + 1) and takes the last move at or before it (a binary search in the positions).  No
// atomics, no floating-point sum: a rerun from the same state is bit-equal.  Contraction is off; the division is the correctly rounded
// one and fp32 denormals are kept (the build has no fast-math): the reference's numpy arithmetic does both.
#include "rows.h"

#pragma clang fp contract(off)

#define MH_THREADS ROWS_THREADS

// ws: b ints, the move positions of the segment at hand
__global__ __launch_bounds__(MH_THREADS) void mh_walk_kernel(const float* __restrict__ sig, int b, int groups, const double* __restrict__ uniforms, int T,
                                                             int B, const unsigned char* __restrict__ take_all, double* __restrict__ state,
                                                             long long* __restrict__ fill_io, long long capacity, int* __restrict__ rows,
                                                             int* __restrict__ counts, long long* __restrict__ span, int* __restrict__ pos) {
    __shared__ int sh_moves;
    const int t = threadIdx.x, lane = t & 63;
    // block-uniform: every thread carries the same values
    double d = state[0];
    long long cnt = (long long)state[1];
    const long long fill0 = fill_io[0];
    long long fill = fill0, listed = 0;
    const long long period = (long long)T + 1;
    for (int g = 0; g < groups; ++g) {
        if (fill >= capacity) {                                        // the pool is full: the reference's loop never reaches this batch
            if (t == 0) counts[g] = -1;
            continue;
        }
        const long long row0 = (long long)g * b;
        if (take_all && take_all[g]) {                                 // "too inefficient": the batch as it is, the chain untouched
            for (int i = t; i < b; i += MH_THREADS) rows[listed + i] = (int)(row0 + i);
            if (t == 0) counts[g] = b;
            fill += b;
            listed += b;
            continue;
        }
        __syncthreads();                                               // (pos and sh_moves may still be read from the segment before)
        if (t < 64) {                                                  // phase 1: wave 0 walks the segment
            const float* s_g = sig + row0;
            const double* u_g = uniforms + row0;
            int moves = 0;
            for (int w0 = 0; w0 < b; w0 += 64) {
                const int i = w0 + lane;
                const bool valid = i < b;
                const float s = valid ? s_g[i] : 0.0f;
                const double u = valid ? u_g[i] : 2.0;
                const float oms = 1.0f - s;
                unsigned long long moved = 0ull;
                int start = 0;                                         // the lanes below it have been passed
                while (start < 64) {
                    const float df = (float)d, omd = (float)(1.0 - d);
                    const float odds = (s * omd) / (df * oms);
                    const float alpha = odds < 1.0f ? odds : 1.0f;
                    const bool mv = valid && lane >= start && !(u > (double)alpha);
                    const unsigned long long hit = __ballot(mv);
                    if (hit == 0ull) break;
                    const int l = __ffsll(hit) - 1;
                    d = (double)__shfl(s, l, 64);
                    moved |= 1ull << l;
                    start = l + 1;
                }
                if ((moved >> lane) & 1ull) pos[moves + __popcll(moved & ((1ull << lane) - 1ull))] = i;
                moves += __popcll(moved);
            }
            if (t == 0) sh_moves = moves;
        }
        __syncthreads();                                               // (also orders wave 0's stores to pos before the reads below)
        const int moves = sh_moves;
        long long emitted = 0;
        if (moves > B) {                                               // phase 2: the emissions, from the move positions
            const int first = pos[B];
            const long long active = (long long)b - first;
            const long long a0 = period - cnt > 0 ? period - cnt : 0;
            if (active > a0) {
                emitted = (active - 1 - a0) / period + 1;
                for (long long k = t; k < emitted; k += MH_THREADS) {
                    const int v = (int)(first + a0 + k * period);
                    int lo = B, hi = moves - 1;                        // the largest j with pos[j] <= v; pos[B] = first <= v
                    while (lo < hi) {
                        const int mid = lo + (hi - lo + 1) / 2;
                        if (pos[mid] <= v) lo = mid; else hi = mid - 1;
                    }
                    rows[listed + k] = (int)(row0 + pos[lo]);
                }
                cnt = active - a0 - (emitted - 1) * period;            // 1 + the active visits after the last emission
            } else {
                cnt += active;
            }
        }
        if (t == 0) counts[g] = (int)emitted;
        fill += emitted;
        listed += emitted;
    }
    if (t == 0) {                                                      // (d is wave 0's: the other waves never walk)
        state[0] = d;
        state[1] = (double)cnt;
        fill_io[0] = fill;
        span[0] = fill0;
        span[1] = listed;
    }
}

// the walk's rows for rows_gather_kernel: dst[span[0] + k] = src[rows[k]], k < min(span[1], listed_max), while span[0] + k < capacity; an index
// outside the source copies nothing
struct WalkedRows {
    const int* rows;
    const long long* span_io;
    int n, listed_max;
    long long capacity;
    __device__ bool span(long long& at, long long& cnt) const {
        at = span_io[0];
        cnt = span_io[1] < listed_max ? span_io[1] : listed_max;
        if (at < 0) return false;
        if (cnt > capacity - at) cnt = capacity - at;
        return true;
    }
    __device__ bool row(long long k, long long& r) const {
        r = rows[k];
        return r >= 0 && r < n;
    }
};

extern "C" {

size_t cgs_mh_ws_bytes(int b, int groups) {
    if (!rows_batches_ok(b, groups)) return 0;
    return (((size_t)b * sizeof(int)) + 7) & ~(size_t)7;
}

int cgs_mh_walk(const float* sig, int b, int groups, const double* uniforms, int T, int B, const unsigned char* take_all, double* state, long long* fill,
                long long capacity, int* rows, int* counts, long long* span, void* ws, size_t ws_bytes, void* stream) {
    if (!rows_batches_ok(b, groups) || T < 0 || B < 0 || capacity < 0)
        return cgs_set_error(CGS_EINVAL, "mh_walk: needs 1 <= b, 1 <= groups <= 2^20, b * groups <= 2^30, T >= 0, B >= 0, capacity >= 0 "
                             "(b=%d groups=%d T=%d B=%d capacity=%lld)", b, groups, T, B, capacity);
    if (!sig || !uniforms || !state || !fill || !rows || !counts || !span)
        return cgs_set_error(CGS_EINVAL, "mh_walk: null sig / uniforms / state / fill / rows / counts / span");
    const size_t need = cgs_mh_ws_bytes(b, groups);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "mh_walk: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 3) return cgs_set_error(CGS_EINVAL, "mh_walk: the workspace must be 4-byte aligned");
    hipLaunchKernelGGL(mh_walk_kernel, dim3(1), dim3(MH_THREADS), 0, (hipStream_t)stream, sig, b, groups, uniforms, T, B, take_all, state, fill, capacity,
                       rows, counts, span, (int*)ws);
    CGS_CHECK_LAUNCH("mh_walk");
    return CGS_OK;
}

int cgs_gather_rows(const float* src, int n, int row, const int* rows, int listed_max, const long long* span, float* dst, long long capacity,
                    void* stream) {
    if (!rows_source_ok(n, row) || listed_max < 0 || listed_max > ROWS_MAX_N || capacity < 0)
        return cgs_set_error(CGS_EINVAL, "gather_rows: needs 0 <= n <= 2^30, 1 <= row <= 2^22, n * row <= 2^40, 0 <= listed_max <= 2^30, capacity >= 0 "
                             "(n=%d row=%d listed_max=%d capacity=%lld)", n, row, listed_max, capacity);
    if (!span) return cgs_set_error(CGS_EINVAL, "gather_rows: null span");
    const long most = capacity < listed_max ? (long)capacity : (long)listed_max;     // rows the gather can have to write
    if (n == 0 || most == 0) return CGS_OK;
    if (!src || !rows || !dst) return cgs_set_error(CGS_EINVAL, "gather_rows: null src / rows / dst");
    rows_gather_launch(src, dst, row, most, WalkedRows{rows, span, n, listed_max, capacity}, (hipStream_t)stream);
    CGS_CHECK_LAUNCH("gather_rows");
    return CGS_OK;
}

}  // extern "C"
