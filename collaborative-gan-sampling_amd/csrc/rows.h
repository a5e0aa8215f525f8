// Row pools of the evaluation legs (drs.hip, mh.hip): the limits of a batch and of a pool, and the one copy of
// listed rows into a pool -- its launch plan and its kernel.  What differs between the two callers is a small device-side policy.
#pragma once
#include "cgs_internal.h"

#define ROWS_THREADS 256
#define ROWS_MAX_N 0x40000000L                                          // rows of a batch, of a source or of a list
#define ROWS_MAX_GROUPS (1 << 20)
#define ROWS_MAX_ROW (1 << 22)                                          // floats per row

// b scores per logical batch, `groups` batches in one call
static inline bool rows_batches_ok(long b, long groups) { return b >= 1 && groups >= 1 && groups <= ROWS_MAX_GROUPS && b * groups <= ROWS_MAX_N; }
// a source of n rows of `row` floats
static inline bool rows_source_ok(long n, long row) { return n >= 0 && n <= ROWS_MAX_N && row >= 1 && row <= ROWS_MAX_ROW && n * row <= (1L << 40); }

// The gather's launch: rows move in 16-byte pieces where the row length and both bases allow, in 4-byte pieces otherwise.  A row of at most
// a block's threads shares the block with its neighbours (rows_per_block of them: thread t has row t / pieces, piece t % pieces), so a
// 2-float row costs two lanes; a longer row (rows_per_block = 0) spans grid_y blocks.  `most`: the rows the gather can have to write.
struct RowsPlan {
    bool wide;
    int pieces, rows_per_block;
    unsigned grid_x, grid_y;
};
static inline RowsPlan rows_gather_plan(int row, const void* src, const void* dst, long most) {
    RowsPlan p;
    p.wide = row % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    p.pieces = p.wide ? row / 4 : row;
    p.rows_per_block = p.pieces <= ROWS_THREADS ? ROWS_THREADS / p.pieces : 0;
    const int per = p.rows_per_block;
    p.grid_x = per ? (unsigned)((most + per - 1) / per) : (unsigned)most;
    p.grid_y = per ? 1u : (unsigned)cgs_ceil_div(p.pieces, ROWS_THREADS);
    return p;
}

#ifdef __HIPCC__
// dst row at + k <- src row r, for k < cnt.  FROM says where the three come from:
//   bool span(long long& at, long long& cnt)      false: nothing to copy
//   bool row(long long k, long long& r)           false: row k copies nothing
template <typename V, typename FROM>
__global__ __launch_bounds__(ROWS_THREADS) void rows_gather_kernel(const V* __restrict__ src, const FROM from, int pieces, int rows_per_block,
                                                                   V* __restrict__ dst) {
    const int t = threadIdx.x;
    long long at, cnt;
    if (!from.span(at, cnt)) return;
    long long k;
    int c;
    if (rows_per_block > 0) {
        const int r = t / pieces;
        if (r >= rows_per_block) return;
        c = t - r * pieces;
        k = (long long)blockIdx.x * rows_per_block + r;
    } else {
        c = blockIdx.y * ROWS_THREADS + t;
        if (c >= pieces) return;
        k = blockIdx.x;
    }
    if (k >= cnt) return;
    long long r;
    if (!from.row(k, r)) return;
    dst[(size_t)(at + k) * pieces + c] = src[(size_t)r * pieces + c];
}

template <typename FROM>
static inline void rows_gather_launch(const float* src, float* dst, int row, long most, const FROM& from, hipStream_t s) {
    const RowsPlan p = rows_gather_plan(row, src, dst, most);
    const dim3 grid(p.grid_x, p.grid_y);
    if (p.wide)
        hipLaunchKernelGGL((rows_gather_kernel<float4, FROM>), grid, dim3(ROWS_THREADS), 0, s, (const float4*)src, from, p.pieces, p.rows_per_block, (float4*)dst);
    else
        hipLaunchKernelGGL((rows_gather_kernel<float, FROM>), grid, dim3(ROWS_THREADS), 0, s, src, from, p.pieces, p.rows_per_block, dst);
}
#endif
