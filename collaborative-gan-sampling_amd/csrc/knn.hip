// Nearest-neighbour queries between two pools of feature vectors, in double on the device (metrics.nn_distance / knn_radii /
// manifold_metrics): one tiled pairwise squared-distance core with three epilogues.
//
//   D2(j, i) = sum_k ((double)q_jk - (double)r_ik)^2        k ascending, one subtract and one fused multiply-add per coordinate
//
// The DIFFERENCE form, not |q|^2 + |r|^2 - 2 q.r, for the reasons kde2d.hip differences raw coordinates first: equal rows give exactly
// 0 (MH pools repeat rows), D2(j, i) and D2(i, j) are the same bits ((-x)^2 == x^2, same k order), and the error is RELATIVE -- every
// term is non-negative, so |D2^ - D2| <= (d + 3) 2^-53 D2 (DESIGN derives it) -- which is what lets the discrete outputs (indices,
// counts, the metrics) equal the host's wherever the inputs' gaps exceed that bound.
//
// 1. knn_kernel<OP>, grid (query tiles, splits), 256 threads.  A block owns 64 queries and walks the 64-reference tiles
//    [split * per, (split + 1) * per).  Per tile the d coordinates go by in chunks of 32: both panels are converted to double on load and
//    parked in LDS k-major ([32][KNN_PITCH], 64 rows + 16 of padding as MOM_LDS_ROW of moments.hip: a thread's four rows are one 32-byte
//    ds_read_b128 pair, the 16 lanes of a query row read 512 contiguous bytes of the reference panel, the query panel is a broadcast).
//    Rows past m / n and columns past d come from predicated loads as exact zeros, nothing outside the inputs is read; the next chunk is
//    loaded to registers while the current one is accumulated.  Thread (t >> 4, t & 15) owns a 4 x 4 sub-tile of double accumulators.
//    A finished tile is parked in LDS transposed ([reference][query]) and scanned by ALL 256 threads: thread (query t & 63, part t >> 6)
//    takes the tile's references part * 16 .. + 15 in ascending order into its epilogue state (references past n are skipped: a
//    wave-uniform test).  After the walk the four parts of a query are merged through LDS, and the block either stores the answer
//    (splits == 1) or leaves the state in ws[split][slot][m].
// 2. knn_reduce_kernel<OP>, one thread per query: merges the splits in ascending order and stores the answer.
// The epilogue states and why their merges do not depend on how the references were cut:
//    NN_MIN   (best D2, its index, D2(j, j)): ordered by (D2, index) lexicographically -- a total order, so the minimum is unique.
//    RADII    the 8 smallest D2 as a sorted list in registers: the k-th smallest VALUE of a multiset is the same whatever the tie order.
//    BALL     an integer count.
// No atomics anywhere: a rerun is bit-identical.  Not built: the matrix-instruction form (|q|^2 + |r|^2 - 2 q.r on v_mfma_f64) -- it would
// save the subtract, at most 2x, and its error bound is absolute (cancellation), which would make every discrete output tie-dependent.
#include "cgs_internal.h"

#define KNN_TILE 64               // queries per block = references per tile
#define KNN_KC 32                 // coordinates per LDS chunk
#define KNN_PITCH 80              // doubles between two coordinates of a panel (64 + 16)
#define KNN_TPITCH 66             // doubles between two references of a parked tile
#define KNN_BLOCKS 512            // blocks aimed at: two per CU
#define KNN_MIN_TILES 4           // at least this many reference tiles per split (a split costs one partial state per query)
#define KNN_MAX_SPLITS 64
#define KNN_MAX_D 2048
#define KNN_MAX_ROWS 0x40000000L  // (32-bit row indices, tile ends included)
#define KNN_MAX_K 8
#define KNN_LDS (2 * KNN_KC * KNN_PITCH)

struct KnnPlan {
    int qt, rt;      // query tiles, reference tiles
    int per, splits; // reference tiles per split, splits
};

// The cut depends on (m, n) alone; the launcher, cgs_knn_ws_bytes and cgs_knn_plan read it here.
static bool knn_plan(KnnPlan& p, long m, long n, int d) {
    if (d < 1 || d > KNN_MAX_D || m < 1 || n < 1 || m > KNN_MAX_ROWS || n > KNN_MAX_ROWS) return false;
    p.qt = (int)((m + KNN_TILE - 1) / KNN_TILE);
    p.rt = (int)((n + KNN_TILE - 1) / KNN_TILE);
    long s = (KNN_BLOCKS + p.qt - 1) / p.qt;
    const long by_n = p.rt / KNN_MIN_TILES > 1 ? p.rt / KNN_MIN_TILES : 1;
    if (s > by_n) s = by_n;
    if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
    p.per = (int)((p.rt + s - 1) / s);
    p.splits = (p.rt + p.per - 1) / p.per;
    return true;
}

static int knn_slots(int op, int k) { return op == CGS_KNN_NN_MIN ? 3 : op == CGS_KNN_RADII ? k : 1; }

static size_t knn_ws_need(const KnnPlan& p, int op, long m, int k) {
    return p.splits > 1 ? (size_t)p.splits * knn_slots(op, k) * (size_t)m * sizeof(double) : 0;
}

struct KnnParams {
    const float* qry;       // [m][d]
    const float* ref;       // [n][d]
    const double* ref_r2;   // BALL: [n]
    double* out_d;          // NN_MIN: [m] (+ [m] D2(j, j) with excl); RADII: [m]
    int* out_i;             // NN_MIN: the index; BALL: the count
    double* ws;             // [splits][slots][m]
    int m, n, d, k, excl;
    int rt, per, splits, slots;
};

template <int OP> struct KnnState;

template <> struct KnnState<CGS_KNN_NN_MIN> {
    static constexpr int NS = 3;
    double best, self;
    int idx;
    __device__ __forceinline__ void init() { best = __builtin_inf(); self = -1.0; idx = -1; }
    __device__ __forceinline__ void take(double v, int i, int j, const KnnParams& p) {
        if (p.excl && i == j) self = v;
        else if (v < best) { best = v; idx = i; }                   // ascending i: the lowest index of equal values stays
    }
    __device__ __forceinline__ void merge(const KnnState& o) {                      // (D2, index) lexicographic; -1 = none compares as the largest index
        if (o.best < best || (o.best == best && (unsigned)o.idx < (unsigned)idx)) { best = o.best; idx = o.idx; }
        if (o.self >= 0.0) self = o.self;                            // exactly one tile holds i == j
    }
    __device__ __forceinline__ double get(int e) const { return e == 0 ? best : e == 1 ? self : (double)idx; }
    __device__ __forceinline__ void set(int e, double v) { if (e == 0) best = v; else if (e == 1) self = v; else idx = (int)v; }
    __device__ __forceinline__ void store(const KnnParams& p, int j) const {
        p.out_d[j] = best;
        if (p.excl) p.out_d[(size_t)p.m + j] = self;
        p.out_i[j] = idx;
    }
};

template <> struct KnnState<CGS_KNN_RADII> {
    static constexpr int NS = KNN_MAX_K;
    double l[KNN_MAX_K];                                             // ascending
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int e = 0; e < KNN_MAX_K; ++e) l[e] = __builtin_inf();
    }
    __device__ __forceinline__ void insert(double v) {
        if (v < l[KNN_MAX_K - 1]) {
            l[KNN_MAX_K - 1] = v;
#pragma unroll
            for (int s = KNN_MAX_K - 1; s > 0; --s) {
                const double a = l[s - 1], b = l[s];
                l[s - 1] = b < a ? b : a;
                l[s] = b < a ? a : b;
            }
        }
    }
    __device__ __forceinline__ void take(double v, int i, int j, const KnnParams& p) {
        if (!(p.excl && i == j)) insert(v);
    }
    __device__ __forceinline__ void merge(const KnnState& o) {
#pragma unroll
        for (int e = 0; e < KNN_MAX_K; ++e) insert(o.l[e]);
    }
    __device__ __forceinline__ double get(int e) const {
        double v = l[0];
#pragma unroll
        for (int s = 1; s < KNN_MAX_K; ++s) v = e == s ? l[s] : v;
        return v;
    }
    __device__ __forceinline__ void set(int e, double v) {
#pragma unroll
        for (int s = 0; s < KNN_MAX_K; ++s) l[s] = e == s ? v : l[s];
    }
    __device__ __forceinline__ void store(const KnnParams& p, int j) const { p.out_d[j] = get(p.k - 1); }
};

template <> struct KnnState<CGS_KNN_BALL_COUNT> {
    static constexpr int NS = 1;
    int cnt;
    __device__ __forceinline__ void init() { cnt = 0; }
    __device__ __forceinline__ void take(double v, int i, int, const KnnParams& p) { cnt += v <= p.ref_r2[i] ? 1 : 0; }
    __device__ __forceinline__ void merge(const KnnState& o) { cnt += o.cnt; }
    __device__ __forceinline__ double get(int) const { return (double)cnt; }       // (a count is below 2^30: exact as a double)
    __device__ __forceinline__ void set(int, double v) { cnt = (int)v; }
    __device__ __forceinline__ void store(const KnnParams& p, int j) const { p.out_i[j] = cnt; }
};

template <int OP>
__global__ __launch_bounds__(256) void knn_kernel(KnnParams p) {
    __shared__ __align__(16) double lds[KNN_LDS];
    double* qs = lds;                                                // [KNN_KC][KNN_PITCH]
    double* rs = lds + KNN_KC * KNN_PITCH;
    const int t = threadIdx.x;
    const int lrow = t >> 2, lseg = t & 3;                           // loader: row lrow of both panels, coordinates lseg * 8 .. + 7 of the chunk
    const int tq = t >> 4, tr = t & 15;                              // accumulator: queries tq * 4 .. + 3, references tr * 4 .. + 3
    const int eq = t & 63, part = t >> 6;                            // epilogue: query eq, references part * 16 .. + 15 of the tile
    const int q0 = blockIdx.x * KNN_TILE;
    const int t0 = blockIdx.y * p.per;
    const int t1 = t0 + p.per < p.rt ? t0 + p.per : p.rt;
    const int nch = (p.d + KNN_KC - 1) / KNN_KC;
    const int steps = (t1 - t0) * nch;                               // (at most 2^24 tiles x 64 chunks)

    float fq[8], fr[8];
    auto fetch = [&](int step) {
        const int tile = t0 + step / nch;
        const int k0 = (step % nch) * KNN_KC + lseg * 8;
        const long jq = (long)q0 + lrow, ir = (long)tile * KNN_TILE + lrow;
        const bool okq = jq < p.m, okr = ir < p.n;
        const float* qp = p.qry + (size_t)(okq ? jq : 0) * p.d;
        const float* rp = p.ref + (size_t)(okr ? ir : 0) * p.d;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + u;
            fq[u] = (okq && k < p.d) ? qp[k] : 0.f;
            fr[u] = (okr && k < p.d) ? rp[k] : 0.f;
        }
    };

    KnnState<OP> st;
    st.init();
    double acc[4][4];
    if (steps > 0) fetch(0);
    for (int step = 0; step < steps; ++step) {
        const int ch = step % nch, tile = t0 + step / nch;
        if (ch == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {                               // rows past the end and columns past d: exact 0 on both sides
            qs[(lseg * 8 + u) * KNN_PITCH + lrow] = (double)fq[u];
            rs[(lseg * 8 + u) * KNN_PITCH + lrow] = (double)fr[u];
        }
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);                       // (block-uniform) in flight under the sums below
        const int kc = p.d - ch * KNN_KC < KNN_KC ? p.d - ch * KNN_KC : KNN_KC;
#pragma unroll 4
        for (int kk = 0; kk < kc; ++kk) {                            // k ascending: the one fixed order
            double qv[4], rv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) qv[a] = qs[kk * KNN_PITCH + tq * 4 + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) rv[b] = rs[kk * KNN_PITCH + tr * 4 + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double df = qv[a] - rv[b];                 // the subtraction first
                    acc[a][b] = fma(df, df, acc[a][b]);
                }
        }
        __syncthreads();
        if (ch == nch - 1) {                                         // (block-uniform) the tile is finished: park it [reference][query]
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int a = 0; a < 4; ++a) lds[(tr * 4 + b) * KNN_TPITCH + tq * 4 + a] = acc[a][b];
            __syncthreads();
            const int j = q0 + eq;
            const long i0 = (long)tile * KNN_TILE + part * 16;
#pragma unroll 4
            for (int e = 0; e < 16; ++e) {
                const long i = i0 + e;
                if (i < p.n) st.take(lds[(part * 16 + e) * KNN_TPITCH + eq], (int)i, j, p);     // (wave-uniform test)
            }
            __syncthreads();
        }
    }

    // the four parts of a query, in part order
#pragma unroll
    for (int e = 0; e < KnnState<OP>::NS; ++e) lds[e * 256 + t] = st.get(e);
    __syncthreads();
    if (t < KNN_TILE) {
#pragma unroll
        for (int pt = 1; pt < 4; ++pt) {
            KnnState<OP> o;
#pragma unroll
            for (int e = 0; e < KnnState<OP>::NS; ++e) o.set(e, lds[e * 256 + pt * 64 + t]);
            st.merge(o);
        }
        const long j = (long)q0 + t;
        if (j < p.m) {
            if (p.splits == 1) st.store(p, (int)j);
            else {
#pragma unroll
                for (int e = 0; e < KnnState<OP>::NS; ++e)           // (unrolled: the list stays in registers)
                    if (e < p.slots) p.ws[((size_t)blockIdx.y * p.slots + e) * (size_t)p.m + j] = st.get(e);
            }
        }
    }
}

template <int OP>
__global__ __launch_bounds__(256) void knn_reduce_kernel(KnnParams p) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= p.m) return;
    KnnState<OP> st;
    st.init();
    for (int s = 0; s < p.splits; ++s) {                             // ascending split order
        KnnState<OP> o;
        o.init();
#pragma unroll
        for (int e = 0; e < KnnState<OP>::NS; ++e)                   // (a partial state carries the first p.slots values; the rest keep init's)
            if (e < p.slots) o.set(e, p.ws[((size_t)s * p.slots + e) * (size_t)p.m + j]);
        st.merge(o);
    }
    st.store(p, (int)j);
}

template <int OP>
static int knn_launch(const char* who, const KnnPlan& pl, KnnParams& k, void* ws, size_t ws_bytes, hipStream_t s) {
    const size_t need = knn_ws_need(pl, OP, k.m, k.k);
    if (need && (!ws || ws_bytes < need)) return cgs_set_error(CGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    if (need && ((uintptr_t)ws & 7)) return cgs_set_error(CGS_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    k.ws = (double*)ws;
    k.rt = pl.rt; k.per = pl.per; k.splits = pl.splits; k.slots = knn_slots(OP, k.k);
    hipLaunchKernelGGL(knn_kernel<OP>, dim3(pl.qt, pl.splits), dim3(256), 0, s, k);
    CGS_CHECK_LAUNCH(who);
    if (pl.splits > 1) {
        hipLaunchKernelGGL(knn_reduce_kernel<OP>, dim3((k.m + 255) / 256), dim3(256), 0, s, k);
        CGS_CHECK_LAUNCH(who);
    }
    return CGS_OK;
}

extern "C" {

int cgs_knn_plan(int m, int n, int d, int* plan) {
    KnnPlan p;
    if (!plan || !knn_plan(p, m, n, d)) return 0;
    plan[0] = p.qt; plan[1] = p.rt; plan[2] = p.per; plan[3] = p.splits;
    return 1;
}

size_t cgs_knn_ws_bytes(int op, int m, int n, int d, int k) {
    KnnPlan p;
    if (op < CGS_KNN_NN_MIN || op > CGS_KNN_BALL_COUNT || !knn_plan(p, m, n, d)) return 0;
    if (op == CGS_KNN_RADII && (k < 1 || k > KNN_MAX_K)) return 0;
    const size_t need = knn_ws_need(p, op, m, k);
    return need > 8 ? need : 8;
}

int cgs_nn_min(const float* qry, int m, const float* ref, int n, int d, int exclude_self, double* out_d2, int* out_idx, void* ws,
               size_t ws_bytes, void* stream) {
    KnnPlan pl;
    if (!knn_plan(pl, m, n, d))
        return cgs_set_error(CGS_EINVAL, "nn_min: needs 1 <= d <= %d and 1 <= m, n <= 2^30 (m=%d n=%d d=%d)", KNN_MAX_D, m, n, d);
    if (exclude_self != 0 && exclude_self != 1) return cgs_set_error(CGS_EINVAL, "nn_min: exclude_self = %d is neither 0 nor 1", exclude_self);
    if (exclude_self && n != m) return cgs_set_error(CGS_EINVAL, "nn_min: exclude_self needs n == m (m=%d n=%d)", m, n);
    if (!qry || !ref || !out_d2 || !out_idx) return cgs_set_error(CGS_EINVAL, "nn_min: null qry / ref / out_d2 / out_idx");
    KnnParams k = {};
    k.qry = qry; k.ref = ref; k.out_d = out_d2; k.out_i = out_idx;
    k.m = m; k.n = n; k.d = d; k.k = 0; k.excl = exclude_self;
    return knn_launch<CGS_KNN_NN_MIN>("nn_min", pl, k, ws, ws_bytes, (hipStream_t)stream);
}

int cgs_knn_radii(const float* x, int n, int d, int k, int exclude_self, const float* other, int n_other, double* out_r2, void* ws,
                  size_t ws_bytes, void* stream) {
    KnnPlan pl;
    const int nref = other ? n_other : n;
    if (!knn_plan(pl, n, nref, d))
        return cgs_set_error(CGS_EINVAL, "knn_radii: needs 1 <= d <= %d and 1 <= n, n_other <= 2^30 (n=%d n_other=%d d=%d)", KNN_MAX_D, n, nref, d);
    if (k < 1 || k > KNN_MAX_K) return cgs_set_error(CGS_EINVAL, "knn_radii: k = %d outside 1..%d", k, KNN_MAX_K);
    if (exclude_self != 0 && exclude_self != 1) return cgs_set_error(CGS_EINVAL, "knn_radii: exclude_self = %d is neither 0 nor 1", exclude_self);
    if (exclude_self && other) return cgs_set_error(CGS_EINVAL, "knn_radii: exclude_self needs other == NULL (the pool against itself)");
    if (nref - exclude_self < k)
        return cgs_set_error(CGS_EINVAL, "knn_radii: %d candidates per row are fewer than k = %d", nref - exclude_self, k);
    if (!x || !out_r2) return cgs_set_error(CGS_EINVAL, "knn_radii: null x / out_r2");
    KnnParams p = {};
    p.qry = x; p.ref = other ? other : x; p.out_d = out_r2;
    p.m = n; p.n = nref; p.d = d; p.k = k; p.excl = exclude_self;
    return knn_launch<CGS_KNN_RADII>("knn_radii", pl, p, ws, ws_bytes, (hipStream_t)stream);
}

int cgs_ball_count(const float* qry, int m, const float* ref, int n, int d, const double* ref_r2, int* out_count, void* ws, size_t ws_bytes,
                   void* stream) {
    KnnPlan pl;
    if (!knn_plan(pl, m, n, d))
        return cgs_set_error(CGS_EINVAL, "ball_count: needs 1 <= d <= %d and 1 <= m, n <= 2^30 (m=%d n=%d d=%d)", KNN_MAX_D, m, n, d);
    if (!qry || !ref || !ref_r2 || !out_count) return cgs_set_error(CGS_EINVAL, "ball_count: null qry / ref / ref_r2 / out_count");
    KnnParams k = {};
    k.qry = qry; k.ref = ref; k.ref_r2 = ref_r2; k.out_i = out_count;
    k.m = m; k.n = n; k.d = d; k.k = 0; k.excl = 0;
    return knn_launch<CGS_KNN_BALL_COUNT>("ball_count", pl, k, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
