// Streaming first and second moments of a pool of feature vectors, in double (the Frechet statistics of metrics.PoolMoments):
//
//   a_i = (double)x[r_i] - (double)shift          sum[j] += sum_i a_ij          gram[j][k] += sum_i a_ij * a_ik
//
// x is fp32 [n][d]; r_i walks all n rows or a list of m row indices.  The Gram update is a rank-m update A^T A on the float64 matrix
// instruction v_mfma_f64_16x16x4_f64: every product and every sum is a double operation, so the error of an entry is the error of a
// double dot product of length m whatever the order (DESIGN.md section 18 derives the bound the tests assert).
//
// 1. moments_gram_kernel, grid (tile pairs, slabs).  The d columns are cut into T = ceil(d / 64) column tiles; only the P = T (T + 1) / 2
//    pairs (J <= K) are computed.  The samples are cut into slabs of `sps` samples (a multiple of the 32-sample tile; the last slab
//    may be short).  A block converts 32 samples x (64 + 64) columns to double, subtracts the shift and parks them in LDS -- rows past
//    the slab's end and columns past d are exact zeros from predicated loads, nothing outside x / rows / shift is read -- then its
//    four waves (2 x 2, a 32 x 32 quadrant each: four 16 x 16 accumulators) walk the 32 samples four at a time.  Operand layout of the
//    f64 instruction: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; both operands are the same LDS read
//    pattern on the J and the K panel.  Result: col = l & 15, row = (l >> 4) + 4 * reg  (NOT the f32 map).  The LDS rows are 80 doubles
//    apart: the 32 lanes a ds_read_b64 serves per cycle are two rows of 16 doubles, 160 dwords apart = 32 banks apart of 64.
//    The next sample tile is loaded to registers while the current one is multiplied.  The block leaves its 64 x 64 partial tile in the
//    workspace; blocks on the diagonal (J == K) leave the 64 column sums of their slab too.
// 2. moments_reduce_kernel, grid (P, 4): adds the slabs in ascending order, then adds the result to gram -- the tile and, through an
//    LDS transpose, its mirror from the same values; of a diagonal tile only the entries on or above the diagonal are used, so gram
//    stays exactly symmetric.  No atomics: a rerun is bit-identical.
//
// Also here: the spatial mean of an activation map [B][HW][C] -> [B][C] (the features of a conv discriminator, engine.score_with_features).
#include "cgs_internal.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- slab / tile plan (restated by tests/test_pool_moments_cpu.py) ----
#define MOM_TILE 64              // columns per tile
#define MOM_TS 32                // samples per LDS tile
#define MOM_BLOCKS 1024          // blocks aimed at: 4 per CU
#define MOM_MIN_SAMPLES 128      // at least this many samples per slab (a slab costs one partial tile set written and read back)
#define MOM_MAX_SLABS 32
#define MOM_MAX_D 2048
#define MOM_LDS_ROW 80           // doubles between two samples of a panel (64 + 16: see above)

struct MomPlan {
    int T, P;        // column tiles, tile pairs on or above the diagonal
    int sps, slabs;  // samples per slab, slabs
};

static bool mom_plan(MomPlan& p, long m, int d) {
    if (d < 1 || d > MOM_MAX_D || m < 0 || m > 0x40000000L) return false;          // (32-bit sample indices, slab ends included)
    p.T = cgs_ceil_div(d, MOM_TILE);
    p.P = p.T * (p.T + 1) / 2;
    if (m == 0) { p.sps = MOM_TS; p.slabs = 0; return true; }
    long slabs = cgs_ceil_div(MOM_BLOCKS, p.P);
    const long most = m / MOM_MIN_SAMPLES > 1 ? m / MOM_MIN_SAMPLES : 1;
    if (slabs > most) slabs = most;
    if (slabs > MOM_MAX_SLABS) slabs = MOM_MAX_SLABS;
    const long per = (m + slabs - 1) / slabs;
    const long sps = (per + MOM_TS - 1) / MOM_TS * MOM_TS;
    p.sps = (int)sps;
    p.slabs = (int)((m + sps - 1) / sps);
    return true;
}

static size_t mom_ws_doubles(const MomPlan& p) {
    return (size_t)p.slabs * ((size_t)p.P * MOM_TILE * MOM_TILE + (size_t)p.T * MOM_TILE);
}

struct MomParams {
    const float* x;      // [n][d]
    const int* rows;     // [m] or null
    const float* shift;  // [d] or null
    double* tiles;       // [slabs][P][64][64]
    double* sums;        // [slabs][T][64]
    int m, d, T, P, sps;
};

// pair index -> (J, K), J <= K, row-major over the upper triangle
__device__ __forceinline__ void mom_pair(int p, int T, int& J, int& K) {
    J = 0;
    while (p >= T - J) { p -= T - J; ++J; }
    K = J + p;
}

__global__ __launch_bounds__(256) void moments_gram_kernel(MomParams p) {
    __shared__ double lds[2][MOM_TS][MOM_LDS_ROW];
    int J, K;
    mom_pair(blockIdx.x, p.T, J, K);
    const bool diag = J == K;
    const int t = threadIdx.x;
    const int c = t & 63, rq = t >> 6;                              // loader: column c of both panels, samples rq, rq + 4, ...
    const int colJ = J * MOM_TILE + c, colK = K * MOM_TILE + c;
    const bool okJ = colJ < p.d, okK = !diag && colK < p.d;
    const double shJ = (okJ && p.shift) ? (double)p.shift[colJ] : 0.0;
    const double shK = (okK && p.shift) ? (double)p.shift[colK] : 0.0;
    const int i0 = blockIdx.y * p.sps;
    const int i1 = i0 + p.sps < p.m ? i0 + p.sps : p.m;             // (the last slab may be short)

    float vJ[MOM_TS / 4], vK[MOM_TS / 4];
    bool in[MOM_TS / 4];
    auto fetch = [&](int base) {
#pragma unroll
        for (int u = 0; u < MOM_TS / 4; ++u) {
            const int i = base + rq + 4 * u;
            in[u] = i < i1;
            vJ[u] = 0.f; vK[u] = 0.f;
            if (in[u]) {
                const size_t r = p.rows ? (size_t)p.rows[i] : (size_t)i;
                const float* xr = p.x + r * (size_t)p.d;
                if (okJ) vJ[u] = xr[colJ];
                if (okK) vK[u] = xr[colK];
            }
        }
    };

    const int lane = t & 63, wv = t >> 6;
    const int wr = wv >> 1, wc = wv & 1;                            // the wave's 32 x 32 quadrant of the 64 x 64 tile
    const int lr = lane >> 4, lc = lane & 15;
    const double (*pa)[MOM_LDS_ROW] = lds[0];
    const double (*pb)[MOM_LDS_ROW] = diag ? lds[0] : lds[1];
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;                                            // diagonal blocks: column c over the samples rq * 8 .. rq * 8 + 7 of every tile

    fetch(i0);
    for (int base = i0; base < i1; base += MOM_TS) {
#pragma unroll
        for (int u = 0; u < MOM_TS / 4; ++u) {                      // convert, THEN subtract, in double; rows past the end and columns past d: exact 0
            lds[0][rq + 4 * u][c] = (in[u] && okJ) ? (double)vJ[u] - shJ : 0.0;
            if (!diag) lds[1][rq + 4 * u][c] = (in[u] && okK) ? (double)vK[u] - shK : 0.0;
        }
        __syncthreads();
        if (base + MOM_TS < i1) fetch(base + MOM_TS);               // (block-uniform) in flight under the products below
        if (diag) {
#pragma unroll
            for (int u = 0; u < MOM_TS / 4; ++u) colsum += lds[0][rq * (MOM_TS / 4) + u][c];
        }
#pragma unroll
        for (int kk = 0; kk < MOM_TS / 4; ++kk) {
            const int i = 4 * kk + lr;
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = pa[i][32 * wr + 16 * a + lc];
#pragma unroll
            for (int b = 0; b < 2; ++b) bv[b] = pb[i][32 * wc + 16 * b + lc];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    double* tile = p.tiles + ((size_t)blockIdx.y * p.P + blockIdx.x) * (MOM_TILE * MOM_TILE);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e)                             // f64 result map: row = (lane >> 4) + 4 * reg, col = lane & 15
                tile[(32 * wr + 16 * a + lr + 4 * e) * MOM_TILE + 32 * wc + 16 * b + lc] = acc[a][b][e];
    if (diag) {                                                     // (block-uniform) the four sample quarters, added in quarter order
        lds[0][rq][c] = colsum;
        __syncthreads();
        if (rq == 0)
            p.sums[((size_t)blockIdx.y * p.T + J) * MOM_TILE + c] = ((lds[0][0][c] + lds[0][1][c]) + lds[0][2][c]) + lds[0][3][c];
    }
}

// grid (P, 4): block (pair, strip) owns rows strip * 16 .. + 15 of the pair's 64 x 64 tile
__global__ __launch_bounds__(256) void moments_reduce_kernel(const double* __restrict__ tiles, const double* __restrict__ sums, double* __restrict__ sum,
                                                             double* __restrict__ gram, int d, int T, int P, int slabs) {
    __shared__ double tr[16][MOM_TILE + 1];
    int J, K;
    mom_pair(blockIdx.x, T, J, K);
    const bool diag = J == K;
    const int t = threadIdx.x, strip = blockIdx.y;
    const int c = t & 63, rq = t >> 6;
    const size_t slab_stride = (size_t)P * MOM_TILE * MOM_TILE;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int rl = pass * 4 + rq, r = strip * 16 + rl;
        const double* src = tiles + (size_t)blockIdx.x * (MOM_TILE * MOM_TILE) + r * MOM_TILE + c;
        double v = 0.0;
        for (int z = 0; z < slabs; ++z) v += src[z * slab_stride];   // ascending slab order
        tr[rl][c] = v;
        const int j = J * MOM_TILE + r, k = K * MOM_TILE + c;
        if (j < d && k < d && (!diag || r <= c)) gram[(size_t)j * d + k] += v;
    }
    __syncthreads();
    const int rl = t & 15, cq = t >> 4;                              // the mirror: gram[k][j], 16 consecutive j per 16 lanes
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int cc = pass * 16 + cq, r = strip * 16 + rl;
        const int j = J * MOM_TILE + r, k = K * MOM_TILE + cc;
        if (j < d && k < d && (!diag || r < cc)) gram[(size_t)k * d + j] += tr[rl][cc];
    }
    if (diag && strip == 0 && t < MOM_TILE) {
        const int j = J * MOM_TILE + t;
        if (j < d) {
            double v = 0.0;
            for (int z = 0; z < slabs; ++z) v += sums[((size_t)z * T + J) * MOM_TILE + t];
            sum[j] += v;
        }
    }
}

// out[b][c] = mean over the HW pixels of x[b][.][c]: the four pixel quarters of a block in double, ascending, added in quarter order
__global__ __launch_bounds__(256) void spatial_mean_kernel(const float* __restrict__ x, float* __restrict__ out, int HW, int C) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int per = (HW + 3) / 4;
    const int h0 = q * per, h1 = h0 + per < HW ? h0 + per : HW;
    double s = 0.0;
    if (c < C)
        for (int h = h0; h < h1; ++h) s += (double)x[((size_t)b * HW + h) * C + c];
    part[q][lane] = s;
    __syncthreads();
    if (q == 0 && c < C) out[(size_t)b * C + c] = (float)((((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (double)HW);
}

extern "C" {

size_t cgs_pool_moments_ws_bytes(int m, int d) {
    MomPlan p;
    if (!mom_plan(p, m, d)) return 0;
    return mom_ws_doubles(p) * sizeof(double);
}

int cgs_pool_moments_accumulate(const float* x, int n, int d, const int* rows, int m, const float* shift, double* sum, double* gram, void* ws,
                                size_t ws_bytes, void* stream) {
    MomPlan p;
    const long count = rows ? m : n;
    if (n < 0 || m < 0 || !mom_plan(p, count, d) || (size_t)n * (size_t)d * sizeof(float) >= 0x80000000UL)
        return cgs_set_error(CGS_EINVAL, "pool_moments_accumulate: needs 1 <= d <= %d, n >= 0, m >= 0 and x below 2 GiB (n=%d d=%d m=%d)", MOM_MAX_D, n, d, m);
    if (count == 0) return CGS_OK;
    if (!x || !sum || !gram) return cgs_set_error(CGS_EINVAL, "pool_moments_accumulate: null x / sum / gram");
    const size_t need = mom_ws_doubles(p) * sizeof(double);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "pool_moments_accumulate: workspace %zu < %zu bytes", ws_bytes, need);
    if ((uintptr_t)ws & 7) return cgs_set_error(CGS_EINVAL, "pool_moments_accumulate: the workspace must be 8-byte aligned");
    MomParams k;
    k.x = x; k.rows = rows; k.shift = shift;
    k.tiles = (double*)ws;
    k.sums = k.tiles + (size_t)p.slabs * p.P * MOM_TILE * MOM_TILE;
    k.m = (int)count; k.d = d; k.T = p.T; k.P = p.P; k.sps = p.sps;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(moments_gram_kernel, dim3(p.P, p.slabs), dim3(256), 0, s, k);
    CGS_CHECK_LAUNCH("pool_moments_accumulate");
    hipLaunchKernelGGL(moments_reduce_kernel, dim3(p.P, 4), dim3(256), 0, s, k.tiles, k.sums, sum, gram, d, p.T, p.P, p.slabs);
    CGS_CHECK_LAUNCH("pool_moments_accumulate");
    return CGS_OK;
}

int cgs_spatial_mean(const float* x, float* out, int B, int HW, int C, void* stream) {
    if (!x || !out || B <= 0 || HW <= 0 || C <= 0 || B > 65535 || (long)B * HW * C * 4 > 0x7fffffffL)
        return cgs_set_error(CGS_EINVAL, "spatial_mean: bad argument (B=%d HW=%d C=%d)", B, HW, C);
    hipLaunchKernelGGL(spatial_mean_kernel, dim3(cgs_ceil_div(C, 64), B), dim3(256), 0, (hipStream_t)stream, x, out, HW, C);
    CGS_CHECK_LAUNCH("spatial_mean");
    return CGS_OK;
}

}  // extern "C"
