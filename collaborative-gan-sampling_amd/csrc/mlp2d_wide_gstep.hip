// The G step of the 2-D generator at 64 < nhidden <= 256 (synthetic/GAN.py:83-101 at the reference's --nhidden=256 --nlayers=6): the function
// of cgs_mlp2d_g_step of mlp2d.hip -- a training-mode forward on z, tf.gradients(generates, g_vars, grad_plugin) for every g_fc kernel and
// bias back through the training-mode batch norm, then w <- w - lr * g -- on the sample tiles of mlp2d_wide.h.
//
// The forward is cgs_mlp2d_wide_gen_fwd itself on the first bytes of the workspace (mlp2d_wide_gen.hip): it leaves every BN layer's
// pre-activations pre [nl-1][B][nhp] and the (mean, rstd) rows.  The batch couples every sample at every BN layer on the way back too
// (FusedBatchNormGrad needs mean(dxhat) and mean(dxhat xhat) over the batch), so a launch per BN layer is the grid-wide barrier:
//   top launch          dh_{nl-2} = grad_plugin W_last^T                        VALU;  epilogue for layer nl-2
//   launch u = nl-2..1  da_u = rstd (dxhat_u - mean(dxhat_u) - xhat_u mean(dxhat_u xhat_u)), stored;
//                       dh_{u-1} = da_u W_u^T                                   mlpw_pass<T, true, true>;  epilogue for layer u-1
//   first-layer launch  da_0 from dxhat_0                                       elementwise
//   weight gradients    dW_l = h_{l-1}^T da_l, 1 <= l <= nl-2                   v_mfma_f32_32x32x2_f32 over sample chunks (section 12's pass B);
//                       dW_0, dW_last, every db                                 VALU chunk sums in ascending sample order
//   update              every gradient element = its chunk partials added in chunk order; gw / gb written, w <- w - lr * g
// One workgroup of 4 waves per tile of T = mlpw_tile(B) samples in the first three kinds of launch.
//
// Epilogue for layer l (H holds dh_l): xhat = (a - mean) rstd and the ReLU decision gamma xhat + beta > 0 are recomputed from pre and stats
// with genw_bn_relu's own statements, so a mask never disagrees with the forward's; dxhat = decision ? dh gamma : 0 goes to dbuf
// [nl-1][B][nhp] in natural unit order (padded units: exact zeros; rows past B: not stored), and every group of 32 consecutive rows leaves
// (sum dxhat, sum dxhat xhat) per unit, one thread per (group, unit) walking the rows in ascending order: the forward's groups.
// Launch u adds the ceil(B / 32) partials of layer u in ascending group order, one unit per thread, and overwrites dxhat_u with da_u in place.
//
// Centring.  xhat as the forward formed it does not sum to zero over the batch: the forward's mean is Chan's combine of ceil(B / 32) group
// means, a chain whose rounding leaves mean(xhat) = e of the order of 1e-5 .. 1e-4 at B = 8200, and da would carry -e mean(dxhat xhat) in
// every sample: B times that in db, and that times any common offset of h in dW.  The group walk therefore leaves sum xhat as well, and
// da is formed with xhat - e and with mean(dxhat xhat) - e mean(dxhat), which is mean(dxhat (xhat - e)).  The ReLU decision and h keep the
// forward's xhat.
//
// h_{l-1} = relu(BN(a_{l-1})) is NOT stored: the weight-gradient launch recomputes it on load from pre and stats (a lane's column is fixed,
// so mean, rstd, gamma, beta are four registers per column), again with genw_bn_relu's statements.
//
// Determinism: groups of 32 rows and chunks of mlpw_chunk(B) samples are functions of B alone; every sum walks its terms in ascending
// order; the MFMA chains are k-ordered.  So every output is a function of the inputs and B alone, not of T or of the CU count.  No atomics.
//
// Workspace (floats), H = nlayers - 1, G = ceil(B / 32):
//   the forward's own  4 H nhp (B + 2 G + 2) bytes: pre | part | stats
//   dbuf  [H][B][nhp]      dxhat, then da
//   bpart [H][G][3][nhp]   (sum dxhat, sum dxhat xhat, sum xhat) of the row groups
//   xs    [B][2]           G(z) when the caller passes no x
//   pw    [nl-2][16][nhp][nhp]   partial dW of the hidden -> hidden layers, [layer][chunk]
//   ps    [16][H nhp (db_l) + 2 nhp (dW_0) + 2 nhp (dW_last, by column) + 4 (db_last, 0, 0)]
#include "mlp2d_wide.h"

#define GSW_PBATCH 16           // partials fetched per round trip, as GENW_PBATCH

// Compensated (Kahan) running sum, terms taken in the order given: the order stays ascending, so the result is still a function of the
// inputs alone, and its rounding error no longer grows with the number of terms.  The sums it is used for cancel in exact arithmetic
// (mean(dxhat) is subtracted from every dxhat; db of a BN-fed bias is zero), so their rounding is what is left of them.
struct GswSum {
    float s = 0.f, c = 0.f;
    __device__ __forceinline__ void add(float x) {
        const float y = x - c, t = s + y;
        c = (t - s) - y;
        s = t;
    }
};

struct GswLayer {
    // the BN layer whose dxhat the epilogue forms (top and layer launches)
    const float* pre_l; const float* stats_l; const float* gamma_l; const float* beta_l; float* dbuf_l; float* bpart_l;
    // the BN layer u above it (layer launches and the first-layer launch)
    const float* pre_u; const float* stats_u; const float* bpart_u; float* dbuf_u;
    const float* w_up;                                 // W_last [nh][2] (top) or W_u [nh][nh]
    const float* gplug;                                // top: [B][2]
    int nh, nhp, B;
};

struct GswLds {
    float* H;          // [T][nhp + 4], unit j at position hpos(j)
    float* slab;       // [2][nhp][T/2], mlpw_pass's; the epilogue keeps xhat [T][nhp] (natural order) there
    float* bn;         // [4][nhp]: mean, rstd, gamma, beta of layer l, unit j at index j
    float* up;         // [5][nhp]: mean, rstd, mean(dxhat), mean(dxhat (xhat - e)), e = mean(xhat) of layer u; the top launch: the two
                       // columns of W_last
    float* gp;         // [T][2]: the tile's grad_plugin
};

template <int T>
__device__ __forceinline__ GswLds gsw_lds(float* smem, int nhp) {
    GswLds L;
    L.H = smem;
    L.slab = L.H + T * (nhp + 4);
    L.bn = L.slab + 2 * nhp * (T / 2);
    L.up = L.bn + 4 * nhp;
    L.gp = L.up + 5 * nhp;
    return L;
}

// nh = 256: T = 64: 138.5 KiB (one block per CU); T = 32: 73.8 KiB (two)
static size_t gsw_smem(int T, int nhp) { return (size_t)(T * (nhp + 4) + 2 * nhp * (T / 2) + 9 * nhp + 2 * T) * sizeof(float); }

// thread j < nhp: (mean, rstd, gamma, beta) of unit j of layer l; padded units: zeros (there is no gamma or beta to read there)
__device__ __forceinline__ void gsw_load_bn(const GswLayer& a, float* bn) {
    const int j = threadIdx.x, nh = a.nh, nhp = a.nhp;
    if (j >= nhp) return;
    const bool in = j < nh;
    bn[j] = in ? a.stats_l[j] : 0.f;
    bn[nhp + j] = in ? a.stats_l[nhp + j] : 0.f;
    bn[2 * nhp + j] = in ? a.gamma_l[j] : 0.f;
    bn[3 * nhp + j] = in ? a.beta_l[j] : 0.f;
}

// thread j < nhp: (mean, rstd, mean(dxhat), mean(dxhat (xhat - e)), e) of unit j of layer u, the three batch means from the partials of its
// row groups added in ascending group order
__device__ __forceinline__ void gsw_load_up(const GswLayer& a, float* up) {
    const int j = threadIdx.x, nh = a.nh, nhp = a.nhp;
    if (j >= nhp) return;
    float mean = 0.f, rstd = 0.f, c1 = 0.f, c2 = 0.f, ex = 0.f;
    if (j < nh) {
        const int G = (a.B + 31) >> 5;
        GswSum s1, s2, s3;
        for (int p0 = 0; p0 < G; p0 += GSW_PBATCH) {
            float p1[GSW_PBATCH], p2[GSW_PBATCH], p3[GSW_PBATCH];
#pragma unroll
            for (int q = 0; q < GSW_PBATCH; ++q) {
                const bool in = p0 + q < G;
                p1[q] = in ? a.bpart_u[(size_t)(p0 + q) * 3 * nhp + j] : 0.f;
                p2[q] = in ? a.bpart_u[(size_t)(p0 + q) * 3 * nhp + nhp + j] : 0.f;
                p3[q] = in ? a.bpart_u[(size_t)(p0 + q) * 3 * nhp + 2 * nhp + j] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < GSW_PBATCH; ++q)
                if (p0 + q < G) { s1.add(p1[q]); s2.add(p2[q]); s3.add(p3[q]); }
        }
        c1 = s1.s / (float)a.B; ex = s3.s / (float)a.B; c2 = s2.s / (float)a.B - ex * c1;
        mean = a.stats_u[j]; rstd = a.stats_u[nhp + j];
    }
    up[j] = mean; up[nhp + j] = rstd; up[2 * nhp + j] = c1; up[3 * nhp + j] = c2; up[4 * nhp + j] = ex;
}

// tf FusedBatchNormGrad, training: da = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), xhat the forward's, centred (see the top)
__device__ __forceinline__ float gsw_da(float a, float dx, const float* up, int nhp, int j) {
    const float ru = up[nhp + j], xh = (a - up[j]) * ru;
    return ru * (dx - up[2 * nhp + j] - (xh - up[4 * nhp + j]) * up[3 * nhp + j]);
}

// H <- da_u of the tile's rows (rows past B and padded units: 0); da_u replaces dxhat_u in dbuf
template <int T>
__device__ __forceinline__ void gsw_fill_da(const GswLayer& a, const GswLds& L, int row0, int rows) {
    const int nh = a.nh, nhp = a.nhp, HS = nhp + 4;
    for (int e = threadIdx.x; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        float da = 0.f;
        if (row < rows && j < nh) {
            const size_t o = (size_t)(row0 + row) * nhp + j;
            da = gsw_da(a.pre_u[o], a.dbuf_u[o], L.up, nhp, j);
            a.dbuf_u[o] = da;
        }
        L.H[row * HS + hpos(j)] = da;
    }
}

// H holds dh_l of the tile: dxhat_l -> dbuf (rows below B; padded units exact zeros) and the two sums of each 32-row group with a row below B
template <int T>
__device__ __forceinline__ void gsw_epilogue(const GswLayer& a, const GswLds& L, int row0, int rows) {
    const int nh = a.nh, nhp = a.nhp, HS = nhp + 4;
    float* X = L.slab;
    for (int e = threadIdx.x; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        float* hp = &L.H[row * HS + hpos(j)];
        float dx = 0.f, xh = 0.f;
        if (row < rows && j < nh) {
            xh = (a.pre_l[(size_t)(row0 + row) * nhp + j] - L.bn[j]) * L.bn[nhp + j];             // genw_bn_relu's statements
            dx = fmaf(xh, L.bn[2 * nhp + j], L.bn[3 * nhp + j]) > 0.f ? *hp * L.bn[2 * nhp + j] : 0.f;
        }
        *hp = dx; X[row * nhp + j] = xh;
        if (row < rows) a.dbuf_l[(size_t)(row0 + row) * nhp + j] = dx;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < (T / 32) * nhp; t += MLPW_THREADS) {
        const int g = t / nhp, j = t - g * nhp, n = min(32, rows - 32 * g);
        if (n <= 0) continue;
        const float* col = L.H + 32 * g * HS + hpos(j);
        const float* xc = X + 32 * g * nhp + j;
        GswSum s1, s2, s3;
        for (int r = 0; r < n; ++r) { const float dx = col[r * HS], xh = xc[r * nhp]; s1.add(dx); s2.add(dx * xh); s3.add(xh); }
        float* P = a.bpart_l + (size_t)(row0 / 32 + g) * 3 * nhp;
        P[j] = s1.s; P[nhp + j] = s2.s; P[2 * nhp + j] = s3.s;
    }
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void gsw_top_kernel(GswLayer a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GswLds L = gsw_lds<T>(smem, a.nhp);
    const int tid = threadIdx.x, nh = a.nh, nhp = a.nhp, HS = nhp + 4;
    const int row0 = blockIdx.x * T, rows = min(T, a.B - row0);
    gsw_load_bn(a, L.bn);
    if (tid < nhp) {
        L.up[tid] = tid < nh ? a.w_up[2 * tid] : 0.f;
        L.up[nhp + tid] = tid < nh ? a.w_up[2 * tid + 1] : 0.f;
    }
    if (tid < 2 * T) L.gp[tid] = (tid >> 1) < rows ? a.gplug[2 * (size_t)row0 + tid] : 0.f;
    __syncthreads();
    for (int e = tid; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        L.H[row * HS + hpos(j)] = fmaf(L.gp[2 * row + 1], L.up[nhp + j], L.gp[2 * row] * L.up[j]);
    }
    __syncthreads();
    gsw_epilogue<T>(a, L, row0, rows);
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void gsw_layer_kernel(GswLayer a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GswLds L = gsw_lds<T>(smem, a.nhp);
    const int row0 = blockIdx.x * T, rows = min(T, a.B - row0);
    gsw_load_up(a, L.up);
    gsw_load_bn(a, L.bn);
    __syncthreads();
    gsw_fill_da<T>(a, L, row0, rows);
    __syncthreads();
    MlpWParams p = {};
    p.nh = a.nh; p.nhp = a.nhp;
    MlpWLds M = {};
    M.H = L.H; M.slab = L.slab;
    mlpw_pass<T, true, true>(p, M, a.w_up, nullptr, 0);
    gsw_epilogue<T>(a, L, row0, rows);
}

// dxhat_0 -> da_0 in place, 64 rows per workgroup
__global__ __launch_bounds__(MLPW_THREADS) void gsw_first_kernel(GswLayer a) {
    __shared__ float up[5 * 256];
    const int nh = a.nh, nhp = a.nhp;
    const int row0 = blockIdx.x * 64, rows = min(64, a.B - row0);
    gsw_load_up(a, up);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        if (j >= nh) continue;                          // padded units stay the exact zeros the epilogue stored
        const size_t o = (size_t)(row0 + row) * nhp + j;
        a.dbuf_u[o] = gsw_da(a.pre_u[o], a.dbuf_u[o], up, nhp, j);
    }
}

struct GswGrad {
    const float* pre; const float* stats; const float* dbuf;        // [H][B][nhp], [H][2][nhp], [H][B][nhp] (da)
    const float* gamma[MLPW_MAX_LAYERS - 1]; const float* beta[MLPW_MAX_LAYERS - 1];
    const float* z; const float* gplug;
    float* pw; float* ps;
    int nlayers, nh, nhp, B, chunk, nchunks, sstride;
};

// blocks [0, nmfma): 4 waves, wave task t = 4 block + wave -> (hidden -> hidden layer, chunk, 64 x 64 block of dW): mlpw_wgrad_kernel's
// product with the A fragment recomputed, h = relu(BN(a)), from the pre-activations.
// blocks [nmfma, nmfma + nchunks (nl-1)): (chunk, BN layer l): thread j < nhp sums column j of da_l over the chunk (db_l); l = 0 adds
// z^T da_0; l = nl-2 adds h_{nl-2}^T grad_plugin and, in threads 0 and 1, the column sums of grad_plugin (db_last).
__global__ __launch_bounds__(MLPW_THREADS) void gsw_wgrad_kernel(GswGrad q, int nmfma) {
    const int tid = threadIdx.x, B = q.B, nh = q.nh, nhp = q.nhp, nhid = q.nlayers - 1;
    const size_t lstride = (size_t)B * nhp;
    if ((int)blockIdx.x < nmfma) {
        const int NB = nhp >> 5, NB2 = (NB + 1) >> 1, per = NB2 * NB2;
        const int lane = tid & 63, h = lane >> 5, c31 = lane & 31;
        const int t = blockIdx.x * 4 + (tid >> 6);
        if (t >= (q.nlayers - 2) * q.nchunks * per) return;
        const int lc = t / per, blk = t - lc * per, hl = lc / q.nchunks, c = lc - hl * q.nchunks;       // hl = 0: dW of layer 1
        const int ti = 2 * (blk / NB2), tj = 2 * (blk % NB2);
        const bool i1 = ti + 1 < NB, j1 = tj + 1 < NB;
        const int s0 = c * q.chunk, s1 = min(B, s0 + q.chunk);
        const int col = ti * 32 + c31;
        const float* A = q.pre + hl * lstride + col;
        const float* D = q.dbuf + (hl + 1) * lstride + tj * 32 + c31;
        const float* S = q.stats + (size_t)hl * 2 * nhp;
        const bool in0 = col < nh, in1 = i1 && col + 32 < nh;
        const float m0 = in0 ? S[col] : 0.f, r0 = in0 ? S[nhp + col] : 0.f, g0 = in0 ? q.gamma[hl][col] : 0.f, e0 = in0 ? q.beta[hl][col] : 0.f;
        const float m1 = in1 ? S[col + 32] : 0.f, r1 = in1 ? S[nhp + col + 32] : 0.f, g1 = in1 ? q.gamma[hl][col + 32] : 0.f,
                    e1 = in1 ? q.beta[hl][col + 32] : 0.f;
        mlpw_f16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
#pragma unroll 1
        for (int s = s0; s < s1; s += 8) {                                  // 4 MFMA steps of 2 samples; the chunk size is a multiple of 8
            float a0[4], a1[4], b0[4], b1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                                   // rows past the chunk's end (the last chunk's past B) enter as zero
                const int ss = s + 2 * u + h;
                const bool ok = ss < s1;
                const size_t o = (size_t)ss * nhp;
                a0[u] = (ok && in0) ? fmaxf(fmaf((A[o] - m0) * r0, g0, e0), 0.f) : 0.f;
                a1[u] = (ok && in1) ? fmaxf(fmaf((A[o + 32] - m1) * r1, g1, e1), 0.f) : 0.f;
                b0[u] = ok ? D[o] : 0.f; b1[u] = (ok && j1) ? D[o + 32] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b0[u], acc[0][0], 0, 0, 0);
                if (j1) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b1[u], acc[0][1], 0, 0, 0);
                if (i1) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], b0[u], acc[1][0], 0, 0, 0);
                if (i1 && j1) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], b1[u], acc[1][1], 0, 0, 0);
            }
        }
        float* P = q.pw + (size_t)lc * nhp * nhp;                           // [layer][chunk][nhp][nhp]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if ((a && !i1) || (b && !j1)) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r)     // accumulator element r of lane (h, c31): row (r & 3) + 8 (r >> 2) + 4 h, column c31
                    P[(size_t)((ti + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * nhp + (tj + b) * 32 + c31] = acc[a][b][r];
            }
        return;
    }
    const int sb = blockIdx.x - nmfma, c = sb / nhid, l = sb - c * nhid;
    const int s0 = c * q.chunk, s1 = min(B, s0 + q.chunk);
    float* S = q.ps + (size_t)c * q.sstride;
    if (tid < nhp) {
        // 16 samples' loads in flight, then their terms added in ascending sample order (the chunk size is a multiple of 16; rows past the
        // chunk's end add an exact zero)
        const float* D = q.dbuf + l * lstride + tid;
        GswSum db;
        float g0 = 0.f, g1 = 0.f;
#pragma unroll 1
        for (int s = s0; s < s1; s += 16) {
            float d[16], x0[16], x1[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int ss = s + u;
                const bool ok = ss < s1;
                d[u] = ok ? D[(size_t)ss * nhp] : 0.f;
                x0[u] = x1[u] = 0.f;
                if (ok && l == 0) { x0[u] = q.z[2 * (size_t)ss]; x1[u] = q.z[2 * (size_t)ss + 1]; }
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) { db.add(d[u]); g0 = fmaf(x0[u], d[u], g0); g1 = fmaf(x1[u], d[u], g1); }
        }
        S[l * nhp + tid] = db.s;
        if (l == 0) { S[nhid * nhp + tid] = g0; S[(nhid + 1) * nhp + tid] = g1; }
        if (l == nhid - 1) {
            const bool in = tid < nh;
            const float* A = q.pre + l * lstride + tid;
            const float* St = q.stats + (size_t)l * 2 * nhp;
            const float m = in ? St[tid] : 0.f, r = in ? St[nhp + tid] : 0.f, ga = in ? q.gamma[l][tid] : 0.f, be = in ? q.beta[l][tid] : 0.f;
            float w0 = 0.f, w1 = 0.f;
#pragma unroll 1
            for (int s = s0; s < s1; s += 16) {
                float a[16], p0[16], p1[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int ss = s + u;
                    const bool ok = ss < s1;
                    a[u] = (ok && in) ? fmaxf(fmaf((A[(size_t)ss * nhp] - m) * r, ga, be), 0.f) : 0.f;
                    p0[u] = ok ? q.gplug[2 * (size_t)ss] : 0.f;
                    p1[u] = ok ? q.gplug[2 * (size_t)ss + 1] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) { w0 = fmaf(a[u], p0[u], w0); w1 = fmaf(a[u], p1[u], w1); }
            }
            S[(nhid + 2) * nhp + tid] = w0; S[(nhid + 3) * nhp + tid] = w1;
        }
    }
    if (l == nhid - 1 && tid < 2) {
        float a = 0.f;
        for (int s = s0; s < s1; ++s) a += q.gplug[2 * (size_t)s + tid];
        S[(nhid + 4) * nhp + tid] = a;
    }
}

struct GswPtrs {
    float* w[MLPW_MAX_LAYERS];
    float* b[MLPW_MAX_LAYERS];
    float* gw[MLPW_MAX_LAYERS];      // may be null
    float* gb[MLPW_MAX_LAYERS];
};

// element e of [hidden -> hidden dW: (nl-2) nh nh | dW_0: 2 nh | dW_last: 2 nh | db_l: (nl-1) nh | db_last: 2]
__global__ __launch_bounds__(256) void gsw_update_kernel(GswPtrs q, const float* __restrict__ pw, const float* __restrict__ ps, int nchunks, int sstride,
                                                         int nlayers, int nh, int nhp, float lr) {
    const int nhid = nlayers - 1, nhh = nh * nh, nbig = (nlayers - 2) * nhh, total = nbig + (nhid + 4) * nh + 2;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
#pragma clang fp contract(off)      // var -= lr * grad as two roundings (GradientDescentOptimizer's ApplyGradientDescent)
        const float* P;
        size_t stride;
        float *wv, *gv;
        if (e < nbig) {
            const int hl = e / nhh, r = e - hl * nhh, i = r / nh, j = r - i * nh;
            stride = (size_t)nhp * nhp;
            P = pw + (size_t)hl * nchunks * stride + (size_t)i * nhp + j;
            wv = q.w[hl + 1] + r; gv = q.gw[hl + 1] ? q.gw[hl + 1] + r : nullptr;
        } else {
            int r = e - nbig;
            stride = sstride;
            if (r < 2 * nh) {                                   // dW_0 [2][nh]
                P = ps + (nhid + r / nh) * nhp + r % nh;
                wv = q.w[0] + r; gv = q.gw[0] ? q.gw[0] + r : nullptr;
            } else if ((r -= 2 * nh) < 2 * nh) {                // dW_last [nh][2]
                P = ps + (nhid + 2 + (r & 1)) * nhp + (r >> 1);
                wv = q.w[nhid] + r; gv = q.gw[nhid] ? q.gw[nhid] + r : nullptr;
            } else if ((r -= 2 * nh) < nhid * nh) {             // db_l [nh]
                const int l = r / nh, j = r - l * nh;
                P = ps + l * nhp + j;
                wv = q.b[l] + j; gv = q.gb[l] ? q.gb[l] + j : nullptr;
            } else {                                            // db_last [2]
                r -= nhid * nh;
                P = ps + (nhid + 4) * nhp + r;
                wv = q.b[nhid] + r; gv = q.gb[nhid] ? q.gb[nhid] + r : nullptr;
            }
        }
        float g = 0.f;
        for (int c = 0; c < nchunks; ++c) g += P[c * stride];
        if (gv) *gv = g;
        if (lr != 0.f) *wv = *wv - lr * g;
    }
}

static size_t gsw_fwd_floats(int B, int nlayers, int nhp) {          // genw_ws_floats of mlp2d_wide_gen.hip
    return (size_t)(nlayers - 1) * nhp * ((size_t)B + 2 * (size_t)cgs_ceil_div(B, 32) + 2);
}

static int gsw_sstride(int nlayers, int nhp) { return (nlayers + 3) * nhp + 4; }

static size_t gsw_ws_floats(int B, int nlayers, int nhp) {
    const size_t H = nlayers - 1, G = cgs_ceil_div(B, 32);
    return gsw_fwd_floats(B, nlayers, nhp) + H * B * nhp + H * G * 3 * nhp + 2 * (size_t)B +
           (size_t)MLPW_MAX_CHUNKS * ((size_t)(nlayers - 2) * nhp * nhp + gsw_sstride(nlayers, nhp));
}

template <int T>
static int gsw_tile_launch(const GswLayer& a, bool top, hipStream_t st) {
    const size_t smem = gsw_smem(T, a.nhp);
    const dim3 grid(cgs_ceil_div(a.B, T)), block(MLPW_THREADS);
    if (top) {
        CGS_SMEM_ATTR(160 * 1024, "mlp2d_wide_g_step", gsw_top_kernel<T>);
        hipLaunchKernelGGL(gsw_top_kernel<T>, grid, block, smem, st, a);
    } else {
        CGS_SMEM_ATTR(160 * 1024, "mlp2d_wide_g_step", gsw_layer_kernel<T>);
        hipLaunchKernelGGL(gsw_layer_kernel<T>, grid, block, smem, st, a);
    }
    CGS_CHECK_LAUNCH("mlp2d_wide_g_step");
    return CGS_OK;
}

static bool gsw_shape_ok(int nlayers, int nhidden) { return nlayers >= 2 && nlayers <= MLPW_MAX_LAYERS && nhidden >= 65 && nhidden <= 256; }

extern "C" {

size_t cgs_mlp2d_wide_g_step_ws_bytes(int B, int nlayers, int nhidden) {
    if (B <= 0 || B > (1 << 24) || !gsw_shape_ok(nlayers, nhidden)) return 0;
    return gsw_ws_floats(B, nlayers, cgs_round_up(nhidden, 32)) * sizeof(float);
}

int cgs_mlp2d_wide_g_step(float* const* w, float* const* b, const float* const* gamma, const float* const* beta, float* const* moving_mean,
                          float* const* moving_variance, int nlayers, int nhidden, const float* z, const float* grad_plugin, int B, float eps,
                          float lr, float* const* gw, float* const* gb, float* x, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mlp2d_wide_g_step";
    // the checks of cgs_mlp2d_g_step, in its order: shape, weights, grad_plugin, batch-norm variables, batch, workspace
    if (!gsw_shape_ok(nlayers, nhidden)) return cgs_set_error(CGS_EINVAL, "%s: nlayers=%d nhidden=%d (need 2..6, 65..256)", who, nlayers, nhidden);
    if (!w || !b) return cgs_set_error(CGS_EINVAL, "%s: null weight array", who);
    for (int l = 0; l < nlayers; ++l)
        if (!w[l] || !b[l]) return cgs_set_error(CGS_EINVAL, "%s: null weight", who);
    if (!grad_plugin) return cgs_set_error(CGS_EINVAL, "%s: null grad_plugin", who);
    if (!gamma || !beta || !moving_mean || !moving_variance) return cgs_set_error(CGS_EINVAL, "%s: null batch-norm array", who);
    for (int l = 0; l < nlayers - 1; ++l)
        if (!gamma[l] || !beta[l] || !moving_mean[l] || !moving_variance[l]) return cgs_set_error(CGS_EINVAL, "%s: null batch-norm variable", who);
    if (!z || B < 2 || B > (1 << 24) || !(eps > 0.f)) return cgs_set_error(CGS_EINVAL, "%s: bad argument (B=%d, training=1)", who, B);
    const int nl = nlayers, nhp = cgs_round_up(nhidden, 32), H = nl - 1, G = cgs_ceil_div(B, 32);
    const size_t need = gsw_ws_floats(B, nl, nhp) * sizeof(float);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const size_t lstride = (size_t)B * nhp, pstride = (size_t)G * 2 * nhp, bstride = (size_t)G * 3 * nhp;
    float* pre = (float*)ws;
    float* stats = pre + H * lstride + H * pstride;
    float* dbuf = pre + gsw_fwd_floats(B, nl, nhp);
    float* bpart = dbuf + H * lstride;
    float* xs = bpart + H * bstride;
    float* pw = xs + 2 * (size_t)B;
    float* ps = pw + (size_t)MLPW_MAX_CHUNKS * (nl - 2) * nhp * nhp;
    int rc = cgs_mlp2d_wide_gen_fwd((const float* const*)w, (const float* const*)b, gamma, beta, moving_mean, moving_variance, nl, nhidden, z,
                                    x ? x : xs, B, 1, eps, nullptr, ws, gsw_fwd_floats(B, nl, nhp) * sizeof(float), stream);
    if (rc) return rc;
    const int T = mlpw_tile(B);
    // top: output -> layer nl-2; then layer u -> u-1 for u = nl-2 .. 1; then layer 0 alone (its da)
    for (int u = nl - 1; u >= 0; --u) {
        GswLayer a = {};
        a.w_up = w[u];
        if (u == nl - 1) a.gplug = grad_plugin;
        else {
            a.pre_u = pre + u * lstride; a.stats_u = stats + (size_t)u * 2 * nhp; a.bpart_u = bpart + u * bstride; a.dbuf_u = dbuf + u * lstride;
        }
        if (u > 0) {
            const int l = u - 1;
            a.pre_l = pre + l * lstride; a.stats_l = stats + (size_t)l * 2 * nhp; a.gamma_l = gamma[l]; a.beta_l = beta[l];
            a.dbuf_l = dbuf + l * lstride; a.bpart_l = bpart + l * bstride;
        }
        a.nh = nhidden; a.nhp = nhp; a.B = B;
        if (u > 0) {
            rc = T == 32 ? gsw_tile_launch<32>(a, u == nl - 1, st) : gsw_tile_launch<64>(a, u == nl - 1, st);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(gsw_first_kernel, dim3(cgs_ceil_div(B, 64)), dim3(MLPW_THREADS), 0, st, a);
            CGS_CHECK_LAUNCH("mlp2d_wide_g_step");
        }
    }
    GswGrad q = {};
    q.pre = pre; q.stats = stats; q.dbuf = dbuf;
    for (int l = 0; l < H; ++l) { q.gamma[l] = gamma[l]; q.beta[l] = beta[l]; }
    q.z = z; q.gplug = grad_plugin; q.pw = pw; q.ps = ps;
    q.nlayers = nl; q.nh = nhidden; q.nhp = nhp; q.B = B;
    q.chunk = mlpw_chunk(B); q.nchunks = cgs_ceil_div(B, q.chunk); q.sstride = gsw_sstride(nl, nhp);
    const int NB2 = (nhp / 32 + 1) / 2, nmfma = cgs_ceil_div((nl - 2) * q.nchunks * NB2 * NB2, 4);
    hipLaunchKernelGGL(gsw_wgrad_kernel, dim3(nmfma + q.nchunks * H), dim3(MLPW_THREADS), 0, st, q, nmfma);
    CGS_CHECK_LAUNCH("mlp2d_wide_g_step");
    GswPtrs p;
    for (int l = 0; l < MLPW_MAX_LAYERS; ++l) {
        p.w[l] = l < nl ? w[l] : nullptr; p.b[l] = l < nl ? b[l] : nullptr;
        p.gw[l] = (gw && l < nl) ? gw[l] : nullptr; p.gb[l] = (gb && l < nl) ? gb[l] : nullptr;
    }
    const int total = (nl - 2) * nhidden * nhidden + (H + 4) * nhidden + 2;
    hipLaunchKernelGGL(gsw_update_kernel, dim3(cgs_ceil_div(total, 256)), dim3(256), 0, st, p, pw, ps, q.nchunks, q.sstride, nl, nhidden, nhp, lr);
    CGS_CHECK_LAUNCH("mlp2d_wide_g_step");
    return CGS_OK;
}

}  // extern "C"
