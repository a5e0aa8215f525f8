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
// by mlp2d_xhat and mlp2d_bn_relu, the forward's own functions, so a mask never disagrees with the forward's; dxhat = decision ? dh gamma : 0 goes to dbuf
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
// so mean, rstd, gamma, beta are four registers per column: GswBnCol), again by mlp2d_xhat and mlp2d_bn_relu.
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
//   ps    [16][mlpw_small_stride at two outputs: H nhp (db_l) + 2 nhp (dW_0) + 2 nhp (dW_last, by column) + 4 (db_last, 0, 0)]
#include "mlp2d_wide.h"

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

struct GswLds : MlpWTileLds {        // slab: mlpw_pass's; the epilogue keeps xhat [T][nhp] (natural order) there
    float* bn;         // [4][nhp]: mean, rstd, gamma, beta of layer l (mlpw_bn_row)
    float* up;         // [5][nhp]: mean, rstd, mean(dxhat), mean(dxhat (xhat - e)), e = mean(xhat) of layer u; the top launch: the two
                       // columns of W_last
    float* gp;         // [T][2]: the tile's grad_plugin
};

template <int T>
__device__ __forceinline__ GswLds gsw_lds(float* smem, int nhp) {
    GswLds L;
    L.bn = mlpw_tile_lds<T>(L, smem, nhp);
    L.up = L.bn + 4 * nhp;
    L.gp = L.up + 5 * nhp;
    return L;
}

// nh = 256: T = 64: 138.5 KiB (one block per CU); T = 32: 73.8 KiB (two)
static size_t gsw_smem(int T, int nhp) { return (mlpw_tile_floats(T, nhp) + 9 * nhp + 2 * T) * sizeof(float); }

// thread j < nhp: (mean, rstd, gamma, beta) of unit j of layer l
__device__ __forceinline__ void gsw_load_bn(const GswLayer& a, float* bn) {
    const int j = threadIdx.x, nh = a.nh, nhp = a.nhp;
    if (j < nhp) mlpw_bn_row(bn, nh, nhp, j, j < nh ? a.stats_l[j] : 0.f, j < nh ? a.stats_l[nhp + j] : 0.f, a.gamma_l, a.beta_l);
}

// thread j < nhp: (mean, rstd, mean(dxhat), mean(dxhat (xhat - e)), e) of unit j of layer u, the three batch means from the partials of its
// row groups added in ascending group order
__device__ __forceinline__ void gsw_load_up(const GswLayer& a, float* up) {
    const int j = threadIdx.x, nh = a.nh, nhp = a.nhp;
    if (j >= nhp) return;
    float mean = 0.f, rstd = 0.f, c1 = 0.f, c2 = 0.f, ex = 0.f;
    if (j < nh) {
        GswSum s1, s2, s3;
        mlpw_walk_partials<3>(a.bpart_u, (a.B + 31) >> 5, nhp, j, [&](int, const float (&p)[3]) { s1.add(p[0]); s2.add(p[1]); s3.add(p[2]); });
        c1 = s1.s / (float)a.B; ex = s3.s / (float)a.B; c2 = s2.s / (float)a.B - ex * c1;
        mean = a.stats_u[j]; rstd = a.stats_u[nhp + j];
    }
    up[j] = mean; up[nhp + j] = rstd; up[2 * nhp + j] = c1; up[3 * nhp + j] = c2; up[4 * nhp + j] = ex;
}

// tf FusedBatchNormGrad, training: da = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), xhat the forward's, centred (see the top)
__device__ __forceinline__ float gsw_da(float a, float dx, const float* up, int nhp, int j) {
    const float ru = up[nhp + j], xh = mlp2d_xhat(a, up[j], ru);
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
            xh = mlpw_bn_xhat(a.pre_l[(size_t)(row0 + row) * nhp + j], L.bn, nhp, j);
            dx = mlp2d_bn_relu(xh, L.bn[2 * nhp + j], L.bn[3 * nhp + j]) > 0.f ? *hp * L.bn[2 * nhp + j] : 0.f;      // the forward's h > 0
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
    mlpw_pass<T, true, true>(L, a.nh, a.nhp, a.w_up, nullptr);
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
    const float* gamma[MLP2D_MAX_LAYERS - 1]; const float* beta[MLP2D_MAX_LAYERS - 1];
    const float* z; const float* gplug;
    float* pw; float* ps;
    int nlayers, nh, nhp, B, chunk, nchunks, sstride;
};

// (mean, rstd, gamma, beta) of column `col` of BN layer l in registers, zeros in a padded column; h(a) = relu(BN(a)) of a pre-activation
struct GswBnCol {
    float m, r, g, e;
    bool in;
    __device__ __forceinline__ GswBnCol(const GswGrad& q, int l, int col, bool on = true) {
        const float* S = q.stats + (size_t)l * 2 * q.nhp;
        in = on && col < q.nh;
        m = in ? S[col] : 0.f; r = in ? S[q.nhp + col] : 0.f; g = in ? q.gamma[l][col] : 0.f; e = in ? q.beta[l][col] : 0.f;
    }
    __device__ __forceinline__ float h(float a) const { return mlp2d_bn_relu(mlp2d_xhat(a, m, r), g, e); }
};

// blocks [0, nmfma): mlpw_wgrad_mfma, the A fragment h = relu(BN(a)) recomputed from the pre-activations on load.
// blocks [nmfma, nmfma + nchunks (nl-1)): (chunk, BN layer l): thread j < nhp sums column j of da_l over the chunk (db_l); l = 0 adds
// z^T da_0; l = nl-2 adds h_{nl-2}^T grad_plugin and, in threads 0 and 1, the column sums of grad_plugin (db_last).
__global__ __launch_bounds__(MLPW_THREADS) void gsw_wgrad_kernel(GswGrad q, int nmfma) {
    const int tid = threadIdx.x, B = q.B, nhp = q.nhp, nhid = q.nlayers - 1;
    const size_t lstride = (size_t)B * nhp;
    if ((int)blockIdx.x < nmfma) {
        mlpw_wgrad_mfma(q.nlayers, nhp, B, q.chunk, q.nchunks, q.dbuf, q.pw, [&](int hl, int col, bool i1) {
            return [A = q.pre + hl * lstride + col, c0 = GswBnCol(q, hl, col), c1 = GswBnCol(q, hl, col + 32, i1)](size_t o, bool ok, float& a0, float& a1) {
                a0 = (ok && c0.in) ? c0.h(A[o]) : 0.f; a1 = (ok && c1.in) ? c1.h(A[o + 32]) : 0.f;
            };
        });
        return;
    }
    const int sb = blockIdx.x - nmfma, c = sb / nhid, l = sb - c * nhid;
    const int s0 = c * q.chunk, s1 = min(B, s0 + q.chunk);
    float* S = q.ps + (size_t)c * q.sstride;
    if (tid < nhp) {
        const float* D = q.dbuf + l * lstride + tid;
        GswSum db;
        float g0 = 0.f, g1 = 0.f;
        mlpw_walk_samples<3>(s0, s1, [&](int ss, bool ok, float (&v)[3]) {
            v[0] = ok ? D[(size_t)ss * nhp] : 0.f;
            v[1] = v[2] = 0.f;
            if (ok && l == 0) { v[1] = q.z[2 * (size_t)ss]; v[2] = q.z[2 * (size_t)ss + 1]; }
        }, [&](const float (&v)[3]) { db.add(v[0]); g0 = fmaf(v[1], v[0], g0); g1 = fmaf(v[2], v[0], g1); });
        S[l * nhp + tid] = db.s;
        if (l == 0) { S[nhid * nhp + tid] = g0; S[(nhid + 1) * nhp + tid] = g1; }
        if (l == nhid - 1) {
            const float* A = q.pre + l * lstride + tid;
            const GswBnCol bn(q, l, tid);
            float w0 = 0.f, w1 = 0.f;
            mlpw_walk_samples<3>(s0, s1, [&](int ss, bool ok, float (&v)[3]) {
                v[0] = (ok && bn.in) ? bn.h(A[(size_t)ss * nhp]) : 0.f;
                v[1] = ok ? q.gplug[2 * (size_t)ss] : 0.f;
                v[2] = ok ? q.gplug[2 * (size_t)ss + 1] : 0.f;
            }, [&](const float (&v)[3]) { w0 = fmaf(v[0], v[1], w0); w1 = fmaf(v[0], v[2], w1); });
            S[(nhid + 2) * nhp + tid] = w0; S[(nhid + 3) * nhp + tid] = w1;
        }
    }
    if (l == nhid - 1 && tid < 2) {
        float a = 0.f;
        for (int s = s0; s < s1; ++s) a += q.gplug[2 * (size_t)s + tid];
        S[(nhid + 4) * nhp + tid] = a;
    }
}

static size_t gsw_ws_floats(int B, int nlayers, int nhp) {
    const size_t H = nlayers - 1, G = cgs_ceil_div(B, 32);
    return genw_ws_floats(B, nlayers, nhp) + H * B * nhp + H * G * 3 * nhp + 2 * (size_t)B +
           (size_t)MLPW_MAX_CHUNKS * ((size_t)(nlayers - 2) * nhp * nhp + mlpw_small_stride(nlayers, nhp, 2));
}

extern "C" {

size_t cgs_mlp2d_wide_g_step_ws_bytes(int B, int nlayers, int nhidden) {
    if (B <= 0 || B > (1 << 24) || !mlpw_gen_shape_ok(nlayers, nhidden)) return 0;
    return gsw_ws_floats(B, nlayers, cgs_round_up(nhidden, 32)) * sizeof(float);
}

int cgs_mlp2d_wide_g_step(float* const* w, float* const* b, const float* const* gamma, const float* const* beta, float* const* moving_mean,
                          float* const* moving_variance, int nlayers, int nhidden, const float* z, const float* grad_plugin, int B, float eps,
                          float lr, float* const* gw, float* const* gb, float* x, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mlp2d_wide_g_step";
    int rc = mlp2d_check_net(who, (const float* const*)w, (const float* const*)b, nlayers, nhidden, MLP2D_WIDE_MIN_NH, MLP2D_MAX_NH);
    if (rc) return rc;
    if (!grad_plugin) return cgs_set_error(CGS_EINVAL, "%s: null grad_plugin", who);
    const int nl = nlayers, nhp = cgs_round_up(nhidden, 32), H = nl - 1, G = cgs_ceil_div(B, 32);
    rc = mlp2d_check_gen(who, gamma, beta, moving_mean, moving_variance, nl, z, B, 1 << 24, 1, eps, gsw_ws_floats(B, nl, nhp) * sizeof(float), ws,
                         ws_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t lstride = (size_t)B * nhp, pstride = (size_t)G * 2 * nhp, bstride = (size_t)G * 3 * nhp;
    float* pre = (float*)ws;
    float* stats = pre + H * lstride + H * pstride;
    float* dbuf = pre + genw_ws_floats(B, nl, nhp);
    float* bpart = dbuf + H * lstride;
    float* xs = bpart + H * bstride;
    float* pw = xs + 2 * (size_t)B;
    float* ps = pw + (size_t)MLPW_MAX_CHUNKS * (nl - 2) * nhp * nhp;
    rc = cgs_mlp2d_wide_gen_fwd((const float* const*)w, (const float* const*)b, gamma, beta, moving_mean, moving_variance, nl, nhidden, z,
                                    x ? x : xs, B, 1, eps, nullptr, ws, genw_ws_floats(B, nl, nhp) * sizeof(float), stream);
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
            rc = u == nl - 1 ? mlpw_launch_tile<gsw_top_kernel<32>, gsw_top_kernel<64>>(T, B, gsw_smem(T, nhp), who, who, st, a)
                             : mlpw_launch_tile<gsw_layer_kernel<32>, gsw_layer_kernel<64>>(T, B, gsw_smem(T, nhp), who, who, st, a);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(gsw_first_kernel, dim3(cgs_ceil_div(B, 64)), dim3(MLPW_THREADS), 0, st, a);
            CGS_CHECK_LAUNCH(who);
        }
    }
    GswGrad q = {};
    q.pre = pre; q.stats = stats; q.dbuf = dbuf;
    for (int l = 0; l < H; ++l) { q.gamma[l] = gamma[l]; q.beta[l] = beta[l]; }
    q.z = z; q.gplug = grad_plugin; q.pw = pw; q.ps = ps;
    q.nlayers = nl; q.nh = nhidden; q.nhp = nhp; q.B = B;
    q.chunk = mlpw_chunk(B); q.nchunks = cgs_ceil_div(B, q.chunk); q.sstride = mlpw_small_stride(nl, nhp, 2);
    const int nmfma = mlpw_wgrad_blocks(nl, nhp, q.nchunks);
    hipLaunchKernelGGL(gsw_wgrad_kernel, dim3(nmfma + q.nchunks * H), dim3(MLPW_THREADS), 0, st, q, nmfma);
    CGS_CHECK_LAUNCH(who);
    return mlpw_update<2>(who, mlp2d_vars(w, b, gw, gb, nl), pw, ps, q.nchunks, nl, nhidden, nhp, lr, nullptr, st);
}

}  // extern "C"
