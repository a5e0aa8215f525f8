// The forward of the 2-D generator at 64 < nhidden <= 256 (the reference's 25-Gaussians runs: --nhidden=256 --nlayers=6): the function of
// gen_fwd_kernel of mlp2d.hip -- z[B,2] -> dense -> BN -> ReLU -> [dense -> BN -> ReLU] x (nlayers-2) -> dense -> x[B,2] -- on the sample
// tiles of mlp2d_wide.h.
//
// Training mode.  The batch couples every sample at every BN layer, so a launch per dense layer is the grid-wide barrier (as in mlp2d.hip):
//   launch 0            a_0 = z W_0 + b_0                                              VALU
//   launch l = 1..nl-2  a_l = relu(BN_{l-1}(a_{l-1})) W_l + b_l                        mlpw_pass<T, false, true>: v_mfma_f32_32x32x2_f32, W_l streamed from L2
//   launch nl-1         x   = relu(BN_{nl-2}(a_{nl-2})) W_last + b_last                VALU, 4 lanes per row (mlpw_rowdot)
// One workgroup of 4 waves per tile of T = mlpw_tile(B) samples.  Launch l >= 1 first turns the partial statistics of a_{l-1} into (mean,
// rstd), fills H [T][nhp + 4] in LDS from the stored a_{l-1} through relu(gamma (a - mean) rstd + beta) -- padded units nh <= j < nhp and
// rows past B enter as 0 -- and contracts.  The accumulators start at the bias and go to H as they are: no ReLU, no mask.  From H the rows
// below B go to the workspace, and every group of 32 consecutive rows leaves (mean, M2) per unit, summed over its rows in ascending order.
//
// Determinism: a partial belongs to rows [32 g, min(B, 32 g + 32)), whatever T is (a T = 64 tile writes two); the consumer combines the
// ceil(B / 32) partials in ascending g (mlpw_walk_partials) with Chan's update (gen_combine's statements).  A row's pre-activation is a k-ascending fmaf chain
// from the bias.  So every output is a function of the inputs and B alone, not of T or of the CU count.  No atomics.
// Every workgroup of launch l repeats the combine (one unit per thread, ceil(B / 32) steps); workgroup 0 also writes what a call writes
// once: the layer's (mean, rstd) row, batch_stats, and the moving averages v -= (v - value) * 0.1f (two roundings), value = the batch mean /
// the Bessel-corrected batch variance.  Normalisation itself uses the biased variance.
//
// Inference mode: the moving statistics replace the batch's, nothing couples the samples, and the whole net runs for a tile in ONE
// launch (H stays in LDS from layer to layer, BN + ReLU applied to it in place).  Nothing is written but x.
//
// Workspace (floats), H = nlayers - 1 BN layers, G = ceil(B / 32), nhp = nhidden rounded up to 32:
//   pre   [H][B][nhp]     the pre-activations, unit j at index j (natural order), padded units exact zeros: section 12's layout, which
//                         mlpw_wgrad_kernel can read as it reads acts / deltas
//   part  [H][G][2][nhp]  (mean, M2) of the row groups
//   stats [H][2][nhp]     (mean, rstd) of the batch, padded units 0
//   bytes = 4 H nhp (B + 2 G + 2)
#include "mlp2d_wide.h"

struct GenWLayer {
    const float* w; const float* b;                    // the dense layer of this launch: [din][dout], [dout]
    const float* gamma; const float* beta;             // launches l >= 1: BN of layer l-1 ...
    float* mmean; float* mvar;                         // ... its moving statistics, updated by workgroup 0
    const float* pre_in; const float* part_in;         // ... a_{l-1} [B][nhp] and its partials [G][2][nhp]
    float* stats_in;                                   // ... (mean, rstd) [2][nhp], written by workgroup 0
    float* bstat;                                      // ... optional (mean, biased variance) [2][nh]
    float* pre_out; float* part_out;                   // launches l < nlayers-1: a_l and its partials
    const float* z;                                    // launch 0: [B][2]
    float* x;                                          // launch nlayers-1: [B][2]
    int nh, nhp, B;
    float eps;
};

struct GenWNet {                                       // inference mode: the whole net
    const float* w[MLP2D_MAX_LAYERS]; const float* b[MLP2D_MAX_LAYERS];
    const float* gamma[MLP2D_MAX_LAYERS - 1]; const float* beta[MLP2D_MAX_LAYERS - 1];
    const float* mmean[MLP2D_MAX_LAYERS - 1]; const float* mvar[MLP2D_MAX_LAYERS - 1];
    const float* z; float* x;
    int nlayers, nh, nhp, B;
    float eps;
};

struct GenWLds : MlpWTileLds {       // slab: mlpw_pass's
    float* bn;         // [4][nhp]: mean, rstd, gamma, beta of the BN layer being applied (mlpw_bn_row)
    float* wl;         // [2][nhp]: the two columns of the last layer in position order
    float* zs;         // [T][2]: the tile's z
};

template <int T>
__device__ __forceinline__ GenWLds genw_lds(float* smem, int nhp) {
    GenWLds L;
    L.bn = mlpw_tile_lds<T>(L, smem, nhp);
    L.wl = L.bn + 4 * nhp;
    L.zs = L.wl + 2 * nhp;
    return L;
}

// nh = 256: T = 64: 135.5 KiB (one block per CU); T = 32: 70.8 KiB (two)
static size_t genw_smem(int T, int nhp) { return (mlpw_tile_floats(T, nhp) + 6 * nhp + 2 * T) * sizeof(float); }

// Thread j < nhp: (mean, rstd, gamma, beta) of unit j of the BN layer below into L.bn, from the partials of its row groups in ascending
// order.  Workgroup 0 writes the layer's statistics row, batch_stats and the moving averages.
__device__ __forceinline__ void genw_bn_train(const GenWLayer& a, float* bn) {
    const int j = threadIdx.x, nh = a.nh, nhp = a.nhp;
    if (j >= nhp) return;
    float mean = 0.f, rstd = 0.f;
    if (j < nh) {
        float n = 0.f, m = 0.f, M2 = 0.f;
        mlpw_walk_partials<2>(a.part_in, (a.B + 31) >> 5, nhp, j, [&](int g, const float (&p)[2]) {       // Chan's update, p = (mean, M2) of group g
            const float nb = (float)min(32, a.B - g * 32);
            const float nab = n + nb, d = p[0] - m;
            m = m + d * (nb / nab);
            M2 = M2 + p[1] + d * d * (n * nb / nab);
            n = nab;
        });
        mean = m;
        const float var = M2 / (float)a.B;
        rstd = 1.f / sqrtf(var + a.eps);
        if (blockIdx.x == 0) {
#pragma clang fp contract(off)      // assign_moving_average: v -= (v - value) * (1 - decay), decay 0.9 -> 0.1f; moving_variance takes the
                                    // Bessel-corrected batch variance of the fused kernel
            if (a.bstat) { a.bstat[j] = mean; a.bstat[nh + j] = var; }
            const float vu = var * ((float)a.B / (float)(a.B - 1));
            a.mmean[j] = a.mmean[j] - (a.mmean[j] - mean) * 0.1f;
            a.mvar[j] = a.mvar[j] - (a.mvar[j] - vu) * 0.1f;
        }
    }
    if (blockIdx.x == 0) { a.stats_in[j] = mean; a.stats_in[nhp + j] = rstd; }
    mlpw_bn_row(bn, nh, nhp, j, mean, rstd, a.gamma, a.beta);
}

// H <- relu(BN(a_{l-1})) of the tile's rows; rows past B and padded units (variance 0, no gamma / beta) enter as 0
template <int T>
__device__ __forceinline__ void genw_fill(const GenWLayer& a, const GenWLds& L, int row0, int rows) {
    const int nh = a.nh, nhp = a.nhp, HS = nhp + 4;
    for (int e = threadIdx.x; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        float h = 0.f;
        if (row < rows && j < nh) h = mlpw_bn_apply(a.pre_in[(size_t)(row0 + row) * nhp + j], L.bn, nhp, j);
        L.H[row * HS + hpos(j)] = h;
    }
}

// H (the tile's a_l) -> the workspace, rows below B only, and the (mean, M2) of each of the tile's groups of 32 rows that has a row below B
template <int T>
__device__ __forceinline__ void genw_emit(const GenWLayer& a, const GenWLds& L, int row0, int rows) {
    const int nhp = a.nhp, HS = nhp + 4;
    mlpw_store_h<T>(L, nhp, a.pre_out + (size_t)row0 * nhp, rows);
    for (int t = threadIdx.x; t < (T / 32) * nhp; t += MLPW_THREADS) {
        const int g = t / nhp, j = t - g * nhp, n = min(32, rows - 32 * g);
        if (n <= 0) continue;
        const float* col = L.H + 32 * g * HS + hpos(j);
        float sum = 0.f;
        for (int r = 0; r < n; ++r) sum += col[r * HS];
        const float mean = sum / (float)n;
        float M2 = 0.f;
        for (int r = 0; r < n; ++r) { const float d = col[r * HS] - mean; M2 = fmaf(d, d, M2); }
        float* P = a.part_out + (size_t)(row0 / 32 + g) * 2 * nhp;
        P[j] = mean; P[nhp + j] = M2;
    }
}

__device__ __forceinline__ void genw_load_last(const float* __restrict__ w, float* wl, int nh, int nhp) {
    for (int j = threadIdx.x; j < nhp; j += MLPW_THREADS) {
        const int q = hpos(j);
        wl[q] = j < nh ? w[2 * j] : 0.f;
        wl[nhp + q] = j < nh ? w[2 * j + 1] : 0.f;
    }
}

// x = H W_last + b_last by mlpw_rowdot
template <int T>
__device__ __forceinline__ void genw_out(const GenWLds& L, const float* __restrict__ b, float* __restrict__ x, int nhp, int row0, int rows) {
    const int tid = threadIdx.x, row = tid >> 2;
    if (tid >= 4 * T) return;                          // whole waves
    float p[2];
    mlpw_rowdot<2>(L, L.wl, nhp, p);
    if ((tid & 3) == 0 && row < rows) { x[2 * (size_t)(row0 + row)] = p[0] + b[0]; x[2 * (size_t)(row0 + row) + 1] = p[1] + b[1]; }
}

template <int T>
__device__ __forceinline__ void genw_load_z(const float* __restrict__ z, float* zs, int row0, int rows) {
    const int tid = threadIdx.x;
    if (tid < 2 * T) zs[tid] = (tid >> 1) < rows ? z[2 * (size_t)row0 + tid] : 0.f;
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void genw_first_kernel(GenWLayer a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GenWLds L = genw_lds<T>(smem, a.nhp);
    const int row0 = blockIdx.x * T, rows = min(T, a.B - row0);
    genw_load_z<T>(a.z, L.zs, row0, rows);
    __syncthreads();
    mlpw_first<T, false>(L, L.zs, a.w, a.b, a.nh, a.nhp);
    __syncthreads();
    genw_emit<T>(a, L, row0, rows);
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void genw_hidden_kernel(GenWLayer a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GenWLds L = genw_lds<T>(smem, a.nhp);
    const int row0 = blockIdx.x * T, rows = min(T, a.B - row0);
    genw_bn_train(a, L.bn);
    __syncthreads();
    genw_fill<T>(a, L, row0, rows);
    __syncthreads();
    mlpw_pass<T, false, true>(L, a.nh, a.nhp, a.w, a.b);
    genw_emit<T>(a, L, row0, rows);
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void genw_last_kernel(GenWLayer a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GenWLds L = genw_lds<T>(smem, a.nhp);
    const int row0 = blockIdx.x * T, rows = min(T, a.B - row0);
    genw_bn_train(a, L.bn);
    genw_load_last(a.w, L.wl, a.nh, a.nhp);
    __syncthreads();
    genw_fill<T>(a, L, row0, rows);
    __syncthreads();
    genw_out<T>(L, a.b, a.x, a.nhp, row0, rows);
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void genw_infer_kernel(GenWNet a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nh = a.nh, nhp = a.nhp, HS = nhp + 4, nl = a.nlayers, tid = threadIdx.x;
    const GenWLds L = genw_lds<T>(smem, nhp);
    const int row0 = blockIdx.x * T, rows = min(T, a.B - row0);
    genw_load_z<T>(a.z, L.zs, row0, rows);
    genw_load_last(a.w[nl - 1], L.wl, nh, nhp);
    __syncthreads();
    for (int l = 0; l < nl - 1; ++l) {
        if (l == 0) {
            mlpw_first<T, false>(L, L.zs, a.w[0], a.b[0], nh, nhp);
        } else {
            mlpw_pass<T, false, true>(L, nh, nhp, a.w[l], a.b[l]);
        }
        if (tid < nhp) {
            const bool in = tid < nh;
            mlpw_bn_row(L.bn, nh, nhp, tid, in ? a.mmean[l][tid] : 0.f, in ? 1.f / sqrtf(a.mvar[l][tid] + a.eps) : 0.f, a.gamma[l], a.beta[l]);
        }
        __syncthreads();
        for (int e = tid; e < T * nhp; e += MLPW_THREADS) {
            const int row = e / nhp, j = e - row * nhp;
            float* hp = &L.H[row * HS + hpos(j)];
            *hp = j < nh ? mlpw_bn_apply(*hp, L.bn, nhp, j) : 0.f;
        }
        __syncthreads();
    }
    genw_out<T>(L, a.b[nl - 1], a.x, nhp, row0, rows);
}

// launch l of the training forward
static int genw_train_launch(int T, const GenWLayer& a, int l, int nlayers, hipStream_t st) {
    const char* who = "mlp2d_wide_gen_fwd";
    const size_t smem = genw_smem(T, a.nhp);
    if (l == 0) return mlpw_launch_tile<genw_first_kernel<32>, genw_first_kernel<64>>(T, a.B, smem, who, who, st, a);
    if (l < nlayers - 1) return mlpw_launch_tile<genw_hidden_kernel<32>, genw_hidden_kernel<64>>(T, a.B, smem, who, who, st, a);
    return mlpw_launch_tile<genw_last_kernel<32>, genw_last_kernel<64>>(T, a.B, smem, who, who, st, a);
}

extern "C" {

size_t cgs_mlp2d_wide_gen_ws_bytes(int B, int nlayers, int nhidden) {
    if (B <= 0 || B > (1 << 24) || !mlpw_gen_shape_ok(nlayers, nhidden)) return 0;
    return genw_ws_floats(B, nlayers, cgs_round_up(nhidden, 32)) * sizeof(float);
}

int cgs_mlp2d_wide_gen_fwd(const float* const* w, const float* const* b, const float* const* gamma, const float* const* beta,
                           float* const* moving_mean, float* const* moving_variance, int nlayers, int nhidden, const float* z, float* x,
                           int B, int is_training, float eps, float* batch_stats, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mlp2d_wide_gen_fwd";
    int rc = mlp2d_check_net(who, w, b, nlayers, nhidden, MLP2D_WIDE_MIN_NH, MLP2D_MAX_NH);
    if (rc) return rc;
    if (!x) return cgs_set_error(CGS_EINVAL, "%s: null output", who);
    const int train = is_training != 0, nhp = cgs_round_up(nhidden, 32), H = nlayers - 1, G = cgs_ceil_div(B, 32);
    // B <= 2^24: the row counts of the combine are floats
    rc = mlp2d_check_gen(who, gamma, beta, moving_mean, moving_variance, nlayers, z, B, 1 << 24, train, eps,
                         genw_ws_floats(B, nlayers, nhp) * sizeof(float), ws, ws_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int T = mlpw_tile(B);
    if (!train) {
        GenWNet a = {};
        for (int l = 0; l < nlayers; ++l) { a.w[l] = w[l]; a.b[l] = b[l]; }
        for (int l = 0; l < H; ++l) { a.gamma[l] = gamma[l]; a.beta[l] = beta[l]; a.mmean[l] = moving_mean[l]; a.mvar[l] = moving_variance[l]; }
        a.z = z; a.x = x; a.nlayers = nlayers; a.nh = nhidden; a.nhp = nhp; a.B = B; a.eps = eps;
        return mlpw_launch_tile<genw_infer_kernel<32>, genw_infer_kernel<64>>(T, B, genw_smem(T, nhp), who, who, st, a);
    }
    float* pre = (float*)ws;
    float* part = pre + (size_t)H * B * nhp;
    float* stats = part + (size_t)H * G * 2 * nhp;
    for (int l = 0; l < nlayers; ++l) {
        GenWLayer a = {};
        a.w = w[l]; a.b = b[l];
        if (l > 0) {
            a.gamma = gamma[l - 1]; a.beta = beta[l - 1]; a.mmean = moving_mean[l - 1]; a.mvar = moving_variance[l - 1];
            a.pre_in = pre + (size_t)(l - 1) * B * nhp; a.part_in = part + (size_t)(l - 1) * G * 2 * nhp;
            a.stats_in = stats + (size_t)(l - 1) * 2 * nhp;
            a.bstat = batch_stats ? batch_stats + (size_t)(l - 1) * 2 * nhidden : nullptr;
        } else {
            a.z = z;
        }
        if (l < nlayers - 1) { a.pre_out = pre + (size_t)l * B * nhp; a.part_out = part + (size_t)l * G * 2 * nhp; }
        else a.x = x;
        a.nh = nhidden; a.nhp = nhp; a.B = B; a.eps = eps;
        rc = genw_train_launch(T, a, l, nlayers, st);
        if (rc) return rc;
    }
    return CGS_OK;
}

}  // extern "C"
