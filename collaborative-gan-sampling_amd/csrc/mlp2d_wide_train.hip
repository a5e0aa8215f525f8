// The D step of the 2-D net at 64 < nhidden <= 256 (synthetic/main.py:361-370 at the reference's --nhidden=256 --nlayers=6):
//   d_loss = mean_b BCE(D(real_b), 1) + mean_b BCE(D(fake_b), 0),  w <- w - lr * d d_loss / dw  for every D variable.
// What mlp2d.hip does per sample with every layer in LDS, done per sample TILE on the pass of mlp2d_wide.h, in four launches:
//
// Pass A (mlpw_train_kernel<T>, one launch per part: real rows, target 1; fake rows, target 0): the tile walk of mlpw_eval -- H in LDS,
//   the hidden -> hidden layers and their adjoints by mlpw_pass -- seeded with scale * (sigmoid(logit) - target), scale = 1 / B_part,
//   where the refiner has 1.  After every layer the tile's H is copied to the workspace: forward the post-ReLU activation A_l, backward
//   the masked gradient Delta_l w.r.t. the pre-activation of layer l.  The row's seed and its BCE term (mlp_train_fwdbwd_kernel's
//   formula) go there too.  Rows past B of a tail tile are never stored.
// Pass B (mlpw_wgrad_kernel): dW_l = A_{l-1}^T Delta_l of the hidden -> hidden layers on v_mfma_f32_32x32x2_f32: a lane supplies (row
//   lane & 31, reduction index lane >> 5), the reduction index is the sample, so both fragments are 32 consecutive floats of one sample's
//   workspace row, read straight from global memory.  A wave owns a 64 x 64 block of one layer's dW (2 x 2 MFMA tiles) for one CHUNK of
//   samples and writes its partial block to the workspace.  The other gradients -- x^T Delta_0, A_{nl-2}^T dlast, every db_l = column
//   sums of Delta_l, sum dlast, the two loss sums -- are VALU sums over the chunk's samples in ascending order, one thread per column
//   (16 samples' loads in flight at a time), in further blocks of the same launch; they leave partials too.
// Pass C (mlpw_update_kernel): every gradient element = its partials added in chunk order; gw / gb written, w <- w - lr * g.
//
// Determinism: the chunk size is a function of B_total alone (mlpw_chunk: 128 ceil(B_total / 2048) samples, hence at most 16 chunks),
// never of the device; inside a chunk the MFMA's k-ordered chain and the VALU loops walk the samples in ascending order; pass C adds the
// chunks in ascending order.  No atomics.
//
// Workspace order: acts and deltas are [layer][sample][nhp], real rows first, then the fake rows; within a row unit j stands at index j
// (NATURAL order: pass A undoes the LDS image's hpos() on its way out), padded units nh <= j < nhp included, which hold exact zeros.
// So pass B needs no column bound, and reads rows s >= B_total of its last chunk as zero.
//   floats: acts   [nl-1][Bt][nhp] | deltas [nl-1][Bt][nhp] | dlast [Bt] | bce [Bt]
//           | partial dW  [nl-2][16][nhp][nhp]
//           | partial small [16][(nl-1) nhp (db_l) + 2 nhp (dW_0) + nhp (dW_last) + 4 (db_last, loss real, loss fake, 0)]
// At 256 x 6 and 1000 + 1000 rows: 20.5 MB of activations and gradients + 16.8 MB of partial tiles = 37.3 MB.
#include "mlp2d_wide.h"

struct MlpWTrainWs {
    float* acts;
    float* deltas;
    float* dlast;
    float* bce;
    float* pw;      // partial dW of the hidden -> hidden layers
    float* ps;      // partial small pieces
    int Bt, chunk, nchunks, sstride;
};

static size_t mlpw_train_ws_floats(int Bt, int nlayers, int nhp) {
    const size_t nhid = nlayers - 1;
    return 2 * nhid * Bt * nhp + 2 * (size_t)Bt + (size_t)MLPW_MAX_CHUNKS * ((nlayers - 2) * (size_t)nhp * nhp + (nhid + 3) * nhp + 4);
}

static MlpWTrainWs mlpw_train_ws(float* ws, int Bt, int nlayers, int nhp) {
    MlpWTrainWs s;
    const size_t nhid = nlayers - 1;
    s.acts = ws;
    s.deltas = s.acts + nhid * Bt * nhp;
    s.dlast = s.deltas + nhid * Bt * nhp;
    s.bce = s.dlast + Bt;
    s.pw = s.bce + Bt;
    s.ps = s.pw + (size_t)MLPW_MAX_CHUNKS * (nlayers - 2) * nhp * nhp;
    s.Bt = Bt; s.chunk = mlpw_chunk(Bt); s.nchunks = cgs_ceil_div(Bt, s.chunk); s.sstride = (int)(nhid + 3) * nhp + 4;
    return s;
}

// the tile's H (LDS image, unit j at hpos(j)) -> dst[row0 + row][j], rows of the tile below `rows` only
template <int T>
__device__ __forceinline__ void mlpw_store_h(const MlpWLds& L, int nhp, float* __restrict__ dst, int rows) {
    const int HS = nhp + 4;
    for (int e = threadIdx.x; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        if (row < rows) dst[(size_t)row * nhp + j] = L.H[row * HS + hpos(j)];
    }
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void mlpw_train_kernel(MlpWParams p, const float* __restrict__ x, int B, int part0,
                                                                  float target, float scale, MlpWTrainWs ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpWLds L = mlpw_lds<T>(smem, p.nlayers, p.nhp);
    mlpw_load(p, L);
    const int tid = threadIdx.x, nh = p.nh, nhp = p.nhp, NB = nhp >> 5, HS = nhp + 4, nl = p.nlayers;
    const long row0 = (long)blockIdx.x * T;
    const int rows = (int)(B - row0 < T ? B - row0 : T);                   // rows of this tile that exist
    const size_t lstride = (size_t)ws.Bt * nhp, base = (size_t)(part0 + row0) * nhp;
    if (tid < 2 * T) L.xs[tid] = (tid >> 1) < rows ? x[2 * row0 + tid] : 0.f;
    __syncthreads();
    for (int e = tid; e < T * nhp; e += MLPW_THREADS) {                     // as mlpw_eval
        const int row = e / nhp, j = e - row * nhp;
        float a = 0.f;
        if (j < nh) a = fmaf(L.xs[2 * row + 1], p.w[0][nh + j], fmaf(L.xs[2 * row], p.w[0][j], p.b[0][j]));
        const unsigned long long m = __ballot(a > 0.f);
        if ((tid & 31) == 0) L.masks[row * NB + (j >> 5)] = (unsigned)((tid & 32) ? m >> 32 : m);
        L.H[row * HS + hpos(j)] = fmaxf(a, 0.f);
    }
    __syncthreads();
    mlpw_store_h<T>(L, nhp, ws.acts + base, rows);
    for (int l = 1; l < nl - 1; ++l) {
        mlpw_pass<T, false>(p, L, p.w[l], p.b[l], l);
        mlpw_store_h<T>(L, nhp, ws.acts + l * lstride + base, rows);
    }
    const int row = tid >> 2, q4 = tid & 3;
    if (tid < 4 * T) {
        float part = 0.f;
        for (int q = q4; q < nhp; q += 4) part = fmaf(L.H[row * HS + q], L.wlp[q], part);
        part += __shfl_xor(part, 1, 64);
        part += __shfl_xor(part, 2, 64);
        const float logit = part + p.b[nl - 1][0];
        const float seed = scale * (mlpw_sigmoid(logit) - target);        // d (scale * BCE(logit, target)) / d logit
        if (q4 == 0) {
            L.xs[row] = seed;                                              // the points are spent: xs carries the seeds to the next loop
            if (row < rows) {
                ws.dlast[part0 + row0 + row] = seed;
                ws.bce[part0 + row0 + row] = scale * (fmaxf(logit, 0.f) - logit * target + log1pf(expf(-fabsf(logit))));
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < T * nhp; e += MLPW_THREADS) {
        const int row_ = e / nhp, j = e - row_ * nhp;
        const unsigned mw = L.masks[((nl - 2) * T + row_) * NB + (j >> 5)];
        L.H[row_ * HS + hpos(j)] = (j < nh && ((mw >> (j & 31)) & 1u)) ? L.xs[row_] * p.w[nl - 1][j] : 0.f;
    }
    __syncthreads();
    mlpw_store_h<T>(L, nhp, ws.deltas + (nl - 2) * lstride + base, rows);
    for (int l = nl - 2; l >= 1; --l) {
        mlpw_pass<T, true>(p, L, p.w[l], nullptr, l - 1);
        mlpw_store_h<T>(L, nhp, ws.deltas + (l - 1) * lstride + base, rows);
    }
}

// blocks [0, nmfma): 4 waves, wave task t = 4 block + wave -> (hidden -> hidden layer, chunk, 64 x 64 block of dW).
// blocks [nmfma, nmfma + nchunks (nl-1)): (chunk, hidden layer l): thread j < nhp sums column j of Delta_l over the chunk (db_l); l = 0 adds
// x^T Delta_0; l = nl-2 adds A_{nl-2}^T dlast and, in threads 0..2, sum dlast and the two loss sums.
__global__ __launch_bounds__(MLPW_THREADS) void mlpw_wgrad_kernel(MlpWTrainWs ws, int nlayers, int nhp, int nmfma, const float* __restrict__ xr, int Br,
                                                                  const float* __restrict__ xf) {
    const int tid = threadIdx.x, Bt = ws.Bt, nhid = nlayers - 1;
    const size_t lstride = (size_t)Bt * nhp;
    if ((int)blockIdx.x < nmfma) {
        const int NB = nhp >> 5, NB2 = (NB + 1) >> 1, per = NB2 * NB2;
        const int lane = tid & 63, h = lane >> 5, c31 = lane & 31;
        const int t = blockIdx.x * 4 + (tid >> 6);
        if (t >= (nlayers - 2) * ws.nchunks * per) return;
        const int lc = t / per, blk = t - lc * per, hl = lc / ws.nchunks, c = lc - hl * ws.nchunks;     // hl = 0: dW of layer 1
        const int ti = 2 * (blk / NB2), tj = 2 * (blk % NB2);
        const bool i1 = ti + 1 < NB, j1 = tj + 1 < NB;
        const int s0 = c * ws.chunk, s1 = min(Bt, s0 + ws.chunk);
        const float* A = ws.acts + hl * lstride + ti * 32 + c31;
        const float* D = ws.deltas + (hl + 1) * lstride + tj * 32 + c31;
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
            for (int u = 0; u < 4; ++u) {                                   // rows past the chunk's end (the last chunk's past B_total) read as zero
                const int ss = s + 2 * u + h;
                const bool ok = ss < s1;
                const size_t o = (size_t)ss * nhp;
                a0[u] = ok ? A[o] : 0.f; a1[u] = (ok && i1) ? A[o + 32] : 0.f;
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
        float* P = ws.pw + (size_t)lc * nhp * nhp;                          // [layer][chunk][nhp][nhp]
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
    const int s0 = c * ws.chunk, s1 = min(Bt, s0 + ws.chunk);
    float* S = ws.ps + (size_t)c * ws.sstride;
    if (tid < nhp) {
        // 16 samples' loads in flight, then their terms added in ascending sample order: the sums are those of a plain serial loop without
        // a load's latency per term (the chunk size is a multiple of 16; rows past the chunk's end add an exact zero)
        const float* D = ws.deltas + l * lstride + tid;
        float db = 0.f, g0 = 0.f, g1 = 0.f;
#pragma unroll 1
        for (int s = s0; s < s1; s += 16) {
            float d[16], x0[16], x1[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int ss = s + u;
                const bool ok = ss < s1;
                d[u] = ok ? D[(size_t)ss * nhp] : 0.f;
                x0[u] = x1[u] = 0.f;
                if (ok && l == 0) {
                    const float* xp = ss < Br ? xr + 2 * (size_t)ss : xf + 2 * (size_t)(ss - Br);
                    x0[u] = xp[0]; x1[u] = xp[1];
                }
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) { db += d[u]; g0 = fmaf(x0[u], d[u], g0); g1 = fmaf(x1[u], d[u], g1); }
        }
        S[l * nhp + tid] = db;
        if (l == 0) { S[nhid * nhp + tid] = g0; S[(nhid + 1) * nhp + tid] = g1; }
        if (l == nhid - 1) {
            const float* A = ws.acts + l * lstride + tid;
            float g = 0.f;
#pragma unroll 1
            for (int s = s0; s < s1; s += 16) {
                float a[16], dl[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int ss = s + u;
                    const bool ok = ss < s1;
                    a[u] = ok ? A[(size_t)ss * nhp] : 0.f;
                    dl[u] = ok ? ws.dlast[ss] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) g = fmaf(a[u], dl[u], g);
            }
            S[(nhid + 2) * nhp + tid] = g;
        }
    }
    if (l == nhid - 1 && tid < 3) {
        const float* v = tid == 0 ? ws.dlast : ws.bce;
        const int lo = tid == 2 ? max(s0, Br) : s0, hi = tid == 1 ? min(s1, Br) : s1;       // thread 1: the real rows; thread 2: the fake rows
        float a = 0.f;
        for (int s = lo; s < hi; ++s) a += v[s];
        S[(nhid + 3) * nhp + tid] = a;
    }
}

struct MlpWTrainPtrs {
    float* w[MLPW_MAX_LAYERS];
    float* b[MLPW_MAX_LAYERS];
    float* gw[MLPW_MAX_LAYERS];      // may be null
    float* gb[MLPW_MAX_LAYERS];
};

// element e of [hidden -> hidden dW: (nl-2) nh nh | dW_0: 2 nh | dW_last: nh | db_l: (nl-1) nh | db_last: 1 | loss: 2]
__global__ __launch_bounds__(256) void mlpw_update_kernel(MlpWTrainPtrs q, MlpWTrainWs ws, int nlayers, int nh, int nhp, float lr, float* __restrict__ loss) {
    const int nhid = nlayers - 1, nhh = nh * nh, nbig = (nlayers - 2) * nhh, total = nbig + (nhid + 3) * nh + 3;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
#pragma clang fp contract(off)      // var -= lr * grad as two roundings (GradientDescentOptimizer's ApplyGradientDescent)
        const float* P;
        size_t stride;
        float *wv, *gv;
        if (e < nbig) {
            const int hl = e / nhh, r = e - hl * nhh, i = r / nh, j = r - i * nh;
            stride = (size_t)nhp * nhp;
            P = ws.pw + (size_t)hl * ws.nchunks * stride + (size_t)i * nhp + j;
            wv = q.w[hl + 1] + r; gv = q.gw[hl + 1] ? q.gw[hl + 1] + r : nullptr;
        } else {
            int r = e - nbig;
            stride = ws.sstride;
            if (r < 2 * nh) {                                   // dW_0 [2][nh]
                P = ws.ps + (nhid + r / nh) * nhp + r % nh;
                wv = q.w[0] + r; gv = q.gw[0] ? q.gw[0] + r : nullptr;
            } else if ((r -= 2 * nh) < nh) {                    // dW_last [nh][1]
                P = ws.ps + (nhid + 2) * nhp + r;
                wv = q.w[nhid] + r; gv = q.gw[nhid] ? q.gw[nhid] + r : nullptr;
            } else if ((r -= nh) < nhid * nh) {                 // db_l [nh]
                const int l = r / nh, j = r - l * nh;
                P = ws.ps + l * nhp + j;
                wv = q.b[l] + j; gv = q.gb[l] ? q.gb[l] + j : nullptr;
            } else if ((r -= nhid * nh) == 0) {                 // db_last
                P = ws.ps + (nhid + 3) * nhp;
                wv = q.b[nhid]; gv = q.gb[nhid];
            } else {                                            // d_loss_real, d_loss_fake
                P = ws.ps + (nhid + 3) * nhp + r;
                wv = nullptr; gv = loss ? loss + (r - 1) : nullptr;
            }
        }
        float g = 0.f;
        for (int c = 0; c < ws.nchunks; ++c) g += P[c * stride];
        if (gv) *gv = g;
        if (wv && lr != 0.f) *wv = *wv - lr * g;
    }
}

template <int T>
static int mlpw_train_launch(const MlpWParams& p, const float* x, int B, int part0, float target, const MlpWTrainWs& ws, hipStream_t st) {
    const size_t smem = mlpw_smem(T, p.nlayers, p.nhp);
    CGS_SMEM_ATTR(160 * 1024, "mlp2d_wide_d_step", mlpw_train_kernel<T>);
    hipLaunchKernelGGL(mlpw_train_kernel<T>, dim3(cgs_ceil_div(B, T)), dim3(MLPW_THREADS), smem, st, p, x, B, part0, target, 1.f / (float)B, ws);
    CGS_CHECK_LAUNCH("mlpw_train");
    return CGS_OK;
}

size_t cgs_mlp2d_wide_train_ws(int Bt, int nlayers, int nh) { return mlpw_train_ws_floats(Bt, nlayers, cgs_round_up(nh, 32)) * sizeof(float); }

// the caller (mlp2d.hip) has checked every argument and the workspace size; 64 < nh <= 256
int cgs_mlp2d_wide_train(float* const* w, float* const* b, int nlayers, int nh, const float* real, int B_real, const float* fake, int B_fake,
                         float lr, float* const* gw, float* const* gb, float* loss, void* ws_, hipStream_t st) {
    MlpWParams p;
    mlpw_fill(p, (const float* const*)w, (const float* const*)b, nlayers, nh);
    const int Bt = B_real + B_fake, nhp = p.nhp, nhid = nlayers - 1;
    const MlpWTrainWs ws = mlpw_train_ws((float*)ws_, Bt, nlayers, nhp);
    for (int part = 0; part < 2; ++part) {      // real rows (target 1) then fake rows (target 0); each loss term is a MEAN
        const int B = part ? B_fake : B_real, part0 = part ? B_real : 0;
        const float* x = part ? fake : real;
        const int rc = mlpw_tile(B) == 32 ? mlpw_train_launch<32>(p, x, B, part0, part ? 0.f : 1.f, ws, st)
                                          : mlpw_train_launch<64>(p, x, B, part0, part ? 0.f : 1.f, ws, st);
        if (rc) return rc;
    }
    const int NB2 = (nhp / 32 + 1) / 2, nmfma = cgs_ceil_div((nlayers - 2) * ws.nchunks * NB2 * NB2, 4);
    hipLaunchKernelGGL(mlpw_wgrad_kernel, dim3(nmfma + ws.nchunks * nhid), dim3(MLPW_THREADS), 0, st, ws, nlayers, nhp, nmfma, real, B_real, fake);
    CGS_CHECK_LAUNCH("mlpw_wgrad");
    MlpWTrainPtrs q;
    for (int l = 0; l < MLPW_MAX_LAYERS; ++l) {
        q.w[l] = l < nlayers ? w[l] : nullptr; q.b[l] = l < nlayers ? b[l] : nullptr;
        q.gw[l] = (gw && l < nlayers) ? gw[l] : nullptr; q.gb[l] = (gb && l < nlayers) ? gb[l] : nullptr;
    }
    const int total = (nlayers - 2) * nh * nh + (nhid + 3) * nh + 3;
    hipLaunchKernelGGL(mlpw_update_kernel, dim3(cgs_ceil_div(total, 256)), dim3(256), 0, st, q, ws, nlayers, nh, nhp, lr, loss);
    CGS_CHECK_LAUNCH("mlpw_update");
    return CGS_OK;
}
