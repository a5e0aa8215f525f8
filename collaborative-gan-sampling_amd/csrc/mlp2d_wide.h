// What the kernels of the wide 2-D nets (64 < nhidden <= 256) share, each piece stated once (what the 64-unit
// kernels share with them -- the net's pointers, the refiner's rule, xhat / bn_relu -- is in mlp2d_shared.h):
//   the tile      the head of every tile kernel's LDS image (H, slab), the hidden -> hidden pass on the fp32 MFMA, the tile-size rule, the
//                 launch of a tile kernel, and the walks every net takes through H: first layer, 4-lanes-per-row product, top gradient, H -> memory
//   batch norm    the (mean, rstd, gamma, beta) row and xhat / relu(gamma xhat + beta) on it, the batched walk over row-group partials
//   gradients     the sample chunk, the dW product of a hidden -> hidden layer, the 16-in-flight column sums, the update kernel
// The layout is described at the top of mlp2d_wide.hip.  mlp2d_wide.hip (score, refine) and mlp2d_wide_train.hip (D step) are the
// discriminator; mlp2d_wide_gen.hip (forward) and mlp2d_wide_gstep.hip (G step) the generator.
#pragma once
#include "mlp2d_shared.h"

#define MLPW_THREADS 256
#define MLPW_MAX_CHUNKS 16

// Sample chunk of the weight-gradient products (mlp2d_wide_train.hip, mlp2d_wide_gstep.hip): a function of the batch alone, at most
// MLPW_MAX_CHUNKS chunks, a multiple of 128 samples
static int mlpw_chunk(int Bt) { return 128 * cgs_ceil_div(Bt, 128 * MLPW_MAX_CHUNKS); }

// Blocks of a weight-gradient launch that run mlpw_wgrad_mfma: 4 wave tasks each, a task per (hidden -> hidden layer, chunk, 64 x 64 block of dW)
static int mlpw_wgrad_blocks(int nlayers, int nhp, int nchunks) {
    const int NB2 = (nhp / 32 + 1) / 2;
    return cgs_ceil_div((nlayers - 2) * nchunks * NB2 * NB2, 4);
}

// Small partials of a weight-gradient launch, per chunk, for a net with `nout` outputs:
//   [(nl-1) nhp (db_l) | 2 nhp (dW_0) | nout nhp (dW_last, by column) | 4 (db_last [nout], then what the step adds: the D step's two loss sums)]
static int mlpw_small_stride(int nlayers, int nhp, int nout) { return (nlayers + 1 + nout) * nhp + 4; }

static bool mlpw_gen_shape_ok(int nlayers, int nhidden) { return mlp2d_shape_ok(nlayers, nhidden, MLP2D_WIDE_MIN_NH, MLP2D_MAX_NH); }

// Workspace floats of the generator's training forward (mlp2d_wide_gen.hip: pre | part | stats), the first bytes of the G step's
static size_t genw_ws_floats(int B, int nlayers, int nhp) {
    return (size_t)(nlayers - 1) * nhp * ((size_t)B + 2 * (size_t)cgs_ceil_div(B, 32) + 2);
}

typedef float mlpw_f16 __attribute__((ext_vector_type(16)));

// The head of every tile kernel's LDS image; each kernel family appends its own rows (MlpWLds below, GenWLds, GswLds)
struct MlpWTileLds {
    float* H;          // [T][nhp + 4], unit j at position hpos(j)
    float* slab;       // [2][nhp][T/2] swizzled (see the top of mlp2d_wide.hip)
};

static size_t mlpw_tile_floats(int T, int nhp) { return (size_t)T * (nhp + 4) + 2 * (size_t)nhp * (T / 2); }

// fills the head; -> the first float after it
template <int T>
__device__ __forceinline__ float* mlpw_tile_lds(MlpWTileLds& L, float* smem, int nhp) {
    L.H = smem;
    L.slab = L.H + T * (nhp + 4);
    return L.slab + 2 * nhp * (T / 2);
}

struct MlpWLds : MlpWTileLds {
    unsigned* masks;   // [nlayers-1][T][nhp/32]: bit (j & 31) of word j >> 5 = (pre-activation of unit j > 0)
    float* w1p;        // [2][nhp]  first-layer rows in position order (the adjoint's reduction walks positions)
    float* wlp;        // [nhp]     last-layer column in position order
    float* xs;         // [T][2]    the tile's current points
};

__device__ __forceinline__ int hpos(int k) { return (k & ~7) | ((k & 1) << 2) | ((k >> 1) & 3); }

template <int T>
__device__ __forceinline__ MlpWLds mlpw_lds(float* smem, int nlayers, int nhp) {
    MlpWLds L;
    L.masks = (unsigned*)mlpw_tile_lds<T>(L, smem, nhp);
    L.w1p = (float*)(L.masks + (nlayers - 1) * T * (nhp >> 5));
    L.wlp = L.w1p + 2 * nhp;
    L.xs = L.wlp + nhp;
    return L;
}

static size_t mlpw_smem(int T, int nlayers, int nhp) {
    return (mlpw_tile_floats(T, nhp) + (size_t)(nlayers - 1) * T * (nhp / 32) + 3 * nhp + 2 * T) * sizeof(float);
}

__device__ __forceinline__ void mlpw_load(const Mlp2dParams& p, const MlpWLds& L) {
    for (int j = threadIdx.x; j < p.nhp; j += MLPW_THREADS) {
        const bool in = j < p.nh;
        const int q = hpos(j);
        L.w1p[q] = in ? p.w[0][j] : 0.f;
        L.w1p[p.nhp + q] = in ? p.w[0][p.nh + j] : 0.f;
        L.wlp[q] = in ? p.w[p.nlayers - 1][j] : 0.f;
    }
}

// One hidden -> hidden layer for the tile.  Forward: H <- relu(H W + bias), mask bits of layer `ml` written to masks [nlayers-1][T][nhp/32].
// Backward: H <- (H W^T) with the mask of layer `ml` (the layer below) applied to the result, which is what the next pass down, or the first
// layer's adjoint, needs.
// RAW (the generator): no ReLU, no mask read or written.  Forward (mlp2d_wide_gen.hip): H <- H W + bias as it leaves the accumulators;
// backward (mlp2d_wide_gstep.hip): H <- H W^T from a zero accumulator.
template <int T, bool BWD, bool RAW = false>
__device__ __forceinline__ void mlpw_pass(const MlpWTileLds& L, int nh, int nhp, const float* __restrict__ W, const float* __restrict__ bias,
                                          unsigned* masks = nullptr, int ml = 0) {
    constexpr int NRB = T / 32, KS = T / 2, NSL = KS / 4, CPS = 16 / NSL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c31 = lane & 31;
    const int NB = nhp >> 5, NS = nhp / KS, HS = nhp + 4;
    const bool on0 = wave < NB, on1 = wave + 4 < NB;      // the wave's two column strips exist

    mlpw_f16 acc[2][NRB];
#pragma unroll
    for (int cbi = 0; cbi < 2; ++cbi) {
        const int j = (wave + 4 * cbi) * 32 + c31;
        const float bv = (!BWD && j < nh) ? bias[j] : 0.f;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cbi][rb][r] = bv;
    }

    // staging: a thread brings 4 reduction indices r0 + 2e of one output column c (= positions 4 qd .. 4 qd + 3, r0 = 8 (qd >> 1) + (qd & 1))
    // per step i.  Forward: c = tid (nhp <= 256 = the block), qd = i: each load instruction walks a row of W along its lanes.
    // Backward: qd = tid % NSL, c = tid / NSL + i 256/NSL: NSL lanes cover the KS floats of row c that the slab needs.
    const int sc0 = BWD ? tid / NSL : tid, sqd0 = BWD ? tid % NSL : 0;
    const float* Wt = W + (BWD ? sc0 * nh + 8 * (sqd0 >> 1) + (sqd0 & 1) : sc0);      // offsets below stay under 256 * 256
    float4 st[NSL];
    auto fetch = [&](int s) {
#pragma unroll
        for (int i = 0; i < NSL; ++i) {
            const int c = BWD ? sc0 + i * (MLPW_THREADS / NSL) : sc0, qd = BWD ? sqd0 : i;
            const int r0 = s * KS + 8 * (qd >> 1) + (qd & 1);
            auto at = [&](int e) {
                const int r = r0 + 2 * e;
                const int o = BWD ? i * (MLPW_THREADS / NSL) * nh + s * KS + 2 * e : r * nh;
                return (c < nh && r < nh) ? Wt[o] : 0.f;
            };
            st[i] = make_float4(at(0), at(1), at(2), at(3));
        }
    };
    auto stage = [&](int buf) {
        float* S = L.slab + buf * nhp * KS;
#pragma unroll
        for (int i = 0; i < NSL; ++i) {
            const int c = BWD ? sc0 + i * (MLPW_THREADS / NSL) : sc0, qd = BWD ? sqd0 : i;
            if (c < nhp) *(float4*)&S[(c * NSL + (qd ^ ((c / CPS) & (NSL - 1)))) * 4] = st[i];
        }
    };

    fetch(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) fetch(s + 1);
        if (on0) {
            const float* S = L.slab + (s & 1) * nhp * KS;
#pragma unroll
            for (int g = 0; g < KS / 8; ++g) {
                float4 a[NRB], b[2];
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) a[rb] = *(const float4*)&L.H[(rb * 32 + c31) * HS + s * KS + 8 * g + 4 * h];
#pragma unroll
                for (int cbi = 0; cbi < 2; ++cbi) {
                    const int c = (wave + 4 * cbi) * 32 + c31;
                    if (cbi ? on1 : on0) b[cbi] = *(const float4*)&S[(c * NSL + ((2 * g + h) ^ ((c / CPS) & (NSL - 1)))) * 4];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a_[2] = {i == 0 ? a[0].x : i == 1 ? a[0].y : i == 2 ? a[0].z : a[0].w,
                                         i == 0 ? a[NRB - 1].x : i == 1 ? a[NRB - 1].y : i == 2 ? a[NRB - 1].z : a[NRB - 1].w};
#pragma unroll
                    for (int cbi = 0; cbi < 2; ++cbi) {
                        if (!(cbi ? on1 : on0)) continue;
                        const float b_ = i == 0 ? b[cbi].x : i == 1 ? b[cbi].y : i == 2 ? b[cbi].z : b[cbi].w;
#pragma unroll
                        for (int rb = 0; rb < NRB; ++rb)
                            acc[cbi][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_[rb], b_, acc[cbi][rb], 0, 0, 0);
                    }
                }
            }
        }
        if (s + 1 < NS) stage((s + 1) & 1);
        __syncthreads();          // slab s read by every wave (and, at the last slab, H too); slab s + 1 written
    }

    // accumulator element r of lane (h, c31): row (r & 3) + 8 (r >> 2) + 4 h, column c31 of the 32x32 block
#pragma unroll
    for (int cbi = 0; cbi < 2; ++cbi) {
        if (!(cbi ? on1 : on0)) continue;
        const int cb = wave + 4 * cbi, q = hpos(cb * 32 + c31);
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                float v = acc[cbi][rb][r];
                if constexpr (RAW) { L.H[row * HS + q] = v; continue; }
                unsigned* mw = &masks[(ml * T + row) * NB + cb];
                if (!BWD) {
                    const unsigned long long m = __ballot(v > 0.f);       // low word: row of h = 0; high word: row + 4 of h = 1
                    if (c31 == 0) *mw = (unsigned)(h ? m >> 32 : m);
                    v = fmaxf(v, 0.f);
                } else {
                    v = ((*mw >> c31) & 1u) ? v : 0.f;
                }
                L.H[row * HS + q] = v;
            }
    }
    __syncthreads();
}

// ---- the walks through H that every net takes ----------------------------------------------------------------------------------------------

// First layer: H <- x W_0 + b_0 for the tile's points xs [T][2], padded units 0.  MASK (the discriminator): H <- relu of it, the decisions
// to `mask` [T][nhp/32].  T * nhp is a multiple of 1024: whole waves, 32 consecutive units of a row per half wave.
template <int T, bool MASK>
__device__ __forceinline__ void mlpw_first(const MlpWTileLds& L, const float* xs, const float* __restrict__ w, const float* __restrict__ b, int nh,
                                           int nhp, unsigned* mask = nullptr) {
    const int tid = threadIdx.x, NB = nhp >> 5, HS = nhp + 4;
    for (int e = tid; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        float a = 0.f;
        if (j < nh) a = fmaf(xs[2 * row + 1], w[nh + j], fmaf(xs[2 * row], w[j], b[j]));
        if constexpr (MASK) {
            const unsigned long long m = __ballot(a > 0.f);
            if ((tid & 31) == 0) mask[row * NB + (j >> 5)] = (unsigned)((tid & 32) ? m >> 32 : m);
            a = fmaxf(a, 0.f);
        }
        L.H[row * HS + hpos(j)] = a;
    }
}

// Row tid >> 2 of H times N columns cols [N][nhp] (position order), in every thread tid < 4 T: its 4 lanes walk the positions in the same
// order for every T, a fmaf chain each, and add up across lanes.  The logit, d logit / dx and the generator's x are this walk.
template <int N>
__device__ __forceinline__ void mlpw_rowdot(const MlpWTileLds& L, const float* cols, int nhp, float (&out)[N]) {
    const int row = threadIdx.x >> 2, HS = nhp + 4;
#pragma unroll
    for (int c = 0; c < N; ++c) out[c] = 0.f;
    for (int q = threadIdx.x & 3; q < nhp; q += 4) {
        const float h = L.H[row * HS + q];
#pragma unroll
        for (int c = 0; c < N; ++c) out[c] = fmaf(h, cols[c * nhp + q], out[c]);
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1)
#pragma unroll
        for (int c = 0; c < N; ++c) out[c] += __shfl_xor(out[c], m, 64);
}

// Top of the backward: H <- the gradient w.r.t. the top hidden layer's pre-activation = that layer's mask applied to w_last [nh] (times
// the row's seed [T] where SEED)
template <int T, bool SEED>
__device__ __forceinline__ void mlpw_top_grad(const MlpWTileLds& L, const unsigned* mask, const float* __restrict__ w_last, const float* seed,
                                              int nh, int nhp) {
    const int NB = nhp >> 5, HS = nhp + 4;
    for (int e = threadIdx.x; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        const unsigned mw = mask[row * NB + (j >> 5)];
        float g = 0.f;
        if (j < nh && ((mw >> (j & 31)) & 1u)) {
            if constexpr (SEED) g = seed[row] * w_last[j];
            else g = w_last[j];
        }
        L.H[row * HS + hpos(j)] = g;
    }
}

// the tile's H (LDS image, unit j at hpos(j)) -> dst[row][j] (natural order), rows of the tile below `rows` only
template <int T>
__device__ __forceinline__ void mlpw_store_h(const MlpWTileLds& L, int nhp, float* __restrict__ dst, int rows) {
    const int HS = nhp + 4;
    for (int e = threadIdx.x; e < T * nhp; e += MLPW_THREADS) {
        const int row = e / nhp, j = e - row * nhp;
        if (row < rows) dst[(size_t)row * nhp + j] = L.H[row * HS + hpos(j)];
    }
}

// One evaluation for the tile's points L.xs: logit and d logit / dx of row tid >> 2 in every thread tid < 4 T (4 lanes per row).
template <int T>
__device__ __forceinline__ void mlpw_eval(const Mlp2dParams& p, const MlpWLds& L, float& logit, float& dldx0, float& dldx1) {
    const int nh = p.nh, nhp = p.nhp, nl = p.nlayers, MW = T * (nhp >> 5);      // MW: words of one layer's masks
    const bool own = threadIdx.x < 4 * T;
    __syncthreads();              // xs (and, on the first call, w1p / wlp) written; the previous evaluation's reads of H done
    mlpw_first<T, true>(L, L.xs, p.w[0], p.b[0], nh, nhp, L.masks);
    __syncthreads();
    for (int l = 1; l < nl - 1; ++l) mlpw_pass<T, false>(L, nh, nhp, p.w[l], p.b[l], L.masks, l);
    if (own) {
        float v[1];
        mlpw_rowdot<1>(L, L.wlp, nhp, v);
        logit = v[0] + p.b[nl - 1][0];
    }
    __syncthreads();
    mlpw_top_grad<T, false>(L, L.masks + (nl - 2) * MW, p.w[nl - 1], nullptr, nh, nhp);
    __syncthreads();
    for (int l = nl - 2; l >= 1; --l) mlpw_pass<T, true>(L, nh, nhp, p.w[l], nullptr, L.masks, l - 1);
    if (own) {
        float d[2];
        mlpw_rowdot<2>(L, L.w1p, nhp, d);
        dldx0 = d[0]; dldx1 = d[1];
    }
}

// ---- batch norm on load (the generator) -----------------------------------------------------------------------------------------------------

// bn [4][nhp]: (mean, rstd, gamma, beta) of a BN layer, unit j at index j
__device__ __forceinline__ float mlpw_bn_xhat(float a, const float* bn, int nhp, int j) { return mlp2d_xhat(a, bn[j], bn[nhp + j]); }
__device__ __forceinline__ float mlpw_bn_apply(float a, const float* bn, int nhp, int j) {
    return mlp2d_bn_relu(mlpw_bn_xhat(a, bn, nhp, j), bn[2 * nhp + j], bn[3 * nhp + j]);
}

// thread j < nhp: unit j's entries of bn.  A padded unit has no gamma or beta to read and takes zeros; its mean and rstd come in as 0.
__device__ __forceinline__ void mlpw_bn_row(float* bn, int nh, int nhp, int j, float mean, float rstd, const float* __restrict__ gamma,
                                            const float* __restrict__ beta) {
    const bool in = j < nh;
    bn[j] = mean; bn[nhp + j] = rstd; bn[2 * nhp + j] = in ? gamma[j] : 0.f; bn[3 * nhp + j] = in ? beta[j] : 0.f;
}

// Unit j's row-group partials part [G][NP][nhp], MLP2D_PBATCH groups' loads in flight, handed to use(g, v[NP]) in ascending group order
template <int NP, class Use>
__device__ __forceinline__ void mlpw_walk_partials(const float* __restrict__ part, int G, int nhp, int j, Use&& use) {
    for (int g0 = 0; g0 < G; g0 += MLP2D_PBATCH) {
        float v[MLP2D_PBATCH][NP];
#pragma unroll
        for (int q = 0; q < MLP2D_PBATCH; ++q)
#pragma unroll
            for (int k = 0; k < NP; ++k) v[q][k] = g0 + q < G ? part[((size_t)(g0 + q) * NP + k) * nhp + j] : 0.f;
#pragma unroll
        for (int q = 0; q < MLP2D_PBATCH; ++q)
            if (g0 + q < G) use(g0 + q, v[q]);
    }
}

// ---- weight gradients and the update (mlp2d_wide_train.hip, mlp2d_wide_gstep.hip) ------------------------------------------------------------

// dW_l = A_{l-1}^T Delta_l of the hidden -> hidden layers on v_mfma_f32_32x32x2_f32, for the wave task t = 4 block + wave -> (layer hl + 1,
// chunk, 64 x 64 block of dW = 2 x 2 MFMA tiles): a lane supplies (row lane & 31, reduction index lane >> 5), the reduction index is the
// sample, so both fragments are 32 consecutive floats of one sample's workspace row.  deltas [nl-1][Bt][nhp]; the partial block goes to
// pw [layer][chunk][nhp][nhp].  The A fragment comes from loadA = makeA(hl, column, i1): loadA(o, ok, a0, a1) <- A_hl[sample][column],
// [column + 32] at row offset o, zeros where !ok (and a1 where !i1).
template <class MakeA>
__device__ __forceinline__ void mlpw_wgrad_mfma(int nlayers, int nhp, int Bt, int chunk, int nchunks, const float* __restrict__ deltas,
                                                float* __restrict__ pw, MakeA&& makeA) {
    const int tid = threadIdx.x, NB = nhp >> 5, NB2 = (NB + 1) >> 1, per = NB2 * NB2;
    const int lane = tid & 63, h = lane >> 5, c31 = lane & 31;
    const int t = blockIdx.x * 4 + (tid >> 6);
    if (t >= (nlayers - 2) * nchunks * per) return;
    const int lc = t / per, blk = t - lc * per, hl = lc / nchunks, c = lc - hl * nchunks;     // hl = 0: dW of layer 1
    const int ti = 2 * (blk / NB2), tj = 2 * (blk % NB2);
    const bool i1 = ti + 1 < NB, j1 = tj + 1 < NB;
    const int s0 = c * chunk, s1 = min(Bt, s0 + chunk);
    const auto loadA = makeA(hl, ti * 32 + c31, i1);
    const float* D = deltas + (hl + 1) * ((size_t)Bt * nhp) + tj * 32 + c31;
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
        for (int u = 0; u < 4; ++u) {                                   // rows past the chunk's end (the last chunk's past Bt) enter as zero
            const int ss = s + 2 * u + h;
            const bool ok = ss < s1;
            const size_t o = (size_t)ss * nhp;
            loadA(o, ok, a0[u], a1[u]);
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
    float* P = pw + (size_t)lc * nhp * nhp;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if ((a && !i1) || (b && !j1)) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r)     // accumulator element r of lane (h, c31): row (r & 3) + 8 (r >> 2) + 4 h, column c31
                P[(size_t)((ti + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * nhp + (tj + b) * 32 + c31] = acc[a][b][r];
        }
}

// The VALU sums over a chunk's samples [s0, s1): 16 samples' loads in flight -- load(s, ok, v[N]), zeros where !ok -- then their terms taken
// by use(v[N]) in ascending sample order: the sums are those of a plain serial loop without a load's latency per term (the chunk size is
// a multiple of 16; rows past the chunk's end add an exact zero)
template <int N, class Load, class Use>
__device__ __forceinline__ void mlpw_walk_samples(int s0, int s1, Load&& load, Use&& use) {
#pragma unroll 1
    for (int s = s0; s < s1; s += 16) {
        float v[16][N];
#pragma unroll
        for (int u = 0; u < 16; ++u) load(s + u, s + u < s1, v[u]);
#pragma unroll
        for (int u = 0; u < 16; ++u) use(v[u]);
    }
}

// elements of the update of a net with `nout` outputs; the D step (nout = 1) appends its two loss sums
static __host__ __device__ int mlpw_update_elems(int nlayers, int nh, int nout) { return (nlayers - 2) * nh * nh + (nlayers + 1 + nout) * nh + nout + (nout == 1 ? 2 : 0); }

// Every gradient element = its chunk partials added in ascending chunk order; gw / gb written, w <- w - lr * g.
// element e of [hidden -> hidden dW: (nl-2) nh nh | dW_0: 2 nh | dW_last: NOUT nh | db_l: (nl-1) nh | db_last: NOUT | NOUT = 1: loss: 2],
// the small ones where mlpw_small_stride puts them
template <int NOUT>
__global__ __launch_bounds__(256) void mlpw_update_kernel(Mlp2dVars q, const float* __restrict__ pw, const float* __restrict__ ps, int nchunks,
                                                          int sstride, int nlayers, int nh, int nhp, float lr, float* __restrict__ loss) {
    const int nhid = nlayers - 1, nhh = nh * nh, nbig = (nlayers - 2) * nhh, tail = (nhid + 2 + NOUT) * nhp;
    const int total = mlpw_update_elems(nlayers, nh, NOUT);
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
            } else if ((r -= 2 * nh) < NOUT * nh) {             // dW_last [nh][NOUT]
                P = ps + (nhid + 2 + r % NOUT) * nhp + r / NOUT;
                wv = q.w[nhid] + r; gv = q.gw[nhid] ? q.gw[nhid] + r : nullptr;
            } else if ((r -= NOUT * nh) < nhid * nh) {          // db_l [nh]
                const int l = r / nh, j = r - l * nh;
                P = ps + l * nhp + j;
                wv = q.b[l] + j; gv = q.gb[l] ? q.gb[l] + j : nullptr;
            } else if ((r -= nhid * nh) < NOUT) {               // db_last [NOUT]
                P = ps + tail + r;
                wv = q.b[nhid] + r; gv = q.gb[nhid] ? q.gb[nhid] + r : nullptr;
            } else {                                            // d_loss_real, d_loss_fake
                P = ps + tail + r;
                wv = nullptr; gv = loss ? loss + (r - NOUT) : nullptr;
            }
        }
        float g = 0.f;
        for (int c = 0; c < nchunks; ++c) g += P[c * stride];
        if (gv) *gv = g;
        if (wv && lr != 0.f) *wv = *wv - lr * g;
    }
}

template <int NOUT>
static int mlpw_update(const char* who, const Mlp2dVars& q, const float* pw, const float* ps, int nchunks, int nlayers, int nh, int nhp, float lr,
                       float* loss, hipStream_t st) {
    const int total = mlpw_update_elems(nlayers, nh, NOUT);
    hipLaunchKernelGGL(mlpw_update_kernel<NOUT>, dim3(cgs_ceil_div(total, 256)), dim3(256), 0, st, q, pw, ps, nchunks,
                       mlpw_small_stride(nlayers, nhp, NOUT), nlayers, nh, nhp, lr, loss);
    CGS_CHECK_LAUNCH(who);
    return CGS_OK;
}

// ---- tiles on the host --------------------------------------------------------------------------------------------------------------------------

// Sample tile.  A T = 64 block streams every weight once per 64 samples and needs the CU's LDS to itself; two T = 32 blocks share a CU
// and its matrix units, so a T = 32 block costs about half a T = 64 block of a CU's time and twice its weight traffic per sample.
// With n64 / n32 tiles on `cus` CUs the busiest CU carries ceil(n64 / cus) units of work at T = 64 and ceil(n32 / cus) / 2 at T = 32:
// T = 32 where that is strictly less (B = 1000: 32 blocks on 32 CUs instead of 16 on 16), T = 64 on a tie (B = 10 000: 157 blocks, one
// each on 157 CUs, against 313 blocks with 57 CUs carrying two: the same critical path at half the L2 reads).
static int mlpw_tile(int B) {
    static int cus_[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 63;
    if (!cus_[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cus_[dev] = n;
    }
    const int cus = cus_[dev], n64 = cgs_ceil_div(B, 64), n32 = cgs_ceil_div(B, 32);
    return 2 * cgs_ceil_div(n64, cus) > cgs_ceil_div(n32, cus) ? 32 : 64;
}

// One launch of the tile kernel K (an instantiation at T) over the tiles of B samples: the LDS attribute once per kernel and device (the
// flag inside CGS_SMEM_ATTR is this function's, one per K), the launch, its check.  `who` names the entry point, `what` the launch.
template <auto K, class... Args>
static int mlpw_launch(int T, int B, size_t smem, const char* who, const char* what, hipStream_t st, const Args&... args) {
    CGS_SMEM_ATTR(160 * 1024, who, K);
    hipLaunchKernelGGL(K, dim3(cgs_ceil_div(B, T)), dim3(MLPW_THREADS), smem, st, args...);
    CGS_CHECK_LAUNCH(what);
    return CGS_OK;
}

// ... of the instantiation for T = mlpw_tile(B): K32 at 32, K64 at 64
template <auto K32, auto K64, class... Args>
static int mlpw_launch_tile(int T, int B, size_t smem, const char* who, const char* what, hipStream_t st, const Args&... args) {
    return T == 32 ? mlpw_launch<K32>(32, B, smem, who, what, st, args...) : mlpw_launch<K64>(64, B, smem, who, what, st, args...);
}
