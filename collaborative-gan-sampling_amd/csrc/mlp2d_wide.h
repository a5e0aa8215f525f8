// What the sample-tile kernels of the wide 2-D discriminator share: the LDS image of a tile, the hidden -> hidden pass on the fp32 MFMA,
// one evaluation (logit and d logit / dx), the tile-size rule.  The layout is described at the top of mlp2d_wide.hip; mlp2d_wide_train.hip
// builds the D step on the same pass.
#pragma once
#include "cgs_internal.h"

#define MLPW_MAX_LAYERS 6
#define MLPW_THREADS 256
#define MLPW_MAX_CHUNKS 16

// Sample chunk of the weight-gradient products (mlp2d_wide_train.hip, mlp2d_wide_gstep.hip): a function of the batch alone, at most
// MLPW_MAX_CHUNKS chunks, a multiple of 128 samples
static int mlpw_chunk(int Bt) { return 128 * cgs_ceil_div(Bt, 128 * MLPW_MAX_CHUNKS); }

typedef float mlpw_f16 __attribute__((ext_vector_type(16)));

struct MlpWParams {
    const float* w[MLPW_MAX_LAYERS];   // layer l: [din_l][dout_l] row-major
    const float* b[MLPW_MAX_LAYERS];
    int nlayers, nh, nhp;              // nhp = nh rounded up to 32
};

struct MlpWLds {
    float* H;          // [T][nhp + 4], unit j at position hpos(j)
    float* slab;       // [2][nhp][T/2] swizzled (see above)
    unsigned* masks;   // [nlayers-1][T][nhp/32]: bit (j & 31) of word j >> 5 = (pre-activation of unit j > 0)
    float* w1p;        // [2][nhp]  first-layer rows in position order (the adjoint's reduction walks positions)
    float* wlp;        // [nhp]     last-layer column in position order
    float* xs;         // [T][2]    the tile's current points
};

__device__ __forceinline__ int hpos(int k) { return (k & ~7) | ((k & 1) << 2) | ((k >> 1) & 3); }

template <int T>
__device__ __forceinline__ MlpWLds mlpw_lds(float* smem, int nlayers, int nhp) {
    MlpWLds L;
    L.H = smem;
    L.slab = L.H + T * (nhp + 4);
    L.masks = (unsigned*)(L.slab + 2 * nhp * (T / 2));
    L.w1p = (float*)(L.masks + (nlayers - 1) * T * (nhp >> 5));
    L.wlp = L.w1p + 2 * nhp;
    L.xs = L.wlp + nhp;
    return L;
}

static size_t mlpw_smem(int T, int nlayers, int nhp) {
    return (size_t)(T * (nhp + 4) + 2 * nhp * (T / 2) + (nlayers - 1) * T * (nhp / 32) + 3 * nhp + 2 * T) * sizeof(float);
}

__device__ __forceinline__ void mlpw_load(const MlpWParams& p, const MlpWLds& L) {
    for (int j = threadIdx.x; j < p.nhp; j += MLPW_THREADS) {
        const bool in = j < p.nh;
        const int q = hpos(j);
        L.w1p[q] = in ? p.w[0][j] : 0.f;
        L.w1p[p.nhp + q] = in ? p.w[0][p.nh + j] : 0.f;
        L.wlp[q] = in ? p.w[p.nlayers - 1][j] : 0.f;
    }
}

// One hidden -> hidden layer for the tile.  Forward: H <- relu(H W + bias), mask bits of layer `ml` written.  Backward: H <- (H W^T) with
// the mask of layer `ml` (the layer below) applied to the result, which is what the next pass down, or the first layer's adjoint, needs.
// RAW (the generator): no ReLU, no mask read or written.  Forward (mlp2d_wide_gen.hip): H <- H W + bias as it leaves the accumulators;
// backward (mlp2d_wide_gstep.hip): H <- H W^T from a zero accumulator.
template <int T, bool BWD, bool RAW = false>
__device__ __forceinline__ void mlpw_pass(const MlpWParams& p, const MlpWLds& L, const float* __restrict__ W, const float* __restrict__ bias,
                                          int ml) {
    constexpr int NRB = T / 32, KS = T / 2, NSL = KS / 4, CPS = 16 / NSL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c31 = lane & 31;
    const int nh = p.nh, nhp = p.nhp, NB = nhp >> 5, NS = nhp / KS, HS = nhp + 4;
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
                unsigned* mw = &L.masks[(ml * T + row) * NB + cb];
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

// One evaluation for the tile's points L.xs: logit and d logit / dx of row tid >> 2 in every thread tid < 4 T (4 lanes per row).
template <int T>
__device__ __forceinline__ void mlpw_eval(const MlpWParams& p, const MlpWLds& L, float& logit, float& dldx0, float& dldx1) {
    const int tid = threadIdx.x, nh = p.nh, nhp = p.nhp, NB = nhp >> 5, HS = nhp + 4, nl = p.nlayers;
    __syncthreads();              // xs (and, on the first call, w1p / wlp) written; the previous evaluation's reads of H done
    for (int e = tid; e < T * nhp; e += MLPW_THREADS) {         // T * nhp is a multiple of 1024: whole waves, 32 consecutive units of a row per half
        const int row = e / nhp, j = e - row * nhp;
        float a = 0.f;
        if (j < nh) a = fmaf(L.xs[2 * row + 1], p.w[0][nh + j], fmaf(L.xs[2 * row], p.w[0][j], p.b[0][j]));
        const unsigned long long m = __ballot(a > 0.f);
        if ((tid & 31) == 0) L.masks[row * NB + (j >> 5)] = (unsigned)((tid & 32) ? m >> 32 : m);
        L.H[row * HS + hpos(j)] = fmaxf(a, 0.f);
    }
    __syncthreads();
    for (int l = 1; l < nl - 1; ++l) mlpw_pass<T, false>(p, L, p.w[l], p.b[l], l);
    const int row = tid >> 2, q4 = tid & 3;
    if (tid < 4 * T) {
        float part = 0.f;
        for (int q = q4; q < nhp; q += 4) part = fmaf(L.H[row * HS + q], L.wlp[q], part);
        part += __shfl_xor(part, 1, 64);
        part += __shfl_xor(part, 2, 64);
        logit = part + p.b[nl - 1][0];
    }
    __syncthreads();
    // backward: G = d logit / d h of the top hidden layer, masked by that layer's ReLU
    for (int e = tid; e < T * nhp; e += MLPW_THREADS) {
        const int row_ = e / nhp, j = e - row_ * nhp;
        const unsigned mw = L.masks[((nl - 2) * T + row_) * NB + (j >> 5)];
        L.H[row_ * HS + hpos(j)] = (j < nh && ((mw >> (j & 31)) & 1u)) ? p.w[nl - 1][j] : 0.f;
    }
    __syncthreads();
    for (int l = nl - 2; l >= 1; --l) mlpw_pass<T, true>(p, L, p.w[l], nullptr, l - 1);
    if (tid < 4 * T) {
        float d0 = 0.f, d1 = 0.f;
        for (int q = q4; q < nhp; q += 4) {
            const float g = L.H[row * HS + q];
            d0 = fmaf(g, L.w1p[q], d0);
            d1 = fmaf(g, L.w1p[nhp + q], d1);
        }
        d0 += __shfl_xor(d0, 1, 64); d1 += __shfl_xor(d1, 1, 64);
        d0 += __shfl_xor(d0, 2, 64); d1 += __shfl_xor(d1, 2, 64);
        dldx0 = d0; dldx1 = d1;
    }
}

__device__ __forceinline__ float mlpw_sigmoid(float v) { return v >= 0.f ? 1.f / (1.f + expf(-v)) : expf(v) / (1.f + expf(v)); }

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

static void mlpw_fill(MlpWParams& p, const float* const* w, const float* const* b, int nlayers, int nh) {
    for (int l = 0; l < MLPW_MAX_LAYERS; ++l) { p.w[l] = l < nlayers ? w[l] : nullptr; p.b[l] = l < nlayers ? b[l] : nullptr; }
    p.nlayers = nlayers; p.nh = nh; p.nhp = cgs_round_up(nh, 32);
}
