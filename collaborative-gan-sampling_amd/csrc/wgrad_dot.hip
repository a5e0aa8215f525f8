// The two gradient kernels the D step of a PatchGAN discriminator adds to wgrad.hip's (BASELINE config 5; shaping.DShaper):
//
// 1. Weight gradient of a convolution to ONE output channel over a deep reduction (K = kh * kw * Cin >= 1024), the backward-weight
//    twin of conv_dot.hip: the logit head 4x4 x 512 -> 1.  On wgrad.hip's GEMM the single output channel is padded to a 128-column
//    tile (1/128 of the issued MFMA work is useful).  Here
//
//      dW[ky][kx][c] (+)= sum_{b,oh,ow} x[b, oh*s+ky-pt, ow*s+kx-pl, c] * dy[b,oh,ow]
//
//    is an axpy per output pixel: a thread owns one float4 of consecutive channels of one tap (a wave: 1 KB of one tap's row,
//    coalesced), walks a slab of consecutive output pixels and adds x * dy[m] -- dy[m] is uniform over the block.  Padding taps are
//    skipped (no load).  A pixel's channel vector is read by the kh*kw taps' threads: the blocks of one slab differ in blockIdx.y
//    only, so they sit on one XCD and all but the first read come from its L2.  One partial dW per slab, the slabs added in a fixed
//    order by a second kernel (no atomics: a rerun is bit-identical), optionally accumulating into dW (two D passes: real + refined).
//
// 2. scale / offset gradients of an instance norm from the per-sample sums its backward-data call left in its workspace: the twin
//    of cgs_bn_train_param_grads (wgrad.hip).
#include "cgs_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- slab plan (restated by tests/test_patchgan_shaping_cpu.py) ----
#define CO1_THREADS 256          // float4 columns (tap, channel quad) per block
#define CO1_UNROLL 4             // pixels in flight per thread
#define CO1_BLOCKS 1024          // blocks aimed at: 4 per CU
#define CO1_MIN_PIX 32           // at least this many pixels per slab (a slab costs one partial dW written and read back)
#define CO1_MAX_SLABS 256

struct Co1Params {
    const float* x;      // [B,H,W,C]
    const float* dy;     // [B,Ho,Wo]
    float* slab;         // [slabs][K]
    int H, W, C, Ho, Wo;
    int kw, S, pt, pl;
    int cq;              // float4 per pixel
    int K4;              // float4 columns = kh * kw * cq
    int M;               // output pixels B * Ho * Wo
    int pps;             // pixels per slab
    int slabs;
};

__global__ __launch_bounds__(CO1_THREADS) void wgrad_cout1_kernel(Co1Params p) {
    const int j = blockIdx.y * CO1_THREADS + threadIdx.x;
    if (j >= p.K4) return;
    const int tap = j / p.cq, q = j - tap * p.cq;
    const int offy = tap / p.kw - p.pt, offx = tap % p.kw - p.pl;
    const int m0 = blockIdx.x * p.pps;
    const int m1 = m0 + p.pps < p.M ? m0 + p.pps : p.M;          // (the last slab may be short)
    const int RC = p.Ho * p.Wo;
    int b = m0 / RC;
    int oh = (m0 - b * RC) / p.Wo, ow = m0 - b * RC - oh * p.Wo;
    const float* __restrict__ xq = p.x + 4 * q;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m1; m += CO1_UNROLL) {
        f32x4 v[CO1_UNROLL];
        float d[CO1_UNROLL];
        bool in[CO1_UNROLL];
#pragma unroll
        for (int u = 0; u < CO1_UNROLL; ++u) {
            in[u] = false; d[u] = 0.f; v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (m + u < m1) {                                      // (block-uniform)
                d[u] = p.dy[m + u];
                const int iy = oh * p.S + offy, ix = ow * p.S + offx;
                in[u] = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                if (in[u]) v[u] = *(const f32x4*)(xq + ((size_t)(b * p.H + iy) * p.W + ix) * p.C);     // a padding tap is not read
                if (++ow == p.Wo) {
                    ow = 0;
                    if (++oh == p.Ho) { oh = 0; ++b; }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < CO1_UNROLL; ++u)
            if (in[u]) {
                acc.x = fmaf(v[u].x, d[u], acc.x); acc.y = fmaf(v[u].y, d[u], acc.y);
                acc.z = fmaf(v[u].z, d[u], acc.z); acc.w = fmaf(v[u].w, d[u], acc.w);
            }
    }
    *(f32x4*)(p.slab + ((size_t)blockIdx.x * p.K4 + j) * 4) = acc;
}

// dW[4j .. 4j+3] (+)= sum_z slab[z][4j .. 4j+3]: a block serves 64 float4 columns, its four waves a quarter of the slabs each (in
// ascending order), the four sums added in wave order -- a fixed tree for a given slab count.
__global__ __launch_bounds__(256) void wgrad_cout1_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw, int K4, int slabs,
                                                                 int accumulate, int vec) {
    __shared__ f32x4 red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int per = (slabs + 3) / 4;
    const int z0 = wv * per, z1 = z0 + per < slabs ? z0 + per : slabs;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (j < K4) {
#pragma unroll 8
        for (int z = z0; z < z1; ++z) s += *(const f32x4*)(slab + ((size_t)z * K4 + j) * 4);
    }
    red[wv][lane] = s;
    __syncthreads();
    if (wv != 0 || j >= K4) return;
    f32x4 t = red[0][lane];
    t += red[1][lane]; t += red[2][lane]; t += red[3][lane];
    float* o = dw + 4 * (size_t)j;
    if (vec) {
        if (accumulate) t += *(const f32x4*)o;
        *(f32x4*)o = t;
    } else {                                                       // (a gradient tensor that is not 16-byte aligned)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = accumulate ? o[e] + t[e] : t[e];
    }
}

// the shapes cgs_conv_dot_ok takes on the forward side for one output channel; sets the plan
static bool co1_plan(Co1Params& p, int B, int H, int W, int Cin, int kh, int kw, int sh, int sw) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0) return false;
    if ((Cin % 4) != 0 || (long)kh * kw * Cin < 1024 || sh != sw) return false;
    const long Ho = cgs_ceil_div(H, sh), Wo = cgs_ceil_div(W, sw);
    if ((long)B * H * W * Cin * 4 > 0x7fffffffL || (long)kh * kw * Cin * 4 > 0x7fffffffL) return false;      // (32-bit pixel and column indices)
    p.H = H; p.W = W; p.C = Cin; p.Ho = (int)Ho; p.Wo = (int)Wo;
    p.kw = kw; p.S = sh;
    p.pt = cgs_same_pad_before(H, kh, sh); p.pl = cgs_same_pad_before(W, kw, sw);
    p.cq = Cin / 4;
    p.K4 = kh * kw * p.cq;
    p.M = (int)(B * Ho * Wo);
    const int colblocks = cgs_ceil_div(p.K4, CO1_THREADS);
    if (colblocks > 65535) return false;
    int slabs = cgs_ceil_div(CO1_BLOCKS, colblocks);
    const int most = p.M / CO1_MIN_PIX > 1 ? p.M / CO1_MIN_PIX : 1;
    if (slabs > most) slabs = most;
    if (slabs > CO1_MAX_SLABS) slabs = CO1_MAX_SLABS;
    p.pps = cgs_round_up(cgs_ceil_div(p.M, slabs), CO1_UNROLL);
    p.slabs = cgs_ceil_div(p.M, p.pps);
    return true;
}

__global__ void instnorm_param_grad_kernel(const float* __restrict__ stat2, int B, double HWd, float* __restrict__ dscale,
                                           float* __restrict__ doffset, int C, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, g = 0.0;                                       // (ascending b, in double: one rounding at the end)
    for (int b = 0; b < B; ++b) {
        a += (double)stat2[(size_t)b * 2 * C + c];
        g += (double)stat2[(size_t)b * 2 * C + C + c];
    }
    const float db = (float)(a * HWd), dg = (float)(g * HWd);
    doffset[c] = accumulate ? doffset[c] + db : db;
    dscale[c] = accumulate ? dscale[c] + dg : dg;
}

extern "C" {

size_t cgs_conv_wgrad_cout1_ws_bytes(int B, int H, int W, int Cin, int kh, int kw, int sh, int sw) {
    Co1Params p;
    if (!co1_plan(p, B, H, W, Cin, kh, kw, sh, sw)) return 0;
    return (size_t)p.slabs * p.K4 * 4 * sizeof(float);
}

int cgs_conv2d_nhwc_bwd_weight_cout1(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int kh, int kw, int sh,
                                     int sw, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    Co1Params p;
    if (!x || !dy || !dw || !co1_plan(p, B, H, W, Cin, kh, kw, sh, sw))
        return cgs_set_error(CGS_EINVAL, "conv2d_nhwc_bwd_weight_cout1: needs Cin %% 4 == 0, kh*kw*Cin >= 1024, sh == sw (B=%d %dx%dx%d k=%dx%d s=%dx%d)",
                             B, H, W, Cin, kh, kw, sh, sw);
    if (((uintptr_t)x & 15) || ((uintptr_t)ws & 15))
        return cgs_set_error(CGS_EINVAL, "conv2d_nhwc_bwd_weight_cout1: x and the workspace must be 16-byte aligned");
    const size_t need = (size_t)p.slabs * p.K4 * 4 * sizeof(float);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "conv2d_nhwc_bwd_weight_cout1: workspace %zu < %zu bytes", ws_bytes, need);
    p.x = x; p.dy = dy; p.slab = (float*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wgrad_cout1_kernel, dim3(p.slabs, cgs_ceil_div(p.K4, CO1_THREADS)), dim3(CO1_THREADS), 0, s, p);
    CGS_CHECK_LAUNCH("conv2d_nhwc_bwd_weight_cout1");
    hipLaunchKernelGGL(wgrad_cout1_reduce_kernel, dim3(cgs_ceil_div(p.K4, 64)), dim3(256), 0, s, p.slab, dw, p.K4, p.slabs, accumulate,
                       ((uintptr_t)dw & 15) == 0 ? 1 : 0);
    CGS_CHECK_LAUNCH("conv2d_nhwc_bwd_weight_cout1");
    return CGS_OK;
}

int cgs_instnorm_param_grads(const void* bwd_ws, int B, int HW, int C, float* dscale, float* doffset, int accumulate, void* stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || (C & 3) || B > 65535 || !bwd_ws || !dscale || !doffset)
        return cgs_set_error(CGS_EINVAL, "instnorm_param_grads: bad argument (B=%d HW=%d C=%d)", B, HW, C);
    const float* stat2 = (const float*)bwd_ws + cgs_instnorm_stat2_offset(B, HW, C);
    hipLaunchKernelGGL(instnorm_param_grad_kernel, dim3(cgs_ceil_div(C, 64)), dim3(64), 0, (hipStream_t)stream, stat2, B, (double)HW, dscale,
                       doffset, C, accumulate);
    CGS_CHECK_LAUNCH("instnorm_param_grads");
    return CGS_OK;
}

}  // extern "C"
