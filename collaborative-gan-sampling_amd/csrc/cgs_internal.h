// Internal declarations shared by the kernels of libcgs_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cgs_hip.h"

int cgs_set_error(int code, const char* fmt, ...);
void cgs_note_kernel(const char* name);   // remembered per thread, read back by cgs_last_kernel()
void cgs_note_flops(double executed);     // ... by cgs_last_executed_flops()
void cgs_add_flops(double executed);      // (accumulating form: one entry point may launch several batch chunks)
void cgs_note_tail(int tiles, int split); // ... by cgs_last_tail_tiles() / cgs_last_tail_split()
void cgs_note_igemm_plan(int xcd_map, int cls_flip, int uni, int gx, int splitk);   // ... by cgs_last_igemm_plan()

#define CGS_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) return cgs_set_error(CGS_ELAUNCH, "%s: %s", name, hipGetErrorString(e_)); \
    } while (0)

static inline int cgs_ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int cgs_round_up(int a, int b) { return cgs_ceil_div(a, b) * b; }

// TF 'SAME' padding before the first pixel.
static inline int cgs_same_pad_before(int size, int k, int s) {
    int out = cgs_ceil_div(size, s);
    int tot = (out - 1) * s + k - size;
    if (tot < 0) tot = 0;
    return tot / 2;
}

// ---------------------------------------------------------------------------------------------
// One "conv layer relation": a BIG tensor [B,Hb,Wb,Cb] and a SMALL tensor [B,Hs,Ws,Cs] with
// Hs = ceil(Hb/s), tied by weights w[kh][kw][Cb][Cs] (conv HWIO: Cb=Cin,Cs=Cout; deconv
// [kh,kw,Cout,Cin]: Cb=Cout,Cs=Cin -- the same layout, because conv2d_transpose is defined as the
// adjoint of the conv with that filter).  Two contractions exist:
//   F (big -> small): conv fwd, deconv bwd-data.   reduce over (tap, Cb), N = Cs
//   T (small -> big): deconv fwd, conv bwd-data.   reduce over (tap, Cs), N = Cb; s*s parity classes
// ---------------------------------------------------------------------------------------------
struct CgsLayer {
    int kh, kw, sh, sw;
    int Hb, Wb, Cb, Hs, Ws, Cs;
};

#define CGS_BN_MAX_BLOCKS 512   // stage-1 partial blocks of the per-channel reductions (bn.hip workspace layout)
size_t cgs_bn_stat2_offset(int C);                        // floats in front of stat2[2][C] in a batch norm's workspace (bn.hip)
size_t cgs_instnorm_stat2_offset(int B, int HW, int C);   // floats in front of stat2[B][2][C] in an instance norm's workspace (bn.hip)
#define CGS_BK 32           // K-tile of the implicit GEMM
#define CGS_MAX_CLASSES 4   // stride <= 2 for the T direction

struct IgemmClass {
    int R, C;        // base-pixel grid of this class per image (rows of the GEMM: M = B*R*C)
    int py, px;      // output pixel = (r*So + py, c*So + px)
    int nty, ntx;    // taps of this class: t = ta*ntx + tb
    int dy0, dx0;    // input pixel = (r*S + dy0 + ta*dstep, c*S + dx0 + tb*dstep)
    int ky0, kx0;    // weight tap of (ta,tb) = (ky0 + ta*kstep, kx0 + tb*kstep)
    int K;           // nty*ntx*Cred
    int w_off;       // float offset of this class' packed weights
    int slab_off;    // float offset of this class' split-K slabs
};

struct IgemmParams {
    const float* in;
    const float* wp;     // packed weights [class][Kpad/4][Np][4]
    const float* bias;
    const float* ep_a;
    const float* ep_b;
    const float* ep_aux; // [same shape as out] for the *_BWD epilogues
    float* out;
    int B, Hin, Win, Cred;      // input tensor (reduction channels per tap)
    int Hout, Wout, N, Np;      // output tensor, N channels (Np = N rounded up to 64)
    int S, So, dstep, kstep;
    int epilogue;
    int pix_major;       // GEMM rows ordered (pixel, image) instead of (image, pixel): enables zero-tap skipping
    int splitk;          // > 1: blockIdx.z splits the K tiles; raw partial tiles go to slab, reduced by a second kernel
    float* slab;         // [class][split][M_c][Np]
    int tap_parity;      // VEC K order visits the taps even offsets first, then odd, per axis (stride-2 F direction)
    int xcd_map;         // block id -> (XCD, local index) decode: an m-tile's n-tiles run on one XCD (see igemm_kernel)
    int cls_flip;        // two-round launches of several parity classes: in the odd round every group of cls_flip consecutive classes runs in reverse order (0 = off; igemm_kernel)
    int uni;             // uniform-tile K loop allowed (host policy, see cgs_igemm_launch)
    int lpt;             // pixel-major only: m-tiles visit the pixels in perm[] order (most valid taps first)
    unsigned* sign_out;  // != null: sign bitmask of the stored output (layout: cgs_hip.h, "sign masks"); wide epilogue, N % 32 == 0, no split-K
    long sign_plane;     // words per 32-channel plane of the mask = pixels of the WHOLE tensor (a launch may be one batch chunk of it)
    float* stat_part;    // != null: per-(m-tile, wave row) column sums / sums of squares of the output, [class][2 * m-tiles][2][N] (fused norm statistics)
    int stat_cls_rows;   // partial rows per parity class = 2 * m-tiles of a class (the launcher sets it)
    // Norm-BACKWARD statistics (round 6; stat_part != null and ns_mean != null, CGS_EPI_NONE, ep_aux = x): the launch is the backward-data
    // pass that produces the gradient dy w.r.t. the OUTPUT of a norm (+ lrelu) whose input x has the shape of this launch's result; the
    // partial rows then hold [sum d | sum d * xhat] with d = dy * lrelu'(scale * x + shift), xhat = (x - mean) * invstd -- the two column
    // sums the norm's backward pass otherwise takes in a pass of its own over dy and x (bn.hip, bn_partial_kernel<1>).
    // ns_mean / ns_inv are [groups][N], ns_gamma / ns_beta [N]; ns_gimg = images per statistics group (0: the whole batch is one group).
    const float* ns_mean = nullptr;
    const float* ns_inv = nullptr;
    const float* ns_gamma = nullptr;
    const float* ns_beta = nullptr;
    float ns_leak = 1.f;
    int ns_gimg = 0;
    // Fused momentum update (up_mom != null; CGS_EPI_NONE, no bias, no statistics / sign mask, N % 4 == 0, VEC): the launch is the backward-data
    // pass whose result g is the gradient w.r.t. the refined feature; instead of storing g, the element's owner applies refine_update1 to
    // out (= the feature theta, read AND written) and up_mom (the momentum buffer, same shape) -- the igemm_up_kernel twin's epilogue, or the
    // reduce kernel of a split-K / tail-split launch.  g itself never goes to memory.
    float* up_mom = nullptr;
    float up_rate = 0.f, up_alpha = 0.f;
    int up_first = 0;
    int vec;            // the 32-channel-chunk K order / 16-byte row gathers apply: Cred % 32 == 0 and at most 16 taps per axis
    int prio_t[3];       // progress thresholds (1/256 of the block's K tiles) at which a block steps its wave priority down; 0 = off
    // tail split (igemm.hip, "tail split"): the LAST tail_n tiles of the launch (the end of the last class in dispatch order) are each
    // contracted by tail_s blocks over disjoint K ranges into compact partial tiles slab[tail tile][split][BM][BN], which
    // tail_reduce_kernel sums in a fixed order and finishes (bias, epilogue, store).  tail_s <= 1: off.
    int tail_from, tail_n, tail_s;
    int nclasses;
    IgemmClass cls[CGS_MAX_CLASSES];
    unsigned char perm[CGS_MAX_CLASSES][256];   // per class: base pixels sorted by descending valid-tap count
};

// i-th tap visited along one axis of an n-tap kernel: natural order, or evens then odds
__host__ __device__ inline int cgs_tap_order(int i, int n, int parity_first) {
    if (!parity_first) return i;
    const int ne = (n + 1) >> 1;
    return i < ne ? 2 * i : 2 * (i - ne) + 1;
}

// GEMM rows of parity class i of a launch
static inline long cgs_igemm_rows(const IgemmParams& p, int i) { return (long)p.B * p.cls[i].R * p.cls[i].C; }
// one launch addresses its tensors with 32-bit byte offsets (the caller splits the batch)
static inline bool cgs_igemm_over_2gib(const IgemmParams& p) {
    return (long)p.B * p.Hout * p.Wout * p.N * 4 > 0x7fffffffL || (long)p.B * p.Hin * p.Win * p.Cred * 4 > 0x7fffffffL;
}
// Fused statistics: one partial row per (128-row tile, wave row), the parity classes back to back (equal M: cgs_conv_stat_layout).
// -> partial rows per class (IgemmParams::stat_cls_rows), -1 = parity classes of unequal size
static inline int cgs_igemm_stat_cls_rows(const IgemmParams& p) {
    const long M0 = cgs_igemm_rows(p, 0);
    for (int i = 1; i < p.nclasses; ++i)
        if (cgs_igemm_rows(p, i) != M0) return -1;
    return (int)(2 * ((M0 + 127) / 128));
}
// Block ids per class (grid x) of a launch of mtiles x nblk_n tiles, and the decode that reads them (IgemmParams::xcd_map; igemm_kernel,
// igemm_bx6_kernel): the per-XCD decode runs over the m-tile count padded to 8
static inline long cgs_igemm_grid_x(long mtiles, int nblk_n, int* xcd_map) {
    *xcd_map = (mtiles % 8 == 0 || mtiles >= 64) ? 1 : 0;        // per-XCD decode only where it keeps the 8 XCDs evenly loaded
    return (*xcd_map ? (mtiles + 7) / 8 * 8 : mtiles) * nblk_n;
}

// geometry builders (igemm.hip)
void cgs_geom_F(const CgsLayer& L, IgemmParams& p);
void cgs_geom_T(const CgsLayer& L, IgemmParams& p);
size_t cgs_packed_floats(const IgemmParams& p);

// launchers
int cgs_pack_weights(const IgemmParams& p, const CgsLayer& L, bool dirT, const float* w, float* packed, hipStream_t s);
int cgs_igemm_launch(const IgemmParams& p, void* slab, size_t slab_bytes, hipStream_t s);
size_t cgs_igemm_splitk_bytes(const IgemmParams& p);   // slab bytes the launch would like for split-K (0 = no split-K)
size_t cgs_igemm_slab_bytes(const IgemmParams& p);     // ... for split-K or the tail split: what a workspace should offer behind the packed weights
void cgs_igemm_row_policy(IgemmParams& p, int BM);     // sets pix_major, lpt, perm (BM = rows of the launch's block tile)
void cgs_igemm_count_flops(const IgemmParams& p, int BM);
// split-bf16 implicit GEMM (igemm_bx6.hip): fp32 operands as three bf16 pieces each, six bf16 MFMA products, fp32 accumulate
int cgs_igemm_bx6_ok(const CgsLayer& L, bool dirT, int B, bool any_size);
size_t cgs_igemm_bx6_packed_bytes(const IgemmParams& p);
int cgs_pack_weights_bx6(const IgemmParams& p, const CgsLayer& L, bool dirT, const float* w, void* packed, hipStream_t s);
int cgs_igemm_bx6_launch(const IgemmParams& p, hipStream_t s);
int cgs_contraction_mode();                             // thread-local: CGS_CONTRACTION_* (api.hip)
// where a launch of this geometry (behind its packed weights: slab_bytes of workspace) would apply the fused momentum update: CGS_UPDATE_* of
// cgs_hip.h, 0 = it cannot (the launcher then refuses up_mom)
int cgs_igemm_update_form(const IgemmParams& p, size_t slab_bytes);
int cgs_igemm_row_order(const IgemmParams& p);       // GEMM row order the launcher will pick: 0 (image, pixel); 1 (pixel, image); 2 (pixel, image) in whole 128-image tiles
// the launch's whole plan for cgs_conv_igemm_plan (form: CGS_FORM_*; 0 = the launcher would refuse the form)
int cgs_igemm_plan_info_of(const IgemmParams& p, int form, size_t slab_bytes, cgs_igemm_plan_info* info, unsigned char* perm);
size_t cgs_convt_quad_ws_floats_bound(int kh, int kw, int Cs);
int cgs_convt_taps_ok(const CgsLayer& L);          // 4x4 stride-2 transposed conv to one channel: all 16 taps as MFMA columns (convt_taps.hip)
int cgs_convt_taps_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias, float* out, int epilogue,
                          const float* ep_a, const float* ep_aux, hipStream_t s);
int cgs_conv_dot_ok(const CgsLayer& L, int epilogue);       // forward conv to <= 4 channels over a deep reduction: a wave per output pixel (conv_dot.hip)
int cgs_conv_dot_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias, float* out, int epilogue,
                        const float* ep_a, const float* ep_b, hipStream_t s);
int cgs_conv_taps_ok(const CgsLayer& L, int epilogue);      // its forward twin: 4x4 stride-2 conv FROM one channel (K = 16)
int cgs_conv_taps_signs_ok(const CgsLayer& L, int epilogue);
int cgs_conv_taps_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias, float* out, int epilogue,
                         const float* ep_a, const float* ep_b, const float* ep_aux, const unsigned* aux_signs, hipStream_t s);
int cgs_convt_quad_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias, float* out,
                          int epilogue, const float* ep_a, const float* ep_aux, float* ws, size_t ws_bytes, int prepacked,
                          hipStream_t s);
int cgs_convt_smalln_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias,
                            float* out, int epilogue, hipStream_t s);

// fused epilogue math shared by the conv-family kernels (device code only): the element epilogue of smallc.h with ocml's tanhf, every mode
#ifdef __HIPCC__
#include "smallc.h"
__device__ __forceinline__ float epilogue_apply(float v, int mode, float a, float b, float aux) { return epilogue_elem<EPI_TANHF>(v, mode, a, b, aux); }

// The element arithmetic of norm + lrelu (bn.hip; the norm-backward statistics of igemm_epilogue.h), each formula once:
//   y  = lrelu(fma(x, scale, shift))                     scale = gamma * invstd, shift = beta - mean * scale
//   d  = dy * lrelu'(fma(x, scale, shift)),              xhat = (x - mean) * invstd
//   dx = scale * (d - m1 - xhat * m2)                    m1 = mean(d), m2 = mean(d * xhat)
__device__ __forceinline__ float norm_fwd1(float x, float sc, float sh, float leak) {
    const float o = fmaf(x, sc, sh);
    return o > 0.f ? o : leak * o;
}
__device__ __forceinline__ float norm_d1(float x, float dy, float sc, float sh, float leak) {
    const float u = fmaf(x, sc, sh);
    return dy * (u > 0.f ? 1.f : leak);
}
// ... d with the two column sums it feeds: sa += d, sb += d * xhat
__device__ __forceinline__ float norm_d_acc1(float x, float dy, float mu, float inv, float sc, float sh, float leak, float& sa, float& sb) {
    const float d = norm_d1(x, dy, sc, sh, leak);
    sa += d; sb = fmaf(d, (x - mu) * inv, sb);
    return d;
}
__device__ __forceinline__ float norm_dx1(float x, float d, float mu, float inv, float sc, float m1, float m2) {
    const float xh = (x - mu) * inv;
    return sc * (d - m1 - xh * m2);
}

// The loss seed of the refinement loop, each formula once (elementwise.hip; the one-logit head of api.hip).
__device__ __forceinline__ float sigmoid_stable(float v) { return v >= 0.f ? 1.f / (1.f + expf(-v)) : expf(v) / (1.f + expf(v)); }
//   d loss / d logit of the unreduced loss (cgs_hip.h, CGS_LOSS_*).  BCE: sigmoid(v) - 1 = -1/(1+exp(v)), written to stay accurate for large |v|
template <int KIND>
__device__ __forceinline__ float loss_seed1(float v) {
    if (KIND == CGS_LOSS_BCE) return v >= 0.f ? -expf(-v) / (1.f + expf(-v)) : -1.f / (1.f + expf(v));
    if (KIND == CGS_LOSS_LSQ) return 2.f * (v - 1.f);
    return -1.f;
}
//   the ladam rule's per-sample state from the sample's score sig = mean_p sigmoid(logit) (cgs_ladam_seed): one thread per sample
__device__ __forceinline__ void ladam_seed1(const cgs_ladam_seed& la, int b, float sig, const float* loss_in = nullptr) {
#pragma clang fp contract(off)   // separately rounded mul / add (policy.py:50,56)
    const float loss = loss_in ? loss_in[b] : la.s_real[0] - sig;
    const float avg = la.first ? loss : 0.5f * la.loss_avg[b] + 0.5f * loss;
    la.loss_avg[b] = avg;
    const float c = fminf(fmaxf(avg + 0.5f, 0.f), 10000.f);
    la.gain[b] = c * c;
}
// The momentum / sgd step of the refinement loop on ONE element, once (policy.py:27-37; the clip: collaborator.py:69-70): m <- alpha * m +
// rate * g (the first step: rate * g), theta <- theta - m.  elementwise.hip's refine_update_kernel and the update epilogues of igemm.hip
// (igemm_epilogue.h, the reduce kernels) call it: sampling/policy.py is bit-exact against the reference's op sequence, so that sequence
// lives here only -- separately rounded mul / add in every caller.
__device__ __forceinline__ void refine_update1(float g, float rate, float alpha, int first, int use_clip, float vmin, float vmax, float& theta,
                                               float& m) {
#pragma clang fp contract(off)
    const float lg = rate * g;
    const float am = alpha * m;
    const float mv = first ? lg : am + lg;
    m = mv;
    float t = theta - mv;
    if (use_clip) t = fminf(fmaxf(t, vmin), vmax);
    theta = t;
}
#endif


// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the DEVICE's code object: set it once per device (a process may drive
// several GPUs) and report a failure instead of letting the launch that follows fail with an unrelated message.
// CGS_SMEM_ATTR(bytes, "who", kernel<template, args>) -- the kernel last, so its commas need no parentheses.
#define CGS_SMEM_ATTR(bytes, who, ...)                                                                                  \
    do {                                                                                                                \
        static bool smem_done_[64] = {};                                                                                \
        int smem_dev_ = 0;                                                                                              \
        (void)hipGetDevice(&smem_dev_);                                                                                 \
        smem_dev_ &= 63;                                                                                                \
        if (!smem_done_[smem_dev_]) {                                                                                   \
            hipError_t smem_e_ = hipFuncSetAttribute((const void*)(__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
            if (smem_e_ != hipSuccess) return cgs_set_error(CGS_ELAUNCH, "%s: MaxDynamicSharedMemorySize: %s", who, hipGetErrorString(smem_e_)); \
            smem_done_[smem_dev_] = true;                                                                               \
        }                                                                                                               \
    } while (0)

// CGS_LAUNCH_T(kernel, (template, args), grid, block, smem, stream, kernel args...): launches kernel<template, args> and notes its name for
// cgs_last_kernel() as rocprofv3 prints it, "kernel<template, args>" -- the argument list stands once, so the name cannot drift from the launch.
#define CGS_TARGS_(...) __VA_ARGS__
#define CGS_STR_(...) #__VA_ARGS__
#define CGS_STR(...) CGS_STR_(__VA_ARGS__)
#define CGS_LAUNCH_T(kernel, targs, grid, block, smem, stream, ...)                                                     \
    do {                                                                                                                \
        hipLaunchKernelGGL((kernel<CGS_TARGS_ targs>), grid, block, smem, stream, __VA_ARGS__);                         \
        cgs_note_kernel(#kernel "<" CGS_STR(CGS_TARGS_ targs) ">");                                                     \
    } while (0)

// Persistent blocks, each a contiguous run of tiles (device side: block_run): ceil(tiles / slots) tiles a block, but never 2 or 3 -- a run
// of >= 4 amortises what a block loads once, and a launch too small for that (< 4 tiles for each of 256 CUs) keeps one tile per block.
static inline void cgs_persistent_run(long tiles, long slots, long* per, long* blocks) {
    *per = (tiles + slots - 1) / slots;
    if (*per < 4) *per = tiles >= 4 * 256 ? 4 : 1;
    *blocks = (tiles + *per - 1) / *per;
}

// the 2-D discriminator at 64 < nhidden <= 256 (mlp2d_wide.hip); arguments already checked by the entry points of mlp2d.hip
int cgs_mlp2d_wide_saliency(const float* const* w, const float* const* b, int nlayers, int nh, const float* x, float* sig, float* sal, int B,
                            float inv_batch, hipStream_t st);
int cgs_refine2d_wide(const float* const* w, const float* const* b, int nlayers, int nh, const float* x, float mean_host,
                      const float* mean_dev, float inv_batch, int steps, float rate, int method, float* best_x, float* best_step,
                      float* traj, int B, hipStream_t st);

bool cgs_convt_quad_fits(const CgsLayer& L);
int cgs_conv_smalln_f_ok(const CgsLayer& L, int B, int epilogue);
size_t cgs_conv_smalln_f_ws_floats(const CgsLayer& L);
int cgs_conv_smalln_f_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias, float* out,
                             int epilogue, float* ws, size_t ws_bytes, int prepacked, hipStream_t s);
int cgs_conv_patch_ok(const CgsLayer& L, int epilogue);
int cgs_conv_patch_T_ok(const CgsLayer& L);          // backward-data of a stride-1 conv with <= 4 output channels
size_t cgs_conv_patch_ws_floats(const CgsLayer& L, bool dirT);
int cgs_conv_patch_launch(const CgsLayer& L, bool dirT, int B, const float* in, const float* w, const float* bias, float* out,
                          int epilogue, const float* ep_a, const float* ep_b, const float* ep_aux, float* ws, size_t ws_bytes,
                          int prepacked, hipStream_t s, const unsigned* aux_signs = nullptr);
int cgs_conv_patch_signs_ok(const CgsLayer& L, bool dirT, int epilogue);     // can the *_BWD epilogue take a sign mask instead of the fp32 aux tensor?
int cgs_igemm_signs_ok(const IgemmParams& p);                                 // can this launch leave the sign mask of its output? (call after the geometry is set)
