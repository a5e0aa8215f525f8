// Device pieces shared by the small-channel convolution kernels (convt_quad.hip, convt_taps.hip, conv_patch.hip, convt_smalln.hip,
// conv_smalln_f.hip), each stated once.  cgs_internal.h includes this file: epilogue_apply is an instance of the element epilogue below.
#pragma once
#include <hip/hip_runtime.h>

#include "cgs_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// acc += A * B over the 16 k's two f32x4 fragments hold: four steps of v_mfma_f32_16x16x4_f32, fragment element e = k-quad element e
__device__ __forceinline__ void mfma16x4(f32x4& acc, f32x4 a, f32x4 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// tanh(x) = 1 - 2 / (exp(2x) + 1) on the hardware exp2 / rcp (5 VALU ops; ocml's tanhf is ~25, and every VALU op of an MFMA kernel's
// epilogue costs matrix time on its SIMD): absolute error <= 2.4e-7 over the whole range (1 ulp of exp2 and rcp at results <= 1), +-1 at +-inf
__device__ __forceinline__ float fast_tanh(float x) {
    const float t = __builtin_amdgcn_exp2f(x * 2.885390081777927f);      // exp(2x); inf for large x -> rcp 0 -> 1, 0 for very negative x -> -1
    return 1.f - 2.f * __builtin_amdgcn_rcpf(t + 1.f);
}

// Hand-over of LDS data between the lanes of ONE wave (a staging tile no other wave touches): LDS operations of one wave complete in
// order, so no s_barrier is needed; the fences and the wave barrier only keep the compiler from moving LDS accesses across this point.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the element epilogue (cgs_hip.h, CGS_EPI_*) ----
// TANH says which tanh a kernel uses -- grep for EPI_TANHF / EPI_FAST_TANH to see who uses which.  MODES: the modes the kernel serves
// (bit m = mode m); any other mode stores v as it is, and its arithmetic is not compiled in.
enum { EPI_TANHF = 0, EPI_FAST_TANH = 1 };
constexpr unsigned epi_bit(int mode) { return 1u << mode; }
constexpr unsigned EPI_MODES_ALL = 0x7fu;
static_assert(CGS_EPI_TANH_BWD == 6, "EPI_MODES_ALL and epilogue_elem cover modes 0 .. 6: a new mode needs a case of its own");
constexpr unsigned EPI_MODES_BWD = epi_bit(CGS_EPI_RELU_BWD_AFFINE) | epi_bit(CGS_EPI_LRELU_BWD) | epi_bit(CGS_EPI_TANH_BWD);
constexpr unsigned EPI_MODES_T_FWD = epi_bit(CGS_EPI_LRELU) | epi_bit(CGS_EPI_TANH);      // the transposed kernels' forward modes (no affine_relu: api.hip, smalln_ok)

template <int TANH, unsigned MODES = EPI_MODES_ALL>
__device__ __forceinline__ float epilogue_elem(float v, int mode, float a, float b, float aux) {
    switch (mode) {
        case CGS_EPI_LRELU: if (MODES & epi_bit(CGS_EPI_LRELU)) return fmaxf(v, 0.2f * v); break;
        case CGS_EPI_AFFINE_RELU: if (MODES & epi_bit(CGS_EPI_AFFINE_RELU)) return fmaxf(fmaf(a, v, b), 0.f); break;
        case CGS_EPI_TANH: if (MODES & epi_bit(CGS_EPI_TANH)) return TANH == EPI_FAST_TANH ? fast_tanh(v) : tanhf(v); break;
        case CGS_EPI_RELU_BWD_AFFINE: if (MODES & epi_bit(CGS_EPI_RELU_BWD_AFFINE)) return aux > 0.f ? v * a : 0.f; break;
        case CGS_EPI_LRELU_BWD: if (MODES & epi_bit(CGS_EPI_LRELU_BWD)) return aux > 0.f ? v : 0.2f * v; break;
        case CGS_EPI_TANH_BWD: if (MODES & epi_bit(CGS_EPI_TANH_BWD)) return v * (1.f - aux * aux); break;
        default: break;
    }
    return v;
}

// ---- sign masks, consumer side (cgs_hip.h "sign masks"; the producer is epilogue_rows_signs of igemm_epilogue.h) ----
// A mask holds one 32-bit word per pixel and 32-channel group, a plane of words per group; bit 8e + q <-> channel 4q + e, i.e. bit
// 8 * (c % 4) + (c % 32) / 4 <-> channel c (the producer's lanes hold 4 consecutive channels).  A consumer un-shuffles the word of pixel L
// into lane L as "bit c <-> channel c" (in its own statements: DESIGN.md 31).  Its accumulator register is pixel pix in lanes 0-31 and pixel pix + 4 in lanes 32-63, lane j of a
// half on channel j (v_mfma_f32_32x32x2_f32's C/D layout), so two v_readlane ARE the 64-bit lane mask of "aux > 0":
__device__ __forceinline__ bool sign_lane_positive(unsigned nw, int pix) {
    const unsigned lo = __builtin_amdgcn_readlane(nw, pix), hi = __builtin_amdgcn_readlane(nw, pix + 4);
    return __builtin_amdgcn_inverse_ballot_w64(((unsigned long long)hi << 32) | lo);
}

// ---- buffer descriptors: 32-bit byte offsets, range-checked by the hardware (a load past num_records returns zeros, a store is dropped) ----
constexpr unsigned BUFFER_OOB = 0xFFFFFFF0u;      // the offset a lane passes to read zeros: past every tensor a launch accepts (< 2 GiB)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* ptr, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, (int)bytes, 0x00020000);
}
// num_records 0: every lane reads zeros whatever its offset -- a whole row outside the image without a branch
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc_empty(const void* ptr) { return buffer_rsrc(ptr, 0u); }

// ---- persistent blocks: block blockIdx.x walks items [begin, end) of total, per items a block (the host rule: cgs_persistent_run) ----
__device__ __forceinline__ bool block_run(int per, int total, int& begin, int& end) {
    begin = blockIdx.x * per;
    end = begin + per < total ? begin + per : total;
    return begin < end;
}

// flat index q of a patch of rowf-float rows -> patch row (returned) and element e inside it.  inv_rowf = 1.0f / rowf: the float quotient
// is q / rowf up to one off for q < 2^20, fixed by the two compares (an integer division is ~40 VALU ops)
__device__ __forceinline__ int patch_split(int q, int rowf, float inv_rowf, int& e) {
    int pr = (int)((float)q * inv_rowf);
    if (pr * rowf > q) --pr;
    if ((pr + 1) * rowf <= q) ++pr;
    e = q - pr * rowf;
    return pr;
}
