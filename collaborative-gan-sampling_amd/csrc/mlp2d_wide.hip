// The 2-D discriminator at 64 < nhidden <= 256 (the reference's 25-Gaussians runs pass --nhidden=256 --nlayers=6): the same function
// as mlp_eval of mlp2d.hip -- logit and d logit / dx of 2 -> nh -> ... -> nh -> 1 with ReLU -- for a TILE of T samples per workgroup.
// Four 256x256 layers and their transposes are 2 MB, so nothing is LDS-resident here but the tile's activations:
//   H [T][nhp]            the activations (forward) or the gradient w.r.t. them (backward), one buffer, rewritten layer by layer
//   forward   H_out = relu(H_in W_l + b_l)      on v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fmaf chain that starts at the bias
//   backward  G_in  = (G_out . mask_l) W_l^T    the same tile shape, the ReLU masks kept as bits [layer][sample][unit]
// W_l streams from global memory (L2-resident: the whole 25-Gaussians D is 1 MB) in slabs of KS = T/2 reduction indices through two LDS
// buffers; the load of slab s+1 is in flight while slab s is contracted.  Both directions read the SAME row-major W_l[k][j]: the
// LDS image of a slab is [output column][reduction index], so the backward (output k, reduction j) copies runs of a row, and the
// forward (output j, reduction k) transposes on its way in: four loads down a column, one 16-byte LDS write.
// Each of the 4 waves owns the 32-column strips wave, wave + 4 of the output and all T rows of them.
// The first layer (2 -> nh), the last (nh -> 1) and their adjoints are VALU, 4 lanes per sample.
//
// nh is padded to nhp, the next multiple of 32 (the MFMA granule), with zero weights and zero bias: a padded unit's pre-activation is
// exactly 0, its mask bit 0, its gradient 0.  Rows past B of the last tile are computed on x = 0 and never stored.
//
// Reduction-index order in LDS: the A / B operand of 32x32x2 is one float per lane, lane half h = lane >> 5 supplying k = 2i + h of step i.
// Storing index k of every group of 8 at position hpos(k) = 4 (k & 1) + (k >> 1) puts the 4 values a lane needs for 4 consecutive steps
// side by side: one ds_read_b128 per operand per 4 MFMAs, and K still walked in ascending order.
//   H rows are padded by 4 floats: row stride = 1 or 9 (mod 16) 16-byte slots, so the 16 rows of a ds_read_b128 lane group hit 16 slots.
//   A slab column is KS floats (NSL = KS/4 slots) unpadded, slot s of column c stored at s ^ ((c / (16/NSL)) % NSL): the 16 columns of a
//   lane group again hit 16 different slots.  (A pad instead would cost 8 KB at T = 32 and the second resident block with it.)
// LDS at nh = 256, 6 layers: T = 64: 142.5 KiB (one block per CU); T = 32: 72.8 KiB (two).
#include "mlp2d_wide.h"

// sigmoid [B] and saliency [B,2] = inv_batch * (sigmoid - 1) * d logit / dx for the tile blockIdx.x
template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void mlp_saliency_wide_kernel(Mlp2dParams p, const float* __restrict__ x, float* __restrict__ sig,
                                                                         float* __restrict__ sal, int B, float inv_batch) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpWLds L = mlpw_lds<T>(smem, p.nlayers, p.nhp);
    mlpw_load(p, L);
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * T;
    if (tid < 2 * T) L.xs[tid] = row0 + (tid >> 1) < B ? x[2 * row0 + tid] : 0.f;
    float logit = 0.f, d0 = 0.f, d1 = 0.f;
    mlpw_eval<T>(p, L, logit, d0, d1);
    const long s = row0 + (tid >> 2);
    if (tid < 4 * T && (tid & 3) == 0 && s < B) {
        const float sg = sigmoid_stable(logit);
        sig[s] = sg;
        if (sal) { sal[2 * s] = inv_batch * (sg - 1.f) * d0; sal[2 * s + 1] = inv_batch * (sg - 1.f) * d1; }
    }
}

// refine2d_kernel of mlp2d.hip for a tile: the 4 lanes of a row all carry that sample's Refine2dState; lane 0 of them posts the moved
// point to xs and stores.
template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void refine2d_wide_kernel(Mlp2dParams p, const float* __restrict__ x_in, float real_mean_host,
                                                                     const float* __restrict__ real_mean_dev, float inv_batch, int steps,
                                                                     float rate, int method, float* __restrict__ best_x,
                                                                     float* __restrict__ best_step, float* __restrict__ traj, int B) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpWLds L = mlpw_lds<T>(smem, p.nlayers, p.nhp);
    mlpw_load(p, L);
    const float real_mean = real_mean_dev ? real_mean_dev[0] : real_mean_host;
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * T, s = row0 + (tid >> 2);
    const bool own = tid < 4 * T, lead = own && (tid & 3) == 0 && s < B;
    float x0 = 0.f, x1 = 0.f;
    if (own && s < B) { x0 = x_in[2 * s]; x1 = x_in[2 * s + 1]; }
    if (own && (tid & 3) == 0) { L.xs[2 * (tid >> 2)] = x0; L.xs[2 * (tid >> 2) + 1] = x1; }
    Refine2dState r(x0, x1);
    float logit = 0.f, d0 = 0.f, d1 = 0.f;
    for (int i = 0; ; ++i) {
        mlpw_eval<T>(p, L, logit, d0, d1);
        r.seen(i, logit, d0, d1, inv_batch, real_mean);
        if (traj && lead) r.record(traj, (size_t)s, steps, i);
        if (i == steps) break;
        r.step(i, method, rate);
        if (own && (tid & 3) == 0) { L.xs[2 * (tid >> 2)] = r.x0; L.xs[2 * (tid >> 2) + 1] = r.x1; }
    }
    if (lead) { best_x[2 * s] = r.bx0; best_x[2 * s + 1] = r.bx1; best_step[s] = r.bs; }
}

// the callers (mlp2d.hip) have checked every argument; 64 < nh <= 256
int cgs_mlp2d_wide_saliency(const float* const* w, const float* const* b, int nlayers, int nh, const float* x, float* sig, float* sal, int B,
                            float inv_batch, hipStream_t st) {
    const Mlp2dParams p = mlp2d_params(w, b, nlayers, nh);
    const int T = mlpw_tile(B);
    return mlpw_launch_tile<mlp_saliency_wide_kernel<32>, mlp_saliency_wide_kernel<64>>(
        T, B, mlpw_smem(T, nlayers, p.nhp), "mlp2d_sigmoid_saliency", "mlp2d_sigmoid_saliency", st, p, x, sig, sal, B, inv_batch);
}

int cgs_refine2d_wide(const float* const* w, const float* const* b, int nlayers, int nh, const float* x, float mean_host,
                      const float* mean_dev, float inv_batch, int steps, float rate, int method, float* best_x, float* best_step,
                      float* traj, int B, hipStream_t st) {
    const Mlp2dParams p = mlp2d_params(w, b, nlayers, nh);
    const int T = mlpw_tile(B);
    return mlpw_launch_tile<refine2d_wide_kernel<32>, refine2d_wide_kernel<64>>(T, B, mlpw_smem(T, nlayers, p.nhp), "refine2d", "refine2d", st, p, x,
                                                                                mean_host, mean_dev, inv_batch, steps, rate, method, best_x,
                                                                                best_step, traj, B);
}
