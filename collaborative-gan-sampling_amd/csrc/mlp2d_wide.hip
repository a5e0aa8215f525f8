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
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void mlp_saliency_wide_kernel(MlpWParams p, const float* __restrict__ x, float* __restrict__ sig,
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
        const float sg = mlpw_sigmoid(logit);
        sig[s] = sg;
        if (sal) { sal[2 * s] = inv_batch * (sg - 1.f) * d0; sal[2 * s + 1] = inv_batch * (sg - 1.f) * d1; }
    }
}

// refine2d_kernel of mlp2d.hip for a tile: the 4 lanes of a row all carry that sample's state; lane 0 of them posts the moved point
// to xs and stores.  The update statements are refine2d_kernel's.
template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void refine2d_wide_kernel(MlpWParams p, const float* __restrict__ x_in, float real_mean_host,
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
    float logit = 0.f, d0 = 0.f, d1 = 0.f, g0 = 0.f, g1 = 0.f, loss = 0.f;
    float bx0 = x0, bx1 = x1, bl = 0.f, bs = 0.f;
    float m0 = 0.f, m1 = 0.f, v0 = 0.f, v1 = 0.f, ll = 0.f;
    // refine2d_kernel's loop turned so that the evaluation stands once in the code: pass i evaluates the point of step i (i = 0: the
    // input), then takes step i + 1 from it
    for (int i = 0; ; ++i) {
#pragma clang fp contract(off)
        mlpw_eval<T>(p, L, logit, d0, d1);
        const float sg = mlpw_sigmoid(logit);
        g0 = inv_batch * (sg - 1.f) * d0; g1 = inv_batch * (sg - 1.f) * d1;
        loss = real_mean - sg;                                     // refiner_cpu.py:28
        if (i == 0) bl = loss;
        else if (bl - loss > 0.f) { bl = loss; bx0 = x0; bx1 = x1; bs = (float)i; }              // refiner_cpu.py:58-61
        if (traj && lead) { traj[((size_t)s * (steps + 1) + i) * 2] = x0; traj[((size_t)s * (steps + 1) + i) * 2 + 1] = x1; }
        if (i == steps) break;
        if (method == 0) {
            x0 -= rate * g0; x1 -= rate * g1;
        } else if (method == 1) {
            const float a0 = rate * g0, a1 = rate * g1;
            m0 = i == 0 ? a0 : 0.9f * m0 + a0; m1 = i == 0 ? a1 : 0.9f * m1 + a1;
            x0 -= m0; x1 -= m1;
        } else {                                                   // ladam, policy.py:39-61
            if (i == 0) { m0 = g0; m1 = g1; v0 = g0 * g0; v1 = g1 * g1; ll = loss; }
            else {
                m0 = 0.9f * m0 + 0.1f * g0; m1 = 0.9f * m1 + 0.1f * g1;        // (1. - 0.9) rounds to 0.1f in float32
                v0 = 0.5f * v0 + 0.5f * (g0 * g0); v1 = 0.5f * v1 + 0.5f * (g1 * g1);
                ll = 0.5f * ll + 0.5f * loss;
            }
            const float c = fmaxf(ll + 0.5f, 0.f);
            const float rs = c * c;
            x0 -= rate * m0 / (sqrtf(v0) + 1e-8f) * rs; x1 -= rate * m1 / (sqrtf(v1) + 1e-8f) * rs;
        }
        if (own && (tid & 3) == 0) { L.xs[2 * (tid >> 2)] = x0; L.xs[2 * (tid >> 2) + 1] = x1; }
    }
    if (lead) { best_x[2 * s] = bx0; best_x[2 * s + 1] = bx1; best_step[s] = bs; }
}

// the callers (mlp2d.hip) have checked every argument; 64 < nh <= 256
int cgs_mlp2d_wide_saliency(const float* const* w, const float* const* b, int nlayers, int nh, const float* x, float* sig, float* sal, int B,
                            float inv_batch, hipStream_t st) {
    MlpWParams p;
    mlpw_fill(p, w, b, nlayers, nh);
    const int T = mlpw_tile(B);
    return mlpw_launch_tile<mlp_saliency_wide_kernel<32>, mlp_saliency_wide_kernel<64>>(
        T, B, mlpw_smem(T, nlayers, p.nhp), "mlp2d_sigmoid_saliency", "mlp2d_sigmoid_saliency", st, p, x, sig, sal, B, inv_batch);
}

int cgs_refine2d_wide(const float* const* w, const float* const* b, int nlayers, int nh, const float* x, float mean_host,
                      const float* mean_dev, float inv_batch, int steps, float rate, int method, float* best_x, float* best_step,
                      float* traj, int B, hipStream_t st) {
    MlpWParams p;
    mlpw_fill(p, w, b, nlayers, nh);
    const int T = mlpw_tile(B);
    return mlpw_launch_tile<refine2d_wide_kernel<32>, refine2d_wide_kernel<64>>(T, B, mlpw_smem(T, nlayers, p.nhp), "refine2d", "refine2d", st, p, x,
                                                                                mean_host, mean_dev, inv_batch, steps, rate, method, best_x,
                                                                                best_step, traj, B);
}
