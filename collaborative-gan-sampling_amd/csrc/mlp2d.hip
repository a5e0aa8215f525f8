// The 2-D path of the reference on the GPU: synthetic/GAN.py:28-37,105-111 (ReLU MLP discriminator on 2-D points,
// its sigmoid and the "saliency" d mean_b softplus(-logit_b) / dx) and the whole host loop of
// sampling/refiner_cpu.py:19-81 (K ladam / momentum / sgd steps with best-loss tracking and trajectory recording)
// as ONE launch: BASELINE config 1 (Imbal-8Gaussians, batch 512, K = 10) without the K+2 host<->framework round trips.
//
// One wave per sample (samples are independent given the real-batch baseline), lane j = hidden unit j (nhidden <= 64):
//   forward  h_out[j] = relu(b[j] + sum_k h_in[k] * W[k][j])   : h_in[k] broadcast by readlane, W row k from LDS
//   backward g_in[k]  = sum_j g_out[j] * W[k][j]               : lane k walks row k of the TRANSPOSED copy W^T[j][k]
// Both LDS walks are stride-1 across lanes (conflict free).  All layers' weights (and transposes) live in LDS.
#include "mlp2d_shared.h"
#include <climits>

__device__ __forceinline__ float bcast(float v, int k) { return __shfl(v, k, 64); }

// LDS layout: per hidden->hidden layer l (1 .. nlayers-2): W [64][64] then W^T [64][64] (zero padded to 64);
// first layer W1 [2][64], b of every layer [64], last layer w [64].
struct MlpLds {
    float* w1;      // [2][64]
    float* wl;      // [64]   last layer column
    float* bias;    // [nlayers][64]
    float* wh;      // [(nlayers-2)][2][64][64]
};

__device__ __forceinline__ MlpLds mlp_lds(float* smem, int nlayers) {
    MlpLds L;
    L.w1 = smem; L.wl = smem + 128; L.bias = smem + 192; L.wh = smem + 192 + nlayers * 64;
    return L;
}

__device__ void mlp_load(const Mlp2dParams& p, const MlpLds& L) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < 128; i += nt) { const int k = i >> 6, j = i & 63; L.w1[i] = j < p.nh ? p.w[0][k * p.nh + j] : 0.f; }
    for (int i = tid; i < 64; i += nt) L.wl[i] = i < p.nh ? p.w[p.nlayers - 1][i] : 0.f;
    for (int i = tid; i < p.nlayers * 64; i += nt) {
        const int l = i >> 6, j = i & 63;
        const int dout = l == p.nlayers - 1 ? 1 : p.nh;
        L.bias[i] = j < dout ? p.b[l][j] : 0.f;
    }
    for (int l = 1; l < p.nlayers - 1; ++l)
        for (int i = tid; i < 4096; i += nt) {
            const int k = i >> 6, j = i & 63;
            const float v = (k < p.nh && j < p.nh) ? p.w[l][k * p.nh + j] : 0.f;
            L.wh[(size_t)(l - 1) * 8192 + i] = v;                       // W[k][j]
            L.wh[(size_t)(l - 1) * 8192 + 4096 + j * 64 + k] = v;       // W^T[j][k]
        }
    __syncthreads();
}

// Forward for the wave's sample at (x0, x1), lane j = hidden unit j: -> the logit.  masks[l] = the ReLU decisions of hidden layer l;
// keep(l, h) sees every hidden activation.
template <class Keep>
__device__ __forceinline__ float mlp_forward(const Mlp2dParams& p, const MlpLds& L, float x0, float x1, int lane,
                                             unsigned long long (&masks)[MLP2D_MAX_LAYERS], Keep&& keep) {
    float h = fmaf(x1, L.w1[64 + lane], fmaf(x0, L.w1[lane], L.bias[lane]));
    masks[0] = __ballot(h > 0.f);
    h = fmaxf(h, 0.f);
    keep(0, h);
    for (int l = 1; l < p.nlayers - 1; ++l) {
        const float* W = L.wh + (size_t)(l - 1) * 8192;
        float a = L.bias[l * 64 + lane];
#pragma unroll 8
        for (int k = 0; k < 64; ++k) a = fmaf(bcast(h, k), W[k * 64 + lane], a);
        masks[l] = __ballot(a > 0.f);
        h = fmaxf(a, 0.f);
        keep(l, h);
    }
    float part = h * L.wl[lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    return part + L.bias[(p.nlayers - 1) * 64];
}

// Backward from g = the gradient w.r.t. the top hidden activation (lane = unit): -> the gradient w.r.t. the first layer's pre-activation;
// keep(l, g) sees the gradient w.r.t. the pre-activation of every hidden layer l.
template <class Keep>
__device__ __forceinline__ float mlp_backward(const Mlp2dParams& p, const MlpLds& L, int lane, const unsigned long long (&masks)[MLP2D_MAX_LAYERS],
                                              float g, Keep&& keep) {
    for (int l = p.nlayers - 2; l >= 1; --l) {
        g = ((masks[l] >> lane) & 1ull) ? g : 0.f;
        keep(l, g);
        const float* WT = L.wh + (size_t)(l - 1) * 8192 + 4096;
        float a = 0.f;
#pragma unroll 8
        for (int jj = 0; jj < 64; ++jj) a = fmaf(bcast(g, jj), WT[jj * 64 + lane], a);
        g = a;
    }
    g = ((masks[0] >> lane) & 1ull) ? g : 0.f;
    keep(0, g);
    return g;
}

// one evaluation for the wave's sample at (x0, x1): logit and d logit / d x
__device__ __forceinline__ void mlp_eval(const Mlp2dParams& p, const MlpLds& L, float x0, float x1, int lane, float& logit,
                                         float& dldx0, float& dldx1) {
    unsigned long long masks[MLP2D_MAX_LAYERS];
    const auto none = [](int, float) {};
    logit = mlp_forward(p, L, x0, x1, lane, masks, none);
    const float g = mlp_backward(p, L, lane, masks, L.wl[lane], none);
    float d0 = g * L.w1[lane], d1 = g * L.w1[64 + lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { d0 += __shfl_xor(d0, off, 64); d1 += __shfl_xor(d1, off, 64); }
    dldx0 = d0; dldx1 = d1;
}

// sigmoid [B] and saliency [B,2] = inv_batch * (sigmoid - 1) * d logit / dx   (synthetic/GAN.py:108-111)
__global__ __launch_bounds__(1024) void mlp_saliency_kernel(Mlp2dParams p, const float* __restrict__ x, float* __restrict__ sig,
                                                            float* __restrict__ sal, int B, float inv_batch) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpLds L = mlp_lds(smem, p.nlayers);
    mlp_load(p, L);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int s = blockIdx.x * nw + wave; s < B; s += gridDim.x * nw) {
        float logit, d0, d1;
        mlp_eval(p, L, x[2 * s], x[2 * s + 1], lane, logit, d0, d1);
        if (lane == 0) {
            const float sg = sigmoid_stable(logit);
            sig[s] = sg;
            if (sal) { sal[2 * s] = inv_batch * (sg - 1.f) * d0; sal[2 * s + 1] = inv_batch * (sg - 1.f) * d1; }
        }
    }
}

// the whole refiner_cpu loop for one sample per wave (Refine2dState of mlp2d_shared.h): pass i evaluates the point of step i
__global__ __launch_bounds__(1024) void refine2d_kernel(Mlp2dParams p, const float* __restrict__ x_in, float real_mean_host,
                                                        const float* __restrict__ real_mean_dev,
                                                        float inv_batch, int steps, float rate, int method,
                                                        float* __restrict__ best_x, float* __restrict__ best_step,
                                                        float* __restrict__ traj /* [B][steps+1][2] or null */, int B) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpLds L = mlp_lds(smem, p.nlayers);
    mlp_load(p, L);
    const float real_mean = real_mean_dev ? real_mean_dev[0] : real_mean_host;      // device scalar: no host round trip per batch
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int s = blockIdx.x * nw + wave; s < B; s += gridDim.x * nw) {
        Refine2dState r(x_in[2 * s], x_in[2 * s + 1]);
        for (int i = 0; ; ++i) {
            float logit, d0, d1;
            mlp_eval(p, L, r.x0, r.x1, lane, logit, d0, d1);
            r.seen(i, logit, d0, d1, inv_batch, real_mean);
            if (traj && lane == 0) r.record(traj, (size_t)s, steps, i);
            if (i == steps) break;
            r.step(i, method, rate);
        }
        if (lane == 0) { best_x[2 * s] = r.bx0; best_x[2 * s + 1] = r.bx1; best_step[s] = r.bs; }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// D shaping step of the 2-D net (synthetic/main.py:366-370 -> synthetic/GAN.py:69-74,98-99):
//   d_loss = mean_b BCE(D(real_b), 1) + mean_b BCE(D(refined_b), 0);  GradientDescentOptimizer(lrd).minimize(d_loss, d_vars)
// Pass A (one wave per sample, the same LDS-resident walk as above): forward keeping every hidden activation, backward
// from the loss seed keeping every pre-activation gradient.  Pass B (one block per layer): dW_l = A_{l-1}^T Delta_l and
// db_l = column sums of Delta_l, summed over the samples in a FIXED order (deterministic), then w -= lr * g in place.
// ------------------------------------------------------------------------------------------------------------------
// acts / deltas: [B_total][nlayers-1][64]; dlast / bce: [B_total]
__global__ __launch_bounds__(1024) void mlp_train_fwdbwd_kernel(Mlp2dParams p, const float* __restrict__ x, int B, int row0, float target,
                                                                float scale, float* __restrict__ acts, float* __restrict__ deltas,
                                                                float* __restrict__ dlast, float* __restrict__ bce) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpLds L = mlp_lds(smem, p.nlayers);
    mlp_load(p, L);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nhid = p.nlayers - 1;
    for (int s = blockIdx.x * nw + wave; s < B; s += gridDim.x * nw) {
        float* A = acts + (size_t)(row0 + s) * nhid * 64;
        float* D = deltas + (size_t)(row0 + s) * nhid * 64;
        unsigned long long masks[MLP2D_MAX_LAYERS];
        const float logit = mlp_forward(p, L, x[2 * s], x[2 * s + 1], lane, masks, [&](int l, float h) { A[l * 64 + lane] = h; });
        const float seed = scale * (sigmoid_stable(logit) - target);            // d (scale * BCE(logit, target)) / d logit
        if (lane == 0) {
            dlast[row0 + s] = seed;
            bce[row0 + s] = scale * (fmaxf(logit, 0.f) - logit * target + log1pf(expf(-fabsf(logit))));
        }
        mlp_backward(p, L, lane, masks, seed * L.wl[lane], [&](int l, float g) { D[l * 64 + lane] = g; });
    }
}

// The sample tile of the two weight-gradient kernels: 64 samples' inputs of a layer and its output gradients
struct MlpGradTile {
    float As[64][65];
    __attribute__((aligned(16))) float Ds[64][64];
};

// block l < nlayers: gradient (+ SGD step) of layer l; block nlayers: the two loss sums.  1024 threads: thread -> row i = t / 16
// of the [din][dout] kernel and 4 columns j4 .. j4+3; the sample dimension is walked in tiles of 64 staged through LDS.
__global__ __launch_bounds__(1024) void mlp_train_grad_kernel(Mlp2dVars q, int nlayers, int nh, const float* __restrict__ xr, int Br,
                                                              const float* __restrict__ xf, int Bf, const float* __restrict__ acts,
                                                              const float* __restrict__ deltas, const float* __restrict__ dlast,
                                                              const float* __restrict__ bce, float lr, float* __restrict__ loss) {
    __shared__ MlpGradTile T;
    const int t = threadIdx.x, Bt = Br + Bf, nhid = nlayers - 1;
    const int l = blockIdx.x;
    if (l == nlayers) {            // d_loss_real, d_loss_fake: fixed-order strided sums + a fixed tree
        float* red = &T.As[0][0];
        for (int part = 0; part < 2; ++part) {
            const int lo = part ? Br : 0, hi = part ? Bt : Br;
            float s = 0.f;
            for (int i = lo + t; i < hi; i += 1024) s += bce[i];
            red[t] = s;
            __syncthreads();
            for (int w = 512; w > 0; w >>= 1) { if (t < w) red[t] += red[t + w]; __syncthreads(); }
            if (t == 0 && loss) loss[part] = red[0];
            __syncthreads();
        }
        return;
    }
    const int din = l == 0 ? 2 : nh, dout = l == nlayers - 1 ? 1 : nh;
    const int i = t >> 4, j4 = (t & 15) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, accb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < Bt; b0 += 64) {
        for (int e = t; e < 4096; e += 1024) {             // stage 64 samples: inputs of the layer and its output gradients
            const int bb = e >> 6, c = e & 63, b = b0 + bb;
            float a = 0.f, d = 0.f;
            if (b < Bt) {
                if (l == 0) { if (c < 2) a = b < Br ? xr[2 * b + c] : xf[2 * (b - Br) + c]; }
                else a = acts[((size_t)b * nhid + (l - 1)) * 64 + c];
                if (l == nlayers - 1) { if (c == 0) d = dlast[b]; }
                else d = deltas[((size_t)b * nhid + l) * 64 + c];
            }
            T.As[bb][c] = a; T.Ds[bb][c] = d;
        }
        __syncthreads();
#pragma unroll 8
        for (int bb = 0; bb < 64; ++bb) {
            const float a = T.As[bb][i];
            const float4 d = *(const float4*)&T.Ds[bb][j4];
            acc[0] = fmaf(a, d.x, acc[0]); acc[1] = fmaf(a, d.y, acc[1]); acc[2] = fmaf(a, d.z, acc[2]); acc[3] = fmaf(a, d.w, acc[3]);
            accb[0] += d.x; accb[1] += d.y; accb[2] += d.z; accb[3] += d.w;
        }
        __syncthreads();
    }
    for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)      // var -= lr * grad as two roundings (GradientDescentOptimizer's ApplyGradientDescent)
        const int j = j4 + e;
        if (i < din && j < dout) {
            const size_t o = (size_t)i * dout + j;
            if (q.gw[l]) q.gw[l][o] = acc[e];
            if (lr != 0.f) q.w[l][o] = q.w[l][o] - lr * acc[e];
        }
        if (i == 0 && j < dout) {
            if (q.gb[l]) q.gb[l][j] = accb[e];
            if (lr != 0.f) q.b[l][j] = q.b[l][j] - lr * accb[e];
        }
    }
}

static size_t mlp_smem(int nlayers) { return (size_t)(192 + nlayers * 64 + (nlayers - 2) * 8192) * sizeof(float); }

// One launch of the wave-per-sample kernel K over B samples: 16 waves a block, at most 256 blocks; the LDS attribute once per kernel and
// device (the flag inside CGS_SMEM_ATTR is this function's, one per K), the launch, its check.  `who` names the entry point, `what` the launch.
template <auto K, class... Args>
static int mlp_launch(int B, int nlayers, const char* who, const char* what, void* stream, const Args&... args) {
    CGS_SMEM_ATTR(160 * 1024, who, K);
    int blocks = (B + 15) / 16; if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(K, dim3(blocks), dim3(1024), mlp_smem(nlayers), (hipStream_t)stream, args...);
    CGS_CHECK_LAUNCH(what);
    return CGS_OK;
}

extern "C" {

int cgs_mlp2d_sigmoid_saliency(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x,
                               float* sigmoid, float* saliency, int B, float inv_batch, void* stream) {
    const int rc = mlp2d_check_net("mlp2d_sigmoid_saliency", w, b, nlayers, nhidden, 1, MLP2D_MAX_NH);
    if (rc) return rc;
    if (B <= 0 || !x || !sigmoid) return cgs_set_error(CGS_EINVAL, "mlp2d_sigmoid_saliency: bad argument");
    if (nhidden > MLP2D_NARROW_MAX_NH) return cgs_mlp2d_wide_saliency(w, b, nlayers, nhidden, x, sigmoid, saliency, B, inv_batch, (hipStream_t)stream);
    return mlp_launch<mlp_saliency_kernel>(B, nlayers, "mlp2d_sigmoid_saliency", "mlp2d_sigmoid_saliency", stream, mlp2d_params(w, b, nlayers, nhidden), x,
                                           sigmoid, saliency, B, inv_batch);
}

static int refine2d_launch(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x, float mean_host,
                           const float* mean_dev, float inv_batch, int steps, float rate, int method, float* best_x, float* best_step,
                           float* traj, int B, void* stream) {
    const int rc = mlp2d_check_net("refine2d", w, b, nlayers, nhidden, 1, MLP2D_MAX_NH);
    if (rc) return rc;
    if (B <= 0 || steps < 0 || method < 0 || method > 2 || !x || !best_x || !best_step) return cgs_set_error(CGS_EINVAL, "refine2d: bad argument");
    if (nhidden > MLP2D_NARROW_MAX_NH)
        return cgs_refine2d_wide(w, b, nlayers, nhidden, x, mean_host, mean_dev, inv_batch, steps, rate, method, best_x, best_step, traj, B,
                                 (hipStream_t)stream);
    return mlp_launch<refine2d_kernel>(B, nlayers, "refine2d", "refine2d", stream, mlp2d_params(w, b, nlayers, nhidden), x, mean_host, mean_dev, inv_batch,
                                       steps, rate, method, best_x, best_step, traj, B);
}

int cgs_refine2d(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x, float real_sigmoid_mean,
                 float inv_batch, int steps, float rate, int method, float* best_x, float* best_step, float* traj, int B,
                 void* stream) {
    return refine2d_launch(w, b, nlayers, nhidden, x, real_sigmoid_mean, nullptr, inv_batch, steps, rate, method, best_x, best_step, traj, B, stream);
}

int cgs_refine2d_devbase(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x,
                         const float* real_sigmoid_mean_dev, float inv_batch, int steps, float rate, int method, float* best_x,
                         float* best_step, float* traj, int B, void* stream) {
    if (!real_sigmoid_mean_dev) return cgs_set_error(CGS_EINVAL, "refine2d_devbase: null baseline pointer");
    return refine2d_launch(w, b, nlayers, nhidden, x, 0.f, real_sigmoid_mean_dev, inv_batch, steps, rate, method, best_x, best_step, traj, B, stream);
}

size_t cgs_mlp2d_train_ws_bytes(int B_total, int nlayers) {
    if (B_total <= 0 || nlayers < 2 || nlayers > MLP2D_MAX_LAYERS) return 0;
    return ((size_t)B_total * (nlayers - 1) * 64 * 2 + (size_t)B_total * 2) * sizeof(float);
}

int cgs_mlp2d_d_step(float* const* w, float* const* b, int nlayers, int nhidden, const float* real, int B_real, const float* fake,
                     int B_fake, float lr, float* const* gw, float* const* gb, float* loss, void* ws, size_t ws_bytes, void* stream) {
    int rc = mlp2d_check_net("mlp2d_d_step", (const float* const*)w, (const float* const*)b, nlayers, nhidden, 1, MLP2D_NARROW_MAX_NH);
    if (rc) return rc;
    if (B_real <= 0 || B_fake <= 0 || !real || !fake) return cgs_set_error(CGS_EINVAL, "mlp2d_d_step: bad argument");
    const int Bt = B_real + B_fake;
    const size_t need = cgs_mlp2d_train_ws_bytes(Bt, nlayers);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "mlp2d_d_step: workspace %zu < %zu bytes", ws_bytes, need);
    float* acts = (float*)ws;
    float* deltas = acts + (size_t)Bt * (nlayers - 1) * 64;
    float* dlast = deltas + (size_t)Bt * (nlayers - 1) * 64;
    float* bce = dlast + Bt;
    const Mlp2dParams p = mlp2d_params((const float* const*)w, (const float* const*)b, nlayers, nhidden);
    for (int part = 0; part < 2; ++part) {      // real rows (target 1) then refined rows (target 0); each loss term is a MEAN
        const int B = part ? B_fake : B_real;
        rc = mlp_launch<mlp_train_fwdbwd_kernel>(B, nlayers, "mlp2d_d_step", "mlp_train_fwdbwd", stream, p, part ? fake : real, B, part ? B_real : 0,
                                                 part ? 0.f : 1.f, 1.f / (float)B, acts, deltas, dlast, bce);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(mlp_train_grad_kernel, dim3(nlayers + 1), dim3(1024), 0, (hipStream_t)stream, mlp2d_vars(w, b, gw, gb, nlayers), nlayers, nhidden,
                       real, B_real, fake, B_fake, acts, deltas, dlast, bce, lr, loss);
    CGS_CHECK_LAUNCH("mlp_train_grad");
    return CGS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// The 2-D generator G (synthetic/GAN.py:39-49): z[B,2] -> dense -> BN -> ReLU -> [dense -> BN -> ReLU] x (nlayers-2) -> dense -> x[B,2],
// BN = tf.contrib.layers.batch_norm(decay=0.9, epsilon=1e-5, scale=True, updates_collections=None).  Unlike D, the batch couples
// every sample at every BN layer, so one launch per dense layer: launch l computes the pre-activations a_l of its samples from
// BN+ReLU of a_{l-1} (L2-resident workspace), and the BN statistics of a_l come from per-wave partials that launch l+1 combines.
//   * wave w owns the CONTIGUOUS samples [w*chunk, min(B, (w+1)*chunk)); lane = unit.  Its partial is (mean_w, M2_w) of its own
//     samples (two passes over values the same lane just wrote); every wave of the next launch combines the W partials in index
//     order (Chan et al.'s pairwise update), so mean / variance are deterministic and free of the E[a^2]-E[a]^2 cancellation.
//   * the dense weights live in registers: lane j keeps column j (forward) or row j (backward) of the layer, and the 64-term dot
//     products broadcast the other operand with v_readlane, no LDS.
// Backward (g_optim, GAN.py:83-101): the BN backward needs two more per-unit batch sums (sum dxhat, sum dxhat*xhat); the same
// partial / combine split, one launch per BN layer from the top down, then one block per dense layer sums its weight and bias
// gradients over the samples in a fixed order and applies w -= lr*g (the D step's mlp_train_grad_kernel pattern).
// ------------------------------------------------------------------------------------------------------------------
#define GEN_WMAX 256          // at most 256 waves (partials) per layer; >= 8 samples per wave below that

// (bcast above and rlane stay two: each kernel family keeps the broadcast it was built and measured on; one helper for both was not tried)
__device__ __forceinline__ float rlane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// (mean, biased variance) of the unit `lane` from the W wave partials [W][2][64], in wave order.  Every wave is non-empty (gen_plan).
__device__ void gen_combine(const float* __restrict__ part, int W, int chunk, int B, int lane, float& mean, float& var) {
    float n = 0.f, m = 0.f, M2 = 0.f;
    for (int p0 = 0; p0 < W; p0 += MLP2D_PBATCH) {
        float pm[MLP2D_PBATCH], pM[MLP2D_PBATCH];
#pragma unroll
        for (int q = 0; q < MLP2D_PBATCH; ++q) {
            const bool in = p0 + q < W;
            pm[q] = in ? part[(size_t)(p0 + q) * 128 + lane] : 0.f;
            pM[q] = in ? part[(size_t)(p0 + q) * 128 + 64 + lane] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < MLP2D_PBATCH; ++q) {
            if (p0 + q >= W) break;
            const float nb = (float)min(chunk, B - (p0 + q) * chunk);
            const float nab = n + nb, d = pm[q] - m;
            m = m + d * (nb / nab);
            M2 = M2 + pM[q] + d * d * (n * nb / nab);
            n = nab;
        }
    }
    mean = m; var = M2 / (float)B;
}

// (sum dxhat, sum dxhat*xhat) of the unit `lane` from the W wave partials, in wave order
__device__ void gen_sum2(const float* __restrict__ part, int W, int lane, float& s1, float& s2) {
    s1 = 0.f; s2 = 0.f;
    for (int p0 = 0; p0 < W; p0 += MLP2D_PBATCH) {
        float a[MLP2D_PBATCH], b[MLP2D_PBATCH];
#pragma unroll
        for (int q = 0; q < MLP2D_PBATCH; ++q) {
            const bool in = p0 + q < W;
            a[q] = in ? part[(size_t)(p0 + q) * 128 + lane] : 0.f;
            b[q] = in ? part[(size_t)(p0 + q) * 128 + 64 + lane] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < MLP2D_PBATCH; ++q) { s1 += a[q]; s2 += b[q]; }
    }
}

struct GenFwd {
    const float* w; const float* b;                    // dense layer l: [din][dout], [dout]
    const float* gamma; const float* beta;             // BN of layer l-1 (l >= 1)
    float* mmean; float* mvar;                         // its moving statistics (read: inference; updated: training)
    const float* z;                                    // l == 0: [B][2]
    const float* pre_in; const float* part_in;         // l >= 1: a_{l-1} [B][64]; training: its wave partials
    float* stats_in;                                   // training: (mean, rstd) of layer l-1 [2][64] for the backward
    float* bstat;                                      // optional: (mean, biased var) of layer l-1 [2][nh]
    float* pre_out; float* part_out;                   // l < nlayers-1: a_l and its partials
    float* x;                                          // l == nlayers-1: [B][2] (may be null)
    int l, nlayers, nh, B, W, chunk, train;
    float eps;
};

__global__ __launch_bounds__(256) void gen_fwd_kernel(GenFwd a) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.W) return;                              // whole waves only
    const bool last = a.l == a.nlayers - 1;
    const int nh = a.nh, din = a.l == 0 ? 2 : nh, dout = last ? 2 : nh;
    float mean = 0.f, rstd = 0.f, gam = 0.f, bet = 0.f;
    if (a.l > 0 && lane < nh) {                        // BN of layer l-1, lane = its unit
        float var;
        if (a.train) gen_combine(a.part_in, a.W, a.chunk, a.B, lane, mean, var);
        else { mean = a.mmean[lane]; var = a.mvar[lane]; }
        rstd = 1.f / sqrtf(var + a.eps);
        gam = a.gamma[lane]; bet = a.beta[lane];
        if (a.train && w == 0) {
#pragma clang fp contract(off)      // assign_moving_average: v -= (v - value) * (1 - decay), decay 0.9 -> 0.1f; moving_variance takes the
                                    // Bessel-corrected batch variance of the fused kernel
            a.stats_in[lane] = mean; a.stats_in[64 + lane] = rstd;
            if (a.bstat) { a.bstat[lane] = mean; a.bstat[nh + lane] = var; }
            const float vu = var * ((float)a.B / (float)(a.B - 1));
            a.mmean[lane] = a.mmean[lane] - (a.mmean[lane] - mean) * 0.1f;
            a.mvar[lane] = a.mvar[lane] - (a.mvar[lane] - vu) * 0.1f;
        }
    }
    float wc[64];
    float bias = 0.f, b0 = 0.f, b1 = 0.f;
    if (!last) {
#pragma unroll
        for (int k = 0; k < 64; ++k) wc[k] = (k < din && lane < dout) ? a.w[k * dout + lane] : 0.f;     // column `lane`
        bias = lane < dout ? a.b[lane] : 0.f;
    } else {
        wc[0] = lane < nh ? a.w[lane * 2] : 0.f;                                                      // row `lane`
        wc[1] = lane < nh ? a.w[lane * 2 + 1] : 0.f;
        b0 = a.b[0]; b1 = a.b[1];
    }
    const int s0 = w * a.chunk, s1 = min(a.B, s0 + a.chunk);
    float sum = 0.f;
    for (int s = s0; s < s1; ++s) {
        if (a.l == 0) {
            const float acc = fmaf(a.z[2 * s + 1], wc[1], fmaf(a.z[2 * s], wc[0], bias));
            a.pre_out[(size_t)s * 64 + lane] = acc;
            sum += acc;
            continue;
        }
        const float h = lane < nh ? mlp2d_bn_relu(mlp2d_xhat(a.pre_in[(size_t)s * 64 + lane], mean, rstd), gam, bet) : 0.f;
        if (!last) {
            float acc = bias;
#pragma unroll
            for (int k = 0; k < 64; ++k) acc = fmaf(rlane(h, k), wc[k], acc);
            a.pre_out[(size_t)s * 64 + lane] = acc;
            sum += acc;
        } else {
            float p0 = h * wc[0], p1 = h * wc[1];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { p0 += __shfl_xor(p0, off, 64); p1 += __shfl_xor(p1, off, 64); }
            if (lane == 0 && a.x) { a.x[2 * s] = p0 + b0; a.x[2 * s + 1] = p1 + b1; }
        }
    }
    if (last || !a.train) return;
    const float mw = sum / (float)(s1 - s0);
    float M2 = 0.f;
    for (int s = s0; s < s1; ++s) { const float d = a.pre_out[(size_t)s * 64 + lane] - mw; M2 = fmaf(d, d, M2); }
    a.part_out[(size_t)w * 128 + lane] = mw;
    a.part_out[(size_t)w * 128 + 64 + lane] = M2;
}

// One BN layer of the backward.  "Upper" is what feeds the gradient down: the output (top: grad_plugin through W_last) or hidden
// layer u (its dxhat -> da, then through W_u).  "Lower" (has_low) is hidden layer l = u-1: dxhat_l = gamma_l * relu'(y_l) * dh_l and
// its wave partials (sum dxhat, sum dxhat*xhat).  dbuf holds dxhat and is overwritten with da in place.
struct GenBwd {
    int top, has_low;
    const float* gplug;                                // top: [B][2]
    const float* w_up;                                 // W_last [nh][2] (top) or W_u [nh][nh]
    const float* part_u; const float* pre_u; const float* stats_u; float* dbuf_u;
    const float* pre_l; const float* stats_l; const float* gamma_l; const float* beta_l; float* dbuf_l; float* part_l;
    int nh, B, W, chunk;
};

__global__ __launch_bounds__(256) void gen_bwd_kernel(GenBwd a) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.W) return;
    const int nh = a.nh;
    const bool on = lane < nh;
    float wr[64];
    float mu = 0.f, ru = 0.f, c1 = 0.f, c2 = 0.f;
    if (a.top) {
        wr[0] = on ? a.w_up[lane * 2] : 0.f;
        wr[1] = on ? a.w_up[lane * 2 + 1] : 0.f;
    } else {
        if (a.has_low) {
#pragma unroll
            for (int j = 0; j < 64; ++j) wr[j] = (on && j < nh) ? a.w_up[lane * nh + j] : 0.f;      // row `lane` of W_u
        }
        if (on) {
            float s1, s2;
            gen_sum2(a.part_u, a.W, lane, s1, s2);
            const float invB = 1.f / (float)a.B;
            c1 = s1 * invB; c2 = s2 * invB;
            mu = a.stats_u[lane]; ru = a.stats_u[64 + lane];
        }
    }
    float ml = 0.f, rl = 0.f, gl = 0.f, bl = 0.f;
    if (a.has_low && on) { ml = a.stats_l[lane]; rl = a.stats_l[64 + lane]; gl = a.gamma_l[lane]; bl = a.beta_l[lane]; }
    const int s0 = w * a.chunk, s1 = min(a.B, s0 + a.chunk);
    float t1 = 0.f, t2 = 0.f;
    for (int s = s0; s < s1; ++s) {
        float dh;
        if (a.top) {
            dh = fmaf(a.gplug[2 * s + 1], wr[1], a.gplug[2 * s] * wr[0]);
        } else {
            const size_t o = (size_t)s * 64 + lane;
            const float xh = on ? mlp2d_xhat(a.pre_u[o], mu, ru) : 0.f;
            const float da = on ? ru * (a.dbuf_u[o] - c1 - xh * c2) : 0.f;        // tf FusedBatchNormGrad, training
            a.dbuf_u[o] = da;
            if (!a.has_low) continue;
            dh = 0.f;
#pragma unroll
            for (int j = 0; j < 64; ++j) dh = fmaf(rlane(da, j), wr[j], dh);
        }
        const size_t o = (size_t)s * 64 + lane;
        float dx = 0.f, xh = 0.f;
        if (on) {
            xh = mlp2d_xhat(a.pre_l[o], ml, rl);
            dx = fmaf(xh, gl, bl) > 0.f ? dh * gl : 0.f;
        }
        a.dbuf_l[o] = dx;
        t1 += dx; t2 = fmaf(dx, xh, t2);
    }
    if (!a.has_low) return;
    a.part_l[(size_t)w * 128 + lane] = t1;
    a.part_l[(size_t)w * 128 + 64 + lane] = t2;
}

struct GenGrad {
    Mlp2dVars v;
    const float* gamma[MLP2D_MAX_LAYERS - 1]; const float* beta[MLP2D_MAX_LAYERS - 1];
    const float* z; const float* gplug; const float* pre; const float* stats; const float* dbuf;
    int nlayers, nh, B;
    float lr;
};

// block l: dW_l = in_l^T da_l, db_l = column sums of da_l (in_0 = z, in_l = relu(BN(a_{l-1})) recomputed exactly as the forward did;
// da of the last layer = grad_plugin), samples in tiles of 64 in a fixed order; then w -= lr*g in place.
__global__ __launch_bounds__(1024) void gen_grad_kernel(GenGrad q) {
    __shared__ MlpGradTile T;
    const int t = threadIdx.x, l = blockIdx.x, nh = q.nh, B = q.B;
    const bool last = l == q.nlayers - 1;
    const int din = l == 0 ? 2 : nh, dout = last ? 2 : nh;
    const int i = t >> 4, j4 = (t & 15) * 4;
    const float* pin = l > 0 ? q.pre + (size_t)(l - 1) * B * 64 : nullptr;
    const float* sl = l > 0 ? q.stats + (size_t)(l - 1) * 128 : nullptr;
    const float* dl = last ? nullptr : q.dbuf + (size_t)l * B * 64;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, accb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += 64) {
        for (int e = t; e < 4096; e += 1024) {
            const int bb = e >> 6, c = e & 63, b = b0 + bb;
            float x = 0.f, d = 0.f;
            if (b < B) {
                if (l == 0) { if (c < 2) x = q.z[2 * b + c]; }
                else if (c < nh) x = mlp2d_bn_relu(mlp2d_xhat(pin[(size_t)b * 64 + c], sl[c], sl[64 + c]), q.gamma[l - 1][c], q.beta[l - 1][c]);
                if (last) { if (c < 2) d = q.gplug[2 * b + c]; }
                else d = dl[(size_t)b * 64 + c];
            }
            T.As[bb][c] = x; T.Ds[bb][c] = d;
        }
        __syncthreads();
#pragma unroll 8
        for (int bb = 0; bb < 64; ++bb) {
            const float x = T.As[bb][i];
            const float4 d = *(const float4*)&T.Ds[bb][j4];
            acc[0] = fmaf(x, d.x, acc[0]); acc[1] = fmaf(x, d.y, acc[1]); acc[2] = fmaf(x, d.z, acc[2]); acc[3] = fmaf(x, d.w, acc[3]);
            accb[0] += d.x; accb[1] += d.y; accb[2] += d.z; accb[3] += d.w;
        }
        __syncthreads();
    }
    for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)      // var -= lr * grad as two roundings (ApplyGradientDescent)
        const int j = j4 + e;
        if (i < din && j < dout) {
            const size_t o = (size_t)i * dout + j;
            if (q.v.gw[l]) q.v.gw[l][o] = acc[e];
            if (q.lr != 0.f) q.v.w[l][o] = q.v.w[l][o] - q.lr * acc[e];
        }
        if (i == 0 && j < dout) {
            if (q.v.gb[l]) q.v.gb[l][j] = accb[e];
            if (q.lr != 0.f) q.v.b[l][j] = q.v.b[l][j] - q.lr * accb[e];
        }
    }
}

// waves per layer and samples per wave: <= GEN_WMAX waves, >= 8 samples each below that, none empty
static void gen_plan(int B, int& W, int& chunk) {
    W = cgs_ceil_div(B, 8);
    if (W > GEN_WMAX) W = GEN_WMAX;
    chunk = cgs_ceil_div(B, W);
    W = cgs_ceil_div(B, chunk);
}

// The workspace, H = nlayers - 1: pre [H][B][64] | part [H][GEN_WMAX][2][64] | stats [H][2][64] | the G step's dbuf [H][B][64]
struct GenWs {
    float* ws;
    size_t H, npre, npart;      // floats of one layer's pre (or dbuf) and of its partials
    GenWs(void* ws_, int B, int nlayers) : ws((float*)ws_), H(nlayers - 1), npre((size_t)B * 64), npart((size_t)GEN_WMAX * 128) {}
    float* pre(int l) const { return ws + l * npre; }
    float* part(int l) const { return ws + H * npre + l * npart; }
    float* stats(int l) const { return ws + H * (npre + npart) + (size_t)l * 128; }
    float* dbuf(int l) const { return ws + H * (npre + npart + 128) + l * npre; }
    size_t floats(int with_backward) const { return H * (npre * (with_backward ? 2 : 1) + npart + 128); }
};

static size_t gen_ws_floats(int B, int nlayers, int with_backward) { return GenWs(nullptr, B, nlayers).floats(with_backward); }

static int gen_forward(const Mlp2dParams& p, const float* const* gamma, const float* const* beta, float* const* mm, float* const* mv,
                       const float* z, float* x, int B, int train, float eps, float* bstat, const GenWs& ws, hipStream_t st) {
    const int nl = p.nlayers;
    int W, chunk;
    gen_plan(B, W, chunk);
    for (int l = 0; l < nl; ++l) {
        GenFwd a = {};
        a.w = p.w[l]; a.b = p.b[l];
        if (l > 0) {
            a.gamma = gamma[l - 1]; a.beta = beta[l - 1]; a.mmean = mm[l - 1]; a.mvar = mv[l - 1];
            a.pre_in = ws.pre(l - 1); a.part_in = ws.part(l - 1); a.stats_in = ws.stats(l - 1);
            a.bstat = bstat ? bstat + (size_t)(l - 1) * 2 * p.nh : nullptr;
        } else {
            a.z = z;
        }
        if (l < nl - 1) { a.pre_out = ws.pre(l); a.part_out = ws.part(l); }
        else a.x = x;
        a.l = l; a.nlayers = nl; a.nh = p.nh; a.B = B; a.W = W; a.chunk = chunk; a.train = train; a.eps = eps;
        hipLaunchKernelGGL(gen_fwd_kernel, dim3(cgs_ceil_div(W, 4)), dim3(256), 0, st, a);
        CGS_CHECK_LAUNCH("mlp2d_gen_fwd");
    }
    return CGS_OK;
}

extern "C" {

size_t cgs_mlp2d_gen_ws_bytes(int B, int nlayers, int with_backward) {
    if (B <= 0 || nlayers < 2 || nlayers > MLP2D_MAX_LAYERS) return 0;
    return gen_ws_floats(B, nlayers, with_backward) * sizeof(float);
}

int cgs_mlp2d_gen_fwd(const float* const* w, const float* const* b, const float* const* gamma, const float* const* beta,
                      float* const* moving_mean, float* const* moving_variance, int nlayers, int nhidden, const float* z, float* x, int B,
                      int is_training, float eps, float* batch_stats, void* ws, size_t ws_bytes, void* stream) {
    int rc = mlp2d_check_net("mlp2d_gen_fwd", w, b, nlayers, nhidden, 1, MLP2D_NARROW_MAX_NH);
    if (rc) return rc;
    if (!x) return cgs_set_error(CGS_EINVAL, "mlp2d_gen_fwd: null output");
    rc = mlp2d_check_gen("mlp2d_gen_fwd", gamma, beta, moving_mean, moving_variance, nlayers, z, B, INT_MAX, is_training != 0, eps,
                         gen_ws_floats(B, nlayers, 0) * sizeof(float), ws, ws_bytes);
    if (rc) return rc;
    return gen_forward(mlp2d_params(w, b, nlayers, nhidden), gamma, beta, moving_mean, moving_variance, z, x, B, is_training != 0, eps,
                       is_training ? batch_stats : nullptr, GenWs(ws, B, nlayers), (hipStream_t)stream);
}

int cgs_mlp2d_g_step(float* const* w, float* const* b, const float* const* gamma, const float* const* beta, float* const* moving_mean,
                     float* const* moving_variance, int nlayers, int nhidden, const float* z, const float* grad_plugin, int B, float eps,
                     float lr, float* const* gw, float* const* gb, float* x, void* ws, size_t ws_bytes, void* stream) {
    int rc = mlp2d_check_net("mlp2d_g_step", (const float* const*)w, (const float* const*)b, nlayers, nhidden, 1, MLP2D_NARROW_MAX_NH);
    if (rc) return rc;
    if (!grad_plugin) return cgs_set_error(CGS_EINVAL, "mlp2d_g_step: null grad_plugin");
    rc = mlp2d_check_gen("mlp2d_g_step", gamma, beta, moving_mean, moving_variance, nlayers, z, B, INT_MAX, 1, eps,
                         gen_ws_floats(B, nlayers, 1) * sizeof(float), ws, ws_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const GenWs s(ws, B, nlayers);
    rc = gen_forward(mlp2d_params((const float* const*)w, (const float* const*)b, nlayers, nhidden), gamma, beta, moving_mean, moving_variance, z, x, B,
                     1, eps, nullptr, s, st);
    if (rc) return rc;
    const int nl = nlayers;
    int W, chunk;
    gen_plan(B, W, chunk);
    // top: output -> layer nl-2; then layer u -> u-1 for u = nl-2 .. 1; then layer 0 alone (its da)
    for (int u = nl - 1; u >= 0; --u) {
        GenBwd a = {};
        a.top = u == nl - 1; a.has_low = u > 0;
        a.w_up = w[u];
        if (a.top) a.gplug = grad_plugin;
        else {
            a.part_u = s.part(u); a.pre_u = s.pre(u); a.stats_u = s.stats(u); a.dbuf_u = s.dbuf(u);
        }
        if (a.has_low) {
            const int l = u - 1;
            a.pre_l = s.pre(l); a.stats_l = s.stats(l); a.gamma_l = gamma[l]; a.beta_l = beta[l]; a.dbuf_l = s.dbuf(l); a.part_l = s.part(l);
        }
        a.nh = nhidden; a.B = B; a.W = W; a.chunk = chunk;
        hipLaunchKernelGGL(gen_bwd_kernel, dim3(cgs_ceil_div(W, 4)), dim3(256), 0, st, a);
        CGS_CHECK_LAUNCH("mlp2d_gen_bwd");
    }
    GenGrad q = {};
    q.v = mlp2d_vars(w, b, gw, gb, nl);
    for (int l = 0; l < nl - 1; ++l) { q.gamma[l] = gamma[l]; q.beta[l] = beta[l]; }
    q.z = z; q.gplug = grad_plugin; q.pre = s.pre(0); q.stats = s.stats(0); q.dbuf = s.dbuf(0);
    q.nlayers = nl; q.nh = nhidden; q.B = B; q.lr = lr;
    hipLaunchKernelGGL(gen_grad_kernel, dim3(nl), dim3(1024), 0, st, q);
    CGS_CHECK_LAUNCH("mlp2d_gen_grad");
    return CGS_OK;
}

}  // extern "C"
