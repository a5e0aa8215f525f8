// What the 2-D kernels share, narrow (mlp2d.hip: one wave per sample, nhidden <= 64) and wide (mlp2d_wide*.hip: a sample tile per block,
// 64 < nhidden <= 256), each piece stated once:
//   the net        its parameter and variable pointers as a kernel argument, and their fills
//   the refiner    the per-sample state of sampling/refiner_cpu.py's loop and its two operations
//   batch norm     xhat and relu(gamma xhat + beta); how many partials a batched walk keeps in flight
// The shape limits and the refusals are in mlp2d_check.h; the stable sigmoid is sigmoid_stable of cgs_internal.h.
#pragma once
#include "cgs_internal.h"
#include "mlp2d_check.h"

struct Mlp2dParams {
    const float* w[MLP2D_MAX_LAYERS];   // layer l: [din_l][dout_l] row-major (tf.layers.dense kernel)
    const float* b[MLP2D_MAX_LAYERS];
    int nlayers, nh, nhp;               // dims: 2 -> nh -> ... -> nh -> 1 (D) or 2 (G); nhp = nh rounded up to 32 (the wide kernels' MFMA granule)
};

static Mlp2dParams mlp2d_params(const float* const* w, const float* const* b, int nlayers, int nh) {
    Mlp2dParams p;
    for (int l = 0; l < MLP2D_MAX_LAYERS; ++l) { p.w[l] = l < nlayers ? w[l] : nullptr; p.b[l] = l < nlayers ? b[l] : nullptr; }
    p.nlayers = nlayers; p.nh = nh; p.nhp = cgs_round_up(nh, 32);
    return p;
}

// the variables a step updates and where their gradients go
struct Mlp2dVars {
    float* w[MLP2D_MAX_LAYERS];
    float* b[MLP2D_MAX_LAYERS];
    float* gw[MLP2D_MAX_LAYERS];      // may be null
    float* gb[MLP2D_MAX_LAYERS];
};

static Mlp2dVars mlp2d_vars(float* const* w, float* const* b, float* const* gw, float* const* gb, int nlayers) {
    Mlp2dVars q;
    for (int l = 0; l < MLP2D_MAX_LAYERS; ++l) {
        q.w[l] = l < nlayers ? w[l] : nullptr; q.b[l] = l < nlayers ? b[l] : nullptr;
        q.gw[l] = (gw && l < nlayers) ? gw[l] : nullptr; q.gb[l] = (gb && l < nlayers) ? gb[l] : nullptr;
    }
    return q;
}

// ---- the refiner ----------------------------------------------------------------------------------------------------------------------------
// One sample of sampling/refiner_cpu.py:19-81: the point, the best point / loss / step so far, and the state of the update rule
// (policy.py:26-61, numpy branch).  Pass i of a kernel's loop evaluates the point of step i (i = 0: the input), calls seen(i, ..) on what
// it found there and, unless i is the last step, step(i, ..) to move to the point of step i + 1.  method: 0 sgd, 1 momentum, 2 ladam.
struct Refine2dState {
    float x0, x1;
    float bx0, bx1, bl, bs;
    float m0, m1, v0, v1, ll;
    float g0, g1, loss;         // at the current point

    __device__ __forceinline__ Refine2dState(float x0_, float x1_)
        : x0(x0_), x1(x1_), bx0(x0_), bx1(x1_), bl(0.f), bs(0.f), m0(0.f), m1(0.f), v0(0.f), v1(0.f), ll(0.f), g0(0.f), g1(0.f), loss(0.f) {}

    // the loss and its gradient at the current point from D's logit there and d logit / dx; the best point moves only on a strict gain
    __device__ __forceinline__ void seen(int i, float logit, float d0, float d1, float inv_batch, float real_mean) {
#pragma clang fp contract(off)
        const float sg = sigmoid_stable(logit);
        g0 = inv_batch * (sg - 1.f) * d0; g1 = inv_batch * (sg - 1.f) * d1;        // synthetic/GAN.py:108-111
        loss = real_mean - sg;                                                     // refiner_cpu.py:28
        if (i == 0) bl = loss;
        else if (bl - loss > 0.f) { bl = loss; bx0 = x0; bx1 = x1; bs = (float)i; }              // refiner_cpu.py:58-61
    }

    // step i + 1 from the point of step i
    __device__ __forceinline__ void step(int i, int method, float rate) {
#pragma clang fp contract(off)
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
    }

    // the point of step i of sample s into traj [B][steps + 1][2]
    __device__ __forceinline__ void record(float* __restrict__ traj, size_t s, int steps, int i) const {
        traj[(s * (steps + 1) + i) * 2] = x0; traj[(s * (steps + 1) + i) * 2 + 1] = x1;
    }
};

// ---- batch norm (the generators) ---------------------------------------------------------------------------------------------------------------

// The forward's xhat and h = relu(gamma xhat + beta).  Whatever recomputes an activation or a ReLU decision from a stored pre-activation
// calls these two, so a decision (mlp2d_bn_relu(..) > 0) never disagrees with the forward's.
__device__ __forceinline__ float mlp2d_xhat(float a, float mean, float rstd) { return (a - mean) * rstd; }
__device__ __forceinline__ float mlp2d_bn_relu(float xhat, float gamma, float beta) { return fmaxf(fmaf(xhat, gamma, beta), 0.f); }

#define MLP2D_PBATCH 16          // partials fetched per round trip: their consumers are serial chains, their loads need not be
