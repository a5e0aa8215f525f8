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
//           | partial small [16][mlpw_small_stride at one output: (nl-1) nhp (db_l) + 2 nhp (dW_0) + nhp (dW_last) + 4 (db_last, loss real, loss fake, 0)]
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
    return 2 * nhid * Bt * nhp + 2 * (size_t)Bt + (size_t)MLPW_MAX_CHUNKS * ((nlayers - 2) * (size_t)nhp * nhp + mlpw_small_stride(nlayers, nhp, 1));
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
    s.Bt = Bt; s.chunk = mlpw_chunk(Bt); s.nchunks = cgs_ceil_div(Bt, s.chunk); s.sstride = mlpw_small_stride(nlayers, nhp, 1);
    return s;
}

template <int T>
__global__ __launch_bounds__(MLPW_THREADS, T == 32 ? 2 : 1) void mlpw_train_kernel(Mlp2dParams p, const float* __restrict__ x, int B, int part0,
                                                                  float target, float scale, MlpWTrainWs ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpWLds L = mlpw_lds<T>(smem, p.nlayers, p.nhp);
    mlpw_load(p, L);
    const int tid = threadIdx.x, nh = p.nh, nhp = p.nhp, nl = p.nlayers, MW = T * (nhp >> 5);
    const long row0 = (long)blockIdx.x * T;
    const int rows = (int)(B - row0 < T ? B - row0 : T);                   // rows of this tile that exist
    const size_t lstride = (size_t)ws.Bt * nhp, base = (size_t)(part0 + row0) * nhp;
    if (tid < 2 * T) L.xs[tid] = (tid >> 1) < rows ? x[2 * row0 + tid] : 0.f;
    __syncthreads();
    // mlpw_eval's composition, H stored after every layer and the top gradient seeded
    mlpw_first<T, true>(L, L.xs, p.w[0], p.b[0], nh, nhp, L.masks);
    __syncthreads();
    mlpw_store_h<T>(L, nhp, ws.acts + base, rows);
    for (int l = 1; l < nl - 1; ++l) {
        mlpw_pass<T, false>(L, nh, nhp, p.w[l], p.b[l], L.masks, l);
        mlpw_store_h<T>(L, nhp, ws.acts + l * lstride + base, rows);
    }
    if (tid < 4 * T) {
        const int row = tid >> 2;
        float v[1];
        mlpw_rowdot<1>(L, L.wlp, nhp, v);
        const float logit = v[0] + p.b[nl - 1][0];
        const float seed = scale * (sigmoid_stable(logit) - target);        // d (scale * BCE(logit, target)) / d logit
        if ((tid & 3) == 0) {
            L.xs[row] = seed;                                              // the points are spent: xs carries the seeds to the top gradient
            if (row < rows) {
                ws.dlast[part0 + row0 + row] = seed;
                ws.bce[part0 + row0 + row] = scale * (fmaxf(logit, 0.f) - logit * target + log1pf(expf(-fabsf(logit))));
            }
        }
    }
    __syncthreads();
    mlpw_top_grad<T, true>(L, L.masks + (nl - 2) * MW, p.w[nl - 1], L.xs, nh, nhp);
    __syncthreads();
    mlpw_store_h<T>(L, nhp, ws.deltas + (nl - 2) * lstride + base, rows);
    for (int l = nl - 2; l >= 1; --l) {
        mlpw_pass<T, true>(L, nh, nhp, p.w[l], nullptr, L.masks, l - 1);
        mlpw_store_h<T>(L, nhp, ws.deltas + (l - 1) * lstride + base, rows);
    }
}

// blocks [0, nmfma): mlpw_wgrad_mfma, the A fragment loaded from acts.
// blocks [nmfma, nmfma + nchunks (nl-1)): (chunk, hidden layer l): thread j < nhp sums column j of Delta_l over the chunk (db_l); l = 0 adds
// x^T Delta_0; l = nl-2 adds A_{nl-2}^T dlast and, in threads 0..2, sum dlast and the two loss sums.
__global__ __launch_bounds__(MLPW_THREADS) void mlpw_wgrad_kernel(MlpWTrainWs ws, int nlayers, int nhp, int nmfma, const float* __restrict__ xr, int Br,
                                                                  const float* __restrict__ xf) {
    const int tid = threadIdx.x, Bt = ws.Bt, nhid = nlayers - 1;
    const size_t lstride = (size_t)Bt * nhp;
    if ((int)blockIdx.x < nmfma) {
        mlpw_wgrad_mfma(nlayers, nhp, Bt, ws.chunk, ws.nchunks, ws.deltas, ws.pw, [&](int hl, int col, bool i1) {
            return [A = ws.acts + hl * lstride + col, i1](size_t o, bool ok, float& a0, float& a1) {
                a0 = ok ? A[o] : 0.f; a1 = (ok && i1) ? A[o + 32] : 0.f;
            };
        });
        return;
    }
    const int sb = blockIdx.x - nmfma, c = sb / nhid, l = sb - c * nhid;
    const int s0 = c * ws.chunk, s1 = min(Bt, s0 + ws.chunk);
    float* S = ws.ps + (size_t)c * ws.sstride;
    if (tid < nhp) {
        const float* D = ws.deltas + l * lstride + tid;
        float db = 0.f, g0 = 0.f, g1 = 0.f;
        mlpw_walk_samples<3>(s0, s1, [&](int ss, bool ok, float (&v)[3]) {
            v[0] = ok ? D[(size_t)ss * nhp] : 0.f;
            v[1] = v[2] = 0.f;
            if (ok && l == 0) {
                const float* xp = ss < Br ? xr + 2 * (size_t)ss : xf + 2 * (size_t)(ss - Br);
                v[1] = xp[0]; v[2] = xp[1];
            }
        }, [&](const float (&v)[3]) { db += v[0]; g0 = fmaf(v[1], v[0], g0); g1 = fmaf(v[2], v[0], g1); });
        S[l * nhp + tid] = db;
        if (l == 0) { S[nhid * nhp + tid] = g0; S[(nhid + 1) * nhp + tid] = g1; }
        if (l == nhid - 1) {
            const float* A = ws.acts + l * lstride + tid;
            // not through mlpw_walk_samples: with it the compiler turns every load of both walks into a branch of its own
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

extern "C" {

size_t cgs_mlp2d_wide_train_ws_bytes(int B_total, int nlayers, int nhidden) {
    if (B_total <= 0 || !mlp2d_shape_ok(nlayers, nhidden, MLP2D_WIDE_MIN_NH, MLP2D_MAX_NH)) return 0;
    return mlpw_train_ws_floats(B_total, nlayers, cgs_round_up(nhidden, 32)) * sizeof(float);
}

int cgs_mlp2d_wide_d_step(float* const* w, float* const* b, int nlayers, int nhidden, const float* real, int B_real, const float* fake,
                          int B_fake, float lr, float* const* gw, float* const* gb, float* loss, void* ws_, size_t ws_bytes, void* stream) {
    int rc = mlp2d_check_net("mlp2d_wide_d_step", (const float* const*)w, (const float* const*)b, nlayers, nhidden, MLP2D_WIDE_MIN_NH, MLP2D_MAX_NH);
    if (rc) return rc;
    if (B_real <= 0 || B_fake <= 0 || (long)B_real + B_fake > (1 << 24) || !real || !fake) return cgs_set_error(CGS_EINVAL, "mlp2d_wide_d_step: bad argument");
    const size_t need = cgs_mlp2d_wide_train_ws_bytes(B_real + B_fake, nlayers, nhidden);
    if (!ws_ || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "mlp2d_wide_d_step: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const Mlp2dParams p = mlp2d_params((const float* const*)w, (const float* const*)b, nlayers, nhidden);
    const int Bt = B_real + B_fake, nhp = p.nhp, nhid = nlayers - 1;
    const MlpWTrainWs ws = mlpw_train_ws((float*)ws_, Bt, nlayers, nhp);
    for (int part = 0; part < 2; ++part) {      // real rows (target 1) then fake rows (target 0); each loss term is a MEAN
        const int B = part ? B_fake : B_real, part0 = part ? B_real : 0, T = mlpw_tile(B);
        rc = mlpw_launch_tile<mlpw_train_kernel<32>, mlpw_train_kernel<64>>(T, B, mlpw_smem(T, nlayers, nhp), "mlp2d_wide_d_step", "mlpw_train", st,
                                                                                p, part ? fake : real, B, part0, part ? 0.f : 1.f, 1.f / (float)B, ws);
        if (rc) return rc;
    }
    const int nmfma = mlpw_wgrad_blocks(nlayers, nhp, ws.nchunks);
    hipLaunchKernelGGL(mlpw_wgrad_kernel, dim3(nmfma + ws.nchunks * nhid), dim3(MLPW_THREADS), 0, st, ws, nlayers, nhp, nmfma, real, B_real, fake);
    CGS_CHECK_LAUNCH("mlpw_wgrad");
    return mlpw_update<1>("mlpw_update", mlp2d_vars(w, b, gw, gb, nlayers), ws.pw, ws.ps, ws.nchunks, nlayers, nhidden, nhp, lr, loss, st);
}

}  // extern "C"
