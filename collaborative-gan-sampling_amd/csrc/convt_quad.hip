// Transposed stride-2 convolution with <= 4 output channels on the fp32 matrix cores, "quad" form:
// the last generator deconv (64 -> 3, nsgan/GAN.py:99 / DCGAN g_h4) and the backward-data of the first
// discriminator conv (3 <- 64, nsgan/GAN.py:64 via sampling/collaborator.py:31).
//
// With N = 3 output channels a per-parity-class GEMM fills 3 of 32 MFMA columns.  Instead one GEMM row
// is an input-resolution pixel ("quad") and its columns are all 2x2 output pixels x N channels of that
// quad (4N <= 16 columns = one v_mfma_f32_16x16x4_f32 tile); K runs over the quad's input neighbourhood
// (<= 3x3 pixels) x Cs channels, with zero weights where a (neighbour, parity) pair has no tap:
//
//   out[b, 2r+py, 2c+px, n] = epi(bias[n] + sum_{dy,dx,ci} in[b, r+dy, c+dx, ci] * Wq[(dy,dx,ci)][(py,px,n)])
//
// 12 of 16 columns and 25 of 36 (neighbour,parity) pairs carry work: ~52 % useful MFMA work instead of ~9 %.
// A fragments are read straight from global memory (each lane one float4 = 4 consecutive ci of its
// row; the K order inside a 16-channel chunk is permuted identically for A and B so no shuffle is
// needed); the packed weights (37 KB for 9 x 64 x 16) sit in LDS for the whole block.
#include "cgs_internal.h"

struct QuadParams {
    const float* in;     // [B,Hs,Ws,Cs]
    const float* wq;     // packed [K/4][16][4], K = ny*nx*Cs
    const float* bias;   // [N] or null
    const float* ep_a;   // [N] for RELU_BWD_AFFINE
    const float* ep_aux; // [B,2Hs,2Ws,N] for the *_BWD epilogues
    float* out;          // [B,2Hs,2Ws,N]
    int B, Hs, Ws, Cs, N;
    int dmin_y, ny, dmin_x, nx;
    int epilogue;
};

// w[kh][kw][N][Cs] -> Wq[(a,bq,ci)][(py,px,n)], a/bq index the neighbourhood rows/cols (dy = dmin_y + a)
__global__ void pack_quad_weights_kernel(const float* __restrict__ w, float* __restrict__ wq, int kh, int kw, int N, int Cs,
                                         int pt, int pl, int dmin_y, int ny, int dmin_x, int nx) {
    const int K = ny * nx * Cs;
    const int total = K * 16;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int e = i & 3, col = (i >> 2) & 15, k = (i >> 6) * 4 + e;
        const int nb = k / Cs, ci = k - nb * Cs;
        const int a = nb / nx, bq = nb - a * nx;
        const int cls = col / N, n = col - cls * N;
        float v = 0.f;
        if (cls < 4) {
            const int py = cls >> 1, px = cls & 1;
            const int ky = py + pt - 2 * (dmin_y + a), kx = px + pl - 2 * (dmin_x + bq);
            if (ky >= 0 && ky < kh && kx >= 0 && kx < kw) v = w[((size_t)(ky * kw + kx) * N + n) * Cs + ci];
        }
        wq[i] = v;
    }
}

template <int MT>
__global__ __launch_bounds__(256) void convt_quad_mfma_kernel(QuadParams p) {
    extern __shared__ __attribute__((aligned(16))) float Bs[];
    const int tid = threadIdx.x;
    const int K = p.ny * p.nx * p.Cs;
    for (int i = tid; i < K * 4; i += 256) ((f32x4*)Bs)[i] = ((const f32x4*)p.wq)[i];
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, i = lane & 15;
    const long HW = (long)p.Hs * p.Ws;
    const long total = (long)p.B * HW;
    const long q0 = ((long)blockIdx.x * 4 + wave) * (16 * MT);
    if (q0 >= total) return;

    int pbase[MT], pr[MT], pc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const long q = q0 + t * 16 + i;
        if (q < total) {
            const int b = (int)(q / HW);
            const int rem = (int)(q - (long)b * HW);
            pr[t] = rem / p.Ws; pc[t] = rem - pr[t] * p.Ws; pbase[t] = b * p.Hs;
        } else {
            pr[t] = -(1 << 20); pc[t] = 0; pbase[t] = 0;
        }
    }
    const int nchunk = p.Cs >> 4;
    const int nit = p.ny * p.nx * nchunk;

    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 a_cur[MT], a_nxt[MT];
#define LOAD_A(dst, it_)                                                                              \
    do {                                                                                              \
        const int nb_ = (it_) / nchunk, ch_ = (it_) - nb_ * nchunk;                                   \
        const int a_ = nb_ / p.nx, b_ = nb_ - a_ * p.nx;                                              \
        const int dy_ = p.dmin_y + a_, dx_ = p.dmin_x + b_;                                           \
        _Pragma("unroll") for (int t = 0; t < MT; ++t) {                                              \
            const int iy = pr[t] + dy_, ix = pc[t] + dx_;                                             \
            f32x4 v = {0.f, 0.f, 0.f, 0.f};                                                           \
            if ((unsigned)iy < (unsigned)p.Hs && (unsigned)ix < (unsigned)p.Ws)                       \
                v = *(const f32x4*)(p.in + ((size_t)(pbase[t] + iy) * p.Ws + ix) * p.Cs + ch_ * 16 + g * 4); \
            dst[t] = v;                                                                               \
        }                                                                                             \
    } while (0)

    LOAD_A(a_cur, 0);
    for (int it = 0; it < nit; ++it) {
        if (it + 1 < nit) LOAD_A(a_nxt, it + 1);
        // B fragment: k-quad (it*4 + g), column i
        const f32x4 fb = *(const f32x4*)(Bs + ((size_t)(it * 4 + g) * 16 + i) * 4);
#pragma unroll
        for (int t = 0; t < MT; ++t) mfma16x4(acc[t], a_cur[t], fb);
#pragma unroll
        for (int t = 0; t < MT; ++t) a_cur[t] = a_nxt[t];
    }
#undef LOAD_A

    // epilogue.  C/D of 16x16x4: col = lane & 15, row = (lane >> 4) * 4 + reg
    const int col = i;
    const int cls = col / p.N, n = col - cls * p.N;
    if (cls >= 4) return;
    const int py = cls >> 1, px = cls & 1;
    const float bias = p.bias ? p.bias[n] : 0.f;
    const float ea = p.epilogue == CGS_EPI_RELU_BWD_AFFINE ? p.ep_a[n] : 1.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long q = q0 + t * 16 + g * 4 + r;
            if (q >= total) continue;
            const int b = (int)(q / HW);
            const int rem = (int)(q - (long)b * HW);
            const int rr = rem / p.Ws, cc = rem - rr * p.Ws;
            float v = acc[t][r] + bias;
            const size_t o = ((size_t)(b * 2 * p.Hs + 2 * rr + py) * (2 * p.Ws) + 2 * cc + px) * p.N + n;
            const float y = p.epilogue >= CGS_EPI_RELU_BWD_AFFINE ? p.ep_aux[o] : 0.f;
            p.out[o] = epilogue_elem<EPI_TANHF, EPI_MODES_T_FWD | EPI_MODES_BWD>(v, p.epilogue, ea, 0.f, y);
        }
}

// ------------------------------------------------------------------------------------------------
// LDS-patch variant: a block owns a TH x TW tile of quads of one image (8 x 32, or 16 x 16 for narrow / ragged grids: tiles may
// hang over the right / bottom edge, their loads read zeros and their stores are clipped).  Per
// 16-channel chunk the (TH+ny-1) x (TW+nx-1) input patch is staged ONCE in LDS (double buffered, the next chunk's
// global loads in flight under the MFMAs) and every neighbour's A fragment is a conflict-free ds_read_b128 from it:
// each input element leaves L2 ~1.3x instead of 9x.  The 4 image rows x 64 pixels x N channels a wave produces
// are transposed through LDS and stored (and the aux tensor loaded) as 16-byte accesses of whole 768-byte rows.
// ------------------------------------------------------------------------------------------------
// Persistent: a block copies the packed weights to LDS ONCE and walks a contiguous run of tiles (image-major: the tiles of an
// image follow each other, so their halo rows are re-read from this CU's L1 / this XCD's L2 instead of from HBM); the patch
// pipeline runs across tile boundaries (chunk 0 of the next tile is fetched under the last chunk's MFMAs of this one).
// NYX = 3: the 3 x 3 neighbourhood of a 5 x 5 (or 4 x 4) stride-2 layer at compile time -- every LDS fragment address is then the
// lane's base plus an instruction immediate; NYX = 0: neighbourhood from the parameters.
// The block's LDS, kernel and launcher alike: packed weights [K/4][16][4] | patch [2][PH][PW][16] (the epilogue stages in a patch buffer)
struct QuadLds {
    static constexpr int PL = 6;                           // float4 of a patch a thread stages: ceil(10*34*4 / 256), ceil(18*18*4 / 256)
    static constexpr int th(int tw) { return 256 / tw; }   // tile height (quads) of a tile tw wide
    static constexpr int ph(int tw, int ny) { return th(tw) + ny - 1; }      // patch rows / cols (pixels)
    static constexpr int pw(int tw, int nx) { return tw + nx - 1; }
    static constexpr int patch_f4(int ph, int pw) { return ph * pw * 4; }    // float4 per 16-channel patch
};

template <int NPAD, int TW, int NYX>   // NPAD = N (<= 4); TW = tile width in quads (32 or 16), tile height 256 / TW
__global__ __launch_bounds__(256, 2) void convt_quad_lds_kernel(QuadParams p, int tiles_total, int tiles_per_block) {
    constexpr int TH = QuadLds::th(TW);
    constexpr int QR = TH / 4;                              // quad rows per wave (2 or 4)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, i = lane & 15;
    const int ny = NYX ? NYX : p.ny, nx = NYX ? NYX : p.nx;
    const int K = ny * nx * p.Cs;
    const int PH = QuadLds::ph(TW, ny), PW = QuadLds::pw(TW, nx);
    const int patch_f4 = QuadLds::patch_f4(PH, PW);
    float* Bs = smem;                                      // [K/4][16][4]
    float* Ps = smem + (size_t)K * 16;                     // [2][PH][PW][16]
    int t_begin, t_end;
    if (!block_run(tiles_per_block, tiles_total, t_begin, t_end)) return;
    for (int q = tid; q < K * 4; q += 256) ((f32x4*)Bs)[q] = ((const f32x4*)p.wq)[q];

    const int tiles_x = (p.Ws + TW - 1) / TW, tiles_y = (p.Hs + TH - 1) / TH;
    const int tpi = tiles_x * tiles_y;

    const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.in, (unsigned)p.B * (unsigned)p.Hs * (unsigned)p.Ws * (unsigned)p.Cs * 4u);
    constexpr int PL = QuadLds::PL;
    f32x4 st[PL];
    int l_pr[PL], l_pc[PL];                                // this thread's patch elements (pixel row / col inside the patch), -2^20 = none
    unsigned l_src[PL];                                    // ... and their byte offset relative to the patch origin pixel, chunk 0
#pragma unroll
    for (int u = 0; u < PL; ++u) {
        const int q = tid + 256 * u;
        const int pixel = q >> 2;
        const int pr = pixel / PW, pc = pixel - pr * PW;
        l_pr[u] = q < patch_f4 ? pr : -(1 << 20); l_pc[u] = pc;
        l_src[u] = (unsigned)(((pr * p.Ws + pc) * p.Cs + (q & 3) * 4) * 4);
    }
    const int nchunk = p.Cs >> 4;
    unsigned okmask = 0;                                   // bit u: element u of the CURRENTLY LOADING tile lies inside the image
#define TILE_DECODE(t_, b_, r0_, c0_)                                                                       \
    do {                                                                                                    \
        b_ = (t_) / tpi;                                                                                    \
        const int trem_ = (t_) - b_ * tpi;                                                                  \
        r0_ = (trem_ / tiles_x) * TH; c0_ = (trem_ - (trem_ / tiles_x) * tiles_x) * TW;                     \
    } while (0)
    // validity of this thread's elements for the tile at (r0_, c0_): once per tile, not per chunk
#define PATCH_VALID(r0_, c0_)                                                                              \
    do {                                                                                                    \
        okmask = 0;                                                                                         \
        _Pragma("unroll") for (int u = 0; u < PL; ++u)                                                      \
            if ((unsigned)((r0_) + l_pr[u] + p.dmin_y) < (unsigned)p.Hs && (unsigned)((c0_) + l_pc[u] + p.dmin_x) < (unsigned)p.Ws) okmask |= 1u << u; \
    } while (0)
#define LOAD_PATCH(b_, r0_, c0_, ch_)                                                                      \
    do {                                                                                                    \
        const unsigned org_ = (unsigned)(((((b_) * p.Hs + (r0_) + p.dmin_y) * p.Ws + (c0_) + p.dmin_x) * p.Cs + (ch_) * 16) * 4);   /* scalar */ \
        _Pragma("unroll") for (int u = 0; u < PL; ++u) {                                                    \
            const unsigned off = (okmask >> u) & 1u ? org_ + l_src[u] : BUFFER_OOB;                        \
            st[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off, 0, 0));   \
        }                                                                                                   \
    } while (0)
#define STORE_PATCH(buf_)                                                                                  \
    _Pragma("unroll") for (int u = 0; u < PL; ++u) {                                                       \
        const int q = tid + 256 * u;                                                                       \
        if (q < patch_f4) ((f32x4*)(Ps + (size_t)(buf_) * patch_f4 * 4))[q] = st[u];                       \
    }

    int b, r0, c0;
    TILE_DECODE(t_begin, b, r0, c0);
    PATCH_VALID(r0, c0);
    LOAD_PATCH(b, r0, c0, 0);
    STORE_PATCH(0);
    __syncthreads();
    constexpr int N = NPAD;
    const int rowf = 2 * TW * N;                           // floats per output image row of the tile
    const int cls = i / N, n = i - cls * N;
    const float bias = (cls < 4 && p.bias) ? p.bias[n] : 0.f;
    int buf = 0;
    for (int t = t_begin; t < t_end; ++t) {
        int nb = b, nr0 = r0, nc0 = c0;
        const bool more = t + 1 < t_end;
        if (more) TILE_DECODE(t + 1, nb, nr0, nc0);
        f32x4 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ch = 0; ch < nchunk; ++ch) {
            const bool last = ch + 1 == nchunk;
            const bool fetch = !last || more;                               // next chunk of this tile, or chunk 0 of the next tile
            if (fetch) {
                if (!last) { LOAD_PATCH(b, r0, c0, ch + 1); }
                else { PATCH_VALID(nr0, nc0); LOAD_PATCH(nb, nr0, nc0, 0); }
            }
            const float* P = Ps + (size_t)buf * patch_f4 * 4;
#pragma unroll
            for (int a = 0; a < ny; ++a)
#pragma unroll
                for (int bq = 0; bq < nx; ++bq) {
                    const int it = (a * nx + bq) * nchunk + ch;            // k-quad group index of (neighbour, chunk)
                    const f32x4 fb = *(const f32x4*)(Bs + ((size_t)(it * 4 + g) * 16 + i) * 4);
                    f32x4 fa[4];
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int pr = (TW == 32 ? 2 * wave + (tt >> 1) : 4 * wave + tt) + a, pc = (TW == 32 ? 16 * (tt & 1) : 0) + i + bq;
                        fa[tt] = *(const f32x4*)(P + ((size_t)(pr * PW + pc) * 4 + g) * 4);
                    }
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) mfma16x4(acc[tt], fa[tt], fb);
                }
            if (fetch) { STORE_PATCH(buf ^ 1); }
            __syncthreads();
            buf ^= 1;
        }
        // ---- epilogue: transpose the wave's image rows x (2 TW px x N) through LDS, then 16-byte row accesses.  The staging
        // area is the patch buffer the last chunk was read from (buf ^ 1 now: free since the barrier above; the other buffer
        // already holds chunk 0 of the next tile) ----
        float* E = Ps + (size_t)(buf ^ 1) * patch_f4 * 4 + (size_t)wave * 2 * QR * rowf;      // [2*QR image rows][2*TW*N]
        if (cls < 4) {
            const int py = cls >> 1, px = cls & 1;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = (TW == 32 ? 16 * (tt & 1) : 0) + g * 4 + r;    // quad column inside the tile
                    E[(2 * (TW == 32 ? (tt >> 1) : tt) + py) * rowf + (2 * c + px) * N + n] = acc[tt][r] + bias;
                }
        }
        wave_lds_sync();
        const int f4_per_row = rowf / 4;                       // 48 for N = 3, TW = 32
        const int live_f = 2 * (p.Ws - c0 < TW ? p.Ws - c0 : TW) * N;      // floats of a tile row that lie inside the image
        for (int q = lane; q < 2 * QR * f4_per_row; q += 64) {
            const int yr = q / f4_per_row, xq = q - yr * f4_per_row;
            const int y = 2 * (r0 + QR * wave) + yr;
            if (y >= 2 * p.Hs || xq * 4 >= live_f) continue;
            const size_t o = ((size_t)(b * 2 * p.Hs + y) * (2 * p.Ws) + 2 * c0) * N + xq * 4;
            f32x4 v = *(const f32x4*)(E + yr * rowf + xq * 4);
            if (p.epilogue == CGS_EPI_TANH) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fast_tanh(v[e]);
            } else if (p.epilogue == CGS_EPI_LRELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.2f * v[e]);
            } else if (p.epilogue >= CGS_EPI_RELU_BWD_AFFINE) {
                const f32x4 y4 = *(const f32x4*)(p.ep_aux + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (p.epilogue == CGS_EPI_TANH_BWD) v[e] *= (1.f - y4[e] * y4[e]);
                    else if (p.epilogue == CGS_EPI_LRELU_BWD) v[e] = y4[e] > 0.f ? v[e] : 0.2f * v[e];
                    else v[e] = y4[e] > 0.f ? v[e] * p.ep_a[(xq * 4 + e) % N] : 0.f;
                }
            }
            *(f32x4*)(p.out + o) = v;
        }
        if (more) __syncthreads();          // every wave is done with its staging rows before the next tile's chunk 1 lands there
        b = nb; r0 = nr0; c0 = nc0;
    }
#undef TILE_DECODE
#undef PATCH_VALID
#undef LOAD_PATCH
#undef STORE_PATCH
}

// ------------------------------------------------------------------------------------------------
// "Rows" form (the fast path for kw * N <= 16, e.g. the 5x5 64 -> 3 layers of every DCGAN here): the quad form above spends
// 48 % of its MFMA work on structural zeros (12 of 16 columns, 25 of 36 (neighbour, parity) pairs).  Here the vertical taps are
// folded into K EXACTLY (an output row of parity py sums over the ky of that parity: 2 + 3 = kh row taps for a row PAIR, no
// zero rows) and the horizontal taps become the GEMM's columns, (kx, n) = kw * N of 16:
//
//   Q[Y][c][(kx, n)] = sum_{ky = Y + pt - 2r, ci} in[b, r, c, ci] * w[ky][kx][n][ci]              (MFMA, 94 % useful for 5x5x3)
//   out[b, Y, X, n]  = epi(bias[n] + sum_{kx = X + pl - 2c} Q[Y][c][(kx, n)])                     (<= 3 terms, from LDS)
//
// One wave owns TWO consecutive output row pairs (rows 2R0 .. 2R0+3) of one image: M = the Ws input pixels of a row (MT tiles of
// 16), its A fragments come straight from global memory (each lane one float4 = 4 channels of its pixel; the ny + 1 = 4 input rows
// are read once for both pairs, and again by the neighbouring task that shares two of them -> L1/L2), the packed weights
// (kh * Cs * 16 floats, 20 KB) sit in LDS for the whole persistent block, and the waves never synchronise with each other.  The
// horizontal gather runs through a per-wave LDS staging tile with a per-lane plan kept in an LDS table; the summation order is
// fixed (deterministic).  Reference semantics: tf.nn.conv2d_transpose 'SAME' (nsgan/ops.py:48-67) and the conv's
// Conv2DBackpropInput (sampling/collaborator.py:31).
// ------------------------------------------------------------------------------------------------
struct RowsParams {
    const float* in;     // [B,Hs,Ws,Cs]
    const float* wp;     // packed [kh*Cs/4][16][4]: k = ky*Cs + ci, column = kx*N + n
    const float* bias;   // [N] or null
    const float* ep_a;   // [N] for RELU_BWD_AFFINE
    const float* ep_aux; // [B,2Hs,2Ws,N] for the *_BWD epilogues
    float* out;          // [B,2Hs,2Ws,N]
    int B, Hs, Ws, Cs;
    int kh, kw, pt, pl;
    int dmin_y, ny;      // input rows R + dmin_y .. R + dmin_y + ny - 1 feed the output row pair (2R, 2R+1)
    int epilogue;
};

// w[kh][kw][N][Cs] -> Wp[(ky*Cs + ci)/4][col = kx*N + n][(ky*Cs + ci)%4]
__global__ void pack_rows_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int kh, int kw, int N, int Cs) {
    const int total = kh * Cs * 16;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int e = i & 3, col = (i >> 2) & 15, k = (i >> 6) * 4 + e;
        const int ky = k / Cs, ci = k - ky * Cs;
        const int kx = col / N, n = col - kx * N;
        wp[i] = kx < kw ? w[((size_t)(ky * kw + kx) * N + n) * Cs + ci] : 0.f;
    }
}

// S5: the geometry of a 5x5 'SAME' layer with 64 input channels at compile time (kh = 5, pt = 1, rows R0-1 .. R0+2, 4 chunks): the 16
// (row, chunk) steps of a task become straight-line code -- which row taps apply to a step is known, the loads of step s + 2
// are in flight under the MFMAs of step s with exact vmcnt waits (with the generic form's uniform branches the compiler waits
// for vmcnt(0) before every MFMA group, which serialises loads and matrix work: 133 us instead of 9x for dcgan64's g_h4)
// NP: output row pairs per task.  2 (round 2): 4 input rows per 2 pairs, every input row read by two tasks (HBM bytes 475 MB for
// 319 algorithmic on dcgan64's g_h4).  4: 6 input rows per 4 pairs -- a quarter fewer loads, 1.5 reads per row instead of 2 -- for
// twice the accumulators (64 VGPRs; the launch runs two blocks = 4 waves per SIMD anyway, so 128 VGPRs are there).
// AUXE: the *_BWD epilogues (an aux tensor of the output's shape); compiled apart so that the forward form carries no aux registers.
// A block's LDS, kernel and launcher alike: packed weights [kh*Cs/4][16][4] | NWV staging tiles | Tg, Tb [NU][64][4] | Tq [NU][64].
// Staging of one output row pair: [2 rows][SP pixels = -2 .. 16 MT][SL floats]; the pixels < 0 and >= Ws and the columns >= 16 stay
// zero, so the gather needs no bounds: its three terms are the lane's base address + instruction immediates.
struct RowsLds {
    static constexpr int NWV = 8, SL = 20;                                          // waves per block, floats per staged pixel
    static constexpr int sp(int mt) { return mt * 16 + 3; }
    static constexpr int sw(int mt) { return 2 * sp(mt) * SL; }                     // floats of a wave's staging tile
    static constexpr int nu(int n, int mt) { return (2 * (2 * mt * 16 * n / 4) + 63) / 64; }      // float4 of a row pair per lane
    static constexpr size_t floats(size_t wfl, int n, int mt) { return wfl + (size_t)NWV * sw(mt) + (size_t)nu(n, mt) * 64 * 9; }
};

template <int N, int MT, bool S5, int NP, bool AUXE>   // N output channels, MT 16-pixel tiles per input row (Ws <= 16 * MT)
__global__ __launch_bounds__(512, 4) void convt_rows_kernel(RowsParams p, int tasks_total, int tasks_per_block) {
    const int kh = S5 ? 5 : p.kh, pt = S5 ? 1 : p.pt, dmin_y = S5 ? -1 : p.dmin_y, ny = S5 ? 3 : p.ny;
    constexpr int NYO = 2 * NP;                             // output rows per task
    constexpr int NWV = RowsLds::NWV, SL = RowsLds::SL, SP = RowsLds::sp(MT), SW = RowsLds::sw(MT), NU = RowsLds::nu(N, MT);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (tells the compiler it is wave-uniform: task indices, row offsets and descriptors stay in SGPRs)
    const int g = lane >> 4, i = lane & 15;
    float* Wl = smem;
    float* S = smem + (size_t)kh * p.Cs * 16 + (size_t)wave * SW;
    int t_begin, t_end;
    if (!block_run(tasks_per_block, tasks_total, t_begin, t_end)) return;
    for (int q = tid; q < kh * p.Cs * 4; q += 64 * NWV) ((f32x4*)Wl)[q] = ((const f32x4*)p.wp)[q];
    for (int q = lane; q < SW; q += 64) S[q] = 0.f;
    __syncthreads();

    const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.in, (unsigned)p.B * (unsigned)p.Hs * (unsigned)p.Ws * (unsigned)p.Cs * 4u);
    const __amdgpu_buffer_rsrc_t null_rsrc = buffer_rsrc_empty(p.in);
    // loop-invariant per-lane part of the A addresses: pixel (16m + i), channels 4g.. (past the row -> out of range -> zeros)
    unsigned coff[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) coff[m] = 16 * m + i < p.Ws ? (unsigned)(((16 * m + i) * p.Cs + 4 * g) * 4) : BUFFER_OOB;
    // gather plan of this lane: float4 q = lane + 64u of a row pair -> output row yr, floats 4xq..4xq+3 of that row; each float
    // (X, n) sums Q[yr][c][(kx, n)] over kx = kx0, kx0 + 2, kx0 + 4 with kx0 = (X + pl) & 1 and 2c = X + pl - kx: one step in kx
    // is one pixel down and 2N columns up, a constant stride, and every out-of-range term lands on a zero of the staging tile
    // (c < 0 or >= Ws: zero pixels; kx >= kw: zero-weight column 15 or the never-written columns 16..19).  goff is the address
    // of the LAST term (lowest address), the others are immediates.
    const int f4_per_row = 2 * p.Ws * N / 4;
    constexpr int GSTEP = SL - 2 * N;                       // floats from term kx + 2 to term kx
    // (the plan depends on the lane only: it lives in LDS, one copy per block, and is read back per row pair -- its 18 values per
    // lane would otherwise sit in VGPRs through the K loop)
    int* Tg = (int*)(smem + (size_t)kh * p.Cs * 16 + (size_t)NWV * SW);       // [NU][64][4] staging offsets of the last term
    float* Tb = (float*)(Tg + NU * 64 * 4);                                        // [NU][64][4] bias of each float
    int* Tq = (int*)(Tb + NU * 64 * 4);                                            // [NU][64] float offset of the float4 inside the row pair's output, -1 = none
    if (wave == 0) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int q = lane + 64 * u;
            const int yr = q / f4_per_row, xq = q - yr * f4_per_row;
            Tq[u * 64 + lane] = q < 2 * f4_per_row ? yr * (2 * p.Ws * N) + xq * 4 : -1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = xq * 4 + e;
                const int X = f / N, n = f - X * N;
                Tb[(u * 64 + lane) * 4 + e] = p.bias ? p.bias[n] : 0.f;
                const int kx = ((X + p.pl) & 1) + 4;            // the last of the three terms
                const int c = (X + p.pl - kx) >> 1;             // exact (even numerator); -2 <= c <= Ws for kw <= 6 (pl <= 2)
                Tg[(u * 64 + lane) * 4 + e] = q < 2 * f4_per_row ? ((yr * SP + c + 2) * SL + kx * N + n) : 0;
            }
        }
    }
    __syncthreads();
    const int nchunk = S5 ? 4 : p.Cs >> 4;
    const int nrow = ny + NP - 1;                         // input rows feeding NP consecutive output row pairs
    constexpr int NIT5 = (3 + NP - 1) * 4;                // S5: (row, chunk) steps of a task
    const int nit = S5 ? NIT5 : nrow * nchunk;
    const size_t out_row = (size_t)2 * p.Ws * N;

    // a task = NP consecutive output row pairs (R0 .. R0 + NP - 1) of one image: the ny + NP - 1 input rows R0 + dmin_y .. are read
    // once for all of them (a row pair alone needs 3), the packed weights of a row tap serve both M tiles
    const int pairs_y = (p.Hs + NP - 1) / NP;
    for (int t = t_begin + wave; t < t_end; t += NWV) {
        const int b = t / pairs_y, R0 = (t - b * pairs_y) * NP;
        f32x4 acc[NYO][MT];
#pragma unroll
        for (int y = 0; y < NYO; ++y)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[y][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 a0[MT], a1[MT], a2[MT];
#define ROWS_LOAD_A(dst, it_)                                                                              \
    do {                                                                                                    \
        const int d_ = (it_) / nchunk, j_ = (it_) - d_ * nchunk;                                            \
        const int rr_ = R0 + dmin_y + d_;                                                                 \
        /* a row outside the image reads through the EMPTY descriptor (num_records 0: every lane gets zeros): no branch */ \
        const bool rok_ = (unsigned)rr_ < (unsigned)p.Hs;                                                   \
        const unsigned sb_ = rok_ ? (unsigned)((((b * p.Hs + rr_) * p.Ws) * p.Cs + 16 * j_) * 4) : 0u;   /* scalar */ \
        _Pragma("unroll") for (int m = 0; m < MT; ++m)                                                      \
            dst[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rok_ ? in_rsrc : null_rsrc, coff[m], sb_, 0)); \
    } while (0)
#define ROWS_MFMA(a_, acc_, ky_, j_)                                                                        \
    do {                                                                                                    \
        const f32x4 fb = *(const f32x4*)(Wl + ((size_t)((((ky_) * p.Cs) >> 2) + 4 * (j_) + g) * 16 + i) * 4); \
        _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                                    \
            acc_[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_[m].x, fb.x, acc_[m], 0, 0, 0);                \
            acc_[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_[m].y, fb.y, acc_[m], 0, 0, 0);                \
            acc_[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_[m].z, fb.z, acc_[m], 0, 0, 0);                \
            acc_[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_[m].w, fb.w, acc_[m], 0, 0, 0);                \
        }                                                                                                   \
    } while (0)
    // input row R0 + dmin_y + d feeds output row 2 R0 + y through the row tap ky = pt - 2 (dmin_y + d) + y (if that is a tap)
#define ROWS_STEP(a_, it_)                                                                                  \
    do {                                                                                                    \
        const int d_ = (it_) / nchunk, j_ = (it_) - d_ * nchunk;                                            \
        const int ky_ = pt - 2 * (dmin_y + d_);                                                         \
        _Pragma("unroll") for (int y = 0; y < NYO; ++y)                                                     \
            if ((unsigned)(ky_ + y) < (unsigned)kh) ROWS_MFMA(a_, acc[y], ky_ + y, j_);                   \
    } while (0)
        // the aux values of the backward epilogues (NP = 2: the first row pair's are requested before the K loop, the next pair's
        // before the current pair's gather; the tall form has no registers for a second set and requests each pair's before its
        // accumulators go through the staging tile)
        constexpr bool AUX2 = AUXE && NP == 2;
        f32x4 aux[AUXE ? NU : 1], aux_n[AUX2 ? NU : 1];
        if constexpr (AUX2) {
            const size_t o0 = ((size_t)(b * 2 * p.Hs + 2 * R0)) * out_row;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int gq0 = Tq[u * 64 + lane];
                if (gq0 >= 0) aux[u] = *(const f32x4*)(p.ep_aux + o0 + gq0);
            }
        }
        ROWS_LOAD_A(a0, 0);
        if (1 < nit) ROWS_LOAD_A(a1, 1);
#pragma unroll
        for (int it = 0; it < (S5 ? NIT5 : nit); it += 3) {   // two steps of loads in flight under each step's MFMAs
            // (sched_barrier: left alone, the scheduler hoists the straight-line form's fragment reads and loads far ahead and spills)
            if (it + 2 < nit) ROWS_LOAD_A(a2, it + 2);
            if (S5) __builtin_amdgcn_sched_barrier(0);
            ROWS_STEP(a0, it);
            if (S5) __builtin_amdgcn_sched_barrier(0);
            if (it + 1 < nit) {
                if (it + 3 < nit) ROWS_LOAD_A(a0, it + 3);
                if (S5) __builtin_amdgcn_sched_barrier(0);
                ROWS_STEP(a1, it + 1);
                if (S5) __builtin_amdgcn_sched_barrier(0);
            }
            if (it + 2 < nit) {
                if (it + 4 < nit) ROWS_LOAD_A(a1, it + 4);
                if (S5) __builtin_amdgcn_sched_barrier(0);
                ROWS_STEP(a2, it + 2);
                if (S5) __builtin_amdgcn_sched_barrier(0);
            }
        }
#undef ROWS_LOAD_A
#undef ROWS_MFMA
#undef ROWS_STEP
#pragma unroll
        for (int hp = 0; hp < NP; ++hp) {                   // the row pairs, one after the other through the staging tile
            if (R0 + hp >= p.Hs) break;
            const size_t o_pair = ((size_t)(b * 2 * p.Hs + 2 * (R0 + hp))) * out_row;
            int gq[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) gq[u] = Tq[u * 64 + lane];
            if constexpr (AUX2) {     // this pair's aux values were requested one pair ago; request the next pair's now
                if (hp > 0) {
#pragma unroll
                    for (int u = 0; u < NU; ++u) aux[u] = aux_n[u];
                }
                if (hp + 1 < NP && R0 + hp + 1 < p.Hs) {
#pragma unroll
                    for (int u = 0; u < NU; ++u)
                        if (gq[u] >= 0) aux_n[u] = *(const f32x4*)(p.ep_aux + o_pair + 2 * out_row + gq[u]);
                }
            } else if constexpr (AUXE) {
#pragma unroll
                for (int u = 0; u < NU; ++u)
                    if (gq[u] >= 0) aux[u] = *(const f32x4*)(p.ep_aux + o_pair + gq[u]);
            }
            // Q -> staging (C/D layout of 16x16x4: column = lane & 15, row = (lane >> 4) * 4 + reg); the previous reads of the tile
            // are complete (LDS operations of one wave finish in order; the fences only pin the compiler)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    S[(2 + 16 * m + 4 * g + r) * SL + i] = acc[2 * hp][m][r];
                    S[(SP + 2 + 16 * m + 4 * g + r) * SL + i] = acc[2 * hp + 1][m][r];
                }
            wave_lds_sync();
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (gq[u] < 0) continue;
                f32x4 v;
                const int4 go = *(const int4*)(Tg + (u * 64 + lane) * 4);
                const f32x4 gb = *(const f32x4*)(Tb + (u * 64 + lane) * 4);
                const int goff[4] = {go.x, go.y, go.z, go.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* q_ = S + goff[e];
                    v[e] = ((gb[e] + q_[2 * GSTEP]) + q_[GSTEP]) + q_[0];             // kx0, kx0 + 2, kx0 + 4: a fixed order
                }
                if (p.epilogue == CGS_EPI_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fast_tanh(v[e]);
                } else if (p.epilogue == CGS_EPI_LRELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.2f * v[e]);
                } else if (AUXE && p.epilogue >= CGS_EPI_RELU_BWD_AFFINE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float y = aux[AUXE ? u : 0][e];
                        if (p.epilogue == CGS_EPI_TANH_BWD) v[e] *= (1.f - y * y);
                        else if (p.epilogue == CGS_EPI_LRELU_BWD) v[e] = y > 0.f ? v[e] : 0.2f * v[e];
                        else v[e] = y > 0.f ? v[e] * p.ep_a[(gq[u] + e) % N] : 0.f;
                    }
                }
                *(f32x4*)(p.out + o_pair + gq[u]) = v;
            }
            wave_lds_sync();
        }
    }
}

// geometry-only eligibility (the packed layout differs from the quad form's, and a cached packed workspace is keyed by the
// family and the geometry): kw * N columns fit one MFMA tile, whole float4 output rows, weights + staging fit the LDS
static int rows_mt(const CgsLayer& L) {
    if (!(L.Cb == 1 || L.Cb == 3) || L.kw * L.Cb > 16 || L.kw > 6 || (L.Cs % 16) != 0 || ((2 * L.Ws * L.Cb) % 4) != 0) return 0;
    if ((size_t)L.kh * L.Cs * 16 * sizeof(float) > 64 * 1024) return 0;
    if (L.Ws > 32) return 0;                   // (four pixel tiles x four output rows of accumulators do not fit 128 VGPRs)
    return L.Ws <= 16 ? 1 : 2;
}


// the neighbourhood of a quad along one axis: input offsets d = (parity + pad - tap) / 2 over the pairs of matching parity -> lowest d, count
static void quad_range(int k, int pad, int& lo, int& n) {
    int hi = -(1 << 20);
    lo = 1 << 20;
    for (int par = 0; par < 2; ++par)
        for (int kk = 0; kk < k; ++kk)
            if (((par + pad - kk) & 1) == 0) {
                const int d = (par + pad - kk) / 2;
                if (d < lo) lo = d;
                if (d > hi) hi = d;
            }
    n = hi - lo + 1;
}

// ... of a layer, into p; pt / pl = TF 'SAME' padding before the first pixel.  -> bytes of the quad forms' packed weight image [ny*nx*Cs][16]
static size_t quad_geom(const CgsLayer& L, QuadParams& p, int& pt, int& pl) {
    pt = cgs_same_pad_before(L.Hb, L.kh, 2); pl = cgs_same_pad_before(L.Wb, L.kw, 2);
    quad_range(L.kh, pt, p.dmin_y, p.ny);
    quad_range(L.kw, pl, p.dmin_x, p.nx);
    return (size_t)p.ny * p.nx * L.Cs * 16 * sizeof(float);
}

size_t cgs_convt_quad_ws_floats_bound(int kh, int kw, int Cs) {
    return (size_t)((kh + 1) / 2 + 1) * ((kw + 1) / 2 + 1) * Cs * 16;
}

// the quad forms keep the whole packed weight image in LDS: large kernels x many channels do not fit
static constexpr size_t QUAD_WEIGHT_BYTES_MAX = 150 * 1024;
bool cgs_convt_quad_fits(const CgsLayer& L) {
    QuadParams p;
    int pt, pl;
    return quad_geom(L, p, pt, pl) <= QUAD_WEIGHT_BYTES_MAX;
}

// Rows form.  Persistent blocks of 8 independent waves, two per CU (512 blocks), each a contiguous run of tasks.  Not cgs_persistent_run:
// a run is a whole number of rounds of the block's 8 waves, however short.
static int rows_launch(const CgsLayer& L, const QuadParams& q, int mt, int pt, int pl, const float* w, size_t ws_bytes, int prepacked, hipStream_t s) {
    RowsParams r;
    r.in = q.in; r.wp = q.wq; r.bias = q.bias; r.out = q.out; r.ep_a = q.ep_a; r.ep_aux = q.ep_aux;
    r.B = q.B; r.Hs = L.Hs; r.Ws = L.Ws; r.Cs = L.Cs; r.kh = L.kh; r.kw = L.kw; r.pt = pt; r.pl = pl;
    r.dmin_y = q.dmin_y; r.ny = q.ny; r.epilogue = q.epilogue;
    const size_t wfl = (size_t)L.kh * L.Cs * 16;
    if (!r.wp || ws_bytes < wfl * sizeof(float)) return cgs_set_error(CGS_EWORKSPACE, "convt_rows: workspace %zu < %zu bytes", ws_bytes, wfl * sizeof(float));
    if (!prepacked) {
        hipLaunchKernelGGL(pack_rows_weights_kernel, dim3((unsigned)((wfl + 255) / 256)), dim3(256), 0, s, w, (float*)q.wq, L.kh, L.kw, L.Cb, L.Cs);      // (wq is the caller's workspace)
        CGS_CHECK_LAUNCH("pack_rows_weights");
    }
    const bool auxe = r.epilogue >= CGS_EPI_RELU_BWD_AFFINE;
    const bool s5 = L.Cb == 3 && L.kh == 5 && L.Cs == 64 && pt == 1 && r.dmin_y == -1 && r.ny == 3;
    // output row pairs per task: the forward 5x5 64 -> 3 layers run the tall form (with an aux epilogue its 64 accumulators + the
    // aux values do not fit 128 VGPRs: 35 spilled registers)
    const bool tall = s5 && L.Hs >= 8 && !auxe;
    const long tasks = (long)r.B * ((L.Hs + (tall ? 3 : 1)) / (tall ? 4 : 2));
    if (tasks == 0) return CGS_OK;
    long blocks = (tasks + RowsLds::NWV - 1) / RowsLds::NWV;
    if (blocks > 512) blocks = 512;
    const long per = ((tasks + blocks - 1) / blocks + RowsLds::NWV - 1) / RowsLds::NWV * RowsLds::NWV;
    blocks = (tasks + per - 1) / per;
    const size_t smem = RowsLds::floats(wfl, L.Cb, mt) * sizeof(float);
#define ROWS_LAUNCH_(NN, MM, SS, PP, AA)                                                                           \
    {                                                                                                              \
        CGS_SMEM_ATTR(160 * 1024, "convt_rows", convt_rows_kernel<NN, MM, SS, PP, AA>);                            \
        CGS_LAUNCH_T(convt_rows_kernel, (NN, MM, SS, PP, AA), dim3((unsigned)blocks), dim3(512), smem, s, r, (int)tasks, (int)per); \
    }
#define ROWS_LAUNCH(NN, MM, SS) if (auxe) ROWS_LAUNCH_(NN, MM, SS, 2, true) else ROWS_LAUNCH_(NN, MM, SS, 2, false)
#define ROWS_LAUNCH_MT(MM)                                                                                         \
    if (L.Cb == 1) ROWS_LAUNCH(1, MM, false) else if (tall) ROWS_LAUNCH_(3, MM, true, 4, false)                    \
    else if (s5) ROWS_LAUNCH(3, MM, true) else ROWS_LAUNCH(3, MM, false)
    if (mt == 1) { ROWS_LAUNCH_MT(1) } else { ROWS_LAUNCH_MT(2) }
#undef ROWS_LAUNCH_MT
#undef ROWS_LAUNCH
#undef ROWS_LAUNCH_
    CGS_CHECK_LAUNCH("convt_rows");
    return CGS_OK;
}

// LDS-patch form: TW x 256 / TW quad tiles; two persistent blocks per CU (the 37 KB weight image is copied to LDS once per block)
static int quad_lds_launch(const CgsLayer& L, const QuadParams& p, int TW, size_t smem, hipStream_t s) {
    const bool wide = TW == 32, nyx3 = p.ny == 3 && p.nx == 3;
    const long tiles = (long)p.B * cgs_ceil_div(L.Hs, QuadLds::th(TW)) * cgs_ceil_div(L.Ws, TW);
    long per, blocks;
    cgs_persistent_run(tiles, 512, &per, &blocks);
#define QUAD_LDS_LAUNCH(NN, TT, YX)                                                                                \
    {                                                                                                              \
        CGS_SMEM_ATTR(160 * 1024, "convt_quad_lds", convt_quad_lds_kernel<NN, TT, YX>);                            \
        CGS_LAUNCH_T(convt_quad_lds_kernel, (NN, TT, YX), dim3((unsigned)blocks), dim3(256), smem, s, p, (int)tiles, (int)per); \
    }
#define QUAD_LDS_CASE(NN)                                                                                          \
    case NN:                                                                                                       \
        if (wide && nyx3) QUAD_LDS_LAUNCH(NN, 32, 3) else if (wide) QUAD_LDS_LAUNCH(NN, 32, 0)                     \
        else if (nyx3) QUAD_LDS_LAUNCH(NN, 16, 3) else QUAD_LDS_LAUNCH(NN, 16, 0)                                  \
        break;
    switch (L.Cb) {
        QUAD_LDS_CASE(1) QUAD_LDS_CASE(2) QUAD_LDS_CASE(3) QUAD_LDS_CASE(4)
        default: return cgs_set_error(CGS_EINVAL, "convt_quad: N=%d", L.Cb);
    }
#undef QUAD_LDS_CASE
#undef QUAD_LDS_LAUNCH
    CGS_CHECK_LAUNCH("convt_quad_lds");
    return CGS_OK;
}

// global-load form: any neighbourhood, any row alignment; a block = 4 waves x 4 tiles of 16 quads
static int quad_mfma_launch(const QuadParams& p, size_t need, hipStream_t s) {
    CGS_SMEM_ATTR(QUAD_WEIGHT_BYTES_MAX, "convt_quad_mfma", convt_quad_mfma_kernel<4>);
    const long blocks = ((long)p.B * p.Hs * p.Ws + 64 * 4 - 1) / (64 * 4);
    CGS_LAUNCH_T(convt_quad_mfma_kernel, (4), dim3((unsigned)blocks), dim3(256), need, s, p);
    CGS_CHECK_LAUNCH("convt_quad_mfma");
    return CGS_OK;
}

// The chooser: taps (convt_taps.hip; it reads the raw weights and the input as float4 -- a view at an unaligned offset keeps the packed
// forms) -> rows -> the quad forms on their packed image: LDS patch (8 x 32 quad tiles, or 16 x 16 clipped at the edges for grids that are not
// whole 8 x 32 tiles; a neighbourhood <= 3 x 3, 16-byte aligned output rows, staging rows inside a patch buffer) -> global loads
int cgs_convt_quad_launch(const CgsLayer& L, int B, const float* in, const float* w, const float* bias, float* out,
                          int epilogue, const float* ep_a, const float* ep_aux, float* ws, size_t ws_bytes, int prepacked,
                          hipStream_t s) {
    if ((long)B * L.Hs * L.Ws * L.Cs * 4 > 0x7fffffffL) return cgs_set_error(CGS_EINVAL, "convt_quad: input exceeds 2 GiB (split the batch)");
    if (cgs_convt_taps_ok(L) && !(((uintptr_t)w | (uintptr_t)in) & 15)) return cgs_convt_taps_launch(L, B, in, w, bias, out, epilogue, ep_a, ep_aux, s);
    QuadParams p;
    p.in = in; p.wq = ws; p.bias = bias; p.out = out; p.ep_a = ep_a; p.ep_aux = ep_aux;
    p.B = B; p.Hs = L.Hs; p.Ws = L.Ws; p.Cs = L.Cs; p.N = L.Cb; p.epilogue = epilogue;
    int pt, pl;
    const size_t need = quad_geom(L, p, pt, pl);
    if (const int mt = rows_mt(L)) return rows_launch(L, p, mt, pt, pl, w, ws_bytes, prepacked, s);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "convt_quad: workspace %zu < %zu bytes", ws_bytes, need);
    if (need > QUAD_WEIGHT_BYTES_MAX) return cgs_set_error(CGS_EINVAL, "convt_quad: packed weights (%zu B) exceed LDS", need);
    if (!prepacked) {
        hipLaunchKernelGGL(pack_quad_weights_kernel, dim3((unsigned)((need / sizeof(float) + 255) / 256)), dim3(256), 0, s, w, ws, L.kh, L.kw,
                           L.Cb, L.Cs, pt, pl, p.dmin_y, p.ny, p.dmin_x, p.nx);
        CGS_CHECK_LAUNCH("pack_quad_weights");
    }
    if ((long)B * L.Hs * L.Ws == 0) return CGS_OK;
    const int TW = (L.Ws % 32) == 0 && (L.Hs % 8) == 0 ? 32 : 16;
    const size_t patch = (size_t)QuadLds::patch_f4(QuadLds::ph(TW, p.ny), QuadLds::pw(TW, p.nx)) * 4, smem = need + 2 * patch * sizeof(float);
    if (p.ny <= 3 && p.nx <= 3 && ((2 * L.Ws * L.Cb) % 4) == 0 && smem <= 160 * 1024 && (size_t)4 * 256 * L.Cb <= 2 * patch)
        return quad_lds_launch(L, p, TW, smem, s);
    return quad_mfma_launch(p, need, s);
}
