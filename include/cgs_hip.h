/*
 * cgs_hip.h -- C ABI of libcgs_hip.so: the MI355X (gfx950) kernels under the
 * collaborative-sampling refinement hot path.
 *
 * The reference (vita-epfl/collaborative-gan-sampling) has no FFI layer: its hot
 * path (sampling/collaborator.py:26-88) is made of stock TensorFlow ops reached
 * through nsgan/ops.py.  Each entry point below replaces one of those TF call
 * sites (cited per function; paths are under the reference root).  The host
 * side that mirrors the reference's Python operator / sampler classes sits on
 * top of this ABI (collaborative-gan-sampling_amd/ops.py, sampling/ *.py) and
 * binds it with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions:
 *   - plain C: raw DEVICE pointers + ints; no torch / hip types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = the null stream);
 *   - activations NHWC fp32; conv weights HWIO [kh,kw,Cin,Cout]
 *     (nsgan/ops.py:39); deconv weights [kh,kw,Cout,Cin] (nsgan/ops.py:51);
 *     linear weights [in,out] (nsgan/ops.py:76);
 *   - TF 'SAME' padding everywhere (extra pixel bottom/right);
 *   - caller allocates every output and workspace; nothing is allocated or
 *     freed inside; calls are asynchronous on `stream` and graph-capturable;
 *   - return 0 on success, a negative CGS_E* code otherwise; never throws;
 *     cgs_last_error() gives a thread-local message.
 */
#ifndef CGS_HIP_H
#define CGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGS_OK 0
#define CGS_EINVAL (-1)   /* bad argument / unsupported shape */
#define CGS_EWORKSPACE (-2) /* workspace too small */
#define CGS_ELAUNCH (-3)  /* HIP launch error */

/* epilogues fused into the conv / deconv / linear kernels (applied after +bias) */
#define CGS_EPI_NONE 0
#define CGS_EPI_LRELU 1        /* max(v, leak*v), leak = 0.2        nsgan/ops.py:69-70            */
#define CGS_EPI_AFFINE_RELU 2  /* relu(a[c]*v + b[c]) = inference-mode bn + relu, nsgan/GAN.py:96-98 */
#define CGS_EPI_TANH 3         /* tanh(v)                            nsgan/GAN.py:100              */
/* backward-data epilogues: the produced gradient is w.r.t. the OUTPUT of the layer below; these fold that
 * layer's activation gradient in (aux = the layer-below's saved output, same shape as the result; no bias) */
#define CGS_EPI_RELU_BWD_AFFINE 4  /* aux > 0 ? v*a[c] : 0     through relu(a*x+b)   nsgan/GAN.py:96-98 */
#define CGS_EPI_LRELU_BWD 5        /* v * (aux > 0 ? 1 : 0.2)  through lrelu         nsgan/ops.py:69-70 */
#define CGS_EPI_TANH_BWD 6         /* v * (1 - aux*aux)        through tanh          nsgan/GAN.py:100   */

/* which transposition of the weights a conv-family call contracts over */
#define CGS_CONV_FWD 0          /* tf.nn.conv2d                        nsgan/ops.py:41 */
#define CGS_CONV_BWD_DATA 1     /* its input gradient (tf.gradients)   sampling/collaborator.py:31 */
#define CGS_DECONV_FWD 2        /* tf.nn.conv2d_transpose              nsgan/ops.py:55 */
#define CGS_DECONV_BWD_DATA 3   /* its input gradient                  sampling/collaborator.py:31 */

/* the loss a refinement step descends, per logit and unreduced (the func_loss of Refiner.set_env, sampling/collaborator.py:30-31),
 * and the D-side training losses (cgs_gan_logits_grad) */
#define CGS_LOSS_BCE 0     /* softplus(-l)   dl = sigmoid(l) - 1        nsgan/GAN.py:176-177                     */
#define CGS_LOSS_LSQ 1     /* (l - 1)^2      dl = 2 (l - 1)             least squares, the PatchGAN's usual loss */
#define CGS_LOSS_LINEAR 2  /* -l             dl = -1                    generator side of hinge / Wasserstein    */
#define CGS_LOSS_HINGE 3   /* D side only: relu(1 - l) on real, relu(1 + l) on fake                            */

/* The per-sample state of the ladam rule (sampling/policy.py:48-51,56), advanced ONCE per sample by the seed launch of a step:
 *   loss[b]     = s_real[0] - mean_p sigmoid(logits[b,p])        (sampling/refiner_cpu.py:28,55; the score of cgs_sigmoid_rowmean)
 *   loss_avg[b] = first ? loss[b] : 0.5 * loss_avg[b] + 0.5 * loss[b]
 *   gain[b]     = clamp(loss_avg[b] + 0.5, 0, 1e4)^2
 * Every pointer is device memory; s_real is one float, read at launch time (a captured launch replays with the value of the day). */
typedef struct cgs_ladam_seed {
    const float* s_real;
    float* loss_avg;   /* [B] read (unless first) and written */
    float* gain;       /* [B] written */
    int first;
} cgs_ladam_seed;

int cgs_version(void);
/* sha256 (64 hex digits) of the kernel sources this library was built from (every .hip and .h file of csrc/, then include/cgs_hip.h), embedded at
 * build time (csrc/Makefile, csrc/stamp.hip).  The host binding refuses a library whose stamp differs from the sources it ships with
 * (cgs_amd/lib.py::load); bench.py reports this embedded value, so a measured number names the code that produced it. */
const char* cgs_source_sha(void);
const char* cgs_last_error(void);
/* Name of the compute kernel the calling thread's most recent conv-family call launched (for profiling).
 * The norm entry points (cgs_bn_train_lrelu_fwd / _fwd_from_partials / _bwd_data, cgs_instnorm_lrelu_fwd / _bwd_data,
 * cgs_groupnorm_lrelu_fwd_from_partials, cgs_norm_lrelu_bwd_from_partials) leave the name of the FORM they launched, with
 * "_fwd" or "_bwd" appended:
 *   norm_small     one launch, statistics + apply from registers          (<= 128 rows per group)
 *   norm_passes    partial sums -> finalize -> apply                      (from x, more rows)
 *   norm_fa        one launch, finalize + apply from the partial rows     (<= 16 partial rows per group and a tensor of <= 2 MB)
 *   norm_finalize  one-stage finalize -> apply                            (from partials otherwise)
 *   norm_sliced    slice sums -> finalize of the slices -> apply          (>= 1024 partial rows, one group, one segment)
 * so a test can pin the path a shape takes (tests/test_gpu_norm_paths.py). */
const char* cgs_last_kernel(void);
/* Floating-point operations that call really issued to the matrix cores: 2 x (algorithmic multiply-accumulates minus those
 * of zero-padding taps the kernel skipped).  0 = the kernel skips nothing (executed = algorithmic).  For rooflines. */
double cgs_last_executed_flops(void);
/* Tail split of the calling thread's most recent conv-family call (0 / 0 = none): how many of the launch's last output tiles were
 * contracted by several workgroups over disjoint ranges of the reduction, and by how many each -- a scheduling detail of the
 * implicit GEMM (a launch whose tile count leaves a partial last round of workgroups; csrc/igemm.hip), reported for profiling and
 * tests.  The partial tiles are added in a fixed order: results stay bit-identical from run to run. */
int cgs_last_tail_tiles(void);
int cgs_last_tail_split(void);
/* Launch plan of the calling thread's most recent implicit-GEMM launch (all 0: the call ran another family), for tests:
 * out[0] = per-XCD block decode on (1) / off (0), out[1] = classes per group reversed in odd rounds (0 = no flip),
 * out[2] = uniform-tile K loop allowed, out[3] = grid x (block ids per class and K slice), out[4] = split-K factor (1 = none).
 * Scheduling details of csrc/igemm.hip: results do not depend on them. */
void cgs_last_igemm_plan(int out[5]);
/* The same plan BEFORE the launch, and the rest of it (host only: needs no device, launches nothing; for tests and profiling).
 * Arguments as cgs_conv_family's; form = what the entry point adds to the plain call (CGS_FORM_*: the *_fwd_stats, *_bwd_data_nstats,
 * *_fwd_signs and *_bwd_data_update entry points); ws_bytes = the call's whole workspace.  Returns 0 where the call would not run the
 * exact-fp32 implicit GEMM (CGS_FAMILY_IGEMM) in ONE launch or where that launch would refuse the form, otherwise 1 and *info: the
 * instantiation as cgs_last_kernel will name it (a constant string), the reduce kernel that follows it, what cgs_last_tail_tiles / _split,
 * cgs_last_igemm_plan and cgs_last_executed_flops will say, the priority thresholds, the GEMM row order (as cgs_conv_update_form's) and,
 * per parity class c, perm_len[c] base pixels in the order the m-tiles visit them, written to perm[256 * c ...] (perm: 1024 bytes or NULL;
 * perm_len 0 = natural order).  Without a device the round rules apply as on the MI355X's 256 compute units (cgs_conv_ws_bytes_for too). */
#define CGS_FORM_PLAIN 0
#define CGS_FORM_STATS 1
#define CGS_FORM_NSTATS 2
#define CGS_FORM_SIGNS 3
#define CGS_FORM_UPDATE 4
#define CGS_REDUCE_NONE 0
#define CGS_REDUCE_TAIL 1            /* tail_reduce_kernel<false>   */
#define CGS_REDUCE_TAIL_UPDATE 2     /* tail_reduce_kernel<true>    */
#define CGS_REDUCE_SPLITK 3          /* splitk_reduce_kernel<false> */
#define CGS_REDUCE_SPLITK_UPDATE 4   /* splitk_reduce_kernel<true>  */
#define CGS_REDUCE_SPLITK_STATS 5    /* splitk_reduce_stats_kernel  */
typedef struct cgs_igemm_plan_info {
    const char* kernel;
    int reduce;
    int tail_tiles, tail_split;
    int plan[5];
    int prio_t[3];
    int row_order;
    int perm_len[4];
    double executed_flops;
} cgs_igemm_plan_info;
int cgs_conv_igemm_plan(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                        int epilogue, int form, size_t ws_bytes, cgs_igemm_plan_info* info, unsigned char* perm);

/* Contraction arithmetic of the implicit-GEMM layers, per calling THREAD (default CGS_CONTRACTION_F32; no process-wide state).
 * F32: v_mfma_f32_32x32x2_f32 -- exact fp32 products, an fp32 fma chain over K: what tf.nn.conv2d / conv2d_transpose / matmul
 *      (nsgan/ops.py:41,55,81) compute at the reference's precision.  The headline numbers are measured in this mode.
 * BX6: opt-in.  Calls whose output channels are a multiple of 64, that reduce over whole 32-channel chunks (Cred % 32 == 0, at most
 *      16 taps per axis) and whose grid fills the GPU (>= 256 blocks, K >= 512) -- cgs_conv_family says which -- run on the bf16 matrix
 *      cores instead: every fp32 operand is split exactly into three bf16 pieces and six of the nine piece
 *      products are accumulated in fp32 (the dropped ones are below 3 * 2^-24 of the product): the result differs from the F32
 *      mode's by rounding errors of the size of an fp32 chain's own (igemm_bx6.hip; error analysis: DESIGN.md), in 6/16 of
 *      the matrix time.  Everything else (families, epilogues, fused statistics, layouts) is unchanged; the packed-weight
 *      layout differs, which cgs_conv_family reports as CGS_FAMILY_IGEMM_BX6 (key cached workspaces by it).
 * BX6_ALL: BX6 for every call whose geometry allows it, whatever its size (test coverage of the kernel on small shapes).
 * Set it before the thread's calls -- including cgs_conv_family / cgs_conv_signs_ok / cgs_conv_stat_* queries, which answer
 * for the mode in force.  Returns CGS_OK or CGS_EINVAL. */
#define CGS_CONTRACTION_F32 0
#define CGS_CONTRACTION_BX6 1
#define CGS_CONTRACTION_BX6_ALL 2
int cgs_set_contraction(int mode);
int cgs_get_contraction(void);

/* Bytes of workspace a conv-family call needs for its packed copy of the weights
 * (op = one of CGS_CONV_* above; Cin/Cout are those of the LAYER, i.e. of the
 * forward op, for the backward variants too). */
size_t cgs_conv_ws_bytes(int op, int kh, int kw, int sh, int sw, int Cin, int Cout);
/* Same, plus room for the split-K partial slabs the library uses when the launch would otherwise
 * leave most CUs idle (small batch x small spatial size, e.g. the MNIST fc layers at batch 64).
 * B, H, W as passed to the entry point.  Optional: with only cgs_conv_ws_bytes() bytes the call runs un-split.
 * Layout: [packed weights | slabs]; ws_prepacked refers to the first part only. */
size_t cgs_conv_ws_bytes_for(int op, int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw);

/* Kernel family a conv-family call with these arguments will run, given 16-byte aligned pointers and a workspace of
 * ws_bytes (B, H, W, Cin, Cout as passed to the entry point; Ho, Wo = the deconv ops' output size, ignored for the conv
 * ops).  Each family keeps its OWN packed-weight layout in the workspace, so a caller
 * that sets ws_prepacked must key its cached workspaces by (weights, op, geometry, family): the epilogue takes part in
 * the choice.  CGS_FAMILY_SMALLN_T packs nothing.  Negative = error. */
#define CGS_FAMILY_IGEMM 0      /* implicit GEMM on the fp32 matrix cores (igemm.hip)                     */
#define CGS_FAMILY_QUAD 1       /* <= 4 output channels, transposed stride 2 (convt_quad.hip)             */
#define CGS_FAMILY_SMALLN_T 2   /* same, VALU form (convt_smalln.hip)                                     */
#define CGS_FAMILY_SMALLN_F 3   /* stride-1 forward conv with <= 4 output channels (conv_smalln_f.hip)    */
#define CGS_FAMILY_PATCH 4      /* 3-channel strided / stem convs from an LDS patch (conv_patch.hip)      */
#define CGS_FAMILY_TAPS 5       /* 4x4 stride-2 conv from ONE channel, K = 16 taps (convt_taps.hip); reads the weights unpacked */
#define CGS_FAMILY_DOT 6        /* forward conv to <= 4 channels over a deep reduction (conv_dot.hip); weights unpacked         */
#define CGS_FAMILY_IGEMM_BX6 7  /* implicit GEMM through split-bf16 MFMA (igemm_bx6.hip): only after cgs_set_contraction       */
int cgs_conv_family(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                    int epilogue, size_t ws_bytes);

/* conv2d: y[B,Ho,Wo,Cout] = conv(x[B,H,W,Cin], w[kh,kw,Cin,Cout], stride, 'SAME') + bias, then epilogue.
 * Replaces tf.nn.conv2d + tf.nn.bias_add at nsgan/ops.py:41-44 (Ho = ceil(H/sh)).
 * ws/ws_bytes: see cgs_conv_ws_bytes; ws_prepacked != 0 means ws already holds the packed
 * weights from an earlier call with the same w (frozen weights: pack once). bias may be NULL. */
int cgs_conv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y,
                        int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                        int epilogue, const float* ep_a, const float* ep_b,
                        void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* The same conv (no fused epilogue) that also leaves per-block column sums of its OUTPUT -- sum and sum of squares per
 * channel -- in stat_part[G][2][Cout], so the batch-statistics batch norm that follows it in D (nsgan/GAN.py:65 -> nsgan/ops.py:19-26)
 * does not re-read the tensor for its statistics pass.  G = cgs_conv_stat_partials(...) (same B, H, W, ..., ws_bytes as the call);
 * 0 = the fused form is not available for this call (another kernel family, Cout % 4 != 0, a batch the library would split):
 * use cgs_conv2d_nhwc_fwd + cgs_bn_train_lrelu_fwd.  Deterministic (fixed reduction trees). */
int cgs_conv_stat_partials(int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, size_t ws_bytes);
int cgs_conv2d_nhwc_fwd_stats(const float* x, const float* w, const float* bias, float* y,
                              int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                              void* ws, size_t ws_bytes, int ws_prepacked,
                              float* stat_part, size_t stat_part_bytes, void* stream);

/* The same statistics per GROUP of group_images consecutive images, and for the transposed convolution too: what an instance norm
 * behind a conv / deconv needs (a group = one sample; CycleGAN generator and PatchGAN discriminator of BASELINE config 5 -- the
 * reference ships no code for them), and D's batch norm (nsgan/GAN.py:65,67 -> nsgan/ops.py:19-26) when several logical batches
 * share one launch (a group = one logical batch: every batch keeps the statistics the reference computes for it alone).
 * cgs_conv_stat_layout says where a group's partial rows lie in the [rows][2][Cout] buffer that cgs_conv2d_nhwc_fwd_stats
 * (op = CGS_CONV_FWD; Ho, Wo ignored) / cgs_deconv2d_nhwc_fwd_stats (op = CGS_DECONV_FWD) fill (and, with the *_BWD_DATA ops, the
 * [rows][2][Cin] buffer of the *_bwd_data_nstats entry points below): group g owns, for every segment
 * s < *nseg, the *rows_per_seg rows starting at row s * *seg_stride + g * *rows_per_seg.  Returns the buffer's row count; 0 = not
 * available (another kernel family, Cout % 4 != 0, a split batch, parity classes of unequal size, a group that does not end on
 * a 64-row boundary of the launch's row order).  cgs_groupnorm_lrelu_fwd_from_partials (below) consumes it. */
int cgs_conv_stat_layout(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                         int group_images, size_t ws_bytes, int* rows_per_seg, int* nseg, int* seg_stride);
int cgs_deconv2d_nhwc_fwd_stats(const float* x, const float* w, const float* bias, float* y,
                                int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                                void* ws, size_t ws_bytes, int ws_prepacked,
                                float* stat_part, size_t stat_part_bytes, void* stream);

/* The BACKWARD half of the same fusion (round 6).  tf.gradients through D's batch norm (sampling/collaborator.py:31 over
 * nsgan/ops.py:19-26, nsgan/GAN.py:65,67) needs two column sums over the gradient dy that arrives at the norm's output:
 * sum d and sum d * xhat, d = dy * lrelu'(gamma * xhat + beta), xhat = (x - mean) * invstd.  dy is the RESULT of the backward-data
 * pass of the convolution above the norm, so that launch can leave them: cgs_conv2d_nhwc_bwd_data_nstats /
 * cgs_deconv2d_nhwc_bwd_data_nstats are cgs_conv2d_nhwc_bwd_data / cgs_deconv2d_nhwc_bwd_data (no epilogue) that also read
 * x_norm -- the norm's input, same shape as dx -- and write the sums as partial rows [rows][2][Cin] (one per 64 GEMM rows):
 * cgs_conv_stat_layout with op = CGS_CONV_BWD_DATA / CGS_DECONV_BWD_DATA (same argument meaning as the entry point's) says where
 * the rows of every group of group_images consecutive images lie (group_images = B: batch norm over the whole batch; 1: instance
 * norm; b: fused logical batches), 0 = not available (then: the plain backward-data + cgs_bn_train_lrelu_bwd_data /
 * cgs_instnorm_lrelu_bwd_data).  mean / invstd are [B / group_images][Cin], gamma / beta [Cin].
 * cgs_norm_lrelu_bwd_from_partials finishes the norm's backward-data from them: finalize + ONE pass over dy and x (the sums pass of
 * cgs_bn_train_lrelu_bwd_data -- 2 of its 5 tensor passes -- is gone); dy / x are [groups][M_group][C], dx may be dy.
 * ws: cgs_bn_ws_bytes(M, C) / cgs_instnorm_ws_bytes(groups, M_group, C) cover it.  Deterministic (fixed reduction trees). */
int cgs_conv2d_nhwc_bwd_data_nstats(const float* dy, const float* w, float* dx,
                                    int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                                    const float* x_norm, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                    float leak, int group_images, void* ws, size_t ws_bytes, int ws_prepacked,
                                    float* stat_part, size_t stat_part_bytes, void* stream);
int cgs_deconv2d_nhwc_bwd_data_nstats(const float* dy, const float* w, float* dx,
                                      int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                                      const float* x_norm, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                      float leak, int group_images, void* ws, size_t ws_bytes, int ws_prepacked,
                                      float* stat_part, size_t stat_part_bytes, void* stream);
int cgs_norm_lrelu_bwd_from_partials(const float* dy, const float* x, const float* part, int groups, int rows_per_seg, int nseg,
                                     int seg_stride, const float* gamma, const float* beta, const float* mean, const float* invstd,
                                     float leak, float* dx, int M_group, int C, void* ws, size_t ws_bytes, void* stream);

/* conv2d backward-data: dx[B,H,W,Cin] = d/dx of the conv above applied to dy[B,Ho,Wo,Cout].
 * Replaces the Conv2DBackpropInput node tf.gradients emits (sampling/collaborator.py:31).
 * epilogue: CGS_EPI_NONE or one of the *_BWD modes (ep_aux [B,H,W,Cin], ep_a [Cin]). */
int cgs_conv2d_nhwc_bwd_data(const float* dy, const float* w, float* dx,
                             int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                             int epilogue, const float* ep_a, const float* ep_aux,
                             void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* deconv2d: y[B,Ho,Wo,Cout] = conv2d_transpose(x[B,H,W,Cin], w[kh,kw,Cout,Cin], output_shape, stride) + bias,
 * then epilogue.  Replaces tf.nn.conv2d_transpose + bias_add at nsgan/ops.py:55,61-62
 * (requires H == ceil(Ho/sh), W == ceil(Wo/sw)). */
int cgs_deconv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y,
                          int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                          int epilogue, const float* ep_a, const float* ep_b,
                          void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* deconv2d backward-data: dx[B,H,W,Cin] from dy[B,Ho,Wo,Cout] (a strided 'SAME' conv with the deconv weights). */
int cgs_deconv2d_nhwc_bwd_data(const float* dy, const float* w, float* dx,
                               int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                               int epilogue, const float* ep_a, const float* ep_aux,
                               void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* ---- the refinement loop's momentum step inside the backward-data launch that produces its gradient ------------------------------
 * sampling/collaborator.py:31,66 descends theta along g = d loss / d theta, and g is the RESULT of the backward-data pass of the
 * generator tail's first layer; it serves nothing but cgs_refine_update (below), which reads g, theta and m and writes theta and m in a
 * launch of its own.  cgs_conv2d_nhwc_bwd_data_update / cgs_deconv2d_nhwc_bwd_data_update are cgs_conv2d_nhwc_bwd_data /
 * cgs_deconv2d_nhwc_bwd_data (no epilogue) that do not store g: at the element g[i] would have gone to they apply
 *     m[i] <- first ? rate * g[i] : alpha * m[i] + rate * g[i];   theta[i] <- theta[i] - m[i]
 * -- cgs_refine_update without the clip, the same separately rounded operations on the same fp32 value of g: theta and m come out
 * bit-identical to the two-launch form.  theta and m have the shape of dx, 16-byte aligned.
 * cgs_conv_update_form (op = CGS_CONV_BWD_DATA / CGS_DECONV_BWD_DATA; arguments as the entry point's) says BEFORE the call -- and before a
 * graph capture -- where the update would be applied: in the implicit GEMM's own epilogue, or in the reduce pass of a launch that is split
 * over K or whose tail tiles are; 0 = not offered (another kernel family or contraction mode, Cin % 4 != 0, a reduction that is not whole
 * 32-channel chunks, the 256 x 64 tile, a batch the library would split): the entry point then returns CGS_EINVAL and touches neither
 * theta nor m -- use the plain backward-data + cgs_refine_update.  *row_order (may be NULL): the launch's GEMM row order, 0 = (image,
 * pixel), 1 = (pixel, image), 2 = (pixel, image) in whole 128-image tiles. */
#define CGS_UPDATE_EPILOGUE 1   /* the igemm_up_kernel twin's epilogue                          */
#define CGS_UPDATE_SPLITK 2     /* the reduce pass of a launch split over K                     */
#define CGS_UPDATE_TAIL 3       /* the twin's epilogue, and the reduce pass of the tail tiles   */
int cgs_conv_update_form(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                         size_t ws_bytes, int* row_order);
int cgs_conv2d_nhwc_bwd_data_update(const float* dy, const float* w, float* theta, float* m,
                                    int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw,
                                    float rate, float alpha, int first,
                                    void* ws, size_t ws_bytes, int ws_prepacked, void* stream);
int cgs_deconv2d_nhwc_bwd_data_update(const float* dy, const float* w, float* theta, float* m,
                                      int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                                      float rate, float alpha, int first,
                                      void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* ---- sign masks -------------------------------------------------------------------------------------------------------
 * d relu / d lrelu need ONE BIT of the saved activation (is it > 0), not the fp32 tensor: where the consumer of that
 * gradient is an HBM-bound kernel -- the backward-data of the generator's last, 3-channel deconv (a strided conv of the
 * image gradient whose epilogue applies relu'(y) * a of nsgan/GAN.py:98-99's bn + relu; tf.gradients at
 * sampling/collaborator.py:31) -- the producing forward launch leaves a bitmask next to its output and the backward launch
 * reads that instead (8 MB instead of 268 MB for the 32x32x64 map at batch 1024).
 * Layout, for a tensor [P pixels][C channels], C % 32 == 0: one plane of P words per 32-channel group,
 * uint32 word[(c / 32) * P + p], bit 8 * (c % 4) + (c % 32) / 4 is set iff x[p][c] > 0 (the bit order of the producing
 * epilogue's lane layout; the consumer un-shuffles it).  Caller-allocated, P * C / 8 bytes, 4-byte aligned.
 * cgs_conv_signs_ok: 1 if the call with these arguments can LEAVE a mask (op a forward with CGS_EPI_LRELU / CGS_EPI_AFFINE_RELU)
 * or TAKE one (op a backward-data with CGS_EPI_LRELU_BWD / CGS_EPI_RELU_BWD_AFFINE); 0 = use the fp32 aux tensor. */
int cgs_conv_signs_ok(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                      int epilogue, size_t ws_bytes);
/* cgs_deconv2d_nhwc_fwd that also writes the sign mask of y (after the epilogue) to signs. */
int cgs_deconv2d_nhwc_fwd_signs(const float* x, const float* w, const float* bias, float* y,
                                int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                                int epilogue, const float* ep_a, const float* ep_b, unsigned* signs,
                                void* ws, size_t ws_bytes, int ws_prepacked, void* stream);
/* cgs_deconv2d_nhwc_bwd_data whose relu' / lrelu' epilogue reads the sign mask of the saved activation (shape of dx). */
int cgs_deconv2d_nhwc_bwd_data_signs(const float* dy, const float* w, float* dx,
                                     int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw,
                                     int epilogue, const float* ep_a, const unsigned* aux_signs,
                                     void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* linear: y[B,out] = x[B,in] @ w[in,out] + bias, then epilogue (NONE or LRELU).
 * Replaces tf.matmul + bias at nsgan/ops.py:81-83.  ws as for conv (op CGS_CONV_FWD, kh=kw=1). */
int cgs_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int in, int out,
                   int epilogue, void* ws, size_t ws_bytes, int ws_prepacked, void* stream);
/* The single-logit head of D (nsgan/GAN.py:68: linear(net, 1)) and the loss seed of the refinement loop in one launch:
 * logits[b] = x[b,:] . w + bias; dlogits[b] = sigmoid(logits[b]) - 1 (nsgan/GAN.py:176-177 through tf.gradients,
 * sampling/collaborator.py:31); logit_mean[b] = logits[b] (collaborator.py:34-37 with one logit per sample).
 * = cgs_linear_fwd(out = 1) followed by cgs_bce_ones_grad_rowmean(P = 1), bit for bit. */
int cgs_linear_out1_bce(const float* x, const float* w, const float* bias, float* logits, float* dlogits, float* logit_mean, int B, int in,
                        void* stream);
/* The same head with the loss seed of cgs_refine_loss_seed(kind, ladam) at P = 1: = cgs_linear_fwd(out = 1) followed by that seed, bit
 * for bit (kind CGS_LOSS_BCE without ladam launches the kernel of cgs_linear_out1_bce itself). */
int cgs_linear_out1_seed(const float* x, const float* w, const float* bias, float* logits, float* dlogits, float* logit_mean, int B, int in,
                         int kind, const cgs_ladam_seed* ladam, void* stream);
/* linear backward-data: dx[B,in] = dy[B,out] @ w^T   (ws: op CGS_CONV_BWD_DATA, kh=kw=1). */
int cgs_linear_bwd_data(const float* dy, const float* w, float* dx, int B, int in, int out,
                        void* ws, size_t ws_bytes, int ws_prepacked, void* stream);

/* Batch-statistics batch norm (tf.contrib.layers.batch_norm(is_training=True), nsgan/ops.py:19-26)
 * fused with the lrelu that follows it in D (nsgan/GAN.py:65,67).  x is [M,C] (M = B*H*W or B).
 *   fwd : mean[c], invstd[c] = 1/sqrt(biased_var+eps) are written (saved for backward);
 *         y = lrelu(gamma*(x-mean)*invstd + beta, leak)   (leak = 1 gives plain bn).
 *   ws  : cgs_bn_ws_bytes(M, C) bytes of scratch for the two-stage deterministic reduction. */
size_t cgs_bn_ws_bytes(int M, int C);
int cgs_bn_train_lrelu_fwd(const float* x, const float* gamma, const float* beta, float eps, float leak,
                           float* y, float* mean, float* invstd, int M, int C,
                           void* ws, size_t ws_bytes, void* stream);
/*   fwd from the partial sums a cgs_conv2d_nhwc_fwd_stats call left (part[G][2][C]): statistics pass skipped. */
int cgs_bn_train_lrelu_fwd_from_partials(const float* x, const float* part, int G, const float* gamma, const float* beta,
                                         float eps, float leak, float* y, float* mean, float* invstd, int M, int C,
                                         void* ws, size_t ws_bytes, void* stream);
/*   bwd : dx = gamma*invstd*(dy' - mean(dy') - xhat*mean(dy'*xhat)), dy' = dy*lrelu'(bn(x)),
 *         the input gradient tf.gradients builds for the two ops (sampling/collaborator.py:31). */
int cgs_bn_train_lrelu_bwd_data(const float* dy, const float* x, const float* gamma, const float* beta,
                                const float* mean, const float* invstd, float leak, float* dx, int M, int C,
                                void* ws, size_t ws_bytes, void* stream);

/* Synchronised batch statistics: ONE logical batch whose rows are split over several GPUs (the reference computes D's
 * batch norm over the whole batch, nsgan/GAN.py:175 -> nsgan/ops.py:19-26).  Each pass is cut at the per-channel sums:
 *   cgs_bn_sync_fwd_sums : sums[0..C) = sum_m x, sums[C..2C) = sum_m x^2 over the LOCAL rows, in double
 *   -- caller: all-reduce(SUM) of the 2*C doubles over the ranks (RCCL) --
 *   cgs_bn_sync_fwd_apply: statistics from the global sums and M_total = total rows; y, mean, invstd as cgs_bn_train_lrelu_fwd
 *   cgs_bn_sync_bwd_sums : sums = {sum dy', sum dy'*xhat} over the local rows (mean / invstd = the saved global statistics)
 *   -- all-reduce --
 *   cgs_bn_sync_bwd_apply: dx as cgs_bn_train_lrelu_bwd_data with the global means.
 * With one rank (M_total = M) the results equal the unsplit entry points'.  ws: cgs_bn_ws_bytes(M, C). */
int cgs_bn_sync_fwd_sums(const float* x, double* sums, int M, int C, void* ws, size_t ws_bytes, void* stream);
int cgs_bn_sync_fwd_apply(const float* x, const float* gamma, const float* beta, float eps, float leak, const double* sums,
                          long long M_total, float* y, float* mean, float* invstd, int M, int C,
                          void* ws, size_t ws_bytes, void* stream);
int cgs_bn_sync_bwd_sums(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                         const float* invstd, float leak, double* sums, int M, int C, void* ws, size_t ws_bytes, void* stream);
int cgs_bn_sync_bwd_apply(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                          const float* invstd, float leak, const double* sums, long long M_total, float* dx, int M, int C,
                          void* ws, size_t ws_bytes, void* stream);

/* Instance norm (+ lrelu; leak = 0 gives relu, 1 plain): statistics over the HW pixels of every (sample, channel);
 * x is [B,HW,C].  CycleGAN-style generators / PatchGAN discriminators (BASELINE config 5; the reference ships no
 * code for them).  mean / invstd are [B,C].  ws: cgs_instnorm_ws_bytes(B, HW, C). */
size_t cgs_instnorm_ws_bytes(int B, int HW, int C);
int cgs_instnorm_lrelu_fwd(const float* x, const float* scale, const float* offset, float eps, float leak, float* y,
                           float* mean, float* invstd, int B, int HW, int C, void* ws, size_t ws_bytes, void* stream);
int cgs_instnorm_lrelu_bwd_data(const float* dy, const float* x, const float* scale, const float* offset,
                                const float* mean, const float* invstd, float leak, float* dx, int B, int HW, int C,
                                void* ws, size_t ws_bytes, void* stream);
/*   fwd of a norm over groups of rows from the partial sums the producing convolution left (cgs_conv_stat_layout): x is
 *   [groups][M_group][C], mean / invstd [groups][C]; ws >= groups * 4 * C floats.  Instance norm: groups = B, M_group = HW. */
int cgs_groupnorm_lrelu_fwd_from_partials(const float* x, const float* part, int groups, int rows_per_seg, int nseg, int seg_stride,
                                          const float* gamma, const float* beta, float eps, float leak, float* y, float* mean,
                                          float* invstd, int M_group, int C, void* ws, size_t ws_bytes, void* stream);
/* out = a + b (residual connections). */
int cgs_add(const float* a, const float* b, float* out, size_t n, void* stream);

/* Inference-mode bn folded to a per-channel affine (nsgan/GAN.py:87,94): a = gamma/sqrt(mv+eps), b = beta - a*mm. */
int cgs_bn_fold(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                float eps, float* a, float* b, int C, void* stream);
/* y = relu(a[c]*x + b[c]) and its input gradient dx = dy*(y>0)*a[c]  (G-tail bn+relu, nsgan/GAN.py:96-98). */
int cgs_affine_relu_fwd(const float* x, const float* a, const float* b, float* y, int M, int C, void* stream);
int cgs_affine_relu_bwd(const float* dy, const float* y, const float* a, float* dx, int M, int C, void* stream);
/* y = a[c]*x + b[c] (inference-mode bn with no activation after it) and dx = dy*a[c]. */
int cgs_affine_fwd(const float* x, const float* a, const float* b, float* y, int M, int C, void* stream);
int cgs_affine_bwd(const float* dy, const float* a, float* dx, int M, int C, void* stream);
/* y = max(x, leak*x) and dx = dy*(y>0 ? 1 : leak)   (nsgan/ops.py:69-70). */
int cgs_lrelu_fwd(const float* x, float leak, float* y, size_t n, void* stream);
int cgs_lrelu_bwd(const float* dy, const float* y, float leak, float* dx, size_t n, void* stream);
/* y = tanh(x), dx = dy*(1-y*y)   (nsgan/GAN.py:100). */
int cgs_tanh_fwd(const float* x, float* y, size_t n, void* stream);
int cgs_tanh_bwd(const float* dy, const float* y, float* dx, size_t n, void* stream);

/* Loss seed: dlogit = sigmoid(logit) - 1 = d softplus(-logit)/d logit, the gradient of
 * tf.nn.sigmoid_cross_entropy_with_logits(labels=1) summed over the batch (nsgan/GAN.py:176-177,
 * sampling/collaborator.py:31), and the per-sample mean logit over P patch entries
 * (sampling/collaborator.py:34-37).  logits is [B,P]. */
int cgs_bce_ones_grad_rowmean(const float* logits, float* dlogits, float* logit_mean, int B, int P, void* stream);
/* The loss seed of any refinement loss: dlogits = d loss(kind) / d logit (CGS_LOSS_BCE, _LSQ, _LINEAR; the gradient of the SUM of the
 * unreduced loss, collaborator.py:30-31) and logit_mean as cgs_bce_ones_grad_rowmean writes it, bit for bit, whatever the kind (the
 * selection of collaborator.py:76 does not depend on the loss).  kind CGS_LOSS_BCE gives that entry's dlogits bit for bit.
 * ladam: NULL, or the ladam rule's per-sample state, advanced by this launch (cgs_ladam_seed above). */
int cgs_refine_loss_seed(const float* logits, int kind, float* dlogits, float* logit_mean, int B, int P, const cgs_ladam_seed* ladam,
                         void* stream);

/* loss[i] = softplus(-logits[i]) = tf.nn.sigmoid_cross_entropy_with_logits(labels=1), unreduced (nsgan/GAN.py:176-177),
 * and its input gradient dlogits[i] = dloss[i] * (sigmoid(logits[i]) - 1)  (what tf.gradients emits, collaborator.py:31). */
int cgs_bce_ones_fwd(const float* logits, float* loss, size_t n, void* stream);
int cgs_bce_ones_bwd(const float* dloss, const float* logits, float* dlogits, size_t n, void* stream);
/* sigmoids[b] = mean over the P logits of sample b of sigmoid(logit): self.fake_sigmoids = tf.nn.sigmoid(self.fake_logits)
 * (nsgan/GAN.py:154-155; P = 1 there), the discriminator score the accept / reject step reads (nsgan/GAN.py:409,422). */
int cgs_sigmoid_rowmean(const float* logits, float* sigmoids, int B, int P, void* stream);
/* The GAN training losses unreduced, for the operator API (ops.least_squares_loss / hinge_loss): kind CGS_LOSS_LSQ (l - target)^2,
 * CGS_LOSS_HINGE relu(1 - l) at target 1 | relu(1 + l) at target 0, CGS_LOSS_LINEAR -l.  dloss == NULL: out[i] = loss(logits[i]);
 * else out[i] = dloss[i] * d loss / d logit (the formulas of cgs_gan_logits_grad). */
int cgs_gan_loss(const float* logits, int kind, float target, const float* dloss, float* out, size_t n, void* stream);
/* y = min(max(x, vmin), vmax): tf.clip_by_value on the refined map (sampling/collaborator.py:69-70). */
int cgs_clip(const float* x, float vmin, float vmax, float* y, size_t n, void* stream);

/* One refinement step's state update, fused (sampling/policy.py:31-37 momentum / :27-29 sgd,
 * sampling/collaborator.py:66-70 clip):
 *   m = first ? rate*g : alpha*m + rate*g ; theta -= m ; theta = clip(theta, vmin, vmax) if use_clip.
 * alpha = 0 and first = 1 give sgd.  n = B*F elements. */
int cgs_refine_update(float* theta, float* m, const float* g, float rate, float alpha, int first,
                      int use_clip, float vmin, float vmax, size_t n, void* stream);
/* The ladam state of cgs_ladam_seed from a per-sample loss[B] the caller already holds on the device (PolicyAdaptive.apply_gradient with
 * a loss): loss_avg = first ? loss : 0.5 * loss_avg + 0.5 * loss; gain = clamp(loss_avg + 0.5, 0, 1e4)^2. */
int cgs_ladam_gain(const float* loss, float* loss_avg, float* gain, int first, int B, void* stream);
/* The ladam rule on activation maps (sampling/policy.py:53-59 with :48-51 done by the seed launch), one pass, per element i of B*F:
 *   m = first ? g : 0.9*m + c1*g ;  v = first ? g*g : 0.5*v + c2*(g*g) ;  theta -= (rate*m / (sqrt(v) + 1e-8)) * gain[i / F]
 * then the clip of cgs_refine_update.  c1 = (float)(1.0 - 0.9), c2 = (float)(1.0 - 0.5).  Every operation is rounded on its own, in
 * this order.  gain: the B floats a seed launch given a cgs_ladam_seed, or cgs_ladam_gain, left. */
int cgs_refine_update_ladam(float* theta, float* m, float* v, const float* g, const float* gain, float rate, int first, int use_clip,
                            float vmin, float vmax, int B, int F, void* stream);
/* Best-sample selection (sampling/collaborator.py:76-83): for each sample b
 *   upd = forced ? forced[b] == step_index : logit[b] > best_logit[b]      (strict >)
 *   best_logit[b], best_theta[b,:], best_step[b] = upd ? (logit[b], theta[b,:], step_index+1) : unchanged
 * forced = the probabilistic-mode index vector (int32, device) or NULL for deterministic mode. */
int cgs_refine_select(const float* theta, const float* logit, const int32_t* forced, int step_index,
                      float* best_theta, float* best_logit, float* best_step, int B, int F, void* stream);
/* cgs_refine_select_rows(rows -> best_rows) followed by cgs_refine_select(theta -> best_theta, scalars) with the two row copies in one
 * launch: the per-step bookkeeping of the engine (the rendered image follows the selection of the refined map).
 * tickets: NULL, or B ints of device memory that are ZERO at the call and are left zero by it (the caller clears them once and hands the
 * same buffer to every call on one stream): the scalars are then updated in the same launch, by the last block of each selected sample. */
int cgs_refine_select2(const float* rows, float* best_rows, int Frows, const float* theta, float* best_theta, int F, const float* logit,
                       const int32_t* forced, int step_index, float* best_logit, float* best_step, int* tickets, int B, void* stream);
/* The row copy of cgs_refine_select alone (same predicate, best_logit is only read): lets a second per-sample
 * tensor -- e.g. the rendered image of the step -- follow the same selection.  Call it BEFORE cgs_refine_select. */
int cgs_refine_select_rows(const float* src, const float* logit, const int32_t* forced, int step_index, float* dst,
                           const float* best_logit, int B, int F, void* stream);

/* ---- the 2-D path (BASELINE config 1: synthetic/ MLP GAN) ----------------------------------------------------------
 * ReLU MLP discriminator on 2-D points, 2 -> nhidden x (nlayers-1) -> 1 (synthetic/GAN.py:28-37); w[l] is layer l's
 * [din,dout] kernel (tf.layers.dense), b[l] its bias; w / b are HOST arrays of nlayers DEVICE pointers; nlayers 2..6.
 * cgs_mlp2d_sigmoid_saliency, cgs_refine2d and cgs_refine2d_devbase take 1 <= nhidden <= 256, chosen by nhidden alone: up to 64 the
 * one-wave-per-sample kernels with every layer in LDS (mlp2d.hip); 65..256 (the 25-Gaussians D: 256 x 6) the sample-tile kernels on
 * v_mfma_f32_32x32x2_f32 with the weights streamed from L2 (mlp2d_wide.hip).  The training entry points below stay at nhidden <= 64; the D step, the
 * generator's forward and the G step have second entry points for 65..256 (cgs_mlp2d_wide_d_step, cgs_mlp2d_wide_gen_fwd, cgs_mlp2d_wide_g_step).
 *   sigmoid[B]    = sigmoid(D(x))                                              synthetic/GAN.py:108
 *   saliency[B,2] = inv_batch * d sum_b softplus(-logit_b) / dx  (inv_batch = 1/B keeps the reduce_mean factor of :109-111)
 * saliency may be NULL. */
int cgs_mlp2d_sigmoid_saliency(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x,
                               float* sigmoid, float* saliency, int B, float inv_batch, void* stream);
/* The whole host loop of sampling/refiner_cpu.py:26-66 in one launch (nhidden <= 64: one wave per sample; 65..256: a tile of 32 or
 * 64 samples per workgroup, no workspace either way): K steps of
 * sgd (method 0) / momentum (1) / ladam (2) (sampling/policy.py:26-61) on x[B,2] with loss = real_sigmoid_mean - sigmoid,
 * best-loss tracking (best_x[B,2], best_step[B]) and, if traj != NULL, the trajectory traj[B,K+1,2]. */
int cgs_refine2d(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x,
                 float real_sigmoid_mean, float inv_batch, int steps, float rate, int method,
                 float* best_x, float* best_step, float* traj, int B, void* stream);

/* The same with the baseline read from DEVICE memory (one float): the real batch's mean sigmoid never visits the host, so
 * consecutive batches queue without a synchronisation.  nhidden <= 256 like cgs_refine2d. */
int cgs_refine2d_devbase(const float* const* w, const float* const* b, int nlayers, int nhidden, const float* x,
                         const float* real_sigmoid_mean_dev, float inv_batch, int steps, float rate, int method,
                         float* best_x, float* best_step, float* traj, int B, void* stream);

/* The 2-D net's D shaping step (synthetic/main.py:366-370): gradients of
 *   d_loss = mean_b BCE(D(real_b), 1) + mean_b BCE(D(fake_b), 0)                     synthetic/GAN.py:69-74
 * w.r.t. every D variable and, if lr != 0, tf.train.GradientDescentOptimizer(lr)'s step w -= lr*g IN PLACE (synthetic/GAN.py:98-99).
 * w / b (and the optional gw / gb gradient outputs, same shapes; NULL or NULL entries = not returned) are HOST arrays of nlayers
 * DEVICE pointers; loss (device, 2 floats, may be NULL) <- (d_loss_real, d_loss_fake) BEFORE the update.  Deterministic
 * (fixed summation order).  nhidden <= 64.  ws: cgs_mlp2d_train_ws_bytes(B_real + B_fake, nlayers). */
size_t cgs_mlp2d_train_ws_bytes(int B_total, int nlayers);
int cgs_mlp2d_d_step(float* const* w, float* const* b, int nlayers, int nhidden, const float* real, int B_real,
                     const float* fake, int B_fake, float lr, float* const* gw, float* const* gb, float* loss,
                     void* ws, size_t ws_bytes, void* stream);

/* The same step for 65 <= nhidden <= 256 (mlp2d_wide_train.hip; nlayers 2..6; anything else: CGS_EINVAL): arguments and meaning as
 * cgs_mlp2d_d_step.  A sample tile per workgroup keeps every layer's activation and masked pre-activation gradient in the workspace;
 * the hidden -> hidden weight gradients are [nhidden x B_total] . [B_total x nhidden] products on v_mfma_f32_32x32x2_f32 over sample
 * chunks whose size depends on B_total alone, their partial tiles added in chunk order: deterministic, no atomics.  The workspace layout
 * is internal; ws: cgs_mlp2d_wide_train_ws_bytes(B_real + B_fake, nlayers, nhidden) (0 on a bad argument), CGS_EWORKSPACE if smaller. */
size_t cgs_mlp2d_wide_train_ws_bytes(int B_total, int nlayers, int nhidden);
int cgs_mlp2d_wide_d_step(float* const* w, float* const* b, int nlayers, int nhidden, const float* real, int B_real,
                          const float* fake, int B_fake, float lr, float* const* gw, float* const* gb, float* loss,
                          void* ws, size_t ws_bytes, void* stream);

/* The 2-D generator G (synthetic/GAN.py:39-49): z[B,2] -> dense(2->nh) -> BN -> ReLU -> [dense(nh->nh) -> BN -> ReLU] x (nlayers-2)
 * -> dense(nh->2) -> x[B,2], BN = tf.contrib.layers.batch_norm(decay=0.9, epsilon, scale=True, updates_collections=None).
 * w / b: HOST arrays of nlayers DEVICE pointers (w[l] the [din,dout] kernel of generator/g_fc<l+1>); gamma / beta / moving_mean /
 * moving_variance: HOST arrays of nlayers-1 DEVICE pointers ([nhidden] each: generator/BatchNorm[_k]/...).  nlayers 2..6, nhidden <= 64.
 * Training mode (is_training != 0, B >= 2; gan.generates, GAN.py:63): BN normalises with the batch mean and biased variance and, as part
 * of the same call (updates_collections=None), moves moving_mean / moving_variance IN PLACE: v -= (v - value) * 0.1, value = the batch
 * mean / the Bessel-corrected batch variance (what TF 1.x's FusedBatchNorm returns as batch_variance).  batch_stats (device, may be NULL): [nlayers-1][2][nhidden]
 * <- (mean, biased variance) of every BN layer.  Inference mode (gan.fake_samples, GAN.py:105): the moving statistics, nothing
 * written but x.  Deterministic (fixed summation order, no atomics).  ws: cgs_mlp2d_gen_ws_bytes(B, nlayers, 0). */
size_t cgs_mlp2d_gen_ws_bytes(int B, int nlayers, int with_backward);
int cgs_mlp2d_gen_fwd(const float* const* w, const float* const* b, const float* const* gamma, const float* const* beta,
                      float* const* moving_mean, float* const* moving_variance, int nlayers, int nhidden, const float* z, float* x, int B,
                      int is_training, float eps, float* batch_stats, void* ws, size_t ws_bytes, void* stream);
/* The same forward for 65 <= nhidden <= 256 (mlp2d_wide_gen.hip; nlayers 2..6; anything else: CGS_EINVAL): arguments and meaning as
 * cgs_mlp2d_gen_fwd, B <= 2^24.  A sample tile per workgroup, the hidden -> hidden layers on v_mfma_f32_32x32x2_f32 with the weights
 * streamed from L2; training mode is one launch per dense layer, inference mode one launch.  The batch statistics are (mean, M2) partials
 * of fixed groups of 32 consecutive rows combined in ascending order: a function of the inputs and B alone.  Deterministic, no atomics.
 * The workspace keeps every BN layer's pre-activations [nlayers-1][B][nhp] (nhp = nhidden rounded up to 32, padded units zero), which the
 * generator's backward needs, then the group partials and the per-layer (mean, rstd) rows:
 *   cgs_mlp2d_wide_gen_ws_bytes(B, nlayers, nhidden) = 4 (nlayers-1) nhp (B + 2 ceil(B / 32) + 2)   (0 on a bad argument);
 * CGS_EWORKSPACE if smaller (both modes).  The G update at this width is cgs_mlp2d_wide_g_step below. */
size_t cgs_mlp2d_wide_gen_ws_bytes(int B, int nlayers, int nhidden);
int cgs_mlp2d_wide_gen_fwd(const float* const* w, const float* const* b, const float* const* gamma, const float* const* beta,
                           float* const* moving_mean, float* const* moving_variance, int nlayers, int nhidden, const float* z, float* x,
                           int B, int is_training, float eps, float* batch_stats, void* ws, size_t ws_bytes, void* stream);
/* The G update g_optim (GAN.py:83-101, run at synthetic/main.py:379-380): a training-mode forward on z (moving statistics updated as
 * above; x[B,2] <- G(z) if x != NULL), the gradients tf.gradients(generates, g_vars, grad_plugin) of every g_fc kernel and bias back
 * through the training-mode BN, and, if lr != 0, GradientDescentOptimizer(lr)'s w -= lr*g IN PLACE.  g_vars holds only the names with
 * 'g_' (GAN.py:84): gamma / beta are never written.  gw / gb: optional gradient outputs like cgs_mlp2d_d_step's.  Deterministic.
 * ws: cgs_mlp2d_gen_ws_bytes(B, nlayers, 1). */
int cgs_mlp2d_g_step(float* const* w, float* const* b, const float* const* gamma, const float* const* beta, float* const* moving_mean,
                     float* const* moving_variance, int nlayers, int nhidden, const float* z, const float* grad_plugin, int B, float eps,
                     float lr, float* const* gw, float* const* gb, float* x, void* ws, size_t ws_bytes, void* stream);
/* The same update for 65 <= nhidden <= 256 (mlp2d_wide_gstep.hip; nlayers 2..6; anything else: CGS_EINVAL), 2 <= B <= 2^24: arguments,
 * meaning and order of checks as cgs_mlp2d_g_step.  The forward is cgs_mlp2d_wide_gen_fwd on the first bytes of the workspace; the way
 * back is one launch per BN layer on the same sample tiles (hidden -> hidden layers on v_mfma_f32_32x32x2_f32), the batch sums of the BN
 * backward from fixed groups of 32 rows added in ascending order, the hidden -> hidden weight gradients MFMA products over sample chunks
 * whose size depends on B alone, added in chunk order: a function of the inputs and B alone, no atomics.  The rest of the workspace is
 * internal; ws: cgs_mlp2d_wide_g_step_ws_bytes(B, nlayers, nhidden) (0 on a bad argument), CGS_EWORKSPACE if smaller. */
size_t cgs_mlp2d_wide_g_step_ws_bytes(int B, int nlayers, int nhidden);
int cgs_mlp2d_wide_g_step(float* const* w, float* const* b, const float* const* gamma, const float* const* beta, float* const* moving_mean,
                          float* const* moving_variance, int nlayers, int nhidden, const float* z, const float* grad_plugin, int B, float eps,
                          float lr, float* const* gw, float* const* gb, float* x, void* ws, size_t ws_bytes, void* stream);

/* ---- discriminator shaping step (the caller after the refinement path: nsgan/GAN.py:270-272, 126-146) ----------
 * Weight gradients of D's layers, the BCE seed with 0/1 targets, and the Adam update.  NOT part of the frozen-weight
 * refinement loop; provided so the method's only training step (shape D on refined samples) runs on the same ABI. */
/* dw[kh,kw,Cin,Cout] (+)= d/dw of conv2d_nhwc_fwd(x, w) contracted with dy[B,Ho,Wo,Cout] (Conv2DBackpropFilter). */
size_t cgs_conv_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw);
int cgs_conv2d_nhwc_bwd_weight(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                               int kh, int kw, int sh, int sw, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dw[kh,kw,Cout,Cin] (+)= d/dw of deconv2d_nhwc_fwd(x, w) contracted with dy[B,Hout,Wout,Cout]: the generator's update (nsgan/GAN.py:132-146
 * through nsgan/ops.py:48-67).  The same kernels, split plan and fixed-order slab reduction as the conv entry with the roles swapped (the filter
 * is that of the 'SAME' conv Hout -> Hin: big = dy, small = x, reduction over the B*Hin*Win pixels of x); no atomics, a function of the inputs
 * alone.  CGS_EINVAL unless (Hout, Wout) is a 'SAME' pre-image of (Hin, Win) (ceil(Hout/sh) == Hin, ceil(Wout/sw) == Win; the query then
 * returns 0); CGS_EWORKSPACE below cgs_deconv_wgrad_ws_bytes of the same arguments. */
size_t cgs_deconv_wgrad_ws_bytes(int B, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int kh, int kw, int sh, int sw);
int cgs_deconv2d_nhwc_bwd_weight(const float* x, const float* dy, float* dw, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Cout,
                                 int kh, int kw, int sh, int sw, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dw[in,out] (+)= x[B,in]^T dy[B,out]   (ws: cgs_conv_wgrad_ws_bytes(B,1,1,in,out,1,1,1,1)). */
int cgs_linear_bwd_weight(const float* x, const float* dy, float* dw, int B, int in, int out, int accumulate,
                          void* ws, size_t ws_bytes, void* stream);
/* db[C] (+)= column sums of dy[M,C]   (ws: cgs_bn_ws_bytes(M, C)). */
int cgs_bias_grad(const float* dy, float* db, int M, int C, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dgamma, dbeta (+)= from the statistics the immediately preceding cgs_bn_train_lrelu_bwd_data call left in ITS
 * workspace `bwd_ws` (same M, C). */
int cgs_bn_train_param_grads(const void* bwd_ws, int M, int C, float* dgamma, float* dbeta, int accumulate, void* stream);
/* The D step of a PatchGAN discriminator (BASELINE config 5; the reference ships no code for it: the same step, nsgan/GAN.py:270-272,
 * on a logit MAP -- shaping.DShaper._backward).
 * dscale, doffset [C] (+)= the instance norm's parameter gradients from the per-sample sums {mean(d), mean(d * xhat)} the immediately
 * preceding cgs_instnorm_lrelu_bwd_data call left in ITS workspace `bwd_ws` (same B, HW, C; either of its paths):
 * doffset[c] = HW * sum_b mean_b(d), dscale[c] = HW * sum_b mean_b(d * xhat), the samples added in ascending order in double.
 * Deterministic, no atomics. */
int cgs_instnorm_param_grads(const void* bwd_ws, int B, int HW, int C, float* dscale, float* doffset, int accumulate, void* stream);
/* dw[kh,kw,Cin] (+)= weight gradient of a 'SAME' convolution to ONE output channel over a deep reduction, dy [B,Ho,Wo] (the PatchGAN
 * logit head 4x4 x 512 -> 1; the backward-weight twin of the forward's dot-product family, wgrad_dot.hip).  Takes what that family
 * takes: Cin % 4 == 0, kh * kw * Cin >= 1024, sh == sw, x 16-byte aligned; anything else is CGS_EINVAL before any launch (the query
 * then returns 0) -- cgs_conv2d_nhwc_bwd_weight serves every shape.  The B * Ho * Wo pixels are cut into slabs, one partial dw per slab
 * in the workspace, added in slab order: no atomics, a function of the inputs alone.  Padding taps are not read.
 * ws: cgs_conv_wgrad_cout1_ws_bytes of the same arguments, 16-byte aligned; CGS_EWORKSPACE if smaller. */
size_t cgs_conv_wgrad_cout1_ws_bytes(int B, int H, int W, int Cin, int kh, int kw, int sh, int sw);
int cgs_conv2d_nhwc_bwd_weight_cout1(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int kh, int kw,
                                     int sh, int sw, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dlogits[i] = scale*(sigmoid(logits[i]) - target); loss_sum[0] = scale * sum_i BCE(logits[i], target) (may be NULL).
 * tf.nn.sigmoid_cross_entropy_with_logits + reduce_mean (nsgan/GAN.py:126-131) with scale = 1/n. */
int cgs_bce_logits_grad(const float* logits, float target, float scale, float* dlogits, float* loss_sum, int n, void* stream);
/* The same seed for the other GAN training losses, one block, the same fixed-order sum.  With t = target (1 real, 0 fake; the
 * generator's step is CGS_LOSS_LSQ with target 1, or CGS_LOSS_LINEAR):
 *   CGS_LOSS_BCE     as cgs_bce_logits_grad, bit for bit
 *   CGS_LOSS_LSQ     loss (l - t)^2                      dl = scale * 2 (l - t)
 *   CGS_LOSS_HINGE   loss relu(1 - l) | relu(1 + l)      dl = scale * (l < 1 ? -1 : 0) | scale * (l > -1 ? 1 : 0)
 *   CGS_LOSS_LINEAR  loss -l                             dl = -scale
 * loss_sum[0] = scale * sum_i loss_i (may be NULL).  target must be 0 or 1 for CGS_LOSS_HINGE. */
int cgs_gan_logits_grad(const float* logits, int kind, float target, float scale, float* dlogits, float* loss_sum, int n, void* stream);
/* Adam (tf.train.AdamOptimizer semantics, nsgan/GAN.py:141-146): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * w -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) supplied by the caller. */
int cgs_adam_step(float* w, const float* g, float* m, float* v, float lr_t, float beta1, float beta2, float eps,
                  size_t n, void* stream);
/* The Adam step of EVERY variable of one optimizer in one launch (the d_optim / g_optim of nsgan/GAN.py:141-146, as
 * training.GanTrainer's captured iteration runs them: cgs_amd/kernels.py::AdamTable.step).  `table` [n_slots] and `plan` [n_chunks] are
 * DEVICE arrays the host builds once: block b of the launch updates elements [begin, begin + count) of slot plan[b].slot, chunks are
 * disjoint, never cross a slot, and cover every element once (kernels.adam_chunk_plan).  A slot with n == 0 is legal and gets no chunk.
 * `lr_t` is read from DEVICE memory, so the launch has the same arguments at every step and a captured hipGraph replays it; the
 * host writes the step's value there in stream order.  Per element the arithmetic is cgs_adam_step's own (one shared device
 * function).  No atomics, no host synchronisation.  Refuses n_slots <= 0, a null table, a null lr_t, a null plan with n_chunks > 0. */
typedef struct cgs_adam_slot {
    float* w;
    const float* g;
    float* m;
    float* v;
    unsigned long long n;
} cgs_adam_slot;
typedef struct cgs_adam_chunk {
    int slot;
    unsigned count;
    unsigned long long begin;
} cgs_adam_chunk;
int cgs_adam_multi(const cgs_adam_slot* table, int n_slots, const cgs_adam_chunk* plan, int n_chunks, const float* lr_t,
                   float beta1, float beta2, float eps, void* stream);
/* The moving averages of one batch norm (ops.bn, nsgan/ops.py:19-26, as generator(z, is_training=True) moves them at nsgan/GAN.py:120) from
 * the statistics its training-mode forward saved: moving_mean = decay * moving_mean + (1 - decay) * mean, and the same for moving_var with
 * the biased batch variance 1 / invstd^2 - eps.  One launch per norm (training.GStepper.forward on the captured path).  `decay` is a
 * double so that 1 - decay is rounded to float once. */
int cgs_bn_moving_update(const float* mean, const float* invstd, float* moving_mean, float* moving_var, int C, double decay,
                         float eps, void* stream);

/* Streaming Frechet statistics of a pool of feature vectors (metrics.PoolMoments; the FD row of the reference's evaluate loop,
 * nsgan/GAN.py:306, without ever holding the pool): with a_i = (double)x[r_i] - (double)shift,
 *   sum[j] += sum_i a_ij        gram[j][k] += sum_i a_ij * a_ik        (both ADDED to; double throughout, v_mfma_f64_16x16x4_f64)
 * x: [n][d] fp32 row-major contiguous, below 2 GiB.  rows == NULL: the n rows of x (m is then only checked to be >= 0); else m row
 * indices into x, which the kernel TRUSTS (0 <= rows[i] < n is the caller's duty; a row may repeat).  shift: [d] or NULL (= 0).
 * 1 <= d <= 2048; anything else is CGS_EINVAL before any launch (the query then returns 0); no sample (m == 0 with rows, n == 0 without) is
 * a no-op that launches nothing and dereferences nothing.  Only tile pairs on or above the diagonal are computed and the mirror is
 * written from the same values: gram stays exactly symmetric if it was.  The samples are cut into slabs whose number depends on
 * (m, d) alone, each slab leaves its partial tiles in the workspace, and a second launch adds them in ascending order: no atomics,
 * reruns are bit-equal.  ws: cgs_pool_moments_ws_bytes(m, d) bytes for m samples, 8-byte aligned; CGS_EWORKSPACE if smaller. */
size_t cgs_pool_moments_ws_bytes(int m, int d);
int cgs_pool_moments_accumulate(const float* x, int n, int d, const int* rows, int m, const float* shift, double* sum, double* gram,
                                void* ws, size_t ws_bytes, void* stream);
/* out[b][c] = mean over the HW pixels of x[b][.][c] (x: [B][HW][C]), summed in double and rounded once: a conv discriminator's feature
 * map as one vector per sample (engine.RefineEngine.score_with_features). */
int cgs_spatial_mean(const float* x, float* out, int B, int HW, int C, void* stream);

/* ---- the Frechet distance of two pools from their moment states, on the device (csrc/frechet.hip) ----
 * cgs_f64_matmul: C = alpha * A * B + diag * I for row-major d x d doubles, 1 <= d <= 2048; every product and sum a double operation on
 * v_mfma_f64_16x16x4_f64, each result one accumulation chain in ascending k (no K split, no atomics: reruns are bit-equal).  B is a
 * general matrix.  c must not alias a or b.  d out of range, a null pointer or an aliased c: CGS_EINVAL before any launch.
 * cgs_frechet_from_moments: sum / gram are the device doubles of a metrics.PoolMoments ([d] and [d][d]), shift a device float [d] or
 * NULL (= 0), n the number of rows behind them.  With
 *     mean = shift + sum / n        cov = (gram - sum sum^T / n) / (n - ddof), symmetrised  (shift-invariant: the pools' shifts may differ)
 *     dmu  = ((double)shift_r - (double)shift_f) + sum_r / n_r - sum_f / n_f
 * out (8 device doubles) receives
 *     [0] fd = |dmu|^2 + Tr S_r + Tr S_f - 2 Tr (S_r^{1/2} S_f S_r^{1/2})^{1/2}     [1] |dmu|^2     [2] Tr S_r     [3] Tr S_f
 *     [4] Tr (S_r^{1/2} S_f S_r^{1/2})^{1/2}  (= Tr (S_r S_f)^{1/2})     [5] / [6] iterations used by the first / second root
 *     [7] status: 0 = tolerance met, 1 = stalled and the last good iterate kept, 2 = iteration cap  (the larger of the two roots')
 * Both roots are of symmetric positive semi-definite matrices, by the coupled Newton-Schulz iteration on A / |A|_F (three products per
 * step); a step is accepted while the trace still converges, the iteration stops at |delta Tr| <= max(1e-15, d 2^-52) Tr, or -- from the
 * fifth step on -- discards the step at which |delta Tr| stops shrinking below 1e-6 Tr, or at max_iters.  An exactly zero covariance has
 * root 0 (no division).  Everything is queued on `stream`: no host synchronisation, no read-back; the stop decision is taken on the
 * device (traces and norms reduced in a fixed order, a rerun is bit-equal) and turns the remaining queued launches -- their number is
 * fixed by max_iters -- into early exits.  ws: cgs_frechet_ws_bytes(d) bytes, 8-byte aligned; nothing past them is written.
 * CGS_EINVAL before any launch: d outside 1..2048 (the query then returns 0), n <= 0 or n - ddof <= 0, a null sum / gram / out, a
 * misaligned workspace, max_iters outside 1..64; CGS_EWORKSPACE: a null or short workspace. */
int cgs_f64_matmul(const double* a, const double* b, double* c, int d, double alpha, double diag, void* stream);
size_t cgs_frechet_ws_bytes(int d);
int cgs_frechet_from_moments(const double* sum_r, const double* gram_r, const float* shift_r, long long n_r, const double* sum_f,
                             const double* gram_f, const float* shift_f, long long n_f, int d, int ddof, int max_iters, double* out, void* ws,
                             size_t ws_bytes, void* stream);

/* ---- calibration and 2-D mode statistics of a pool, additive, in double on the device (csrc/diagnostics.hip) ----
 * Calibration of D's scores (the reference's calibration_diagnostic, sampling/utils_sampling.py:186-299).  p: n fp32 scores, widened to
 * double exactly; label: 0 (fake) or 1 (real), one per call; edges: n_bins + 1 ascending doubles ON THE DEVICE
 * (np.linspace(0., 1. + 1e-8, n_bins + 1) on the host); 1 <= n_bins <= 64.  The slot of a score is the number of edges <= p, minus one,
 * compared in double (np.digitize(p, edges) - 1): S = n_bins + 1 slots, the last one catching p >= edges[n_bins] and NaN.  A score
 * below edges[0] is counted in `under` and nowhere else.  The call ADDS to state, 3 S + 11 doubles:
 *     [0, S)       count per slot            [S, 2S)  sum of p per slot            [2S, 3S)  sum of y per slot
 *     3S + 0..4    n | sum (y - p) | sum p (1 - p) | sum (y - p)^2 | under
 *     3S + 5 + 3y  n_y | sum of p | max of p   over the scores of label y (y = 0, 1; max: NaN ignored; the other label's three stay)
 * Counts are doubles holding integers (exact below 2^53).  Every sum is a double sum in an order fixed by (n, n_bins): blocks over
 * contiguous chunks leave one partial row each in ws, a one-block launch adds the rows in ascending order (max for the maximum) and
 * then to state; no floating-point atomics, so two calls on the same inputs from the same state end bit-equal.
 * Modes of a 2-D pool (utils_sampling.py:132-161).  x: [n][2] fp32; centeroids: [k][2] doubles ON THE DEVICE, 1 <= k <= 64.  Per sample and
 * mode dist = sqrt(dx * dx + dy * dy) with dx = double(x0) - c0, dy = double(x1) - c1, products and sum rounded separately (numpy's
 * linalg.norm).  The call ADDS to state, k + 3 doubles:
 *     [0, k)  samples with dist_j < thres (a sample may hit several modes)     k: n | k + 1: samples with min_j dist_j < thres | k + 2: sum of min_j dist_j
 * Errors: n_bins / k / label out of range or n < 0 or n > 2^30 is CGS_EINVAL before any launch (the query then returns 0); n == 0 is a
 * no-op that dereferences nothing (query 0); ws: *_ws_bytes(n, .) bytes, 8-byte aligned, CGS_EWORKSPACE if smaller. */
size_t cgs_calibration_ws_bytes(int n, int n_bins);
int cgs_calibration_accumulate(const float* p, int n, int label, const double* edges, int n_bins, double* state, void* ws, size_t ws_bytes,
                               void* stream);
size_t cgs_mode_stats_ws_bytes(int n, int k);
int cgs_mode_stats_accumulate(const float* x, int n, const double* centeroids, int k, double thres, double* state, void* ws, size_t ws_bytes,
                              void* stream);

/* ---- the density map of a 2-D sample pool on a grid, additive, in double on the device (csrc/kde2d.hip) ----
 * The arithmetic of the reference's draw_kde (sampling/utils_sampling.py:97-112).  x: [n][2] fp32; axis_x: gx fp32 coordinates, axis_y:
 * gy; whiten: the three doubles w00, w10, w11 of the lower-triangular W = L^-1, C = L L^T the kernel covariance, ON THE DEVICE.  The
 * call ADDS to state, gx * gy + 1 contiguous doubles:
 *     [i * gy + j]  sum_k exp(-1/2 |W (g_ij - x_k)|^2),  g_ij = (axis_x[i], axis_y[j])  (UN-normalised)        [gx * gy]  n
 * The density is state[i * gy + j] / (state[gx * gy] * 2 pi sqrt(det C)), sqrt(det C) = 1 / (w00 w11): the reader's division.  Per pair
 * the difference of the raw fp32 coordinates is taken first and whitened after, in fp32, through v_exp_f32; fp32 sums run over at most
 * 128 samples and are then added in double.  The samples are cut into slices whose number depends on (n, gx * gy) alone, each slice
 * leaves one double per cell in ws, a second launch adds them in ascending order and then to state: no floating-point atomics, two
 * calls on the same inputs from the same state end bit-equal.
 * Errors: gx < 1, gy < 1, gx * gy > 2^20, n < 0 or n > 2^30 is CGS_EINVAL before any launch (the query then returns 0); n == 0 is a no-op
 * that dereferences nothing (query 0); ws: cgs_kde2d_ws_bytes(n, gx, gy) bytes, 8-byte aligned, CGS_EWORKSPACE if smaller. */
size_t cgs_kde2d_ws_bytes(int n, int gx, int gy);
int cgs_kde2d_accumulate(const float* x, int n, const float* axis_x, int gx, const float* axis_y, int gy, const double* whiten, double* state,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- discriminator rejection sampling on the device (csrc/drs.hip) ----
 * cgs_drs_decide: the accept decision of the reference's Rejector (sampling/rejector.py:16-34: acceptance_probability and sampling), once
 * per logical batch.  sig: groups * b fp32 sigmoids, group g = rows [g b, (g + 1) b); uniforms: one double per row ON THE DEVICE (the
 * host draws them: np.random.rand(b) per group, in group order); state: one double on the device, the running bound D_tilde_M.  Per
 * group, in order, as if rejector.sampling had been called once per batch:
 *     d = logit(clip(double(s), 1e-14, 1 - 1e-14))          M_g = max(M_{g-1}, max d)   (M_{-1} = *state; *state leaves as M_{groups-1})
 *     F = (d - M_g) - log(1 - exp((d - M_g) - epsilon))     gamma = percentile(F over the group, shift_percent), numpy's linear method
 *     P = 1 / (1 + exp(-(F - gamma)))                       mask = uniforms < P                   counts[g] = rows of the group accepted
 * shift_percent in [0, 100], or any negative value for the reference's shift_percent=None (gamma = 0).  The two order statistics behind
 * gamma come from an exact radix select; every operation is a separately rounded double one in the reference's order (1 - exp(x), not
 * -expm1(x)), logit in scipy.special's form.  bounds (NULL or groups doubles): M_g per group; P (NULL or one double per row); mask: one
 * byte per row, 0 or 1; counts: groups ints.  No floating-point atomics: a rerun from the same state is bit-equal.  A NaN score is not
 * supported.  ws: cgs_drs_ws_bytes(b, groups) bytes, 8-byte aligned, CGS_EWORKSPACE if smaller; b < 1, groups < 1 or > 2^20,
 * b * groups > 2^30, shift_percent > 100 or NaN, epsilon <= 0: CGS_EINVAL before any launch (the query then returns 0).
 * cgs_drs_set_max: *state = logit(clip(max of the n scores)) (rejector.py:11-14 on np.amax(sigmoid_real), nsgan/GAN.py:314).
 * cgs_compact_rows: the stable compaction behind eval_reject[cnt:cnt + k] = batch[accept] (nsgan/GAN.py:324-338, synthetic/main.py:161-167).
 * src: [n][row] fp32; the rows i with mask[i] != 0, or every row of group i / (n / groups) if take_all (NULL or groups bytes) flags it (the
 * "too inefficient" branch, GAN.py:332-338), are copied in ascending order of i to dst[offset + k], k = 0, 1, ...; rows with
 * offset + k >= capacity are dropped (dst: at least capacity rows); *total (a device int) = the UNCLIPPED number of selected rows.  n == 0
 * writes *total = 0 and nothing else.  ws: cgs_compact_rows_ws_bytes(n) bytes, 4-byte aligned.  n outside [0, 2^30] or no whole number of
 * groups, row outside [1, 2^22], n * row > 2^40, offset < 0, capacity < 0: CGS_EINVAL before any launch. */
size_t cgs_drs_ws_bytes(int b, int groups);
int cgs_drs_decide(const float* sig, int b, int groups, const double* uniforms, double epsilon, double shift_percent, double* state, double* bounds,
                   double* P, unsigned char* mask, int* counts, void* ws, size_t ws_bytes, void* stream);
int cgs_drs_set_max(const float* sig, int n, double* state, void* stream);
size_t cgs_compact_rows_ws_bytes(int n);
int cgs_compact_rows(const float* src, int n, int row, const unsigned char* mask, const unsigned char* take_all, int groups, float* dst, long long offset,
                     long long capacity, int* total, void* ws, size_t ws_bytes, void* stream);

/* ---- the Metropolis-Hastings independence chain on the device (csrc/mh.hip) ----
 * cgs_mh_walk: what the reference's IndependenceSampler (sampling/idpsampler.py:4-53) emits, once per logical batch ("segment").  sig:
 * groups * b fp32 sigmoids, segment g = rows [g b, (g + 1) b); uniforms: one double per row ON THE DEVICE (the host draws them:
 * np.random.uniform(0, 1, size=b) per walked segment, in segment order); state: two doubles on the device, d (the score of the chain's
 * current state; the chain must be started) and cnt (visits since the last emission), both carried from segment to segment and from
 * call to call.  Per proposal i of a segment, in order, every operation a separately rounded fp32 one, in this order:
 *     odds  = (s_i * omd) / (df * (1.0f - s_i))        omd = (float)(1.0 - d), df = (float)d, d held as a double
 *     alpha = odds < 1.0f ? odds : 1.0f                (Python's min(1.0, odds): a NaN gives 1.0)
 *     moved = !(u_i > (double)alpha);  if moved: d = s_i
 * and per segment, from the positions pos[0] < pos[1] < ... of its moves (the burn-in B counts moves of THIS segment, the held row is
 * reset per segment): nothing is emitted unless the segment has more than B moves; first = pos[B]; the visits v = first .. b - 1 are
 * active, a = v - first; emissions at a = a0, a0 + (T + 1), a0 + 2 (T + 1), ..., a0 = max(0, T + 1 - cnt); the emitted row is the last
 * move position <= v; cnt afterwards = 1 + (active visits after the last emission), or cnt + (active visits) if nothing was emitted.
 * This is numpy 2's arithmetic for fp32 scores and a Python-float or np.float32 seed; float64 scores or an np.float64 seed (numpy then
 * promotes the ratio to double) are not this entry point's.  Scores outside [0, 1] or NaN: an unspecified in-range result, no fault.
 * The segments are taken in order.  fill (one device long long): the UNCLIPPED number of rows the pool has received so far.  A segment
 * that starts with *fill >= capacity is NOT walked: counts[g] = -1, state untouched, nothing listed -- rounds queued ahead of the one that
 * fills the pool leave the chain where the reference's loop would.  A segment flagged in take_all (NULL or groups bytes) is not walked
 * either: its b rows are listed in order, counts[g] = b, state untouched (the "too inefficient" branch, nsgan/GAN.py:369-375,420-426).
 * Every other segment is walked; then *fill += counts[g], also past capacity.  rows (groups * b ints): indices into the call's rows, in
 * emission order; counts: groups ints; span (2 long long): {*fill at entry, rows listed by this call}.  One wavefront owns the chain: it
 * tests a window of 64 proposals against the current state at once and jumps to the first that moves (moves + windows serial steps); the
 * emissions follow from the move positions in closed form over the block.  No atomics: a rerun from the same state is bit-equal.
 * ws: cgs_mh_ws_bytes(b, groups) bytes, 4-byte aligned, CGS_EWORKSPACE if smaller; b < 1, groups < 1 or > 2^20, b * groups > 2^30,
 * T < 0, B < 0, capacity < 0: CGS_EINVAL before any launch (the query then returns 0 for a bad shape).
 * cgs_gather_rows: the copy behind eval[cnt:cnt + k] = batch[rows] (nsgan/GAN.py:362-368,413-419, synthetic/main.py:196-200).  src: [n][row]
 * fp32; dst[span[0] + k] = src[rows[k]] for k < min(span[1], listed_max), listed_max the number of ints rows holds; rows with
 * span[0] + k >= capacity are dropped (dst: at least capacity rows); a rows[k] outside [0, n) copies nothing for that k; a row may repeat.
 * 16-byte pieces where row % 4 == 0 and both bases are 16-byte aligned, 4-byte pieces otherwise.  n outside [0, 2^30], row outside
 * [1, 2^22], n * row > 2^40, listed_max outside [0, 2^30], capacity < 0: CGS_EINVAL before any launch. */
size_t cgs_mh_ws_bytes(int b, int groups);
int cgs_mh_walk(const float* sig, int b, int groups, const double* uniforms, int T, int B, const unsigned char* take_all, double* state, long long* fill,
                long long capacity, int* rows, int* counts, long long* span, void* ws, size_t ws_bytes, void* stream);
int cgs_gather_rows(const float* src, int n, int row, const int* rows, int listed_max, const long long* span, float* dst, long long capacity,
                    void* stream);

/* ---- nearest-neighbour queries between two pools of feature vectors, in double on the device (csrc/knn.hip) ----
 * qry: [m][d] fp32, ref: [n][d] fp32, 1 <= d <= 2048, 1 <= m, n <= 2^30.  Every entry point evaluates the squared distance in the
 * DIFFERENCE form, in double, k ascending, one fused multiply-add per coordinate:
 *     D2(j, i) = sum_k (double(q_jk) - double(r_ik))^2
 * so that equal rows give exactly 0, D2(j, i) and D2(i, j) are the same bits, and the error is relative: |D2^ - D2| <= (d + 3) 2^-53 D2.
 * The n x m matrix is never stored: a block owns 64 queries, walks its share of the 64-reference tiles and keeps the answer per query.
 * Where there are too few query tiles to fill the device the references are cut into `splits` runs of `tiles_per_split` tiles
 * (cgs_knn_plan; a function of (m, n) alone), each run leaves a partial answer in ws and a second launch merges them in ascending order.
 * The merges are order-free by construction (below), so the result does not depend on the split.  No atomics: a rerun is bit-equal.
 * cgs_nn_min: out_d2[j] = min_i D2(j, i), out_idx[j] = the LOWEST i that attains it.  exclude_self = 1 (needs n == m; ref is then the
 *     query pool itself or a pool of the same length) leaves i == j out of the minimum and stores D2(j, j) in out_d2[m + j]: out_d2 is
 *     then 2 m doubles.  No candidate (exclude_self with n == 1): out_d2[j] = +inf, out_idx[j] = -1.  The reference's pairwise_distance
 *     (sampling/utils_sampling.py:126-130: min over i of cdist + 10 I) is min(sqrt(out_d2[j]), sqrt(out_d2[m + j]) + 10) exactly,
 *     because sqrt is monotone and correctly rounded: the minimum of the roots is the root of the minimum.
 * cgs_knn_radii: out_r2[j] = the k-th smallest D2 from row j of x to the rows of `other` ([n_other][d]), or, other == NULL, to the rows
 *     of x itself -- without row j where exclude_self = 1 (exclude_self needs other == NULL).  1 <= k <= 8; the k-th smallest VALUE of
 *     a multiset does not depend on how ties are ordered.  Fewer than k candidates is CGS_EINVAL with a text, not an infinity.
 * cgs_ball_count: out_count[j] = #{ i : D2(j, i) <= ref_r2[i] }, ref_r2: n doubles on the device.
 * cgs_knn_ws_bytes(op, m, n, d, k): bytes of ws for op = CGS_KNN_NN_MIN / CGS_KNN_RADII / CGS_KNN_BALL_COUNT (k: of the radii only; m = rows
 *     of the query side, n = rows of the reference side), at least 8; 0 = the call would be refused.  ws 8-byte aligned, CGS_EWORKSPACE
 *     if smaller.  cgs_knn_plan: plan[4] = {query tiles, reference tiles, tiles_per_split, splits}; returns 0 where the shape is refused.
 * Errors (CGS_EINVAL before any launch and before any pointer is looked at): d, m, n out of range, exclude_self not 0 / 1 or with
 * n != m, k outside 1..8, fewer than k candidates.  Non-finite inputs give unspecified values, no fault. */
#define CGS_KNN_NN_MIN 0
#define CGS_KNN_RADII 1
#define CGS_KNN_BALL_COUNT 2
int cgs_knn_plan(int m, int n, int d, int* plan);
size_t cgs_knn_ws_bytes(int op, int m, int n, int d, int k);
int cgs_nn_min(const float* qry, int m, const float* ref, int n, int d, int exclude_self, double* out_d2, int* out_idx, void* ws,
               size_t ws_bytes, void* stream);
int cgs_knn_radii(const float* x, int n, int d, int k, int exclude_self, const float* other, int n_other, double* out_r2, void* ws,
                  size_t ws_bytes, void* stream);
int cgs_ball_count(const float* qry, int m, const float* ref, int n, int d, const double* ref_r2, int* out_count, void* ws, size_t ws_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGS_HIP_H */
