// extern "C" entry points of libcgs_hip.so (declared in include/cgs_hip.h): argument checking,
// geometry, weight packing and kernel dispatch.  No allocation, no synchronisation.
#include <stdarg.h>
#include <stdio.h>

#include "cgs_internal.h"

static thread_local char g_err[512] = "";
static thread_local const char* g_last_kernel = "";

static thread_local double g_last_flops = 0.0;
static thread_local int g_last_tail[2] = {0, 0};
void cgs_note_tail(int tiles, int split) { g_last_tail[0] = tiles; g_last_tail[1] = split; }
static thread_local int g_last_plan[5] = {0, 0, 0, 0, 0};
void cgs_note_igemm_plan(int xcd_map, int cls_flip, int uni, int gx, int splitk) {
    g_last_plan[0] = xcd_map; g_last_plan[1] = cls_flip; g_last_plan[2] = uni; g_last_plan[3] = gx; g_last_plan[4] = splitk;
}
static thread_local int g_contraction = CGS_CONTRACTION_F32;
int cgs_contraction_mode() { return g_contraction; }

void cgs_note_kernel(const char* name) { g_last_kernel = name; }
void cgs_note_flops(double f) { g_last_flops = f; }
void cgs_add_flops(double f) { g_last_flops += f; }      // per launch: a call that splits its batch (run_dir) sums its chunks

int cgs_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" {

int cgs_version(void) { return 117; }
const char* cgs_last_error(void) { return g_err; }
const char* cgs_last_kernel(void) { return g_last_kernel; }
double cgs_last_executed_flops(void) { return g_last_flops; }
int cgs_last_tail_tiles(void) { return g_last_tail[0]; }
int cgs_last_tail_split(void) { return g_last_tail[1]; }
void cgs_last_igemm_plan(int out[5]) {
    if (out) for (int i = 0; i < 5; ++i) out[i] = g_last_plan[i];
}
int cgs_set_contraction(int mode) {
    if (mode < CGS_CONTRACTION_F32 || mode > CGS_CONTRACTION_BX6_ALL) return cgs_set_error(CGS_EINVAL, "set_contraction: mode %d", mode);
    g_contraction = mode;
    return CGS_OK;
}
int cgs_get_contraction(void) { return g_contraction; }

}  // extern "C"

// One call of a conv / deconv op as the kernels see it: the layer relation and the direction it is contracted in.  The ONLY place that
// knows which tensor of an op is the big one (conv: its input side (H, W, Cin); deconv: its output side (Ho, Wo, Cout)) and which ops
// run small -> big (conv backward-data, deconv forward).  A conv's small side is derived; a deconv's big side is what the caller says
// (the entry points check it with check_layer; a planning query may take it on trust or pass a bound).
struct ConvCall { CgsLayer L; bool dirT, deconv, bwd; };

static ConvCall conv_call_of(int op, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw) {
    ConvCall c;
    c.deconv = (op == CGS_DECONV_FWD || op == CGS_DECONV_BWD_DATA);
    c.bwd = (op == CGS_CONV_BWD_DATA || op == CGS_DECONV_BWD_DATA);
    c.dirT = (op == CGS_CONV_BWD_DATA || op == CGS_DECONV_FWD);
    CgsLayer& L = c.L;
    L.kh = kh; L.kw = kw; L.sh = sh; L.sw = sw;
    // weights are [kh][kw][Cb][Cs]: conv Cb=Cin,Cs=Cout; deconv Cb=Cout,Cs=Cin
    if (!c.deconv) { L.Hb = H; L.Wb = W; L.Cb = Cin; L.Hs = cgs_ceil_div(H, sh > 0 ? sh : 1); L.Ws = cgs_ceil_div(W, sw > 0 ? sw : 1); L.Cs = Cout; }
    else { L.Hs = H; L.Ws = W; L.Cs = Cin; L.Hb = Ho; L.Wb = Wo; L.Cb = Cout; }
    return c;
}

static int check_layer(const CgsLayer& L, const char* who) {
    if (L.kh <= 0 || L.kw <= 0 || L.sh <= 0 || L.sw <= 0 || L.Hb <= 0 || L.Wb <= 0 || L.Cb <= 0 || L.Cs <= 0)
        return cgs_set_error(CGS_EINVAL, "%s: non-positive dimension", who);
    if (L.Hs != cgs_ceil_div(L.Hb, L.sh) || L.Ws != cgs_ceil_div(L.Wb, L.sw))
        return cgs_set_error(CGS_EINVAL, "%s: 'SAME' geometry mismatch: big %dx%d stride %dx%d needs small %dx%d, got %dx%d", who,
                             L.Hb, L.Wb, L.sh, L.sw, cgs_ceil_div(L.Hb, L.sh), cgs_ceil_div(L.Wb, L.sw), L.Hs, L.Ws);
    return CGS_OK;
}

// The implicit-GEMM geometry of a call: every member determinate (pointers null, planner fields 0, the ns_* defaults), so it can be
// handed to the planners of igemm.hip as it is; run_dir adds its pointers.  A transposed launch has sh * sw <= CGS_MAX_CLASSES parity
// classes: for larger strides (which run_dir refuses and no planner is asked about) the geometry fields stay 0.
static IgemmParams igemm_geometry(const CgsLayer& L, bool dirT, int B, int epilogue) {
    IgemmParams p{};
    p.B = B; p.epilogue = epilogue;
    if (!dirT) cgs_geom_F(L, p);
    else if (L.sh <= 2 && L.sw <= 2) cgs_geom_T(L, p);
    return p;
}

// one launch addresses its tensors with 32-bit byte offsets: a call splits its batch so each launch stays < 2 GiB
static size_t in_image_floats(const IgemmParams& p) { return (size_t)p.Hin * p.Win * p.Cred; }
static size_t out_image_floats(const IgemmParams& p) { return (size_t)p.Hout * p.Wout * p.N; }
static size_t images_per_launch(const IgemmParams& p) {
    const size_t in_img = in_image_floats(p) * 4, out_img = out_image_floats(p) * 4;
    return 0x7fffffffUL / (in_img > out_img ? in_img : out_img);
}
static bool whole_batch_in_one_launch(const IgemmParams& p) { return images_per_launch(p) >= (size_t)p.B; }

static bool smalln_ok(const CgsLayer& L, int epilogue) {
    return L.Cb <= 4 && L.sh == 2 && L.sw == 2 && L.Hb == 2 * L.Hs && L.Wb == 2 * L.Ws && (L.Cs % 4) == 0 &&
           epilogue != CGS_EPI_AFFINE_RELU;
}

// Which kernel family (and therefore which packed-weight layout in the workspace) serves a call.  ONE decision function:
// run_dir() dispatches on it and cgs_conv_family() reports it, so a caller that caches packed workspaces can key them by
// the family and never hand one family's packed image to another (the epilogue and the pointer alignment take
// part in the choice, not only the geometry).  g = igemm_geometry() of the call (its batch size and epilogue are the call's).
static int choose_family(const CgsLayer& L, bool dirT, const IgemmParams& g, bool have_ws, size_t ws_bytes, bool in_al, bool ws_al,
                         bool rest_al) {
    const int B = g.B, epilogue = g.epilogue;
    if (dirT && smalln_ok(L, epilogue)) {
        if ((L.Cs % 16) == 0 && have_ws && cgs_convt_quad_fits(L)) return CGS_FAMILY_QUAD;
        if (epilogue < CGS_EPI_RELU_BWD_AFFINE) return CGS_FAMILY_SMALLN_T;             // VALU form (any Cs % 4 == 0), packs nothing
    }
    if (!dirT && cgs_conv_smalln_f_ok(L, B, epilogue) && have_ws && ws_bytes >= cgs_conv_smalln_f_ws_floats(L) * sizeof(float) &&
        in_al && ws_al)
        return CGS_FAMILY_SMALLN_F;
    if (!dirT && cgs_conv_taps_ok(L, epilogue)) return CGS_FAMILY_TAPS;                     // K = 16 taps: no packed weights, no alignment needs
    if (!dirT && cgs_conv_dot_ok(L, epilogue) && in_al) return CGS_FAMILY_DOT;             // (after the stride-1 VALU head kernel, which serves the large grids)
    const bool patch_f = !dirT && cgs_conv_patch_ok(L, epilogue), patch_t = dirT && cgs_conv_patch_T_ok(L);
    if ((patch_f || patch_t) && have_ws && ws_bytes >= cgs_conv_patch_ws_floats(L, dirT) * sizeof(float) && ws_al && rest_al)
        return CGS_FAMILY_PATCH;
    // the calling thread opted into the split-bf16 contraction (cgs_set_contraction): the calls it serves leave the fp32 kernel
    // (... if the workspace can hold its three bf16 weight planes, 6 bytes per weight: an undersized one keeps the fp32 kernel, whose
    // packed image it was sized for, instead of failing with EWORKSPACE -- the patch family above falls back the same way)
    if (g_contraction != CGS_CONTRACTION_F32 && cgs_igemm_bx6_ok(L, dirT, B, g_contraction == CGS_CONTRACTION_BX6_ALL)) {
        if (have_ws && ws_bytes >= cgs_igemm_bx6_packed_bytes(g)) return CGS_FAMILY_IGEMM_BX6;
    }
    return CGS_FAMILY_IGEMM;
}

// ... as the planning queries ask: a workspace of ws_bytes, every pointer aligned
static int planned_family(const ConvCall& c, const IgemmParams& g, size_t ws_bytes) { return choose_family(c.L, c.dirT, g, ws_bytes > 0, ws_bytes, true, true, true); }

// norm-backward statistics of a backward-data call (IgemmParams::ns_*; x rides in ep_aux)
struct NsArgs { const float *mean, *invstd, *gamma, *beta; float leak; int group_images; };

// What an entry point passes beside the plain conv arguments.  FORM_STATS (*_fwd_stats): the launch leaves the column sums of its output
// as partial rows in stat_part; FORM_NSTATS (*_bwd_data_nstats): the norm backward's two column sums, from ns and x_norm (in ep_aux);
// FORM_SIGNS (*_signs): a forward leaves the sign mask of its output in sign_out, a backward-data takes aux_signs for the fp32 ep_aux;
// FORM_UPDATE (*_bwd_data_update): the result is not stored -- the momentum step of the refinement loop is applied to ``out`` (the feature) and up_mom.
enum ConvForm { FORM_PLAIN = CGS_FORM_PLAIN, FORM_STATS = CGS_FORM_STATS, FORM_NSTATS = CGS_FORM_NSTATS, FORM_SIGNS = CGS_FORM_SIGNS, FORM_UPDATE = CGS_FORM_UPDATE };
struct ConvExtras {
    ConvForm form = FORM_PLAIN;
    float* stat_part = nullptr; size_t stat_part_bytes = 0;
    NsArgs ns = {};
    unsigned* sign_out = nullptr; const unsigned* aux_signs = nullptr;
    float* up_mom = nullptr; float up_rate = 0.f, up_alpha = 0.f; int up_first = 0;
};

static int run_dir(const ConvCall& c, int B, const float* in, const float* w, const float* bias, float* out, int epilogue,
                   const float* ep_a, const float* ep_b, const float* ep_aux, void* ws, size_t ws_bytes, int prepacked, hipStream_t s,
                   const char* who, const ConvExtras& x) {
    const CgsLayer& L = c.L;
    const bool dirT = c.dirT, nstats = x.form == FORM_NSTATS;
    cgs_note_flops(0.0);
    cgs_note_tail(0, 0);
    cgs_note_igemm_plan(0, 0, 0, 0, 0);
    if (B <= 0) return cgs_set_error(CGS_EINVAL, "%s: B=%d", who, B);
    if (!in || !w || !out) return cgs_set_error(CGS_EINVAL, "%s: null tensor", who);
    if (epilogue < CGS_EPI_NONE || epilogue > CGS_EPI_TANH_BWD) return cgs_set_error(CGS_EINVAL, "%s: epilogue %d", who, epilogue);
    if (epilogue == CGS_EPI_AFFINE_RELU && (!ep_a || !ep_b)) return cgs_set_error(CGS_EINVAL, "%s: affine epilogue needs a,b", who);
    if (epilogue >= CGS_EPI_RELU_BWD_AFFINE && ((!ep_aux && !x.aux_signs) || (epilogue == CGS_EPI_RELU_BWD_AFFINE && !ep_a)))
        return cgs_set_error(CGS_EINVAL, "%s: backward epilogue %d needs aux%s", who, epilogue, epilogue == CGS_EPI_RELU_BWD_AFFINE ? " and a" : "");
    if (dirT && (L.sh > 2 || L.sw > 2)) return cgs_set_error(CGS_EINVAL, "%s: transposed direction supports stride <= 2", who);
    const bool rest_al = !(((uintptr_t)out & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)ep_a & 15) || ((uintptr_t)ep_b & 15) ||
                           ((uintptr_t)ep_aux & 15));
    IgemmParams p = igemm_geometry(L, dirT, B, epilogue);
    const int fam = choose_family(L, dirT, p, ws != nullptr, ws_bytes, !((uintptr_t)in & 15), !((uintptr_t)ws & 15), rest_al);
    if (x.stat_part && fam != CGS_FAMILY_IGEMM && fam != CGS_FAMILY_IGEMM_BX6) return cgs_set_error(CGS_EINVAL, "%s: fused statistics are an implicit-GEMM feature (see cgs_conv_stat_partials)", who);
    if (nstats && (!x.stat_part || fam != CGS_FAMILY_IGEMM)) return cgs_set_error(CGS_EINVAL, "%s: norm-backward statistics are a feature of the exact-fp32 implicit GEMM (see cgs_conv_stat_layout)", who);
    if (x.form == FORM_UPDATE && (!x.up_mom || fam != CGS_FAMILY_IGEMM)) return cgs_set_error(CGS_EINVAL, "%s: the fused update is a feature of the exact-fp32 implicit GEMM (see cgs_conv_update_form)", who);
    if (x.sign_out && fam != CGS_FAMILY_IGEMM && fam != CGS_FAMILY_IGEMM_BX6) return cgs_set_error(CGS_EINVAL, "%s: this call cannot leave a sign mask (see cgs_conv_signs_ok)", who);
    if (x.aux_signs && fam != CGS_FAMILY_PATCH && fam != CGS_FAMILY_TAPS) return cgs_set_error(CGS_EINVAL, "%s: this call cannot take a sign mask (see cgs_conv_signs_ok)", who);
    if (((uintptr_t)x.sign_out & 3) || ((uintptr_t)x.aux_signs & 3)) return cgs_set_error(CGS_EINVAL, "%s: sign mask must be 4-byte aligned", who);
    switch (fam) {
        case CGS_FAMILY_QUAD:
            return cgs_convt_quad_launch(L, B, in, w, bias, out, epilogue, ep_a, ep_aux, (float*)ws, ws_bytes, prepacked, s);
        case CGS_FAMILY_SMALLN_T:
            return cgs_convt_smalln_launch(L, B, in, w, bias, out, epilogue, s);
        case CGS_FAMILY_SMALLN_F:
            return cgs_conv_smalln_f_launch(L, B, in, w, bias, out, epilogue, (float*)ws, ws_bytes, prepacked, s);
        case CGS_FAMILY_DOT:
            return cgs_conv_dot_launch(L, B, in, w, bias, out, epilogue, ep_a, ep_b, s);
        case CGS_FAMILY_TAPS:
            return cgs_conv_taps_launch(L, B, in, w, bias, out, epilogue, ep_a, ep_b, ep_aux, x.aux_signs, s);
        case CGS_FAMILY_PATCH:
            return cgs_conv_patch_launch(L, dirT, B, in, w, bias, out, epilogue, ep_a, ep_b, ep_aux, (float*)ws, ws_bytes, prepacked, s, x.aux_signs);
        default: break;
    }
    p.in = in; p.bias = bias; p.ep_a = ep_a; p.ep_b = ep_b; p.ep_aux = ep_aux; p.out = out;
    p.stat_part = x.stat_part;
    if (nstats) { p.ns_mean = x.ns.mean; p.ns_inv = x.ns.invstd; p.ns_gamma = x.ns.gamma; p.ns_beta = x.ns.beta; p.ns_leak = x.ns.leak; p.ns_gimg = x.ns.group_images >= B ? 0 : x.ns.group_images; }
    if (x.form == FORM_UPDATE) { p.up_mom = x.up_mom; p.up_rate = x.up_rate; p.up_alpha = x.up_alpha; p.up_first = x.up_first; }
    p.sign_out = x.sign_out;
    p.sign_plane = (long)B * (dirT ? L.Hb * L.Wb : L.Hs * L.Ws);
    const bool bx6 = fam == CGS_FAMILY_IGEMM_BX6;
    const size_t need = bx6 ? cgs_igemm_bx6_packed_bytes(p) : cgs_packed_floats(p) * sizeof(float);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    if (((uintptr_t)ws & 15) || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)bias & 15) ||
        ((uintptr_t)ep_a & 15) || ((uintptr_t)ep_b & 15) || ((uintptr_t)ep_aux & 15))
        return cgs_set_error(CGS_EINVAL, "%s: pointers must be 16-byte aligned", who);
    p.wp = (const float*)ws;
    if (!prepacked) {
        int rc = bx6 ? cgs_pack_weights_bx6(p, L, dirT, w, ws, s) : cgs_pack_weights(p, L, dirT, w, (float*)ws, s);
        if (rc) return rc;
    }
    const size_t chunk = images_per_launch(p), in_img = in_image_floats(p), out_img = out_image_floats(p);
    if (chunk < 1) return cgs_set_error(CGS_EINVAL, "%s: one image exceeds 2 GiB", who);
    if (x.stat_part && !whole_batch_in_one_launch(p)) return cgs_set_error(CGS_EINVAL, "%s: fused statistics need the batch in one launch", who);
    if (p.up_mom && !whole_batch_in_one_launch(p)) return cgs_set_error(CGS_EINVAL, "%s: the fused update needs the batch in one launch", who);
    for (size_t b0 = 0; b0 < (size_t)B; b0 += chunk) {
        p.B = (int)(B - b0 < chunk ? B - b0 : chunk);
        p.in = in + b0 * in_img;
        p.out = out + b0 * out_img;
        p.ep_aux = ep_aux ? ep_aux + b0 * out_img : nullptr;
        p.sign_out = x.sign_out ? x.sign_out + b0 * p.Hout * p.Wout : nullptr;      // (plane-major: the chunk's pixels inside every plane)
        int rc = bx6 ? cgs_igemm_bx6_launch(p, s) : cgs_igemm_launch(p, (char*)ws + need, ws_bytes - need, s);
        if (rc) return rc;
    }
    return CGS_OK;
}

// cgs_conv_family's answer (< 0: bad argument) with, for cgs_conv_signs_ok, the call and the geometry it was decided on
struct ConvPlan { int fam; ConvCall c; IgemmParams g; };

static ConvPlan conv_plan_of(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue,
                             size_t ws_bytes) {
    ConvPlan q{};
    if (op < CGS_CONV_FWD || op > CGS_DECONV_BWD_DATA || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 ||
        sh <= 0 || sw <= 0) {
        q.fam = cgs_set_error(CGS_EINVAL, "conv_family: bad argument");
    } else {
        q.c = conv_call_of(op, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw);
        q.g = igemm_geometry(q.c.L, q.c.dirT, B, epilogue);
        q.fam = planned_family(q.c, q.g, ws_bytes);
    }
    return q;
}

// The norm-backward arguments of a *_bwd_data_nstats call: the backward-data of a conv / deconv whose result is the gradient w.r.t. the
// OUTPUT of a norm (+ lrelu) over x_norm (same shape as the result): the launch also leaves the norm backward's two column sums as
// partial rows (cgs_conv_stat_layout with the *_BWD_DATA op says where a group's rows lie; cgs_norm_lrelu_bwd_from_partials consumes
// them).  The result itself is the plain backward-data (no epilogue).
static int nstats_check(const char* who, const float* x_norm, const NsArgs& ns, const float* stat_part) {
    if (!x_norm || !ns.mean || !ns.invstd || !ns.gamma || !ns.beta) return cgs_set_error(CGS_EINVAL, "%s: null statistics argument", who);
    if (((uintptr_t)x_norm | (uintptr_t)ns.mean | (uintptr_t)ns.invstd | (uintptr_t)ns.gamma | (uintptr_t)ns.beta | (uintptr_t)stat_part) & 15)
        return cgs_set_error(CGS_EINVAL, "%s: pointers must be 16-byte aligned", who);
    return CGS_OK;
}

// The body of every conv / deconv / linear entry point: resolve the op, check what the form adds, dispatch.
static int conv_entry(const char* who, int op, const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cin,
                      int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue, const float* ep_a, const float* ep_b,
                      const float* ep_aux, void* ws, size_t ws_bytes, int prepacked, void* stream, const ConvExtras& x = ConvExtras()) {
    const ConvCall c = conv_call_of(op, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw);
    if (x.form == FORM_SIGNS) {
        if (!x.sign_out && !x.aux_signs) return cgs_set_error(CGS_EINVAL, "%s: null sign mask", who);
        if (!cgs_conv_signs_ok(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ws_bytes))
            return cgs_set_error(CGS_EINVAL, "%s: not available for this call (cgs_conv_signs_ok == 0)", who);
    }
    if (x.form == FORM_PLAIN && c.bwd && epilogue != CGS_EPI_NONE && epilogue < CGS_EPI_RELU_BWD_AFFINE)
        return cgs_set_error(CGS_EINVAL, "%s: epilogue %d", who, epilogue);
    int rc = check_layer(c.L, who);
    if (rc) return rc;
    if (x.form == FORM_STATS || x.form == FORM_NSTATS) {
        const bool conv_fwd = x.form == FORM_STATS && !c.deconv;          // (has a query of its own; the other three ask for the layout)
        int a, b, d;
        const int G = conv_fwd ? cgs_conv_stat_partials(B, H, W, Cin, Cout, kh, kw, sh, sw, ws_bytes)
                               : cgs_conv_stat_layout(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, x.form == FORM_NSTATS ? x.ns.group_images : B,
                                                      ws_bytes, &a, &b, &d);
        if (G == 0) return cgs_set_error(CGS_EINVAL, "%s: not available for this call (%s == 0)", who, conv_fwd ? "cgs_conv_stat_partials" : "cgs_conv_stat_layout");
        if (x.form == FORM_NSTATS && (rc = nstats_check(who, ep_aux, x.ns, x.stat_part))) return rc;
        const size_t need = (size_t)G * 2 * (c.bwd ? Cin : Cout) * sizeof(float);        // [rows][2][channels of the tensor the launch writes]
        if (!x.stat_part || x.stat_part_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "%s: partials buffer %zu < %zu bytes", who, x.stat_part_bytes, need);
        if ((uintptr_t)x.stat_part & 15) return cgs_set_error(CGS_EINVAL, "%s: partials buffer must be 16-byte aligned", who);
    }
    if (x.form == FORM_UPDATE) {          // (asked BEFORE anything is launched: a refused call leaves the feature and the momentum buffer untouched)
        if (!cgs_conv_update_form(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, ws_bytes, nullptr))
            return cgs_set_error(CGS_EINVAL, "%s: not available for this call (cgs_conv_update_form == 0)", who);
        if (!out || !x.up_mom || (((uintptr_t)out | (uintptr_t)x.up_mom) & 15)) return cgs_set_error(CGS_EINVAL, "%s: theta and m must be 16-byte aligned tensors", who);
    }
    return run_dir(c, B, in, w, bias, out, epilogue, ep_a, ep_b, ep_aux, ws, ws_bytes, prepacked, (hipStream_t)stream, who, x);
}

extern "C" {

size_t cgs_conv_ws_bytes(int op, int kh, int kw, int sh, int sw, int Cin, int Cout) {
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || Cin <= 0 || Cout <= 0) return 0;
    const ConvCall c = conv_call_of(op, 0, 0, Cin, 0, 0, Cout, kh, kw, sh, sw);       // (independent of the spatial size)
    const int Cb = c.L.Cb, Cs = c.L.Cs;
    const bool dirT = c.dirT;
    // (the split-bf16 form keeps three bf16 planes = 6 bytes per weight: sized for it wherever its geometry applies, whatever the
    // calling thread's contraction mode, so a workspace serves both)
    const int Cred = dirT ? Cs : Cb, Nn = dirT ? Cb : Cs;
    const size_t per_w = ((Cred % 32) == 0 && (Nn % 64) == 0 && kh <= 16 && kw <= 16) ? 6 : sizeof(float);
    if (!dirT) return (size_t)cgs_round_up(kh * kw * Cb, CGS_BK) * cgs_round_up(Cs, 64) * per_w;
    // T: per parity class, taps of that class (independent of the spatial size: pads only permute classes)
    size_t n = 0;
    for (int a = 0; a < sh; ++a)
        for (int b = 0; b < sw; ++b) {
            const int nty = a < kh ? (kh - a + sh - 1) / sh : 0, ntx = b < kw ? (kw - b + sw - 1) / sw : 0;
            n += (size_t)cgs_round_up(nty * ntx * Cs, CGS_BK) * cgs_round_up(Cb, 64);
        }
    if (Cb <= 4 && sh == 2 && sw == 2) {      // quad-form small-N kernel keeps its own packed copy
        const size_t q = cgs_convt_quad_ws_floats_bound(kh, kw, Cs);
        if (q > n) n = q;
    }
    return n * (per_w > sizeof(float) && !(Cb <= 4 && sh == 2 && sw == 2) ? per_w : sizeof(float));
}

size_t cgs_conv_ws_bytes_for(int op, int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw) {
    const size_t packed = cgs_conv_ws_bytes(op, kh, kw, sh, sw, Cin, Cout);
    if (B <= 0 || H <= 0 || W <= 0 || packed == 0) return packed;
    // H, W are the op's INPUT spatial size for conv fwd / deconv fwd and for their backward-datas the size of
    // the tensor the gradient is taken w.r.t. (the arguments of the entry points); a deconv's output is bounded by stride * input
    const ConvCall c = conv_call_of(op, H, W, Cin, H * sh, W * sw, Cout, kh, kw, sh, sw);
    if (c.dirT && (sh > 2 || sw > 2)) return packed;
    return packed + cgs_igemm_slab_bytes(igemm_geometry(c.L, c.dirT, B, CGS_EPI_NONE));
}

int cgs_conv_family(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue,
                    size_t ws_bytes) {
    return conv_plan_of(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ws_bytes).fam;
}

int cgs_conv_stat_partials(int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, size_t ws_bytes) {
    const ConvCall c = conv_call_of(CGS_CONV_FWD, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw);
    if (check_layer(c.L, "conv_stat_partials")) return 0;
    const IgemmParams g = igemm_geometry(c.L, c.dirT, B, CGS_EPI_NONE);
    const int fam = planned_family(c, g, ws_bytes);
    if (B <= 0 || (Cout & 3) || (fam != CGS_FAMILY_IGEMM && fam != CGS_FAMILY_IGEMM_BX6)) return 0;       // (both leave the same partial rows)
    if (!whole_batch_in_one_launch(g)) return 0;                     // the entry point would split the batch
    const long M = (long)B * c.L.Hs * c.L.Ws;
    return (int)(2 * ((M + 127) / 128));                             // one partial row per (128-row tile, wave row)
}

// Where the partial rows of one GROUP of group_images consecutive images lie in the [rows][2][Cout] buffer a *_fwd_stats call fills
// (one row per 64 GEMM rows; the parity classes of a transposed convolution back to back): group g owns, for every segment
// s < nseg, the rows_per_seg rows from s * seg_stride + g * rows_per_seg.  Image-major launches: a segment per parity class;
// pixel-major launches (whole 128-image tiles): a segment per (class, base pixel).  Returns the total row count, 0 = unavailable.
int cgs_conv_stat_layout(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int group_images,
                         size_t ws_bytes, int* rows_per_seg, int* nseg, int* seg_stride) {
    if (op < CGS_CONV_FWD || op > CGS_DECONV_BWD_DATA || B <= 0 || group_images <= 0 || (B % group_images) || !rows_per_seg || !nseg || !seg_stride)
        return 0;
    const ConvCall c = conv_call_of(op, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw);
    // the channel count of the tensor the launch WRITES (the statistics' columns): the forward ops write Cout channels, the backward-data
    // ops (norm-backward statistics, cgs_*_bwd_data_nstats) the gradient w.r.t. their input: Cin channels
    if ((c.bwd ? Cin : Cout) & 3) return 0;
    if (check_layer(c.L, "conv_stat_layout")) return 0;
    if (c.dirT && (sh > 2 || sw > 2)) return 0;
    const IgemmParams p = igemm_geometry(c.L, c.dirT, B, CGS_EPI_NONE);
    const int fam = planned_family(c, p, ws_bytes);
    if (fam != CGS_FAMILY_IGEMM && (c.bwd || fam != CGS_FAMILY_IGEMM_BX6)) return 0;         // (the backward sums: the exact-fp32 kernel only)
    if (!whole_batch_in_one_launch(p)) return 0;                     // the entry point would split the batch
    const int RC = p.cls[0].R * p.cls[0].C;
    for (int i = 1; i < p.nclasses; ++i)
        if (p.cls[i].R * p.cls[i].C != RC) return 0;                 // (odd output sizes: parity classes of different size)
    if (RC <= 0) return 0;
    const long M = (long)B * RC;
    const long cls_rows = 2 * ((M + 127) / 128);
    if (cls_rows * p.nclasses > 0x7fffffffL) return 0;
    if (group_images == B) {                                         // one group: every partial row belongs to it, whatever the row order
        *rows_per_seg = (int)(cls_rows * p.nclasses); *nseg = 1; *seg_stride = 0;
        return (int)(cls_rows * p.nclasses);
    }
    const int order = cgs_igemm_row_order(p);
    if (order == 0) {                                                // rows (image, pixel): a group's rows are contiguous inside every class
        if (((long)group_images * RC) % 64) return 0;
        *rows_per_seg = (int)((long)group_images * RC / 64); *nseg = p.nclasses; *seg_stride = (int)cls_rows;
    } else if (order == 2) {                                         // rows (pixel, image), B % 128 == 0: 64 consecutive images of one pixel per row
        if (group_images % 64) return 0;
        *rows_per_seg = group_images / 64; *nseg = p.nclasses * RC; *seg_stride = B / 64;
    } else {
        return 0;
    }
    return (int)(cls_rows * p.nclasses);
}

// ---- the fused momentum update (cgs_hip.h, cgs_*_bwd_data_update): where the call would apply it, 0 = not offered ----
int cgs_conv_update_form(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, size_t ws_bytes,
                         int* row_order) {
    if (row_order) *row_order = 0;
    if (op != CGS_CONV_BWD_DATA && op != CGS_DECONV_BWD_DATA) return 0;
    const ConvPlan q = conv_plan_of(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, CGS_EPI_NONE, ws_bytes);
    if (q.fam != CGS_FAMILY_IGEMM || check_layer(q.c.L, "conv_update_form")) return 0;
    if (q.c.dirT && (sh > 2 || sw > 2)) return 0;
    if (!whole_batch_in_one_launch(q.g)) return 0;                  // the entry point would split the batch
    const size_t packed = cgs_packed_floats(q.g) * sizeof(float);
    if (ws_bytes < packed) return 0;
    if (row_order) *row_order = cgs_igemm_row_order(q.g);
    return cgs_igemm_update_form(q.g, ws_bytes - packed);
}

// ---- the launch plan of a call before it is launched (cgs_hip.h; host only) ----
int cgs_conv_igemm_plan(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue, int form,
                        size_t ws_bytes, cgs_igemm_plan_info* info, unsigned char* perm) {
    if (!info || form < CGS_FORM_PLAIN || form > CGS_FORM_UPDATE || epilogue < CGS_EPI_NONE || epilogue > CGS_EPI_TANH_BWD) return 0;
    const ConvPlan q = conv_plan_of(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ws_bytes);
    if (q.fam != CGS_FAMILY_IGEMM || check_layer(q.c.L, "conv_igemm_plan")) return 0;
    if (q.c.dirT && (sh > 2 || sw > 2)) return 0;
    // (the forms are the entry points': statistics and sign masks of a forward, norm-backward statistics and the update of a backward-data)
    if (q.c.bwd != (form == CGS_FORM_NSTATS || form == CGS_FORM_UPDATE) && form != CGS_FORM_PLAIN) return 0;
    if (!whole_batch_in_one_launch(q.g)) return 0;                  // the entry point would split the batch
    const size_t packed = cgs_packed_floats(q.g) * sizeof(float);
    if (ws_bytes < packed) return 0;
    return cgs_igemm_plan_info_of(q.g, form, ws_bytes - packed, info, perm);
}

// ---- sign masks (cgs_hip.h): the activation gradient of relu / lrelu needs one bit per element of the saved activation ----
int cgs_conv_signs_ok(int op, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue,
                      size_t ws_bytes) {
    const ConvPlan q = conv_plan_of(op, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ws_bytes);
    const int fam = q.fam;
    if (fam < 0) return 0;
    if (epilogue >= CGS_EPI_RELU_BWD_AFFINE)          // consumer: a backward-data whose epilogue applies relu' / lrelu'
        return (fam == CGS_FAMILY_PATCH && cgs_conv_patch_signs_ok(q.c.L, q.c.dirT, epilogue)) || (fam == CGS_FAMILY_TAPS && cgs_conv_taps_signs_ok(q.c.L, epilogue));
    if (fam == CGS_FAMILY_IGEMM_BX6)            // producer on the split-bf16 kernel: whole 64-column wave tiles, never split over K
        return (epilogue == CGS_EPI_AFFINE_RELU || epilogue == CGS_EPI_LRELU) && whole_batch_in_one_launch(q.g);
    if (fam != CGS_FAMILY_IGEMM || (q.c.dirT && (sh > 2 || sw > 2))) return 0;    // producer: a forward with the relu / lrelu epilogue
    if (!whole_batch_in_one_launch(q.g)) return 0;                                // (a split batch may fall under the split-K threshold)
    return cgs_igemm_signs_ok(q.g);
}

int cgs_conv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                        int Cout, int kh, int kw, int sh, int sw, int epilogue, const float* ep_a, const float* ep_b,
                        void* ws, size_t ws_bytes, int ws_prepacked, void* stream) {
    return conv_entry("conv2d_nhwc_fwd", CGS_CONV_FWD, x, w, bias, y, B, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw, epilogue, ep_a, ep_b, nullptr, ws, ws_bytes,
                      ws_prepacked, stream);
}

int cgs_conv2d_nhwc_bwd_data(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout, int kh,
                             int kw, int sh, int sw, int epilogue, const float* ep_a, const float* ep_aux, void* ws,
                             size_t ws_bytes, int ws_prepacked, void* stream) {
    return conv_entry("conv2d_nhwc_bwd_data", CGS_CONV_BWD_DATA, dy, w, nullptr, dx, B, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw, epilogue, ep_a, nullptr, ep_aux, ws,
                      ws_bytes, ws_prepacked, stream);
}

int cgs_deconv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                          int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue, const float* ep_a,
                          const float* ep_b, void* ws, size_t ws_bytes, int ws_prepacked, void* stream) {
    return conv_entry("deconv2d_nhwc_fwd", CGS_DECONV_FWD, x, w, bias, y, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ep_a, ep_b, nullptr, ws, ws_bytes,
                      ws_prepacked, stream);
}

int cgs_deconv2d_nhwc_bwd_data(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Ho, int Wo,
                               int Cout, int kh, int kw, int sh, int sw, int epilogue, const float* ep_a,
                               const float* ep_aux, void* ws, size_t ws_bytes, int ws_prepacked, void* stream) {
    return conv_entry("deconv2d_nhwc_bwd_data", CGS_DECONV_BWD_DATA, dy, w, nullptr, dx, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ep_a, nullptr, ep_aux,
                      ws, ws_bytes, ws_prepacked, stream);
}

int cgs_conv2d_nhwc_fwd_stats(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                              int Cout, int kh, int kw, int sh, int sw, void* ws, size_t ws_bytes, int ws_prepacked,
                              float* stat_part, size_t stat_part_bytes, void* stream) {
    return conv_entry("conv2d_nhwc_fwd_stats", CGS_CONV_FWD, x, w, bias, y, B, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw, CGS_EPI_NONE, nullptr, nullptr, nullptr, ws,
                      ws_bytes, ws_prepacked, stream, ConvExtras{FORM_STATS, stat_part, stat_part_bytes});
}

int cgs_deconv2d_nhwc_fwd_stats(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Ho, int Wo,
                                int Cout, int kh, int kw, int sh, int sw, void* ws, size_t ws_bytes, int ws_prepacked, float* stat_part,
                                size_t stat_part_bytes, void* stream) {
    return conv_entry("deconv2d_nhwc_fwd_stats", CGS_DECONV_FWD, x, w, bias, y, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, CGS_EPI_NONE, nullptr, nullptr, nullptr,
                      ws, ws_bytes, ws_prepacked, stream, ConvExtras{FORM_STATS, stat_part, stat_part_bytes});
}

int cgs_conv2d_nhwc_bwd_data_nstats(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout, int kh, int kw, int sh,
                                    int sw, const float* x_norm, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                    float leak, int group_images, void* ws, size_t ws_bytes, int ws_prepacked, float* stat_part,
                                    size_t stat_part_bytes, void* stream) {
    return conv_entry("conv2d_nhwc_bwd_data_nstats", CGS_CONV_BWD_DATA, dy, w, nullptr, dx, B, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw, CGS_EPI_NONE, nullptr, nullptr,
                      x_norm, ws, ws_bytes, ws_prepacked, stream, ConvExtras{FORM_NSTATS, stat_part, stat_part_bytes, NsArgs{mean, invstd, gamma, beta, leak,
                      group_images}});
}

int cgs_deconv2d_nhwc_bwd_data_nstats(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh,
                                      int kw, int sh, int sw, const float* x_norm, const float* mean, const float* invstd, const float* gamma,
                                      const float* beta, float leak, int group_images, void* ws, size_t ws_bytes, int ws_prepacked,
                                      float* stat_part, size_t stat_part_bytes, void* stream) {
    return conv_entry("deconv2d_nhwc_bwd_data_nstats", CGS_DECONV_BWD_DATA, dy, w, nullptr, dx, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, CGS_EPI_NONE, nullptr,
                      nullptr, x_norm, ws, ws_bytes, ws_prepacked, stream, ConvExtras{FORM_NSTATS, stat_part, stat_part_bytes, NsArgs{mean, invstd, gamma, beta,
                      leak, group_images}});
}

int cgs_conv2d_nhwc_bwd_data_update(const float* dy, const float* w, float* theta, float* m, int B, int H, int W, int Cin, int Cout, int kh,
                                    int kw, int sh, int sw, float rate, float alpha, int first, void* ws, size_t ws_bytes, int ws_prepacked,
                                    void* stream) {
    ConvExtras x;
    x.form = FORM_UPDATE; x.up_mom = m; x.up_rate = rate; x.up_alpha = alpha; x.up_first = first ? 1 : 0;
    return conv_entry("conv2d_nhwc_bwd_data_update", CGS_CONV_BWD_DATA, dy, w, nullptr, theta, B, H, W, Cin, 0, 0, Cout, kh, kw, sh, sw, CGS_EPI_NONE, nullptr,
                      nullptr, nullptr, ws, ws_bytes, ws_prepacked, stream, x);
}

int cgs_deconv2d_nhwc_bwd_data_update(const float* dy, const float* w, float* theta, float* m, int B, int H, int W, int Cin, int Ho, int Wo,
                                      int Cout, int kh, int kw, int sh, int sw, float rate, float alpha, int first, void* ws, size_t ws_bytes,
                                      int ws_prepacked, void* stream) {
    ConvExtras x;
    x.form = FORM_UPDATE; x.up_mom = m; x.up_rate = rate; x.up_alpha = alpha; x.up_first = first ? 1 : 0;
    return conv_entry("deconv2d_nhwc_bwd_data_update", CGS_DECONV_BWD_DATA, dy, w, nullptr, theta, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, CGS_EPI_NONE,
                      nullptr, nullptr, nullptr, ws, ws_bytes, ws_prepacked, stream, x);
}

int cgs_deconv2d_nhwc_fwd_signs(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                                int Ho, int Wo, int Cout, int kh, int kw, int sh, int sw, int epilogue, const float* ep_a,
                                const float* ep_b, unsigned* signs, void* ws, size_t ws_bytes, int ws_prepacked, void* stream) {
    return conv_entry("deconv2d_nhwc_fwd_signs", CGS_DECONV_FWD, x, w, bias, y, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ep_a, ep_b, nullptr, ws,
                      ws_bytes, ws_prepacked, stream, ConvExtras{FORM_SIGNS, nullptr, 0, NsArgs{}, signs, nullptr});
}

int cgs_deconv2d_nhwc_bwd_data_signs(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Ho, int Wo,
                                     int Cout, int kh, int kw, int sh, int sw, int epilogue, const float* ep_a,
                                     const unsigned* aux_signs, void* ws, size_t ws_bytes, int ws_prepacked, void* stream) {
    return conv_entry("deconv2d_nhwc_bwd_data_signs", CGS_DECONV_BWD_DATA, dy, w, nullptr, dx, B, H, W, Cin, Ho, Wo, Cout, kh, kw, sh, sw, epilogue, ep_a, nullptr,
                      nullptr, ws, ws_bytes, ws_prepacked, stream, ConvExtras{FORM_SIGNS, nullptr, 0, NsArgs{}, nullptr, aux_signs});
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// linear with a single output column (the D logit head, nsgan/GAN.py:68): wave-reduced dot product
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_out1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y,
                                                              int B, int K, int epilogue) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const float* row = x + (size_t)b * K;
    float s = 0.f;
    if ((K & 3) == 0) {
        for (int k = lane * 4; k < K; k += 256) {
            const float4 a = *(const float4*)(row + k), ww = *(const float4*)(w + k);
            s = fmaf(a.x, ww.x, s); s = fmaf(a.y, ww.y, s); s = fmaf(a.z, ww.z, s); s = fmaf(a.w, ww.w, s);
        }
    } else {
        for (int k = lane; k < K; k += 64) s = fmaf(row[k], w[k], s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
        float v = s + (bias ? bias[0] : 0.f);
        if (epilogue == CGS_EPI_LRELU) v = fmaxf(v, 0.2f * v);
        y[b] = v;
    }
}

// the logit head and the loss seed in one launch (the last launches of every D forward of the refinement loop, both a few microseconds of
// latency): y[b] = x[b] . w + bias; dl[b] = d loss(KIND) / dy (BCE: sigmoid(y[b]) - 1, the stable form of the seed kernels); lm[b] = y[b];
// with LADAM the sample's ladam state from sigmoid(y[b]) (cgs_refine_loss_seed at P = 1)
template <int KIND, bool LADAM>
__device__ __forceinline__ void linear_out1_seed_body(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ y, float* __restrict__ dl, float* __restrict__ lm, int B, int K,
                                                      const cgs_ladam_seed& la) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const float* row = x + (size_t)b * K;
    float s = 0.f;
    if ((K & 3) == 0) {
        for (int k = lane * 4; k < K; k += 256) {
            const float4 a = *(const float4*)(row + k), ww = *(const float4*)(w + k);
            s = fmaf(a.x, ww.x, s); s = fmaf(a.y, ww.y, s); s = fmaf(a.z, ww.z, s); s = fmaf(a.w, ww.w, s);
        }
    } else {
        for (int k = lane; k < K; k += 64) s = fmaf(row[k], w[k], s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
        const float v = s + (bias ? bias[0] : 0.f);
        y[b] = v;
        dl[b] = loss_seed1<KIND>(v);
        lm[b] = v;
        if (LADAM) ladam_seed1(la, b, sigmoid_stable(v));
    }
}

__global__ __launch_bounds__(256) void linear_out1_bce_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ y, float* __restrict__ dl, float* __restrict__ lm, int B, int K) {
    linear_out1_seed_body<CGS_LOSS_BCE, false>(x, w, bias, y, dl, lm, B, K, cgs_ladam_seed{});
}

template <int KIND, bool LADAM>
__global__ __launch_bounds__(256) void linear_out1_seed_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ y, float* __restrict__ dl, float* __restrict__ lm, int B, int K,
                                                               cgs_ladam_seed la) {
    linear_out1_seed_body<KIND, LADAM>(x, w, bias, y, dl, lm, B, K, la);
}

__global__ __launch_bounds__(256) void linear_out1_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                              float* __restrict__ dx, int B, int K) {
    const size_t n = (size_t)B * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / K), k = (int)(i - (size_t)b * K);
        dx[i] = dy[b] * w[k];
    }
}

extern "C" {

int cgs_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int in, int out, int epilogue,
                   void* ws, size_t ws_bytes, int ws_prepacked, void* stream) {
    if (B <= 0 || in <= 0 || out <= 0) return cgs_set_error(CGS_EINVAL, "linear_fwd: B=%d in=%d out=%d", B, in, out);
    if (epilogue != CGS_EPI_NONE && epilogue != CGS_EPI_LRELU) return cgs_set_error(CGS_EINVAL, "linear_fwd: epilogue %d", epilogue);
    if (out == 1) {
        hipLaunchKernelGGL(linear_out1_fwd_kernel, dim3(cgs_ceil_div(B, 4)), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, B, in, epilogue);
        CGS_CHECK_LAUNCH("linear_out1_fwd");
        return CGS_OK;
    }
    // a 1x1 convolution over a 1x1 image
    return conv_entry("linear_fwd", CGS_CONV_FWD, x, w, bias, y, B, 1, 1, in, 0, 0, out, 1, 1, 1, 1, epilogue, nullptr, nullptr, nullptr, ws, ws_bytes, ws_prepacked,
                      stream);
}

int cgs_linear_out1_bce(const float* x, const float* w, const float* bias, float* logits, float* dlogits, float* logit_mean, int B, int in,
                        void* stream) {
    if (B <= 0 || in <= 0 || !x || !w || !logits || !dlogits || !logit_mean) return cgs_set_error(CGS_EINVAL, "linear_out1_bce: bad argument");
    hipLaunchKernelGGL(linear_out1_bce_kernel, dim3(cgs_ceil_div(B, 4)), dim3(256), 0, (hipStream_t)stream, x, w, bias, logits, dlogits, logit_mean, B, in);
    CGS_CHECK_LAUNCH("linear_out1_bce");
    return CGS_OK;
}

int cgs_linear_out1_seed(const float* x, const float* w, const float* bias, float* logits, float* dlogits, float* logit_mean, int B, int in,
                         int kind, const cgs_ladam_seed* ladam, void* stream) {
    if (B <= 0 || in <= 0 || !x || !w || !logits || !dlogits || !logit_mean) return cgs_set_error(CGS_EINVAL, "linear_out1_seed: bad argument");
    if (kind != CGS_LOSS_BCE && kind != CGS_LOSS_LSQ && kind != CGS_LOSS_LINEAR) return cgs_set_error(CGS_EINVAL, "linear_out1_seed: kind %d", kind);
    if (ladam && (!ladam->s_real || !ladam->loss_avg || !ladam->gain)) return cgs_set_error(CGS_EINVAL, "linear_out1_seed: ladam state with a null pointer");
    if (kind == CGS_LOSS_BCE && !ladam) return cgs_linear_out1_bce(x, w, bias, logits, dlogits, logit_mean, B, in, stream);
    const dim3 grid(cgs_ceil_div(B, 4)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const cgs_ladam_seed la = ladam ? *ladam : cgs_ladam_seed{};
#define OUT1_SEED(KIND, LADAM) hipLaunchKernelGGL((linear_out1_seed_kernel<KIND, LADAM>), grid, block, 0, st, x, w, bias, logits, dlogits, logit_mean, B, in, la)
    if (kind == CGS_LOSS_BCE) OUT1_SEED(CGS_LOSS_BCE, true);
    else if (kind == CGS_LOSS_LSQ) { if (ladam) OUT1_SEED(CGS_LOSS_LSQ, true); else OUT1_SEED(CGS_LOSS_LSQ, false); }
    else { if (ladam) OUT1_SEED(CGS_LOSS_LINEAR, true); else OUT1_SEED(CGS_LOSS_LINEAR, false); }
#undef OUT1_SEED
    CGS_CHECK_LAUNCH("linear_out1_seed");
    return CGS_OK;
}

int cgs_linear_bwd_data(const float* dy, const float* w, float* dx, int B, int in, int out, void* ws, size_t ws_bytes,
                        int ws_prepacked, void* stream) {
    if (B <= 0 || in <= 0 || out <= 0) return cgs_set_error(CGS_EINVAL, "linear_bwd_data: B=%d in=%d out=%d", B, in, out);
    if (out == 1) {
        size_t n = (size_t)B * in;
        unsigned blocks = (unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
        hipLaunchKernelGGL(linear_out1_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, w, dx, B, in);
        CGS_CHECK_LAUNCH("linear_out1_bwd");
        return CGS_OK;
    }
    return conv_entry("linear_bwd_data", CGS_CONV_BWD_DATA, dy, w, nullptr, dx, B, 1, 1, in, 0, 0, out, 1, 1, 1, 1, CGS_EPI_NONE, nullptr, nullptr, nullptr, ws,
                      ws_bytes, ws_prepacked, stream);
}

}  // extern "C"
