// The shape limits and the refusals that the entry points of the 2-D nets share, narrow (mlp2d.hip) and wide (mlp2d_wide*.hip): one
// order, one text.  An entry point's own checks (its output, its grad_plugin) stand between the two calls.
#pragma once
#include "cgs_internal.h"

#define MLP2D_MAX_LAYERS 6        // mlp2d.hip keeps all layers (and their transposes) in LDS: 6 layers = 133 KB of 160 KB
#define MLP2D_NARROW_MAX_NH 64    // one lane per unit: the wave-per-sample kernels of mlp2d.hip
#define MLP2D_WIDE_MIN_NH 65      // the sample-tile kernels of mlp2d_wide*.hip
#define MLP2D_MAX_NH 256

static bool mlp2d_shape_ok(int nlayers, int nh, int min_nh, int max_nh) { return nlayers >= 2 && nlayers <= MLP2D_MAX_LAYERS && nh >= min_nh && nh <= max_nh; }

// the shape, then the weight arrays, then every weight
static int mlp2d_check_net(const char* who, const float* const* w, const float* const* b, int nlayers, int nh, int min_nh, int max_nh) {
    if (!mlp2d_shape_ok(nlayers, nh, min_nh, max_nh))
        return cgs_set_error(CGS_EINVAL, "%s: nlayers=%d nhidden=%d (need 2..%d, %d..%d)", who, nlayers, nh, MLP2D_MAX_LAYERS, min_nh, max_nh);
    if (!w || !b) return cgs_set_error(CGS_EINVAL, "%s: null weight array", who);
    for (int l = 0; l < nlayers; ++l)
        if (!w[l] || !b[l]) return cgs_set_error(CGS_EINVAL, "%s: null weight", who);
    return CGS_OK;
}

// the generator's batch-norm variables, then z, the batch (training needs two rows; max_B: what the kernels' float row counts allow) and
// eps, then the workspace
static int mlp2d_check_gen(const char* who, const float* const* gamma, const float* const* beta, float* const* mm, float* const* mv, int nlayers,
                           const float* z, int B, int max_B, int train, float eps, size_t need, void* ws, size_t ws_bytes) {
    if (!gamma || !beta || !mm || !mv) return cgs_set_error(CGS_EINVAL, "%s: null batch-norm array", who);
    for (int l = 0; l < nlayers - 1; ++l)
        if (!gamma[l] || !beta[l] || !mm[l] || !mv[l]) return cgs_set_error(CGS_EINVAL, "%s: null batch-norm variable", who);
    if (!z || B < (train ? 2 : 1) || B > max_B || !(eps > 0.f)) return cgs_set_error(CGS_EINVAL, "%s: bad argument (B=%d, training=%d)", who, B, train);
    if (!ws || ws_bytes < need) return cgs_set_error(CGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return CGS_OK;
}
