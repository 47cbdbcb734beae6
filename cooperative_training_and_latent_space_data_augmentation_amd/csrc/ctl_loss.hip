// Segmentation losses next to ce2d (ctl_elem.hip): class-weighted cross-entropy, focal, soft Dice and foreground soft Dice of fp32 NHWC
// logits against an int64 label map (medseg/models/custom_loss.py: cross_entropy_2D :706-740, FocalLoss :222-255, SoftDiceLoss :356-396,
// SelectiveSoftDiceLoss :434-471).  HBM-bound streaming kernels: a pixel's channel row lives in registers, its softmax is recomputed by
// the backward instead of being stored.  Sums are two-stage and ordered (per-block fp64 partials, one finalize block): no float atomics,
// the same bits on every call.  Nothing is read back; no launch argument changes from step to step.
//
// A label outside 0..c-1 is no class: one-hot 0 for every k, weight 0.  Labels are only ever compared with a class index.
//
// The distance-map losses ('boundary', 'hausdorff dt'; no upstream counterpart) stream the same way with one or two fp32 NHWC field tensors
// beside the logits (ctl_dist.hip writes them); ctl_confident_label is the thresholding of a prediction whose fields 'hausdorff dt' needs.
#include "ctl_rows.h"

#define EB CTL_ROW_THREADS   // threads per block
#define LOSS_MAX_STREAM_BLOCKS 2048

struct ctl_w16 { float v[CTL_ROW_MAXC]; };      // normalised class weights, a launch argument (constant from step to step)

// ------------------------------------------------------------------------------------------------ point-wise kinds
// pixel term of the loss and the factor f of its gradient f * (p_k - t_k):
//   weighted cross-entropy: -w[y] log p_y,           f = w[y]
//   focal:                  -(1 - p_y)^gamma log p_y, f = (1 - p_y)^gamma    (upstream detaches p_y, custom_loss.py:243)
// 1 - p_y is formed as (sum of the other exponentials) / s: no cancellation where p_y is close to 1.
template <int CT>
__device__ __forceinline__ float pw_factor(int kind, const float* e, float s, int c, int64_t l, const ctl_w16& w, float gamma) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    if (kind == CTL_LOSS_WCE) {
        float wl = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) wl = (l == (int64_t)k) ? w.v[k] : wl;
        return wl;
    }
    float so = 0.f;
    bool valid = false;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) { const bool hit = l == (int64_t)k; so += hit ? 0.f : e[k]; valid = valid || hit; }
    return valid ? powf(so / s, gamma) : 0.f;
}
template <int CT>
__global__ __launch_bounds__(EB) void seg_pw_partial_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                             int64_t pixels, int c_rt, int kind, ctl_w16 w, float gamma,
                                                             double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    __shared__ double sm[EB / 64];
    const int c = CT ? CT : c_rt;
    const int64_t stride = (int64_t)gridDim.x * EB;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < pixels; i += stride) {
        float v[NC], x[NC];
        ctl_row_load<CT>(logit, i, c, v);
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) x[k] = v[k];
        float s;
        const float m = ctl_row_exp<CT>(v, c, s);
        const int64_t l = label[i];
        float xl = m;      // (no class: log p = -log s, times the factor 0)
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) xl = (l == (int64_t)k) ? x[k] : xl;
        const float f = pw_factor<CT>(kind, v, s, c, l, w, gamma);
        acc += (double)(-(f * (xl - m - logf(s))));
    }
    acc = ctl_block_sum_double<EB / 64>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(EB) void seg_pw_finalize_kernel(const double* __restrict__ partial, int blocks, double mul,
                                                              float* __restrict__ out) {
    __shared__ double sm[EB / 64];
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += EB) s += partial[b];
    s = ctl_block_sum_double<EB / 64>(s, sm);
    if (threadIdx.x == 0) out[0] = (float)(s * mul);
}

// ------------------------------------------------------------------------------------------------ Dice kinds, forward
// pass 1: grid (blocks of a sample, sample); partial[b][block][k][3] = sum p_k, sum p_k t_k, count of y == k over the block's pixels
template <int CT>
__global__ __launch_bounds__(EB) void dice_partial_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label, int64_t hw,
                                                           int c_rt, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    __shared__ double sm[EB / 64][3 * CTL_ROW_MAXC];
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const float* __restrict__ x = logit + b * hw * c;
    const int64_t* __restrict__ y = label + b * hw;
    double sp[NC], spt[NC];
    int cnt[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) { sp[k] = 0.0; spt[k] = 0.0; cnt[k] = 0; }
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < hw; i += stride) {
        float v[NC];
        ctl_row_load<CT>(x, i, c, v);
        float s;
        ctl_row_exp<CT>(v, c, s);
        const float r = 1.f / s;
        const int64_t l = y[i];
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            const double p = (double)(v[k] * r);
            const bool hit = l == (int64_t)k;
            sp[k] += p;
            spt[k] += hit ? p : 0.0;
            cnt[k] += hit ? 1 : 0;
        }
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) {
        const double a = wave_sum_double(sp[k]), t = wave_sum_double(spt[k]), n = wave_sum_double((double)cnt[k]);
        if ((threadIdx.x & 63) == 0) { sm[wv][3 * k] = a; sm[wv][3 * k + 1] = t; sm[wv][3 * k + 2] = n; }
    }
    CTL_BLOCK_ROWS_STORE(sm, EB / 64, 3 * c, partial + ((b * gridDim.x + blockIdx.x) * c) * 3);
}
// pass 2, one block: a group of 16 lanes sums the `nb` block rows of one (sample, class) in a fixed order, the group's first lane forms
// the Dice term and the two coefficients of the backward:  g_k = dL/dp_k = coef[b][k][0] * t_k + coef[b][k][1]
//   term = num / U,  U = sum p + count + s,  num = 2 (sum p t + s)   ['dice']   or   2 sum p t + s   ['foreground dice', classes >= 1]
//   loss = 1 - (sum of the terms) / div;   coef[0] = -(2 / U) / div,  coef[1] = (num / U^2) / div;   0 for a class that is not selected
__global__ __launch_bounds__(EB) void dice_finalize_kernel(const double* __restrict__ partial, int items, int nb, int c, int fg, double div,
                                                            double* __restrict__ coef, float* __restrict__ loss) {
#pragma clang fp contract(off)
    __shared__ double sm[EB / 64];
    const double smooth = 0.01;
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    double acc = 0.0;
    for (int base = 0; base < items; base += EB / 16) {
        const int it = base + grp;
        const bool ok = it < items;
        const int64_t b = ok ? it / c : 0;
        const int k = ok ? it % c : 0;
        double sp = 0.0, spt = 0.0, n = 0.0;
        if (ok) {
            for (int j = lane; j < nb; j += 16) {
                const double* __restrict__ q = partial + ((b * nb + j) * c + k) * 3;
                sp += q[0]; spt += q[1]; n += q[2];
            }
        }
        CTL_GROUP16_SUM3(sp, spt, n);
        if (ok && lane == 0) {
            const bool sel = !fg || k >= 1;
            const double U = sp + n + smooth;
            const double num = fg ? 2.0 * spt + smooth : 2.0 * (spt + smooth);
            coef[(int64_t)it * 2] = sel ? -(2.0 / U) / div : 0.0;
            coef[(int64_t)it * 2 + 1] = sel ? (num / (U * U)) / div : 0.0;
            acc += sel ? num / U : 0.0;
        }
    }
    acc = ctl_block_sum_double<EB / 64>(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(1.0 - acc / div);
}

// ------------------------------------------------------------------------------------------------ backward of every kind
// grid (blocks of a sample, sample).  point-wise kinds: dlogit_k = gout / pixels * f * (p_k - t_k).  Dice kinds: with g_k from the
// coefficient table, dlogit_j = gout * p_j * sum_k p_k (g_j - g_k), formed in fp64 (it cancels where the row is confident).
template <int CT>
__global__ __launch_bounds__(EB) void seg_loss_bwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                           const float* __restrict__ gout, const double* __restrict__ coef, int64_t hw,
                                                           int c_rt, int kind, ctl_w16 w, float gamma, float pixels_f,
                                                           float* __restrict__ dlogit) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const float* __restrict__ x = logit + b * hw * c;
    const int64_t* __restrict__ y = label + b * hw;
    float* __restrict__ dx = dlogit + b * hw * c;
    const bool dice = kind == CTL_LOSS_DICE || kind == CTL_LOSS_FG_DICE;
    const float go = gout[0];
    const float gs = go / pixels_f;
    double ca[NC], cb[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const bool on = dice && k < c;
        ca[k] = on ? coef[(b * c + k) * 2] : 0.0;
        cb[k] = on ? coef[(b * c + k) * 2 + 1] : 0.0;
    }
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < hw; i += stride) {
        float v[NC];
        ctl_row_load<CT>(x, i, c, v);
        float s;
        ctl_row_exp<CT>(v, c, s);
        const float r = 1.f / s;
        const int64_t l = y[i];
        if (dice) {
            // sum_k p_k (g_j - g_k) = g_j S - dot with S the sum of the ROUNDED p_k (1 only up to 1e-7): every p_k enters with its own
            // relative accuracy, so a confident row's small gradient keeps its relative accuracy too
            double g[NC], dot = 0.0, S = 0.0;
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) {
                v[k] = v[k] * r;
                g[k] = (l == (int64_t)k) ? ca[k] + cb[k] : cb[k];
                dot += (double)v[k] * g[k];
                S += (double)v[k];
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) v[k] = (float)((double)go * ((double)v[k] * (g[k] * S - dot)));
        } else {
            const float gf = gs * pw_factor<CT>(kind, v, s, c, l, w, gamma);
            float so = 0.f;      // p_y - 1 = -(sum of the other exponentials) / s: no cancellation where p_y is close to 1
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) so += (l == (int64_t)k) ? 0.f : v[k];
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) v[k] = gf * ((l == (int64_t)k) ? -(so * r) : v[k] * r);
        }
        ctl_row_store<CT>(dx, i, c, v);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
static inline bool kind_is_dice(int kind) { return kind == CTL_LOSS_DICE || kind == CTL_LOSS_FG_DICE; }
// the tensor limit of both loss families: logits of c floats per pixel beside labels of 8 bytes per pixel
static int loss_check_2gib(const char* who, int64_t b, int64_t hw, int c) {
    const int64_t row_bytes = c * 4 > 8 ? c * 4 : 8;
    CTL_REQUIRE(hw < ((int64_t)1 << 31) && b * hw < ((int64_t)1 << 31) / row_bytes,
                "%s: %lld x %lld pixels of %d classes reach the 2 GiB tensor limit", who, (long long)b, (long long)hw, c);
    return CTL_OK;
}
// the checks every entry shares; the message names the entry
static int seg_loss_check(const char* who, int kind, int64_t b, int64_t hw, int c) {
    CTL_REQUIRE(kind >= CTL_LOSS_WCE && kind <= CTL_LOSS_FG_DICE, "%s: unknown loss kind %d", who, kind);
    CTL_REQUIRE(b > 0 && hw > 0, "%s: sizes must be positive (batch %lld, pixels per sample %lld)", who, (long long)b, (long long)hw);
    if (int rc = ctl_check_channels(who, c, "classes")) return rc;
    CTL_REQUIRE(kind != CTL_LOSS_FG_DICE || c >= 2, "%s: foreground dice needs at least 2 classes (got %d)", who, c);
    if (int rc = ctl_check_batch(who, b)) return rc;
    return loss_check_2gib(who, b, hw, c);
}
// w' = w / sum(w) * c in fp64, handed to the kernels as fp32 (custom_loss.py:733-734); NULL = upstream's uniform 1/c, i.e. all ones
static int seg_loss_weights(const char* who, int kind, int c, const double* class_weights, float gamma, ctl_w16* w) {
    for (int k = 0; k < CTL_ROW_MAXC; ++k) w->v[k] = k < c ? 1.f : 0.f;
    if (kind == CTL_LOSS_WCE && class_weights) {
        double wn[CTL_ROW_MAXC];
        if (int rc = ctl_class_weights_norm(who, c, class_weights, wn)) return rc;
        for (int k = 0; k < c; ++k) w->v[k] = (float)wn[k];
    }
    CTL_REQUIRE(kind != CTL_LOSS_FOCAL || (std::isfinite(gamma) && gamma >= 0.f), "%s: focal gamma %g (finite, >= 0)", who, (double)gamma);
    return CTL_OK;
}

extern "C" int32_t ctl_seg_loss_blocks(int32_t b, int64_t hw) {
    return (b > 0 && hw > 0) ? ctl_sample_blocks(b, hw, EB, CTL_RED_BLOCKS) : 0;
}
extern "C" size_t ctl_seg_loss_ws_doubles(int32_t kind, int32_t b, int64_t hw, int32_t c) {
    if (seg_loss_check("seg_loss_ws_doubles", kind, b, hw, c) != CTL_OK) return 0;
    if (!kind_is_dice(kind)) return CTL_RED_BLOCKS;
    return (size_t)b * ctl_sample_blocks(b, hw, EB, CTL_RED_BLOCKS) * c * 3 + (size_t)b * c * 2;
}
extern "C" int ctl_seg_loss_fwd(int32_t kind, const float* logit, const int64_t* label, const double* class_weights, float gamma,
                                int32_t b, int64_t hw, int32_t c, double* ws, float* loss, ctl_stream stream) {
    CTL_REQUIRE(logit && label && ws && loss, "seg_loss_fwd: null pointer");
    if (int rc = seg_loss_check("seg_loss_fwd", kind, b, hw, c)) return rc;
    ctl_w16 w;
    if (int rc = seg_loss_weights("seg_loss_fwd", kind, c, class_weights, gamma, &w)) return rc;
    const bool v4 = ctl_vec4(c, logit);
    if (kind_is_dice(kind)) {
        const int nb = ctl_sample_blocks(b, hw, EB, CTL_RED_BLOCKS);
        double* coef = ws + (size_t)b * nb * c * 3;
        const int fg = kind == CTL_LOSS_FG_DICE;
        CTL_ROW_DISPATCH(dice_partial_kernel, v4, dim3(nb, b), logit, label, hw, c, ws);
        dice_finalize_kernel<<<dim3(1), dim3(EB), 0, S_>>>(ws, b * c, nb, c, fg, (double)b * (double)(fg ? c - 1 : c), coef, loss);
    } else {
        const int64_t pixels = (int64_t)b * hw;
        CTL_ROW_DISPATCH(seg_pw_partial_kernel, v4, dim3(CTL_RED_BLOCKS), logit, label, pixels, c, kind, w, gamma, ws);
        seg_pw_finalize_kernel<<<dim3(1), dim3(EB), 0, S_>>>(ws, CTL_RED_BLOCKS, 1.0 / (double)pixels, loss);
    }
    ctl_count_launches(1);      // partial + finalize
    CTL_LAUNCH_CHECK("seg_loss_fwd");
    return CTL_OK;
}
extern "C" int ctl_seg_loss_bwd(int32_t kind, const float* logit, const int64_t* label, const double* class_weights, float gamma,
                                const float* gout, const double* ws, int32_t b, int64_t hw, int32_t c, float* dlogit, ctl_stream stream) {
    CTL_REQUIRE(logit && label && gout && dlogit, "seg_loss_bwd: null pointer");
    if (int rc = seg_loss_check("seg_loss_bwd", kind, b, hw, c)) return rc;
    CTL_REQUIRE(!kind_is_dice(kind) || ws, "seg_loss_bwd: null pointer (the Dice kinds read the coefficient table of the forward from ws)");
    ctl_w16 w;
    if (int rc = seg_loss_weights("seg_loss_bwd", kind, c, class_weights, gamma, &w)) return rc;
    const double* coef = kind_is_dice(kind) ? ws + (size_t)b * ctl_sample_blocks(b, hw, EB, CTL_RED_BLOCKS) * c * 3 : nullptr;
    const dim3 grid(ctl_sample_blocks(b, hw, EB, LOSS_MAX_STREAM_BLOCKS), b);
    const float pixels_f = (float)((int64_t)b * hw);
    CTL_ROW_DISPATCH(seg_loss_bwd_kernel, ctl_vec4(c, logit, dlogit), grid, logit, label, gout, coef, hw, c, kind, w, gamma, pixels_f, dlogit);
    CTL_LAUNCH_CHECK("seg_loss_bwd");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ distance-map losses
// p = softmax(x) as the kernels above form it (exp(x - max) * (1 / sum), fp32); everything behind it is fp64.  Classes 1..c-1, div = b (c-1) hw.
//   boundary      g_k = a_k / div                          (a = the signed map of the label),            term = sum_k p_k a_k
//   hausdorff dt  g_k = 2 (p_k - t_k) (a_k + b_k) / div    (a, b = squared fields of label / prediction), term = sum_k (p_k - t_k)^2 (a_k + b_k)
// and dL/dx_j = p_j (g_j S - sum_k p_k g_k) with S the sum of the rounded p_k, as the Dice backward has it.
template <int CT>
__device__ __forceinline__ void dl_fields(int kind, const float* __restrict__ fa, const float* __restrict__ fb, int64_t i, int c, double* d) {
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    float a[NC], b[NC];
    ctl_row_load<CT>(fa, i, c, a);
    if (kind == CTL_DLOSS_HAUSDORFF_DT) ctl_row_load<CT>(fb, i, c, b);
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) d[k] = k == 0 ? 0.0 : (kind == CTL_DLOSS_HAUSDORFF_DT ? (double)a[k] + (double)b[k] : (double)a[k]);
}
template <int CT>
__global__ __launch_bounds__(EB) void dist_loss_partial_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                                const float* __restrict__ fa, const float* __restrict__ fb, int64_t pixels,
                                                                int c_rt, int kind, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    __shared__ double sm[EB / 64];
    const int c = CT ? CT : c_rt;
    const int64_t stride = (int64_t)gridDim.x * EB;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < pixels; i += stride) {
        float v[NC];
        double d[NC];
        ctl_row_load<CT>(logit, i, c, v);
        float s;
        ctl_row_exp<CT>(v, c, s);
        const float r = 1.f / s;
        dl_fields<CT>(kind, fa, fb, i, c, d);
        const int64_t l = kind == CTL_DLOSS_HAUSDORFF_DT ? label[i] : -1;
#pragma unroll
        for (int k = 1; k < NC; ++k) if (k < c) {
            const double p = (double)(v[k] * r);
            if (kind == CTL_DLOSS_HAUSDORFF_DT) {
                const double e = p - (l == (int64_t)k ? 1.0 : 0.0);
                acc += e * e * d[k];
            } else {
                acc += p * d[k];
            }
        }
    }
    acc = ctl_block_sum_double<EB / 64>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
template <int CT>
__global__ __launch_bounds__(EB) void dist_loss_bwd_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label,
                                                            const float* __restrict__ fa, const float* __restrict__ fb,
                                                            const float* __restrict__ gout, int64_t pixels, int c_rt, int kind, double inv_div,
                                                            float* __restrict__ dlogit) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    const int c = CT ? CT : c_rt;
    const double go = (double)gout[0];
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < pixels; i += stride) {
        float v[NC];
        double d[NC], g[NC];
        ctl_row_load<CT>(logit, i, c, v);
        float s;
        ctl_row_exp<CT>(v, c, s);
        const float r = 1.f / s;
        dl_fields<CT>(kind, fa, fb, i, c, d);
        const int64_t l = kind == CTL_DLOSS_HAUSDORFF_DT ? label[i] : -1;
        double dot = 0.0, S = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            v[k] = v[k] * r;
            const double p = (double)v[k];
            g[k] = kind == CTL_DLOSS_HAUSDORFF_DT ? 2.0 * (p - (l == (int64_t)k ? 1.0 : 0.0)) * d[k] * inv_div : d[k] * inv_div;
            dot += p * g[k];
            S += p;
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) v[k] = (float)(go * ((double)v[k] * (g[k] * S - dot)));
        ctl_row_store<CT>(dlogit, i, c, v);
    }
}
// first class whose softmax probability exceeds 1/2 (at most one can), else 255
template <int CT>
__global__ __launch_bounds__(EB) void confident_label_kernel(const float* __restrict__ logit, int64_t pixels, int c_rt, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    const int c = CT ? CT : c_rt;
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < pixels; i += stride) {
        float v[NC];
        ctl_row_load<CT>(logit, i, c, v);
        float s;
        ctl_row_exp<CT>(v, c, s);
        const float r = 1.f / s;
        int q = 255;
#pragma unroll
        for (int k = NC - 1; k >= 0; --k) if (k < c) q = v[k] * r > 0.5f ? k : q;
        out[i] = (uint8_t)q;
    }
}

static int dist_loss_check(const char* who, int kind, int64_t b, int64_t hw, int c) {
    CTL_REQUIRE(kind == CTL_DLOSS_BOUNDARY || kind == CTL_DLOSS_HAUSDORFF_DT, "%s: unknown loss kind %d (0: boundary, 1: hausdorff dt)", who, kind);
    CTL_REQUIRE(b > 0 && hw > 0, "%s: sizes must be positive (batch %lld, pixels per sample %lld)", who, (long long)b, (long long)hw);
    CTL_REQUIRE(c >= 2 && c <= CTL_ROW_MAXC, "%s: %d classes (2 .. %d: the loss runs over the classes 1 .. c-1)", who, c, CTL_ROW_MAXC);
    return loss_check_2gib(who, b, hw, c);
}
extern "C" size_t ctl_dist_loss_ws_doubles(int32_t kind, int32_t b, int64_t hw, int32_t c) {
    return dist_loss_check("dist_loss_ws_doubles", kind, b, hw, c) == CTL_OK ? CTL_RED_BLOCKS : 0;
}
extern "C" int ctl_dist_loss_fwd(int32_t kind, const float* logit, const int64_t* label, const float* field_a, const float* field_b, int32_t b,
                                 int64_t hw, int32_t c, double* ws, float* loss, ctl_stream stream) {
    CTL_REQUIRE(logit && field_a && ws && loss, "dist_loss_fwd: null pointer");
    if (int rc = dist_loss_check("dist_loss_fwd", kind, b, hw, c)) return rc;
    CTL_REQUIRE(kind != CTL_DLOSS_HAUSDORFF_DT || (label && field_b), "dist_loss_fwd: null pointer (hausdorff dt reads the label map and two fields)");
    const int64_t pixels = (int64_t)b * hw;
    CTL_ROW_DISPATCH(dist_loss_partial_kernel, ctl_vec4(c, logit, field_a, field_b), dim3(CTL_RED_BLOCKS), logit, label, field_a, field_b, pixels, c, kind, ws);
    seg_pw_finalize_kernel<<<dim3(1), dim3(EB), 0, S_>>>(ws, CTL_RED_BLOCKS, 1.0 / ((double)pixels * (double)(c - 1)), loss);
    ctl_count_launches(1);      // partial + finalize
    CTL_LAUNCH_CHECK("dist_loss_fwd");
    return CTL_OK;
}
extern "C" int ctl_dist_loss_bwd(int32_t kind, const float* logit, const int64_t* label, const float* field_a, const float* field_b,
                                 const float* gout, int32_t b, int64_t hw, int32_t c, float* dlogit, ctl_stream stream) {
    CTL_REQUIRE(logit && field_a && gout && dlogit, "dist_loss_bwd: null pointer");
    if (int rc = dist_loss_check("dist_loss_bwd", kind, b, hw, c)) return rc;
    CTL_REQUIRE(kind != CTL_DLOSS_HAUSDORFF_DT || (label && field_b), "dist_loss_bwd: null pointer (hausdorff dt reads the label map and two fields)");
    const int64_t pixels = (int64_t)b * hw;
    const double inv_div = 1.0 / ((double)pixels * (double)(c - 1));
    const dim3 grid(ctl_blocks(pixels, EB, LOSS_MAX_STREAM_BLOCKS));
    const bool v4 = ctl_vec4(c, logit, field_a, field_b) && ((uintptr_t)dlogit & 15) == 0;
    CTL_ROW_DISPATCH(dist_loss_bwd_kernel, v4, grid, logit, label, field_a, field_b, gout, pixels, c, kind, inv_div, dlogit);
    CTL_LAUNCH_CHECK("dist_loss_bwd");
    return CTL_OK;
}
extern "C" int ctl_confident_label(const float* logit, uint8_t* out, int64_t pixels, int32_t c, ctl_stream stream) {
    CTL_REQUIRE(logit && out, "confident_label: null pointer");
    CTL_REQUIRE(pixels > 0 && pixels < ((int64_t)1 << 31) / (c > 0 ? c * 4 : 4), "confident_label: %lld pixels (positive, below the 2 GiB tensor limit)",
                (long long)pixels);
    if (int rc = ctl_check_channels("confident_label", c, "classes")) return rc;
    const dim3 grid(ctl_blocks(pixels, EB, LOSS_MAX_STREAM_BLOCKS));
    CTL_ROW_DISPATCH(confident_label_kernel, ctl_vec4(c, logit), grid, logit, pixels, c, out);
    CTL_LAUNCH_CHECK("confident_label");
    return CTL_OK;
}
