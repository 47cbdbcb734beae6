// Predictions back on the patient's native grid: the inverse of ctl_resample_inplane + ctl_crop_or_pad (include/ctl_hip.h, "native-grid
// restoration").
//   ctl_restore_scores   window-grid class scores (NHWC) -> native-grid uint8 labels and, optionally, the native-grid soft prediction:
//                        bilinear in fp64 over the logits or over the per-pixel softmax, arg-max on the fp64 values, one launch
//   ctl_restore_labels   window-grid uint8 labels -> native-grid uint8 labels, nearest neighbour, one launch
// One thread per native voxel, lanes along x: neighbouring lanes read the same or neighbouring window pixels (L2 / L1 hits) and every
// store of a wave is contiguous.  No workspace, no atomics, no readback: the launches depend on the shapes only.
#include "ctl_device.h"
#include <math.h>

#pragma clang fp contract(off)      // every multiply and add rounds on its own (the numpy statement's order), as in ctl_prep.hip

#define RB 256
#define RESTORE_MAX_C 16
#define RESTORE_TENSOR_BYTES (1ll << 31)

// one axis of one native index: the window coordinate u = i * q - d, whether the voxel is inside on this axis, and the two taps
struct rs_axis {
    double t;       // weight of tap i1
    int i0, i1;     // clamped separately: u in [-0.5, 0) reads pixel 0 twice
    int nn;         // nearest pixel, clamp(floor(u + 0.5))
    bool inside;
};

__device__ __forceinline__ rs_axis rs_coord(int i, double q, int d, int size_res, int size_win) {
    rs_axis a;
    const double c = __dmul_rn((double)i, q);                  // one multiply, never contracted into the subtraction
    const double u = c - (double)d;
    a.inside = c < (double)size_res - 0.5 && u >= -0.5 && u < (double)size_win - 0.5;
    const double f = floor(u);
    a.t = u - f;
    const int fi = a.inside ? (int)f : 0;                      // outside: u may be anything, the taps are not used
    a.i0 = fi < 0 ? 0 : (fi > size_win - 1 ? size_win - 1 : fi);
    a.i1 = fi + 1 < 0 ? 0 : (fi + 1 > size_win - 1 ? size_win - 1 : fi + 1);
    const int ni = a.inside ? (int)floor(u + 0.5) : 0;
    a.nn = ni < 0 ? 0 : (ni > size_win - 1 ? size_win - 1 : ni);
    return a;
}

// softmax of one window pixel in fp64: exp(x_k - max) / sum_j exp(x_j - max), the sum in ascending j
template <int C>
__device__ __forceinline__ void rs_softmax(double* s) {
    double m = s[0];
#pragma unroll
    for (int k = 1; k < C; ++k) m = s[k] > m ? s[k] : m;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < C; ++k) { s[k] = exp(s[k] - m); sum = k ? sum + s[k] : s[k]; }
#pragma unroll
    for (int k = 0; k < C; ++k) s[k] = s[k] / sum;
}

// CT = 4: a tap is one aligned 16-byte load and everything stays in registers; CT = 0: any class count, the taps are re-read per class
// (the second read hits L1) and, in mode 1, each tap's maximum and sum are formed first, so no per-class array is indexed at run time.
template <int CT>
__global__ __launch_bounds__(RB) void restore_scores_kernel(const float* __restrict__ src, uint8_t* __restrict__ label, float* __restrict__ soft,
                                                             int n, int c, int hc, int wc, int h, int w, int rh, int rw, int dy, int dx,
                                                             double qh, double qw, int mode) {
    const int64_t plane = (int64_t)h * w;
    const int64_t total = (int64_t)n * plane;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % w);
        const int64_t r = i / w;
        const int y = (int)(r % h);
        const int64_t b = r / h;
        const rs_axis ay = rs_coord(y, qh, dy, rh, hc), ax = rs_coord(x, qw, dx, rw, wc);
        float* so = soft ? soft + b * c * plane + (int64_t)y * w + x : nullptr;
        if (!(ay.inside && ax.inside)) {
            label[i] = 0;
            if (so)
                for (int k = 0; k < c; ++k) so[k * plane] = (mode == 1 && k == 0) ? 1.f : 0.f;
            continue;
        }
        const float* img = src + b * hc * wc * c;
        const float* p00 = img + ((int64_t)ay.i0 * wc + ax.i0) * c;
        const float* p01 = img + ((int64_t)ay.i0 * wc + ax.i1) * c;
        const float* p10 = img + ((int64_t)ay.i1 * wc + ax.i0) * c;
        const float* p11 = img + ((int64_t)ay.i1 * wc + ax.i1) * c;
        const double tx = ax.t, ty = ay.t, ux = 1.0 - ax.t, uy = 1.0 - ay.t;
        double best = 0.0;
        int bi = 0;
        if (CT == 4) {
            const f32x4 a00 = *reinterpret_cast<const f32x4*>(p00), a01 = *reinterpret_cast<const f32x4*>(p01);
            const f32x4 a10 = *reinterpret_cast<const f32x4*>(p10), a11 = *reinterpret_cast<const f32x4*>(p11);
            double s00[4] = {a00.x, a00.y, a00.z, a00.w}, s01[4] = {a01.x, a01.y, a01.z, a01.w};
            double s10[4] = {a10.x, a10.y, a10.z, a10.w}, s11[4] = {a11.x, a11.y, a11.z, a11.w};
            if (mode == 1) { rs_softmax<4>(s00); rs_softmax<4>(s01); rs_softmax<4>(s10); rs_softmax<4>(s11); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double top = s00[k] * ux + s01[k] * tx;
                const double bot = s10[k] * ux + s11[k] * tx;
                const double v = top * uy + bot * ty;
                if (k == 0 || v > best) { best = v; bi = k; }
                if (so) so[k * plane] = (float)v;
            }
        } else {
            double m00 = 0.0, m01 = 0.0, m10 = 0.0, m11 = 0.0, z00 = 1.0, z01 = 1.0, z10 = 1.0, z11 = 1.0;
            if (mode == 1) {
                m00 = p00[0]; m01 = p01[0]; m10 = p10[0]; m11 = p11[0];
                for (int k = 1; k < c; ++k) {
                    const double v00 = p00[k], v01 = p01[k], v10 = p10[k], v11 = p11[k];
                    m00 = v00 > m00 ? v00 : m00; m01 = v01 > m01 ? v01 : m01;
                    m10 = v10 > m10 ? v10 : m10; m11 = v11 > m11 ? v11 : m11;
                }
                for (int k = 0; k < c; ++k) {
                    const double e00 = exp((double)p00[k] - m00), e01 = exp((double)p01[k] - m01);
                    const double e10 = exp((double)p10[k] - m10), e11 = exp((double)p11[k] - m11);
                    z00 = k ? z00 + e00 : e00; z01 = k ? z01 + e01 : e01;
                    z10 = k ? z10 + e10 : e10; z11 = k ? z11 + e11 : e11;
                }
            }
            for (int k = 0; k < c; ++k) {
                double s00 = p00[k], s01 = p01[k], s10 = p10[k], s11 = p11[k];
                if (mode == 1) {
                    s00 = exp(s00 - m00) / z00; s01 = exp(s01 - m01) / z01;
                    s10 = exp(s10 - m10) / z10; s11 = exp(s11 - m11) / z11;
                }
                const double top = s00 * ux + s01 * tx;
                const double bot = s10 * ux + s11 * tx;
                const double v = top * uy + bot * ty;
                if (k == 0 || v > best) { best = v; bi = k; }
                if (so) so[k * plane] = (float)v;
            }
        }
        label[i] = (uint8_t)bi;
    }
}

__global__ __launch_bounds__(RB) void restore_labels_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int hc, int wc,
                                                             int h, int w, int rh, int rw, int dy, int dx, double qh, double qw) {
    const int64_t total = (int64_t)n * h * w;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % w);
        const int64_t r = i / w;
        const int y = (int)(r % h);
        const int64_t b = r / h;
        const rs_axis ay = rs_coord(y, qh, dy, rh, hc), ax = rs_coord(x, qw, dx, rw, wc);
        uint8_t v = 0;
        if (ay.inside && ax.inside) v = src[(b * hc + ay.nn) * wc + ax.nn];
        dst[i] = v;
    }
}

// the checks both entries share: sizes, ratios, the 2 GiB limit of the label volumes
#define RESTORE_REQUIRE_GEOMETRY(who)                                                                                                      \
    CTL_REQUIRE(n > 0 && win_h > 0 && win_w > 0 && h > 0 && w > 0 && res_h > 0 && res_w > 0,                                               \
                who ": sizes must be positive (n %d, window %d x %d, native %d x %d, resampled %d x %d)", n, win_h, win_w, h, w, res_h,    \
                res_w);                                                                                                                    \
    CTL_REQUIRE(q_h > 0.0 && q_w > 0.0 && isfinite(q_h) && isfinite(q_w), who ": spacing ratios %g, %g must be positive and finite", q_h,  \
                q_w)

extern "C" int ctl_restore_scores(const float* scores, int32_t n, int32_t c, int32_t win_h, int32_t win_w, int32_t h, int32_t w,
                                  int32_t res_h, int32_t res_w, int32_t off_y, int32_t off_x, double q_h, double q_w, int32_t mode,
                                  uint8_t* label, float* soft, ctl_stream stream) {
    CTL_REQUIRE(scores && label, "restore_scores: null pointer (scores and label are required)");
    RESTORE_REQUIRE_GEOMETRY("restore_scores");
    CTL_REQUIRE(c >= 1 && c <= RESTORE_MAX_C, "restore_scores: %d classes (1..%d)", c, RESTORE_MAX_C);
    CTL_REQUIRE(mode == 0 || mode == 1, "restore_scores: mode %d (0 = logit, 1 = prob)", mode);
    CTL_REQUIRE((int64_t)n * c * win_h * win_w * 4 < RESTORE_TENSOR_BYTES && (int64_t)n * h * w < RESTORE_TENSOR_BYTES &&
                    (!soft || (int64_t)n * c * h * w * 4 < RESTORE_TENSOR_BYTES),
                "restore_scores: %d x %d x %d x %d -> %d x %d reaches the 2 GiB tensor limit (32-bit byte offsets)", n, c, win_h, win_w, h, w);
    const dim3 grid(ctl_blocks((int64_t)n * h * w, RB, 2048)), blk(RB);
    if (ctl_vec4(c, scores))
        restore_scores_kernel<4><<<grid, blk, 0, S_>>>(scores, label, soft, n, c, win_h, win_w, h, w, res_h, res_w, off_y, off_x, q_h, q_w, mode);
    else
        restore_scores_kernel<0><<<grid, blk, 0, S_>>>(scores, label, soft, n, c, win_h, win_w, h, w, res_h, res_w, off_y, off_x, q_h, q_w, mode);
    CTL_LAUNCH_CHECK("restore_scores");
    return CTL_OK;
}

extern "C" int ctl_restore_labels(const uint8_t* labels, int32_t n, int32_t win_h, int32_t win_w, int32_t h, int32_t w, int32_t res_h,
                                  int32_t res_w, int32_t off_y, int32_t off_x, double q_h, double q_w, uint8_t* out, ctl_stream stream) {
    CTL_REQUIRE(labels && out, "restore_labels: null pointer (labels and out are required)");
    RESTORE_REQUIRE_GEOMETRY("restore_labels");
    CTL_REQUIRE((int64_t)n * win_h * win_w < RESTORE_TENSOR_BYTES && (int64_t)n * h * w < RESTORE_TENSOR_BYTES,
                "restore_labels: %d x %d x %d -> %d x %d reaches the 2 GiB tensor limit (32-bit byte offsets)", n, win_h, win_w, h, w);
    restore_labels_kernel<<<dim3(ctl_blocks((int64_t)n * h * w, RB, 2048)), dim3(RB), 0, S_>>>(labels, out, n, win_h, win_w, h, w, res_h, res_w,
                                                                                              off_y, off_x, q_h, q_w);
    CTL_LAUNCH_CHECK("restore_labels");
    return CTL_OK;
}
