// Training augmentation of a whole batch on the device (medseg/dataset_loader/transform.py:46-86 runs it per slice on the host): flip,
// contrast / brightness, random affine, choice rotation, elastic deformation, centre crop -- ONE resampling of image and label.
// Gather and stencil work: no MFMA, no atomics, fixed launch counts, identical bits on every call.
//   ctl_aug_field   elastic displacement alpha * G_sigma(u) of every sample and both axes (elastic_transform.py:41-58): a row pass and a
//                   column pass, each from an LDS-staged line with the normalised weights of scipy's gaussian_filter
//   ctl_aug_warp    per-plane min / max partials, then one gather over the crop window: bilinear image taps through the intensity
//                   map (intensity_transform.py:136-162), nearest-neighbour label
//   ctl_aug_spline_coeffs / ctl_aug_warp_cubic   the same gather through a cubic spline (elastic_transform.py:84-92): B-spline coefficients
//                   of the image and of every class indicator, then 4x4 taps
//   ctl_aug_bias    smooth multiplicative bias field, min-max normalisation, Gaussian noise (intensity_transform.py:373-546), a pre-pass
//   ctl_aug_coarse_field   the displacement of the 3x3 coarse grid (elastic_transform.py:105-172); both at the end of this file
// The contract of all of them is written out in include/ctl_hip.h.
#include "ctl_device.h"

#define AUG_B 256
#define AUG_MAX_SIDE 512          // LDS staging of one row / one column tile is sized for this
#define AUG_MAX_RADIUS 1024       // int(4 sigma + 0.5) is clamped here: twice the largest side, every tap beyond a side reads zeros anyway
#define AUG_COLS 16               // columns of one column-pass tile: 512 x 16 floats = 32 KiB of LDS
#define AUG_BPP 64                // min / max partial blocks per plane (the scheme of ctl_rescale_intensity)
#define AUG_TW 64                 // warp tile: 64 pixels along x (one wave per row: coalesced stores) x 4 rows

static inline bool aug_shape_ok(int n, int hp, int wp, int hc, int wc) {
    return n > 0 && n <= 65535 && hp > 0 && wp > 0 && hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE && hc > 0 && wc > 0 && hc <= hp && wc <= wp;
}
static inline size_t aug_tmp_bytes(int n, int hp, int wp) { return ctl_align256((size_t)n * 2 * hp * wp * sizeof(float)); }
static inline size_t aug_partial_bytes(int n) { return ctl_align256((size_t)n * AUG_BPP * 2 * sizeof(float)); }

extern "C" size_t ctl_aug_ws_bytes(int32_t n, int32_t hp, int32_t wp) { return aug_shape_ok(n, hp, wp, 1, 1) ? aug_tmp_bytes(n, hp, wp) : 0; }
extern "C" size_t ctl_aug_warp_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc) {
    return aug_shape_ok(n, hp, wp, hc, wc) ? aug_partial_bytes(n) : 0;
}

struct aug_range { const void* p; size_t bytes; };
// true when one of the `nw` written ranges at the front of r[] overlaps any other range of r[] (NULL ranges are skipped)
static bool aug_any_overlap(const aug_range* r, int count, int nw) {
    for (int i = 0; i < nw; ++i)
        for (int j = 0; j < count; ++j) {
            if (j == i || (j < nw && j < i)) continue;
            if (ctl_overlap(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) return true;
        }
    return false;
}

// ------------------------------------------------------------------------------------------------ elastic displacement
// uniform in [-1, 1) on a 2^-23 grid from (seed, sample * 2 + axis, pixel): stateless, the same value whatever the launch geometry
__device__ __forceinline__ float aug_uniform(uint64_t seed, int plane, int pixel) {
    const uint64_t h = ctl_mix64(seed ^ ctl_mix64(((uint64_t)(uint32_t)plane << 32) | (uint32_t)pixel));
    return (float)(h >> 40) * (1.0f / 8388608.0f) - 1.0f;
}

// Weights of scipy.ndimage.gaussian_filter1d(sigma, truncate=4.0): radius R = int(4 sigma + 0.5), w[k] = exp(-k^2 / (2 sigma^2)) / sum over
// -R..R, formed in fp64 and rounded once.  Only w[0 .. min(R, side - 1)] is stored (farther taps read the zero border); the sum runs
// over the whole radius.  sigma <= 0 or NaN: radius 0, the identity.  Returns the stored radius; ends with a barrier.
__device__ int aug_weights(float sigma, int side, float* __restrict__ w, double* __restrict__ red) {
    const double sd = (double)sigma;
    int radius = 0;
    if (sigma > 0.f) {
        const double r = 4.0 * sd + 0.5;
        radius = r >= (double)AUG_MAX_RADIUS ? AUG_MAX_RADIUS : (int)r;
    }
    const double q = radius > 0 ? -0.5 / (sd * sd) : 0.0;
    double part = 0.0;
    for (int k = threadIdx.x; k <= radius; k += AUG_B) {
        const double e = exp(q * (double)k * (double)k);
        part += k ? 2.0 * e : e;
    }
    part = wave_sum_double(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    double total = 0.0;
    for (int i = 0; i < AUG_B / 64; ++i) total += red[i];
    const int stored = radius < side - 1 ? radius : side - 1;
    for (int k = threadIdx.x; k <= stored; k += AUG_B) w[k] = (float)(exp(q * (double)k * (double)k) / total);
    __syncthreads();
    return stored;
}

// one block = one row of one (sample, axis) plane: u made or read into LDS, filtered along x
__global__ __launch_bounds__(AUG_B) void aug_field_row_kernel(const float* __restrict__ noise, const uint64_t* __restrict__ seeds,
                                                               const float* __restrict__ alpha, const float* __restrict__ sigma, int hp, int wp,
                                                               float* __restrict__ tmp) {
    __shared__ float row[AUG_MAX_SIDE];
    __shared__ float w[AUG_MAX_SIDE];
    __shared__ double red[AUG_B / 64];
    const int y = blockIdx.x, b = blockIdx.z, plane = b * 2 + (int)blockIdx.y;
    if (alpha[b] == 0.f) return;                               // block-uniform: the column pass writes this sample's zeros
    const int64_t base = ((int64_t)plane * hp + y) * wp;
    for (int x = threadIdx.x; x < wp; x += AUG_B) row[x] = noise ? noise[base + x] : aug_uniform(seeds[b], plane, y * wp + x);
    const int r = aug_weights(sigma[b], wp, w, red);           // its barriers also publish row[]
    for (int x = threadIdx.x; x < wp; x += AUG_B) {
        float acc = 0.f;
        for (int k = -r; k <= r; ++k) {                        // k is wave-uniform: w[] is a broadcast read, row[] a conflict-free one
            const int xx = x + k;
            if (xx >= 0 && xx < wp) acc = fmaf(w[k < 0 ? -k : k], row[xx], acc);
        }
        tmp[base + x] = acc;
    }
}

// one block = AUG_COLS columns of one (sample, axis) plane over the whole height: filtered along y, times alpha
__global__ __launch_bounds__(AUG_B) void aug_field_col_kernel(const float* __restrict__ tmp, const float* __restrict__ alpha,
                                                               const float* __restrict__ sigma, int hp, int wp, float* __restrict__ field) {
    __shared__ float col[AUG_MAX_SIDE * AUG_COLS];
    __shared__ float w[AUG_MAX_SIDE];
    __shared__ double red[AUG_B / 64];
    const int b = blockIdx.z, plane = b * 2 + (int)blockIdx.y;
    const int lx = threadIdx.x % AUG_COLS, ly = threadIdx.x / AUG_COLS, x = (int)blockIdx.x * AUG_COLS + lx;
    const int64_t base = (int64_t)plane * hp * wp;
    const float a = alpha[b];
    if (a == 0.f) {                                            // block-uniform
        if (x < wp)
            for (int y = ly; y < hp; y += AUG_B / AUG_COLS) field[base + (int64_t)y * wp + x] = 0.f;
        return;
    }
    for (int y = ly; y < hp; y += AUG_B / AUG_COLS) col[y * AUG_COLS + lx] = x < wp ? tmp[base + (int64_t)y * wp + x] : 0.f;
    const int r = aug_weights(sigma[b], hp, w, red);
    for (int y = ly; y < hp; y += AUG_B / AUG_COLS) {
        float acc = 0.f;
        for (int k = -r; k <= r; ++k) {
            const int yy = y + k;
            if (yy >= 0 && yy < hp) acc = fmaf(w[k < 0 ? -k : k], col[yy * AUG_COLS + lx], acc);
        }
        if (x < wp) field[base + (int64_t)y * wp + x] = a * acc;
    }
}

extern "C" int ctl_aug_field(const float* noise, const uint64_t* seeds, const float* alpha, const float* sigma, int32_t n, int32_t hp,
                             int32_t wp, float* field, void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(n > 0 && n <= 65535 && hp > 0 && wp > 0, "aug_field: n (1..65535), hp and wp must be positive (got %d, %d, %d)", n, hp, wp);
    CTL_REQUIRE(hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE, "aug_field: the LDS staging holds planes up to %d x %d, got %d x %d", AUG_MAX_SIDE,
                AUG_MAX_SIDE, hp, wp);
    CTL_REQUIRE(noise || seeds, "aug_field: neither a noise array nor per-sample seeds");
    CTL_REQUIRE(alpha && sigma, "aug_field: alpha and sigma (device float [n]) are required");
    CTL_REQUIRE(field, "aug_field: no output field");
    CTL_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "aug_field: the workspace must be a 256-byte aligned device buffer");
    CTL_REQUIRE(workspace_bytes >= aug_tmp_bytes(n, hp, wp), "aug_field: workspace of %zu bytes, ctl_aug_ws_bytes asks for %zu", workspace_bytes,
                aug_tmp_bytes(n, hp, wp));
    const size_t fbytes = (size_t)n * 2 * hp * wp * sizeof(float);
    const aug_range r[] = {{field, fbytes}, {workspace, aug_tmp_bytes(n, hp, wp)}, {noise, fbytes}, {seeds, (size_t)n * 8}, {alpha, (size_t)n * 4},
                           {sigma, (size_t)n * 4}};
    CTL_REQUIRE(!aug_any_overlap(r, 6, 2), "aug_field: field and workspace must not overlap each other or an input");
    float* tmp = (float*)workspace;
    aug_field_row_kernel<<<dim3((unsigned)hp, 2, (unsigned)n), dim3(AUG_B), 0, S_>>>(noise, seeds, alpha, sigma, hp, wp, tmp);
    aug_field_col_kernel<<<dim3((unsigned)ctl_cdiv(wp, AUG_COLS), 2, (unsigned)n), dim3(AUG_B), 0, S_>>>(tmp, alpha, sigma, hp, wp, field);
    ctl_count_launches(1);
    CTL_LAUNCH_CHECK("aug_field");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ warp
__global__ __launch_bounds__(AUG_B) void aug_minmax_partial_kernel(const float* __restrict__ x, int plane_elems, float* __restrict__ partial) {
    __shared__ float sm[2 * AUG_B / 64];
    const float* xp = x + (int64_t)blockIdx.y * plane_elems;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = (int)blockIdx.x * AUG_B + threadIdx.x; i < plane_elems; i += AUG_BPP * AUG_B) {
        const float v = xp[i];
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    ctl_block_minmax<AUG_B>(mn, mx, sm);
    if (threadIdx.x == 0) { partial[((int64_t)blockIdx.y * AUG_BPP + blockIdx.x) * 2] = mn; partial[((int64_t)blockIdx.y * AUG_BPP + blockIdx.x) * 2 + 1] = mx; }
}

// s = M (p + d(p) - c) + c of output pixel (y, x) of sample b in fp32 (prm = the sample's matrix), shared by both gathers
__device__ __forceinline__ void aug_source(const float* __restrict__ field, const float* prm, int b, int y, int x, int hp, int wp, int cy,
                                           int cx, float& sr, float& sc) {
    const int py = y + cy, px = x + cx;                        // inside the padded grid: cy + hc <= hp, cx + wc <= wp
    const int64_t plane = (int64_t)hp * wp;
    float qr = (float)py, qc = (float)px;
    if (field) {
        qr += field[(int64_t)b * 2 * plane + (int64_t)py * wp + px];
        qc += field[((int64_t)b * 2 + 1) * plane + (int64_t)py * wp + px];
    }
    const float cr = 0.5f * (float)(hp - 1), cc = 0.5f * (float)(wp - 1);
    qr -= cr; qc -= cc;
    sr = prm[0] * qr + prm[1] * qc + prm[2] + cr;
    sc = prm[3] * qr + prm[4] * qc + prm[5] + cc;
    // everything at or beyond one pixel outside the array is zero: clamping there changes no result and keeps the conversions defined
    sr = fminf(fmaxf(sr, -2.f), (float)hp + 1.f);
    sc = fminf(fmaxf(sc, -2.f), (float)wp + 1.f);
}

__global__ __launch_bounds__(AUG_B) void aug_warp_kernel(const float* __restrict__ image, const int64_t* __restrict__ label,
                                                          const float* __restrict__ matrix, const float* __restrict__ intensity,
                                                          const float* __restrict__ field, const float* __restrict__ partial, int hp, int wp,
                                                          int hc, int wc, int cy, int cx, float* __restrict__ image_out,
                                                          int64_t* __restrict__ label_out) {
    __shared__ float sm[2 * AUG_B / 64];
    __shared__ float prm[8];                                   // the sample's matrix (6) and intensity scalars (2), read once per block
    const int b = blockIdx.z;
    float mn = INFINITY, mx = -INFINITY;
    if (threadIdx.x < AUG_BPP) { mn = partial[((int64_t)b * AUG_BPP + threadIdx.x) * 2]; mx = partial[((int64_t)b * AUG_BPP + threadIdx.x) * 2 + 1]; }
    if (threadIdx.x < 6) prm[threadIdx.x] = matrix[b * 6 + threadIdx.x];
    else if (threadIdx.x < 8) prm[threadIdx.x] = intensity[b * 2 + threadIdx.x - 6];
    ctl_block_minmax<AUG_B>(mn, mx, sm);                       // its barriers also publish prm[]
    const int x = (int)blockIdx.x * AUG_TW + (threadIdx.x & 63), y = (int)blockIdx.y * (AUG_B / AUG_TW) + (threadIdx.x >> 6);
    if (x >= wc || y >= hc) return;
    const int64_t plane = (int64_t)hp * wp;
    float sr, sc;
    aug_source(field, prm, b, y, x, hp, wp, cy, cx, sr, sc);
    const float fy0 = floorf(sr), fx0 = floorf(sc);
    const int y0 = (int)fy0, x0 = (int)fx0;
    const double wy = (double)(sr - fy0), wx = (double)(sc - fx0);
    const float scale = prm[6], bright = prm[7];
    const float* ip = image + (int64_t)b * plane;
    double tap[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ty = y0 + (t >> 1), tx = x0 + (t & 1);
        float v = 0.f;
        if (ty >= 0 && ty < hp && tx >= 0 && tx < wp) v = fminf(fmaxf(fmaf(ip[(int64_t)ty * wp + tx], scale, bright), mn), mx);
        tap[t] = (double)v;
    }
    // four taps combined in fp64 and rounded once: the value error stays at the rounding of the intensity map and of the store
    const double top = tap[0] + wx * (tap[1] - tap[0]), bot = tap[2] + wx * (tap[3] - tap[2]);
    const int64_t o = ((int64_t)b * hc + y) * wc + x;
    image_out[o] = (float)(top + wy * (bot - top));
    const int ry = (int)floorf(sr + 0.5f), rx = (int)floorf(sc + 0.5f);
    int64_t lv = 0;
    if (ry >= 0 && ry < hp && rx >= 0 && rx < wp) lv = label[(int64_t)b * plane + (int64_t)ry * wp + rx];
    label_out[o] = lv;
}

extern "C" int ctl_aug_warp(const float* image, const int64_t* label, const float* matrix, const float* intensity, const float* field,
                            int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc, float* image_out, int64_t* label_out, void* workspace,
                            size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(n > 0 && n <= 65535 && hp > 0 && wp > 0 && hc > 0 && wc > 0, "aug_warp: n (1..65535) and every size must be positive (got n %d, %d x %d -> %d x %d)",
                n, hp, wp, hc, wc);
    CTL_REQUIRE(hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE, "aug_warp: planes up to %d x %d (the limit of ctl_aug_field), got %d x %d", AUG_MAX_SIDE,
                AUG_MAX_SIDE, hp, wp);
    CTL_REQUIRE(hc <= hp && wc <= wp, "aug_warp: the crop %d x %d is larger than the input %d x %d", hc, wc, hp, wp);
    CTL_REQUIRE(image && label, "aug_warp: image and label are both required");
    CTL_REQUIRE(matrix && intensity, "aug_warp: matrix (float [n,2,3]) and intensity (float [n,2]) are required");
    CTL_REQUIRE(image_out && label_out, "aug_warp: image_out and label_out are both required");
    CTL_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "aug_warp: the workspace must be a 256-byte aligned device buffer");
    CTL_REQUIRE(workspace_bytes >= aug_partial_bytes(n), "aug_warp: workspace of %zu bytes, ctl_aug_warp_ws_bytes asks for %zu", workspace_bytes,
                aug_partial_bytes(n));
    const size_t in_px = (size_t)n * hp * wp, out_px = (size_t)n * hc * wc;
    const aug_range r[] = {{image_out, out_px * 4}, {label_out, out_px * 8}, {workspace, aug_partial_bytes(n)}, {image, in_px * 4}, {label, in_px * 8},
                           {field, in_px * 8}, {matrix, (size_t)n * 24}, {intensity, (size_t)n * 8}};
    CTL_REQUIRE(!aug_any_overlap(r, 8, 3), "aug_warp: an output or the workspace overlaps another array (the gather reads whole input planes)");
    float* partial = (float*)workspace;
    const int cy = (hp - hc + 1) / 2, cx = (wp - wc + 1) / 2;      // ceil((Hp - Hc) / 2): MySpecialCrop, affine_transform.py:280-283
    aug_minmax_partial_kernel<<<dim3(AUG_BPP, (unsigned)n), dim3(AUG_B), 0, S_>>>(image, hp * wp, partial);
    aug_warp_kernel<<<dim3((unsigned)ctl_cdiv(wc, AUG_TW), (unsigned)ctl_cdiv(hc, AUG_B / AUG_TW), (unsigned)n), dim3(AUG_B), 0, S_>>>(
        image, label, matrix, intensity, field, partial, hp, wp, hc, wc, cy, cx, image_out, label_out);
    ctl_count_launches(1);
    CTL_LAUNCH_CHECK("aug_warp");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ cubic spline
// Coefficients C(v) = scipy.ndimage.spline_filter(v, order=3, mode='reflect') of 1 + n_class planes per sample (plane 0: the image through
// the intensity map, plane 1 + k: the indicator of label k, formed while the row is staged), then a 4x4-tap gather over them.  The
// one-pole recursion of the prefilter (z = sqrt(3) - 2) is the two-sided sequence h[k] = sqrt(3) z^|k| over the symmetric extension
// d c b a | a b c d | d c b a; it is cut at |k| <= AUG_SP_R, where what is dropped is below 1e-23 of the sum, so each pass is an FIR over an
// LDS-staged, already reflected line like the passes of ctl_aug_field.  fp64 accumulation, fp32 storage of both stages.
// A line shorter than AUG_SP_SHORT is the one case where scipy is not that exact inverse: the last term of its causal initialisation
// reads the running sum in place of the first sample, an error of about |z|^(2 len) (4e-7 at 5 samples, below 1e-17 from 16 on).  The
// contract is scipy's result, so such a line goes through scipy's own recursion, by one thread: at most 15 samples.
#define AUG_SP_R 40
#define AUG_SP_SHORT 16
#define AUG_MAX_CLASS 16          // as ctl_confusion_hist

static inline bool aug_spline_ok(int n, int hp, int wp, int n_class, int min_class) {
    return aug_shape_ok(n, hp, wp, 1, 1) && n_class >= min_class && n_class <= AUG_MAX_CLASS;
}
static inline size_t aug_planes_bytes(int n, int hp, int wp, int n_class) { return ctl_align256((size_t)n * (1 + n_class) * hp * wp * sizeof(float)); }
static inline size_t aug_spline_bytes(int n, int hp, int wp, int n_class) { return aug_partial_bytes(n) + aug_planes_bytes(n, hp, wp, n_class); }
static inline size_t aug_cubic_bytes(int n, int hp, int wp, int n_class) { return aug_partial_bytes(n) + 2 * aug_planes_bytes(n, hp, wp, n_class); }

extern "C" size_t ctl_aug_spline_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t n_class) {
    return aug_spline_ok(n, hp, wp, n_class, 0) ? aug_spline_bytes(n, hp, wp, n_class) : 0;
}
extern "C" size_t ctl_aug_warp_cubic_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc, int32_t n_class) {
    return aug_shape_ok(n, hp, wp, hc, wc) && aug_spline_ok(n, hp, wp, n_class, 1) ? aug_cubic_bytes(n, hp, wp, n_class) : 0;
}

// index i of a line of `len` samples under the half-sample symmetric extension, folded as often as it takes (len may be 1)
__device__ __forceinline__ int aug_reflect(int i, int len) {
    const int period = 2 * len;
    int m = i % period;
    if (m < 0) m += period;
    return m < len ? m : period - 1 - m;
}
// h[k] = (-6 z / (1 - z^2)) z^k = sqrt(3) z^k for k = 0 .. AUG_SP_R; the caller's barrier publishes it
__device__ __forceinline__ void aug_spline_taps(double* __restrict__ h) {
    if (threadIdx.x <= AUG_SP_R) {
        const double z = sqrt(3.0) - 2.0;
        double p = sqrt(3.0);
        for (int k = 0; k < (int)threadIdx.x; ++k) p *= z;
        h[threadIdx.x] = p;
    }
}
// scipy's spline_filter1d(order=3, mode='reflect') on c[0], c[stride], .. (n < AUG_SP_SHORT samples) in place, statement by statement
// (ni_splines.c: gain, _init_causal_reflect, the causal and the anticausal sweep)
__device__ void aug_spline_recursion(double* c, int n, int stride) {
    const double z = sqrt(3.0) - 2.0;
    double z_n = 1.0;
    for (int i = 0; i < n; ++i) { c[i * stride] *= (1.0 - z) * (1.0 - 1.0 / z); z_n *= z; }
    const double c0 = c[0];
    double z_i = z;
    c[0] = c[0] + z_n * c[(n - 1) * stride];
    for (int i = 1; i < n; ++i) {                              // at i = n - 1 this reads c[0] as it stands: scipy's result, not the exact sum
        c[0] += z_i * (c[i * stride] + z_n * c[(n - 1 - i) * stride]);
        z_i *= z;
    }
    c[0] = c[0] * (z / (1.0 - z_n * z_n)) + c0;
    for (int i = 1; i < n; ++i) c[i * stride] += z * c[(i - 1) * stride];
    c[(n - 1) * stride] *= z / (z - 1.0);
    for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
}
#define AUG_SP_FIR(line, at, stride)                                                                         \
    double acc = 0.0;                                                                                        \
    for (int k = AUG_SP_R; k > 0; --k) acc = fma(h[k], (double)line[((at) - k) * (stride)] + (double)line[((at) + k) * (stride)], acc); \
    acc = fma(h[0], (double)line[(at) * (stride)], acc)

// one block = one row of one (sample, plane): the reflected row of v or of the indicator staged in fp64, filtered along x
__global__ __launch_bounds__(AUG_B) void aug_spline_row_kernel(const float* __restrict__ image, const int64_t* __restrict__ label,
                                                                const float* __restrict__ intensity, const float* __restrict__ partial, int hp,
                                                                int wp, float* __restrict__ tmp) {
    __shared__ double ext[AUG_MAX_SIDE + 2 * AUG_SP_R];
    __shared__ double h[AUG_SP_R + 1];
    __shared__ float sm[2 * AUG_B / 64];
    const int y = blockIdx.x, pl = blockIdx.y, b = blockIdx.z;
    const int64_t in_row = ((int64_t)b * hp + y) * wp;
    aug_spline_taps(h);
    if (pl == 0) {                                             // block-uniform
        float mn = INFINITY, mx = -INFINITY;
        if (threadIdx.x < AUG_BPP) { mn = partial[((int64_t)b * AUG_BPP + threadIdx.x) * 2]; mx = partial[((int64_t)b * AUG_BPP + threadIdx.x) * 2 + 1]; }
        ctl_block_minmax<AUG_B>(mn, mx, sm);
        const double scale = (double)intensity[b * 2], bright = (double)intensity[b * 2 + 1];
        for (int j = threadIdx.x; j < wp + 2 * AUG_SP_R; j += AUG_B)
            ext[j] = fmin(fmax(fma((double)image[in_row + aug_reflect(j - AUG_SP_R, wp)], scale, bright), (double)mn), (double)mx);
    } else {
        const int64_t k = pl - 1;
        for (int j = threadIdx.x; j < wp + 2 * AUG_SP_R; j += AUG_B) ext[j] = label[in_row + aug_reflect(j - AUG_SP_R, wp)] == k ? 1.0 : 0.0;
    }
    __syncthreads();
    const int64_t out_row = (((int64_t)b * gridDim.y + pl) * hp + y) * wp;
    if (wp < AUG_SP_SHORT) {                                   // block-uniform
        if (threadIdx.x == 0) aug_spline_recursion(ext + AUG_SP_R, wp, 1);
        __syncthreads();
        if ((int)threadIdx.x < wp) tmp[out_row + threadIdx.x] = (float)ext[AUG_SP_R + threadIdx.x];
        return;
    }
    for (int x = threadIdx.x; x < wp; x += AUG_B) {
        AUG_SP_FIR(ext, x + AUG_SP_R, 1);
        tmp[out_row + x] = (float)acc;
    }
}

// one block = AUG_COLS columns of one (sample, plane) over the whole reflected height: filtered along y
__global__ __launch_bounds__(AUG_B) void aug_spline_col_kernel(const float* __restrict__ tmp, int hp, int wp, float* __restrict__ coeffs) {
    __shared__ float col[(AUG_MAX_SIDE + 2 * AUG_SP_R) * AUG_COLS];
    __shared__ double h[AUG_SP_R + 1];
    __shared__ double line[AUG_SP_SHORT * AUG_COLS];
    const int lx = threadIdx.x % AUG_COLS, ly = threadIdx.x / AUG_COLS, x = (int)blockIdx.x * AUG_COLS + lx;
    const int64_t base = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * hp * wp;
    if (hp < AUG_SP_SHORT) {                                   // block-uniform: one thread per column
        if (ly == 0 && x < wp) {
            for (int y = 0; y < hp; ++y) line[y * AUG_COLS + lx] = (double)tmp[base + (int64_t)y * wp + x];
            aug_spline_recursion(line + lx, hp, AUG_COLS);
            for (int y = 0; y < hp; ++y) coeffs[base + (int64_t)y * wp + x] = (float)line[y * AUG_COLS + lx];
        }
        return;
    }
    aug_spline_taps(h);
    for (int j = ly; j < hp + 2 * AUG_SP_R; j += AUG_B / AUG_COLS)
        col[j * AUG_COLS + lx] = x < wp ? tmp[base + (int64_t)aug_reflect(j - AUG_SP_R, hp) * wp + x] : 0.f;
    __syncthreads();
    const float* cl = col + lx;
    for (int y = ly; y < hp; y += AUG_B / AUG_COLS) {
        AUG_SP_FIR(cl, y + AUG_SP_R, AUG_COLS);
        if (x < wp) coeffs[base + (int64_t)y * wp + x] = (float)acc;
    }
}

// min / max partials, rows, columns: 3 launches
static void aug_spline_launch(const float* image, const int64_t* label, const float* intensity, int n, int hp, int wp, int n_class,
                              void* workspace, float* coeffs, ctl_stream stream) {
    float* partial = (float*)workspace;
    float* tmp = (float*)((char*)workspace + aug_partial_bytes(n));
    aug_minmax_partial_kernel<<<dim3(AUG_BPP, (unsigned)n), dim3(AUG_B), 0, S_>>>(image, hp * wp, partial);
    aug_spline_row_kernel<<<dim3((unsigned)hp, (unsigned)(1 + n_class), (unsigned)n), dim3(AUG_B), 0, S_>>>(image, label, intensity, partial, hp, wp, tmp);
    aug_spline_col_kernel<<<dim3((unsigned)ctl_cdiv(wp, AUG_COLS), (unsigned)(1 + n_class), (unsigned)n), dim3(AUG_B), 0, S_>>>(tmp, hp, wp, coeffs);
}

extern "C" int ctl_aug_spline_coeffs(const float* image, const int64_t* label, const float* intensity, int32_t n, int32_t hp, int32_t wp,
                                     int32_t n_class, float* coeffs, void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(n > 0 && n <= 65535 && hp > 0 && wp > 0, "aug_spline_coeffs: n (1..65535), hp and wp must be positive (got %d, %d, %d)", n, hp, wp);
    CTL_REQUIRE(hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE, "aug_spline_coeffs: the LDS staging holds planes up to %d x %d, got %d x %d", AUG_MAX_SIDE,
                AUG_MAX_SIDE, hp, wp);
    CTL_REQUIRE(n_class >= 0 && n_class <= AUG_MAX_CLASS, "aug_spline_coeffs: n_class must be 0..%d, got %d", AUG_MAX_CLASS, n_class);
    CTL_REQUIRE(image && intensity, "aug_spline_coeffs: image and intensity (float [n,2]) are required");
    CTL_REQUIRE(label || n_class == 0, "aug_spline_coeffs: n_class %d asks for indicator planes, but there is no label", n_class);
    CTL_REQUIRE(coeffs, "aug_spline_coeffs: no output coeffs");
    CTL_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "aug_spline_coeffs: the workspace must be a 256-byte aligned device buffer");
    CTL_REQUIRE(workspace_bytes >= aug_spline_bytes(n, hp, wp, n_class), "aug_spline_coeffs: workspace of %zu bytes, ctl_aug_spline_ws_bytes asks for %zu",
                workspace_bytes, aug_spline_bytes(n, hp, wp, n_class));
    const size_t in_px = (size_t)n * hp * wp;
    const aug_range r[] = {{coeffs, in_px * (1 + n_class) * 4}, {workspace, aug_spline_bytes(n, hp, wp, n_class)}, {image, in_px * 4},
                           {n_class ? label : nullptr, in_px * 8}, {intensity, (size_t)n * 8}};
    CTL_REQUIRE(!aug_any_overlap(r, 5, 2), "aug_spline_coeffs: coeffs and workspace must not overlap each other or an input");
    aug_spline_launch(image, label, intensity, n, hp, wp, n_class, workspace, coeffs, stream);
    ctl_count_launches(2);
    CTL_LAUNCH_CHECK("aug_spline_coeffs");
    return CTL_OK;
}

// cubic B-spline weights of the taps floor(s) - 1 .. floor(s) + 2 for t = s - floor(s)
__device__ __forceinline__ void aug_bspline3(double t, double* __restrict__ w) {
    const double u = 1.0 - t;
    w[0] = u * u * u * (1.0 / 6.0);
    w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) * (1.0 / 6.0);
    w[2] = (4.0 - 6.0 * u * u + 3.0 * u * u * u) * (1.0 / 6.0);
    w[3] = t * t * t * (1.0 / 6.0);
}

__global__ __launch_bounds__(AUG_B) void aug_warp_cubic_kernel(const float* __restrict__ coeffs, const float* __restrict__ matrix,
                                                                const float* __restrict__ field, int hp, int wp, int hc, int wc, int cy, int cx,
                                                                int n_class, float* __restrict__ image_out, int64_t* __restrict__ label_out) {
    __shared__ float prm[6];
    const int b = blockIdx.z;
    if (threadIdx.x < 6) prm[threadIdx.x] = matrix[b * 6 + threadIdx.x];
    __syncthreads();
    const int x = (int)blockIdx.x * AUG_TW + (threadIdx.x & 63), y = (int)blockIdx.y * (AUG_B / AUG_TW) + (threadIdx.x >> 6);
    if (x >= wc || y >= hc) return;
    float sr, sc;
    aug_source(field, prm, b, y, x, hp, wp, cy, cx, sr, sc);
    const int64_t o = ((int64_t)b * hc + y) * wc + x;
    if (!(sr >= -0.5f && sr <= (float)hp - 0.5f && sc >= -0.5f && sc <= (float)wp - 0.5f)) {      // a border pulled into view is zero
        image_out[o] = 0.f;
        label_out[o] = 0;
        return;
    }
    const float fy0 = floorf(sr), fx0 = floorf(sc);
    double wy[4], wx[4];                                       // formed once, shared by the 1 + n_class planes
    aug_bspline3((double)(sr - fy0), wy);
    aug_bspline3((double)(sc - fx0), wx);
    int ry[4], rx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { ry[t] = aug_reflect((int)fy0 - 1 + t, hp) * wp; rx[t] = aug_reflect((int)fx0 - 1 + t, wp); }
    const int64_t plane = (int64_t)hp * wp;
    const float* cp = coeffs + (int64_t)b * (1 + n_class) * plane;
    int64_t lv = 0;
    for (int pl = 0; pl <= n_class; ++pl, cp += plane) {
        double val = 0.0;                                      // 16 taps combined in fp64, rounded once
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float* rp = cp + ry[t];
            val += wy[t] * (wx[0] * (double)rp[rx[0]] + wx[1] * (double)rp[rx[1]] + wx[2] * (double)rp[rx[2]] + wx[3] * (double)rp[rx[3]]);
        }
        if (pl == 0) image_out[o] = (float)val;
        else if (val >= 0.5) lv = pl - 1;                      // ascending: the largest class at or above 0.5 stays (elastic_transform.py:84-92)
    }
    label_out[o] = lv;
}

extern "C" int ctl_aug_warp_cubic(const float* image, const int64_t* label, const float* matrix, const float* intensity, const float* field,
                                  int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc, int32_t n_class, float* image_out,
                                  int64_t* label_out, void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(n > 0 && n <= 65535 && hp > 0 && wp > 0 && hc > 0 && wc > 0,
                "aug_warp_cubic: n (1..65535) and every size must be positive (got n %d, %d x %d -> %d x %d)", n, hp, wp, hc, wc);
    CTL_REQUIRE(hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE, "aug_warp_cubic: planes up to %d x %d (the LDS staging of the prefilter), got %d x %d",
                AUG_MAX_SIDE, AUG_MAX_SIDE, hp, wp);
    CTL_REQUIRE(hc <= hp && wc <= wp, "aug_warp_cubic: the crop %d x %d is larger than the input %d x %d", hc, wc, hp, wp);
    CTL_REQUIRE(n_class >= 1 && n_class <= AUG_MAX_CLASS, "aug_warp_cubic: n_class must be 1..%d, got %d", AUG_MAX_CLASS, n_class);
    CTL_REQUIRE(image && label, "aug_warp_cubic: image and label are both required");
    CTL_REQUIRE(matrix && intensity, "aug_warp_cubic: matrix (float [n,2,3]) and intensity (float [n,2]) are required");
    CTL_REQUIRE(image_out && label_out, "aug_warp_cubic: image_out and label_out are both required");
    CTL_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "aug_warp_cubic: the workspace must be a 256-byte aligned device buffer");
    CTL_REQUIRE(workspace_bytes >= aug_cubic_bytes(n, hp, wp, n_class), "aug_warp_cubic: workspace of %zu bytes, ctl_aug_warp_cubic_ws_bytes asks for %zu",
                workspace_bytes, aug_cubic_bytes(n, hp, wp, n_class));
    const size_t in_px = (size_t)n * hp * wp, out_px = (size_t)n * hc * wc;
    const aug_range r[] = {{image_out, out_px * 4}, {label_out, out_px * 8}, {workspace, aug_cubic_bytes(n, hp, wp, n_class)}, {image, in_px * 4},
                           {label, in_px * 8}, {field, in_px * 8}, {matrix, (size_t)n * 24}, {intensity, (size_t)n * 8}};
    CTL_REQUIRE(!aug_any_overlap(r, 8, 3), "aug_warp_cubic: an output or the workspace overlaps another array (the gather reads whole coefficient planes)");
    float* coeffs = (float*)((char*)workspace + aug_spline_bytes(n, hp, wp, n_class));
    const int cy = (hp - hc + 1) / 2, cx = (wp - wc + 1) / 2;
    aug_spline_launch(image, label, intensity, n, hp, wp, n_class, workspace, coeffs, stream);
    aug_warp_cubic_kernel<<<dim3((unsigned)ctl_cdiv(wc, AUG_TW), (unsigned)ctl_cdiv(hc, AUG_B / AUG_TW), (unsigned)n), dim3(AUG_B), 0, S_>>>(
        coeffs, matrix, field, hp, wp, hc, wc, cy, cx, n_class, image_out, label_out);
    ctl_count_launches(3);
    CTL_LAUNCH_CHECK("aug_warp_cubic");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ bias field
// MyRandomPurtarbationV2 (intensity_transform.py:373-546) as a pre-pass that writes a new image: the host fits the bicubic spline and hands
// over its knots, coefficients and the normalisation scalar (the record of include/ctl_hip.h); launch 1 evaluates it per pixel (de Boor in
// both axes from per-block LDS tables of the four non-zero basis values of every row and column), multiplies, and leaves min / max / sum
// partials; launch 2 reduces them, normalises, adds the noise.  fp64 from the fp32 record, one rounding per launch.
#define AUG_BIAS_FLOATS 192
#define AUG_BIAS_KNOTS 16
#define AUG_BIAS_COEF 12
#define AUG_BIAS_MIN_SIDE 128
#define AUG_BIAS_TY 8             // offsets into the record
#define AUG_BIAS_TX 24
#define AUG_BIAS_C 40
#define AUG_COARSE_FLOATS 24

static inline bool aug_bias_ok(int n, int hp, int wp) {
    return n > 0 && n <= 65535 && hp == wp && (hp & 1) == 0 && hp >= AUG_BIAS_MIN_SIDE && hp <= AUG_MAX_SIDE;
}
static inline size_t aug_bias_plane_bytes(int n, int hp, int wp) { return ctl_align256((size_t)n * hp * wp * sizeof(float)); }
static inline size_t aug_bias_partial_bytes(int n) { return ctl_align256((size_t)n * AUG_BPP * 3 * sizeof(double)); }
static inline size_t aug_bias_bytes(int n, int hp, int wp) { return aug_bias_plane_bytes(n, hp, wp) + aug_bias_partial_bytes(n); }

extern "C" size_t ctl_aug_bias_ws_bytes(int32_t n, int32_t hp, int32_t wp) { return aug_bias_ok(n, hp, wp) ? aug_bias_bytes(n, hp, wp) : 0; }

// FITPACK's fpbspl for degree 3: x is clamped to [t[3], t[nt - 4]] (what bispev does with an argument beyond the data), l = the span with
// t[l] <= x < t[l + 1] (the last one at the right end), h[0..3] = B_{l-3} .. B_l at x
__device__ __forceinline__ int aug_bias_basis(const double* __restrict__ t, int nt, double x, double* __restrict__ h) {
    x = fmin(fmax(x, t[3]), t[nt - 4]);
    int l = 3;
    while (l < nt - 5 && x >= t[l + 1]) ++l;
    h[0] = 1.0;
    h[1] = h[2] = h[3] = 0.0;
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
        double hh[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (i < j) {
                const int li = l + 1 + i, lj = li - j;
                const double f = hh[i] / (t[li] - t[lj]);
                h[i] += f * (t[li] - x);
                h[i + 1] = f * (x - t[lj]);
            }
        }
    }
    return l;
}
// knot count of an axis as the kernels use it: whatever the record holds, every index derived from it stays inside the record
__device__ __forceinline__ int aug_bias_knots(float v) { return v >= 8.f && v <= (float)AUG_BIAS_KNOTS ? (int)v : 8; }

// grid (AUG_BPP, n): a block strides over its sample's plane.  partial: double [n][AUG_BPP][3] = {min v, max v, sum of the input}
__global__ __launch_bounds__(AUG_B) void aug_bias_field_kernel(const float* __restrict__ image, const float* __restrict__ bias, int side,
                                                                float* __restrict__ v_out, double* __restrict__ partial) {
    __shared__ double ty[AUG_BIAS_KNOTS], tx[AUG_BIAS_KNOTS], cf[AUG_BIAS_COEF * AUG_BIAS_COEF];
    __shared__ double by[AUG_MAX_SIDE * 4], bx[AUG_MAX_SIDE * 4];
    __shared__ unsigned char ly[AUG_MAX_SIDE], lx[AUG_MAX_SIDE];
    __shared__ double red[3 * AUG_B / 64];
    const int b = blockIdx.y;
    const float* rec = bias + (int64_t)b * AUG_BIAS_FLOATS;
    if (rec[0] == 0.f) return;                                 // block-uniform: launch 2 copies this sample through
    const int nty = aug_bias_knots(rec[1]), ntx = aug_bias_knots(rec[2]);
    if (threadIdx.x < AUG_BIAS_KNOTS) { ty[threadIdx.x] = (double)rec[AUG_BIAS_TY + threadIdx.x]; tx[threadIdx.x] = (double)rec[AUG_BIAS_TX + threadIdx.x]; }
    if (threadIdx.x < AUG_BIAS_COEF * AUG_BIAS_COEF) cf[threadIdx.x] = (double)rec[AUG_BIAS_C + threadIdx.x];
    __syncthreads();
    const int half = side / 2;                                 // pixel (y, x) sits at (y - Hp / 2, x - Wp / 2) of the knot grid
    for (int i = threadIdx.x; i < 2 * side; i += AUG_B) {
        const bool rows = i < side;
        const int p = rows ? i : i - side;
        double h[4];
        const int l = aug_bias_basis(rows ? ty : tx, rows ? nty : ntx, (double)(p - half), h);
        double* dst = (rows ? by : bx) + p * 4;
        dst[0] = h[0]; dst[1] = h[1]; dst[2] = h[2]; dst[3] = h[3];
        (rows ? ly : lx)[p] = (unsigned char)(l - 3);
    }
    __syncthreads();
    const double scale = (double)rec[3], lo = 1.0 - (double)rec[4], hi = 1.0 + (double)rec[4];
    const int plane = side * side;
    const float* ip = image + (int64_t)b * plane;
    float* vp = v_out + (int64_t)b * plane;
    double mn = INFINITY, mx = -INFINITY, sum = 0.0;
    for (int i = (int)blockIdx.x * AUG_B + threadIdx.x; i < plane; i += AUG_BPP * AUG_B) {
        const int y = i / side, x = i - y * side;
        const double* hy = by + y * 4;
        const double* hx = bx + x * 4;
        const double* c = cf + (int)ly[y] * AUG_BIAS_COEF + (int)lx[x];
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            s += hy[r] * (hx[0] * c[r * AUG_BIAS_COEF] + hx[1] * c[r * AUG_BIAS_COEF + 1] + hx[2] * c[r * AUG_BIAS_COEF + 2] + hx[3] * c[r * AUG_BIAS_COEF + 3]);
        const float pix = ip[i];
        const float v = (float)((double)pix * fmin(fmax(scale * s, lo), hi));
        vp[i] = v;
        mn = fmin(mn, (double)v); mx = fmax(mx, (double)v); sum += (double)pix;
    }
    for (int o = 32; o > 0; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o)); mx = fmax(mx, __shfl_xor(mx, o)); }
    sum = wave_sum_double(sum);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv * 3] = mn; red[wv * 3 + 1] = mx; red[wv * 3 + 2] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < AUG_B / 64; ++i) { mn = fmin(mn, red[i * 3]); mx = fmax(mx, red[i * 3 + 1]); sum += red[i * 3 + 2]; }
        double* pp = partial + ((int64_t)b * AUG_BPP + blockIdx.x) * 3;
        pp[0] = mn; pp[1] = mx; pp[2] = sum;
    }
}

// standard normal from (seed, sample, pixel): the counter hash and the two uniforms of ctl_noise_clamp, Box-Muller in fp64
__device__ __forceinline__ double aug_normal(uint64_t seed, int sample, int pixel) {
    const uint64_t h = ctl_mix64(seed ^ ctl_mix64(((uint64_t)(uint32_t)sample << 32) | (uint32_t)pixel));
    const double u1 = (double)((h >> 40) + 1) * (1.0 / 16777216.0);          // (0, 1]
    const double u2 = (double)((h >> 8) & 0xFFFFFFu) * (1.0 / 16777216.0);   // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__global__ __launch_bounds__(AUG_B) void aug_bias_norm_kernel(const float* __restrict__ image, const float* __restrict__ v,
                                                               const float* __restrict__ bias, const double* __restrict__ partial,
                                                               const float* __restrict__ noise, const uint64_t* __restrict__ seeds, int plane,
                                                               float* __restrict__ out) {
    __shared__ double st[3];
    const int b = blockIdx.y;
    const float* rec = bias + (int64_t)b * AUG_BIAS_FLOATS;
    const bool on = rec[0] != 0.f;                             // block-uniform
    if (on && threadIdx.x < 64) {                              // AUG_BPP partials = one wave, combined in a fixed order
        const double* pp = partial + ((int64_t)b * AUG_BPP + threadIdx.x) * 3;
        double mn = pp[0], mx = pp[1];
        for (int o = 32; o > 0; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o)); mx = fmax(mx, __shfl_xor(mx, o)); }
        const double sum = wave_sum_double(pp[2]);
        if (threadIdx.x == 0) { st[0] = mn; st[1] = mx; st[2] = sum; }
    }
    __syncthreads();
    const float* ip = image + (int64_t)b * plane;
    float* op = out + (int64_t)b * plane;
    if (!on || !(fabs(st[2]) > 1e-6)) {                        // stage off, or a black plane: bit for bit
        for (int i = (int)blockIdx.x * AUG_B + threadIdx.x; i < plane; i += AUG_BPP * AUG_B) op[i] = ip[i];
        return;
    }
    const double mn = st[0], den = (st[1] - st[0]) + 1e-8, eps = (double)rec[5];
    const float* vp = v + (int64_t)b * plane;
    const uint64_t seed = seeds ? seeds[b] : 0;
    for (int i = (int)blockIdx.x * AUG_B + threadIdx.x; i < plane; i += AUG_BPP * AUG_B) {
        double o = ((double)vp[i] - mn) / den;
        if (eps > 0.0) {
            const double nz = noise ? (double)noise[(int64_t)b * plane + i] : aug_normal(seed, b, i);
            o = fmin(fmax(o + eps * nz, 0.0), 1.0);
        }
        op[i] = (float)o;
    }
}

extern "C" int ctl_aug_bias(const float* image, const float* bias, const float* noise, const uint64_t* seeds, int32_t n, int32_t hp, int32_t wp,
                            float* out, void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(n > 0 && n <= 65535, "aug_bias: n must be 1..65535, got %d", n);
    CTL_REQUIRE(hp == wp && (hp & 1) == 0 && hp >= AUG_BIAS_MIN_SIDE && hp <= AUG_MAX_SIDE,
                "aug_bias: the plane must be square with an even side of %d..%d (intensity_transform.py:439, :448), got %d x %d", AUG_BIAS_MIN_SIDE,
                AUG_MAX_SIDE, hp, wp);
    CTL_REQUIRE(image && bias, "aug_bias: image and bias (float [n,%d]) are required", AUG_BIAS_FLOATS);
    CTL_REQUIRE(noise || seeds, "aug_bias: neither a noise array nor per-sample seeds");
    CTL_REQUIRE(out, "aug_bias: no output image");
    CTL_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "aug_bias: the workspace must be a 256-byte aligned device buffer");
    CTL_REQUIRE(workspace_bytes >= aug_bias_bytes(n, hp, wp), "aug_bias: workspace of %zu bytes, ctl_aug_bias_ws_bytes asks for %zu", workspace_bytes,
                aug_bias_bytes(n, hp, wp));
    const size_t px = (size_t)n * hp * wp * sizeof(float);
    const aug_range r[] = {{out, px}, {workspace, aug_bias_bytes(n, hp, wp)}, {image, px}, {noise, px}, {bias, (size_t)n * AUG_BIAS_FLOATS * 4},
                           {seeds, (size_t)n * 8}};
    CTL_REQUIRE(!aug_any_overlap(r, 6, 2), "aug_bias: out and workspace must not overlap each other or an input");
    float* v = (float*)workspace;
    double* partial = (double*)((char*)workspace + aug_bias_plane_bytes(n, hp, wp));
    aug_bias_field_kernel<<<dim3(AUG_BPP, (unsigned)n), dim3(AUG_B), 0, S_>>>(image, bias, hp, v, partial);
    aug_bias_norm_kernel<<<dim3(AUG_BPP, (unsigned)n), dim3(AUG_B), 0, S_>>>(image, v, bias, partial, noise, seeds, hp * wp, out);
    ctl_count_launches(1);
    CTL_LAUNCH_CHECK("aug_bias");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ coarse-grid displacement
// MyElasticTransformCoarseGrid.gen_deformation_field (elastic_transform.py:121-137): two 3x3 planes resized to Hp x Wp by a cubic spline
// under the whole-sample symmetric extension c b | a b c | b a, clipped to the planes' own range.  The host hands over the prefiltered
// coefficients and the clip bounds; one launch, 4x4 taps per pixel in fp64, rounded once.
__device__ __forceinline__ int aug_mirror3(int i) {
    int m = i % 4;
    if (m < 0) m += 4;
    return m < 3 ? m : 4 - m;
}
__global__ __launch_bounds__(AUG_B) void aug_coarse_field_kernel(const float* __restrict__ coarse, int hp, int wp, float* __restrict__ field) {
    const int b = blockIdx.z, a = blockIdx.y;
    const float* rec = coarse + (int64_t)b * AUG_COARSE_FLOATS;
    const int i = (int)blockIdx.x * AUG_B + threadIdx.x;
    if (i >= hp * wp) return;
    float* fp = field + ((int64_t)b * 2 + a) * hp * wp;
    if (rec[22] == 0.f) { fp[i] = 0.f; return; }              // block-uniform
    const int r = i / wp, c = i - r * wp;
    const double sy = ((double)r + 0.5) * (3.0 / (double)hp) - 0.5, sx = ((double)c + 0.5) * (3.0 / (double)wp) - 0.5;
    const double fy = floor(sy), fx = floor(sx);
    double wy[4], wx[4];
    aug_bspline3(sy - fy, wy);
    aug_bspline3(sx - fx, wx);
    const float* cf = rec + a * 9;
    double val = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float* rp = cf + aug_mirror3((int)fy - 1 + t) * 3;
        double row = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) row += wx[u] * (double)rp[aug_mirror3((int)fx - 1 + u)];
        val += wy[t] * row;
    }
    fp[i] = (float)fmin(fmax(val, (double)rec[18 + a * 2]), (double)rec[19 + a * 2]);
}

extern "C" int ctl_aug_coarse_field(const float* coarse, int32_t n, int32_t hp, int32_t wp, float* field, ctl_stream stream) {
    CTL_REQUIRE(n > 0 && n <= 65535 && hp > 0 && wp > 0, "aug_coarse_field: n (1..65535), hp and wp must be positive (got %d, %d, %d)", n, hp, wp);
    CTL_REQUIRE(hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE, "aug_coarse_field: planes up to %d x %d (the limit of ctl_aug_warp), got %d x %d", AUG_MAX_SIDE,
                AUG_MAX_SIDE, hp, wp);
    CTL_REQUIRE(coarse, "aug_coarse_field: coarse (float [n,%d]) is required", AUG_COARSE_FLOATS);
    CTL_REQUIRE(field, "aug_coarse_field: no output field");
    const aug_range r[] = {{field, (size_t)n * 2 * hp * wp * sizeof(float)}, {coarse, (size_t)n * AUG_COARSE_FLOATS * 4}};
    CTL_REQUIRE(!aug_any_overlap(r, 2, 1), "aug_coarse_field: field must not overlap coarse");
    aug_coarse_field_kernel<<<dim3((unsigned)ctl_cdiv(hp * wp, AUG_B), 2, (unsigned)n), dim3(AUG_B), 0, S_>>>(coarse, hp, wp, field);
    CTL_LAUNCH_CHECK("aug_coarse_field");
    return CTL_OK;
}
