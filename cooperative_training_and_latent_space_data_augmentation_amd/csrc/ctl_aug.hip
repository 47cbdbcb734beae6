// Training augmentation of a whole batch on the device (medseg/dataset_loader/transform.py:46-86 runs it per slice on the host): flip,
// contrast / brightness, random affine, choice rotation, elastic deformation, centre crop -- ONE resampling of image and label.
// Gather and stencil work: no MFMA, no atomics, fixed launch counts, identical bits on every call.
//   ctl_aug_field   elastic displacement alpha * G_sigma(u) of every sample and both axes (elastic_transform.py:41-58): a row pass and a
//                   column pass, each from an LDS-staged line with the normalised weights of scipy's gaussian_filter
//   ctl_aug_warp    per-plane min / max partials, then one gather over the crop window: bilinear image taps through the intensity
//                   map (intensity_transform.py:136-162), nearest-neighbour label
// The contract of both is written out in include/ctl_hip.h.
#include "ctl_common.h"

#define AUG_B 256
#define AUG_MAX_SIDE 512          // LDS staging of one row / one column tile is sized for this
#define AUG_MAX_RADIUS 1024       // int(4 sigma + 0.5) is clamped here: twice the largest side, every tap beyond a side reads zeros anyway
#define AUG_COLS 16               // columns of one column-pass tile: 512 x 16 floats = 32 KiB of LDS
#define AUG_BPP 64                // min / max partial blocks per plane (the scheme of ctl_rescale_intensity)
#define AUG_TW 64                 // warp tile: 64 pixels along x (one wave per row: coalesced stores) x 4 rows
#define S_ (hipStream_t) stream

static inline size_t aug_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline bool aug_shape_ok(int n, int hp, int wp, int hc, int wc) {
    return n > 0 && n <= 65535 && hp > 0 && wp > 0 && hp <= AUG_MAX_SIDE && wp <= AUG_MAX_SIDE && hc > 0 && wc > 0 && hc <= hp && wc <= wp;
}
static inline size_t aug_tmp_bytes(int n, int hp, int wp) { return aug_align((size_t)n * 2 * hp * wp * sizeof(float)); }
static inline size_t aug_partial_bytes(int n) { return aug_align((size_t)n * AUG_BPP * 2 * sizeof(float)); }

extern "C" size_t ctl_aug_ws_bytes(int32_t n, int32_t hp, int32_t wp) { return aug_shape_ok(n, hp, wp, 1, 1) ? aug_tmp_bytes(n, hp, wp) : 0; }
extern "C" size_t ctl_aug_warp_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc) {
    return aug_shape_ok(n, hp, wp, hc, wc) ? aug_partial_bytes(n) : 0;
}

struct aug_range { const void* p; size_t bytes; };
// true when one of the `nw` written ranges at the front of r[] overlaps any other range of r[] (NULL ranges are skipped)
static bool aug_any_overlap(const aug_range* r, int count, int nw) {
    for (int i = 0; i < nw; ++i)
        for (int j = 0; j < count; ++j) {
            if (j == i || (j < nw && j < i) || !r[i].p || !r[j].p) continue;
            const uintptr_t a = (uintptr_t)r[i].p, b = (uintptr_t)r[j].p;
            if (a < b + r[j].bytes && b < a + r[i].bytes) return true;
        }
    return false;
}

// ------------------------------------------------------------------------------------------------ elastic displacement
__device__ __forceinline__ uint64_t aug_mix(uint64_t z) {      // splitmix64 finaliser, the generator of ctl_io.hip / ctl_mask.hip
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform in [-1, 1) on a 2^-23 grid from (seed, sample * 2 + axis, pixel): stateless, the same value whatever the launch geometry
__device__ __forceinline__ float aug_uniform(uint64_t seed, int plane, int pixel) {
    const uint64_t h = aug_mix(seed ^ aug_mix(((uint64_t)(uint32_t)plane << 32) | (uint32_t)pixel));
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
__device__ __forceinline__ void aug_block_minmax(float& mn, float& mx, float* sm) {
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wv * 2] = mn; sm[wv * 2 + 1] = mx; }
    __syncthreads();
    mn = sm[0]; mx = sm[1];
    for (int i = 1; i < AUG_B / 64; ++i) { mn = fminf(mn, sm[i * 2]); mx = fmaxf(mx, sm[i * 2 + 1]); }
    __syncthreads();
}
__global__ __launch_bounds__(AUG_B) void aug_minmax_partial_kernel(const float* __restrict__ x, int plane_elems, float* __restrict__ partial) {
    __shared__ float sm[2 * AUG_B / 64];
    const float* xp = x + (int64_t)blockIdx.y * plane_elems;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = (int)blockIdx.x * AUG_B + threadIdx.x; i < plane_elems; i += AUG_BPP * AUG_B) {
        const float v = xp[i];
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    aug_block_minmax(mn, mx, sm);
    if (threadIdx.x == 0) { partial[((int64_t)blockIdx.y * AUG_BPP + blockIdx.x) * 2] = mn; partial[((int64_t)blockIdx.y * AUG_BPP + blockIdx.x) * 2 + 1] = mx; }
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
    aug_block_minmax(mn, mx, sm);                              // its barriers also publish prm[]
    const int x = (int)blockIdx.x * AUG_TW + (threadIdx.x & 63), y = (int)blockIdx.y * (AUG_B / AUG_TW) + (threadIdx.x >> 6);
    if (x >= wc || y >= hc) return;
    const int py = y + cy, px = x + cx;                        // inside the padded grid: cy + hc <= hp, cx + wc <= wp
    const int64_t plane = (int64_t)hp * wp;
    float qr = (float)py, qc = (float)px;
    if (field) {
        qr += field[(int64_t)b * 2 * plane + (int64_t)py * wp + px];
        qc += field[((int64_t)b * 2 + 1) * plane + (int64_t)py * wp + px];
    }
    const float cr = 0.5f * (float)(hp - 1), cc = 0.5f * (float)(wp - 1);
    qr -= cr; qc -= cc;
    float sr = prm[0] * qr + prm[1] * qc + prm[2] + cr;
    float sc = prm[3] * qr + prm[4] * qc + prm[5] + cc;
    // everything at or beyond one pixel outside the array is zero: clamping there changes no result and keeps the conversions defined
    sr = fminf(fmaxf(sr, -2.f), (float)hp + 1.f);
    sc = fminf(fmaxf(sc, -2.f), (float)wp + 1.f);
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
