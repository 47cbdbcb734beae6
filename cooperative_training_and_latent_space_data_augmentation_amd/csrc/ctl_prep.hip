// Patient volume preparation on the device: what upstream does per volume on the host before a tensor reaches the network.
//   ctl_order_stats        exact order statistics of float32 segments: a most-significant-digit-first radix select over the
//                          order-preserving 32-bit key, four 8-bit passes with per-block LDS histograms, integer atomics only
//   ctl_percentile_apply   np.percentile (linear) formed from four order statistics in fp64, then the clip + scale of
//                          normalize_minmax_data (medseg/dataset_loader/dataset_utils.py:15-36) or of MyNormalizeMedicPercentile
//                          (medseg/dataset_loader/_utils/intensity_transform.py:216-269), one pass
//   ctl_resample_inplane   resample_by_spacing (dataset_utils.py:39-63) with keep_z_spacing: linear for the image, nearest for the label
// All of it is HBM-bound integer / element-wise work: no MFMA, no floating-point atomics, no readback, a launch sequence that depends
// on the shapes only.
#include "ctl_device.h"
#include <math.h>

#pragma clang fp contract(off)      // every multiply and add below rounds on its own (numpy / torch order), as in ctl_io.hip

#define PB 256
#define PREP_MAX_RANK 8
#define PREP_BPS 128                 // most blocks that share one segment (the pass-0 block histograms are sized for it)
#define PREP_EPB 4096                // elements per block aimed at
#define PREP_TENSOR_BYTES (1ll << 31)

struct prep_ranks { uint32_t k[PREP_MAX_RANK]; };

// ------------------------------------------------------------------------------------------------ radix select
// key order == float order (-0.0 before +0.0, negatives reversed); a NaN is just another key, which element it displaces is unspecified
__device__ __forceinline__ uint32_t prep_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float prep_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// exclusive prefix sum over the block's 256 bins (thread t holds bin t); s_w: 4 words of LDS
__device__ __forceinline__ uint32_t prep_excl_scan(uint32_t cnt, uint32_t* s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                       // the previous scan's readers are done with s_w
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (int i = 0; i < w; ++i) off += s_w[i];
    return off + inc - cnt;
}

// The digits the first `p` passes decided, for every rank: s_prefix[r] = the top 8p key bits of the wanted element, right-aligned.
// Every block re-derives them from the histograms the earlier launches left: pass 0 = the sum of the per-block histograms `bh`
// ([bps][256], the same for every rank), pass q >= 1 = hist[r][q - 1][256] (elements whose first q digits are the rank's).
// The remaining rank always lies inside the chosen bin, so exactly one thread selects per step.
__device__ __forceinline__ void prep_derive(const uint32_t* __restrict__ bh, int bps, const uint32_t* __restrict__ hist, int n_rank,
                                            const prep_ranks& rk, int p, uint32_t* s_prefix, uint32_t* s_w, uint32_t* s_sel) {
    const int t = threadIdx.x;
    if (t < 2) s_sel[t] = 0;
    uint32_t c0 = 0;
    for (int b = 0; b < bps; ++b) c0 += bh[b * 256 + t];
    const uint32_t e0 = prep_excl_scan(c0, s_w);
    for (int r = 0; r < n_rank; ++r) {
        uint32_t k = rk.k[r], prefix = 0;
        for (int q = 0; q < p; ++q) {
            uint32_t c = c0, e = e0;
            if (q) {
                c = hist[(r * 3 + q - 1) * 256 + t];
                e = prep_excl_scan(c, s_w);
            }
            __syncthreads();                               // the previous step's readers are done with s_sel
            if (c != 0 && k >= e && k - e < c) { s_sel[0] = (uint32_t)t; s_sel[1] = k - e; }
            __syncthreads();
            prefix = (prefix << 8) | s_sel[0];
            k = s_sel[1];
        }
        if (t == 0) s_prefix[r] = prefix;
    }
    __syncthreads();
}

// hist[digit] += 1 for the lanes with `pred`, aggregated inside the wave first: a volume that is mostly one background value would
// otherwise send the whole wave to one LDS bin.  Two rounds peel the digit of the first remaining lane (one add of the lane count by
// that lane), what is left adds per lane.  Must be called by the whole wave (uniform control flow); counts are integers, so the
// result does not depend on the path taken.
__device__ __forceinline__ void prep_wave_add(uint32_t* hist, uint32_t digit, bool pred) {
    const int lane = threadIdx.x & 63;
    uint64_t act = __ballot(pred);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (act == 0) break;
        const int leader = __ffsll((unsigned long long)act) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)digit, leader);
        const uint64_t same = __ballot(pred && digit == d0) & act;
        if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
        act &= ~same;
    }
    if ((act >> lane) & 1) atomicAdd(&hist[digit], 1u);
}

// pass p (0..3) over the elements: grid (bps, segments).  Pass 0 stores each block's histogram (plain stores, every word: the
// workspace needs no initialisation) and zeroes the global histograms of the later passes; pass p >= 1 counts digit p of the
// elements that carry a rank's prefix (ranks with equal prefixes share one LDS histogram) and adds to hist[r][p - 1].
__global__ __launch_bounds__(PB) void prep_select_pass_kernel(const float* __restrict__ x, int64_t seg_elems, int n_rank, prep_ranks rk,
                                                               int p, int bps, uint32_t* __restrict__ ws_bh, uint32_t* __restrict__ ws_hist) {
    __shared__ uint32_t sh[PREP_MAX_RANK * 256];
    __shared__ uint32_t s_prefix[PREP_MAX_RANK], s_up[PREP_MAX_RANK], s_rep[PREP_MAX_RANK], s_w[4], s_sel[2], s_nu;
    const int t = threadIdx.x;
    const int64_t seg = blockIdx.y;
    uint32_t* bh = ws_bh + seg * PREP_BPS * 256;
    uint32_t* hist = ws_hist + seg * n_rank * 3 * 256;
    int nu = 1;
    if (p == 0) {
        for (int i = blockIdx.x * PB + t; i < n_rank * 3 * 256; i += bps * PB) hist[i] = 0u;
    } else {
        prep_derive(bh, bps, hist, n_rank, rk, p, s_prefix, s_w, s_sel);
        if (t == 0) {
            int n = 0;
            for (int r = 0; r < n_rank; ++r) {
                int u = 0;
                while (u < n && s_up[u] != s_prefix[r]) ++u;
                if (u == n) s_up[n++] = s_prefix[r];
                s_rep[r] = (uint32_t)u;
            }
            s_nu = (uint32_t)n;
        }
        __syncthreads();
        nu = __builtin_amdgcn_readfirstlane((int)s_nu);
    }
    for (int i = t; i < nu * 256; i += PB) sh[i] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * p;
    const float* xs = x + seg * seg_elems;
    for (int64_t base = (int64_t)blockIdx.x * PB; base < seg_elems; base += (int64_t)bps * PB) {       // block-uniform trip count
        const int64_t i = base + t;
        const bool valid = i < seg_elems;
        const uint32_t key = valid ? prep_key(xs[i]) : 0u;
        const uint32_t digit = (key >> shift) & 255u;
        const uint32_t top = p ? (key >> (shift + 8)) : 0u;
        for (int u = 0; u < nu; ++u) prep_wave_add(sh + u * 256, digit, valid && (p == 0 || top == s_up[u]));
    }
    __syncthreads();
    if (p == 0) {
        bh[blockIdx.x * 256 + t] = sh[t];
    } else {
        for (int r = 0; r < n_rank; ++r) {
            const uint32_t c = sh[s_rep[r] * 256 + t];
            if (c) atomicAdd(&hist[(r * 3 + p - 1) * 256 + t], c);                                     // integer: order-independent
        }
    }
}

// after the four passes every key is known: grid (segments)
__global__ __launch_bounds__(PB) void prep_select_finish_kernel(int n_rank, prep_ranks rk, int bps, const uint32_t* __restrict__ ws_bh,
                                                                 const uint32_t* __restrict__ ws_hist, float* __restrict__ out) {
    __shared__ uint32_t s_prefix[PREP_MAX_RANK], s_w[4], s_sel[2];
    const int64_t seg = blockIdx.x;
    prep_derive(ws_bh + seg * PREP_BPS * 256, bps, ws_hist + seg * n_rank * 3 * 256, n_rank, rk, 4, s_prefix, s_w, s_sel);
    if ((int)threadIdx.x < n_rank) out[seg * n_rank + threadIdx.x] = prep_unkey(s_prefix[threadIdx.x]);
}

static inline bool prep_select_shape_ok(int32_t segments, int32_t n_rank) {
    return segments >= 1 && segments <= 65535 && n_rank >= 1 && n_rank <= PREP_MAX_RANK;
}

extern "C" size_t ctl_order_stats_ws_bytes(int32_t segments, int32_t n_rank) {
    if (!prep_select_shape_ok(segments, n_rank)) return 0;
    return (size_t)segments * 256 * (PREP_BPS + 3 * (size_t)n_rank) * sizeof(uint32_t);
}

extern "C" int ctl_order_stats(const float* x, int32_t segments, int64_t seg_elems, const int64_t* ranks, int32_t n_rank, float* out,
                               void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(x && ranks && out && workspace, "order_stats: null pointer (x, ranks, out and workspace are required)");
    CTL_REQUIRE(n_rank >= 1 && n_rank <= PREP_MAX_RANK, "order_stats: n_rank %d (1..%d ranks per call)", n_rank, PREP_MAX_RANK);
    CTL_REQUIRE(segments >= 1 && segments <= 65535 && seg_elems >= 1, "order_stats: %d segments of %lld elements (1..65535 segments, at least one element)",
                segments, (long long)seg_elems);
    CTL_REQUIRE(seg_elems < PREP_TENSOR_BYTES / 4 && (int64_t)segments * seg_elems * 4 < PREP_TENSOR_BYTES,
                "order_stats: %d x %lld floats reach the 2 GiB tensor limit (32-bit byte offsets)", segments, (long long)seg_elems);
    prep_ranks rk = {};
    for (int r = 0; r < n_rank; ++r) {
        CTL_REQUIRE(ranks[r] >= 0 && ranks[r] < seg_elems, "order_stats: rank %lld (entry %d) outside [0, %lld)", (long long)ranks[r], r,
                    (long long)seg_elems);
        rk.k[r] = (uint32_t)ranks[r];
    }
    const size_t need = ctl_order_stats_ws_bytes(segments, n_rank);
    CTL_REQUIRE(workspace_bytes >= need, "order_stats: workspace of %zu bytes, %zu needed (ctl_order_stats_ws_bytes)", workspace_bytes, need);
    CTL_REQUIRE(((uintptr_t)workspace & 3) == 0, "order_stats: the workspace must be 4-byte aligned");
    uint32_t* bh = (uint32_t*)workspace;
    uint32_t* hist = bh + (size_t)segments * PREP_BPS * 256;
    const int bps = (int)ctl_blocks(seg_elems, PREP_EPB, PREP_BPS);
    const dim3 grid((unsigned)bps, (unsigned)segments), blk(PB);
    for (int p = 0; p < 4; ++p) prep_select_pass_kernel<<<grid, blk, 0, S_>>>(x, seg_elems, n_rank, rk, p, bps, bh, hist);
    prep_select_finish_kernel<<<dim3((unsigned)segments), blk, 0, S_>>>(n_rank, rk, bps, bh, hist, out);
    ctl_count_launches(4);                                     // five kernels, CTL_LAUNCH_CHECK counts one
    CTL_LAUNCH_CHECK("order_stats");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ percentile + normalise
// numpy's _lerp (lib/_function_base_impl.py) on two neighbouring order statistics, in fp64, rounded once to float32
__device__ __forceinline__ float prep_lerp(float a, float b, double g) {
    const double A = (double)a, B = (double)b;
    const double d = B - A;
    const double v = g < 0.5 ? A + d * g : B - d * (1.0 - g);
    return (float)v;
}

// grid (blocks, segments); table [segments][4] = the elements of rank k_lo, k_lo + 1, k_hi, k_hi + 1 (upper ranks clamped)
__global__ __launch_bounds__(PB) void prep_percentile_apply_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                                    int64_t seg_elems, double g_lo, double g_hi, int form, float new_min,
                                                                    float new_max, float* __restrict__ out, float* __restrict__ bounds) {
    const int64_t seg = blockIdx.y;
    const float* tb = table + seg * 4;
    const float lo = prep_lerp(tb[0], tb[1], g_lo), hi = prep_lerp(tb[2], tb[3], g_hi);
    if (bounds && blockIdx.x == 0 && threadIdx.x == 0) { bounds[seg * 2] = lo; bounds[seg * 2 + 1] = hi; }
    if (!out) return;                                      // percentiles only
    const float* xs = x + seg * seg_elems;
    float* os = out + seg * seg_elems;
    const int64_t stride = (int64_t)gridDim.x * PB;
    if (form == 0) {                                       // normalize_minmax_data: strict comparisons, (x - lo) / ((1e-10 + hi) - lo)
        const float den = (1e-10f + hi) - lo;
        for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < seg_elems; i += stride) {
            float v = xs[i];
            if (v < lo) v = lo;
            if (v > hi) v = hi;
            os[i] = (v - lo) / den;
        }
    } else {                                               // MyNormalizeMedicPercentile: le / ge, a = range / ((hi - lo) + 1e-8), b = new_max - a hi
        const float a = (new_max - new_min) / ((hi - lo) + 1e-8f);
        const float b = new_max - a * hi;
        for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < seg_elems; i += stride) {
            float v = xs[i];
            if (v <= lo) v = lo;
            if (v >= hi) v = hi;
            const float m = v * a;
            os[i] = m + b;
        }
    }
}

extern "C" int ctl_percentile_apply(const float* x, const float* table, int32_t segments, int64_t seg_elems, double g_lo, double g_hi,
                                    int32_t form, float new_min, float new_max, float* out, float* bounds, ctl_stream stream) {
    CTL_REQUIRE(x && table && (out || bounds), "percentile_apply: null pointer (x, table and one of out / bounds are required)");
    CTL_REQUIRE(segments >= 1 && segments <= 65535 && seg_elems >= 1, "percentile_apply: %d segments of %lld elements (1..65535 segments, at least one element)",
                segments, (long long)seg_elems);
    CTL_REQUIRE(seg_elems < PREP_TENSOR_BYTES / 4 && (int64_t)segments * seg_elems * 4 < PREP_TENSOR_BYTES,
                "percentile_apply: %d x %lld floats reach the 2 GiB tensor limit (32-bit byte offsets)", segments, (long long)seg_elems);
    CTL_REQUIRE(form == 0 || form == 1, "percentile_apply: form %d (0 = minmax, 1 = medic)", form);
    CTL_REQUIRE(g_lo >= 0.0 && g_lo < 1.0 && g_hi >= 0.0 && g_hi < 1.0, "percentile_apply: weights %g, %g outside [0, 1)", g_lo, g_hi);
    const int64_t total = (int64_t)segments * seg_elems;
    CTL_REQUIRE(!ctl_overlap(x, (size_t)total * 4, out, (size_t)total * 4), "percentile_apply: out aliases x (a separate output array is required)");
    const unsigned b = out ? ctl_blocks(seg_elems, PB * 4, 256) : 1;
    prep_percentile_apply_kernel<<<dim3(b, (unsigned)segments), dim3(PB), 0, S_>>>(x, table, seg_elems, g_lo, g_hi, form, new_min,
                                                                                    new_max, out, bounds);
    CTL_LAUNCH_CHECK("percentile_apply");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ in-plane resample
// Output index j reads source coordinate c = j * r (one fp64 multiply); the value is 0 where c >= size - 0.5 on either axis.
__global__ __launch_bounds__(PB) void prep_resample_image_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int h, int w,
                                                                  int nh, int nw, double rh, double rw) {
    const int64_t total = (int64_t)n * nh * nw;
    const int64_t stride = (int64_t)gridDim.x * PB;
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < total; i += stride) {
        const int jx = (int)(i % nw);
        const int64_t q = i / nw;
        const int jy = (int)(q % nh);
        const int64_t b = q / nh;
        const double cy = (double)jy * rh, cx = (double)jx * rw;
        float v = 0.f;
        if (cy < (double)h - 0.5 && cx < (double)w - 0.5) {
            const double fy = floor(cy), fx = floor(cx);
            const double ty = cy - fy, tx = cx - fx;
            int y0 = (int)fy, x0 = (int)fx;
            y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0);
            x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0);
            const int y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1, x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1;
            const float* p = src + b * h * w;
            const double v00 = p[(int64_t)y0 * w + x0], v01 = p[(int64_t)y0 * w + x1];
            const double v10 = p[(int64_t)y1 * w + x0], v11 = p[(int64_t)y1 * w + x1];
            const double top = v00 * (1.0 - tx) + v01 * tx;
            const double bot = v10 * (1.0 - tx) + v11 * tx;
            v = (float)(top * (1.0 - ty) + bot * ty);
        }
        dst[i] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(PB) void prep_resample_label_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int h, int w, int nh,
                                                                  int nw, double rh, double rw) {
    const int64_t total = (int64_t)n * nh * nw;
    const int64_t stride = (int64_t)gridDim.x * PB;
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < total; i += stride) {
        const int jx = (int)(i % nw);
        const int64_t q = i / nw;
        const int jy = (int)(q % nh);
        const int64_t b = q / nh;
        const double cy = (double)jy * rh, cx = (double)jx * rw;
        T v = (T)0;
        if (cy < (double)h - 0.5 && cx < (double)w - 0.5) {
            int y = (int)floor(cy + 0.5), x_ = (int)floor(cx + 0.5);
            y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
            x_ = x_ < 0 ? 0 : (x_ > w - 1 ? w - 1 : x_);
            v = src[(b * h + y) * w + x_];
        }
        dst[i] = v;
    }
}

extern "C" int ctl_resample_inplane(const float* image, const void* label, int32_t label_bytes, int32_t n, int32_t h, int32_t w,
                                    int32_t new_h, int32_t new_w, double r_h, double r_w, float* image_out, void* label_out,
                                    ctl_stream stream) {
    CTL_REQUIRE(image || label, "resample_inplane: null pointer (an image or a label is required)");
    CTL_REQUIRE((!image || image_out) && (!label || label_out), "resample_inplane: null pointer (every input needs its output array)");
    CTL_REQUIRE(n > 0 && h > 0 && w > 0 && new_h > 0 && new_w > 0, "resample_inplane: sizes must be positive (n %d, %d x %d -> %d x %d)", n, h, w,
                new_h, new_w);
    CTL_REQUIRE(r_h > 0.0 && r_w > 0.0 && isfinite(r_h) && isfinite(r_w), "resample_inplane: spacing ratios %g, %g must be positive and finite",
                r_h, r_w);
    CTL_REQUIRE(!label || label_bytes == 1 || label_bytes == 8, "resample_inplane: label element size %d (1 = uint8, 8 = int64)", label_bytes);
    const int64_t eb = label && label_bytes == 8 ? 8 : 4;
    CTL_REQUIRE((int64_t)n * h * w * eb < PREP_TENSOR_BYTES && (int64_t)n * new_h * new_w * eb < PREP_TENSOR_BYTES,
                "resample_inplane: %d x %d x %d -> %d x %d reaches the 2 GiB tensor limit (32-bit byte offsets)", n, h, w, new_h, new_w);
    int64_t blocks = ctl_cdiv64((int64_t)n * new_h * new_w, PB);
    blocks = blocks > 2048 ? 2048 : blocks;
    const dim3 grid((unsigned)blocks), blk(PB);
    if (image) prep_resample_image_kernel<<<grid, blk, 0, S_>>>(image, image_out, n, h, w, new_h, new_w, r_h, r_w);
    if (label) {
        if (label_bytes == 1) prep_resample_label_kernel<uint8_t><<<grid, blk, 0, S_>>>((const uint8_t*)label, (uint8_t*)label_out, n, h, w, new_h, new_w, r_h, r_w);
        else prep_resample_label_kernel<int64_t><<<grid, blk, 0, S_>>>((const int64_t*)label, (int64_t*)label_out, n, h, w, new_h, new_w, r_h, r_w);
    }
    if (image && label) ctl_count_launches(1);                 // two kernels, CTL_LAUNCH_CHECK counts one
    CTL_LAUNCH_CHECK("resample_inplane");
    return CTL_OK;
}
