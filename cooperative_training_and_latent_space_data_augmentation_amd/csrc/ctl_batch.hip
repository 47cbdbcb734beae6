// Device-resident training set: the batch that upstream's per-slice Dataset assembles on the host, gathered by an index list.
//   ctl_slice_foreground   non-zero raw label voxels per slice (the "slice without objects" test, cardiac_ACDC_dataset.py:141-149)
//   ctl_batch_gather       formulate_labels + PadNumpy onto the common canvas (base_segmentation_dataset.py:190-202, transform.py:46-97)
//                          and the origin_image / origin_label pair (base_segmentation_dataset.py:149-186), one launch per batch
// Copies and byte look-ups only: bandwidth-bound, no floating-point arithmetic, no atomics, no readback.  The slice geometry is a
// function of blockIdx alone (index[b], then one table row), so it is fetched once per block through the scalar cache; source rows are
// read at whatever element offset the slice has, output rows are stored as 16-byte vectors wherever the address allows.
#include "ctl_device.h"

#define BB 256
#define BATCH_MAX_SIDE 32768
#define BATCH_MAX_BLOCKS_X 64         // blocks that share one output plane (each strides over the plane's groups of four elements)

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ foreground count
__global__ __launch_bounds__(BB) void slice_foreground_kernel(const uint8_t* __restrict__ label, const int64_t* __restrict__ table,
                                                              int64_t arena_elems, int32_t* __restrict__ counts) {
    __shared__ int s_part[BB / 64];
    const int64_t s = blockIdx.x;
    const int64_t off = table[3 * s], h = table[3 * s + 1], w = table[3 * s + 2];
    int64_t count = 0;
    if (off >= 0 && h > 0 && w > 0 && h <= BATCH_MAX_SIDE && w <= BATCH_MAX_SIDE && off + h * w <= arena_elems) count = h * w;
    const uint8_t* p = label + off;
    int c = 0;
    for (int64_t i = threadIdx.x; i < count; i += BB) c += p[i] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < BB / 64; ++k) t += s_part[k];
        counts[s] = t;
    }
}

extern "C" int ctl_slice_foreground(const uint8_t* label, const int64_t* table, int32_t n_slices, int64_t arena_elems, int32_t* counts,
                                    ctl_stream stream) {
    CTL_REQUIRE(label && table && counts, "slice_foreground: null pointer");
    CTL_REQUIRE(n_slices >= 1 && arena_elems >= 1, "slice_foreground: %d slices in an arena of %lld elements (at least one of each)", n_slices,
                (long long)arena_elems);
    slice_foreground_kernel<<<dim3((unsigned)n_slices), dim3(BB), 0, S_>>>(label, table, arena_elems, counts);
    CTL_LAUNCH_CHECK("slice_foreground");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ gather
// crop_or_pad per axis: target index t reads source index t + d, d = (a - A) / 2 for a >= A, -ceil((A - a) / 2) for a < A
__device__ __forceinline__ int batch_shift(int a, int A) { return a >= A ? (a - A) / 2 : -((A - a + 1) / 2); }

template <typename T> struct batch_vec;
template <> struct batch_vec<float> {
    static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct batch_vec<int64_t> {
    static __device__ __forceinline__ void store(int64_t* p, const int64_t* v) {
        reinterpret_cast<i64x2*>(p)[0] = i64x2{v[0], v[1]};
        reinterpret_cast<i64x2*>(p)[1] = i64x2{v[2], v[3]};
    }
};

// One [H][W] plane of TO at dst from the [h][w] slice of TS at src (h == 0: all zeros).  Groups of four elements, cut so that a whole
// group starts on a 16-byte boundary: group k covers plane elements [4 k - lead, 4 k - lead + 4).
template <typename TO, typename TS, bool MAP>
__device__ __forceinline__ void batch_place(TO* __restrict__ dst, int H, int W, const TS* __restrict__ src, int h, int w,
                                            const uint8_t* s_lut) {
    const int total = H * W;
    const int lead = (int)((reinterpret_cast<uintptr_t>(dst) / sizeof(TO)) & (16 / sizeof(TO) - 1));
    const int groups = (total + lead + 3) >> 2;
    const int dy = batch_shift(h, H), dx = batch_shift(w, W);
    for (int k = blockIdx.x * BB + threadIdx.x; k < groups; k += gridDim.x * BB) {
        const int e0 = 4 * k - lead;
        const int first = e0 < 0 ? 0 : e0;
        int y = first / W, x = first - y * W;
        TO v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + j;
            TO val = (TO)0;
            if (e >= 0 && e < total) {
                const int sy = y + dy, sx = x + dx;
                if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
                    const TS r = src[(int64_t)sy * w + sx];
                    val = MAP ? (TO)s_lut[(uint8_t)r] : (TO)r;
                }
                if (++x == W) { x = 0; ++y; }
            }
            v[j] = val;
        }
        if (e0 >= 0 && e0 + 4 <= total) {
            batch_vec<TO>::store(dst + e0, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j >= 0 && e0 + j < total) dst[e0 + j] = v[j];
        }
    }
}

// grid (blocks per plane, n, 2 or 4): z = 0 canvas image, 1 canvas label, 2 original image, 3 original label
__global__ __launch_bounds__(BB) void batch_gather_kernel(const float* __restrict__ image, const uint8_t* __restrict__ label,
                                                          const int64_t* __restrict__ table, int n_slices, int64_t arena_elems,
                                                          const int32_t* __restrict__ index, const uint8_t* __restrict__ lut, int H, int W,
                                                          float* __restrict__ image_out, int64_t* __restrict__ label_out, int Hc, int Wc,
                                                          float* __restrict__ orig_image, int64_t* __restrict__ orig_label) {
    __shared__ uint8_t s_lut[256];
    const int b = blockIdx.y, which = blockIdx.z;
    if (which & 1) {
        s_lut[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    const int s = index[b];
    int64_t off = 0;
    int h = 0, w = 0;
    if (s >= 0 && s < n_slices) {
        const int64_t o = table[3 * (int64_t)s], hh = table[3 * (int64_t)s + 1], ww = table[3 * (int64_t)s + 2];
        if (o >= 0 && hh > 0 && ww > 0 && hh <= BATCH_MAX_SIDE && ww <= BATCH_MAX_SIDE && o + hh * ww <= arena_elems) {
            off = o; h = (int)hh; w = (int)ww;
        }
    }
    if (which == 0) batch_place<float, float, false>(image_out + (int64_t)b * H * W, H, W, image + off, h, w, s_lut);
    else if (which == 1) batch_place<int64_t, uint8_t, true>(label_out + (int64_t)b * H * W, H, W, label + off, h, w, s_lut);
    else if (which == 2) batch_place<float, float, false>(orig_image + (int64_t)b * Hc * Wc, Hc, Wc, image + off, h, w, s_lut);
    else batch_place<int64_t, uint8_t, true>(orig_label + (int64_t)b * Hc * Wc, Hc, Wc, label + off, h, w, s_lut);
}

extern "C" int ctl_batch_gather(const float* image, const uint8_t* label, const int64_t* table, int32_t n_slices, int64_t arena_elems,
                                const int32_t* index, int32_t n, const uint8_t* lut, int32_t H, int32_t W, float* image_out,
                                int64_t* label_out, int32_t Hc, int32_t Wc, float* orig_image, int64_t* orig_label, ctl_stream stream) {
    CTL_REQUIRE(image && label && table && index && lut && image_out && label_out, "batch_gather: null pointer");
    CTL_REQUIRE((orig_image != nullptr) == (orig_label != nullptr), "batch_gather: the original pair is both orig_image and orig_label, or neither");
    CTL_REQUIRE(n_slices >= 1 && arena_elems >= 1, "batch_gather: %d slices in an arena of %lld elements (at least one of each)", n_slices,
                (long long)arena_elems);
    CTL_REQUIRE(n >= 1 && n <= 65535, "batch_gather: batch of %d samples (1..65535)", n);
    CTL_REQUIRE(H >= 1 && W >= 1 && H <= BATCH_MAX_SIDE && W <= BATCH_MAX_SIDE, "batch_gather: canvas %d x %d (sides 1..%d)", H, W, BATCH_MAX_SIDE);
    CTL_REQUIRE(!orig_image || (Hc >= 1 && Wc >= 1 && Hc <= BATCH_MAX_SIDE && Wc <= BATCH_MAX_SIDE), "batch_gather: crop %d x %d (sides 1..%d)", Hc,
                Wc, BATCH_MAX_SIDE);
    CTL_REQUIRE(reinterpret_cast<uintptr_t>(image_out) % 4 == 0 && reinterpret_cast<uintptr_t>(orig_image) % 4 == 0 &&
                reinterpret_cast<uintptr_t>(label_out) % 8 == 0 && reinterpret_cast<uintptr_t>(orig_label) % 8 == 0,
                "batch_gather: an output is not aligned to its element size");
    int64_t plane = (int64_t)H * W;
    if (orig_image && (int64_t)Hc * Wc > plane) plane = (int64_t)Hc * Wc;
    int64_t bx = ctl_cdiv64(ctl_cdiv64(plane + 3, 4), BB);
    bx = bx > BATCH_MAX_BLOCKS_X ? BATCH_MAX_BLOCKS_X : bx;
    batch_gather_kernel<<<dim3((unsigned)bx, (unsigned)n, orig_image ? 4u : 2u), dim3(BB), 0, S_>>>(
        image, label, table, n_slices, arena_elems, index, lut, H, W, image_out, label_out, Hc, Wc, orig_image, orig_label);
    CTL_LAUNCH_CHECK("batch_gather");
    return CTL_OK;
}
