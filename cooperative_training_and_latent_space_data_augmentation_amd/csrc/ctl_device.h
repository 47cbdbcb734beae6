// Helpers shared by the feature kernels (every .hip file but the conv / weight-gradient families, which like the plan compiler need none
// of this and include ctl_common.h alone).  The kernels over channel rows of NHWC logits (ctl_loss, ctl_consist, ctl_recon, ctl_uncert,
// ctl_elem) include it through ctl_rows.h, which adds the row accessors, the block-row reduction steps and the launch sizing they share.
//   host    S_                       the launchers' stream argument as a hipStream_t
//           ctl_align256             workspace sections start on 256 bytes
//           ctl_blocks               1-D launch sizing: clamp(cdiv(items, threads), 1, cap)
//           ctl_vec4                 may the 16-byte row kernels be used?
//           ctl_overlap              do two device ranges intersect?
//   device  CTL_MIX_*, ctl_mix64     the counter-hash generator (splitmix64)
//           ctl_block_minmax<T>      min / max (float) over a block of T threads, every thread gets both
//           ctl_block_sum_double<W>  sum over a block of W waves, thread 0 gets it
//           ctl_wave_prefix_max / ctl_wave_suffix_min   inclusive integer scans over the 64 lanes of a wave (row passes of the distance transforms)
// (wave_sum_double, the wave step of the sums, is in ctl_common.h.)
#pragma once
#include "ctl_common.h"

#define S_ (hipStream_t) stream

static inline size_t ctl_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Blocks of `threads` items for `items` >= 1 items, at most `cap`: the grid-stride kernels cover the rest.  Several caps are the number
// of per-block partials of an ordered reduction and with it part of the result's bits: a call site never changes its cap.
static inline unsigned ctl_blocks(int64_t items, int64_t threads, int64_t cap) {
    const int64_t b = ctl_cdiv64(items, threads);
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// 16-byte rows (c == 4 floats per pixel) need 16-byte aligned tensors; unused pointer slots stay NULL
static inline bool ctl_vec4(int c, const void* a, const void* b = nullptr, const void* d = nullptr) {
    return c == 4 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)d) & 15) == 0;
}

// true when [a, a + a_bytes) and [b, b + b_bytes) intersect; a NULL range intersects nothing
static inline bool ctl_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + b_bytes && pb < pa + a_bytes;
}

// splitmix64: state increment and finaliser.  Every device random number is ctl_mix64 of a counter; test_rng_exact_gpu, test_io_exact_gpu,
// test_mask_exact_gpu and the goldens pin its bits.
#define CTL_MIX_GAMMA 0x9E3779B97F4A7C15ull
#define CTL_MIX_M1 0xBF58476D1CE4E5B9ull
#define CTL_MIX_M2 0x94D049BB133111EBull
__device__ __forceinline__ uint64_t ctl_mix64(uint64_t z) {
    z += CTL_MIX_GAMMA;
    z = (z ^ (z >> 30)) * CTL_MIX_M1;
    z = (z ^ (z >> 27)) * CTL_MIX_M2;
    return z ^ (z >> 31);
}

// every thread of a block of THREADS gets both; sm: 2 * THREADS / 64 floats.  Ends with a barrier (sm may be reused at once).
template <int THREADS> __device__ __forceinline__ void ctl_block_minmax(float& mn, float& mx, float* sm) {
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[w * 2] = mn; sm[w * 2 + 1] = mx; }
    __syncthreads();
    mn = sm[0]; mx = sm[1];
    for (int i = 1; i < THREADS / 64; ++i) { mn = fminf(mn, sm[i * 2]); mx = fmaxf(mx, sm[i * 2 + 1]); }
    __syncthreads();
}

// Sum over a block of WAVES waves, valid on thread 0; sm: one double per wave.  The order is fixed (lanes by the xor butterfly, then the
// waves in order) and pinned by the loss parity tests and the goldens.
template <int WAVES> __device__ __forceinline__ double ctl_block_sum_double(double v, double* sm) {
    v = wave_sum_double(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) for (int i = 0; i < WAVES; ++i) r += sm[i];
    return r;
}

// Inclusive scans over the 64 lanes of a wave: lane l gets max(v[0..l]) / min(v[l..63]).  Every lane of the wave must call them.
__device__ __forceinline__ int ctl_wave_prefix_max(int v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v = max(v, t);
    }
    return v;
}
__device__ __forceinline__ int ctl_wave_suffix_min(int v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_down(v, d);
        if (lane + d < 64) v = min(v, t);
    }
    return v;
}
