// Helpers shared by the kernels that hold a pixel's channel row of an fp32 NHWC tensor in registers and leave ordered fp64 block rows
// (ctl_loss, ctl_consist, ctl_recon, ctl_uncert; ctl_elem takes the constants and the dispatch only, see its row_load).  A kernel built
// on them compiles to what it is with the statements written out: the row functions are __forceinline__, the two reduction steps are
// macros because as inlined functions the same statements came out as other (equivalent) block layouts and schedules.
//   both    CTL_ROW_MAXC             channel rows have at most 16 entries (losses.MAX_CLASSES restates it in Python)
//           CTL_ROW_THREADS          threads per block of every row kernel
//   device  ctl_row_load / ctl_row_store<CT>   one pixel's row: CT = 4 one 16-byte access, CT = 1 one float, CT = 0 runtime channel count
//           ctl_row_exp<CT>          v <- exp(v - max v), the sum of the exponentials; returns the maximum
//           CTL_BLOCK_ROWS_STORE     the tail of a partial kernel: the waves' LDS rows added in index order, one row written
//           CTL_GROUP16_SUM, _SUM3   xor butterfly over a group of 16 lanes, on one value or on three side by side
//   host    CTL_ROW_DISPATCH, _LDS, _C1         launch the <4> or the <0> (or, for c == 1, the <1>) instantiation of a row kernel
//           ctl_sample_blocks / ctl_tile_blocks  blocks per sample of a (blocks, sample) grid / blocks of a grid-stride pass over tiles
//           ctl_kind_weights         the weight of each selected kind of a loss set, 0 for the others
//           ctl_class_weights_norm   w / sum(w) * c
//           ctl_check_channels / ctl_check_batch / ctl_check_2gib   the extent checks, message texts included
#pragma once
#include <cmath>
#include "ctl_device.h"

#define CTL_ROW_MAXC 16
#define CTL_ROW_THREADS 256

// Channel rows.  CT = 4: one 16-byte load / store per pixel; CT = 1: one float per pixel; CT = 0: runtime channel count, the loops still
// unrolled over CTL_ROW_MAXC with the tail switched off (everything stays in registers).  The arithmetic and its order are the same in
// all three; the kernels keep contraction off so that no form turns a product and a sum into an fma another one keeps apart.
template <int CT> __device__ __forceinline__ void ctl_row_load(const float* __restrict__ base, int64_t i, int c, float* v) {
    if (CT == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(base + i * 4);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if (CT == 1) {
        v[0] = base[i];
    } else {
#pragma unroll
        for (int k = 0; k < CTL_ROW_MAXC; ++k) if (k < c) v[k] = base[i * c + k];
    }
}
template <int CT> __device__ __forceinline__ void ctl_row_store(float* __restrict__ base, int64_t i, int c, const float* v) {
    if (CT == 4) {
        *reinterpret_cast<f32x4*>(base + i * 4) = f32x4{v[0], v[1], v[2], v[3]};
    } else if (CT == 1) {
        base[i] = v[0];
    } else {
#pragma unroll
        for (int k = 0; k < CTL_ROW_MAXC; ++k) if (k < c) base[i * c + k] = v[k];
    }
}
// v <- exp(v - max v), fp32; returns the row maximum, `s` = the sum of the exponentials in index order.  What a caller makes of them
// (multiply by 1 / s, divide by s, log s in fp32 or fp64) is part of its result's bits and stays with the caller.
template <int CT> __device__ __forceinline__ float ctl_row_exp(float* v, int c, float& s) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) m = fmaxf(m, v[k]);
    s = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) { v[k] = expf(v[k] - m); s += v[k]; }
    return m;
}

// The tail of a partial kernel whose wave leaders have left their sums in sm[wave][0 .. nv): thread j < nv adds the waves' entries j in
// index order and writes dst[j].  Every thread of the block takes it (a barrier comes first).
#define CTL_BLOCK_ROWS_STORE(sm, waves, nv, dst)                                          \
    do {                                                                                 \
        __syncthreads();                                                                 \
        if ((int)threadIdx.x < (nv)) {                                                   \
            double a__ = 0.0;                                                            \
            for (int i__ = 0; i__ < (waves); ++i__) a__ += (sm)[i__][threadIdx.x];       \
            (dst)[threadIdx.x] = a__;                                                    \
        }                                                                                \
    } while (0)

// Sum over each aligned group of 16 lanes, every lane gets it; _SUM3 takes three values through the butterfly side by side, step by step
#define CTL_GROUP16_SUM(v) for (int o__ = 8; o__ > 0; o__ >>= 1) (v) += __shfl_xor((v), o__)
#define CTL_GROUP16_SUM3(a, b, d) \
    for (int o__ = 8; o__ > 0; o__ >>= 1) { (a) += __shfl_xor((a), o__); (b) += __shfl_xor((b), o__); (d) += __shfl_xor((d), o__); }

// The <4> (16-byte rows, see ctl_vec4) or the <0> instantiation of a row kernel; _LDS with a dynamic LDS size; _C1 with the <1> form
// for single-channel tensors in front.
#define CTL_ROW_DISPATCH_LDS(kernel, vec4, grid, lds, ...)                                       \
    do {                                                                                         \
        if (vec4) kernel<4><<<grid, dim3(CTL_ROW_THREADS), lds, S_>>>(__VA_ARGS__);              \
        else kernel<0><<<grid, dim3(CTL_ROW_THREADS), lds, S_>>>(__VA_ARGS__);                   \
    } while (0)
#define CTL_ROW_DISPATCH(kernel, vec4, grid, ...) CTL_ROW_DISPATCH_LDS(kernel, vec4, grid, 0, __VA_ARGS__)
#define CTL_ROW_DISPATCH_C1(kernel, c, vec4, grid, lds, ...)                                     \
    do {                                                                                         \
        if ((c) == 1) kernel<1><<<grid, dim3(CTL_ROW_THREADS), lds, S_>>>(__VA_ARGS__);          \
        else CTL_ROW_DISPATCH_LDS(kernel, vec4, grid, lds, __VA_ARGS__);                         \
    } while (0)

// Blocks per sample of a (blocks, sample) grid: at most `cap` blocks over all samples, one per sample where b exceeds the cap.  Where
// the blocks leave partial rows the cap is part of the result's bits (see ctl_blocks).
static inline int ctl_sample_blocks(int64_t b, int64_t hw, int threads, int cap) {
    int64_t nb = ctl_cdiv64(hw, threads), lim = cap / b;
    if (lim < 1) lim = 1;
    return (int)(nb < lim ? nb : lim);
}
// Blocks of a grid-stride pass over the tile x tile pixel tiles of b planes
static inline int ctl_tile_blocks(int64_t b, int h, int w, int tile, int cap) {
    const int64_t n = b * ctl_cdiv(h, tile) * ctl_cdiv(w, tile);
    return (int)(n < cap ? n : cap);
}

// out[t] = weights[t] where bit t of `kinds` is set (it must be finite), else 0
static int ctl_kind_weights(const char* who, int kinds, int nk, const double* weights, double* out) {
    CTL_REQUIRE(weights, "%s: null pointer (weights: one double per kind)", who);
    for (int t = 0; t < nk; ++t) {
        const bool on = (kinds >> t) & 1;
        CTL_REQUIRE(!on || std::isfinite(weights[t]), "%s: the weight of kind %d is %g (finite)", who, t, weights[t]);
        out[t] = on ? weights[t] : 0.0;
    }
    return CTL_OK;
}
// out[k] = w_k / sum(w) * c for k < c in fp64 (custom_loss.py:733-734); the entries from c on are left alone
static int ctl_class_weights_norm(const char* who, int c, const double* class_weights, double* out) {
    double sum = 0.0;
    for (int k = 0; k < c; ++k) sum += class_weights[k];
    CTL_REQUIRE(std::isfinite(sum) && sum > 0.0, "%s: the class weights sum to %g (a finite, positive sum is needed)", who, sum);
    for (int k = 0; k < c; ++k) out[k] = class_weights[k] / sum * (double)c;
    return CTL_OK;
}

// The extent checks of the row kernels' entries, in the steps their entries take them (a kind's own check may stand between two, and the
// first failure is the one reported).  `noun`: "classes" or "channels".
static int ctl_check_channels(const char* who, int c, const char* noun) {
    CTL_REQUIRE(c >= 1 && c <= CTL_ROW_MAXC, "%s: %d %s (1 .. %d)", who, c, noun, CTL_ROW_MAXC);
    return CTL_OK;
}
// the sample is the grid's y
static int ctl_check_batch(const char* who, int64_t b) {
    CTL_REQUIRE(b <= 65535, "%s: batch %lld (at most 65535 samples)", who, (long long)b);
    return CTL_OK;
}
// a tensor of c floats per pixel stays below 2^31 bytes
static int ctl_check_2gib(const char* who, int64_t b, int64_t h, int64_t w, int c, const char* noun) {
    CTL_REQUIRE(h * w < ((int64_t)1 << 31) && b * h * w < ((int64_t)1 << 31) / (c * 4),
                "%s: %lld x %lld x %lld pixels of %d %s reach the 2 GiB tensor limit", who, (long long)b, (long long)h, (long long)w, c, noun);
    return CTL_OK;
}
