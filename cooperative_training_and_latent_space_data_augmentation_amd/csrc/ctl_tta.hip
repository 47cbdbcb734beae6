// Test-time augmentation (include/ctl_hip.h, "test-time augmentation"): the D4 views of a batch of slices, and the merge of the network's
// logits on those views back on the native grid (aligned members, their logit or probability mean, its arg-max).  A project addition:
// upstream has no counterpart.  Both entries are one launch over square pixel tiles; both are the same data movement,
//     dst[r][s] = src[y][x],   (a, b) = tr ? (s, r) : (r, s),   y = fa ? Hs - 1 - a : a,   x = fb ? Ws - 1 - b : b,
// with (tr, fa, fb) the three bits of a view code for the merge (dst = native grid, src = the view) and, for the views (dst = the view,
// src = the native grid), the same bits with the two flips exchanged when the code transposes (the flips act on the view's axes, which
// a transpose exchanges; a transposing code needs a square plane, so Hs = Ws there).
// A pixel is c contiguous floats.  Without a transpose a row of the tile is a run of src pixels, forwards or backwards, and is read
// straight from global memory.  With one, a tile row would read one pixel per src row: the tile is first read along the src rows into
// LDS (rows padded by one access: 16 bytes for the 16-byte form, 4 bytes otherwise, so the column read meets every bank once) and each
// thread then takes its pixel from there.  No arithmetic touches a copied value; the means are ordered sums in registers.  No
// workspace, no atomics, nothing read back, no argument that changes from call to call.
#include <cmath>
#include "ctl_device.h"

#define TB 256                    // threads per block
#define TTA_LDS_FLOATS 4224       // 32 rows of 32 * 4 + 4 floats; the 16 x 16 tile of 16 channels needs 16 * (256 + 1)

#ifndef CTL_TTA_STRIDED
#define CTL_TTA_STRIDED 0         // experiment hook (tools/bench_tta.py): 1 = a transposed view is read one pixel per src row, no LDS tile
#endif

struct tta_codes { int v[CTL_TTA_MAX_VIEWS]; };

// One member's tile.  TS x TS pixels, thread (ly, lx) = (tid / TS, tid % TS) owns the pixels (ly + r * TB / TS, lx), r < TS * TS / TB:
// lanes run along a dst row.  VEC: c == 4 in 16-byte aligned tensors, a pixel moves as 16 bytes.  NC: the row's register count.
// src: the slice's plane [Hs][Ws][c]; (r0, s0): the tile's origin in dst, (hd, wd): dst extent.  Every thread of the block calls this
// (barriers inside when tr), whether or not its pixels are inside the plane; v of an outside pixel is left alone.
template <int TS, int NC, bool VEC>
__device__ __forceinline__ void tta_fetch(const float* __restrict__ src, int tr, int fa, int fb, int hs, int ws, int c, int r0, int s0, int hd,
                                          int wd, float* __restrict__ lds, float (*v)[NC]) {
    constexpr int PPT = TS * TS / TB, ROWS = TB / TS;
    const int lx = threadIdx.x % TS, ly = threadIdx.x / TS;
    if (!tr || CTL_TTA_STRIDED) {
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            const int r = r0 + ly + p * ROWS, s = s0 + lx;
            if (r < hd && s < wd) {
                const int a = tr ? s : r, b = tr ? r : s;
                const int y = fa ? hs - 1 - a : a, x = fb ? ws - 1 - b : b;
                const int64_t at = (int64_t)y * ws + x;
                if (VEC) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(src + at * 4);
                    v[p][0] = t.x; v[p][1] = t.y; v[p][2] = t.z; v[p][3] = t.w;
                } else {
#pragma unroll
                    for (int k = 0; k < NC; ++k) if (k < c) v[p][k] = src[at * c + k];
                }
            }
        }
        return;
    }
    // transposed: LDS row q holds the dst column s0 + q, i.e. a run of src pixels; lanes run along it
    const int pitch = TS * c + (VEC ? 4 : 1);
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
        const int q = ly + p * ROWS;
        const int r = r0 + lx, s = s0 + q;                 // the dst pixel this thread stages
        if (r < hd && s < wd) {
            const int y = fa ? hs - 1 - s : s, x = fb ? ws - 1 - r : r;
            const int64_t at = (int64_t)y * ws + x;
            float* __restrict__ d = lds + q * pitch + lx * c;
            if (VEC) {
                *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(src + at * 4);
            } else {
#pragma unroll
                for (int k = 0; k < NC; ++k) if (k < c) d[k] = src[at * c + k];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
        const int i = ly + p * ROWS;
        if (r0 + i < hd && s0 + lx < wd) {
            const float* __restrict__ d = lds + lx * pitch + i * c;
            if (VEC) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(d);
                v[p][0] = t.x; v[p][1] = t.y; v[p][2] = t.z; v[p][3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < NC; ++k) if (k < c) v[p][k] = d[k];
            }
        }
    }
    __syncthreads();      // the next member may overwrite the tile
}

// (rows here are unrolled over the tile form's NC, 4 or 16, not over CTL_ROW_MAXC, and the softmax below likewise: ctl_row_load /
// ctl_row_store / ctl_row_exp of ctl_rows.h have no such form, so this file keeps its own)
template <int NC, bool VEC> __device__ __forceinline__ void tta_store(float* __restrict__ dst, int64_t at, int c, const float* v) {
    if (VEC) {
        *reinterpret_cast<f32x4*>(dst + at * 4) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) dst[at * c + k] = v[k];
    }
}

// views: block = (tile, slice, member), x [n][h][w][c] -> out [T][n][Ho][Wo][c]
template <int TS, int NC, bool VEC>
__global__ __launch_bounds__(TB) void tta_views_kernel(const float* __restrict__ x, int n, int h, int w, int c, tta_codes codes, int tiles_w,
                                                       int tiles, float* __restrict__ out) {
    constexpr int PPT = TS * TS / TB, ROWS = TB / TS;
    __shared__ __attribute__((aligned(16))) float lds[TTA_LDS_FLOATS];
    const int tile = blockIdx.x % tiles;
    const int64_t bt = blockIdx.x / tiles;                 // t * n + b: the output slice
    const int b = (int)(bt % n), code = codes.v[bt / n];
    const int tr = code & 1, f1 = (code >> 1) & 1, f2 = (code >> 2) & 1;
    const int r0 = (tile / tiles_w) * TS, s0 = (tile % tiles_w) * TS;      // (h == w when tr: the view has the plane's extent either way)
    const int64_t hw = (int64_t)h * w;
    float v[PPT][NC];
    tta_fetch<TS, NC, VEC>(x + b * hw * c, tr, tr ? f2 : f1, tr ? f1 : f2, h, w, c, r0, s0, h, w, lds, v);
    const int lx = threadIdx.x % TS, ly = threadIdx.x / TS;
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
        const int r = r0 + ly + p * ROWS, s = s0 + lx;
        if (r < h && s < w) tta_store<NC, VEC>(out + bt * hw * c, (int64_t)r * w + s, c, v[p]);
    }
}

// merge: block = (tile, slice), logits [T][n][Ho][Wo][c] -> aligned [T][n][h][w][c], merged [n][h][w][c], pred [n][h][w]
template <int TS, int NC, bool VEC>
__global__ __launch_bounds__(TB) void tta_merge_kernel(const float* __restrict__ logits, int T, int n, int h, int w, int c, tta_codes codes,
                                                       int is_prob, int tiles_w, int tiles, float* __restrict__ aligned,
                                                       float* __restrict__ merged, uint8_t* __restrict__ pred) {
#pragma clang fp contract(off)
    constexpr int PPT = TS * TS / TB, ROWS = TB / TS;
    __shared__ __attribute__((aligned(16))) float lds[TTA_LDS_FLOATS];
    const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
    const int r0 = (tile / tiles_w) * TS, s0 = (tile % tiles_w) * TS;
    const int64_t hw = (int64_t)h * w;
    const int lx = threadIdx.x % TS, ly = threadIdx.x / TS;
    const bool reduce = merged || pred;
    float acc[PPT][NC];
#pragma unroll
    for (int p = 0; p < PPT; ++p)
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[p][k] = 0.f;
    for (int t = 0; t < T; ++t) {
        const int code = codes.v[t];
        const int64_t slice = ((int64_t)t * n + b) * hw * c;
        float v[PPT][NC];
        tta_fetch<TS, NC, VEC>(logits + slice, code & 1, (code >> 1) & 1, (code >> 2) & 1, h, w, c, r0, s0, h, w, lds, v);
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            const int r = r0 + ly + p * ROWS, s = s0 + lx;
            if (r < h && s < w) {
                if (aligned) tta_store<NC, VEC>(aligned + slice, (int64_t)r * w + s, c, v[p]);
                if (reduce) {
                    if (is_prob) {         // the member's softmax, the arithmetic of ctl_predictive_stats: max, expf, sum, true division
                        float m = -INFINITY, sum = 0.f;
#pragma unroll
                        for (int k = 0; k < NC; ++k) if (k < c) m = fmaxf(m, v[p][k]);
#pragma unroll
                        for (int k = 0; k < NC; ++k) if (k < c) { v[p][k] = expf(v[p][k] - m); sum += v[p][k]; }
#pragma unroll
                        for (int k = 0; k < NC; ++k) if (k < c) v[p][k] = v[p][k] / sum;
                    }
#pragma unroll
                    for (int k = 0; k < NC; ++k) if (k < c) acc[p][k] = (t == 0 && !is_prob) ? v[p][k] : acc[p][k] + v[p][k];
                }
            }
        }
    }
    if (!reduce) return;
    const float Tf = (float)T;
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
        const int r = r0 + ly + p * ROWS, s = s0 + lx;
        if (r < h && s < w) {
            float best = -INFINITY;
            int yh = 0;
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) {
                acc[p][k] = acc[p][k] / Tf;
                if (acc[p][k] > best) { best = acc[p][k]; yh = k; }      // strict: a tie keeps the lowest index (ctl_argmax_c)
            }
            const int64_t at = (int64_t)r * w + s;
            if (merged) tta_store<NC, VEC>(merged + b * hw * c, at, c, acc[p]);
            if (pred) pred[b * hw + at] = (uint8_t)yh;
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
static int tta_check(const char* who, int T, int64_t n, int64_t h, int64_t w, int c, int cmax, const int32_t* codes) {
    CTL_REQUIRE(T >= 1 && T <= CTL_TTA_MAX_VIEWS, "%s: %d views (1 .. %d)", who, T, CTL_TTA_MAX_VIEWS);
    CTL_REQUIRE(codes, "%s: null pointer (codes)", who);
    CTL_REQUIRE(n > 0 && h > 0 && w > 0, "%s: sizes must be positive (slices %lld, plane %lld x %lld)", who, (long long)n, (long long)h,
                (long long)w);
    CTL_REQUIRE(c >= 1 && c <= cmax, "%s: %d channels (1 .. %d)", who, c, cmax);
    unsigned seen = 0u;
    for (int t = 0; t < T; ++t) {
        CTL_REQUIRE(codes[t] >= 0 && codes[t] <= 7, "%s: view code %d (0 .. 7)", who, (int)codes[t]);
        CTL_REQUIRE(!(seen & (1u << codes[t])), "%s: duplicate view code %d", who, (int)codes[t]);
        seen |= 1u << codes[t];
        CTL_REQUIRE(!(codes[t] & 1) || h == w, "%s: view code %d transposes, the plane %lld x %lld is not square", who, (int)codes[t],
                    (long long)h, (long long)w);
    }
    const int64_t lim = (int64_t)1 << 31;      // (factor by factor: no product here can pass 2^63)
    CTL_REQUIRE(h < lim && w < lim && h * w < lim && n <= (lim - 1) / (h * w * T * c * 4),
                "%s: %d x %lld x %lld x %lld pixels of %d channels reach the 2 GiB tensor limit", who, T, (long long)n, (long long)h,
                (long long)w, c);
    return CTL_OK;
}

// (T * n * h * w * c * 4 < 2^31, so the tiles of all slices and members are fewer than 2^31 blocks)
#define TTA_GRID(TS, slices) const int tiles_w = ctl_cdiv(w, TS), tiles = tiles_w * ctl_cdiv(h, TS); const dim3 grid((unsigned)((int64_t)tiles * (slices)))

extern "C" int ctl_tta_views(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, const int32_t* codes, int32_t T, float* out,
                             ctl_stream stream) {
    CTL_REQUIRE(x && out, "tta_views: null pointer (x or out)");
    if (int rc = tta_check("tta_views", T, n, h, w, c, 4, codes)) return rc;
    tta_codes k{};
    for (int t = 0; t < T; ++t) k.v[t] = codes[t];
    TTA_GRID(32, (int64_t)T * n);
    if (ctl_vec4(c, x, out))
        tta_views_kernel<32, 4, true><<<grid, dim3(TB), 0, S_>>>(x, n, h, w, c, k, tiles_w, tiles, out);
    else
        tta_views_kernel<32, 4, false><<<grid, dim3(TB), 0, S_>>>(x, n, h, w, c, k, tiles_w, tiles, out);
    CTL_LAUNCH_CHECK("tta_views");
    return CTL_OK;
}

extern "C" int ctl_tta_merge(const float* logits, int32_t T, int32_t n, int32_t h, int32_t w, int32_t c, const int32_t* codes, int32_t mode,
                             float* aligned, float* merged, uint8_t* pred, ctl_stream stream) {
    CTL_REQUIRE(logits, "tta_merge: null pointer (logits)");
    CTL_REQUIRE(aligned || merged || pred, "tta_merge: no output asked for (aligned, merged and pred are all null)");
    CTL_REQUIRE(mode == CTL_TTA_LOGIT || mode == CTL_TTA_PROB, "tta_merge: mode %d (CTL_TTA_LOGIT or CTL_TTA_PROB)", (int)mode);
    if (int rc = tta_check("tta_merge", T, n, h, w, c, 16, codes)) return rc;
    tta_codes k{};
    for (int t = 0; t < T; ++t) k.v[t] = codes[t];
    const int is_prob = mode == CTL_TTA_PROB;
    if (c <= 4) {
        TTA_GRID(32, n);
        if (ctl_vec4(c, logits, aligned, merged))
            tta_merge_kernel<32, 4, true><<<grid, dim3(TB), 0, S_>>>(logits, T, n, h, w, c, k, is_prob, tiles_w, tiles, aligned, merged, pred);
        else
            tta_merge_kernel<32, 4, false><<<grid, dim3(TB), 0, S_>>>(logits, T, n, h, w, c, k, is_prob, tiles_w, tiles, aligned, merged, pred);
    } else {
        TTA_GRID(16, n);
        tta_merge_kernel<16, 16, false><<<grid, dim3(TB), 0, S_>>>(logits, T, n, h, w, c, k, is_prob, tiles_w, tiles, aligned, merged, pred);
    }
    CTL_LAUNCH_CHECK("tta_merge");
    return CTL_OK;
}
