// Class fields of a batch of label slices (include/ctl_hip.h, "distance-map losses"): for every class k of a label map y[b][h][w] the exact
// Euclidean distance, within the slice, from a pixel to the nearest pixel on the OTHER side of the set S = {y == k}:
//   p outside S: to the nearest pixel of S;   p inside S: to the nearest pixel not in S;   S empty or the whole plane: 0 everywhere.
// These are the per-step distance maps of the 'boundary' and 'hausdorff dt' losses (ctl_loss.hip): the labels a training step sees are
// warped and gathered on the device, so their maps cannot be precomputed.
//
// Two launches per call, whatever b, n_class, h, w and the content are:
//   1. df_row_kernel     g[b][k][s][y][x] = |x - x'| to the nearest pixel of the row that is in S (s = 0) / not in S (s = 1), uint16 (65535:
//                        none).  One wave per (b, k, row): prefix-max and suffix-min scans of 64 elements with a carry, as sf_row_kernel.
//   2. df_column_kernel  d2[b][k][i][x] = min_j g[b][k][s][j][x]^2 + (i - j)^2 over ALL j, with s chosen by the pixel's own membership:
//                        a pixel reads ONE of the two row maps.  A block owns 64 x and DF_ROWS i of one slice and up to four classes and
//                        walks the column in LDS chunks of DF_JC candidates of both maps, from its own rows outwards; a chunk too far
//                        away to hold a candidate below any minimum of the block ends the walk in its direction (the result is still
//                        the minimum over all j).
// At unit spacing with h, w <= 2048 every squared distance is an integer below 2 * 2047^2 < 2^24: the transform is exact in 32-bit integer
// arithmetic, there is no fp64 column pass (longer axes are refused).  "None" is 2^30, which no sum of a real candidate reaches and no
// sum with it overflows; a minimum at or above it means the other side does not exist in the slice: the field is 0 there.
// Output forms: d2 as fp64 planar [b][k][h][w]; the training forms fp32 in the logits' NHWC layout [b][h][w][k], each value rounded once:
// `squared` from the integer (exact), `signed` from the fp64 square root: F outside S, -(F - 1) inside, 0 where the field is 0.  A thread
// keeps the four classes of its pixels in registers, so a row of four classes leaves as one 16-byte store.
// No readback, no atomics, no data-dependent launch: the same bits on every call and in a graph replay.
#include <math.h>

#include "ctl_device.h"

#define DF_THREADS 256
#define DF_COLS 64                     // lanes of a wave: 64 consecutive x
#define DF_R 8                         // output rows per thread
#define DF_ROWS (4 * DF_R)             // output rows per block (4 waves)
#define DF_JC DF_ROWS                  // candidate rows of both maps staged at a time (2 x 32 x 64 x 4 bytes = 16 KiB): chunk ci holds the rows of row tile ci
#define DF_KG 4                        // classes per block
#define DF_NONE16 65535u
#define DF_NONE (1 << 30)
#define DF_MAXDIM 2048
#define DF_MAXC 16
#define DF_OUTSIDE 255                 // canonical label of a pixel that belongs to no class

__device__ __forceinline__ int df_canon(uint8_t l, int n) { return l < n ? (int)l : DF_OUTSIDE; }
__device__ __forceinline__ int df_canon(int64_t l, int n) { return (l >= 0 && l < n) ? (int)l : DF_OUTSIDE; }

// ------------------------------------------------------------------------------------------------ 1. rows
template <typename LT>
__global__ __launch_bounds__(DF_THREADS) void df_row_kernel(const LT* __restrict__ label, int64_t items, int H, int W, int n,
                                                            uint16_t* __restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * (DF_THREADS / 64) + (threadIdx.x >> 6);      // (b * n + k) * H + y
    if (item >= items) return;                                                 // wave-uniform
    const int y = (int)(item % H);
    const int64_t bk = item / H;
    const int k = (int)(bk % n);
    const LT* lrow = label + ((bk / n) * H + y) * W;
    uint16_t* gin = g + ((bk * 2) * H + y) * W;
    uint16_t* gout = g + ((bk * 2 + 1) * H + y) * W;
    const int far = 1 << 20;
    int cin = -far, cout = -far;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < W && df_canon(lrow[x], n) == k;
        int vi = in ? x : -far, vo = (x < W && !in) ? x : -far;
        vi = max(ctl_wave_prefix_max(vi), cin);
        vo = max(ctl_wave_prefix_max(vo), cout);
        cin = __shfl(vi, 63);
        cout = __shfl(vo, 63);
        if (x < W) {
            gin[x] = vi >= 0 ? (uint16_t)(x - vi) : (uint16_t)DF_NONE16;
            gout[x] = vo >= 0 ? (uint16_t)(x - vo) : (uint16_t)DF_NONE16;
        }
    }
    cin = far; cout = far;
    for (int x0 = ((W - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
        const int x = x0 + lane;
        const bool in = x < W && df_canon(lrow[x], n) == k;
        int vi = in ? x : far, vo = (x < W && !in) ? x : far;
        vi = min(ctl_wave_suffix_min(vi), cin);
        vo = min(ctl_wave_suffix_min(vo), cout);
        cin = __shfl(vi, 0);
        cout = __shfl(vo, 0);
        if (x < W) {                                                           // the same lane wrote gin[x] / gout[x] above
            const unsigned ri = vi < far ? (unsigned)(vi - x) : DF_NONE16, ro = vo < far ? (unsigned)(vo - x) : DF_NONE16;
            gin[x] = (uint16_t)min((unsigned)gin[x], ri);
            gout[x] = (uint16_t)min((unsigned)gout[x], ro);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 2. columns
// blockIdx.x = ((b * groups + class group) * row_tiles + row_tile) * col_blocks + col_block
template <typename LT>
__global__ __launch_bounds__(DF_THREADS) void df_column_kernel(const LT* __restrict__ label, const uint16_t* __restrict__ g, int H, int W, int n,
                                                               int groups, int row_tiles, int col_blocks, int form, void* __restrict__ out_) {
    __shared__ int col[2][DF_JC][DF_COLS];
    __shared__ int wmax[2][DF_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cb = blockIdx.x % col_blocks;
    const int rt = (blockIdx.x / col_blocks) % row_tiles;
    const int kg = (blockIdx.x / (col_blocks * row_tiles)) % groups;
    const int64_t b = blockIdx.x / ((int64_t)col_blocks * row_tiles * groups);
    const int x = cb * DF_COLS + lane;
    const int i0 = rt * DF_ROWS + w * DF_R;
    const int k0 = kg * DF_KG, nk = min(DF_KG, n - k0);
    const int64_t plane = (int64_t)H * W;
    int lab[DF_R];
#pragma unroll
    for (int r = 0; r < DF_R; ++r) lab[r] = (x < W && i0 + r < H) ? df_canon(label[b * plane + (int64_t)(i0 + r) * W + x], n) : DF_OUTSIDE;
    int res[DF_KG][DF_R];
    int it = 0;                                                                // chunks looked at so far (block-uniform)
#pragma unroll
    for (int kk = 0; kk < DF_KG; ++kk) {
#pragma unroll
        for (int r = 0; r < DF_R; ++r) res[kk][r] = 0;
        if (kk >= nk) continue;                                                // block-uniform
        const int k = k0 + kk;
        const uint16_t* gk = g + (b * n + k) * 2 * plane;
        int best[DF_R];
        bool in[DF_R];
#pragma unroll
        for (int r = 0; r < DF_R; ++r) { best[r] = DF_NONE; in[r] = lab[r] == k; }
        // chunks from the tile's own rows outwards, first towards row 0, then towards row H-1.  A chunk whose nearest row is `gap` rows from
        // the tile holds no candidate below gap^2: once that is no less than every minimum the block still carries, this chunk and all
        // farther ones of the direction are left out -- the minima are the same as over all j.
        for (int dir = 0; dir < 2; ++dir) {
            for (int ci = dir ? rt + 1 : rt; dir ? ci < row_tiles : ci >= 0; ci += dir ? 1 : -1) {
                const int jc = ci * DF_JC, nj = min(DF_JC, H - jc);
                const int gap = ci == rt ? 0 : (dir ? jc - (rt * DF_ROWS + DF_ROWS - 1) : rt * DF_ROWS - (jc + nj - 1));
                int m = 0;                                                     // largest minimum of the wave's pixels
#pragma unroll
                for (int r = 0; r < DF_R; ++r) m = (x < W && i0 + r < H) ? max(m, best[r]) : m;
                for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
                if (lane == 0) wmax[it & 1][w] = m;
                __syncthreads();                                               // also: every wave is done with the previous chunk in col
                const int bm = max(max(wmax[it & 1][0], wmax[it & 1][1]), max(wmax[it & 1][2], wmax[it & 1][3]));
                ++it;                                                          // (two buffers: the next write cannot pass a reader of this one)
                if (gap * gap >= bm) break;                                    // block-uniform
                for (int jj = w; jj < 2 * nj; jj += DF_THREADS / 64) {
                    const int s = jj >= nj ? 1 : 0, j = jj - s * nj;
                    int v = DF_NONE;
                    if (x < W) {
                        const int gq = gk[s * plane + (int64_t)(jc + j) * W + x];
                        v = gq == (int)DF_NONE16 ? DF_NONE : gq * gq;
                    }
                    col[s][j][lane] = v;
                }
                __syncthreads();
                const int gw = jc > i0 + DF_R - 1 ? jc - (i0 + DF_R - 1) : (jc + nj - 1 < i0 ? i0 - (jc + nj - 1) : 0);
                if (gw * gw < m) {                                             // wave-uniform (a wave past the end has m = 0: it only helps staging)
                    for (int jj = 0; jj < nj; ++jj) {
                        const int vin = col[0][jj][lane], vout = col[1][jj][lane];
                        const int d0 = i0 - (jc + jj);
#pragma unroll
                        for (int r = 0; r < DF_R; ++r) {
                            const int t = d0 + r;
                            best[r] = min(best[r], (in[r] ? vout : vin) + t * t);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < DF_R; ++r) res[kk][r] = best[r] >= DF_NONE ? 0 : best[r];
    }
    if (x >= W) return;
#pragma unroll
    for (int r = 0; r < DF_R; ++r) {
        const int i = i0 + r;
        if (i >= H) break;
        const int64_t pix = b * plane + (int64_t)i * W + x;
        if (form == CTL_FIELD_D2) {
            double* out = reinterpret_cast<double*>(out_);
#pragma unroll
            for (int kk = 0; kk < DF_KG; ++kk)
                if (kk < nk) out[((b * n + k0 + kk) * H + i) * (int64_t)W + x] = (double)res[kk][r];
            continue;
        }
        float v[DF_KG];
#pragma unroll
        for (int kk = 0; kk < DF_KG; ++kk) {
            const int d2 = res[kk][r];
            if (form == CTL_FIELD_SQUARED) v[kk] = (float)d2;                  // d2 < 2^24: exact
            else {
                const double f = sqrt((double)d2);                             // correctly rounded; one more rounding to fp32
                v[kk] = d2 == 0 ? 0.f : (lab[r] == k0 + kk ? (float)(-(f - 1.0)) : (float)f);
            }
        }
        float* out = reinterpret_cast<float*>(out_) + pix * n + k0;
        if (n == DF_KG && ((uintptr_t)out_ & 15) == 0) *reinterpret_cast<f32x4*>(out) = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int kk = 0; kk < DF_KG; ++kk) if (kk < nk) out[kk] = v[kk];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct df_plan { int groups, rth, cbw; int64_t row_items, col_blocks; size_t bytes; };

static int df_make_plan(const char* who, int32_t b, int32_t h, int32_t w, int32_t n_class, df_plan* p) {
    CTL_REQUIRE(b >= 1 && h >= 1 && w >= 1, "%s: sizes must be positive (batch %d, plane %d x %d)", who, b, h, w);
    CTL_REQUIRE(n_class >= 1 && n_class <= DF_MAXC, "%s: %d classes (1 .. %d)", who, n_class, DF_MAXC);
    CTL_REQUIRE(h <= DF_MAXDIM && w <= DF_MAXDIM, "%s: a plane of %d x %d: an axis longer than %d does not fit the 32-bit integer transform", who, h,
                w, DF_MAXDIM);
    p->groups = ctl_cdiv(n_class, DF_KG);
    p->rth = ctl_cdiv(h, DF_ROWS);
    p->cbw = ctl_cdiv(w, DF_COLS);
    p->row_items = (int64_t)b * n_class * h;
    p->col_blocks = (int64_t)b * p->groups * p->rth * p->cbw;
    const int64_t elems = (int64_t)b * n_class * h * w;
    CTL_REQUIRE(ctl_cdiv64(p->row_items, DF_THREADS / 64) < (1ll << 31) && p->col_blocks < (1ll << 31) && elems < (1ll << 31),
                "%s: the problem is too large for one launch (%d slices of %d x %d, %d classes)", who, b, h, w, n_class);
    p->bytes = ctl_align256((size_t)elems * 2 * sizeof(uint16_t));
    return CTL_OK;
}

extern "C" size_t ctl_class_fields_ws_bytes(int32_t b, int32_t h, int32_t w, int32_t n_class) {
    df_plan p;
    return df_make_plan("class_fields_ws_bytes", b, h, w, n_class, &p) ? 0 : p.bytes;
}

template <typename LT>
static int df_run(const LT* label, int32_t h, int32_t w, int32_t n, int32_t form, void* out, uint16_t* g, const df_plan& p, ctl_stream stream) {
    df_row_kernel<LT><<<dim3((unsigned)ctl_cdiv64(p.row_items, DF_THREADS / 64)), dim3(DF_THREADS), 0, S_>>>(label, p.row_items, h, w, n, g);
    CTL_LAUNCH_CHECK("class_fields_rows");
    df_column_kernel<LT><<<dim3((unsigned)p.col_blocks), dim3(DF_THREADS), 0, S_>>>(label, g, h, w, n, p.groups, p.rth, p.cbw, form, out);
    CTL_LAUNCH_CHECK("class_fields_columns");
    return CTL_OK;
}

extern "C" int ctl_class_fields(const void* label, int32_t label_dtype, int32_t b, int32_t h, int32_t w, int32_t n_class, int32_t form,
                                void* out, void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(label && out && workspace, "class_fields: null pointer");
    CTL_REQUIRE(label_dtype == CTL_LABEL_U8 || label_dtype == CTL_LABEL_I64, "class_fields: unknown label dtype %d (0: uint8, 1: int64)", label_dtype);
    CTL_REQUIRE(form == CTL_FIELD_D2 || form == CTL_FIELD_SIGNED || form == CTL_FIELD_SQUARED,
                "class_fields: unknown form %d (0: d2, 1: signed, 2: squared)", form);
    df_plan p;
    if (int rc = df_make_plan("class_fields", b, h, w, n_class, &p)) return rc;
    CTL_REQUIRE(workspace_bytes >= p.bytes, "class_fields: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    if (label_dtype == CTL_LABEL_U8) return df_run((const uint8_t*)label, h, w, n_class, form, out, (uint16_t*)workspace, p, stream);
    return df_run((const int64_t*)label, h, w, n_class, form, out, (uint16_t*)workspace, p, stream);
}
