// Surface-distance metrics of label volumes on device (include/ctl_hip.h, "surface distances"):
//   ctl_surface_stats   'HD' / 'ASD' of medseg/common_utils/metrics.py:224-230 = measure.py:333-548 on the surface-distance
//                       construction of measure.py:1096-1128 (surface = mask XOR binary_erosion(mask), distances from the exact
//                       Euclidean distance transform of the other mask's surface), every class and both directions of a patient
//   ctl_surface_map     the same passes writing the squared-distance map and / or the surface map of one mask
//
// Masks of different classes are disjoint on one side (pred == c), so ONE byte per voxel and side says everything about the
// surfaces: code = c if the voxel is a surface voxel of class c (1 <= c < n_class), else 0.  With m = (class, side) numbering the
// 2 * (n_class - 1) masks (1 * 1 in map mode), the launches of one call are
//   1. sf_code_kernel     code[side][z][y][x]                                                     (erosion, border_value 0)
//   2. sf_row_kernel      g[m][z][y][x]  = |x - x'| to the nearest surface voxel of m in the row, uint16 (65535: none)
//   3. sf_column_kernel   f[m][z][y][x]  = min_j (g[j] * s_x)^2 + ((y - j) * s_y)^2               (all j: no search window)
//   4. sf_column_kernel   d2[m][z][y][x] = min_j f[j] + ((z - j) * s_z)^2                         (3-D form only)
//   5. sf_finalize_kernel per-block partials -> the table
// i.e. 4 launches for the per-slice 2-D form and 5 for the 3-D form, whatever D, H, W and n_class are.  The last column pass samples
// d2 of mask (c, side) at the surface voxels of mask (c, other side) and reduces max d2 / sum sqrt(d2) / count per block; the
// partials are combined in a fixed order (wave shuffles, waves in order, then a fixed-stride tree in the finalize kernel): no
// floating-point atomics, same bits on every call.  All distance arithmetic is fp64; with unit sampling every value is an integer.
#include <math.h>

#include "ctl_common.h"

#define S_ (hipStream_t) stream
#define SF_THREADS 256
#define SF_COLS 64                     // lanes of a wave: 64 consecutive elements of the contiguous axis
#define SF_R 8                         // output rows per thread of a column pass
#define SF_ROWS (4 * SF_R)             // output rows per block (4 waves)
#define SF_JC 64                       // candidate rows staged in LDS at a time: 64 x 64 fp64 = 32 KiB; longer columns loop over chunks
#define SF_NONE 65535u
#define SF_MAXDIM 65534                // offsets along a row are stored as uint16
#define SF_OUTSIDE 255                 // canonical label of a voxel that belongs to no class

static inline size_t sf_align(size_t b) { return (b + 255) & ~(size_t)255; }

__device__ __forceinline__ int sf_canon_pred(uint8_t p, int n, int fg) { return fg ? (p > 0) : (p < n ? (int)p : SF_OUTSIDE); }
__device__ __forceinline__ int sf_canon_gt(int64_t t, int n, int fg) { return fg ? (t > 0) : ((t >= 0 && t < n) ? (int)t : SF_OUTSIDE); }

// ------------------------------------------------------------------------------------------------ 1. surfaces
// scipy.ndimage.binary_erosion(mask, generate_binary_structure(ndim, conn), border_value=0): a mask voxel survives iff every
// neighbour at L1 offset <= conn (each component in -1..1) is inside the array and inside the mask.  gt == NULL: one side only.
__global__ __launch_bounds__(SF_THREADS) void sf_code_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ gt, int D, int H,
                                                             int W, int n, int fg, int ndim, int conn, int sides,
                                                             uint8_t* __restrict__ code) {
    const int64_t vox = (int64_t)D * H * W;
    const int zr = ndim == 3 ? 1 : 0;
    for (int64_t e = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; e < sides * vox; e += (int64_t)gridDim.x * SF_THREADS) {
        const int s = (int)(e / vox);
        const int64_t v = e - s * vox;
        const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((int64_t)W * H));
        const int lab = s == 0 ? sf_canon_pred(pred[v], n, fg) : sf_canon_gt(gt[v], n, fg);
        bool surf = false;
        if (lab != 0 && lab != SF_OUTSIDE) {
            for (int dz = -zr; dz <= zr; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int l1 = abs(dz) + abs(dy) + abs(dx);
                        if (l1 == 0 || l1 > conn) continue;
                        const int zz = z + dz, yy = y + dy, xx = x + dx;
                        if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) { surf = true; continue; }
                        const int64_t u = ((int64_t)zz * H + yy) * W + xx;
                        const int other = s == 0 ? sf_canon_pred(pred[u], n, fg) : sf_canon_gt(gt[u], n, fg);
                        surf |= other != lab;
                    }
        }
        code[e] = surf ? (uint8_t)lab : (uint8_t)0;
    }
}

// ------------------------------------------------------------------------------------------------ 2. rows
// One wave per (mask, row): a forward max-scan of "last surface x at or before me" and a backward min-scan of "next surface x at or
// after me", 64 elements per step with the carry handed from step to step.
__global__ __launch_bounds__(SF_THREADS) void sf_row_kernel(const uint8_t* __restrict__ code, int64_t rows, int W, int masks, int sides,
                                                            int fg, uint16_t* __restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * (SF_THREADS / 64) + (threadIdx.x >> 6);
    if (item >= masks * rows) return;                                          // wave-uniform
    const int m = (int)(item / rows);
    const int64_t r = item - m * rows;
    const int c = fg ? 1 : m / sides + 1;
    const uint8_t* crow = code + ((int64_t)(m % sides) * rows + r) * W;
    uint16_t* grow = g + ((int64_t)m * rows + r) * W;
    const int far = 1 << 20;
    int carry = -far;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        int v = (x < W && crow[x] == c) ? x : -far;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(v, d);
            if (lane >= d) v = max(v, t);
        }
        v = max(v, carry);
        carry = __shfl(v, 63);
        if (x < W) grow[x] = v >= 0 ? (uint16_t)(x - v) : (uint16_t)SF_NONE;
    }
    carry = far;
    for (int x0 = ((W - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
        const int x = x0 + lane;
        int v = (x < W && crow[x] == c) ? x : far;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_down(v, d);
            if (lane + d < 64) v = min(v, t);
        }
        v = min(v, carry);
        carry = __shfl(v, 0);
        if (x < W) {                                                           // the same lane wrote grow[x] above
            const unsigned left = grow[x];
            const unsigned right = v < far ? (unsigned)(v - x) : SF_NONE;
            grow[x] = (uint16_t)min(left, right);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. / 4. columns
// in[o][j][x] (o < O, j < L, x < X; x contiguous) -> out[o][i][x] = min_j in2[o][j][x] + ((i - j) * s)^2 over ALL j, where in2 is the
// fp64 input (FROM16 = false) or (g * s_in)^2 of the uint16 row offsets (65535 -> +inf).  A block owns 64 x and SF_ROWS i of one o and
// walks the whole column in LDS chunks of SF_JC candidates; a thread keeps SF_R consecutive i in registers, so one LDS read feeds SF_R
// candidates.  blockIdx.x = (o * row_tiles + row_tile) * col_blocks + col_block.
// REDUCE: element (o, i, x) is voxel e % vox of mask e / vox with e its linear index; d2 is sampled where the OTHER side's code carries
// the mask's class, and (max d2, sum sqrt(d2), count) of the block go to partial[blockIdx.x][3].
template <bool FROM16, bool REDUCE>
__global__ __launch_bounds__(SF_THREADS) void sf_column_kernel(const void* __restrict__ in_, int L, int64_t X, double s_in, double s,
                                                               int row_tiles, int col_blocks, double* __restrict__ out,
                                                               const uint8_t* __restrict__ code, int64_t vox, int fg,
                                                               double* __restrict__ partial) {
    __shared__ double col[SF_JC][SF_COLS];
    __shared__ double red[SF_THREADS / 64][3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cb = blockIdx.x % col_blocks;
    const int rt = (blockIdx.x / col_blocks) % row_tiles;
    const int64_t o = blockIdx.x / ((int64_t)col_blocks * row_tiles);
    const int64_t x = (int64_t)cb * SF_COLS + lane;
    const int i0 = rt * SF_ROWS + w * SF_R;
    const int64_t base = o * L * X;
    double best[SF_R];
#pragma unroll
    for (int r = 0; r < SF_R; ++r) best[r] = INFINITY;
    for (int jc = 0; jc < L; jc += SF_JC) {
        const int nj = min(SF_JC, L - jc);
        __syncthreads();
        for (int jj = w; jj < nj; jj += SF_THREADS / 64) {
            double v = INFINITY;
            if (x < X) {
                const int64_t idx = base + (int64_t)(jc + jj) * X + x;
                if (FROM16) {
                    const unsigned gq = reinterpret_cast<const uint16_t*>(in_)[idx];
                    const double gs = (double)gq * s_in;
                    v = gq == SF_NONE ? INFINITY : gs * gs;
                } else {
                    v = reinterpret_cast<const double*>(in_)[idx];
                }
            }
            col[jj][lane] = v;
        }
        __syncthreads();
        if (i0 < L) {                                                          // wave-uniform: a wave past the end only helps staging
            for (int jj = 0; jj < nj; ++jj) {
                const double v = col[jj][lane];
                const double d0 = (double)(i0 - (jc + jj));
#pragma unroll
                for (int r = 0; r < SF_R; ++r) {
                    const double t = (d0 + (double)r) * s;
                    best[r] = fmin(best[r], fma(t, t, v));
                }
            }
        }
    }
    double mx = 0.0, sm = 0.0, cn = 0.0;
    if (x < X) {
#pragma unroll
        for (int r = 0; r < SF_R; ++r) {
            const int i = i0 + r;
            if (i >= L) break;
            const int64_t e = base + (int64_t)i * X + x;
            if (out) out[e] = best[r];
            if (REDUCE) {
                const int64_t m = e / vox, v = e - m * vox;
                const int c = fg ? 1 : (int)(m >> 1) + 1;
                if (code[((m & 1) ^ 1) * vox + v] == c) {
                    mx = fmax(mx, best[r]);
                    sm += sqrt(best[r]);
                    cn += 1.0;
                }
            }
        }
    }
    if (REDUCE) {
        for (int d = 32; d > 0; d >>= 1) {
            mx = fmax(mx, __shfl_xor(mx, d));
            sm += __shfl_xor(sm, d);
            cn += __shfl_xor(cn, d);
        }
        if (lane == 0) { red[w][0] = mx; red[w][1] = sm; red[w][2] = cn; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < SF_THREADS / 64; ++k) { mx = fmax(mx, red[k][0]); sm += red[k][1]; cn += red[k][2]; }
            double* p = partial + (int64_t)blockIdx.x * 3;
            p[0] = mx; p[1] = sm; p[2] = cn;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 5. table
// One block per group o (mask x slice in the 2-D form, mask in the 3-D form): table[o] = {max d2, sum d, source surface voxels,
// either mask empty}.  The partner group (other side of the same class) counts THIS mask's surface voxels, and a mask is empty
// exactly when its surface is.
__global__ __launch_bounds__(SF_THREADS) void sf_finalize_kernel(const double* __restrict__ partial, int bpo, int gpm,
                                                                 double* __restrict__ table) {
    __shared__ double red[SF_THREADS][4];
    const int64_t o = blockIdx.x;
    const int64_t m = o / gpm, partner = (m ^ 1) * gpm + o % gpm;
    double mx = 0.0, sm = 0.0, cn = 0.0, pc = 0.0;
    for (int b = threadIdx.x; b < bpo; b += SF_THREADS) {
        const double* p = partial + (o * bpo + b) * 3;
        mx = fmax(mx, p[0]); sm += p[1]; cn += p[2];
        pc += partial[(partner * bpo + b) * 3 + 2];
    }
    red[threadIdx.x][0] = mx; red[threadIdx.x][1] = sm; red[threadIdx.x][2] = cn; red[threadIdx.x][3] = pc;
    __syncthreads();
    for (int d = SF_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            red[threadIdx.x][0] = fmax(red[threadIdx.x][0], red[threadIdx.x + d][0]);
            red[threadIdx.x][1] += red[threadIdx.x + d][1];
            red[threadIdx.x][2] += red[threadIdx.x + d][2];
            red[threadIdx.x][3] += red[threadIdx.x + d][3];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* t = table + o * 4;
        t[0] = red[0][0]; t[1] = red[0][1]; t[2] = red[0][2];
        t[3] = (red[0][2] == 0.0 || red[0][3] == 0.0) ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct sf_plan {
    int64_t vox, masks, groups;        // voxels, masks (class x side), table rows
    int64_t bpo;                       // blocks (= partials) per group of the reducing pass
    size_t off_code, off_g, off_f, off_partial, bytes;
};

static int sf_check_dims(const char* who, int32_t d, int32_t h, int32_t w, int32_t mode, int32_t connectivity) {
    CTL_REQUIRE(d >= 1 && h >= 1 && w >= 1, "%s: D, H, W must be positive (got %d, %d, %d)", who, d, h, w);
    CTL_REQUIRE(d <= SF_MAXDIM && h <= SF_MAXDIM && w <= SF_MAXDIM, "%s: an axis longer than %d is not supported", who, SF_MAXDIM);
    CTL_REQUIRE(mode == 2 || mode == 3, "%s: mode must be 2 (per-slice 2-D) or 3 (whole-volume 3-D), got %d", who, mode);
    CTL_REQUIRE(connectivity >= 1 && connectivity <= mode, "%s: connectivity %d outside 1..%d", who, connectivity, mode);
    return CTL_OK;
}

static int sf_make_plan(const char* who, int32_t d, int32_t h, int32_t w, int64_t classes, int sides, int32_t mode, bool reduce,
                        sf_plan* p) {
    p->vox = (int64_t)d * h * w;
    p->masks = classes * sides;
    p->groups = mode == 2 ? p->masks * d : p->masks;
    p->bpo = mode == 2 ? (int64_t)ctl_cdiv(w, SF_COLS) * ctl_cdiv(h, SF_ROWS) : ctl_cdiv64((int64_t)h * w, SF_COLS) * ctl_cdiv(d, SF_ROWS);
    const int64_t plane_blocks = p->masks * d * (int64_t)ctl_cdiv(w, SF_COLS) * ctl_cdiv(h, SF_ROWS);
    CTL_REQUIRE(plane_blocks < (1ll << 31) && p->groups * p->bpo < (1ll << 31) && p->masks * p->vox < (1ll << 40),
                "%s: the problem is too large for one launch (%lld masks of %lld voxels)", who, (long long)p->masks, (long long)p->vox);
    size_t off = 0;
    p->off_code = off; off += sf_align((size_t)sides * p->vox);
    p->off_g = off; off += sf_align((size_t)p->masks * p->vox * sizeof(uint16_t));
    p->off_f = off; off += mode == 3 ? sf_align((size_t)p->masks * p->vox * sizeof(double)) : 0;
    p->off_partial = off; off += reduce ? sf_align((size_t)p->groups * p->bpo * 3 * sizeof(double)) : 0;
    p->bytes = off;
    return CTL_OK;
}

static int sf_sampling(const char* who, const double* sampling, int32_t mode, double* s) {
    for (int a = 0; a < mode; ++a) {
        s[a] = sampling ? sampling[a] : 1.0;
        CTL_REQUIRE(isfinite(s[a]) && s[a] > 0.0, "%s: sampling[%d] = %g must be finite and positive", who, a, s[a]);
    }
    return CTL_OK;
}

static inline unsigned sf_blocks(int64_t items, int per_block) {
    int64_t b = ctl_cdiv64(items, per_block);
    return (unsigned)(b > 8192 ? 8192 : b);
}

static int sf_stats_args(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode, int32_t connectivity) {
    int rc = sf_check_dims("surface_stats", d, h, w, mode, connectivity);
    if (rc) return rc;
    CTL_REQUIRE(n_class >= 2 && n_class <= 255, "surface_stats: n_class %d outside 2..255", n_class);
    return CTL_OK;
}

extern "C" int32_t ctl_surface_stats_rows(int32_t d, int32_t n_class, int32_t foreground_only, int32_t mode) {
    if (sf_stats_args(d, 1, 1, n_class, mode, 1)) return CTL_EINVAL;
    return 2 * (foreground_only ? 1 : n_class - 1) * (mode == 2 ? d : 1);
}

extern "C" size_t ctl_surface_stats_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t foreground_only, int32_t mode) {
    sf_plan p;
    if (sf_stats_args(d, h, w, n_class, mode, 1) || sf_make_plan("surface_stats", d, h, w, foreground_only ? 1 : n_class - 1, 2, mode, true, &p))
        return 0;
    return p.bytes;
}

extern "C" int ctl_surface_stats(const uint8_t* pred, const int64_t* gt, int32_t d, int32_t h, int32_t w, int32_t n_class,
                                 int32_t foreground_only, int32_t mode, int32_t connectivity, const double* sampling, double* table,
                                 void* workspace, size_t workspace_bytes, ctl_stream stream) {
    int rc = sf_stats_args(d, h, w, n_class, mode, connectivity);
    if (rc) return rc;
    CTL_REQUIRE(pred && gt && table && workspace, "surface_stats: null pointer");
    double s[3];
    if ((rc = sf_sampling("surface_stats", sampling, mode, s))) return rc;
    sf_plan p;
    const int fg = foreground_only ? 1 : 0;
    if ((rc = sf_make_plan("surface_stats", d, h, w, fg ? 1 : n_class - 1, 2, mode, true, &p))) return rc;
    CTL_REQUIRE(workspace_bytes >= p.bytes, "surface_stats: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    char* ws = (char*)workspace;
    uint8_t* code = (uint8_t*)(ws + p.off_code);
    uint16_t* g = (uint16_t*)(ws + p.off_g);
    double* f = (double*)(ws + p.off_f);
    double* partial = (double*)(ws + p.off_partial);
    const int64_t rows = (int64_t)d * h;
    const int cbw = ctl_cdiv(w, SF_COLS), rth = ctl_cdiv(h, SF_ROWS);
    const double sy = s[mode - 2], sx = s[mode - 1];

    sf_code_kernel<<<dim3(sf_blocks(2 * p.vox, SF_THREADS)), dim3(SF_THREADS), 0, S_>>>(pred, gt, d, h, w, n_class, fg, mode, connectivity, 2, code);
    CTL_LAUNCH_CHECK("surface_code");
    sf_row_kernel<<<dim3((unsigned)ctl_cdiv64(p.masks * rows, SF_THREADS / 64)), dim3(SF_THREADS), 0, S_>>>(code, rows, w, (int)p.masks, 2, fg, g);
    CTL_LAUNCH_CHECK("surface_rows");
    const dim3 grid2((unsigned)(p.masks * d * rth * cbw));
    if (mode == 2) {
        sf_column_kernel<true, true><<<grid2, dim3(SF_THREADS), 0, S_>>>(g, h, w, sx, sy, rth, cbw, nullptr, code, p.vox, fg, partial);
        CTL_LAUNCH_CHECK("surface_columns");
    } else {
        sf_column_kernel<true, false><<<grid2, dim3(SF_THREADS), 0, S_>>>(g, h, w, sx, sy, rth, cbw, f, nullptr, p.vox, fg, nullptr);
        CTL_LAUNCH_CHECK("surface_columns");
        const int64_t plane = (int64_t)h * w;
        const int cb3 = (int)ctl_cdiv64(plane, SF_COLS), rt3 = ctl_cdiv(d, SF_ROWS);
        sf_column_kernel<false, true><<<dim3((unsigned)(p.masks * rt3 * cb3)), dim3(SF_THREADS), 0, S_>>>(f, d, plane, 1.0, s[0], rt3, cb3, nullptr, code,
                                                                                                         p.vox, fg, partial);
        CTL_LAUNCH_CHECK("surface_slices");
    }
    sf_finalize_kernel<<<dim3((unsigned)p.groups), dim3(SF_THREADS), 0, S_>>>(partial, (int)p.bpo, mode == 2 ? d : 1, table);
    CTL_LAUNCH_CHECK("surface_finalize");
    return CTL_OK;
}

extern "C" size_t ctl_surface_map_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t mode) {
    sf_plan p;
    if (sf_check_dims("surface_map", d, h, w, mode, 1) || sf_make_plan("surface_map", d, h, w, 1, 1, mode, false, &p)) return 0;
    return p.bytes;
}

extern "C" int ctl_surface_map(const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t mode, int32_t connectivity,
                               const double* sampling, double* d2_out, uint8_t* surface_out, void* workspace, size_t workspace_bytes,
                               ctl_stream stream) {
    int rc = sf_check_dims("surface_map", d, h, w, mode, connectivity);
    if (rc) return rc;
    CTL_REQUIRE(mask && (d2_out || surface_out) && (workspace || !d2_out), "surface_map: null pointer");
    double s[3];
    if ((rc = sf_sampling("surface_map", sampling, mode, s))) return rc;
    sf_plan p;
    if ((rc = sf_make_plan("surface_map", d, h, w, 1, 1, mode, false, &p))) return rc;
    CTL_REQUIRE(!d2_out || workspace_bytes >= p.bytes, "surface_map: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    char* ws = (char*)workspace;
    uint8_t* code = surface_out ? surface_out : (uint8_t*)(ws + p.off_code);
    sf_code_kernel<<<dim3(sf_blocks(p.vox, SF_THREADS)), dim3(SF_THREADS), 0, S_>>>(mask, nullptr, d, h, w, 2, 1, mode, connectivity, 1, code);
    CTL_LAUNCH_CHECK("surface_code");
    if (!d2_out) return CTL_OK;
    uint16_t* g = (uint16_t*)(ws + p.off_g);
    double* f = (double*)(ws + p.off_f);
    const int64_t rows = (int64_t)d * h;
    const int cbw = ctl_cdiv(w, SF_COLS), rth = ctl_cdiv(h, SF_ROWS);
    sf_row_kernel<<<dim3((unsigned)ctl_cdiv64(rows, SF_THREADS / 64)), dim3(SF_THREADS), 0, S_>>>(code, rows, w, 1, 1, 1, g);
    CTL_LAUNCH_CHECK("surface_rows");
    sf_column_kernel<true, false><<<dim3((unsigned)(d * rth * cbw)), dim3(SF_THREADS), 0, S_>>>(g, h, w, s[mode - 1], s[mode - 2], rth, cbw,
                                                                                              mode == 2 ? d2_out : f, nullptr, p.vox, 1, nullptr);
    CTL_LAUNCH_CHECK("surface_columns");
    if (mode == 3) {
        const int64_t plane = (int64_t)h * w;
        const int cb3 = (int)ctl_cdiv64(plane, SF_COLS), rt3 = ctl_cdiv(d, SF_ROWS);
        sf_column_kernel<false, false><<<dim3((unsigned)(rt3 * cb3)), dim3(SF_THREADS), 0, S_>>>(f, d, plane, 1.0, s[0], rt3, cb3, d2_out, nullptr, p.vox,
                                                                                               1, nullptr);
        CTL_LAUNCH_CHECK("surface_slices");
    }
    return CTL_OK;
}
