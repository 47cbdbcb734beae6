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
//
//   ctl_surface_quantiles   order statistics of the POOLED surface distances of a class (both directions in one list): what 'HD95'
//                       (medpy >= 0.4 `hd95`, per slice by analogy with metrics.py:226-233) needs; 'ASSD' (measure.py:402-455) is two
//                       rows of the statistics table.  A group is a class (3-D form) or a (class, slice) pair (2-D form).  The same
//                       launches with the last column pass in its EMIT form, plus exactly 3 more, whatever D, H, W, n_class, n_q and the
//                       content are:
//   1b. sf_q_count_kernel   surface voxels per (side, slice, class) from code: one block per (side, slice), LDS histogram, plain stores
//   1c. sf_q_scan_kernel    per group: voxels of side 0 / side 1, exclusive scan of their sum = first key slot of the group, cursor = 0
//   3./4. EMIT              every sampled d2 also goes, as its 64 raw bits (a non-negative double orders like its bits), to
//                           keys[first[group] + slot]; slots from ONE integer atomicAdd per wave on the group's cursor.  The order of
//                           the keys of a group differs from call to call; only the multiset is used.
//   6.  sf_q_select_kernel  one block per group: n = pooled count, k = floor((n - 1) * q / 100) in fp64, and the keys of rank k and
//                           min(k + 1, n - 1) by most-significant-digit-first radix selection (eight 8-bit passes, LDS histograms,
//                           integer atomics only).
// No readback, no synchronisation, no data-dependent launch; the max / sum / count partials are those of ctl_surface_stats, bit for bit.
#include <math.h>

#include "ctl_device.h"

#define SF_THREADS 256
#define SF_COLS 64                     // lanes of a wave: 64 consecutive elements of the contiguous axis
#define SF_R 8                         // output rows per thread of a column pass
#define SF_ROWS (4 * SF_R)             // output rows per block (4 waves)
#define SF_JC 64                       // candidate rows staged in LDS at a time: 64 x 64 fp64 = 32 KiB; longer columns loop over chunks
#define SF_NONE 65535u
#define SF_MAXDIM 65534                // offsets along a row are stored as uint16
#define SF_OUTSIDE 255                 // canonical label of a voxel that belongs to no class

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
        v = max(ctl_wave_prefix_max(v), carry);
        carry = __shfl(v, 63);
        if (x < W) grow[x] = v >= 0 ? (uint16_t)(x - v) : (uint16_t)SF_NONE;
    }
    carry = far;
    for (int x0 = ((W - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
        const int x = x0 + lane;
        int v = (x < W && crow[x] == c) ? x : far;
        v = min(ctl_wave_suffix_min(v), carry);
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
// EMIT (with REDUCE): the sampled d2 are also stored as keys of the block's group (mask / 2) * gpm + o % gpm, gpm = groups per mask.
template <bool FROM16, bool REDUCE, bool EMIT = false>
__global__ __launch_bounds__(SF_THREADS) void sf_column_kernel(const void* __restrict__ in_, int L, int64_t X, double s_in, double s,
                                                               int row_tiles, int col_blocks, double* __restrict__ out,
                                                               const uint8_t* __restrict__ code, int64_t vox, int fg,
                                                               double* __restrict__ partial, int gpm = 1,
                                                               const int64_t* __restrict__ first = nullptr,
                                                               unsigned* __restrict__ cursor = nullptr,
                                                               unsigned long long* __restrict__ keys = nullptr) {
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
    unsigned hit = 0;                                                          // EMIT: bit r = best[r] is a sample
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
                    if (EMIT) hit |= 1u << r;
                }
            }
        }
    }
    if (EMIT) {                                                                // every lane of every wave gets here
        const int mine = __popc(hit);
        int incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const int total = __shfl(incl, 63);
        if (total > 0) {                                                       // wave-uniform
            const int64_t grp = (o / gpm >> 1) * gpm + o % gpm;
            unsigned slot = 0;
            if (lane == 0) slot = atomicAdd(cursor + grp, (unsigned)total);
            slot = __shfl(slot, 0) + (unsigned)(incl - mine);
            unsigned long long* dst = keys + first[grp];
#pragma unroll
            for (int r = 0; r < SF_R; ++r)
                if (hit >> r & 1u) dst[slot++] = (unsigned long long)__double_as_longlong(best[r]);
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

// ------------------------------------------------------------------------------------------------ quantiles: key slots
// One block per (side, slice): cnt[(side * D + z) * classes + c - 1] = surface voxels of class c in that slice of that side.  Background
// (code 0, almost every voxel) is skipped, so the LDS atomics see only the sparse surface.  Plain stores: nothing to zero beforehand.
__global__ __launch_bounds__(SF_THREADS) void sf_q_count_kernel(const uint8_t* __restrict__ code, int64_t plane, int classes,
                                                                unsigned* __restrict__ cnt) {
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0;                                                     // SF_THREADS == 256
    __syncthreads();
    const uint8_t* src = code + (int64_t)blockIdx.x * plane;
    if ((plane & 3) == 0) {                                                    // code is 256-byte aligned, so every slice is word aligned
        const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
        for (int64_t i = threadIdx.x; i < plane / 4; i += SF_THREADS) {
            uint32_t v = src4[i];
            while (v) {
                const unsigned b = v & 255u;
                if (b) atomicAdd(&hist[b], 1u);
                v >>= 8;
            }
        }
    } else {
        for (int64_t i = threadIdx.x; i < plane; i += SF_THREADS) {
            const unsigned b = src[i];
            if (b) atomicAdd(&hist[b], 1u);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < classes; c += SF_THREADS) cnt[(int64_t)blockIdx.x * classes + c] = hist[c + 1];
}

// One block.  Group gi = class_index * gpm + zg (gpm = D in the 2-D form, 1 in the 3-D form, where a group sums its class over all
// slices): gn[gi] = {voxels of side 0, of side 1}, first[gi] = exclusive scan of their sums in group order, cursor[gi] = 0.
__global__ __launch_bounds__(SF_THREADS) void sf_q_scan_kernel(const unsigned* __restrict__ cnt, int D, int classes, int gpm, int64_t groups,
                                                               unsigned* __restrict__ gn, int64_t* __restrict__ first,
                                                               unsigned* __restrict__ cursor) {
    __shared__ int64_t wsum[SF_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t g0 = 0; g0 < groups; g0 += SF_THREADS) {
        const int64_t gi = g0 + threadIdx.x;
        unsigned n0 = 0, n1 = 0;
        if (gi < groups) {
            const int c = (int)(gi / gpm), zg = (int)(gi % gpm);
            const int z0 = gpm == 1 ? 0 : zg, z1 = gpm == 1 ? D : zg + 1;
            for (int z = z0; z < z1; ++z) {
                n0 += cnt[(int64_t)z * classes + c];
                n1 += cnt[((int64_t)D + z) * classes + c];
            }
        }
        const int64_t mine = (int64_t)n0 + n1;
        int64_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        __syncthreads();                                                       // wsum of the previous round has been read
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int64_t before = carry, all = 0;
        for (int k = 0; k < SF_THREADS / 64; ++k) {
            if (k < w) before += wsum[k];
            all += wsum[k];
        }
        if (gi < groups) {
            gn[gi * 2] = n0; gn[gi * 2 + 1] = n1;
            first[gi] = before + incl - mine;
            cursor[gi] = 0;
        }
        carry += all;
    }
}

// ------------------------------------------------------------------------------------------------ quantiles: selection
struct sf_qf { double v[4]; };         // the requested fractions q / 100

// One 8-bit digit of the radix selection: among the n keys whose bits above `shift + 8` equal those of `prefix`, find the digit at
// `shift` that holds rank `rank` (0-based, within those keys); returns it, rank becomes the rank inside that digit's keys and `eq` their
// number.  Every thread of the block calls it and gets the same answer.
__device__ __forceinline__ unsigned sf_q_digit(const unsigned long long* __restrict__ keys, unsigned n, unsigned long long prefix, int shift,
                                               unsigned& rank, unsigned& eq, unsigned* hist, unsigned* wtot, unsigned* found) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                                           // hist / found of the previous digit have been read
    hist[threadIdx.x] = 0;
    __syncthreads();
    const bool top = shift == 56;
    const unsigned long long want = top ? 0ull : prefix >> (shift + 8);
    for (unsigned i0 = threadIdx.x; i0 < n; i0 += 4 * SF_THREADS) {
        unsigned long long k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned i = i0 + u * SF_THREADS;
            k[u] = i < n ? keys[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned i = i0 + u * SF_THREADS;
            if (i < n && (top || (k[u] >> (shift + 8)) == want)) atomicAdd(&hist[(unsigned)(k[u] >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    const unsigned mine = hist[threadIdx.x];
    unsigned incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int k = 0; k < w; ++k) before += wtot[k];
    const unsigned excl = before + incl - mine;
    if (rank >= excl && rank < excl + mine) { found[0] = threadIdx.x; found[1] = rank - excl; found[2] = mine; }     // exactly one thread
    __syncthreads();
    rank = found[1];
    eq = found[2];
    return found[0];
}

// One block per group and all n_q fractions: table[gi][j] = {key of rank k, key of rank min(k + 1, n - 1), n, 0}, k = floor((n - 1) * qf),
// or {+inf, +inf, 0, 1} when either mask of the group is empty.  The key after rank k is the same key while copies of it remain, else
// the smallest larger key (one more pass, integer atomicMin in LDS).
__global__ __launch_bounds__(SF_THREADS) void sf_q_select_kernel(const unsigned long long* __restrict__ keys_all, const int64_t* __restrict__ first,
                                                                 const unsigned* __restrict__ gn, sf_qf qf, int n_q, double* __restrict__ table) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wtot[SF_THREADS / 64];
    __shared__ unsigned found[3];
    __shared__ unsigned long long above;
    const int64_t gi = blockIdx.x;
    const unsigned n0 = gn[gi * 2], n1 = gn[gi * 2 + 1];
    const unsigned n = n0 + n1;
    const unsigned long long* keys = keys_all + first[gi];
    for (int j = 0; j < n_q; ++j) {                                            // block-uniform control flow throughout
        double* t = table + (gi * n_q + j) * 4;
        if (n0 == 0 || n1 == 0) {
            if (threadIdx.x == 0) { t[0] = INFINITY; t[1] = INFINITY; t[2] = 0.0; t[3] = 1.0; }
            continue;
        }
        const double v = __dmul_rn((double)(n - 1), qf.v[j]);                  // one multiply, never contracted
        unsigned k = (unsigned)floor(v);
        if (k > n - 1) k = n - 1;
        unsigned long long key = 0;
        unsigned rank = k, eq = 0;
        for (int shift = 56; shift >= 0; shift -= 8)
            key |= (unsigned long long)sf_q_digit(keys, n, key, shift, rank, eq, hist, wtot, found) << shift;
        unsigned long long next = key;
        if (k + 1 < n && rank + 1 >= eq) {                                     // no further copy of `key`: the smallest key above it
            __syncthreads();
            if (threadIdx.x == 0) above = ~0ull;
            __syncthreads();
            unsigned long long lo = ~0ull;
            for (unsigned i = threadIdx.x; i < n; i += SF_THREADS) {
                const unsigned long long c = keys[i];
                if (c > key && c < lo) lo = c;
            }
            if (lo != ~0ull) atomicMin(&above, lo);
            __syncthreads();
            next = above;
        }
        if (threadIdx.x == 0) {
            t[0] = __longlong_as_double((long long)key); t[1] = __longlong_as_double((long long)next); t[2] = (double)n; t[3] = 0.0;
        }
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
    p->off_code = off; off += ctl_align256((size_t)sides * p->vox);
    p->off_g = off; off += ctl_align256((size_t)p->masks * p->vox * sizeof(uint16_t));
    p->off_f = off; off += mode == 3 ? ctl_align256((size_t)p->masks * p->vox * sizeof(double)) : 0;
    p->off_partial = off; off += reduce ? ctl_align256((size_t)p->groups * p->bpo * 3 * sizeof(double)) : 0;
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

// The key lists of ctl_surface_quantiles, behind the statistics workspace.
struct sf_qplan {
    int64_t classes, gpm, groups;      // groups = classes * gpm key lists
    size_t off_cnt, off_gn, off_first, off_cursor, off_keys, bytes;
    sf_qf qf;
    int n_q;
    double* q_table;
};

// The launches of ctl_surface_stats; with `qp` the key-slot kernels, the EMIT form of the last column pass and the selection as well.
// `table` may be NULL with `qp` (no finalize launch then).  Every argument has been checked.
static int sf_run(const uint8_t* pred, const int64_t* gt, int32_t d, int32_t h, int32_t w, int32_t n_class, int fg, int32_t mode,
                  int32_t connectivity, const double* s, double* table, void* workspace, const sf_plan& p, const sf_qplan* qp,
                  ctl_stream stream) {
    char* ws = (char*)workspace;
    uint8_t* code = (uint8_t*)(ws + p.off_code);
    uint16_t* g = (uint16_t*)(ws + p.off_g);
    double* f = (double*)(ws + p.off_f);
    double* partial = (double*)(ws + p.off_partial);
    const int64_t rows = (int64_t)d * h;
    const int cbw = ctl_cdiv(w, SF_COLS), rth = ctl_cdiv(h, SF_ROWS);
    const double sy = s[mode - 2], sx = s[mode - 1];

    unsigned* gn = nullptr;
    int64_t* first = nullptr;
    unsigned* cursor = nullptr;
    unsigned long long* keys = nullptr;
    const int gpm = mode == 2 ? d : 1;

    sf_code_kernel<<<dim3(ctl_blocks(2 * p.vox, SF_THREADS, 8192)), dim3(SF_THREADS), 0, S_>>>(pred, gt, d, h, w, n_class, fg, mode, connectivity, 2, code);
    CTL_LAUNCH_CHECK("surface_code");
    if (qp) {
        unsigned* cnt = (unsigned*)(ws + qp->off_cnt);
        gn = (unsigned*)(ws + qp->off_gn);
        first = (int64_t*)(ws + qp->off_first);
        cursor = (unsigned*)(ws + qp->off_cursor);
        keys = (unsigned long long*)(ws + qp->off_keys);
        sf_q_count_kernel<<<dim3((unsigned)(2 * d)), dim3(SF_THREADS), 0, S_>>>(code, (int64_t)h * w, (int)qp->classes, cnt);
        CTL_LAUNCH_CHECK("surface_q_count");
        sf_q_scan_kernel<<<dim3(1), dim3(SF_THREADS), 0, S_>>>(cnt, d, (int)qp->classes, gpm, qp->groups, gn, first, cursor);
        CTL_LAUNCH_CHECK("surface_q_scan");
    }
    sf_row_kernel<<<dim3((unsigned)ctl_cdiv64(p.masks * rows, SF_THREADS / 64)), dim3(SF_THREADS), 0, S_>>>(code, rows, w, (int)p.masks, 2, fg, g);
    CTL_LAUNCH_CHECK("surface_rows");
    const dim3 grid2((unsigned)(p.masks * d * rth * cbw));
    if (mode == 2 && qp) {
        sf_column_kernel<true, true, true><<<grid2, dim3(SF_THREADS), 0, S_>>>(g, h, w, sx, sy, rth, cbw, nullptr, code, p.vox, fg, partial, gpm, first,
                                                                              cursor, keys);
        CTL_LAUNCH_CHECK("surface_columns_emit");
    } else if (mode == 2) {
        sf_column_kernel<true, true><<<grid2, dim3(SF_THREADS), 0, S_>>>(g, h, w, sx, sy, rth, cbw, nullptr, code, p.vox, fg, partial);
        CTL_LAUNCH_CHECK("surface_columns");
    } else {
        sf_column_kernel<true, false><<<grid2, dim3(SF_THREADS), 0, S_>>>(g, h, w, sx, sy, rth, cbw, f, nullptr, p.vox, fg, nullptr);
        CTL_LAUNCH_CHECK("surface_columns");
        const int64_t plane = (int64_t)h * w;
        const int cb3 = (int)ctl_cdiv64(plane, SF_COLS), rt3 = ctl_cdiv(d, SF_ROWS);
        if (qp) {
            sf_column_kernel<false, true, true><<<dim3((unsigned)(p.masks * rt3 * cb3)), dim3(SF_THREADS), 0, S_>>>(f, d, plane, 1.0, s[0], rt3, cb3, nullptr,
                                                                                                                   code, p.vox, fg, partial, gpm, first,
                                                                                                                   cursor, keys);
            CTL_LAUNCH_CHECK("surface_slices_emit");
        } else {
            sf_column_kernel<false, true><<<dim3((unsigned)(p.masks * rt3 * cb3)), dim3(SF_THREADS), 0, S_>>>(f, d, plane, 1.0, s[0], rt3, cb3, nullptr, code,
                                                                                                             p.vox, fg, partial);
            CTL_LAUNCH_CHECK("surface_slices");
        }
    }
    if (table) {
        sf_finalize_kernel<<<dim3((unsigned)p.groups), dim3(SF_THREADS), 0, S_>>>(partial, (int)p.bpo, gpm, table);
        CTL_LAUNCH_CHECK("surface_finalize");
    }
    if (qp) {
        sf_q_select_kernel<<<dim3((unsigned)qp->groups), dim3(SF_THREADS), 0, S_>>>(keys, first, gn, qp->qf, qp->n_q, qp->q_table);
        CTL_LAUNCH_CHECK("surface_q_select");
    }
    return CTL_OK;
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
    return sf_run(pred, gt, d, h, w, n_class, fg, mode, connectivity, s, table, workspace, p, nullptr, stream);
}

static int sf_q_args(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode, int32_t connectivity, int32_t n_q) {
    int rc = sf_check_dims("surface_quantiles", d, h, w, mode, connectivity);
    if (rc) return rc;
    CTL_REQUIRE(n_class >= 2 && n_class <= 255, "surface_quantiles: n_class %d outside 2..255", n_class);
    CTL_REQUIRE(n_q >= 1 && n_q <= 4, "surface_quantiles: n_q %d outside 1..4", n_q);
    return CTL_OK;
}

static int sf_make_qplan(int32_t d, int32_t h, int32_t w, int64_t classes, int32_t mode, int32_t n_q, sf_plan* p, sf_qplan* qp) {
    int rc = sf_make_plan("surface_quantiles", d, h, w, classes, 2, mode, true, p);
    if (rc) return rc;
    CTL_REQUIRE(p->vox < (1ll << 31), "surface_quantiles: %lld voxels do not fit the 32-bit key counters", (long long)p->vox);
    qp->classes = classes;
    qp->gpm = mode == 2 ? d : 1;
    qp->groups = classes * qp->gpm;
    qp->n_q = n_q;
    size_t off = p->bytes;
    qp->off_cnt = off; off += ctl_align256((size_t)2 * d * classes * sizeof(unsigned));
    qp->off_gn = off; off += ctl_align256((size_t)qp->groups * 2 * sizeof(unsigned));
    qp->off_first = off; off += ctl_align256((size_t)qp->groups * sizeof(int64_t));
    qp->off_cursor = off; off += ctl_align256((size_t)qp->groups * sizeof(unsigned));
    qp->off_keys = off; off += ctl_align256((size_t)2 * p->vox * sizeof(unsigned long long));      // surfaces of one side are disjoint
    qp->bytes = off;
    return CTL_OK;
}

extern "C" size_t ctl_surface_quantiles_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t foreground_only, int32_t mode,
                                                 int32_t n_q) {
    sf_plan p;
    sf_qplan qp;
    if (sf_q_args(d, h, w, n_class, mode, 1, n_q) || sf_make_qplan(d, h, w, foreground_only ? 1 : n_class - 1, mode, n_q, &p, &qp)) return 0;
    return qp.bytes;
}

extern "C" int ctl_surface_quantiles(const uint8_t* pred, const int64_t* gt, int32_t d, int32_t h, int32_t w, int32_t n_class,
                                     int32_t foreground_only, int32_t mode, int32_t connectivity, const double* sampling, const double* q,
                                     int32_t n_q, double* stats_table, double* q_table, void* workspace, size_t workspace_bytes,
                                     ctl_stream stream) {
    int rc = sf_q_args(d, h, w, n_class, mode, connectivity, n_q);
    if (rc) return rc;
    CTL_REQUIRE(pred && gt && q && q_table && workspace, "surface_quantiles: null pointer");
    double s[3];
    if ((rc = sf_sampling("surface_quantiles", sampling, mode, s))) return rc;
    sf_plan p;
    sf_qplan qp;
    const int fg = foreground_only ? 1 : 0;
    if ((rc = sf_make_qplan(d, h, w, fg ? 1 : n_class - 1, mode, n_q, &p, &qp))) return rc;
    for (int j = 0; j < 4; ++j) {
        qp.qf.v[j] = 0.0;
        if (j >= n_q) continue;
        CTL_REQUIRE(isfinite(q[j]) && q[j] >= 0.0 && q[j] <= 100.0, "surface_quantiles: q[%d] = %g outside [0, 100]", j, q[j]);
        qp.qf.v[j] = q[j] / 100.0;
    }
    CTL_REQUIRE(workspace_bytes >= qp.bytes, "surface_quantiles: workspace of %zu bytes, %zu needed", workspace_bytes, qp.bytes);
    qp.q_table = q_table;
    return sf_run(pred, gt, d, h, w, n_class, fg, mode, connectivity, s, stats_table, workspace, p, &qp, stream);
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
    sf_code_kernel<<<dim3(ctl_blocks(p.vox, SF_THREADS, 8192)), dim3(SF_THREADS), 0, S_>>>(mask, nullptr, d, h, w, 2, 1, mode, connectivity, 1, code);
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
