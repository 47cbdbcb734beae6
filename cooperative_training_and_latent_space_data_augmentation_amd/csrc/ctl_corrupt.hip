// MR artefact corruption of a test volume [D,H,W] on the device (the ACDC-C sets: TorchIO's RandomBiasField, RandomSpike, RandomGhosting
// and RandomMotion as medseg/dataset_loader/generate_artefacted_data.py:56-83 applies them).  None of them needs an FFT here:
//   ctl_corrupt_bias      x * exp(cubic polynomial of the normalised voxel coordinates), one element-wise launch
//   ctl_corrupt_spike     a k-space spike is a plane wave in image space: a fixed-order fp64 reduction for sum(x) and X[k], then one
//                         element-wise pass
//   ctl_corrupt_rigid3d   T rigid copies of the volume (trilinear gather, zero outside) in one launch
//   ctl_axis_operator     a spectrum mask along ONE axis is a real L x L matrix along that axis: out[r,j] = sum_k C[j,k] in(k)[r,k mod L]
//                         over up to 1 + CTL_CORRUPT_MAX_COPIES stacked volumes, fp32 FMA tiles through LDS, strided for the outer axes
// No floating-point atomics, every sum in a fixed order: identical bits on every call.  No readback, a launch sequence that depends on
// the shapes only.
#include "ctl_device.h"
#include <math.h>

#define CB 256
#define COR_TENSOR_BYTES (1ll << 31)
#define COR_EPB 2048                 // elements per block the spike reduction aims at
#define COR_NCOEF 20                 // monomials u^i v^j w^k with i + j + k <= 3
#define AX_T 32                      // the axis operator's tile: 32 rows x 32 outputs x 32 terms

static inline bool cor_shape_ok(int32_t d, int32_t h, int32_t w) {
    return d >= 1 && h >= 1 && w >= 1 && (int64_t)d * h * w * 4 < COR_TENSOR_BYTES;
}

// ------------------------------------------------------------------------------------------------ bias field
struct cor_coef { float c[COR_NCOEF]; };

// (t - h + 0.5) / (h - 0.5) with h = n / 2: the numerator and the denominator are exact, one rounding; 0 on an axis of one voxel
__device__ __forceinline__ float cor_coord(int t, int n) {
    const int h = n >> 1;
    return h == 0 ? 0.f : ((float)(t - h) + 0.5f) / ((float)h - 0.5f);
}

__global__ __launch_bounds__(CB) void cor_bias_kernel(const float* __restrict__ x, float* __restrict__ out, int d, int h, int w, cor_coef cf) {
    const int total = d * h * w;
    for (int i = blockIdx.x * CB + threadIdx.x; i < total; i += gridDim.x * CB) {
        const int tw = i % w, q = i / w, th = q % h, td = q / h;
        const float u = cor_coord(td, d), v = cor_coord(th, h), s = cor_coord(tw, w);
        const float pu[4] = {1.f, u, u * u, u * u * u}, pv[4] = {1.f, v, v * v, v * v * v}, pw[4] = {1.f, s, s * s, s * s * s};
        float p = 0.f;
        int idx = 0;
#pragma unroll
        for (int a = 0; a <= 3; ++a)
#pragma unroll
            for (int b = 0; b <= 3 - a; ++b)
#pragma unroll
                for (int c = 0; c <= 3 - a - b; ++c) p += cf.c[idx++] * ((pu[a] * pv[b]) * pw[c]);
        out[i] = x[i] * expf(p);
    }
}

extern "C" int ctl_corrupt_bias(const float* x, const float* coefficients, int32_t d, int32_t h, int32_t w, float* out, ctl_stream stream) {
    CTL_REQUIRE(x && coefficients && out, "corrupt_bias: null pointer (x, coefficients and out are required)");
    CTL_REQUIRE(d >= 1 && h >= 1 && w >= 1, "corrupt_bias: sizes must be positive (%d x %d x %d)", d, h, w);
    CTL_REQUIRE(cor_shape_ok(d, h, w), "corrupt_bias: %d x %d x %d floats reach the 2 GiB tensor limit (32-bit byte offsets)", d, h, w);
    const int64_t n = (int64_t)d * h * w;
    CTL_REQUIRE(!ctl_overlap(x, n * 4, out, n * 4), "corrupt_bias: out aliases x (a separate output array is required)");
    cor_coef cf;
    for (int i = 0; i < COR_NCOEF; ++i) {
        CTL_REQUIRE(isfinite(coefficients[i]), "corrupt_bias: coefficient %d is not finite", i);
        cf.c[i] = coefficients[i];
    }
    cor_bias_kernel<<<dim3(ctl_blocks(n, CB, 4096)), dim3(CB), 0, S_>>>(x, out, d, h, w, cf);
    CTL_LAUNCH_CHECK("corrupt_bias");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ spike
// A pair {k, -k} of spectrum entries set to A changes the image by (m / N) ((A - Re X[k]) cos th + Im X[k] sin th), th = 2 pi k.r / shape,
// m = 2 (1 when k == -k on every axis): X[-k] is the conjugate of X[k] for a real volume.
struct cor_spikes { int32_t n; int32_t k[CTL_CORRUPT_MAX_SPIKES][3]; int32_t mult[CTL_CORRUPT_MAX_SPIKES]; };
#define COR_NVAL (1 + 2 * CTL_CORRUPT_MAX_SPIKES)

static inline int cor_red_blocks(int64_t n) { return (int)ctl_blocks(n, COR_EPB, CTL_CORRUPT_RED_BLOCKS); }

// th / (2 pi) for voxel (td, th, tw): every (k_a t_a) mod n_a is exact in integers, the three fractions are added in fp64
__device__ __forceinline__ double cor_turns(const int32_t* k, int td, int th, int tw, int d, int h, int w) {
    const int m0 = (int)(((int64_t)k[0] * td) % d), m1 = (int)(((int64_t)k[1] * th) % h), m2 = (int)(((int64_t)k[2] * tw) % w);
    return (double)m0 / (double)d + (double)m1 / (double)h + (double)m2 / (double)w;
}

// partial[block][1 + 2 n]: sum x, then (sum x cos th, -sum x sin th) per spike.  Thread sums in index order, lanes by the xor
// butterfly, the four waves in order: a fixed tree.
__global__ __launch_bounds__(CB) void cor_spike_reduce_kernel(const float* __restrict__ x, int d, int h, int w, cor_spikes sp,
                                                               double* __restrict__ partial) {
    __shared__ double s_w[CB / 64][COR_NVAL];
    const int total = d * h * w, nval = 1 + 2 * sp.n;
    double acc[COR_NVAL];
#pragma unroll
    for (int i = 0; i < COR_NVAL; ++i) acc[i] = 0.0;
    for (int i = blockIdx.x * CB + threadIdx.x; i < total; i += gridDim.x * CB) {
        const int tw = i % w, q = i / w, th = q % h, td = q / h;
        const double v = (double)x[i];
        acc[0] += v;
#pragma unroll
        for (int s = 0; s < CTL_CORRUPT_MAX_SPIKES; ++s) {
            if (s < sp.n) {
                double sn, cs;
                sincospi(2.0 * cor_turns(sp.k[s], td, th, tw, d, h, w), &sn, &cs);
                acc[1 + 2 * s] += v * cs;
                acc[2 + 2 * s] -= v * sn;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < COR_NVAL; ++i) {
        const double r = wave_sum_double(acc[i]);
        if (lane == 0) s_w[wv][i] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < nval) {
        double r = 0.0;
        for (int k = 0; k < CB / 64; ++k) r += s_w[k][threadIdx.x];
        partial[(int64_t)blockIdx.x * nval + threadIdx.x] = r;
    }
}

__global__ __launch_bounds__(CB) void cor_spike_apply_kernel(const float* __restrict__ x, float* __restrict__ out, int d, int h, int w,
                                                              cor_spikes sp, double intensity, const double* __restrict__ partial, int nblk) {
    __shared__ double s_tab[COR_NVAL];
    const int total = d * h * w, nval = 1 + 2 * sp.n;
    if ((int)threadIdx.x < nval) {                              // every block re-derives the table from the partials, in block order
        double r = 0.0;
        for (int b = 0; b < nblk; ++b) r += partial[(int64_t)b * nval + threadIdx.x];
        s_tab[threadIdx.x] = r;
    }
    __syncthreads();
    const double amp = intensity * s_tab[0], inv_n = 1.0 / (double)total;
    for (int i = blockIdx.x * CB + threadIdx.x; i < total; i += gridDim.x * CB) {
        const int tw = i % w, q = i / w, th = q % h, td = q / h;
        double add = 0.0;
#pragma unroll
        for (int s = 0; s < CTL_CORRUPT_MAX_SPIKES; ++s) {
            if (s < sp.n) {
                double sn, cs;
                sincospi(2.0 * cor_turns(sp.k[s], td, th, tw, d, h, w), &sn, &cs);
                add += (double)sp.mult[s] * ((amp - s_tab[1 + 2 * s]) * cs + s_tab[2 + 2 * s] * sn);
            }
        }
        out[i] = (float)((double)x[i] + add * inv_n);
    }
}

extern "C" size_t ctl_corrupt_spike_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_spikes) {
    if (!cor_shape_ok(d, h, w) || n_spikes < 1 || n_spikes > CTL_CORRUPT_MAX_SPIKES) return 0;
    return (size_t)cor_red_blocks((int64_t)d * h * w) * (1 + 2 * (size_t)n_spikes) * sizeof(double);
}

extern "C" int ctl_corrupt_spike(const float* x, int32_t d, int32_t h, int32_t w, const int32_t* k, const int32_t* mult, int32_t n_spikes,
                                 double intensity, float* out, void* workspace, size_t workspace_bytes, ctl_stream stream) {
    CTL_REQUIRE(x && k && mult && out && workspace, "corrupt_spike: null pointer (x, k, mult, out and workspace are required)");
    CTL_REQUIRE(d >= 1 && h >= 1 && w >= 1, "corrupt_spike: sizes must be positive (%d x %d x %d)", d, h, w);
    CTL_REQUIRE(cor_shape_ok(d, h, w), "corrupt_spike: %d x %d x %d floats reach the 2 GiB tensor limit (32-bit byte offsets)", d, h, w);
    CTL_REQUIRE(n_spikes >= 1 && n_spikes <= CTL_CORRUPT_MAX_SPIKES, "corrupt_spike: n_spikes %d (1..%d wave-vector pairs per call)", n_spikes,
                CTL_CORRUPT_MAX_SPIKES);
    CTL_REQUIRE(isfinite(intensity), "corrupt_spike: intensity %g is not finite", intensity);
    const int64_t n = (int64_t)d * h * w;
    CTL_REQUIRE(!ctl_overlap(x, n * 4, out, n * 4), "corrupt_spike: out aliases x (a separate output array is required)");
    const int32_t size[3] = {d, h, w};
    cor_spikes sp = {};
    sp.n = n_spikes;
    for (int s = 0; s < n_spikes; ++s) {
        bool self = true;
        for (int a = 0; a < 3; ++a) {
            const int32_t v = k[3 * s + a];
            CTL_REQUIRE(v >= 0 && v < size[a], "corrupt_spike: wave number %d (spike %d, axis %d) outside [0, %d)", v, s, a, size[a]);
            sp.k[s][a] = v;
            self = self && (2 * (int64_t)v) % size[a] == 0;
        }
        CTL_REQUIRE(mult[s] == (self ? 1 : 2), "corrupt_spike: multiplicity %d of spike %d (1 where k == -k on every axis, else 2: here %d)",
                    mult[s], s, self ? 1 : 2);
        sp.mult[s] = mult[s];
    }
    const size_t need = ctl_corrupt_spike_ws_bytes(d, h, w, n_spikes);
    CTL_REQUIRE(workspace_bytes >= need, "corrupt_spike: workspace of %zu bytes, %zu needed (ctl_corrupt_spike_ws_bytes)", workspace_bytes, need);
    CTL_REQUIRE(((uintptr_t)workspace & 7) == 0, "corrupt_spike: the workspace must be 8-byte aligned");
    const int nblk = cor_red_blocks(n);
    cor_spike_reduce_kernel<<<dim3((unsigned)nblk), dim3(CB), 0, S_>>>(x, d, h, w, sp, (double*)workspace);
    cor_spike_apply_kernel<<<dim3(ctl_blocks(n, CB, 4096)), dim3(CB), 0, S_>>>(x, out, d, h, w, sp, intensity, (const double*)workspace, nblk);
    ctl_count_launches(1);                                     // two kernels, CTL_LAUNCH_CHECK counts one
    CTL_LAUNCH_CHECK("corrupt_spike");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ rigid copies
struct cor_rigid { float m[CTL_CORRUPT_MAX_COPIES][12]; };

__device__ __forceinline__ float cor_fetch(const float* __restrict__ x, int z, int y, int xx, int d, int h, int w) {
    return (z >= 0 && z < d && y >= 0 && y < h && xx >= 0 && xx < w) ? x[((int64_t)z * h + y) * w + xx] : 0.f;
}

// out[t][p] = the volume, extended by zeros, interpolated linearly at M_t p + o_t (fp32 coordinates: three fused multiply-adds per axis)
__global__ __launch_bounds__(CB) void cor_rigid_kernel(const float* __restrict__ x, float* __restrict__ out, int d, int h, int w, int copies,
                                                        cor_rigid rg) {
    const int n = d * h * w;
    const int64_t total = (int64_t)n * copies;
    for (int64_t g = (int64_t)blockIdx.x * CB + threadIdx.x; g < total; g += (int64_t)gridDim.x * CB) {
        const int t = (int)(g / n), i = (int)(g % n);
        const int tw = i % w, q = i / w, th = q % h, td = q / h;
        const float* m = rg.m[t];
        const float fd = (float)td, fh = (float)th, fw = (float)tw;
        const float sz = fmaf(m[2], fw, fmaf(m[1], fh, fmaf(m[0], fd, m[3])));
        const float sy = fmaf(m[6], fw, fmaf(m[5], fh, fmaf(m[4], fd, m[7])));
        const float sx = fmaf(m[10], fw, fmaf(m[9], fh, fmaf(m[8], fd, m[11])));
        float v = 0.f;
        if (sz > -1.f && sz < (float)d && sy > -1.f && sy < (float)h && sx > -1.f && sx < (float)w) {      // false for a NaN too
            const float z0f = floorf(sz), y0f = floorf(sy), x0f = floorf(sx);
            const float fz = sz - z0f, fy = sy - y0f, fx = sx - x0f;
            const int z0 = (int)z0f, y0 = (int)y0f, x0 = (int)x0f;
            float c[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float v0 = cor_fetch(x, z0 + a, y0 + b, x0, d, h, w), v1 = cor_fetch(x, z0 + a, y0 + b, x0 + 1, d, h, w);
                    c[a][b] = v0 + fx * (v1 - v0);
                }
            const float e0 = c[0][0] + fy * (c[0][1] - c[0][0]), e1 = c[1][0] + fy * (c[1][1] - c[1][0]);
            v = e0 + fz * (e1 - e0);
        }
        out[g] = v;
    }
}

extern "C" int ctl_corrupt_rigid3d(const float* x, int32_t d, int32_t h, int32_t w, const float* matrices, int32_t copies, float* out,
                                   ctl_stream stream) {
    CTL_REQUIRE(x && matrices && out, "corrupt_rigid3d: null pointer (x, matrices and out are required)");
    CTL_REQUIRE(d >= 1 && h >= 1 && w >= 1, "corrupt_rigid3d: sizes must be positive (%d x %d x %d)", d, h, w);
    CTL_REQUIRE(copies >= 1 && copies <= CTL_CORRUPT_MAX_COPIES, "corrupt_rigid3d: copies %d (1..%d per call)", copies, CTL_CORRUPT_MAX_COPIES);
    CTL_REQUIRE(cor_shape_ok(d, h, w) && (int64_t)d * h * w * copies * 4 < COR_TENSOR_BYTES,
                "corrupt_rigid3d: %d copies of %d x %d x %d floats reach the 2 GiB tensor limit (32-bit byte offsets)", copies, d, h, w);
    const int64_t n = (int64_t)d * h * w;
    CTL_REQUIRE(!ctl_overlap(x, n * 4, out, n * copies * 4), "corrupt_rigid3d: out aliases x (a separate output array is required)");
    cor_rigid rg = {};
    for (int i = 0; i < copies * 12; ++i) {
        CTL_REQUIRE(isfinite(matrices[i]), "corrupt_rigid3d: matrix entry %d of copy %d is not finite", i % 12, i / 12);
        rg.m[i / 12][i % 12] = matrices[i];
    }
    cor_rigid_kernel<<<dim3(ctl_blocks(n * copies, CB, 4096)), dim3(CB), 0, S_>>>(x, out, d, h, w, copies, rg);
    CTL_LAUNCH_CHECK("corrupt_rigid3d");
    return CTL_OK;
}

// ------------------------------------------------------------------------------------------------ operator along one axis
// A volume [D,H,W] seen from axis a of length L is `rows` = N / L rows of L elements: element k of row r lives at
// (r / inner) * L * inner + k * inner + r % inner, inner = the product of the sizes after the axis (1 for the last axis).
// Block = 32 rows x 32 outputs, terms in chunks of 32 through LDS; a thread owns 4 outputs and adds their terms in ascending order of
// (volume, k), one fused multiply-add each.  The 32 lanes of a half wave run along the axis that is contiguous in memory: the outputs j
// for the last axis (INNER1), the rows otherwise, so loads and stores of both forms are coalesced and nothing is transposed in HBM.
// LDS rows are 33 words: the lanes of a half wave read sC[lane][kk] / sA[lane][kk] on 32 different banks (ds_read_b32: bank = word % 32
// per 32-lane group), the other operand is one address (a broadcast); the transposed store sA[lane][a] of the outer axes is conflict
// free for the same reason.
template <bool INNER1>
__global__ __launch_bounds__(CB) void cor_axis_kernel(const float* __restrict__ x0, const float* __restrict__ xs, const float* __restrict__ cm,
                                                       float* __restrict__ out, int rows, int len, int inner, int nvol, int vol_elems) {
    __shared__ float sA[AX_T][AX_T + 1], sC[AX_T][AX_T + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.x * AX_T, j0 = blockIdx.y * AX_T;
    const int64_t kk_total = (int64_t)nvol * len;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < nvol; ++v) {
        const float* __restrict__ src = v == 0 ? x0 : xs + (int64_t)(v - 1) * vol_elems;
        for (int k0 = 0; k0 < len; k0 += AX_T) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int a = ty + 8 * e;
                const int rl = INNER1 ? a : tx, kl = INNER1 ? tx : a;
                const int r = r0 + rl, k = k0 + kl;
                float val = 0.f;
                if (r < rows && k < len)
                    val = INNER1 ? src[(int64_t)r * len + k] : src[((int64_t)(r / inner) * len + k) * inner + r % inner];
                sA[rl][kl] = val;
                const int j = j0 + a, kc = k0 + tx;
                sC[a][tx] = (j < len && kc < len) ? cm[(int64_t)j * kk_total + (int64_t)v * len + kc] : 0.f;
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < AX_T; ++kk) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int a = ty + 8 * e;
                    acc[e] = INNER1 ? fmaf(sC[tx][kk], sA[a][kk], acc[e]) : fmaf(sC[a][kk], sA[tx][kk], acc[e]);
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int a = ty + 8 * e;
        const int r = r0 + (INNER1 ? a : tx), j = j0 + (INNER1 ? tx : a);
        if (r < rows && j < len) {
            if (INNER1) out[(int64_t)r * len + j] = acc[e];
            else out[((int64_t)(r / inner) * len + j) * inner + r % inner] = acc[e];
        }
    }
}

extern "C" int ctl_axis_operator(const float* x0, const float* xs, int32_t n_volumes, int32_t d, int32_t h, int32_t w, int32_t axis,
                                 const float* matrix, float* out, ctl_stream stream) {
    CTL_REQUIRE(x0 && matrix && out, "axis_operator: null pointer (x0, matrix and out are required)");
    CTL_REQUIRE(d >= 1 && h >= 1 && w >= 1, "axis_operator: sizes must be positive (%d x %d x %d)", d, h, w);
    CTL_REQUIRE(axis >= 0 && axis <= 2, "axis_operator: axis %d (0, 1 or 2)", axis);
    CTL_REQUIRE(n_volumes >= 1 && n_volumes <= 1 + CTL_CORRUPT_MAX_COPIES, "axis_operator: n_volumes %d (1..%d stacked volumes)", n_volumes,
                1 + CTL_CORRUPT_MAX_COPIES);
    CTL_REQUIRE(n_volumes == 1 || xs, "axis_operator: null pointer (%d volumes need the stack xs of the volumes after the first)", n_volumes);
    const int64_t n = (int64_t)d * h * w;
    const int32_t size[3] = {d, h, w};
    const int64_t len = size[axis];
    CTL_REQUIRE(cor_shape_ok(d, h, w) && n * (n_volumes - 1) * 4 < COR_TENSOR_BYTES && len * len * n_volumes * 4 < COR_TENSOR_BYTES,
                "axis_operator: %d volumes of %d x %d x %d floats, or the %lld x %lld matrix, reach the 2 GiB tensor limit (32-bit byte offsets)",
                n_volumes, d, h, w, (long long)len, (long long)(len * n_volumes));
    CTL_REQUIRE(!ctl_overlap(x0, n * 4, out, n * 4) && !ctl_overlap(n_volumes > 1 ? xs : nullptr, n * (n_volumes - 1) * 4, out, n * 4),
                "axis_operator: out aliases an input volume (a separate output array is required)");
    const int inner = axis == 0 ? h * w : (axis == 1 ? w : 1);
    const int rows = (int)(n / len);
    const dim3 grid((unsigned)ctl_cdiv(rows, AX_T), (unsigned)ctl_cdiv((int)len, AX_T)), blk(CB);
    CTL_REQUIRE(grid.y <= 65535, "axis_operator: an axis of %lld elements is too long (at most %d)", (long long)len, 65535 * AX_T);
    if (inner == 1) cor_axis_kernel<true><<<grid, blk, 0, S_>>>(x0, xs, matrix, out, rows, (int)len, 1, n_volumes, (int)n);
    else cor_axis_kernel<false><<<grid, blk, 0, S_>>>(x0, xs, matrix, out, rows, (int)len, inner, n_volumes, (int)n);
    CTL_LAUNCH_CHECK("axis_operator");
    return CTL_OK;
}
