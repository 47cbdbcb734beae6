// Adversarial input augmentation (adversarial.py; a project addition, no upstream counterpart): the multiplicative bias field generated from
// a coarse control grid by the uniform cubic B-spline, its adjoint, and the per-sample unit step.  Definitions: include/ctl_hip.h,
// "adversarial input augmentation".  Tensors are fp32, NHWC in memory; theta is [n][gh][gw] in log space, gh = (h - 1) / s + 4.
//
// Forward: ONE launch, one thread per pixel: the 16-term sum S and exp(S) in fp64, f rounded to fp32 once, x' = x f rounded once from fp64.
// Backward: TWO launches, separable, through a workspace of n gw h doubles.  Pass 1 (one block per image row) recomputes f per pixel --
// ONE exp per pixel; a block per control point over its 4s x 4s support would take it 16 times -- forms q = f sum_c g_c x_c in LDS as fp64,
// writes dx = g f, and leaves for every control column b the row's sum_x Bx(x, b) q(x).  Pass 2 (one wave per control point) sums
// By(y, a) times those over the rows of its support.  Both sums run in a fixed order (lanes stride the support, then the xor butterfly):
// no float atomics, nothing is read back, the same bits on every call, at every alignment and in a graph replay.
// Unit step: pass 1 leaves per (sample, chunk of ADV_CHUNK elements) an ordered fp64 sum of squares or the largest magnitude -- the
// chunks are fixed, so the result does not depend on the grid -- pass 2 combines a sample's chunks in order and writes scale g / norm.
#include <cmath>
#include "ctl_device.h"

#define AB 256               // threads per block
#define ADV_MAXC 16
#define ADV_MAX_EDGE 2048
#define ADV_CHUNK 16384      // elements per partial of the unit step
#define ADV_MAX_BLOCKS 4096

// uniform cubic B-spline basis at t in [0, 1): non-negative, sums to 1; w[3] is exactly 0 at t = 0
__device__ __forceinline__ void adv_basis(double t, double* w) {
#pragma clang fp contract(off)
    const double u = 1.0 - t, t2 = t * t, t3 = t2 * t;
    w[0] = u * u * u / 6.0;
    w[1] = (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0;
    w[2] = (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0;
    w[3] = t3 / 6.0;
}
__device__ __forceinline__ double adv_pick(const double* w, int k) { return k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : w[3])); }
// the weight of control index `a` at pixel coordinate p (a - p / s in 0..3)
__device__ __forceinline__ double adv_weight(int64_t p, int s, int a) {
    const int i = (int)(p / s);
    double w[4];
    adv_basis((double)(p - (int64_t)i * s) / (double)s, w);
    return adv_pick(w, a - i);
}

// S(y, x) of one sample: rows of four, then the four rows
__device__ __forceinline__ double adv_spline(const float* __restrict__ th, int gw, int s, int y, int x) {
#pragma clang fp contract(off)
    const int iy = y / s, ix = x / s;
    double wy[4], wx[4];
    adv_basis((double)(y - iy * s) / (double)s, wy);
    adv_basis((double)(x - ix * s) / (double)s, wx);
    const float* __restrict__ p = th + (int64_t)iy * gw + ix;
    double S = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float* __restrict__ r = p + (int64_t)a * gw;
        double ra = wx[0] * (double)r[0];
        ra += wx[1] * (double)r[1];
        ra += wx[2] * (double)r[2];
        ra += wx[3] * (double)r[3];
        S += wy[a] * ra;
    }
    return S;
}

// ------------------------------------------------------------------------------------------------ bias field, forward
__global__ __launch_bounds__(AB) void adv_bias_fwd_kernel(const float* __restrict__ x, const float* __restrict__ theta, int64_t npix, int h, int w,
                                                          int c, int s, int gh, int gw, float* __restrict__ y, float* __restrict__ f) {
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * AB;
    for (int64_t i = (int64_t)blockIdx.x * AB + threadIdx.x; i < npix; i += stride) {
        const int px = (int)(i % w);
        const int64_t r = i / w;
        const int py = (int)(r % h);
        const int64_t smp = r / h;
        const double fd = exp(adv_spline(theta + smp * gh * gw, gw, s, py, px));
        if (f) f[i] = (float)fd;
        for (int k = 0; k < c; ++k) y[i * c + k] = (float)((double)x[i * c + k] * fd);
    }
}

// ------------------------------------------------------------------------------------------------ bias field, backward
// grid (h, n): block (py, smp).  T[smp][b][py] = sum_x Bx(x, b) q(py, x); dx = g f when asked for.
__global__ __launch_bounds__(AB) void adv_bias_bwd_rows_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                               const float* __restrict__ theta, int h, int w, int c, int s, int gh, int gw,
                                                               double* __restrict__ T, float* __restrict__ dx) {
#pragma clang fp contract(off)
    __shared__ double q[ADV_MAX_EDGE];
    const int py = blockIdx.x;
    const int64_t smp = blockIdx.y;
    const float* __restrict__ th = theta + smp * gh * gw;
    const int64_t row = (smp * h + py) * w;
    for (int px = threadIdx.x; px < w; px += AB) {
        const double fd = exp(adv_spline(th, gw, s, py, px));
        const int64_t e = (row + px) * c;
        double acc = 0.0;
        for (int k = 0; k < c; ++k) {
            const double gv = (double)g[e + k];
            acc += gv * (double)x[e + k];
            if (dx) dx[e + k] = (float)(gv * fd);
        }
        q[px] = fd * acc;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = wave; b < gw; b += AB / 64) {
        const int64_t lo64 = (int64_t)(b - 3) * s, hi64 = (int64_t)(b + 1) * s;
        const int lo = lo64 < 0 ? 0 : (int)lo64, hi = hi64 > w ? w : (int)hi64;
        double a = 0.0;
        for (int px = lo + lane; px < hi; px += 64) a += adv_weight(px, s, b) * q[px];
        a = wave_sum_double(a);
        if (lane == 0) T[(smp * gw + b) * h + py] = a;
    }
}

// one wave per control point: dtheta[smp][a][b] = sum_y By(y, a) T[smp][b][y], rounded once
__global__ __launch_bounds__(AB) void adv_bias_bwd_cols_kernel(const double* __restrict__ T, int64_t nout, int h, int s, int gh, int gw,
                                                               float* __restrict__ dtheta) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t o = (int64_t)blockIdx.x * (AB / 64) + (threadIdx.x >> 6);
    if (o >= nout) return;                       // the same in every lane of a wave
    const int b = (int)(o % gw), a = (int)((o / gw) % gh);
    const int64_t smp = o / ((int64_t)gw * gh);
    const int64_t lo64 = (int64_t)(a - 3) * s, hi64 = (int64_t)(a + 1) * s;
    const int lo = lo64 < 0 ? 0 : (int)lo64, hi = hi64 > h ? h : (int)hi64;
    const double* __restrict__ col = T + (smp * gw + b) * h;
    double acc = 0.0;
    for (int py = lo + lane; py < hi; py += 64) acc += adv_weight(py, s, a) * col[py];
    acc = wave_sum_double(acc);
    if (lane == 0) dtheta[o] = (float)acc;
}

// ------------------------------------------------------------------------------------------------ unit step
// sum for 'l2' / 'rms'; for 'linf' the larger magnitude, and a NaN stays (fmax would drop it)
__device__ __forceinline__ double adv_comb(int norm, double a, double b) {
    if (norm == CTL_ADV_LINF) return (b > a || b != b) ? b : a;
    return a + b;
}
// over a block, valid on thread 0: lanes by the xor butterfly, then the waves in order
__device__ __forceinline__ double adv_block_comb(int norm, double v, double* sm) {
    for (int o = 32; o > 0; o >>= 1) v = adv_comb(norm, v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) for (int i = 0; i < AB / 64; ++i) r = adv_comb(norm, r, sm[i]);
    return r;
}

// grid (chunks, n): partial[smp][chunk]
__global__ __launch_bounds__(AB) void adv_norm_partial_kernel(const float* __restrict__ g, int64_t m, int norm, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double sm[AB / 64];
    const int64_t smp = blockIdx.y, lo = (int64_t)blockIdx.x * ADV_CHUNK;
    const int64_t hi = lo + ADV_CHUNK < m ? lo + ADV_CHUNK : m;
    const float* __restrict__ gs = g + smp * m;
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += AB) {
        const double v = (double)gs[i];
        acc = adv_comb(norm, acc, norm == CTL_ADV_LINF ? fabs(v) : v * v);
    }
    acc = adv_block_comb(norm, acc, sm);
    if (threadIdx.x == 0) partial[smp * gridDim.x + blockIdx.x] = acc;
}

// grid (blocks of a sample, n): every block combines the sample's chunks in the same order, then scales its elements
__global__ __launch_bounds__(AB) void adv_scale_kernel(const float* __restrict__ g, int64_t m, int norm, double scale, int chunks,
                                                       const double* __restrict__ partial, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sm[AB / 64];
    __shared__ double factor;
    const int64_t smp = blockIdx.y;
    double acc = 0.0;
    for (int i = threadIdx.x; i < chunks; i += AB) acc = adv_comb(norm, acc, partial[smp * chunks + i]);
    acc = adv_block_comb(norm, acc, sm);
    if (threadIdx.x == 0) {
        const double r = norm == CTL_ADV_LINF ? acc : (norm == CTL_ADV_RMS ? sqrt(acc / (double)m) : sqrt(acc));
        factor = (r > 0.0 && r <= 1.7976931348623157e308) ? scale / r : 0.0;       // a norm of 0, inf or NaN: zeros
    }
    __syncthreads();
    const double k = factor;
    const float* __restrict__ gs = g + smp * m;
    float* __restrict__ os = out + smp * m;
    const int64_t stride = (int64_t)gridDim.x * AB;
    for (int64_t i = (int64_t)blockIdx.x * AB + threadIdx.x; i < m; i += stride) os[i] = k != 0.0 ? (float)((double)gs[i] * k) : 0.f;
}

// ------------------------------------------------------------------------------------------------ launchers
static int adv_check(const char* who, int64_t n, int64_t h, int64_t w, int c, int64_t s, int64_t gh, int64_t gw, bool grid) {
    CTL_REQUIRE(n >= 1 && n <= 65535, "%s: n = %lld samples (1 .. 65535)", who, (long long)n);
    CTL_REQUIRE(h >= 1 && w >= 1 && h <= ADV_MAX_EDGE && w <= ADV_MAX_EDGE, "%s: plane %lld x %lld (1 .. %d on each edge)", who, (long long)h,
                (long long)w, ADV_MAX_EDGE);
    CTL_REQUIRE(c >= 1 && c <= ADV_MAXC, "%s: c = %d channels (1 .. %d)", who, c, ADV_MAXC);
    CTL_REQUIRE(s >= 2, "%s: spacing s = %lld (at least 2)", who, (long long)s);
    if (grid) CTL_REQUIRE(gh == (h - 1) / s + 4 && gw == (w - 1) / s + 4, "%s: grid %lld x %lld (a %lld x %lld plane at spacing %lld has %lld x %lld)",
                          who, (long long)gh, (long long)gw, (long long)h, (long long)w, (long long)s, (long long)((h - 1) / s + 4),
                          (long long)((w - 1) / s + 4));
    CTL_REQUIRE(n * h * w < ((int64_t)1 << 31) / c, "%s: %lld x %lld x %lld pixels of %d channels reach the limit of 2^31 elements", who,
                (long long)n, (long long)h, (long long)w, c);
    return CTL_OK;
}

extern "C" size_t ctl_adv_bias_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t s) {
    if (adv_check("adv_bias_ws_bytes", n, h, w, 1, s, 0, 0, false) != CTL_OK) return 0;
    return sizeof(double) * (size_t)n * (size_t)((w - 1) / s + 4) * (size_t)h;
}

extern "C" int ctl_adv_bias_fwd(const float* x, const float* theta, int32_t n, int32_t h, int32_t w, int32_t c, int32_t s, int32_t gh, int32_t gw,
                                float* y, float* f, ctl_stream stream) {
    CTL_REQUIRE(x && theta && y, "adv_bias_fwd: null pointer");
    if (int rc = adv_check("adv_bias_fwd", n, h, w, c, s, gh, gw, true)) return rc;
    const int64_t npix = (int64_t)n * h * w;
    const size_t xb = sizeof(float) * (size_t)npix * c;
    CTL_REQUIRE(!ctl_overlap(y, xb, x, xb), "adv_bias_fwd: the output overlaps x (in place is not supported)");
    CTL_REQUIRE(!ctl_overlap(f, sizeof(float) * (size_t)npix, x, xb) && !ctl_overlap(f, sizeof(float) * (size_t)npix, y, xb),
                "adv_bias_fwd: the field overlaps x or the output");
    adv_bias_fwd_kernel<<<dim3(ctl_blocks(npix, AB, ADV_MAX_BLOCKS)), dim3(AB), 0, S_>>>(x, theta, npix, h, w, c, s, gh, gw, y, f);
    CTL_LAUNCH_CHECK("adv_bias_fwd");
    return CTL_OK;
}

extern "C" int ctl_adv_bias_bwd(const float* g, const float* x, const float* theta, int32_t n, int32_t h, int32_t w, int32_t c, int32_t s,
                                int32_t gh, int32_t gw, void* ws, size_t ws_bytes, float* dtheta, float* dx, ctl_stream stream) {
    CTL_REQUIRE(g && x && theta && ws && dtheta, "adv_bias_bwd: null pointer");
    if (int rc = adv_check("adv_bias_bwd", n, h, w, c, s, gh, gw, true)) return rc;
    CTL_REQUIRE(((uintptr_t)ws & 7) == 0, "adv_bias_bwd: the workspace must be 8-byte aligned");
    const size_t need = ctl_adv_bias_ws_bytes(n, h, w, s);
    CTL_REQUIRE(ws_bytes >= need, "adv_bias_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const size_t xb = sizeof(float) * (size_t)n * h * w * c;
    CTL_REQUIRE(!ctl_overlap(dx, xb, g, xb) && !ctl_overlap(dx, xb, x, xb), "adv_bias_bwd: dx overlaps g or x (in place is not supported)");
    double* T = (double*)ws;
    const int64_t nout = (int64_t)n * gh * gw;
    adv_bias_bwd_rows_kernel<<<dim3(h, n), dim3(AB), 0, S_>>>(g, x, theta, h, w, c, s, gh, gw, T, dx);
    adv_bias_bwd_cols_kernel<<<dim3((unsigned)ctl_cdiv64(nout, AB / 64)), dim3(AB), 0, S_>>>(T, nout, h, s, gh, gw, dtheta);
    ctl_count_launches(1);
    CTL_LAUNCH_CHECK("adv_bias_bwd");
    return CTL_OK;
}

static int adv_unit_check(const char* who, int64_t n, int64_t m) {
    CTL_REQUIRE(n >= 1 && n <= 65535, "%s: n = %lld samples (1 .. 65535)", who, (long long)n);
    CTL_REQUIRE(m >= 1 && m <= (int64_t)ADV_MAXC * ADV_MAX_EDGE * ADV_MAX_EDGE, "%s: m = %lld elements per sample (1 .. %d x %d x %d)", who,
                (long long)m, ADV_MAXC, ADV_MAX_EDGE, ADV_MAX_EDGE);
    return CTL_OK;
}

extern "C" size_t ctl_adv_unit_scale_ws_bytes(int32_t n, int64_t m) {
    if (adv_unit_check("adv_unit_scale_ws_bytes", n, m) != CTL_OK) return 0;
    return sizeof(double) * (size_t)n * (size_t)ctl_cdiv64(m, ADV_CHUNK);
}

extern "C" int ctl_adv_unit_scale(const float* g, int32_t n, int64_t m, int32_t norm, double scale, void* ws, size_t ws_bytes, float* out,
                                  ctl_stream stream) {
    CTL_REQUIRE(g && ws && out, "adv_unit_scale: null pointer");
    if (int rc = adv_unit_check("adv_unit_scale", n, m)) return rc;
    CTL_REQUIRE(norm == CTL_ADV_L2 || norm == CTL_ADV_RMS || norm == CTL_ADV_LINF, "adv_unit_scale: norm = %d (0 l2, 1 rms, 2 linf)", norm);
    CTL_REQUIRE(std::isfinite(scale), "adv_unit_scale: scale = %g (finite)", scale);
    CTL_REQUIRE(((uintptr_t)ws & 7) == 0, "adv_unit_scale: the workspace must be 8-byte aligned");
    const size_t need = ctl_adv_unit_scale_ws_bytes(n, m);
    CTL_REQUIRE(ws_bytes >= need, "adv_unit_scale: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const size_t gb = sizeof(float) * (size_t)n * (size_t)m;
    CTL_REQUIRE(!ctl_overlap(out, gb, g, gb), "adv_unit_scale: the output overlaps g (in place is not supported)");
    const int chunks = (int)ctl_cdiv64(m, ADV_CHUNK);
    adv_norm_partial_kernel<<<dim3(chunks, n), dim3(AB), 0, S_>>>(g, m, norm, (double*)ws);
    adv_scale_kernel<<<dim3(ctl_blocks(m, AB * 4, 1024), n), dim3(AB), 0, S_>>>(g, m, norm, scale, chunks, (const double*)ws, out);
    ctl_count_launches(1);
    CTL_LAUNCH_CHECK("adv_unit_scale");
    return CTL_OK;
}
